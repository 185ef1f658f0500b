"""GPU: ZK_OP_SHA256 of zk_field_vec_op -- SHA-256 digests, output_rlc and input_rlc of messages that live in device memory -- bit
for bit against the model of tests/sha256_cases.py (hashlib.sha256 and Python integers), converted by the oracle (cref.to_mont).
333 messages of every length at which loading or padding can go wrong, laid with gaps into a buffer at an odd address, under both
index widths and every combination of the optional outputs; overlapping and repeated messages, bytes of 0xff, challenges 0, 1 and
p-1, one 16 KiB message among 63 empty ones; out-of-range rows between valid ones; every refusal; the booking."""
import ctypes
import os
import random
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import sha256_cases as sc  # noqa: E402
from oracle import cref  # noqa: E402

pytestmark = pytest.mark.gpu
P = sc.P
SENTINEL = 0xA5C3A5C3A5C3A5C3
GUARD = 3                                   # sentinel cells in front of and behind every output
INVALID_ARG = -1
OUTPUTS = ("out", "digest", "input_rlc")


def mont(vals):
    return cref.to_mont(list(vals)) if len(vals) else np.zeros((0, 4), dtype=np.uint64)


class Call:
    """one call: the bytes at an ODD device address, offsets and lengths of index_width bytes, and out / digest / input_rlc of n
    rows each inside GUARD sentinel cells.  rows: (offset, length) pairs; a pair that does not lie inside the bytes is expected to
    give zeros.  The model's columns are computed once per Call and shared by every check made on it."""

    def __init__(self, ctx, data, rows, index_width=4, r_out=7, r_in=11, digest=True, input_rlc=True, n=None):
        self.ctx, self.data, self.rows, self.iw, self.r_out, self.r_in = ctx, bytes(data), list(rows), index_width, r_out, r_in
        self.n = len(self.rows) if n is None else n
        self.image = np.concatenate([np.full(1, 0xEE, dtype=np.uint8), np.frombuffer(self.data, dtype=np.uint8)])
        self.src = ctx.to_device(self.image)
        dt = np.uint32 if index_width == 4 else np.uint64
        self.h_offs = np.array([o for o, _ in self.rows] or [0], dtype=dt)
        self.h_lens = np.array([ln for _, ln in self.rows] or [0], dtype=dt)
        self.offs, self.lens = ctx.to_device(self.h_offs), ctx.to_device(self.h_lens)
        on = {"out": True, "digest": digest, "input_rlc": input_rlc}
        self.bufs = {name: ctx.to_device(np.full((len(self.rows) + 2 * GUARD, 4), SENTINEL, dtype=np.uint64)) for name in OUTPUTS if on[name]}
        self.wanted = None

    def out_ptr(self, name="out"):
        return self.bufs[name].ptr + GUARD * 32 if name in self.bufs else None

    def args(self):
        return dict(data=self.src.ptr + 1, total_bytes=len(self.data), offsets=self.offs.ptr, lens=self.lens.ptr, index_width=self.iw, n=self.n, out=self.out_ptr(),
                    r_out=mont([self.r_out])[0], r_in=mont([self.r_in])[0], digest=self.out_ptr("digest"), input_rlc=self.out_ptr("input_rlc"))

    def in_range(self, i):
        off, ln = self.rows[i]
        return off <= len(self.data) and ln <= len(self.data) - off

    def want(self):
        """{name: (rows, 4) uint64 as the device writes them}"""
        if self.wanted is None:
            good = [i for i in range(len(self.rows)) if self.in_range(i)]
            digests, out, inp = sc.expected([self.data[self.rows[i][0]:self.rows[i][0] + self.rows[i][1]] for i in good], self.r_out, self.r_in)
            w = {name: np.zeros((len(self.rows), 4), dtype=np.uint64) for name in OUTPUTS}
            if good:
                w["out"][good] = mont(out)
                w["input_rlc"][good] = mont(inp)
                w["digest"][good] = np.frombuffer(b"".join(digests), dtype=np.uint64).reshape(-1, 4)
            self.wanted = w
        return self.wanted

    def result(self, name):
        """the n rows of an output, after checking that nothing around them was written"""
        got = self.bufs[name].download((len(self.rows) + 2 * GUARD, 4))
        assert (got[:GUARD] == SENTINEL).all() and (got[GUARD + self.n:] == SENTINEL).all(), f"{name}: a row outside [0, n) was written"
        return got[GUARD:GUARD + self.n]

    def check(self):
        self.ctx.sha256(**self.args())
        want = self.want()
        for name in self.bufs:
            got = self.result(name)
            bad = [i for i in range(self.n) if not np.array_equal(got[i], want[name][i])][:5]
            assert not bad, (name, "first differing rows", bad, [self.rows[i] for i in bad])
        for name in ("out", "input_rlc"):
            if name in self.bufs:                                       # canonical: the stored integer is below the modulus
                assert all(sum(int(x) << (64 * j) for j, x in enumerate(row)) < P for row in self.result(name)), name
        assert self.inputs_intact(), "an input was written"

    def inputs_intact(self):
        return (np.array_equal(self.src.download(self.image.shape, np.uint8), self.image) and np.array_equal(self.offs.download(self.h_offs.shape, self.h_offs.dtype), self.h_offs)
                and np.array_equal(self.lens.download(self.h_lens.shape, self.h_lens.dtype), self.h_lens))

    def reset(self):
        for buf in self.bufs.values():
            buf.upload(np.full((len(self.rows) + 2 * GUARD, 4), SENTINEL, dtype=np.uint64))

    def untouched(self):
        return all((buf.download((len(self.rows) + 2 * GUARD, 4)) == SENTINEL).all() for buf in self.bufs.values()) and self.inputs_intact()

    def free(self):
        for buf in (self.src, self.offs, self.lens, *self.bufs.values()):
            buf.free()


def lay_out(rng, lengths, fill=None):
    """the messages one behind the other with gaps of 0 .. 9 bytes: (bytes, [(offset, length)])"""
    data, rows = bytearray(), []
    for n in lengths:
        data += bytes(rng.randrange(256) for _ in range(rng.randrange(10)))
        rows.append((len(data), n))
        data += bytes([fill] * n) if fill is not None else bytes(rng.randrange(256) for _ in range(n))
    return bytes(data), rows


# ---- 1. the main case: 333 messages, more than one workgroup and no multiple of 64
@pytest.fixture(scope="module")
def main_case():
    rng = random.Random(0x333)
    lengths = list(sc.LENGTHS) * 10 + [rng.randrange(600) for _ in range(13)]
    rng.shuffle(lengths)
    assert len(lengths) == 333
    data, rows = lay_out(rng, lengths)
    r_out, r_in = rng.randrange(P), rng.randrange(P)
    digests, out, inp = sc.expected([data[o:o + n] for o, n in rows], r_out, r_in)
    want = {"out": mont(out), "input_rlc": mont(inp), "digest": np.frombuffer(b"".join(digests), dtype=np.uint64).reshape(-1, 4)}
    return data, rows, r_out, r_in, want


@pytest.mark.parametrize("outputs", ["none", "digest", "input_rlc", "both"])
@pytest.mark.parametrize("index_width", [4, 8])
def test_main_case(ctx, main_case, index_width, outputs):
    data, rows, r_out, r_in, want = main_case
    call = Call(ctx, data, rows, index_width, r_out, r_in, digest=outputs in ("digest", "both"), input_rlc=outputs in ("input_rlc", "both"))
    call.wanted = want                                                  # computed once, shared, never changed
    try:
        assert {n for _, n in rows} >= set(sc.LENGTHS) and (call.src.ptr + 1) % 2 == 1
        assert {(o - rows[i - 1][0] - rows[i - 1][1]) for i, (o, _) in enumerate(rows) if i} <= set(range(10))
        call.check()
    finally:
        call.free()


# ---- 2. input variations
def test_overlapping_and_repeated_messages(ctx):
    rng = random.Random(2)
    data = bytes(rng.randrange(256) for _ in range(700))
    rows = [(0, 700), (1, 699), (1, 699), (0, 64), (32, 64), (64, 64), (63, 65), (699, 1), (700, 0), (0, 0), (3, 128), (3, 128), (3, 127), (5, 119), (5, 120), (645, 55), (644, 56)] * 5
    call = Call(ctx, data, rows, 8, rng.randrange(P), rng.randrange(P))
    try:
        call.check()
        got = call.result("digest")
        assert np.array_equal(got[1], got[2]) and not np.array_equal(got[0], got[1])
    finally:
        call.free()


def test_bytes_of_0xff(ctx):
    rng = random.Random(3)
    data, rows = lay_out(rng, sc.LENGTHS, fill=0xFF)
    call = Call(ctx, data, rows, 4, P - 1, P - 1)
    try:
        call.check()
    finally:
        call.free()


@pytest.mark.parametrize("r_out,r_in", [(0, 0), (1, 1), (P - 1, P - 1), (0, P - 1), (1, 0)])
def test_edge_challenges(ctx, r_out, r_in):
    rng = random.Random(4)
    data, rows = lay_out(rng, [0, 1, 8, 9, 31, 55, 56, 63, 64, 65, 300] * 6)
    call = Call(ctx, data, rows, 4, r_out, r_in)
    try:
        call.check()
        want = call.want()
        if r_in == 0:                                                   # only the last byte is left
            assert [int(v) for v in cref.from_mont(want["input_rlc"][:3])] == [0, data[rows[1][0]], data[rows[2][0] + 7]]
        if r_out == 0:                                                  # only the last digest byte is left
            assert int(cref.from_mont(want["out"][:1])[0]) == sc.empty_digest()[31]
    finally:
        call.free()


def test_one_long_message_among_empty_ones_in_a_wave(ctx):
    rng = random.Random(5)
    long_ = bytes(rng.randrange(256) for _ in range(16 * 1024))
    rows = [(len(long_), 0)] * 64
    rows[37] = (0, len(long_))
    call = Call(ctx, long_, rows, 4, rng.randrange(P), rng.randrange(P))
    try:
        call.check()
        assert call.result("digest")[0].tobytes() == sc.empty_digest()
    finally:
        call.free()


# ---- 3. out-of-range rows
@pytest.mark.parametrize("index_width", [4, 8])
def test_out_of_range_rows_write_zeros_between_valid_rows(ctx, index_width):
    rng = random.Random(6)
    data = bytes(rng.randrange(256) for _ in range(500))
    top = (1 << (8 * index_width)) - 1
    bad = [(501, 0), (400, 101), (top, 2)]
    rows = []
    for i in range(70):
        rows.append((rng.randrange(300), rng.randrange(200)))
        if i % 9 == 4:
            rows.append(bad[(i // 9) % 3])
    rows += [(500, 0), (0, 500), (0, 501), (top, top), (0, 1 << (8 * index_width - 1)), (top, 0), (0, top)]
    call = Call(ctx, data, rows, index_width, rng.randrange(P), rng.randrange(P), n=len(rows) - 2)      # rows >= n keep the sentinel
    try:
        assert sum(not call.in_range(i) for i in range(call.n)) >= 10
        call.check()
        for name in OUTPUTS:
            got = call.result(name)
            for i in range(call.n):
                assert call.in_range(i) or not got[i].any(), (name, i)
    finally:
        call.free()


# ---- 4. refusals
def raw_call(zk, ctx, c, n=None, field=0, op=18, flags=0, **over):
    a = c.args()
    a.update(over)
    desc = zk.binding._Sha256(a["data"], a["total_bytes"], a["offsets"], a["lens"], a["digest"], a["input_rlc"], a["index_width"], flags)
    hk = np.ascontiguousarray(np.stack([a["r_out"], a["r_in"]]))
    return zk.lib().zk_field_vec_op(ctx.h, ctypes.c_int(field), ctypes.c_int(op), ctypes.byref(desc), hk.ctypes.data_as(ctypes.c_void_p), ctypes.c_void_p(a["out"]),
                                    ctypes.c_size_t(c.n if n is None else n))


def test_refused_calls_write_nothing_and_leave_the_context_usable(zk, ctx):
    """EACH refusal is followed by its own checks: the guarded outputs and the inputs are untouched, and the next valid call works"""
    rng = random.Random(8)
    data, rows = lay_out(rng, [rng.randrange(150) for _ in range(64)])
    t = Call(ctx, data, rows, 8, rng.randrange(P), rng.randrange(P))
    refusals = []
    out, dg, ir = t.out_ptr(), t.out_ptr("digest"), t.out_ptr("input_rlc")
    a = t.args()
    n = t.n

    def refused(what, **kw):
        assert raw_call(zk, ctx, t, **kw) == INVALID_ARG, what
        ctx.sync()
        assert t.untouched(), what
        t.check()                                                       # the next valid call
        t.reset()
        refusals.append(what)
    try:
        refused("Fq", field=zk.FIELD_FQ)
        for wrong in (0, 1, 2, 3, 5, 16, 255):
            refused(f"index_width {wrong}", index_width=wrong)
        refused("NULL d_offsets", offsets=None)
        refused("NULL d_lens", lens=None)
        refused("8-byte offsets at an address that is 4 mod 8", offsets=a["offsets"] + 4)
        refused("8-byte lengths at an address that is 4 mod 8", lens=a["lens"] + 4)
        refused("4-byte offsets at an address that is 2 mod 4", offsets=a["offsets"] + 2, index_width=4)
        refused("4-byte lengths at an odd address", lens=a["lens"] + 1, index_width=4)
        refused("NULL d_bytes with total_bytes > 0", data=None)
        for bits in (1, 2, 128, 255):
            refused(f"flags {bits}", flags=bits)
        refused("NULL d_out", out=None)
        refused("d_out at an address that is 8 mod 16", out=out + 8)
        refused("d_input_rlc at an address that is 8 mod 16", input_rlc=ir + 8)
        refused("d_bytes inside d_out", data=out + 8)
        refused("d_bytes ends inside d_digest", data=dg - len(data) + 1)
        refused("d_offsets AT d_digest", offsets=dg)
        refused("d_lens inside d_input_rlc", lens=ir + 8)
        refused("d_offsets one entry in front of d_out's last byte", offsets=out + 32 * n - 8)
        refused("d_digest AT d_out", digest=out)
        refused("d_digest one byte into d_out", digest=out + 1)
        refused("d_input_rlc one row into d_digest", input_rlc=dg + 32)
        refused("d_input_rlc AT d_out", input_rlc=out)
        refused("d_out inside d_bytes", out=(a["data"] + 15) // 16 * 16)
        refused("d_digest AT d_lens", digest=a["lens"])
        refused("more rows than one launch grid takes", n=0x7FFFFFFF * 256 + 1)
        refused("2^64 - 1 rows", n=(1 << 64) - 1)
        refused("total_bytes = 2^61", total_bytes=1 << 61)
        refused("total_bytes = 2^64 - 1", total_bytes=(1 << 64) - 1)
        refused("total_bytes = 2^61 with n = 0, where nothing could overlap", total_bytes=1 << 61, n=0)
        for op in (17, 19):
            refused(f"op {op}", op=op)
            refused(f"op {op} over Fq", op=op, field=zk.FIELD_FQ)
        refused("a bad index width with n = 0", index_width=3, n=0)
        refused("flags with n = 0", flags=1, n=0)
        refused("NULL d_lens with n = 0", lens=None, n=0)
        refused("misaligned offsets with n = 0", offsets=a["offsets"] + 4, n=0)
        refused("NULL d_bytes with total_bytes > 0 and n = 0", data=None, n=0)
        refused("Fq with n = 0", field=zk.FIELD_FQ, n=0)
        assert len(refusals) == 48
        assert raw_call(zk, ctx, t, n=0) == 0                           # n = 0: ZK_OK, nothing written
        assert raw_call(zk, ctx, t, n=0, digest=out) == 0               # nothing to overlap
        assert raw_call(zk, ctx, t, data=None, total_bytes=0, n=0) == 0
        assert raw_call(zk, ctx, t, total_bytes=(1 << 61) - 1, n=0) == 0  # the largest size taken; nothing is read for n = 0
        ctx.sync()
        assert t.untouched()
    finally:
        t.free()


def test_a_null_buffer_of_no_bytes_gives_the_empty_digest_and_zeros(zk, ctx):
    """total_bytes = 0 with d_bytes NULL is valid: only the empty message at offset 0 lies inside it"""
    t = Call(ctx, b"", [(0, 0), (0, 1), (1, 0), (0, 0)], 4, 5, 6)
    try:
        assert raw_call(zk, ctx, t, data=None) == 0
        for name in OUTPUTS:
            assert np.array_equal(t.result(name), t.want()[name]), name
        assert t.result("digest")[0].tobytes() == sc.empty_digest() and not t.result("digest")[1].any()
    finally:
        t.free()


def test_r_in_defaults_to_r_out(ctx):
    """Context.sha256 without r_in: the reference's table takes both RLCs under one challenge"""
    rng = random.Random(10)
    data, rows = lay_out(rng, [3, 0, 64, 100])
    r = rng.randrange(P)
    t = Call(ctx, data, rows, 4, r, r)
    try:
        a = t.args()
        del a["r_in"]
        ctx.sha256(**a)
        for name in OUTPUTS:
            assert np.array_equal(t.result(name), t.want()[name]), name
    finally:
        t.free()


# ---- 5. profiling
def test_the_call_books_one_launch_group_and_its_bytes(ctx):
    rng = random.Random(9)
    data, rows = lay_out(rng, [rng.randrange(200) for _ in range(255)])
    n = len(rows)

    def booked(call):
        ctx.sync()
        ctx.prof_reset()
        ctx.prof_enable(True)
        try:
            call.check()
            ms, launches = ctx.prof_get("fr_sha256")
            assert ms > 0 and launches == 1
            return ctx.prof_get_bytes("fr_sha256")
        finally:
            ctx.prof_enable(False)
            ctx.prof_reset()
            call.free()
    assert booked(Call(ctx, data, rows, 4, 3, 4)) == n * (2 * 4 + 32 + 64) + len(data)
    assert booked(Call(ctx, data, rows, 8, 3, 4, digest=False, input_rlc=False)) == n * (2 * 8 + 32) + len(data)
    assert booked(Call(ctx, data, rows, 8, 3, 4, digest=True, input_rlc=False)) == n * (2 * 8 + 32 + 32) + len(data)

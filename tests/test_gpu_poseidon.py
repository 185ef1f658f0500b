"""GPU: ZK_OP_POSEIDON of zk_field_vec_op -- the width-3 Poseidon hash columns from typed cells -- bit for bit against the model of
tests/poseidon_cases.py (Python integers over oracle.hashes.poseidon_spec(3, 8, 57)), converted by the oracle (cref.to_mont).  The
reference's five code-hash vectors through the 31-byte layout at an odd address; head-only calls with every width and row counts
around a wave (64) and a workgroup (256); kinds columns with messages across wave and workgroup boundaries, a message longer than a
workgroup, continue rows without a head, off rows, heads in several workgroups; the word outputs; every refusal; the booked bytes;
equality with zk_host_poseidon_permute_width3 row by row."""
import ctypes
import os
import random
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import poseidon_cases as pc  # noqa: E402
from oracle import cref  # noqa: E402

pytestmark = pytest.mark.gpu
P = pc.P
IN_WIDTHS = (1, 2, 4, 8, 16, 31, 32)
CAP_WIDTHS = (1, 2, 4, 8, 16, 32)
SENTINEL = 0xA5C3A5C3A5C3A5C3
GUARD = 3                                   # sentinel cells in front of and behind every output
INVALID_ARG = -1
HEAD, CONT, OFF = pc.HEAD, pc.CONT, pc.OFF


def mont(vals):
    return cref.to_mont(list(vals)) if len(vals) else np.zeros((0, 4), dtype=np.uint64)


def top(width):
    return P - 1 if width == 32 else (1 << (8 * width)) - 1


def random_values(rng, width, n):
    return [rng.choice([0, top(width), rng.randrange(top(width) + 1), rng.randrange(top(width) + 1)]) for _ in range(n)]


def device_bytes(width, vals):
    """packed little-endian cells; the oracle's Montgomery images for width 32; for width 31 big-endian cells at stride 62, 0xEE between"""
    if width == 32:
        return mont(vals).view(np.uint8).reshape(-1)
    if width == 31:
        raw = np.full(62 * (len(vals) - 1) + 31 if vals else 0, 0xEE, dtype=np.uint8)
        for i, v in enumerate(vals):
            raw[62 * i:62 * i + 31] = np.frombuffer(v.to_bytes(31, "big"), dtype=np.uint8)
        return raw
    return np.frombuffer(b"".join(v.to_bytes(width, "little") for v in vals), dtype=np.uint8)


class Call:
    """the columns of one call in ONE source buffer, each at a 16-byte boundary plus its shift (31-byte cells: an odd address), between
    0xEE filler; out, word0 and word1 of n elements each inside GUARD sentinel cells.  data31: the padded bytes of bytecodes laid end to
    end -- in0 and in1 are then its 31-byte cells, in1 = in0 + 31."""

    def __init__(self, ctx, n, in0=None, in1=None, cap=None, kinds=None, data31=None, words=(True, True), cap_scale=1):
        self.ctx, self.n, self.cap, self.kinds, self.cap_scale = ctx, n, cap, kinds, cap_scale
        self.wanted = {}
        chunks, offs, pos = [], {}, 0

        def place(name, raw, shift):
            nonlocal pos
            size = (shift + len(raw) + 15) // 16 * 16 + 16
            chunk = np.full(size, 0xEE, dtype=np.uint8)
            chunk[shift:shift + len(raw)] = raw
            chunks.append(chunk)
            offs[name] = pos + shift
            pos += size
        if data31 is not None:
            assert len(data31) == 62 * n
            self.in0, self.in1 = [(31, v) for v in pc.rows_of_bytes(data31, n)]
            place("in0", np.frombuffer(data31, dtype=np.uint8), 1)
            offs["in1"] = offs["in0"] + 31
        else:
            self.in0, self.in1 = in0, in1
            place("in0", device_bytes(*in0), 1 if in0[0] == 31 else 0)
            place("in1", device_bytes(*in1), 3 if in1[0] == 31 else 0)
        if cap is not None:
            place("cap", device_bytes(*cap), 0)
        if kinds is not None:
            place("kinds", np.array(kinds, dtype=np.uint8), 5)
        self.image = np.concatenate(chunks)
        self.src = ctx.to_device(self.image)
        self.ptr = {name: self.src.ptr + o for name, o in offs.items()}
        self.bufs = {name: ctx.to_device(np.full((n + 2 * GUARD, 4), SENTINEL, dtype=np.uint64)) for name, on in (("out", True), ("word0", words[0]), ("word1", words[1])) if on}

    def out_ptr(self, name="out"):
        return self.bufs[name].ptr + GUARD * 32 if name in self.bufs else None

    def args(self, final=False):
        return dict(in0=self.ptr["in0"], width0=self.in0[0], in1=self.ptr["in1"], width1=self.in1[0], n=self.n, out=self.out_ptr(), cap=self.ptr.get("cap"),
                    cap_width=self.cap[0] if self.cap else 8, cap_scale=mont([self.cap_scale])[0], kinds=self.ptr.get("kinds"), final=final, word0=self.out_ptr("word0"),
                    word1=self.out_ptr("word1"))

    def want(self, final=False):
        key = (final, self.cap is None)
        if key not in self.wanted:
            self.wanted[key] = self.compute(final)
        return self.wanted[key]

    def compute(self, final):
        out, w0, w1 = pc.expected(self.in0[1], self.in1[1], self.cap[1] if self.cap else None, self.kinds, self.cap_scale, final)
        return {"out": out, "word0": w0, "word1": w1}

    def result(self, name="out"):
        """the n elements of an output, after checking that nothing around them was written"""
        got = self.bufs[name].download((self.n + 2 * GUARD, 4))
        assert (got[:GUARD] == SENTINEL).all() and (got[GUARD + self.n:] == SENTINEL).all(), f"{name}: a cell outside [0, n) was written"
        return got[GUARD:GUARD + self.n]

    def check(self, final=False):
        self.ctx.poseidon(**self.args(final))
        want = self.want(final)
        for name in self.bufs:
            got = self.result(name)
            bad = [i for i in range(self.n) if not np.array_equal(got[i], mont([want[name][i]])[0])][:5]
            assert not bad, (name, "first differing rows", bad)
        assert np.array_equal(self.src.download(self.image.shape, np.uint8), self.image), "an input was written"
        return want

    def reset(self):
        for buf in self.bufs.values():
            buf.upload(np.full((self.n + 2 * GUARD, 4), SENTINEL, dtype=np.uint64))

    def untouched(self):
        return all((buf.download((self.n + 2 * GUARD, 4)) == SENTINEL).all() for buf in self.bufs.values()) and np.array_equal(self.src.download(self.image.shape, np.uint8), self.image)

    def free(self):
        self.src.free()
        for buf in self.bufs.values():
            buf.free()


# ---- 1. the reference's five vectors (eth-types/src/utils/codehash.rs:80-110)
@pytest.fixture(scope="module")
def vectors():
    return pc.golden_vectors()


def test_reference_vectors_in_one_call(ctx, vectors):
    """padded bytes, width 31 at an odd address, an 8-byte length column, cap_scale = 2^64: with the final flag every row of each
    message holds the reference's hash; without it the running values, the last one of a message being the hash"""
    codes = [code for code, _ in vectors]
    data, kinds, lens = pc.code_rows(codes)
    n = len(kinds)
    assert n == 1 + 1 + 1 + 1 + 82
    call = Call(ctx, n, data31=data, cap=(8, lens), kinds=kinds, cap_scale=pc.CAP_SCALE_CODE)
    try:
        assert call.ptr["in0"] % 2 == 1 and call.ptr["in1"] == call.ptr["in0"] + 31
        want = call.check(final=True)
        at = 0
        for code, h in vectors:
            rows = len(pc.padded_bytes(code)) // 62
            assert want["out"][at:at + rows] == [h] * rows
            at += rows
        call.reset()
        want = call.check(final=False)
        assert want["out"][n - 1] == vectors[4][1] and want["out"][:4] == [h for _, h in vectors[:4]] and len(set(want["out"][4:])) == 82
    finally:
        call.free()


def test_empty_code_is_one_head_row_of_zeros(ctx, vectors):
    call = Call(ctx, 1, data31=bytes(62), cap=(8, [0]), kinds=[HEAD], cap_scale=pc.CAP_SCALE_CODE)
    try:
        assert call.check(final=True)["out"] == [vectors[0][1]]
    finally:
        call.free()


# ---- 2. head-only calls: lane = row
@pytest.mark.parametrize("index,n", list(enumerate([1, 63, 64, 65, 255, 256, 257, 513])))
def test_head_only_row_counts_and_every_width(ctx, index, n):
    """eight row counts around a wave and a workgroup; over them in0 and in1 take each of the seven widths and the capacity each of its six"""
    rng = random.Random(100 + n)
    w0, w1, wc = IN_WIDTHS[index % 7], IN_WIDTHS[(index + 3) % 7], CAP_WIDTHS[index % 6]
    call = Call(ctx, n, (w0, random_values(rng, w0, n)), (w1, random_values(rng, w1, n)), cap=(wc, random_values(rng, wc, n)), cap_scale=rng.choice([1, 1 << 64, rng.randrange(P)]))
    try:
        call.check()
    finally:
        call.free()


def test_head_only_width_coverage_of_the_cases_above():
    used0 = {IN_WIDTHS[i % 7] for i in range(8)}
    used1 = {IN_WIDTHS[(i + 3) % 7] for i in range(8)}
    assert used0 == used1 == set(IN_WIDTHS) and {CAP_WIDTHS[i % 6] for i in range(8)} == set(CAP_WIDTHS)


def test_head_only_without_a_capacity_column_and_with_the_final_flag(ctx):
    n = 65
    rng = random.Random(3)
    call = Call(ctx, n, (8, random_values(rng, 8, n)), (16, random_values(rng, 16, n)))
    try:
        want = call.check()
        assert want["out"][0] == pc.SPEC.permute([0, call.in0[1][0], call.in1[1][0]])[0]
        call.reset()
        call.check(final=True)                                          # every row is its own message
    finally:
        call.free()


# ---- 3. kinds
def layout_a(rng):
    """808 rows, four workgroups: a continue on row 0; messages across a wave and a workgroup boundary; one of 301 rows; a continue
    behind an off row; heads in every workgroup; a head on the last row; high bits set in the kind bytes"""
    n = 808
    kinds = [HEAD] * n
    kinds[0] = CONT
    kinds[1] = CONT
    for r in range(61, 70):                 # head at 60, across the wave boundary at 64
        kinds[r] = CONT
    for r in range(251, 262):               # head at 250, across the workgroup boundary at 256
        kinds[r] = CONT
    for r in range(301, 601):               # head at 300: 301 rows, across two workgroup boundaries
        kinds[r] = CONT
    kinds[610] = OFF
    kinds[611] = CONT                       # behind an off row: from the zero state
    kinds[612] = CONT
    kinds[700] = 3
    kinds[701] = OFF
    kinds[n - 2] = OFF
    kinds[n - 1] = HEAD
    return n, [k | (rng.randrange(64) << 2) for k in kinds]


def layout_b(rng):
    """off rows at both ends, short messages between"""
    n = 300
    kinds = [OFF, 3] + [rng.choice([HEAD, CONT, CONT, OFF]) for _ in range(n - 4)] + [OFF, OFF]
    return n, kinds


@pytest.mark.parametrize("final", [False, True])
@pytest.mark.parametrize("layout", [layout_a, layout_b])
def test_kinds(ctx, layout, final):
    rng = random.Random(7)
    n, kinds = layout(rng)
    if layout is layout_a:
        assert len({i // 256 for i, k in enumerate(kinds) if k & 3 == HEAD}) >= 4 and any(k > 3 for k in kinds)
    call = Call(ctx, n, (31, random_values(rng, 31, n)), (8, random_values(rng, 8, n)), cap=(4, random_values(rng, 4, n)), kinds=kinds, cap_scale=1 << 64)
    try:
        want = call.check(final)
        off = [i for i, k in enumerate(kinds) if k & 3 >= OFF]
        assert off and all(want["out"][i] == want["word0"][i] == want["word1"][i] == 0 for i in off)
    finally:
        call.free()


def test_all_rows_off(ctx):
    n = 130
    rng = random.Random(5)
    call = Call(ctx, n, (2, random_values(rng, 2, n)), (32, random_values(rng, 32, n)), cap=(8, random_values(rng, 8, n)), kinds=[OFF + (i & 1) for i in range(n)])
    try:
        want = call.check()
        assert not any(want["out"]) and not any(want["word0"]) and not any(want["word1"])
    finally:
        call.free()


def test_a_kinds_call_follows_a_larger_one_on_the_same_context(ctx):
    """the list and its count live in context scratch: a call of few messages after one of many"""
    rng = random.Random(6)
    for n, kinds in ((600, [HEAD] * 600), (70, [HEAD] + [CONT] * 69)):
        call = Call(ctx, n, (1, random_values(rng, 1, n)), (1, random_values(rng, 1, n)), kinds=kinds)
        try:
            call.check(final=True)
        finally:
            call.free()


# ---- 4. word outputs
@pytest.mark.parametrize("width", [8, 31, 32])
def test_word_outputs(ctx, width):
    n = 70
    rng = random.Random(width)
    kinds = [rng.choice([HEAD, CONT, OFF]) for _ in range(n)]
    call = Call(ctx, n, (width, random_values(rng, width, n)), (width, random_values(rng, width, n)), cap=(8, random_values(rng, 8, n)), kinds=kinds)
    try:
        want = call.check()
        live = [i for i, k in enumerate(kinds) if k < OFF]
        assert [want["word0"][i] for i in live] == [call.in0[1][i] % P for i in live]
    finally:
        call.free()


@pytest.mark.parametrize("words", [(True, False), (False, True), (False, False)])
def test_only_some_of_the_word_outputs(ctx, words):
    n = 66
    rng = random.Random(11)
    kinds = [rng.choice([HEAD, CONT, OFF]) for _ in range(n)]
    for k in (None, kinds):
        call = Call(ctx, n, (31, random_values(rng, 31, n)), (16, random_values(rng, 16, n)), kinds=k, words=words)
        try:
            call.check()
        finally:
            call.free()


# ---- 5. refusals
def raw_call(zk, ctx, c, n=None, field=0, op=14, flags=0, scale=None, **over):
    a = c.args()
    a.update(over)
    desc = zk.binding._Poseidon(a["in0"], a["in1"], a["cap"], a["kinds"], a["word0"], a["word1"], a["width0"], a["width1"], a["cap_width"], flags)
    hk = np.ascontiguousarray(mont([1])[0] if scale is None else scale)
    return zk.lib().zk_field_vec_op(ctx.h, ctypes.c_int(field), ctypes.c_int(op), ctypes.byref(desc), hk.ctypes.data_as(ctypes.c_void_p), ctypes.c_void_p(a["out"]),
                                    ctypes.c_size_t(c.n if n is None else n))


def test_refused_calls_write_nothing_and_leave_the_context_usable(zk, ctx):
    """EACH refusal is followed by its own checks: the guarded outputs and the inputs are untouched, and the next valid call works"""
    n = 64
    rng = random.Random(8)
    kinds = [rng.choice([HEAD, CONT, OFF]) for _ in range(n)]
    t = Call(ctx, n, (8, random_values(rng, 8, n)), (32, random_values(rng, 32, n)), cap=(16, random_values(rng, 16, n)), kinds=kinds)
    refusals = []
    out, w0, w1 = t.out_ptr(), t.out_ptr("word0"), t.out_ptr("word1")
    p = t.ptr

    def refused(what, **kw):
        assert raw_call(zk, ctx, t, **kw) == INVALID_ARG, what
        ctx.sync()
        assert t.untouched(), what
        t.check()                                                       # the next valid call
        t.reset()
        refusals.append(what)
    try:
        refused("Fq", field=zk.FIELD_FQ)
        for wrong in (0, 3, 5, 24, 30, 33, 64):
            refused(f"width0 {wrong}", width0=wrong)
            refused(f"width1 {wrong}", width1=wrong)
            refused(f"cap_width {wrong}", cap_width=wrong)
        refused("cap_width 31", cap_width=31)
        refused("NULL d_in0", in0=None)
        refused("NULL d_in1", in1=None)
        refused("8-byte cells at an address that is 4 mod 8", in0=p["in0"] + 4)
        refused("field elements at an address that is 4 mod 8", in1=p["in1"] + 4)
        refused("halfwords at an odd address", in1=p["in1"] + 1, width1=2)
        refused("a 16-byte capacity at an address that is 8 mod 16", cap=p["cap"] + 8)
        for bits in (2, 4, 128, 254):
            refused(f"flag bits {bits}", flags=bits)
        refused("d_in0 inside d_out", in0=out + 8)
        refused("d_in1 AT d_out", in1=out)
        refused("d_in1 one element in front of d_out", in1=out - 32)
        refused("d_cap inside d_word0", cap=w0 + 16)
        refused("d_kinds inside d_word1", kinds=w1 + 5)
        refused("31-byte cells whose last cell reaches d_out", in0=out - (62 * (n - 1) + 31) + 1, width0=31)
        refused("d_out inside d_in1", out=p["in1"] + 32)
        refused("d_word0 AT d_out", word0=out)
        refused("d_word1 one element into d_word0", word1=w0 + 32)
        refused("d_word1 AT d_in0", word1=p["in0"])
        for op in (13, 15):
            refused(f"op {op}", op=op)
            refused(f"op {op} over Fq", op=op, field=zk.FIELD_FQ)
        refused("a bad width with n = 0", width0=3, n=0)
        refused("a bad capacity width with n = 0", cap_width=31, n=0)
        refused("NULL d_in1 with n = 0", in1=None, n=0)
        refused("a misaligned column with n = 0", in0=p["in0"] + 4, n=0)
        refused("flag bits with n = 0", flags=2, n=0)
        refused("Fq with n = 0", field=zk.FIELD_FQ, n=0)
        assert len(refusals) == 53
        assert raw_call(zk, ctx, t, n=0) == 0                           # n = 0: ZK_OK, nothing written
        assert raw_call(zk, ctx, t, n=0, in1=out) == 0                  # nothing to overlap
        ctx.sync()
        assert t.untouched()
        assert raw_call(zk, ctx, t, cap=None, cap_width=77) == 0        # cap_width is ignored without a capacity column
        t.cap = None
        want = t.want()
        assert np.array_equal(t.result(), mont(want["out"]))
    finally:
        t.free()


# ---- 6. profiling
def test_the_call_books_its_bytes(ctx):
    n = 255
    rng = random.Random(9)

    def booked(call, final=False):
        ctx.sync()
        ctx.prof_reset()
        ctx.prof_enable(True)
        try:
            call.check(final)
            ms, launches = ctx.prof_get("fr_poseidon")
            assert ms > 0 and launches == 1
            return ctx.prof_get_bytes("fr_poseidon")
        finally:
            ctx.prof_enable(False)
            ctx.prof_reset()
            call.free()
    head_only = Call(ctx, n, (31, random_values(rng, 31, n)), (4, random_values(rng, 4, n)), cap=(16, random_values(rng, 16, n)))
    assert booked(head_only) == n * (31 + 4 + 16 + 32 + 64)
    no_words = Call(ctx, n, (32, random_values(rng, 32, n)), (1, random_values(rng, 1, n)), words=(False, False))
    assert booked(no_words) == n * (32 + 1 + 32)
    kinds = [rng.choice([HEAD, CONT, CONT, OFF]) for _ in range(n)]
    with_kinds = Call(ctx, n, (31, random_values(rng, 31, n)), (31, random_values(rng, 31, n)), cap=(8, random_values(rng, 8, n)), kinds=kinds, words=(True, False))
    assert booked(with_kinds, final=True) == n * (31 + 31 + 8 + 1 + 32 + 32)


# ---- 7. against the host permutation on the same inputs
def test_equals_the_host_permutation_row_by_row(zk, ctx):
    n = 257
    rng = random.Random(10)
    vals = [[rng.randrange(P) for _ in range(n)] for _ in range(3)]
    call = Call(ctx, n, (32, vals[1]), (32, vals[2]), cap=(32, vals[0]), words=(False, False))
    try:
        ctx.poseidon(**call.args())
        got = call.result()
        states = np.stack([mont(v) for v in vals], axis=1)              # (n, 3, 4)
        host = np.stack([zk.binding.host_poseidon_permute_width3(states[i])[0] for i in range(n)])
        assert np.array_equal(got, host)
    finally:
        call.free()

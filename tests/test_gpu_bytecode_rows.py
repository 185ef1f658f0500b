"""GPU: ZK_OP_BYTECODE_ROWS of zk_field_vec_op -- every output byte for byte against the model of tests/bytecode_rows_cases.py (the
reference's unroller and assignment loop in Python), with sentinels in front of and behind every buffer.

T = 1024 is the implementation's tile (BC_TILE of csrc/bytecode_rows.hip.hpp): a workgroup takes T rows, and the state that enters a
tile comes out of a 64-ary hierarchy of composed transition maps.  The alignment sweep puts a 70-byte code of PUSH1, PUSH32 and data
behind a first bytecode of every length 0 .. 2 T, so that every byte of every push meets a tile boundary; the large case fills 2^19
rows, 512 tiles, 8 nodes above them and the root above those, with one random bytecode beside small ones."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import bytecode_rows_cases as bc  # noqa: E402
from oracle import bn254  # noqa: E402

pytestmark = pytest.mark.gpu
T = 1024
GUARD = 64                                   # sentinel bytes in front of and behind every buffer
SENT = 0xC3
OK, INVALID_ARG = 0, -1
OUTPUTS = ("tag", "index", "value", "is_code", "push_data_left", "push_data_size", "length", "acc_kinds", "rlc_kinds")
WIDTH = bc.INT_WIDTHS
DTYPE = {1: np.uint8, 4: np.uint32}
FIELD = {"tag": "d_tag", "index": "d_index", "value": "d_value", "is_code": "d_is_code", "push_data_left": "d_push_data_left", "push_data_size": "d_push_data_size",
         "length": "d_length", "acc_kinds": "d_acc_kinds", "rlc_kinds": "d_rlc_kinds"}
MIXED = bytes([0x60, 0x7f, 0x01, 0x7f]) + bytes(range(0x60, 0x80)) + bytes([0x00, 0x60, 0x60, 0x5b, 0x61, 0x7f, 0x7f, 0x02]) + bytes([0x7f] * 3) + bytes(range(0x10, 0x25)) + bytes([0x60, 0x7f])
assert len(MIXED) == 70


def effective(buf, offs, lens, total):
    """what the op takes every entry for: an entry outside the buffer is an empty bytecode"""
    return [bytes(buf[o:o + ln]) if o <= total and ln <= total - o else b"" for o, ln in zip(offs, lens)]


class Call:
    """one call: inputs on the device, every output inside one arena of sentinels that is downloaded at once"""

    def __init__(self, ctx, n, buf, offs, lens, iw=4, outputs=OUTPUTS, hashes=True, odd=False, total=None, rng=None, n_alloc=None):
        rng = rng or np.random.default_rng(len(offs) * 7919 + n)
        self.ctx, self.n, self.iw, self.outputs, self.odd = ctx, n, iw, tuple(outputs), odd
        self.buf = np.asarray(buf, dtype=np.uint8)
        self.total = len(self.buf) if total is None else total
        self.offs, self.lens, self.count = list(offs), list(lens), len(offs)
        idt = np.uint32 if iw == 4 else np.uint64
        # the bytes stand between sentinels of their own: nothing of them is ever written
        self.src_image = np.concatenate([np.full(GUARD + 1, SENT, np.uint8), self.buf, np.full(GUARD, SENT, np.uint8)])
        self.src = ctx.to_device(self.src_image)
        self.d_offs = ctx.to_device(np.array(self.offs + [0], dtype=idt))
        self.d_lens = ctx.to_device(np.array(self.lens + [0], dtype=idt))
        self.hash_vals = rng.integers(0, 2**62, (max(self.count, 1), 4), dtype=np.uint64) if hashes else None
        self.d_hashes = ctx.to_device(self.hash_vals) if hashes else None
        self.empty = rng.integers(0, 2**62, 4, dtype=np.uint64)
        cap = n if n_alloc is None else n_alloc
        self.at, size = {}, 0
        for name in ("out",) + self.outputs:
            width = 32 if name == "out" else WIDTH[name]
            self.at[name] = size + GUARD + (1 if odd and width == 1 else 0)
            size += (2 * GUARD + cap * width + 1 + 63) & ~63
        self.size = size
        self.arena = ctx.to_device(np.full(size, SENT, np.uint8))

    def ptr(self, name):
        return self.arena.ptr + self.at[name] if name in self.at else None

    def kwargs(self):
        kw = dict(data=self.src.ptr + GUARD + 1, total_bytes=self.total, offsets=self.d_offs.ptr, lens=self.d_lens.ptr, index_width=self.iw, count=self.count, n=self.n,
                  hash_out=self.ptr("out"), empty_hash=self.empty, hashes=None if self.d_hashes is None else self.d_hashes.ptr)
        kw.update({name: self.ptr(name) for name in self.outputs})
        return kw

    def run(self):
        self.ctx.bytecode_rows(**self.kwargs())
        self.ctx.sync()
        return self.arena.download(self.size, np.uint8)

    def split(self, image):
        """the n cells of every output; everything else in the arena still holds the sentinel"""
        mask = np.ones(self.size, bool)
        got = {}
        for name, at in self.at.items():
            width = 32 if name == "out" else WIDTH[name]
            mask[at:at + self.n * width] = False
            cells = image[at:at + self.n * width].copy()
            got[name] = cells.view(np.uint64).reshape(self.n, 4) if name == "out" else cells.view(DTYPE[width])
        assert (image[mask] == SENT).all(), "a byte outside the n cells of an output was written"
        return got

    def want(self):
        codes = effective(self.buf, self.offs, self.lens, self.total)
        w = bc.rows_numpy(codes, self.n)
        if self.n <= 6000:                   # the line-by-line model where it is quick, the vectorised one (checked against it on the CPU) above
            m = bc.assign(codes, [0] * len(codes), self.n, 0, fail_fast=False)
            for name in OUTPUTS:
                assert np.array_equal(np.array(m[name], dtype=np.uint64) % 2**32, w[name].astype(np.uint64)), name
        owner = w.pop("owner")
        table = np.concatenate([self.hash_vals[:self.count] if self.hash_vals is not None else np.zeros((self.count, 4), np.uint64), self.empty.reshape(1, 4)])
        w["out"] = table[np.where(owner < 0, self.count, owner)]
        return w

    def check(self, want=None):
        got, want = self.split(self.run()), self.want() if want is None else want
        for name, a in got.items():
            diff = np.asarray(a != want[name]).reshape(self.n, -1).any(axis=1) if self.n else np.zeros(0, bool)
            assert not diff.any(), (name, "first differing rows", np.argwhere(diff)[:5].ravel().tolist(), a[diff][:5].tolist(), want[name][diff][:5].tolist())
        assert np.array_equal(self.src.download(len(self.src_image), np.uint8), self.src_image), "the code bytes were written"
        return got

    def free(self):
        for b in (self.src, self.d_offs, self.d_lens, self.d_hashes, self.arena):
            if b is not None:
                b.free()


def checked(ctx, codes, n=None, gap=3, **kw):
    rng = np.random.default_rng(sum(len(c) for c in codes) + len(codes))
    buf, offs, lens = bc.lay_out(codes, rng, gap)
    total = sum(len(c) + 1 for c in codes)
    call = Call(ctx, total + 37 if n is None else n, buf, offs, lens, rng=rng, **kw)
    try:
        return call.check()
    finally:
        call.free()


def test_alignment_sweep_of_a_mixed_code_against_the_tile_boundaries(ctx):
    """a first bytecode of j zero bytes, j = 0 .. 2 T, pushes the 70-byte code through every alignment to two tile boundaries.  One
    arena and one n for all j: only the first length changes, on the device."""
    n = 2 * T + 70 + 2 + 90
    buf, offs, lens = bc.lay_out([bytes(2 * T), MIXED])
    call = Call(ctx, n, buf, offs, [0, 70])
    try:
        fixed = bc.assign([MIXED], [0], 71, 0)
        block = {name: np.array(fixed[name], dtype=DTYPE[WIDTH[name]]) for name in OUTPUTS}
        table = np.concatenate([call.hash_vals[:2], call.empty.reshape(1, 4)])

        def want(j):
            w = {name: np.zeros(n, DTYPE[WIDTH[name]]) for name in OUTPUTS}
            w["value"][0] = j
            w["length"][:j + 1] = j
            w["tag"][1:j + 1] = 1
            w["is_code"][1:j + 1] = 1
            w["index"][1:j + 1] = np.arange(j)
            for name in OUTPUTS:
                w[name][j + 1:j + 72] = block[name]
            owner = np.full(n, 2)
            owner[:j + 1], owner[j + 1:j + 72] = 0, 1
            w["out"] = table[owner]
            return w

        call.lens[0] = 5                     # the quick construction above is the model's
        model = bc.assign(effective(call.buf, call.offs, call.lens, call.total), [0, 0], n, 0)
        assert all(np.array_equal(np.array(model[name], dtype=np.uint64), want(5)[name].astype(np.uint64)) for name in OUTPUTS)
        for j in range(2 * T + 1):
            call.lens[0] = j
            call.d_lens.upload(np.array([j, 70, 0], dtype=np.uint32))
            got, w = call.split(call.run()), want(j)
            for name, a in got.items():
                assert np.array_equal(a, w[name]), (j, name, np.argwhere(np.asarray(a != w[name]).reshape(n, -1).any(axis=1))[:5].ravel().tolist())
    finally:
        call.free()


@pytest.mark.parametrize("code", [bytes([0x7f] * 200), bytes([0x60] * 200)], ids=["200x7f", "200x60"])
def test_bytes_that_all_look_like_pushes(ctx, code):
    got = checked(ctx, [code])
    assert int(got["is_code"].sum()) == {0x7f: 7, 0x60: 100}[code[0]]


@pytest.mark.parametrize("left", [0, 1, 31])
def test_push32_with_few_bytes_left_before_the_end(ctx, left):
    checked(ctx, [bytes([0x01, 0x02, 0x7f]) + bytes(range(0x60, 0x60 + left)), bytes([0x60, 0x01])])


def test_a_header_directly_behind_truncated_push_data(ctx):
    got = checked(ctx, [bytes([0x7f, 0x60, 0x60]), bytes([0x61, 0xaa, 0xbb, 0x00]), b"", bytes([0x7f])], gap=0)
    assert got["push_data_left"].tolist()[:9] == [0, 0, 32, 31, 0, 0, 2, 1, 0]


def test_a_hundred_empty_bytecodes_in_a_row(ctx):
    got = checked(ctx, [bytes([0x62, 0x01])] + [b""] * 100 + [bytes([0x60, 0x60, 0x60])])
    assert not got["tag"][3:103].any()


def test_no_bytecodes_is_all_padding(ctx):
    call = Call(ctx, 1500, np.zeros(0, np.uint8), [], [])
    try:
        got = call.check()
        assert (got["out"] == call.empty).all() and not any(got[name].any() for name in OUTPUTS)
    finally:
        call.free()


def test_no_rows(ctx):
    buf, offs, lens = bc.lay_out([MIXED])
    call = Call(ctx, 0, buf, offs, lens, n_alloc=8)
    try:
        image = call.run()
        assert (image == SENT).all()
    finally:
        call.free()


@pytest.mark.parametrize("n", [1, 70, 71 + 35, T, T + 1])
def test_n_smaller_than_the_rows_cuts_without_touching_the_rest(ctx, n):
    rng = np.random.default_rng(n)
    checked(ctx, [MIXED, bc.random_code(rng, 2 * T), MIXED], n=n)


def test_n_larger_than_the_rows_pads(ctx):
    rng = np.random.default_rng(11)
    checked(ctx, [bc.random_code(rng, 300), MIXED], n=3 * T + 5)


def test_one_bytecode_that_fills_2_19_rows_beside_small_ones(ctx):
    """512 tiles, 8 nodes of 64 tiles, one root: every level of the 64-ary hierarchy has several nodes"""
    rng = np.random.default_rng(19)
    small = [bc.random_code(rng, int(k)) for k in rng.integers(0, 40, 6)]
    n = 1 << 19
    big = bc.random_code(rng, n - sum(len(c) + 1 for c in small) - 1 - 2, push_share=0.5)
    checked(ctx, small[:3] + [big] + small[3:], n=n)


@pytest.mark.parametrize("iw", [4, 8])
def test_invalid_entries_between_valid_ones_count_as_empty(ctx, iw):
    rng = np.random.default_rng(iw)
    buf = np.frombuffer(bc.random_code(rng, 400), dtype=np.uint8)
    top = 2**(8 * iw)
    offs = [0, 401, 10, 390, top - 1, 100, top - 4, 400, 0, 50]
    lens = [70, 0, top - 1, 11, 1, 33, 8, 0, 401, top - 50]
    call = Call(ctx, 70 + 33 + 10 + 40, buf, offs, lens, iw=iw)
    try:
        call.check()
    finally:
        call.free()


def test_unaligned_overlapping_and_repeated_bytecodes(ctx):
    rng = np.random.default_rng(5)
    buf = np.frombuffer(bc.random_code(rng, 600, push_share=0.4), dtype=np.uint8)
    offs = [1, 2, 3, 1, 1, 250, 251, 599, 0, 7]
    lens = [100, 99, 98, 100, 599, 77, 77, 1, 600, 5]
    call = Call(ctx, sum(lens) + len(lens) + 9, buf, offs, lens)
    try:
        call.check()
    finally:
        call.free()


def test_one_byte_outputs_at_odd_addresses(ctx):
    rng = np.random.default_rng(6)
    for n in (3, 70, T + 7, 2 * T + 3):
        checked(ctx, [bc.random_code(rng, 2 * T + 200, push_share=0.4), MIXED], n=n, odd=True)


@pytest.mark.parametrize("name", OUTPUTS)
def test_each_output_alone(ctx, name):
    rng = np.random.default_rng(8)
    checked(ctx, [MIXED, bc.random_code(rng, T + 50), b"", MIXED], outputs=(name,))


def test_without_code_hashes_the_rows_of_a_bytecode_hold_zero(ctx):
    got = checked(ctx, [MIXED, b"", MIXED], hashes=False)
    assert not got["out"][:143].any() and got["out"][143:].any()


def test_the_hashes_only_call_reads_no_code_byte(ctx):
    """d_bytes points at a buffer that is shorter than total_bytes says: total_bytes is honest about the lengths, and the call, which
    has no output that reads a byte, must not touch it.  The rows come out as if the bytes were there."""
    rng = np.random.default_rng(9)
    codes = [bc.random_code(rng, 3000), MIXED, bc.random_code(rng, 500)]
    buf, offs, lens = bc.lay_out(codes)
    call = Call(ctx, sum(lens) + 3 + 20, buf, offs, lens, outputs=())
    short = ctx.to_device(np.full(2 * GUARD + 16, SENT, np.uint8))
    try:
        kw = call.kwargs()
        kw["data"] = short.ptr + GUARD
        ctx.bytecode_rows(**kw)
        ctx.sync()
        got, want = call.split(call.arena.download(call.size, np.uint8)), call.want()
        assert np.array_equal(got["out"], want["out"])
        assert (short.download(2 * GUARD + 16, np.uint8) == SENT).all()
    finally:
        short.free()
        call.free()


def test_the_same_call_twice_gives_the_same_bytes(ctx):
    rng = np.random.default_rng(10)
    buf, offs, lens = bc.lay_out([bc.random_code(rng, 5 * T, push_share=0.5), MIXED, b"", bc.random_code(rng, 700)])
    call = Call(ctx, sum(lens) + 4 + 50, buf, offs, lens)
    try:
        first = call.run()
        assert np.array_equal(first, call.run())
        call.check()
    finally:
        call.free()


def test_refusals_leave_the_outputs_untouched_and_the_context_usable(zk, ctx):
    b = zk.binding
    rng = np.random.default_rng(12)
    n = 150
    buf, offs, lens = bc.lay_out([MIXED, MIXED])
    call = Call(ctx, n, buf, offs, lens)
    vals = [[int.from_bytes(rng.bytes(31), "little") for _ in range(4)] for _ in range(2)]
    x, y = (ctx.to_device(bc.to_mont(v)) for v in vals)
    add_out = ctx.alloc(128)
    empty = np.ascontiguousarray(call.empty)

    def desc(**change):
        kw = call.kwargs()
        f = dict(d_bytes=kw["data"], total_bytes=kw["total_bytes"], d_offsets=kw["offsets"], d_lens=kw["lens"], d_hashes=kw["hashes"], count=call.count, index_width=4, flags=0)
        f.update({FIELD[name]: kw[name] for name in OUTPUTS})
        f.update(change)
        return b._BytecodeRows(*[f[name] for name, _ in b._BytecodeRows._fields_])

    def refused(d, field=0, op=26, rows=n, out=None, why=""):
        rc = zk.lib().zk_field_vec_op(ctx.h, field, op, ctypes.byref(d), empty.ctypes.data_as(ctypes.c_void_p), ctypes.c_void_p(call.ptr("out") if out is None else out), ctypes.c_size_t(rows))
        ctx.sync()
        assert rc == INVALID_ARG, why
        assert (call.arena.download(call.size, np.uint8) == SENT).all(), why
        assert zk.lib().zk_field_vec_op(ctx.h, 0, 0, ctypes.c_void_p(x.ptr), ctypes.c_void_p(y.ptr), ctypes.c_void_p(add_out.ptr), ctypes.c_size_t(4)) == OK, why
        ctx.sync()
        assert bc.from_mont(add_out.download((4, 4))) == [(u + v) % bn254.R_MOD for u, v in zip(*vals)], why

    try:
        refused(desc(), field=1, why="Fq")
        refused(desc(), field=1, rows=0, why="Fq is looked at before n")
        for iw in (0, 1, 2, 3, 5, 16):
            refused(desc(index_width=iw), why=f"index_width {iw}")
        refused(desc(flags=1), why="flags")
        refused(desc(flags=1), rows=0, why="validated before n is looked at")
        refused(desc(d_offsets=None), why="NULL d_offsets")
        refused(desc(d_lens=None), why="NULL d_lens")
        refused(desc(d_offsets=call.d_offs.ptr + 2), why="misaligned d_offsets")
        refused(desc(d_lens=call.d_lens.ptr + 1), why="misaligned d_lens")
        refused(desc(d_bytes=None), why="NULL d_bytes with bytes")
        refused(desc(d_hashes=call.d_hashes.ptr + 4), why="d_hashes at 4")
        refused(desc(), out=call.ptr("out") + 8, why="d_out at 8")
        for name in ("index", "value", "length"):
            refused(desc(**{FIELD[name]: call.ptr(name) + 2}), why=f"misaligned {name}")
        refused(desc(), rows=2**32, why="n = 2^32")
        refused(desc(total_bytes=2**61), why="total_bytes = 2^61")
        # overlaps: an output with an input, with d_out, with another output
        refused(desc(d_tag=call.src.ptr + GUARD + 10), why="d_tag inside d_bytes")
        refused(desc(d_is_code=call.d_lens.ptr), why="d_is_code over d_lens")
        refused(desc(d_index=call.d_hashes.ptr), why="d_index over d_hashes")
        refused(desc(d_value=call.d_offs.ptr + 4), why="d_value over d_offsets")
        refused(desc(d_acc_kinds=call.ptr("out") + 32 * n - 1), why="d_acc_kinds over the last byte of d_out")
        refused(desc(d_rlc_kinds=call.ptr("tag") + n - 1), why="d_rlc_kinds over the last byte of d_tag")
        refused(desc(d_length=call.ptr("index")), why="d_length is d_index")
        refused(desc(d_push_data_left=call.ptr("push_data_size")), why="d_push_data_left is d_push_data_size")
        for op in (25, 27):
            rc = zk.lib().zk_field_vec_op(ctx.h, 0, op, ctypes.c_void_p(x.ptr), ctypes.c_void_p(y.ptr), ctypes.c_void_p(call.ptr("out")), ctypes.c_size_t(4))
            assert rc == INVALID_ARG, op
            refused(desc(), op=op, rows=4, why=f"op {op}")
        # and the accepted neighbours of some refusals: n = 0 with a valid descriptor, count = 0 without offsets
        assert zk.lib().zk_field_vec_op(ctx.h, 0, 26, ctypes.byref(desc()), empty.ctypes.data_as(ctypes.c_void_p), ctypes.c_void_p(call.ptr("out")), ctypes.c_size_t(0)) == OK
        ctx.sync()
        assert (call.arena.download(call.size, np.uint8) == SENT).all()
        call.check()
    finally:
        for buf_ in (x, y, add_out):
            buf_.free()
        call.free()

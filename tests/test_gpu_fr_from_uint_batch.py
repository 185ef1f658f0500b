"""GPU: zk_fr_from_uint_batch (several columns of packed little-endian unsigned cells -> Montgomery Fr, sixteen columns per launch)
against two references, bit for bit: the oracle's conversion of the Python integers, and the single-column zk_fr_from_uint on the
same device bytes.  Sizes below a sweep, at and around one wave's 256 cells, and a ragged tail; column counts of one launch, a full
launch, one over, two full launches plus one; the five widths interleaved (neighbouring workgroups take different paths) and
sixteen columns of bytes; all-zero, all-ones and random cells; byte and halfword sources one cell past a 16-byte boundary (a partial
first packed word); every output inside a guarded buffer; shared sources; refused arguments write nothing."""
import ctypes
import functools

import numpy as np
import pytest

from oracle import bn254 as b
from oracle import cref

pytestmark = pytest.mark.gpu
WIDTHS = (1, 2, 4, 8, 16)
SIZES = (1, 63, 64, 255, 256, 257, 1021)
COUNTS = (1, 2, 16, 17, 33)
KINDS = ("zero", "ones", "random")
SENTINEL = 0xA5C3A5C3A5C3A5C3
GUARD = 3                                   # sentinel cells in front of and behind every output column


@functools.lru_cache(maxsize=None)
def cells(width: int, n: int, kind: str, salt: int = 0):
    """n cells of `width` bytes as Python integers, and their Montgomery images by the oracle (value * R mod p)"""
    top = (1 << (8 * width)) - 1
    if kind == "zero":
        vals = [0] * n
    elif kind == "ones":
        vals = [top] * n
    else:
        vals, state = [], 0x7E57 + 131 * width + salt
        while len(vals) < n:
            state, lo = b.splitmix64(state)
            state, hi = b.splitmix64(state)
            vals.append((lo | hi << 64) & top)
    want = cref.to_mont(vals)
    want.setflags(write=False)
    return tuple(vals), want


def packed_bytes(vals, width: int) -> np.ndarray:
    return np.frombuffer(b"".join(v.to_bytes(width, "little") for v in vals), dtype=np.uint8)


class Batch:
    """columns laid out in ONE source buffer (each at a 16-byte boundary, bytes and halfwords one cell past it) and ONE output
    buffer full of sentinels (GUARD cells around every column)"""

    def __init__(self, ctx, columns, n):
        self.ctx, self.n, self.columns = ctx, n, columns            # columns: [(width, values, oracle image)]
        self.src_off, pos, chunks = [], 0, []
        for width, vals, _ in columns:
            lead = width if width < 4 else 0
            raw = packed_bytes(vals, width)
            size = (lead + len(raw) + 15) // 16 * 16
            chunk = np.full(size, 0xEE, dtype=np.uint8)
            chunk[lead:lead + len(raw)] = raw
            chunks.append(chunk)
            self.src_off.append(pos + lead)
            pos += size
        self.src = ctx.to_device(np.concatenate(chunks))
        self.stride = n + 2 * GUARD
        self.out = ctx.to_device(np.full((len(columns) * self.stride, 4), SENTINEL, dtype=np.uint64))

    def src_ptrs(self):
        return [self.src.ptr + o for o in self.src_off]

    def out_ptrs(self):
        return [self.out.ptr + (j * self.stride + GUARD) * 32 for j in range(len(self.columns))]

    def widths(self):
        return [c[0] for c in self.columns]

    def download(self):
        return self.out.download((len(self.columns), self.stride, 4))

    def check(self):
        """every column equals the oracle and the single-column call; the guards are untouched"""
        got = self.download()
        assert (got[:, :GUARD] == SENTINEL).all() and (got[:, GUARD + self.n:] == SENTINEL).all(), "a cell outside [0, n) was written"
        single = self.ctx.alloc(self.n * 32)
        try:
            for j, (width, _, want) in enumerate(self.columns):
                assert np.array_equal(got[j, GUARD:GUARD + self.n], want), (j, width)
                lib_single(self.ctx, self.src_ptrs()[j], width, self.n, single.ptr)
                assert np.array_equal(got[j, GUARD:GUARD + self.n], single.download((self.n, 4))), (j, width)
        finally:
            single.free()

    def free(self):
        self.src.free()
        self.out.free()


def lib_single(ctx, src_ptr, width, n, out_ptr):
    import zkevm_circuits_amd as z
    ctx._ck(z.lib().zk_fr_from_uint(ctx.h, ctypes.c_void_p(src_ptr), ctypes.c_uint32(width), ctypes.c_size_t(n), ctypes.c_void_p(out_ptr)))


def raw_call(zk, ctx, ptrs, widths, n, outs, count=None):
    cnt = len(ptrs) if count is None else count
    pp = (ctypes.c_void_p * max(len(ptrs), 1))(*ptrs)
    po = (ctypes.c_void_p * max(len(outs), 1))(*outs)
    wd = (ctypes.c_uint8 * max(len(widths), 1))(*widths)
    return zk.lib().zk_fr_from_uint_batch(ctx.h, pp, wd, cnt, n, po)


@pytest.mark.parametrize("count", COUNTS)
@pytest.mark.parametrize("n", SIZES)
def test_interleaved_widths_equal_both_references(ctx, n, count):
    cols = []
    for j in range(count):
        width, kind = WIDTHS[j % 5], KINDS[(j // 5 + j % 5) % 3]
        cols.append((width,) + cells(width, n, kind, salt=j if kind == "random" else 0))
    batch = Batch(ctx, cols, n)
    try:
        ctx.fr_from_uint_batch(batch.src_ptrs(), batch.widths(), n, batch.out_ptrs())
        batch.check()
    finally:
        batch.free()
    if count >= 15:
        assert {(c[0], KINDS[(j // 5 + j % 5) % 3]) for j, c in enumerate(cols)} == {(w, k) for w in WIDTHS for k in KINDS}      # every width with every kind of cell


@pytest.mark.parametrize("n", SIZES)
def test_sixteen_columns_of_bytes(ctx, n):
    cols = [(1,) + cells(1, n, KINDS[j % 3], salt=j) for j in range(16)]
    batch = Batch(ctx, cols, n)
    try:
        ctx.fr_from_uint_batch(batch.src_ptrs(), batch.widths(), n, batch.out_ptrs())
        batch.check()
    finally:
        batch.free()


@pytest.mark.parametrize("width", WIDTHS)
def test_two_entries_read_the_same_source(ctx, width):
    n = 257
    cols = [(width,) + cells(width, n, "random"), (width,) + cells(width, n, "random"), (4,) + cells(4, n, "ones")]
    batch = Batch(ctx, cols, n)
    try:
        src = batch.src_ptrs()
        ctx.fr_from_uint_batch([src[0], src[0], src[2]], batch.widths(), n, batch.out_ptrs())
        batch.check()
    finally:
        batch.free()


def test_the_profiler_books_one_launch_per_sixteen_columns(ctx):
    n, count = 255, 33
    cols = [(WIDTHS[j % 5],) + cells(WIDTHS[j % 5], n, "random") for j in range(count)]
    batch = Batch(ctx, cols, n)
    ctx.prof_enable(True)
    try:
        ctx.prof_reset()
        ctx.fr_from_uint_batch(batch.src_ptrs(), batch.widths(), n, batch.out_ptrs())
        got = batch.download()
        assert ctx.prof_get("fr_from_uint_batch")[1] == 3
        assert ctx.prof_get_bytes("fr_from_uint_batch") == sum(n * (c[0] + 32) for c in cols)
        assert all(np.array_equal(got[j, GUARD:GUARD + n], c[2]) for j, c in enumerate(cols))
    finally:
        ctx.prof_enable(False)
        ctx.prof_reset()
        batch.free()


@pytest.fixture()
def guarded(ctx):
    n = 64
    cols = [(WIDTHS[j % 5],) + cells(WIDTHS[j % 5], n, "random") for j in range(18)]
    batch = Batch(ctx, cols, n)
    yield batch
    batch.free()


@pytest.mark.parametrize("at", [0, 5, 17])
@pytest.mark.parametrize("wrong", [0, 3, 32])
def test_a_bad_width_is_refused_and_nothing_is_written(zk, ctx, guarded, wrong, at):
    widths = guarded.widths()
    widths[at] = wrong
    assert raw_call(zk, ctx, guarded.src_ptrs(), widths, guarded.n, guarded.out_ptrs()) == -1      # ZK_ERR_INVALID_ARG
    assert (guarded.download() == SENTINEL).all()


@pytest.mark.parametrize("which", ["source", "output", "widths", "table"])
def test_a_null_pointer_is_refused_and_nothing_is_written(zk, ctx, guarded, which):
    src, out = guarded.src_ptrs(), guarded.out_ptrs()
    lib = zk.lib()
    if which == "source":
        src[17] = None
        rc = raw_call(zk, ctx, src, guarded.widths(), guarded.n, out)
    elif which == "output":
        out[2] = None
        rc = raw_call(zk, ctx, src, guarded.widths(), guarded.n, out)
    elif which == "widths":
        rc = lib.zk_fr_from_uint_batch(ctx.h, (ctypes.c_void_p * 18)(*src), None, 18, guarded.n, (ctypes.c_void_p * 18)(*out))
    else:
        rc = lib.zk_fr_from_uint_batch(ctx.h, None, (ctypes.c_uint8 * 18)(*guarded.widths()), 18, guarded.n, (ctypes.c_void_p * 18)(*out))
    assert rc == -1
    assert (guarded.download() == SENTINEL).all()


def test_a_misaligned_source_and_overlapping_outputs_are_refused(zk, ctx, guarded):
    src, out = guarded.src_ptrs(), guarded.out_ptrs()
    bad = list(src)
    bad[3] += 4                                                      # 8-byte cells at an address that is 4 mod 8
    assert raw_call(zk, ctx, bad, guarded.widths(), guarded.n, out) == -1
    bad = list(out)
    bad[9] = out[8] + 32                                             # all but one cell of column 8's output
    assert raw_call(zk, ctx, src, guarded.widths(), guarded.n, bad) == -1
    assert (guarded.download() == SENTINEL).all()


def test_no_columns_is_ok(zk, ctx, guarded):
    assert zk.lib().zk_fr_from_uint_batch(ctx.h, None, None, 0, 64, None) == 0
    assert raw_call(zk, ctx, guarded.src_ptrs(), guarded.widths(), guarded.n, guarded.out_ptrs(), count=0) == 0
    assert raw_call(zk, ctx, guarded.src_ptrs(), guarded.widths(), 0, guarded.out_ptrs()) == 0      # no cells
    assert (guarded.download() == SENTINEL).all()

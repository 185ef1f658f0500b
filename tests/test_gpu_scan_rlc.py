"""GPU: ZK_OP_SCAN_RLC / ZK_OP_SCAN_RLC_REV of zk_field_vec_op -- out[i] = m[kind_i] out[i -+ 1] + w[kind_i] cell[i] along one typed
column (1, 2, 4, 8, 16-byte packed cells, 32-byte Montgomery elements) with a one-byte kind column -- bit for bit against the integer
recurrence, a plain Python loop mod r converted by the oracle (cref.to_mont).

The tiling these sizes assume is that of csrc/vec.hip: a thread folds SCAN_PER = 8 consecutive rows, a block SCAN_THREADS = 256 threads
(2048 rows), k_affine_b takes the block maps in windows of 256 (524 288 rows).  Forward byte columns with kinds at every boundary of
that tiling; one size past the window of block maps in both directions; every width at 2049 and 4097 rows in both directions; cell
pointers at base + width k for k = 0 .. 7 with the kinds at odd addresses; kinds 1, 2, 3 at the first and last position of a thread
chunk, of a block and at the last row; kind bytes with their upper six bits set; d_kinds NULL and d_kinds == d_cells; z0 != 0; the
largest operands; equality with ZK_OP_SCAN_AFFINE fed the expanded columns and with zk_fr_prefix_sum under the all-ones table.  Refused
calls write nothing and leave the context usable; ops 5, 6, 7 and 11 stay refused; a call books one fr_scan_rlc scope."""
import ctypes
import functools

import numpy as np
import pytest

from oracle import bn254 as b
from oracle import cref

pytestmark = pytest.mark.gpu
P = b.R_MOD
SCAN_PER, SCAN_THREADS = 8, 256
BLOCK = SCAN_PER * SCAN_THREADS
WINDOW = BLOCK * SCAN_THREADS
SIX = (1, 2, 4, 8, 16, 32)
SENTINEL = 0xA5C3A5C3A5C3A5C3
GUARD = 3                                   # sentinel cells in front of and behind the output
INVALID_ARG = -1
LEAD = 64                                   # bytes in front of the cells and of the kinds inside their buffers


def rnd_fr(seed, count):
    state, out = 0x5CA9 + 7919 * seed, []
    for _ in range(count):
        words = []
        for _ in range(4):
            state, w = b.splitmix64(state)
            words.append(w)
        out.append((words[0] | words[1] << 64 | words[2] << 128 | words[3] << 192) % P)
    return out


def standard_table(seed):
    """step (r, 1), start (0, 1), hold (1, 0), clear (0, 0)"""
    return [(rnd_fr(seed, 1)[0], 1), (0, 1), (1, 0), (0, 0)]


def random_table(seed):
    v = rnd_fr(seed + 1000, 8)
    return [(v[2 * s], v[2 * s + 1]) for s in range(4)]


def mont(vals):
    return cref.to_mont(list(vals)) if len(vals) else np.zeros((0, 4), dtype=np.uint64)


@functools.lru_cache(maxsize=None)
def cells(width: int, n: int, seed: int = 0, ones: bool = False):
    """n plain values of a column and the bytes that hold them on the device: packed little-endian cells, or the oracle's Montgomery
    images for width 32"""
    rng = np.random.default_rng(1000 * width + seed)
    if width < 32:
        raw = np.full(n * width, 0xFF, dtype=np.uint8) if ones else rng.integers(0, 256, n * width, dtype=np.uint8)
        if n > 8 and not ones:                                          # zero and all-ones cells among the random ones
            raw[:width] = 0
            raw[5 * width:6 * width] = 0xFF
        data = raw.tobytes()
        vals = list(data) if width == 1 else [int.from_bytes(data[i * width:(i + 1) * width], "little") for i in range(n)]
    else:
        vals = [P - 1] * n if ones else rnd_fr(seed + 32, n)
        if n > 8 and not ones:
            vals[0], vals[5] = 0, P - 1
        raw = cref.to_mont(vals).view(np.uint8).reshape(-1)
    raw.setflags(write=False)
    return tuple(vals), raw


@functools.lru_cache(maxsize=None)
def kind_bytes(n: int, seed: int = 0):
    """n kind bytes with random upper bits; every kind occurs (step most often, as in the circuits)"""
    rng = np.random.default_rng(77 + seed)
    low = rng.choice(np.array([0, 0, 0, 0, 0, 1, 2, 3], dtype=np.uint8), n)
    k = (low | (rng.integers(0, 64, n, dtype=np.uint8) << 2)).astype(np.uint8)
    k.setflags(write=False)
    return k


def reference(vals, kinds, table, z0, reverse):
    """the integer recurrence: a plain loop mod r"""
    n = len(vals)
    out, z = [0] * n, z0
    for j in range(n):
        i = n - 1 - j if reverse else j
        m, w = table[int(kinds[i]) & 3 if kinds is not None else 0]
        z = (m * z + w * vals[i]) % P
        out[i] = z
    return out


class Column:
    """cells at base + LEAD + width * shift, kinds at an odd address of their own buffer (kind_off), the output inside sentinels"""

    def __init__(self, ctx, width, raw, n, kinds=None, shift=0, kind_off=1):
        self.ctx, self.n, self.width = ctx, n, width
        self.cell_off = LEAD + width * shift
        self.image = np.full(self.cell_off + len(raw) + LEAD, 0xEE, dtype=np.uint8)
        self.image[self.cell_off:self.cell_off + len(raw)] = raw
        self.src = ctx.to_device(self.image)
        self.kind_image, self.kin = None, None
        if kinds is not None:
            self.kind_off = LEAD + kind_off
            self.kind_image = np.full(self.kind_off + n + LEAD, 0xEE, dtype=np.uint8)
            self.kind_image[self.kind_off:self.kind_off + n] = kinds
            self.kin = ctx.to_device(self.kind_image)
        self.sentinels = np.full((n + 2 * GUARD, 4), SENTINEL, dtype=np.uint64)
        self.out = ctx.to_device(self.sentinels)

    @property
    def cells_ptr(self):
        return self.src.ptr + self.cell_off

    @property
    def kinds_ptr(self):
        return None if self.kin is None else self.kin.ptr + self.kind_off

    @property
    def out_ptr(self):
        return self.out.ptr + GUARD * 32

    def run(self, table, z0=0, reverse=False, kinds_ptr="own"):
        self.ctx.scan_rlc(self.cells_ptr, self.width, self.kinds_ptr if kinds_ptr == "own" else kinds_ptr, mont([v for pair in table for v in pair]),
                          self.n, self.out_ptr, z0=mont([z0])[0], reverse=reverse)
        return self.result()

    def result(self):
        """the n outputs, after checking that nothing around them was written"""
        got = self.out.download((self.n + 2 * GUARD, 4))
        assert (got[:GUARD] == SENTINEL).all() and (got[GUARD + self.n:] == SENTINEL).all(), "a cell outside [0, n) was written"
        return got[GUARD:GUARD + self.n]

    def untouched(self):
        ok = (self.out.download((self.n + 2 * GUARD, 4)) == SENTINEL).all() and np.array_equal(self.src.download(self.image.shape, np.uint8), self.image)
        return ok and (self.kin is None or np.array_equal(self.kin.download(self.kind_image.shape, np.uint8), self.kind_image))

    def free(self):
        for buf in (self.src, self.kin, self.out):
            if buf is not None:
                buf.free()


def check(ctx, width, n, table, z0, reverse, kinds="random", shift=0, kind_off=1, seed=0, ones=False):
    vals, raw = cells(width, n, seed, ones)
    k = kind_bytes(n, seed) if isinstance(kinds, str) else kinds
    col = Column(ctx, width, raw, n, k, shift, kind_off)
    try:
        got = col.run(table, z0, reverse)
        want = mont(reference(vals, k, table, z0, reverse))
        assert np.array_equal(got, want)                               # the oracle's images are canonical, so these are
    finally:
        col.free()


# ---- 1. sizes
@pytest.mark.parametrize("n", [1, 2, 7, 8, 9, 255, 256, 257, 2047, 2048, 2049, 4097])
def test_forward_bytes_at_every_boundary_of_the_tiling(ctx, n):
    check(ctx, 1, n, standard_table(n), rnd_fr(n, 1)[0], False, seed=n)


@pytest.mark.parametrize("reverse", [False, True])
def test_one_size_past_the_window_of_block_maps(ctx, reverse):
    assert WINDOW + 1 == 524289
    check(ctx, 1, WINDOW + 1, standard_table(3), rnd_fr(4, 1)[0], reverse, seed=5)


# ---- 2. widths
@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("n", [2049, 4097])
@pytest.mark.parametrize("width", SIX)
def test_every_width_both_directions(ctx, width, n, reverse):
    table = standard_table(width) if n == 2049 else random_table(width)
    check(ctx, width, n, table, rnd_fr(width + n, 1)[0], reverse, seed=width)


# ---- 3. alignment
@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("width", SIX)
def test_cell_pointers_at_every_multiple_of_the_width_and_kinds_at_odd_addresses(ctx, width, reverse):
    for k in range(8):
        for n in (13, 267):                                            # a column inside two words; one that ends inside a word
            check(ctx, width, n, random_table(k), rnd_fr(k, 1)[0], reverse, shift=k, kind_off=2 * ((k + n) % 4) + 1, seed=k)


# ---- 4. kinds
EDGES = (0, SCAN_PER - 1, SCAN_PER, 2 * SCAN_PER - 1, BLOCK - 1, BLOCK, 2 * BLOCK - 1, 2 * BLOCK)


@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("rot", range(3))
@pytest.mark.parametrize("width", [1, 16])
def test_kinds_at_the_edges_of_chunks_and_blocks_and_at_the_last_row(ctx, width, rot, reverse):
    """kinds 1, 2, 3 at the first and last position of a thread chunk and of a block, in scan order, and at the last row; the three
    rotations put every kind at every such position"""
    n = 2 * BLOCK + 1
    kinds = np.zeros(n, dtype=np.uint8)
    for j, pos in enumerate(EDGES):
        kinds[n - 1 - pos if reverse else pos] = 1 + (j + rot) % 3
    assert kinds[n - 1] != 0 and kinds[0] != 0
    check(ctx, width, n, standard_table(rot), rnd_fr(rot, 1)[0], reverse, kinds=kinds, seed=rot)


@pytest.mark.parametrize("reverse", [False, True])
def test_only_the_low_two_bits_of_a_kind_byte_count(ctx, reverse):
    n = 2049
    vals, raw = cells(2, n, 1)
    high = kind_bytes(n, 9)
    assert (high >> 2).any() and set((high & 3).tolist()) == {0, 1, 2, 3}
    table, z0 = random_table(2), rnd_fr(2, 1)[0]
    a, c = Column(ctx, 2, raw, n, high), Column(ctx, 2, raw, n, high & 3)
    try:
        got = a.run(table, z0, reverse)
        assert np.array_equal(got, c.run(table, z0, reverse))
        assert np.array_equal(got, mont(reference(vals, high & 3, table, z0, reverse)))
    finally:
        a.free()
        c.free()


@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("width", [1, 8])
def test_null_kinds_are_an_all_zero_kind_column(ctx, width, reverse):
    n = 2049
    vals, raw = cells(width, n, 3)
    table, z0 = random_table(3), rnd_fr(3, 1)[0]
    a, c = Column(ctx, width, raw, n, None), Column(ctx, width, raw, n, np.zeros(n, dtype=np.uint8))
    try:
        got = a.run(table, z0, reverse)
        assert np.array_equal(got, c.run(table, z0, reverse))
        assert np.array_equal(got, mont(reference(vals, None, table, z0, reverse)))          # the plain Horner running RLC
    finally:
        a.free()
        c.free()


@pytest.mark.parametrize("reverse", [False, True])
def test_the_kinds_may_be_the_cells(ctx, reverse):
    n = 2049
    vals, raw = cells(1, n, 4)
    table, z0 = standard_table(4), rnd_fr(5, 1)[0]
    col = Column(ctx, 1, raw, n, None, shift=3)
    try:
        got = col.run(table, z0, reverse, kinds_ptr=col.cells_ptr)
        assert np.array_equal(got, mont(reference(vals, raw, table, z0, reverse)))
    finally:
        col.free()


# ---- 5. the largest operands
@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("width", [16, 32])
def test_all_ones_cells_with_m_w_z0_at_p_minus_1(ctx, width, reverse):
    check(ctx, width, 2049, [(P - 1, P - 1)] * 4, P - 1, reverse, ones=True)


# ---- 6. cross-checks on the device
@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("width", [1, 16])
def test_equals_the_affine_scan_of_the_expanded_columns(zk, ctx, width, reverse):
    n = 4097
    vals, raw = cells(width, n, 6)
    kinds, table, z0 = kind_bytes(n, 6), random_table(6), rnd_fr(6, 1)[0]
    a = [table[int(k) & 3][0] for k in kinds]
    bb = [table[int(k) & 3][1] * v % P for k, v in zip(kinds, vals)]
    first = n - 1 if reverse else 0
    bb[first] = (bb[first] + a[first] * z0) % P                        # the affine scan starts from 0: the caller folds a z0 into b
    col = Column(ctx, width, raw, n, kinds)
    d_a, d_b, d_o = ctx.to_device(mont(a)), ctx.to_device(mont(bb)), ctx.alloc(n * 32)
    try:
        ctx.scan_affine(d_a, d_b, d_o, n, reverse=reverse)
        assert np.array_equal(col.run(table, z0, reverse), d_o.download((n, 4)))
    finally:
        for buf in (d_a, d_b, d_o):
            buf.free()
        col.free()


@pytest.mark.parametrize("width", [1, 4])
def test_the_all_ones_table_is_the_prefix_sum_of_the_expanded_cells(ctx, width):
    n = 2049
    vals, raw = cells(width, n, 7)
    col = Column(ctx, width, raw, n, kind_bytes(n, 7))
    d_x, d_z = ctx.to_device(np.zeros((n + 1, 4), dtype=np.uint64)), ctx.alloc((n + 1) * 32)
    try:
        ctx.fr_from_uint(col.src, width, n, d_x, offset_bytes=col.cell_off)
        ctx.fr_prefix_sum(d_x, d_z, n + 1)                             # z[0] = 0, z[i + 1] = z[i] + x[i]
        assert np.array_equal(col.run([(1, 1)] * 4), d_z.download((n + 1, 4))[1:])
    finally:
        d_x.free()
        d_z.free()
        col.free()


# ---- 7. refusals
def raw_call(zk, ctx, cells_ptr, width, kinds_ptr, hk, n, out_ptr, field=0, op=9):
    desc = zk.binding._ScanRlc(cells_ptr, width, kinds_ptr)
    return zk.lib().zk_field_vec_op(ctx.h, ctypes.c_int(field), ctypes.c_int(op), ctypes.byref(desc), hk.ctypes.data_as(ctypes.c_void_p), ctypes.c_void_p(out_ptr), ctypes.c_size_t(n))


@pytest.mark.parametrize("width", [1, 2, 4, 8, 16, 32])
def test_refused_calls_write_nothing_and_leave_the_context_usable(zk, ctx, width):
    """EACH refusal is followed by its own checks: the guarded output and the inputs are untouched, and the next valid call works
    (after which the sentinels are put back for the next refusal)"""
    n = 300
    vals, raw = cells(width, n, 8)
    kinds, table, z0 = kind_bytes(n, 8), standard_table(8), rnd_fr(8, 1)[0]
    col = Column(ctx, width, raw, n, kinds)
    hk = np.ascontiguousarray(mont([z0] + [v for pair in table for v in pair]))
    want = mont(reference(vals, kinds, table, z0, False))
    cp, kp, out = col.cells_ptr, col.kinds_ptr, col.out_ptr
    call = lambda c=cp, w=width, k=kp, o=out, rows=n, **kw: raw_call(zk, ctx, c, w, k, hk, rows, o, **kw)
    refusals = []

    def refused(what, **kw):
        assert call(**kw) == INVALID_ARG, what
        ctx.sync()
        assert col.untouched(), what
        assert call() == 0, what                                       # the next valid call
        assert np.array_equal(col.result(), want), what
        col.out.upload(col.sentinels)
        refusals.append(what)
    try:
        refused("Fq", field=zk.FIELD_FQ)
        refused("Fq, reversed", field=zk.FIELD_FQ, op=10)
        for wrong in (0, 3, 5, 24, 33, 64):
            refused(f"width {wrong}", w=wrong)
        refused("NULL cells", c=None)
        if width > 1:
            refused("cells at a misaligned address", c=cp + (4 if width == 32 else width // 2))
        refused("the cells start inside the output", c=out + 32)
        refused("the output starts inside the last cells", o=cp + (n * width - 1) // 32 * 32)
        refused("the kinds start inside the output", k=out + 7)
        refused("the output starts at or just below the last kind byte", o=(kp + n - 1) // 32 * 32)
        for op in (5, 6, 7, 11):
            refused(f"op {op}", op=op)
            refused(f"op {op} over Fq", op=op, field=zk.FIELD_FQ)
        refused("a bad width with n = 0", w=3, rows=0)
        refused("NULL cells with n = 0", c=None, rows=0)
        assert len(refusals) == (23 if width == 1 else 24)
        assert call(rows=0) == 0                                       # n = 0: ZK_OK, nothing written
        assert call(c=out + 32, rows=0) == 0 and call(k=out, rows=0) == 0          # nothing to overlap
        ctx.sync()
        assert col.untouched()
    finally:
        col.free()


# ---- 8. profiling
@pytest.mark.parametrize("with_kinds", [True, False])
@pytest.mark.parametrize("width,n", [(1, 2049), (16, 255)])
def test_a_call_books_one_scope_with_its_bytes(ctx, width, n, with_kinds):
    vals, raw = cells(width, n, 9)
    kinds = kind_bytes(n, 9) if with_kinds else None
    col = Column(ctx, width, raw, n, kinds)
    table = standard_table(9)
    ctx.sync()
    ctx.prof_reset()
    ctx.prof_enable(True)
    try:
        got = col.run(table, 5, True)
        assert np.array_equal(got, mont(reference(vals, kinds, table, 5, True)))
        ms, calls = ctx.prof_get("fr_scan_rlc")
        assert calls == 1 and ms > 0                                   # one scope, whether the call is one launch or three
        assert ctx.prof_get_bytes("fr_scan_rlc") == n * (width + (1 if with_kinds else 0) + 32)
    finally:
        ctx.prof_enable(False)
        ctx.prof_reset()
        col.free()

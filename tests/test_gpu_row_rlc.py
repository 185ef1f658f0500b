"""GPU: ZK_OP_ROW_RLC of zk_field_vec_op -- out[i] = c + sum_j w_j cell_j[i] across typed columns (1, 2, 4, 8, 16-byte packed cells and
32-byte Montgomery elements) -- bit for bit against Python integers converted by the oracle (cref.to_mont), and against the composition
the library offered before (zk_fr_from_uint_batch, zk_fr_scale, ZK_OP_ADD) on the same device bytes.  Row counts below a sweep, at and
around one wave's 256 rows and a ragged tail; column counts of the empty table, one launch, its edge (63, 64), and chained launches
(65, 129: the sum so far is read back from the output); three shapes of table (all bytes; the six widths interleaved; the eleven
columns of RwRow::rlc with the constant r^11 and descending powers); zero, all-ones and random cells; weights that are powers of a
random r, all p - 1, and some zero.  The columns of a case lie in ONE source buffer, bytes and halfwords one cell past a 16-byte
boundary (a partial first packed word, a different one per width), the output inside sentinels.  The output may be a 32-byte column;
columns may share a source; refused calls write nothing and leave the context usable; op values 5, 6 and 7 stay refused."""
import ctypes
import functools

import numpy as np
import pytest

from oracle import bn254 as b
from oracle import cref

pytestmark = pytest.mark.gpu
P = b.R_MOD
SIZES = (1, 63, 64, 255, 256, 257, 1021)
COUNTS = (0, 1, 2, 16, 17, 63, 64, 65, 129)
KINDS = ("zero", "ones", "random")
WEIGHTS = ("powers", "pm1", "somezero")
SIX = (1, 2, 4, 8, 16, 32)
RW_ROW = (8, 1, 1, 4, 16, 1, 32, 32, 32, 16, 16)
RR_BATCH = 64
SENTINEL = 0xA5C3A5C3A5C3A5C3
GUARD = 3                                   # sentinel cells in front of and behind the output
INVALID_ARG = -1


@functools.lru_cache(maxsize=None)
def cells(width: int, n: int, kind: str, salt: int = 0):
    """n plain values of a column (below 2^(8 width), below p for width 32) and the bytes that hold them on the device: packed
    little-endian cells, or the oracle's Montgomery images for width 32"""
    top = (1 << (8 * width)) - 1 if width < 32 else P - 1
    if kind == "zero":
        vals = [0] * n
    elif kind == "ones":
        vals = [top] * n
    else:
        vals, state = [], 0x7E57 + 131 * width + salt
        while len(vals) < n:
            words = []
            for _ in range(4):
                state, w = b.splitmix64(state)
                words.append(w)
            v = words[0] | words[1] << 64 | words[2] << 128 | words[3] << 192
            vals.append(v & top if width < 32 else v % P)
    if width < 32:
        raw = np.frombuffer(b"".join(v.to_bytes(width, "little") for v in vals), dtype=np.uint8)
    else:
        raw = cref.to_mont(vals).view(np.uint8).reshape(-1)
    raw.setflags(write=False)
    return tuple(vals), raw


def weights(kind: str, count: int, salt: int = 0):
    """(constant, [w_j]) as plain integers"""
    state = 0xC0FFEE + salt
    rnd = []
    for _ in range(count + 2):
        words = []
        for _ in range(4):
            state, w = b.splitmix64(state)
            words.append(w)
        rnd.append((words[0] | words[1] << 64 | words[2] << 128 | words[3] << 192) % P)
    if kind == "powers":
        r = rnd[0]
        return rnd[1], [pow(r, j, P) for j in range(count)]
    if kind == "pm1":
        return P - 1, [P - 1] * count
    return 0, [0 if j % 3 == 1 else rnd[j + 2] for j in range(count)]


def mont(vals):
    return cref.to_mont(list(vals)) if len(vals) else np.zeros((0, 4), dtype=np.uint64)


class Table:
    """the columns of one call laid out in ONE source buffer (each at a 16-byte boundary, bytes and halfwords one cell past it) and
    an output buffer of n elements inside GUARD sentinel cells"""

    def __init__(self, ctx, columns, n):
        self.ctx, self.n, self.columns = ctx, n, columns            # columns: [(width, values, device bytes)]
        self.src_off, pos, chunks = [], 0, []
        for width, _, raw in columns:
            lead = width if width < 4 else 0
            size = (lead + len(raw) + 15) // 16 * 16
            chunk = np.full(size, 0xEE, dtype=np.uint8)
            chunk[lead:lead + len(raw)] = raw
            chunks.append(chunk)
            self.src_off.append(pos + lead)
            pos += size
        self.image = np.concatenate(chunks) if chunks else np.zeros(16, dtype=np.uint8)
        self.src = ctx.to_device(self.image)
        self.out = ctx.to_device(np.full((n + 2 * GUARD, 4), SENTINEL, dtype=np.uint64))

    def ptrs(self):
        return [self.src.ptr + o for o in self.src_off]

    def widths(self):
        return [c[0] for c in self.columns]

    @property
    def out_ptr(self):
        return self.out.ptr + GUARD * 32

    def want(self, const, ws):
        rows = [(const + sum(w * col[1][i] for w, col in zip(ws, self.columns) if w)) % P for i in range(self.n)]
        return mont(rows)

    def result(self):
        """the n outputs, after checking that nothing around them was written"""
        got = self.out.download((self.n + 2 * GUARD, 4))
        assert (got[:GUARD] == SENTINEL).all() and (got[GUARD + self.n:] == SENTINEL).all(), "a cell outside [0, n) was written"
        return got[GUARD:GUARD + self.n]

    def untouched(self):
        return (self.out.download((self.n + 2 * GUARD, 4)) == SENTINEL).all() and np.array_equal(self.src.download(self.image.shape, np.uint8), self.image)

    def free(self):
        self.src.free()
        self.out.free()


def table_of(ctx, widths, n, first_kind=0):
    cols = []
    for j, width in enumerate(widths):
        kind = KINDS[(first_kind + j // len(SIX) + j) % 3]
        cols.append((width,) + cells(width, n, kind, salt=j if kind == "random" else 0))
    return Table(ctx, cols, n)


def run_and_check(ctx, table, const, ws):
    ctx.row_rlc(table.ptrs(), table.widths(), mont(ws), table.n, table.out_ptr, constant=mont([const])[0])
    assert np.array_equal(table.result(), table.want(const, ws))


# ---- 1. against Python integers
@pytest.mark.parametrize("wkind", WEIGHTS)
@pytest.mark.parametrize("shape", ["bytes", "six"])
@pytest.mark.parametrize("count", COUNTS)
@pytest.mark.parametrize("n", SIZES)
def test_equals_python_integers(ctx, n, count, shape, wkind):
    widths = [1] * count if shape == "bytes" else [SIX[j % 6] for j in range(count)]
    table = table_of(ctx, widths, n, first_kind=SIZES.index(n) + WEIGHTS.index(wkind))
    try:
        run_and_check(ctx, table, *weights(wkind, count, salt=n + count))
    finally:
        table.free()


def test_every_width_meets_every_kind_of_cell():
    """the rotation of table_of: with 18 columns or more the six-width shape has every (width, kind) pair in one table"""
    seen = {(SIX[j % 6], KINDS[(j // 6 + j) % 3]) for j in range(63)}
    assert seen == {(w, k) for w in SIX for k in KINDS}


@pytest.mark.parametrize("ckind", range(3))
@pytest.mark.parametrize("n", SIZES)
def test_rw_row_shape(ctx, n, ckind):
    """RwRow::rlc: eleven mixed-width values under a leading one, descending powers: r^11 + v_0 r^10 + ... + v_10"""
    table = table_of(ctx, RW_ROW, n, first_kind=ckind)
    r = weights("powers", 0, salt=n)[0]
    try:
        run_and_check(ctx, table, pow(r, 11, P), [pow(r, 10 - j, P) for j in range(11)])
    finally:
        table.free()


# ---- 2. against the composition on the same device bytes
@pytest.mark.parametrize("n", [255, 1021])
def test_equals_the_composition(zk, ctx, n):
    widths = [SIX[j % 5] for j in range(20)]                       # the narrow widths: what zk_fr_from_uint_batch expands
    table = table_of(ctx, widths, n)
    const, ws = weights("powers", len(widths), salt=n)
    ones = ctx.to_device(np.ones(n, dtype=np.uint8))
    expanded = [ctx.alloc(n * 32) for _ in widths]
    acc = ctx.alloc(n * 32)
    try:
        ctx.fr_from_uint(ones, 1, n, acc)
        ctx.fr_scale(acc, mont([const])[0], n)                     # the constant column
        ctx.fr_from_uint_batch(table.ptrs(), widths, n, expanded)
        for buf, w in zip(expanded, mont(ws)):
            ctx.fr_scale(buf, np.ascontiguousarray(w), n)
            ctx.field_vec_op(zk.FIELD_FR, zk.OP_ADD, acc, buf, acc, n)
        ctx.row_rlc(table.ptrs(), widths, mont(ws), n, table.out_ptr, constant=mont([const])[0])
        assert np.array_equal(table.result(), acc.download((n, 4)))
    finally:
        for buf in expanded + [acc, ones]:
            buf.free()
        table.free()


# ---- 3. the output as a 32-byte column, shared sources
@pytest.mark.parametrize("count", [3, 64, 70])
@pytest.mark.parametrize("n", [64, 257])
def test_the_output_may_be_a_32_byte_column(ctx, n, count):
    """an earlier word RLC continued in place: column 1 of the table IS the output buffer (in the chained case the first launch reads
    and overwrites it, the later launches read the sum so far from the same place)"""
    widths = [SIX[j % 6] for j in range(count)]
    widths[1] = 32
    table = table_of(ctx, widths, n)
    const, ws = weights("powers", count, salt=n)
    try:
        prev = cells(32, n, "random", salt=99)
        table.columns[1] = (32,) + prev
        guarded = np.full((n + 2 * GUARD, 4), SENTINEL, dtype=np.uint64)
        guarded[GUARD:GUARD + n] = np.frombuffer(prev[1].tobytes(), dtype=np.uint64).reshape(n, 4)
        table.out.upload(guarded)
        ptrs = table.ptrs()
        ptrs[1] = table.out_ptr
        ctx.row_rlc(ptrs, widths, mont(ws), n, table.out_ptr, constant=mont([const])[0])
        assert np.array_equal(table.result(), table.want(const, ws))
    finally:
        table.free()


@pytest.mark.parametrize("where", ["last", "at_64", "several"])
@pytest.mark.parametrize("count", [65, 129])
def test_the_output_as_a_column_past_the_first_launch(ctx, count, where):
    """the first launch overwrites the output, so a column that IS the output has to be read by it wherever it stands in the table:
    the last column, the first one past a full launch (index 64), and several places at once (their weights add up), some past 64"""
    n = 257
    at = {"last": [count - 1], "at_64": [64], "several": [0, 63, 64, count - 1]}[where]
    widths = [SIX[j % 6] for j in range(count)]
    for j in at:
        widths[j] = 32
    table = table_of(ctx, widths, n)
    const, ws = weights("powers", count, salt=count + len(at))
    try:
        prev = cells(32, n, "random", salt=77)
        guarded = np.full((n + 2 * GUARD, 4), SENTINEL, dtype=np.uint64)
        guarded[GUARD:GUARD + n] = np.frombuffer(prev[1].tobytes(), dtype=np.uint64).reshape(n, 4)
        table.out.upload(guarded)
        ptrs = table.ptrs()
        for j in at:
            table.columns[j] = (32,) + prev
            ptrs[j] = table.out_ptr
        ctx.row_rlc(ptrs, widths, mont(ws), n, table.out_ptr, constant=mont([const])[0])
        assert np.array_equal(table.result(), table.want(const, ws))
    finally:
        table.free()


@pytest.mark.parametrize("width", SIX)
def test_columns_may_share_a_source(ctx, width):
    n = 257
    table = table_of(ctx, [width, 4, width, width], n, first_kind=2)
    const, ws = weights("powers", 4, salt=width)
    try:
        src = table.ptrs()
        table.columns[2] = table.columns[3] = table.columns[0]
        ctx.row_rlc([src[0], src[1], src[0], src[0]], table.widths(), mont(ws), n, table.out_ptr, constant=mont([const])[0])
        assert np.array_equal(table.result(), table.want(const, ws))
    finally:
        table.free()


# ---- 4. refusals
def raw_call(zk, ctx, ptrs, widths, weights_mont, n, out_ptr, field=0, op=8, count=None, null=None):
    cnt = len(ptrs) if count is None else count
    pp = (ctypes.c_void_p * max(len(ptrs), 1))(*ptrs)
    wd = (ctypes.c_uint8 * max(len(widths), 1))(*widths)
    desc = zk.binding._RowRlc(cnt, None if null == "cols" else ctypes.cast(pp, ctypes.POINTER(ctypes.c_void_p)),
                              None if null == "widths" else ctypes.cast(wd, ctypes.POINTER(ctypes.c_uint8)))
    hk = np.ascontiguousarray(weights_mont)
    return zk.lib().zk_field_vec_op(ctx.h, ctypes.c_int(field), ctypes.c_int(op), ctypes.byref(desc), hk.ctypes.data_as(ctypes.c_void_p), ctypes.c_void_p(out_ptr), ctypes.c_size_t(n))


@pytest.fixture()
def guarded(ctx):
    table = table_of(ctx, [SIX[j % 6] for j in range(18)], 64)
    yield table
    table.free()


def test_refused_calls_write_nothing_and_leave_the_context_usable(zk, ctx, guarded):
    """EACH refusal is followed by its own checks: the guarded output and the inputs are untouched, and the next valid call works
    (after which the sentinels are put back for the next refusal)"""
    t, n = guarded, guarded.n
    const, ws = weights("powers", 18, salt=5)
    hk = mont([const] + ws)
    want = t.want(const, ws)
    sentinels = np.full((n + 2 * GUARD, 4), SENTINEL, dtype=np.uint64)
    ptrs, widths, out = t.ptrs(), t.widths(), t.out_ptr
    call = lambda p=ptrs, w=widths, o=out, rows=n, **kw: raw_call(zk, ctx, p, w, hk, rows, o, **kw)
    refusals = []

    def refused(what, **kw):
        assert call(**kw) == INVALID_ARG, what
        ctx.sync()
        assert t.untouched(), what
        assert call() == 0, what                                       # the next valid call
        assert np.array_equal(t.result(), want), what
        t.out.upload(sentinels)
        refusals.append(what)

    def changed(seq, at, value):
        seq = list(seq)
        seq[at] = value
        return seq
    refused("Fq", field=zk.FIELD_FQ)
    for wrong in (0, 3, 5, 24, 33, 64):
        for at in (0, 17):
            refused(f"width {wrong} at {at}", w=changed(widths, at, wrong))
    refused("a NULL column", p=changed(ptrs, 4, None))
    refused("8-byte cells at an address that is 4 mod 8", p=changed(ptrs, 3, ptrs[3] + 4))
    refused("halfwords at an odd address", p=changed(ptrs, 1, ptrs[1] + 1))
    refused("field elements at an address that is 4 mod 8", p=changed(ptrs, 5, ptrs[5] + 4))
    refused("a byte column inside the output", p=changed(ptrs, 0, out + 7))
    refused("a 16-byte column AT the output", p=changed(ptrs, 4, out))
    refused("a 32-byte column one element into the output", p=changed(ptrs, 5, out + 32))
    refused("a 32-byte column one element in front of the output", p=changed(ptrs, 5, out - 32))
    refused("the output inside a 32-byte column", o=ptrs[5] + 8)
    refused("NULL d_cols", null="cols")
    refused("NULL widths", null="widths")
    for op in (5, 6, 7):
        refused(f"op {op}", op=op)
        refused(f"op {op} over Fq", op=op, field=zk.FIELD_FQ)
    refused("a bad width with n = 0", w=changed(widths, 2, 3), rows=0)
    assert len(refusals) == 31
    assert call(rows=0) == 0                                                                            # n = 0: ZK_OK, nothing written
    assert call(p=changed(ptrs, 4, out), rows=0) == 0                                                   # nothing to overlap
    ctx.sync()
    assert t.untouched()


def test_the_empty_table_gives_the_constant_column(zk, ctx, guarded):
    const = weights("powers", 0, salt=3)[0]
    assert raw_call(zk, ctx, [], [], mont([const]), guarded.n, guarded.out_ptr, null="cols") == 0       # count = 0: the arrays are not looked at
    assert np.array_equal(guarded.result(), mont([const] * guarded.n))
    ctx.row_rlc([], [], None, guarded.n, guarded.out_ptr)                                               # constant defaults to zero
    assert not guarded.result().any()


# ---- 5. profiling
@pytest.mark.parametrize("count", [17, 64, 65])
def test_each_launch_books_one_scope_with_its_bytes(ctx, count):
    n = 255
    table = table_of(ctx, [SIX[j % 6] for j in range(count)], n)
    const, ws = weights("powers", count, salt=1)
    ctx.sync()
    ctx.prof_reset()
    ctx.prof_enable(True)
    try:
        run_and_check(ctx, table, const, ws)
        ms, launches = ctx.prof_get("fr_row_rlc")
        widths = table.widths()
        if count <= RR_BATCH:
            assert launches == 1 and ms > 0
            assert ctx.prof_get_bytes("fr_row_rlc") == n * (sum(widths) + 32)
        else:                                                      # the second launch reads the sum so far as a 32-byte column
            assert launches == 2
            assert ctx.prof_get_bytes("fr_row_rlc") == n * (sum(widths[:RR_BATCH]) + 32) + n * (32 + sum(widths[RR_BATCH:]) + 32)
    finally:
        ctx.prof_enable(False)
        ctx.prof_reset()
        table.free()

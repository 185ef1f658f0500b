"""GPU: ZK_OP_ROW_INV0 of zk_field_vec_op -- out[i] = num[i] * inv0(c + sum_j w_j cell_j[i]), inv0(0) = 0 -- across typed columns (1, 2,
4, 8, 16-byte packed cells and 32-byte Montgomery elements), bit for bit against Python integers (pow(x, -1, r)) converted by the
oracle (cref.to_mont), and against the composition it replaces (ZK_OP_ROW_RLC, zk_fr_batch_invert, ZK_OP_MUL) on the same device
bytes.  Row counts around a sweep (64), a tile (256) and a wave's inversion (1024); every width at every start the loaders allow;
zero denominators at the places where the wave's products are put together, and zeros that arise only modulo r (the reduced sum is
then the integer r, not 0); column counts across the chained launches; every kind of numerator; the output as a denominator column
and as the numerator; every refusal; the booked bytes."""
import ctypes
import random

import numpy as np
import pytest

from oracle import bn254 as b
from oracle import cref

pytestmark = pytest.mark.gpu
P = b.R_MOD
SIX = (1, 2, 4, 8, 16, 32)
RR_BATCH = 64
SENTINEL = 0xA5C3A5C3A5C3A5C3
GUARD = 3                                   # sentinel cells in front of and behind the output
INVALID_ARG = -1


def mont(vals):
    return cref.to_mont(list(vals)) if len(vals) else np.zeros((0, 4), dtype=np.uint64)


def inv0(x):
    return pow(x, -1, P) if x % P else 0


def top(width):
    return (1 << (8 * width)) - 1 if width < 32 else P - 1


def random_values(rng, width, n):
    """n plain values of a column: zero, the largest and random ones"""
    return [rng.choice([0, top(width), rng.randrange(top(width) + 1), rng.randrange(top(width) + 1)]) for _ in range(n)]


def device_bytes(width, vals):
    """packed little-endian cells, or the oracle's Montgomery images for width 32"""
    if width < 32:
        return np.frombuffer(b"".join(v.to_bytes(width, "little") for v in vals), dtype=np.uint8)
    return mont(vals).view(np.uint8).reshape(-1)


class Call:
    """the columns of one call (and its numerator) in ONE source buffer, column j at a 16-byte boundary plus shifts[j] bytes, between
    0xEE filler; the output of n elements inside GUARD sentinel cells"""

    def __init__(self, ctx, cols, n, shifts=None, num=None, num_shift=0):
        self.ctx, self.n, self.cols, self.num = ctx, n, list(cols), num            # cols: [(width, values)], num: (width, values) or None
        shifts = list(shifts or [0] * len(cols))
        placed = list(zip(self.cols, shifts)) + ([(num, num_shift)] if num else [])
        offs, pos, chunks = [], 0, []
        for (width, vals), shift in placed:
            raw = device_bytes(width, vals)
            size = (shift + len(raw) + 15) // 16 * 16 + 16
            chunk = np.full(size, 0xEE, dtype=np.uint8)
            chunk[shift:shift + len(raw)] = raw
            chunks.append(chunk)
            offs.append(pos + shift)
            pos += size
        self.image = np.concatenate(chunks) if chunks else np.full(16, 0xEE, dtype=np.uint8)
        self.src = ctx.to_device(self.image)
        self.ptrs = [self.src.ptr + o for o in offs[:len(self.cols)]]
        self.num_ptr = self.src.ptr + offs[-1] if num else None
        self.out = ctx.to_device(np.full((n + 2 * GUARD, 4), SENTINEL, dtype=np.uint64))

    @property
    def widths(self):
        return [c[0] for c in self.cols]

    @property
    def out_ptr(self):
        return self.out.ptr + GUARD * 32

    def put_in_output(self, vals):
        """the output buffer holds this 32-byte column (for a call whose output IS one of its columns)"""
        guarded = np.full((self.n + 2 * GUARD, 4), SENTINEL, dtype=np.uint64)
        guarded[GUARD:GUARD + self.n] = mont(vals)
        self.out.upload(guarded)

    def want(self, const, ws):
        rows = []
        for i in range(self.n):
            den = (const + sum(w * col[1][i] for w, col in zip(ws, self.cols) if w)) % P
            rows.append((self.num[1][i] if self.num else 1) * inv0(den) % P)
        return rows

    def run(self, const, ws, ptrs=None, num_ptr=None):
        kw = {}
        if self.num:
            kw = {"num": num_ptr or self.num_ptr, "num_width": self.num[0]}
        self.ctx.row_inv0(ptrs or self.ptrs, self.widths, mont(ws), self.n, self.out_ptr, constant=mont([const])[0], **kw)

    def result(self):
        """the n outputs, after checking that nothing around them was written"""
        got = self.out.download((self.n + 2 * GUARD, 4))
        assert (got[:GUARD] == SENTINEL).all() and (got[GUARD + self.n:] == SENTINEL).all(), "a cell outside [0, n) was written"
        return got[GUARD:GUARD + self.n]

    def check(self, const, ws, **kw):
        self.run(const, ws, **kw)
        want = self.want(const, ws)
        assert np.array_equal(self.result(), mont(want))
        return want

    def untouched(self):
        return (self.out.download((self.n + 2 * GUARD, 4)) == SENTINEL).all() and np.array_equal(self.src.download(self.image.shape, np.uint8), self.image)

    def free(self):
        self.src.free()
        self.out.free()


# ---- 1. row counts around the tiling: a sweep is 64 rows, a tile 256, a wave's inversion 1024
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2049])
def test_row_counts_around_the_tiling(ctx, n):
    rng = random.Random(n)
    call = Call(ctx, [(1, [rng.choice([0, 1, 255, rng.randrange(256)]) for _ in range(n)])], n)
    try:
        want = call.check(0, [1])
        assert n < 8 or (0 in want and any(want))
    finally:
        call.free()


# ---- 2. every width as a lone denominator, at every start its loader allows
@pytest.mark.parametrize("width", SIX)
def test_every_width_at_every_start(ctx, width):
    n = 257
    rng = random.Random(width)
    vals = random_values(rng, width, n)
    shifts = range(0, 8, width) if width < 8 else (0, 8) if width == 8 else (0,) if width == 16 else (0, 8, 16, 24)
    w = rng.randrange(1, P)
    for shift in shifts:
        call = Call(ctx, [(width, vals)], n, shifts=[shift])
        try:
            call.check(0, [w])
        finally:
            call.free()


# ---- 3. zero rows where the wave's products are put together
ZERO_PLACES = {
    "row 0": lambda n: {0},
    "lane 63 of sweep 0": lambda n: {63},
    "the last row": lambda n: {n - 1},
    "a whole tile": lambda n: set(range(256, 512)),
    "a whole wave": lambda n: set(range(1024)),
    "every row": lambda n: set(range(n)),
    "every row but one": lambda n: set(range(n)) - {300},
    "every row of a lane": lambda n: set(range(5, 1024, 64)),
    "every row of a lane in one tile": lambda n: {517, 581, 645, 709},
}


@pytest.mark.parametrize("where", sorted(ZERO_PLACES))
def test_zero_rows(ctx, where):
    n = 1025
    rng = random.Random(len(where))
    zeros = ZERO_PLACES[where](n)
    vals = [0 if i in zeros else rng.randrange(1, 1 << 64) for i in range(n)]
    call = Call(ctx, [(8, vals)], n)
    try:
        want = call.check(0, [1])
        assert {i for i, v in enumerate(want) if v == 0} == zeros
    finally:
        call.free()


# ---- 4. zeros that arise only modulo r: the reduced sum is the integer r there
def test_a_difference_of_equal_cells_is_zero(ctx):
    n = 257
    rng = random.Random(4)
    a = [rng.randrange(1 << 64) for _ in range(n)]
    bb = [a[i] if i % 3 == 0 or i in (63, 256) else rng.randrange(1 << 64) for i in range(n)]
    call = Call(ctx, [(8, a), (8, bb)], n)
    try:
        want = call.check(0, [1, P - 1])
        assert sum(v == 0 for v in want) >= n // 3 and any(want)
    finally:
        call.free()


def test_a_cell_against_a_constant_is_zero(ctx):
    n = 257
    rng = random.Random(5)
    k = rng.randrange(1, 1 << 16)
    cells_ = [k if i % 4 == 1 else rng.randrange(1 << 16) for i in range(n)]
    call = Call(ctx, [(2, cells_)], n)
    try:
        want = call.check(P - k, [1])                                  # c = r - cell in every fourth row
        assert all(want[i] == 0 for i in range(1, n, 4)) and any(want)
    finally:
        call.free()


def test_an_element_against_its_own_negative_is_zero(ctx):
    n = 257
    rng = random.Random(6)
    v = [rng.randrange(1, P) for _ in range(n)]
    neg = [(P - v[i]) if i % 2 else rng.randrange(P) for i in range(n)]
    call = Call(ctx, [(32, v), (32, neg)], n)
    try:
        want = call.check(0, [1, 1])
        assert all(want[i] == 0 for i in range(1, n, 2)) and any(want)
    finally:
        call.free()


# ---- 5. column counts: the empty table, one launch, its edge, chained launches (only the last one inverts)
def launches_of(count):
    return 1 if count <= RR_BATCH else 1 + -(-(count - RR_BATCH) // (RR_BATCH - 1))


@pytest.mark.parametrize("count", [0, 1, 2, 63, 64, 65, 130])
def test_column_counts(ctx, count):
    n = 257
    rng = random.Random(count)
    cols = [(SIX[j % 6], random_values(rng, SIX[j % 6], n)) for j in range(count)]
    ws = [rng.choice([1, P - 1, rng.randrange(P)]) for _ in range(count)]
    call = Call(ctx, cols, n, shifts=[(j % 3) * c[0] if c[0] < 4 else 0 for j, c in enumerate(cols)])
    ctx.sync()
    ctx.prof_reset()
    ctx.prof_enable(True)
    try:
        call.check(rng.randrange(1, P), ws)
        assert ctx.prof_get("fr_row_inv0")[1] == launches_of(count)
        assert ctx.prof_get("fr_row_rlc")[1] == 0                      # the earlier launches run the row RLC's kernel under this op's name
    finally:
        ctx.prof_enable(False)
        ctx.prof_reset()
        call.free()
    assert [launches_of(c) for c in (64, 65, 127, 128, 130)] == [1, 2, 2, 3, 3]


def test_the_empty_table_inverts_the_constant(ctx):
    n = 65
    call = Call(ctx, [], n, num=(4, list(range(n))))
    try:
        call.check(7, [])
        call.check(0, [])                                              # inv0(0): the zero column
        assert not call.result().any()
    finally:
        call.free()


# ---- 6. numerators
@pytest.mark.parametrize("num_width", [None, 1, 2, 4, 8, 16, 32])
def test_numerators(ctx, num_width):
    n = 1300                                                           # every tile of a wave's 1024 rows, and a second wave
    rng = random.Random(num_width or 0)
    den = [0 if i % 5 == 2 else rng.randrange(1, 1 << 32) for i in range(n)]
    num = None
    if num_width:
        vals = [0 if i % 7 == 3 else max(1, v) for i, v in enumerate(random_values(rng, num_width, n))]
        num = (num_width, vals)
    for num_shift in ((0, num_width, 3 * num_width) if num_width in (1, 2) else (0,)):       # a numerator's packed words start anywhere too
        call = Call(ctx, [(4, den)], n, num=num, num_shift=num_shift)
        try:
            want = call.check(0, [1])
            assert all(want[i] == 0 for i in range(2, n, 5)), "a zero denominator gives 0 whatever its numerator"
            if num:
                assert all(num[1][i] for i in range(2, n, 35) if i % 7 != 3) and all(want[i] == 0 for i in range(3, n, 7))
            assert any(want)
        finally:
            call.free()


# ---- 7. the output as a column of the call
@pytest.mark.parametrize("n", [64, 257])
def test_the_output_may_be_a_32_byte_denominator_column(ctx, n):
    rng = random.Random(n)
    prev = [0 if i % 9 == 4 else rng.randrange(P) for i in range(n)]
    call = Call(ctx, [(8, random_values(rng, 8, n)), (32, prev), (1, random_values(rng, 1, n))], n, num=(32, random_values(rng, 32, n)))
    try:
        call.put_in_output(prev)
        call.check(rng.randrange(P), [rng.randrange(P), 1, 5], ptrs=[call.ptrs[0], call.out_ptr, call.ptrs[2]])
    finally:
        call.free()


@pytest.mark.parametrize("n", [64, 257])
def test_the_output_may_be_the_32_byte_numerator(ctx, n):
    rng = random.Random(n + 1)
    num = [0 if i % 6 == 1 else rng.randrange(P) for i in range(n)]
    call = Call(ctx, [(8, [0 if i % 4 == 3 else rng.randrange(1 << 64) for i in range(n)]), (2, random_values(rng, 2, n))], n, num=(32, num))
    try:
        call.put_in_output(num)
        call.check(0, [1, 0], num_ptr=call.out_ptr)
    finally:
        call.free()


@pytest.mark.parametrize("at", [[70], [0, 64, 79]])
def test_the_output_as_a_denominator_column_past_the_64th_place(ctx, at):
    """the first launch overwrites the output with the sum so far, so it takes every column that IS the output, wherever it stands"""
    n, count = 257, 80
    rng = random.Random(len(at))
    prev = [rng.randrange(P) for _ in range(n)]
    cols = [(32, prev) if j in at else (SIX[j % 5], random_values(rng, SIX[j % 5], n)) for j in range(count)]
    call = Call(ctx, cols, n)
    try:
        call.put_in_output(prev)
        ptrs = [call.out_ptr if j in at else p for j, p in enumerate(call.ptrs)]
        call.check(rng.randrange(P), [rng.randrange(P) for _ in range(count)], ptrs=ptrs)
    finally:
        call.free()


# ---- 8. refusals
def raw_call(zk, ctx, ptrs, widths, weights_mont, n, out_ptr, field=0, op=12, count=None, null=None, num=None, num_width=0):
    cnt = len(ptrs) if count is None else count
    pp = (ctypes.c_void_p * max(len(ptrs), 1))(*ptrs)
    wd = (ctypes.c_uint8 * max(len(widths), 1))(*widths)
    desc = zk.binding._RowInv0(cnt, None if null == "cols" else ctypes.cast(pp, ctypes.POINTER(ctypes.c_void_p)),
                               None if null == "widths" else ctypes.cast(wd, ctypes.POINTER(ctypes.c_uint8)), num, num_width)
    hk = np.ascontiguousarray(weights_mont)
    return zk.lib().zk_field_vec_op(ctx.h, ctypes.c_int(field), ctypes.c_int(op), ctypes.byref(desc), hk.ctypes.data_as(ctypes.c_void_p), ctypes.c_void_p(out_ptr), ctypes.c_size_t(n))


def test_refused_calls_write_nothing_and_leave_the_context_usable(zk, ctx):
    """EACH refusal is followed by its own checks: the guarded output and the inputs are untouched, and the next valid call works
    (after which the sentinels are put back for the next refusal)"""
    n = 64
    rng = random.Random(8)
    widths = [SIX[j % 6] for j in range(18)]
    t = Call(ctx, [(w, random_values(rng, w, n)) for w in widths], n, num=(8, random_values(rng, 8, n)))
    big = Call(ctx, [(1, random_values(rng, 1, n)) for _ in range(66)], n)
    const, ws = rng.randrange(P), [rng.randrange(P) for _ in range(18)]
    hk = mont([const] + ws)
    want = mont(t.want(const, ws))
    sentinels = np.full((n + 2 * GUARD, 4), SENTINEL, dtype=np.uint64)
    ptrs, out = t.ptrs, t.out_ptr
    call = lambda p=ptrs, w=widths, o=out, rows=n, num=t.num_ptr, nw=8, **kw: raw_call(zk, ctx, p, w, hk, rows, o, num=num, num_width=nw, **kw)
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
    try:
        refused("Fq", field=zk.FIELD_FQ)
        for wrong in (0, 3, 5, 24, 33, 64):
            for at in (0, 17):
                refused(f"width {wrong} at {at}", w=changed(widths, at, wrong))
            refused(f"numerator width {wrong}", nw=wrong)
        refused("a NULL column", p=changed(ptrs, 4, None))
        refused("8-byte cells at an address that is 4 mod 8", p=changed(ptrs, 3, ptrs[3] + 4))
        refused("halfwords at an odd address", p=changed(ptrs, 1, ptrs[1] + 1))
        refused("field elements at an address that is 4 mod 8", p=changed(ptrs, 5, ptrs[5] + 4))
        refused("an 8-byte numerator at an address that is 4 mod 8", num=t.num_ptr + 4)
        refused("a 32-byte numerator at an address that is 4 mod 8", num=ptrs[5] + 4, nw=32)
        refused("a byte column inside the output", p=changed(ptrs, 0, out + 7))
        refused("a 16-byte column AT the output", p=changed(ptrs, 4, out))
        refused("a 32-byte column one element into the output", p=changed(ptrs, 5, out + 32))
        refused("a 32-byte column one element in front of the output", p=changed(ptrs, 5, out - 32))
        refused("the output inside a 32-byte column", o=ptrs[5] + 8)
        refused("an 8-byte numerator AT the output", num=out)
        refused("a 32-byte numerator one element into the output", num=out + 32, nw=32)
        refused("NULL d_cols", null="cols")
        refused("NULL widths", null="widths")
        for op in (5, 6, 7, 11, 13):
            refused(f"op {op}", op=op)
            refused(f"op {op} over Fq", op=op, field=zk.FIELD_FQ)
        refused("a bad width with n = 0", w=changed(widths, 2, 3), rows=0)
        refused("a bad numerator width with n = 0", nw=3, rows=0)
        assert len(refusals) == 46
        # more than 64 terms: the output holds the sum so far and cannot also be the numerator
        hk66 = mont([1] * 67)
        assert raw_call(zk, ctx, big.ptrs, big.widths, hk66, n, big.out_ptr, num=big.out_ptr, num_width=32) == INVALID_ARG
        ctx.sync()
        assert big.untouched()
        assert call(rows=0) == 0                                                                        # n = 0: ZK_OK, nothing written
        assert call(p=changed(ptrs, 4, out), rows=0) == 0                                               # nothing to overlap
        assert call(num=None, nw=77) == 0                                                               # num_width is ignored without a numerator
        t.num = None
        assert np.array_equal(t.result(), mont(t.want(const, ws)))
    finally:
        t.free()
        big.free()


# ---- 9. profiling
def test_each_launch_books_its_bytes(ctx):
    n = 255
    rng = random.Random(9)

    def booked(count, num):
        cols = [(SIX[j % 6], random_values(rng, SIX[j % 6], n)) for j in range(count)]
        call = Call(ctx, cols, n, num=num)
        ctx.sync()
        ctx.prof_reset()
        ctx.prof_enable(True)
        try:
            call.check(1, [rng.randrange(P) for _ in range(count)])
            ms, launches = ctx.prof_get("fr_row_inv0")
            assert ms > 0
            return launches, ctx.prof_get_bytes("fr_row_inv0"), call.widths
        finally:
            ctx.prof_enable(False)
            ctx.prof_reset()
            call.free()
    launches, nbytes, widths = booked(17, None)
    assert (launches, nbytes) == (1, n * (sum(widths) + 32))
    launches, nbytes, widths = booked(17, (2, random_values(rng, 2, n)))
    assert (launches, nbytes) == (1, n * (sum(widths) + 2 + 32))
    launches, nbytes, widths = booked(65, (16, random_values(rng, 16, n)))       # the second launch reads the sum so far as a 32-byte column
    assert (launches, nbytes) == (2, n * (sum(widths[:RR_BATCH]) + 32) + n * (32 + sum(widths[RR_BATCH:]) + 16 + 32))


# ---- 10. against the composition on the same device bytes
@pytest.mark.parametrize("with_num", [False, True])
def test_equals_the_composition(zk, ctx, with_num):
    n = 2049
    rng = random.Random(10 + with_num)
    a = [rng.randrange(1 << 64) for _ in range(n)]
    bb = [a[i] if i % 3 == 0 else rng.randrange(1 << 64) for i in range(n)]
    num = (32, random_values(rng, 32, n)) if with_num else None
    call = Call(ctx, [(8, a), (8, bb), (1, random_values(rng, 1, n))], n, num=num)
    tmp = ctx.alloc(n * 32)
    ws = [1, P - 1, 0]
    try:
        ctx.row_rlc(call.ptrs, call.widths, mont(ws), n, tmp, constant=mont([0])[0])
        ctx.fr_batch_invert(tmp, n)
        if with_num:
            lib = zk.lib()
            assert lib.zk_field_vec_op(ctx.h, zk.FIELD_FR, zk.OP_MUL, ctypes.c_void_p(tmp.ptr), ctypes.c_void_p(call.num_ptr), ctypes.c_void_p(tmp.ptr), ctypes.c_size_t(n)) == 0
        call.run(0, ws)
        got = call.result()
        assert np.array_equal(got, tmp.download((n, 4)))
        assert np.array_equal(got, mont(call.want(0, ws)))
    finally:
        tmp.free()
        call.free()

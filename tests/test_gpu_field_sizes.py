"""GPU: the vector primitives of csrc/vec.hip -- prefix product and sum, Kate division, polynomial evaluation (single, batched,
paired), batch inversion -- against the C oracle, bit for bit, at the sizes where their structure changes and tests/test_gpu_field.py
(which stops at 2^18 elements) never gets: the workload is k = 19 to 23.

scan_run (zk_fr_prefix_product, zk_fr_prefix_sum, the scan inside zk_kate_division): a block scans BLOCK = 2048 elements, k_scan_b
scans the block totals in windows of 256 blocks with a serial carry between windows, so WINDOW = 524 288 elements is the most a
single window covers.
  n = WINDOW - 1, WINDOW          256 blocks: one window, no carry (the last block short by one / full)
  n = WINDOW + 1                  257 blocks: the second window holds one block, which takes the carry
  n = 2 WINDOW + BLOCK + 1        514 blocks: two full windows and a third of two blocks: the carry is carried on, not just handed over once
  Kate division at n - 1 = 2047, 2048, 2049 is one block, one block full, two blocks; n - 1 = WINDOW + 1 takes the carry.

zk_poly_eval: 256 threads a block, at most 1024 blocks -- 262 144 elements a sweep of the grid-stride loop.
  n = 262 144                     one sweep exactly;     n = 262 145: thread 0 of block 0 runs the loop a second time;     n = 2^20 + 1: five sweeps

zk_poly_eval_batch, zk_poly_eval_pairs (k_eval_horner_multi, k_eval_horner_pairs): blocks = min(256, ceil(n / 4096)) and
seg = roundup256(ceil(n / blocks)); below the cap (blocks - 1) seg < n always, so only above it can a block be left without coefficients.
  n = 2^20                        256 blocks of 4096: the cap is reached, no block is empty, 16 Horner steps a thread
  n = 2^20 + 1                    seg = 4352: 241 blocks hold coefficients (the last one 4097 of them), 15 take the `start < end ? .. : zero` branch
  n = 2^21 + 3                    seg = 8448: 249 blocks hold coefficients (33 steps a thread), 7 are empty
  n = 513, 4097                   one and two blocks; coefficients r - 1: the sum a Horner step leaves is at the 3p bound its comment names

zk_fr_batch_invert: a wave with nothing but zeros inverts the empty product; all-zero input; a single zero; 2^20 + 7 elements."""
import random

import numpy as np
import pytest

from oracle import bn254

gpu = pytest.mark.gpu
R = bn254.R_MOD
BLOCK, WINDOW = 2048, 524288
assert (BLOCK, WINDOW) == (8 * 256, 8 * 256 * 256)
N_SCAN = 2 * WINDOW + BLOCK + 1
N_MAX = (1 << 21) + 3
MARKS = [0, BLOCK - 1, BLOCK, WINDOW - 1, WINDOW, WINDOW + BLOCK, 2 * WINDOW - 1, 2 * WINDOW]
assert N_SCAN == 1050625 and MARKS == [0, 2047, 2048, 524287, 524288, 526336, 1048575, 1048576]
X0 = random.Random(0x51E5).randrange(R)
POINTS = [X0, 0, 1, R - 1]


# ---- the host formulas of zk_poly_eval_batch / zk_poly_eval_pairs, restated (no GPU)
def horner_split(n):
    """-> (blocks, seg, blocks that hold coefficients) for n >= 512"""
    blocks = min(256, (n + 4095) // 4096)
    seg = ((n + blocks - 1) // blocks + 255) // 256 * 256
    return blocks, seg, sum(1 for b in range(blocks) if b * seg < n)


def test_host_formulas_of_the_batched_evaluation():
    assert horner_split(1 << 20) == (256, 4096, 256)
    assert horner_split((1 << 20) + 1) == (256, 4352, 241)                     # 15 empty blocks
    assert (1 << 20) + 1 - 240 * 4352 == 4097
    assert horner_split((1 << 21) + 3) == (256, 8448, 249)                     # 7 empty blocks
    assert horner_split(513) == (1, 768, 1) and horner_split(4097) == (2, 2304, 2)
    for n in list(range(512, 9000, 37)) + [70001, 1 << 16, 1 << 18, (1 << 20) - 1, 1 << 20]:        # up to the cap no block is ever empty
        blocks, seg, full = horner_split(n)
        assert full == blocks and blocks * seg >= n
    assert all(horner_split(n)[2] < 256 for n in ((1 << 20) + 1, (1 << 20) + 3841))                 # past it, at once
    # zk_poly_eval: min(1024, ceil(n / 256)) blocks of 256 threads
    assert 1024 * 256 == 262144
    # scan_run: blocks of BLOCK elements, windows of 256 blocks
    assert [(n + BLOCK - 1) // BLOCK for n in (WINDOW - 1, WINDOW, WINDOW + 1, N_SCAN)] == [256, 256, 257, 514]


# ---- operands
class Operands:
    """three polynomials of N_MAX random elements from three seeds (a swap cannot pass), on the device once; a prefix of length n is
    the first n elements.  The scans of the first one over N_SCAN elements, once: their first n values are the scans of its first n."""

    def __init__(self, ctx, cref):
        self.P = [cref.rand_fr_stream(0xF1E1D + i, N_MAX) for i in range(3)]
        self.dP = [ctx.to_device(p) for p in self.P]
        self.dZ = ctx.alloc(N_MAX * 32)
        self.product = cref.prefix_product(self.P[0][:N_SCAN])
        self.sum = cref.prefix_sum(self.P[0][:N_SCAN])
        self.evals = {}

    def eval(self, cref, i, n, x):
        """eval_polynomial of the first n coefficients of polynomial i at x, computed once"""
        key = (i, n, x)
        if key not in self.evals:
            self.evals[key] = cref.eval_polynomial(self.P[i][:n], x)
        return self.evals[key]


@pytest.fixture(scope="module")
def ops(ctx, cref):
    o = Operands(ctx, cref)
    yield o
    for buf in o.dP + [o.dZ]:
        buf.free()


def first_difference(got, want):
    d = np.nonzero((got != want).any(axis=1))[0]
    return None if d.size == 0 else (int(d[0]), int(d.size))


# ---- 1. prefix product and prefix sum
@gpu
@pytest.mark.parametrize("n", [WINDOW - 1, WINDOW, WINDOW + 1, N_SCAN])
def test_prefix_scans_across_windows(ctx, ops, n):
    ctx.fr_prefix_product(ops.dP[0], ops.dZ, n)
    got = ops.dZ.download((n, 4))
    assert np.array_equal(got, ops.product[:n]), first_difference(got, ops.product[:n])
    ctx.fr_prefix_sum(ops.dP[0], ops.dZ, n)
    got = ops.dZ.download((n, 4))
    assert np.array_equal(got, ops.sum[:n]), first_difference(got, ops.sum[:n])


@gpu
@pytest.mark.parametrize("op", ["product", "sum"])
def test_sparse_operand_shows_every_carry(ctx, cref, ops, op):
    """the identity everywhere but at the first and last element of blocks and windows: the scan is a staircase with a step behind each
    mark, so a carry that is lost, applied twice or applied a block late changes whole stretches of it"""
    n = N_SCAN
    A = np.repeat(cref.to_mont([1 if op == "product" else 0]), n, axis=0)
    A[MARKS] = ops.P[1][:len(MARKS)]
    values = cref.from_mont(ops.P[1][:len(MARKS)])
    assert len(set(values)) == len(MARKS) and not {0, 1} & set(values)
    dA = ctx.to_device(A)
    try:
        (ctx.fr_prefix_product if op == "product" else ctx.fr_prefix_sum)(dA, ops.dZ, n)
    finally:
        dA.free()
    got = ops.dZ.download((n, 4))
    want = (cref.prefix_product if op == "product" else cref.prefix_sum)(A)
    assert np.array_equal(got, want), first_difference(got, want)
    # the staircase itself, from the integers: z[i] = the product (sum) of the marked values before i
    steps, acc = [], 1 if op == "product" else 0
    for v in values:
        acc = acc * v % R if op == "product" else (acc + v) % R
        steps.append(acc)
    steps = cref.to_mont(steps)
    for j, mark in enumerate(MARKS):
        end = MARKS[j + 1] if j + 1 < len(MARKS) else n - 1
        assert np.array_equal(got[mark + 1], steps[j]) and np.array_equal(got[end], steps[j]), (j, mark)


@gpu
def test_product_with_a_zero_at_the_window_boundary(ctx, cref, ops):
    n = N_SCAN
    A = ops.P[0][:n].copy()
    A[WINDOW] = 0
    dA = ctx.to_device(A)
    try:
        ctx.fr_prefix_product(dA, ops.dZ, n)
    finally:
        dA.free()
    got = ops.dZ.download((n, 4))
    assert np.array_equal(got[:WINDOW + 1], ops.product[:WINDOW + 1]), first_difference(got[:WINDOW + 1], ops.product[:WINDOW + 1])
    assert got[WINDOW].any() and not got[WINDOW + 1:].any()
    assert np.array_equal(got, cref.prefix_product(A))


# ---- 2. Kate division and single evaluation
@gpu
@pytest.mark.parametrize("nm1", [2047, 2048, 2049, WINDOW + 1])
def test_kate_division_across_blocks_and_windows(ctx, cref, ops, nm1):
    n = nm1 + 1
    C = ops.P[1][:n]
    for z in [X0, 1, R - 1] + ([0] if nm1 < 4096 else []):
        ctx.kate_division(ops.dP[1], n, cref.fr_const(z), ops.dZ)
        got, want = ops.dZ.download((nm1, 4)), cref.kate_division(C, z)
        assert np.array_equal(got, want), (z, first_difference(got, want))


@gpu
@pytest.mark.parametrize("n", [262144, 262145, (1 << 20) + 1])
def test_poly_eval_past_one_sweep_of_the_grid(ctx, cref, ops, n):
    for x in POINTS:
        got = ctx.poly_eval(ops.dP[0], n, cref.fr_const(x))
        assert cref.from_mont(got.reshape(1, 4))[0] == ops.eval(cref, 0, n, x), x


# ---- 3. batched and paired evaluation past the block cap
BIG = [1 << 20, (1 << 20) + 1, (1 << 21) + 3]


@gpu
@pytest.mark.parametrize("n", BIG)
def test_poly_eval_batch_past_the_block_cap(ctx, cref, ops, n):
    for x in POINTS:
        got = cref.from_mont(ctx.poly_eval_batch(ops.dP, n, cref.fr_const(x)))
        assert [int(v) for v in got] == [ops.eval(cref, i, n, x) for i in range(3)], x


@gpu
@pytest.mark.parametrize("n", BIG)
def test_poly_eval_pairs_past_the_block_cap(ctx, cref, ops, n):
    """4 pairs over 3 points, the first point shared by two polynomials, the first polynomial at two points"""
    polys, idx = [0, 1, 2, 0], [0, 0, 1, 2]
    for points in ([X0, 0, 1], [R - 1, X0, 1]):
        got = cref.from_mont(ctx.poly_eval_pairs([ops.dP[i] for i in polys], idx, cref.to_mont(points), n))
        assert [int(v) for v in got] == [ops.eval(cref, i, n, points[p]) for i, p in zip(polys, idx)], points


# ---- 4. coefficients at the lazy-reduction bound
@gpu
@pytest.mark.parametrize("n", [513, 4097])
def test_coefficients_at_the_lazy_reduction_bound(ctx, cref, n):
    full = np.repeat(cref.to_mont([R - 1]), n, axis=0)
    top = np.zeros((n, 4), dtype=np.uint64)
    top[n - 1] = full[0]
    dF, dT = ctx.to_device(full), ctx.to_device(top)
    try:
        want = {}
        for x in POINTS:
            want[x] = (cref.eval_polynomial(full, x), cref.eval_polynomial(top, x))
            assert want[x][1] == (R - 1) * pow(x, n - 1, R) % R
            if x != 1:
                assert want[x][0] == -(pow(x, n, R) - 1) * pow(x - 1, R - 2, R) % R           # -(x^n - 1) / (x - 1)
            else:
                assert want[x][0] == -n % R
            got = cref.from_mont(ctx.poly_eval_batch([dF, dT, dF], n, cref.fr_const(x)))
            assert [int(v) for v in got] == [want[x][0], want[x][1], want[x][0]], x
        got = cref.from_mont(ctx.poly_eval_pairs([dF, dT, dF, dT, dF, dT, dF, dT], [0, 0, 1, 1, 2, 2, 3, 3], cref.to_mont(POINTS), n))
        assert [int(v) for v in got] == [want[x][j] for x in POINTS for j in (0, 1)]
    finally:
        dF.free(), dT.free()


# ---- 5. batch inversion
@gpu
def test_batch_invert_of_nothing_but_zeros(ctx, cref):
    for n in (4096, 1):
        A = np.zeros((n, 4), dtype=np.uint64)
        dA = ctx.to_device(A)
        try:
            ctx.fr_batch_invert(dA, n)
            assert not dA.download((n, 4)).any()
        finally:
            dA.free()
        assert not cref.batch_invert(A).any()


@gpu
def test_batch_invert_past_a_million(ctx, cref, ops):
    """zeros at both ends and in every element of one wave: lane t of the launch owns the elements t, t + nt, .., t + 7 nt"""
    n = (1 << 20) + 7
    nt = ((n + 7) // 8 + 63) // 64 * 64
    A = ops.P[2][:n].copy()
    A[0] = A[n - 1] = 0
    for k in range(8):
        A[k * nt + 64 * 5:k * nt + 64 * 6] = 0
    assert 7 * nt + 64 * 6 < n
    dA = ctx.to_device(A)
    try:
        ctx.fr_batch_invert(dA, n)
        got = dA.download((n, 4))
    finally:
        dA.free()
    want = cref.batch_invert(A)
    assert np.array_equal(got, want), first_difference(got, want)
    assert not got[0].any() and not got[n - 1].any() and not got[64 * 5:64 * 6].any() and got[64 * 6].any()

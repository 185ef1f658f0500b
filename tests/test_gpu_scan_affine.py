"""GPU: the affine scan ops of zk_field_vec_op -- ZK_OP_SCAN_AFFINE out[i] = a[i] out[i-1] + b[i] and ZK_OP_SCAN_AFFINE_REV
out[i] = a[i] out[i+1] + b[i], from the state 0 -- against the big-integer recurrence (a plain Python loop mod r, converted by the
oracle's to_mont), bit for bit, at every boundary of the kernels' tiling; against the prefix sum and the prefix product where the
recurrence degenerates into them; resets (a[i] = 0) at tile boundaries; what the call refuses, and what it books.

The tiling (csrc/vec.hip): SCAN_PER elements per thread, SCAN_THREADS threads per block, and the block maps are scanned in windows of
SCAN_THREADS blocks with a serial carry between windows."""
import ctypes

import numpy as np
import pytest

from oracle import bn254

pytestmark = pytest.mark.gpu
R = bn254.R_MOD
SCAN_PER, SCAN_THREADS = 8, 256
BLOCK = SCAN_PER * SCAN_THREADS                       # 2048 elements per block
WINDOW = BLOCK * SCAN_THREADS                         # 524 288 elements per window of block maps
SIZES = [1, 2, SCAN_PER - 1, SCAN_PER, SCAN_PER + 1, SCAN_THREADS - 1, SCAN_THREADS, SCAN_THREADS + 1, BLOCK - 1, BLOCK, BLOCK + 1,
         2 * BLOCK + 1, WINDOW - 1, WINDOW, WINDOW + 1]
N_MAX = max(SIZES)
INVALID_ARG = -1
assert SIZES == [1, 2, 7, 8, 9, 255, 256, 257, 2047, 2048, 2049, 4097, 524287, 524288, 524289]


def recurrence(a, b, reverse=False):
    """the definition, on Python integers: z = 0 before the first element, then z = a[i] z + b[i] mod r, element by element"""
    out, z = [0] * len(a), 0
    for i in (range(len(a) - 1, -1, -1) if reverse else range(len(a))):
        z = (a[i] * z + b[i]) % R
        out[i] = z
    return out


class Operands:
    """a and b of N_MAX elements from two seeds (a swapped composition cannot pass), their first four cells forced to r-1, 0, 1, r-2;
    on the device once; the forward recurrence over all of them once: its first n values are the recurrence of the first n"""

    def __init__(self, ctx, cref):
        self.A, self.B = cref.rand_fr_stream(0xA5CA, N_MAX), cref.rand_fr_stream(0xB5CB, N_MAX)
        self.A[:4] = self.B[:4] = cref.to_mont([R - 1, 0, 1, R - 2])
        self.a, self.b = cref.from_mont(self.A), cref.from_mont(self.B)
        self.dA, self.dB, self.dO = ctx.to_device(self.A), ctx.to_device(self.B), ctx.alloc(N_MAX * 32)
        self.forward = cref.to_mont(recurrence(self.a, self.b))


@pytest.fixture(scope="module")
def ops(ctx, cref):
    o = Operands(ctx, cref)
    yield o
    for buf in (o.dA, o.dB, o.dO):
        buf.free()


def run(ctx, zk, A, B, reverse=False):
    """the op on host arrays: upload, one call, download"""
    n = A.shape[0]
    dA, dB, dO = ctx.to_device(A), ctx.to_device(B), ctx.alloc(n * 32)
    try:
        ctx.field_vec_op(zk.FIELD_FR, zk.OP_SCAN_AFFINE_REV if reverse else zk.OP_SCAN_AFFINE, dA, dB, dO, n)
        return dO.download((n, 4))
    finally:
        for buf in (dA, dB, dO):
            buf.free()


# ---- 1. parity with the big-integer recurrence
@pytest.mark.parametrize("n", SIZES)
def test_forward_equals_the_integer_recurrence(zk, ctx, ops, n):
    ctx.field_vec_op(zk.FIELD_FR, zk.OP_SCAN_AFFINE, ops.dA, ops.dB, ops.dO, n)
    assert np.array_equal(ops.dO.download((n, 4)), ops.forward[:n])


@pytest.mark.parametrize("n", SIZES)
def test_reverse_equals_the_integer_recurrence(zk, ctx, cref, ops, n):
    ctx.scan_affine(ops.dA, ops.dB, ops.dO, n, reverse=True)
    assert np.array_equal(ops.dO.download((n, 4)), cref.to_mont(recurrence(ops.a[:n], ops.b[:n], reverse=True)))


# ---- 2. resets
@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("n", [2 * BLOCK + 1, WINDOW + 1])
def test_resets_at_tile_boundaries(zk, ctx, cref, ops, n, reverse):
    """a = 0 at the first position of a thread chunk, of a block, of a window, either side of them, and at the last position; in scan
    order, so mirrored in memory for the reverse op"""
    a, A = list(ops.a[:n]), ops.A[:n].copy()
    for pos in (1, SCAN_PER, BLOCK - 1, BLOCK, BLOCK + 1, WINDOW, n - 1):
        if pos < n:
            i = n - 1 - pos if reverse else pos
            a[i], A[i] = 0, 0
    got = run(ctx, zk, A, ops.B[:n], reverse)
    want = recurrence(a, ops.b[:n], reverse)
    step = -1 if reverse else 1
    for pos in (SCAN_PER, BLOCK, n - 1):                                    # a segment starts there: the value is b alone
        i = n - 1 - pos if reverse else pos
        assert want[i] == ops.b[i]
    for pos in (SCAN_PER, BLOCK):                                           # and the state it cuts off was not zero anyway
        i = n - 1 - pos if reverse else pos
        assert want[i - step] != 0
    assert np.array_equal(got, cref.to_mont(want))


# ---- 3. where the recurrence is a scan that already exists
N_CROSS = 2 * BLOCK + 3


def test_with_a_equal_one_it_is_the_prefix_sum(zk, ctx, cref, ops):
    n = N_CROSS
    B = ops.B[:n]
    got = run(ctx, zk, np.repeat(cref.to_mont([1]), n, axis=0), B)
    dB, dZ = ctx.to_device(B), ctx.alloc(n * 32)
    ctx.fr_prefix_sum(dB, dZ, n)                                            # z[0] = 0, z[i + 1] = z[i] + b[i]
    z = dZ.download((n, 4))
    dB.free(), dZ.free()
    assert np.array_equal(got[:n - 1], z[1:])
    assert np.array_equal(got[n - 1:], cref.fe_binop("add", 0, np.ascontiguousarray(z[n - 1:]), np.ascontiguousarray(B[n - 1:])))


def test_with_b_a_unit_impulse_it_is_the_prefix_product(zk, ctx, cref, ops):
    n = N_CROSS
    A = ops.A[:n].copy()
    A[1] = cref.to_mont([5])[0]                                             # the forced zero: this test wants no reset
    assert all(v != 0 for v in cref.from_mont(A))
    B = np.zeros((n, 4), dtype=np.uint64)
    B[0] = cref.to_mont([1])[0]
    got = run(ctx, zk, A, B)
    P = A.copy()
    P[0] = cref.to_mont([1])[0]
    dP, dZ = ctx.to_device(P), ctx.alloc(n * 32)
    ctx.fr_prefix_product(dP, dZ, n)                                        # z[0] = 1, z[i + 1] = z[i] * p[i]
    z = dZ.download((n, 4))
    dP.free(), dZ.free()
    assert np.array_equal(got[:n - 1], z[1:])
    assert np.array_equal(got[n - 1:], cref.fe_binop("mul", 0, np.ascontiguousarray(z[n - 1:]), np.ascontiguousarray(A[n - 1:])))


# ---- 4. the reverse op is the forward op on reversed inputs, reversed
@pytest.mark.parametrize("n", [SCAN_PER + 1, BLOCK + 1])
def test_reverse_is_forward_on_reversed_inputs(zk, ctx, ops, n):
    A, B = ops.A[:n], ops.B[:n]
    fwd = run(ctx, zk, np.ascontiguousarray(A[::-1]), np.ascontiguousarray(B[::-1]))
    assert np.array_equal(run(ctx, zk, A, B, reverse=True), fwd[::-1])


# ---- 5. refusals
def test_refused_calls_launch_nothing_and_leave_the_context_usable(zk, ctx, ops):
    lib, n = zk.lib(), BLOCK + 1
    guard = np.full((n + 1, 4), 0x5A5A5A5A5A5A5A5A, dtype=np.uint64)
    dA, dB, dO = ctx.to_device(ops.A[:n + 1]), ctx.to_device(ops.B[:n + 1]), ctx.to_device(guard)

    def call(field, op, a, b, out, count=n):
        return lib.zk_field_vec_op(ctx.h, ctypes.c_int(field), ctypes.c_int(op), ctypes.c_void_p(a), ctypes.c_void_p(b), ctypes.c_void_p(out), ctypes.c_size_t(count))
    try:
        for op in (zk.OP_SCAN_AFFINE, zk.OP_SCAN_AFFINE_REV):
            assert call(zk.FIELD_FQ, op, dA.ptr, dB.ptr, dO.ptr) == INVALID_ARG
            assert call(zk.FIELD_FR, op, dA.ptr, dB.ptr, dA.ptr) == INVALID_ARG             # out is a
            assert call(zk.FIELD_FR, op, dA.ptr, dB.ptr, dB.ptr) == INVALID_ARG             # out is b
            assert call(zk.FIELD_FR, op, dA.ptr, dB.ptr, dB.ptr + 32) == INVALID_ARG        # out starts one element into b
            assert call(zk.FIELD_FR, op, dA.ptr + 32, dB.ptr, dA.ptr) == INVALID_ARG        # a starts one element into out
        assert call(zk.FIELD_FR, 5, dA.ptr, dB.ptr, dO.ptr) == INVALID_ARG
        assert call(zk.FIELD_FQ, 5, dA.ptr, dB.ptr, dO.ptr) == INVALID_ARG
        ctx.sync()
        assert np.array_equal(dO.download((n + 1, 4)), guard)
        assert np.array_equal(dA.download((n + 1, 4)), ops.A[:n + 1]) and np.array_equal(dB.download((n + 1, 4)), ops.B[:n + 1])
        for op in (zk.OP_SCAN_AFFINE, zk.OP_SCAN_AFFINE_REV):
            assert call(zk.FIELD_FR, op, dA.ptr, dB.ptr, dO.ptr, 0) == 0                    # n = 0: ZK_OK
            assert call(zk.FIELD_FR, op, dA.ptr, dB.ptr, dA.ptr, 0) == 0                    # nothing to overlap
        assert np.array_equal(dO.download((n + 1, 4)), guard)
        assert call(zk.FIELD_FR, zk.OP_SCAN_AFFINE, dA.ptr, dB.ptr, dO.ptr) == 0            # the next valid call
        got = dO.download((n + 1, 4))
        assert np.array_equal(got[:n], ops.forward[:n]) and np.array_equal(got[n:], guard[n:])
    finally:
        for buf in (dA, dB, dO):
            buf.free()


# ---- 6. the element-wise ops keep their aliasing
def test_elementwise_ops_still_write_over_an_input(zk, ctx, cref, ops):
    n = BLOCK + 37
    A, B = ops.A[:n], ops.B[:n]
    dB = ctx.to_device(B)
    for op, name in ((zk.OP_ADD, "add"), (zk.OP_SUB, "sub"), (zk.OP_MUL, "mul")):
        dA = ctx.to_device(A)
        ctx.field_vec_op(zk.FIELD_FR, op, dA, dB, dA, n)
        assert np.array_equal(dA.download((n, 4)), cref.fe_binop(name, 0, np.ascontiguousarray(A), np.ascontiguousarray(B))), name
        dA.free()
    dB.free()


# ---- 7. profiling
def test_one_call_books_one_scope(zk, ctx, ops):
    n = 2 * BLOCK + 1
    ctx.sync()
    ctx.prof_reset()
    ctx.prof_enable(True)
    try:
        ctx.scan_affine(ops.dA, ops.dB, ops.dO, n)
        ms, count = ctx.prof_get("fr_scan_affine")
        assert count == 1 and ms > 0
        assert ctx.prof_get_bytes("fr_scan_affine") == n * 96
    finally:
        ctx.prof_enable(False)
        ctx.prof_reset()

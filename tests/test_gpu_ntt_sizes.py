"""GPU: the NTT at the sizes the other tests do not reach -- 2^23 (digits 8, 8, 7), 2^24 against the oracle's eval_polynomial at
single outputs, 2^25 and 2^27 (no inter-pass tables because of their size; digits of 2^9 in three passes) checked on the device
against zk_poly_eval, and the per-column coset shifts of coeff_to_extended / extended_to_coeff around three passes."""
import ctypes

import numpy as np
import pytest

from oracle import bn254

pytestmark = pytest.mark.gpu

def fetch(zk, c, buf, i):
    """element i of a device column: one 32-byte copy"""
    out = np.empty(4, dtype=np.uint64)
    c._ck(zk.lib().zk_d2h(c.h, out.ctypes.data_as(ctypes.c_void_p), ctypes.c_void_p(buf.ptr + 32 * i), ctypes.c_size_t(32)))
    return out


def spot_indices(n, seed, count):
    """0, 1, n/2, n - 1 and count - 4 more from a seeded generator"""
    rng = np.random.default_rng(seed)
    return [0, 1, n // 2, n - 1] + [int(i) for i in rng.integers(2, n - 1, size=count - 4)]


def device_columns(c, k, count):
    """count random columns of 2^k made on the device (nothing of size n goes up)"""
    bufs = [c.alloc(32 << k) for _ in range(count)]
    for j, b in enumerate(bufs):
        c.fr_random(bytes(range(32)), 2300 + j, 0, b, 1 << k)
    return bufs


def test_2_23_batch_of_three(zk, ctx, cref):
    """k = 23, digits (8, 8, 7), in no other test: three columns in one batch.  The first forward column against best_fft, forward
    and inverse return the input on all three, and the batched coset transform equals the single-column entry point."""
    k, n = 23, 1 << 23
    assert [r["log_np"] for r in zk.binding.host_ntt_plan(k, 3)["launches"]] == [8, 8, 7]
    bufs = device_columns(ctx, k, 3)
    outs = [ctx.alloc(n * 32) for _ in bufs]
    single = ctx.alloc(n * 32)
    try:
        before = [b.download((n, 4)) for b in bufs]
        assert not np.array_equal(before[0], before[1])
        ctx.ntt_batch(bufs, k)
        assert np.array_equal(bufs[0].download((n, 4)), cref.best_fft(before[0], bn254.omega_for_k(k), k))
        assert not np.array_equal(bufs[2].download((64, 4)), before[2][:64])
        ctx.ntt_batch(bufs, k, inverse=True)
        for b, a in zip(bufs, before):
            assert np.array_equal(b.download((n, 4)), a)
        del before
        g = cref.fr_const(0xC05E70 + k)
        ctx.coeff_to_coset_batch(bufs, k, g, outs)
        for b, o in zip(bufs, outs):
            ctx.coeff_to_coset(b, k, g, single)
            assert np.array_equal(o.download((n, 4)), single.download((n, 4)))
    finally:
        for b in bufs + outs + [single]:
            b.free()


def test_2_24_outputs_against_eval_polynomial(zk, ctx, cref):
    """k = 24, digits (8, 8, 8), the only three-pass shape with padded rows in the last pass: out[i] = A(omega^i) by the oracle's
    eval_polynomial at 0, 1, n/2, n - 1 and four seeded indices (a Horner pass over 2^24 coefficients on the CPU per point), and
    the inverse returns the input."""
    k, n = 24, 1 << 24
    A = cref.rand_fr_stream(2424, n)
    w = bn254.omega_for_k(k)
    idx = spot_indices(n, 24, 8)
    d = ctx.to_device(A)
    try:
        ctx.ntt(d, k)
        got = [fetch(zk, ctx, d, i) for i in idx]
        ctx.ntt(d, k, inverse=True)
        assert np.array_equal(d.download((n, 4)), A)
    finally:
        d.free()
    for i, v in zip(idx, got):
        assert cref.from_mont(v.reshape(1, 4))[0] == cref.eval_polynomial(A, pow(w, i, bn254.R_MOD)), i


@pytest.mark.parametrize("k", [25, 27])
def test_tableless_by_size(zk, cref, k):
    """k = 25, digits (9, 8, 8), and 27, digits (9, 9, 9): above 2^24 a domain has no inter-pass tables, and a digit of 2^9 sits in
    a strided pass of three (25) and in the last pass behind a middle digit (27).  All on the device, in a context of its own:
    16 outputs of the forward transform against zk_poly_eval of a copy of the input at omega^i; the inverse through two points
    at which (result - copy) must be 0 -- it is the zero polynomial, or both points are among the fewer than 2^27 roots it has in a
    254-bit field.  zk_poly_eval is a different kernel, tested against the oracle up to n = 100 000 elsewhere: it is anchored at
    this size on the all-ones polynomial (0 at omega, 2^n - 1 at 2), and at k = 25 one output is also compared with the oracle's
    eval_polynomial on a downloaded copy."""
    n = 1 << k
    plan = zk.binding.host_ntt_plan(k, 1)
    assert not plan["tables"] and [r["log_np"] for r in plan["launches"]] == ([9, 8, 8] if k == 25 else [9, 9, 9])
    assert not any(r["fixed"] for r in plan["launches"])
    w = bn254.omega_for_k(k)
    idx = spot_indices(n, k, 16)
    own = zk.Context(0)
    held = []
    try:
        data = own.alloc(n * 32)
        held.append(data)
        copy = own.alloc(n * 32)
        held.append(copy)
        one = cref.fr_const(1)
        own.fr_powers(one, one, data, n)
        assert not own.poly_eval(data, n, cref.fr_const(w)).any()
        assert cref.from_mont(own.poly_eval(data, n, cref.fr_const(2)).reshape(1, 4))[0] == (pow(2, n, bn254.R_MOD) - 1) % bn254.R_MOD
        own.fr_random(bytes(range(32)), k, 0, data, n)
        own._ck(zk.lib().zk_d2d(own.h, ctypes.c_void_p(copy.ptr), ctypes.c_void_p(data.ptr), ctypes.c_size_t(n * 32)))
        own.ntt(data, k)
        for i in idx:
            assert np.array_equal(fetch(zk, own, data, i), own.poly_eval(copy, n, cref.fr_const(pow(w, i, bn254.R_MOD)))), i
        if k == 25:
            i = idx[-1]
            assert cref.from_mont(fetch(zk, own, data, i).reshape(1, 4))[0] == cref.eval_polynomial(copy.download((n, 4)), pow(w, i, bn254.R_MOD))
        own.ntt(data, k, inverse=True)
        own.field_vec_op(zk.binding.FIELD_FR, zk.binding.OP_SUB, data, copy, data, n)
        for x in (0x1234567 + k, pow(7, 1000 + k, bn254.R_MOD)):
            assert not own.poly_eval(data, n, cref.fr_const(x)).any()
    finally:
        for b in held:
            b.free()
        own.close()


def test_coset_shifts_around_three_passes(zk, ctx, cref):
    """EvaluationDomain::coeff_to_extended / extended_to_coeff at ext_k = 21: the shift by zeta^i (before) and zeta^-i (after) as a
    pass of its own, column by column, around three NTT passes"""
    k, ext_k = 19, 21
    n, ne = 1 << k, 1 << ext_k
    plan = zk.binding.host_ntt_plan(ext_k, 1, True, True)
    assert plan["passes"] == 3 and plan["per_launch"] == 1
    A = cref.rand_fr_stream(3000 + k, n)
    dA, dE = ctx.to_device(A), ctx.alloc(ne * 32)
    try:
        ctx.coeff_to_extended(dA, k, ext_k, dE)
        got = dE.download((ne, 4))
        padded = np.zeros((ne, 4), dtype=np.uint64)
        padded[:n] = cref.distribute_powers(A, bn254.FR_ZETA)
        assert np.array_equal(got, cref.best_fft(padded, bn254.omega_for_k(ext_k), ext_k))
        ctx.extended_to_coeff(dE, ext_k)
        back = dE.download((ne, 4))
    finally:
        dA.free()
        dE.free()
    assert np.array_equal(back[:n], A)
    assert not back[n:].any()

"""GPU: g_to_lagrange (csrc/ecntt.hip, the inverse FFT over G1 behind zk_srs_create without a Lagrange basis and behind
zk_srs_downsize) on the cases of tests/ecntt_cases.py -- monomial bases in which butterflies meet identities, the same point twice
and opposite points in different XYZZ representations -- against the big-int model, bit for bit on the affine image.  A generic
SRS (g[j] = s^j G) reaches none of these branches: k_ecntt_load's and k_ecntt_finish's identity rows, mul_scalar29 and neg29pt of
an identity, add29pt's early returns, its fall-through to dbl29pt and its identity result.  k = 10 is 512 butterflies a stage: two
workgroups of k_ecntt_stage, four of load and finish.  The host build of the same butterfly runs in tests/test_ecntt_host.py."""
import os
import random
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import ecntt_cases as ec  # noqa: E402
from oracle import bn254  # noqa: E402

pytestmark = pytest.mark.gpu
R = bn254.R_MOD
CASES = [(k, name) for k in ec.KS for name in ec.case_ids(k)] + [(ec.K_WIDE, name) for name in ec.WIDE_FAMILIES]


def case_of(k, name):
    cases = ec.wide_families() if k == ec.K_WIDE else ec.families(k)
    return next(c for c in cases if c.name == name)


@pytest.mark.parametrize("k,name", CASES)
def test_derived_basis_matches_the_model(ctx, k, name):
    case = case_of(k, name)
    srs = ctx.srs_create(k, case.g)                     # no Lagrange basis supplied: derived on the device
    try:
        assert np.array_equal(srs.download_g(), case.g)
        got = srs.download_g_lagrange()
        bad = np.flatnonzero((got != case.expect).any(axis=1))
        assert bad.size == 0, (name, bad[:8])
    finally:
        srs.destroy()


@pytest.mark.parametrize("k", ec.KS + (ec.K_WIDE,))
def test_downsize_by_two_ignores_the_tail(ctx, cref, k):
    """zk_srs_downsize from k + 2 to k: the first 2^k points of g with the basis of the smaller domain; the other three quarters
    of the larger g (random points) and the larger Lagrange basis (random points too) must not matter"""
    n = 1 << k
    tail, other = cref.hash_to_curve_points(0xD0 + k, 3 * n), cref.hash_to_curve_points(0xD1 + k, 4 * n)
    for case in (ec.wide_families() if k == ec.K_WIDE else ec.families(k)):
        big = ctx.srs_create(k + 2, np.concatenate([case.g, tail]), other)
        small = big.downsize(k)
        try:
            assert small.k == k and np.array_equal(small.download_g(), case.g), case.name
            assert np.array_equal(small.download_g_lagrange(), case.expect), case.name
        finally:
            small.destroy()
            big.destroy()


@pytest.mark.parametrize("k", [1, 6])
def test_downsize_to_the_same_size_copies_and_to_zero_keeps_one_point(ctx, cref, k):
    """new_k == k hands the Lagrange basis through as it is -- a deliberately different one comes back, not the derived one;
    new_k == 0 is one point, its own Lagrange basis, an identity included"""
    n = 1 << k
    other = cref.hash_to_curve_points(0xC0 + k, n)
    for case in ec.families(k):
        assert not np.array_equal(other, case.expect)
        srs = ctx.srs_create(k, case.g, other)
        same, one = srs.downsize(k), srs.downsize(0)
        try:
            assert same.k == k and np.array_equal(same.download_g(), case.g) and np.array_equal(same.download_g_lagrange(), other), case.name
            assert one.k == 0 and np.array_equal(one.download_g(), case.g[:1]) and np.array_equal(one.download_g_lagrange(), case.g[:1]), case.name
        finally:
            for s_ in (same, one, srs):
                s_.destroy()
    assert not ec.families(k)[[c.name for c in ec.families(k)].index("zeros")].g[:1].any()       # one of them was the identity


@pytest.mark.parametrize("k", [6, ec.K_WIDE])
def test_commitments_agree_over_degenerate_bases(ctx, cref, k):
    """commit(coefficients) over g == commit_lagrange(evaluations) over the derived basis, and both are the point the basis
    implies: over root_of_unity(i), g[j] = omega^(i j) G, that is f(omega^i) G (the basis is G at i and identities elsewhere);
    over delta(0, c), g = (c G, O, O, ...), it is f(0) c G (every basis point is c/n G).  f random."""
    n = 1 << k
    rng = random.Random(0xC0 + k)
    roots = [c for c in (ec.wide_families() if k == ec.K_WIDE else ec.families(k)) if c.name.startswith("root_of_unity")]
    c0 = rng.randrange(1, R)
    todo = [(c, lambda f, i=c.a[1]: cref.eval_polynomial(f, i)) for c in roots]         # a[1] = omega^i
    todo.append((ec.delta(k, 0, c0), lambda f: cref.from_mont(f[:1])[0] * c0 % R))
    assert len(roots) == (2 if k == ec.K_WIDE else 4) and all(pow(c.a[1], n, R) == 1 for c in roots)
    for t, (case, value) in enumerate(todo):
        srs = ctx.srs_create(k, case.g)
        f = cref.rand_fr_stream(0xF00 + 16 * k + t, n)
        d = ctx.to_device(f)
        try:
            want = ec.points_of([value(f)])[0]
            assert want.any()
            assert np.array_equal(ctx.commit(srs, d, n), want), case.name
            ctx.ntt(d, k)
            assert np.array_equal(ctx.commit(srs, d, n, lagrange=True), want), case.name
        finally:
            d.free()
            srs.destroy()

"""GPU: zk_srs_setup_with_s (csrc/srs.hip: k_fb_mul over the 8-bit fixed-base table, k_lagrange_den / batch inversion /
k_lagrange_fin) at the toxic-waste values where its scalars degenerate -- s = 0, 1, r - 1, roots of unity of the domain, and
s = 2, 2^248, whose powers are mostly zero bytes -- against the big-int closed form

    g[i] = s^i G (0^0 = 1),     g_lagrange[i] = omega^i (s^n - 1) / (n (s - omega^i)) G     with 1/0 := 0.

1/0 := 0 is what the library's batch inversion computes, and halo2's unsafe_setup_with_s does the same.  For s^n = 1 the factor
s^n - 1 is zero as well, so the Lagrange basis comes out as ALL IDENTITIES.  That is NOT the true Lagrange basis of that g (which is
G at the index i with omega^i = s and identities elsewhere); zk_srs_create(k, g) without a basis derives the true one.  Both are
asserted here to pin the behaviour; it is not meant to change.  oracle/params_file.setup_with_s follows the same formula but
raises on the division by zero, so it is the reference wherever no denominator vanishes (checked for k <= 5)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import ecntt_cases as ec  # noqa: E402
from oracle import bn254 as b  # noqa: E402
from oracle import params_file  # noqa: E402

pytestmark = pytest.mark.gpu
R = b.R_MOD
KS = (0, 1, 5, 9)


def values_of_s(k):
    w = b.omega_for_k(k)
    return {"0": 0, "1": 1, "r-1": R - 1, "2": 2, "2^248": 1 << 248, "omega": w, "omega^3": pow(w, 3, R)}


def closed_form(k, s):
    n = 1 << k
    w = b.omega_for_k(k)
    powers = [pow(s, i, R) for i in range(n)]
    assert powers[0] == 1                                    # also for s = 0
    c = (pow(s, n, R) - 1) * b.fr_inv(n) % R
    inv0 = lambda v: pow(v, -1, R) if v else 0
    return powers, [pow(w, i, R) * c % R * inv0((s - pow(w, i, R)) % R) % R for i in range(n)]


def zero_bytes(v):
    return sum(1 for byte in v.to_bytes(32, "little") if byte == 0)


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("name", ["0", "1", "r-1", "2", "2^248", "omega", "omega^3"])
def test_setup_matches_the_closed_form(ctx, cref, k, name):
    n = 1 << k
    s = values_of_s(k)[name]
    powers, lag = closed_form(k, s)
    srs = ctx.srs_setup_with_s(k, cref.fr_const(s))
    try:
        g, gl = srs.download_g(), srs.download_g_lagrange()
    finally:
        srs.destroy()
    assert np.array_equal(g, ec.points_of(powers))
    assert np.array_equal(gl, ec.points_of(lag))
    # k_fb_mul skips a window whose byte is zero: these scalars are mostly such windows (canonical image, 32 bytes)
    sparse = [v for v in powers + lag if zero_bytes(v) >= 24]
    if name in ("0", "2", "2^248"):
        assert sparse and (k == 0 or len(sparse) >= 2)
        if name == "0":                                      # 1, then zeros: the scalar 0 skips all 32 windows
            assert powers[1:] == [0] * (n - 1) and lag == [b.fr_inv(n)] * n
        if name == "2" and k == 9:
            assert sum(1 for v in powers if zero_bytes(v) == 31) >= 253          # 2^i below r: one non-zero byte each
    if pow(s, n, R) == 1:
        assert name in ("1", "r-1", "omega", "omega^3") or k == 0
        assert not gl.any()                                  # all identities: 1/0 := 0 times s^n - 1 = 0 (see the module docstring)
        m = next(i for i in range(n) if pow(b.omega_for_k(k), i, R) == s)
        true = ec.root_of_unity(k, m).expect if k else g
        derived = ctx.srs_create(k, g)
        try:
            assert np.array_equal(derived.download_g_lagrange(), true)
        finally:
            derived.destroy()
        assert int(true.any(axis=1).sum()) == 1 and np.array_equal(true[m], cref.affine_to_mont([b.G1_GEN])[0])
    else:
        assert name in ("0", "2", "2^248") or (k == 0 and name != "1")
        assert all(v != 0 for v in lag)
        if k <= 5:                                           # no vanishing denominator: the oracle's setup is the same formula
            og, olag, _, _ = params_file.setup_with_s(k, s)
            assert cref.affine_from_mont(g) == og and cref.affine_from_mont(gl) == olag

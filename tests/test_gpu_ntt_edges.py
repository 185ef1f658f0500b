"""GPU: zk_ntt_omega (the transform over a caller's root) and its domain cache, and operands that are extreme as stored words, at
the sizes where the lazily reduced radix-4 steps are deepest (digits of 2^9 and 2^10, and three passes)."""
import numpy as np
import pytest

from oracle import bn254

pytestmark = pytest.mark.gpu
R = bn254.R_MOD


def roots_of(k):
    """omega^-1; omega^3 (still primitive); omega_(k+1)^2 (= omega: the same domain as zk_ntt's); omega_(k-1) (of order n/2)"""
    w = bn254.omega_for_k(k)
    return [("inverse", bn254.fr_inv(w)), ("cube", pow(w, 3, R)), ("square_of_next", pow(bn254.omega_for_k(k + 1), 2, R)), ("half_order", bn254.omega_for_k(k - 1))]


def butterflies_by_definition(a, w, k, outputs):
    """What best_fft's butterflies compute for ANY w with w^n = 1, at the output indices `outputs`: a butterfly subtracts where the
    definition multiplies by w^(n/2), so out[i] = sum_j (-1)^c a[j] w^(i j - c n/2) with c = sum_s bit_s(i) bit_(k-1-s)(j)
    subtractions on the way from a[j] to out[i].  For a primitive root w^(n/2) = -1 and this is the definition; for a root of
    order n/2 it is not (ntt_naive differs)."""
    n = 1 << k
    powers = [1] * n
    for e in range(1, n):
        powers[e] = powers[e - 1] * w % R
    out = []
    for i in outputs:
        acc = 0
        for j in range(n):
            c = bin(i & int(format(j, f"0{k}b")[::-1], 2)).count("1")
            acc += (-1) ** c * a[j] * powers[(i * j - c * (n // 2)) % n]
        out.append(acc % R)
    return out


def definition_rows(a, w, outputs):
    """bn254.ntt_naive, the definition out[i] = sum_j a[j] w^(i j), at the output indices `outputs` only"""
    return [sum(x * pow(w, i * j, R) for j, x in enumerate(a)) % R for i in outputs]


@pytest.mark.parametrize("k", [3, 10, 12, 14])
def test_ntt_omega_and_its_domains(zk, cref, k):
    """Four roots at one size in one context, interleaved with zk_ntt of the same size, then the first call again: every result is
    best_fft over that root, equals what the same call gives alone in a fresh context (the domain cache, keyed by a hash of
    (log_n, omega, scale), hands every root its own domain), and the repeated call is bit-identical.  At the small sizes, k = 3
    and 10, the results are also pinned to the O(n^2) sums: the definition (ntt_naive) for the three primitive roots, and
    best_fft's own sum for the root of order n/2 (every output at k = 3; at k = 10, 32 outputs, and all of them for one root).  For that root ntt_naive does NOT
    give the expected values: the transform is a port of best_fft, whose butterflies take omega^(n/2) = -1, so the definition
    out[i] = sum a[j] omega^(i j) holds for primitive roots only, in the oracle as on the device (include/zkmi355.h says so)."""
    n = 1 << k
    A = cref.rand_fr_stream(5150 + k, n)
    roots = roots_of(k)
    assert roots[2][1] == bn254.omega_for_k(k) and pow(roots[3][1], n // 2, R) == 1 and len({w for _, w in roots}) == 4

    def call(c, w):
        d = c.to_device(A)
        try:
            if w is None:
                c.ntt(d, k)
            else:
                c.ntt_omega(d, k, cref.fr_const(w))
            return d.download((n, 4))
        finally:
            d.free()

    shared = zk.Context(0)
    try:
        together = []
        for _, w in roots:
            together.append(call(shared, w))
            together.append(call(shared, None))
        again = call(shared, roots[0][1])
    finally:
        shared.close()
    assert np.array_equal(again, together[0])
    plain = cref.best_fft(A, bn254.omega_for_k(k), k)
    for j, (name, w) in enumerate(roots):
        assert np.array_equal(together[2 * j], cref.best_fft(A, w, k)), name
        assert np.array_equal(together[2 * j + 1], plain), name
        alone = zk.Context(0)
        try:
            assert np.array_equal(call(alone, w), together[2 * j]), name
        finally:
            alone.close()
    alone = zk.Context(0)
    try:
        assert np.array_equal(call(alone, None), plain)
    finally:
        alone.close()
    if k <= 10:
        a = cref.from_mont(A)
        outputs = list(range(n)) if k == 3 else [0, 1, 2, n // 2 - 1, n // 2, n // 2 + 1, n - 2, n - 1] + [int(i) for i in np.random.default_rng(k).integers(0, n, size=24)]
        for j, (name, w) in enumerate(roots):
            got = cref.from_mont(together[2 * j])
            assert [got[i] for i in outputs] == butterflies_by_definition(a, w, k, outputs), name
            rows = [got[i] for i in outputs]
            assert (rows == definition_rows(a, w, outputs)) == (name != "half_order"), name
            if k == 3 or name == "cube":        # a second of Python at k = 10: the whole of ntt_naive for one root there
                assert (got == bn254.ntt_naive(a, w)) == (name != "half_order"), name


def raw(value, n):
    """n copies of the stored word pattern `value` (four 64-bit limbs, low first): uploaded as it is, no to_mont"""
    return np.tile(np.array([(value >> (64 * i)) & (2 ** 64 - 1) for i in range(4)], dtype=np.uint64), (n, 1))


def extreme_column(cref, pattern, n):
    top = cref.to_mont([R - 1])
    if pattern == "max":                    # every element r - 1 as a field value
        return np.tile(top, (n, 1))
    if pattern == "alternating":            # 0, r - 1, 0, r - 1, ...
        A = np.zeros((n, 4), dtype=np.uint64)
        A[1::2] = top[0]
        return A
    if pattern == "raw_max":                # every stored word pattern r - 1
        return raw(R - 1, n)
    assert pattern == "raw_limbs_full"      # the largest stored pattern below r whose eight low 29-bit limbs are all 2^29 - 1
    v = (((R >> 232) - 1) << 232) | (2 ** 232 - 1)
    assert v < R < v + (1 << 232) and all((v >> (29 * i)) & (2 ** 29 - 1) == 2 ** 29 - 1 for i in range(8))
    return raw(v, n)


@pytest.mark.parametrize("k", [17, 19, 20, 21])
@pytest.mark.parametrize("pattern", ["max", "alternating", "raw_max", "raw_limbs_full"])
def test_extreme_operands_at_the_deepest_steps(ctx, cref, k, pattern):
    """Digits of 2^9 and 2^10 run five radix-4 steps between carry propagations (k = 17 .. 20), k = 21 three passes: operands that
    are extreme as field values and as stored Montgomery words (the 29-bit limb bounds of dit_step are about the words), forward
    against best_fft -- the oracle works on the stored form too -- and back, under the default kernels and under ZK_NTT_FIXED=0."""
    import os
    n = 1 << k
    A = extreme_column(cref, pattern, n)
    want = cref.best_fft(A, bn254.omega_for_k(k), k)
    for fixed in (None, "0"):
        if fixed is not None:
            os.environ["ZK_NTT_FIXED"] = fixed
        d = ctx.to_device(A)
        try:
            ctx.ntt(d, k)
            assert np.array_equal(d.download((n, 4)), want), fixed
            ctx.ntt(d, k, inverse=True)
            assert np.array_equal(d.download((n, 4)), A), fixed
        finally:
            d.free()
            os.environ.pop("ZK_NTT_FIXED", None)

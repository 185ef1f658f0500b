"""Shared by tests/test_ecntt_host.py and tests/test_gpu_g_to_lagrange.py: the inputs on which the group FFT behind
g_to_lagrange (csrc/ecntt.hip, butterfly in csrc/ec29.hip.hpp) meets identities, equal points and opposite points, and a
big-int model of it.

A case is a scalar vector a with g[j] = a[j] G, so every point's discrete logarithm is known and the expected Lagrange basis is
ifft(a)[i] G (oracle scalar multiplication, compared bit for bit on the affine Montgomery image; the identity is an all-zero row).
The model runs the kernels' schedule (bit-reversed load, radix-2 DIT stages s = 0 .. k-1 with w = omega^-(j << (k-1-s)), then 1/n)
on the logarithms and counts, per stage, how many of the 2 * n/2 additions u + (+-w v) double (both operands the same non-identity
point), cancel (opposite points) or have an identity operand.  Every builder asserts its own premise -- which additions are
exceptional, what the output looks like -- so a case cannot silently be a generic one.  `unknown_dlog` has no logarithms: its
expectation is n oracle MSMs."""
import functools
import random
from typing import List, NamedTuple, Optional, Tuple

import numpy as np

from oracle import bn254, cref

R = bn254.R_MOD
KS = (1, 2, 3, 6)                       # every family; one butterfly, one stage with a twiddle, ..., 32 butterflies a stage
K_WIDE = 10                             # 512 butterflies: two workgroups of k_ecntt_stage, four of load and finish
WIDE_FAMILIES = ("all_equal", "root_of_unity(1)", "root_of_unity(n-1)", "delta(n-1)", "odd_zero")
UNKNOWN_DLOG_MAX_K = 5


class Case(NamedTuple):
    name: str
    k: int
    a: Optional[List[int]]              # discrete logarithms, None for unknown_dlog
    g: np.ndarray                       # (n, 8) u64 affine Montgomery
    expect: np.ndarray                  # (n, 8) u64: the Lagrange basis
    counts: Optional[List[Tuple[int, int, int]]]     # per stage (doublings, cancellations, additions with an identity operand)


def omega_inv(k: int) -> int:
    return bn254.fr_inv(bn254.omega_for_k(k))


def model(a: List[int], k: int):
    """-> (ifft(a), per-stage counts) by the kernels' schedule on the logarithms"""
    n = 1 << k
    x = [0] * n
    for i, v in enumerate(a):
        x[bn254.bitrev(i, k) if k else 0] = v % R
    wi = omega_inv(k)
    tw = [pow(wi, j, R) for j in range(max(n // 2, 1))]
    counts = []
    for s in range(k):
        half, dbl, cancel, idop = 1 << s, 0, 0, 0
        for b in range(n // 2):
            j = b & (half - 1)
            i0 = ((b >> s) << (s + 1)) | j
            i1 = i0 + half
            u, wv = x[i0], x[i1] * tw[j << (k - 1 - s)] % R
            for q in (wv, (R - wv) % R):
                if u == 0 or q == 0:
                    idop += 1
                elif u == q:
                    dbl += 1
                elif (u + q) % R == 0:
                    cancel += 1
            x[i0], x[i1] = (u + wv) % R, (u - wv) % R
        counts.append((dbl, cancel, idop))
    ninv = bn254.fr_inv(n)
    return [v * ninv % R for v in x], counts


def points_of(a: List[int]) -> np.ndarray:
    """a[j] G as affine Montgomery rows (zero rows for a[j] = 0)"""
    gen = np.ascontiguousarray(np.repeat(cref.affine_to_mont([bn254.G1_GEN]), len(a), axis=0))
    out = cref.g1_mul(gen, cref.to_mont([v % R for v in a]))
    zero = [i for i, v in enumerate(a) if v % R == 0]
    assert not out[zero].any() and out.any(axis=1).sum() == len(a) - len(zero)      # the oracle's identity is the zero row, and only it
    return out


def _case(name: str, k: int, a: List[int]) -> Case:
    assert len(a) == 1 << k
    out, counts = model(a, k)
    assert out == cref.from_mont(cref.ifft(cref.to_mont(a), k)) if k else out == [a[0] % R]
    return Case(name, k, [v % R for v in a], points_of(a), points_of(out), counts)


def identities(c: Case) -> int:
    return int((~c.expect.any(axis=1)).sum())


def all_equal(k: int, c: int, name: str = "all_equal") -> Case:
    """stage 0 is u + v with u == v (n/2 doublings) and u - v (n/2 identities); from there identities meet identities"""
    n = 1 << k
    case = _case(name, k, [c] * n)
    assert case.counts[0] == (n // 2, n // 2, 0) and all(cn[0] == n >> (s + 1) for s, cn in enumerate(case.counts))
    assert all(cn[2] > 0 for cn in case.counts[1:]) and identities(case) == n - 1
    assert np.array_equal(case.expect[0], points_of([c])[0])
    return case


def root_of_unity(k: int, i: int, name: Optional[str] = None) -> Case:
    """a[j] = omega^(i j).  After every stage each block holds one non-identity point (the DFT of a character is a delta), so in
    every stage exactly n / 2^(s+1) butterflies combine u and w v with u == w v or u == -(w v): one doubling and one cancellation
    each, at j = i mod 2^s -- for odd i a j != 0, where w v is the output of a scalar multiplication and u that of additions, two
    different XYZZ representations.  Expected: G at i, n - 1 identities."""
    n = 1 << k
    w = bn254.omega_for_k(k)
    case = _case(name or f"root_of_unity({i})", k, [pow(w, i * j, R) for j in range(n)])
    assert case.counts == [(n >> (s + 1), n >> (s + 1), 2 * (n // 2) - 2 * (n >> (s + 1))) for s in range(k)]
    if k >= 2 and i % 2:
        assert any(cn[0] > 0 and cn[1] > 0 for cn in case.counts[1:])
    assert identities(case) == n - 1 and np.array_equal(case.expect[i % n], cref.affine_to_mont([bn254.G1_GEN])[0])
    return case


def delta(k: int, m: int, c: int, name: Optional[str] = None) -> Case:
    """one non-identity input: every addition has an identity operand; expected c omega^(-i m) / n G, all equal for m = 0"""
    n = 1 << k
    case = _case(name or f"delta({m})", k, [c if j == m else 0 for j in range(n)])
    assert all(cn == (0, 0, 2 * (n // 2)) for cn in case.counts) and identities(case) == 0
    if m == 0:
        assert (case.expect == case.expect[0]).all()
    return case


def zeros(k: int) -> Case:
    case = _case("zeros", k, [0] * (1 << k))
    assert not case.g.any() and not case.expect.any()
    return case


def halves(k: int, sign: int, rng: random.Random) -> Case:
    """g[j + n/2] = +-g[j], g[j] random: stage 0 pairs them, so its n/2 butterflies double in one output and cancel in the other"""
    n = 1 << k
    lo = [rng.randrange(1, R) for _ in range(n // 2)]
    case = _case("halves(+)" if sign > 0 else "halves(-)", k, lo + [sign * v % R for v in lo])
    assert case.counts[0] == (n // 2, n // 2, 0)
    assert np.array_equal(case.g[n // 2:, :4], case.g[:n // 2, :4]) and np.array_equal(case.g[n // 2:, 4:], case.g[:n // 2, 4:]) == (sign > 0)
    return case


def odd_zero(k: int, rng: random.Random) -> Case:
    """a[j] = 0 for odd j: the second half of the basis repeats the first"""
    n = 1 << k
    case = _case("odd_zero", k, [rng.randrange(1, R) if j % 2 == 0 else 0 for j in range(n)])
    assert np.array_equal(case.expect[:n // 2], case.expect[n // 2:]) and case.counts[-1][2] == 2 * (n // 2)
    return case


def random_case(k: int, rng: random.Random) -> Case:
    """the control: no exceptional addition anywhere"""
    case = _case("random", k, [rng.randrange(1, R) for _ in range(1 << k)])
    assert all(cn == (0, 0, 0) for cn in case.counts)
    return case


def unknown_dlog(k: int) -> Case:
    """hash-to-curve points; expectation by n oracle MSMs with scalars omega^(-i j) / n: no scalar is shared with the code under test"""
    assert k <= UNKNOWN_DLOG_MAX_K
    n = 1 << k
    g = cref.hash_to_curve_points(0xEC0 + k, n)
    wi, ninv = omega_inv(k), bn254.fr_inv(n)
    expect = np.stack([cref.best_multiexp(cref.to_mont([pow(wi, i * j, R) * ninv % R for j in range(n)]), g) for i in range(n)])
    assert g.any(axis=1).all() and len({r.tobytes() for r in g}) == n
    return Case("unknown_dlog", k, None, g, expect, None)


def _distinct(pairs):
    """(name, index) pairs without the indices that repeat an earlier one (small n)"""
    seen, out = set(), []
    for name, i in pairs:
        if i not in seen:
            out.append((name, i))
            seen.add(i)
    return out


def _roots(n: int):
    return _distinct([("root_of_unity(1)", 1), ("root_of_unity(n/2)", n // 2), ("root_of_unity(n-1)", n - 1), ("root_of_unity(3)", 3 % n)])


def _deltas(n: int):
    return _distinct([("delta(0)", 0), ("delta(1)", 1), ("delta(n-1)", n - 1)])


def case_ids(k: int) -> List[str]:
    """names of families(k), without building them (for parametrize)"""
    n = 1 << k
    names = ["all_equal", "all_equal(s=1)"] + [nm for nm, _ in _roots(n)] + [nm for nm, _ in _deltas(n)]
    names += ["zeros", "halves(+)", "halves(-)", "odd_zero", "random"]
    return names + (["unknown_dlog"] if k <= UNKNOWN_DLOG_MAX_K else [])


def _frozen(cases) -> Tuple[Case, ...]:
    for c in cases:
        c.g.setflags(write=False)
        c.expect.setflags(write=False)
    return tuple(cases)


@functools.lru_cache(maxsize=None)
def families(k: int) -> Tuple[Case, ...]:
    """every family at size 2^k (computed once, shared, read-only)"""
    rng = random.Random(0xECF0 + k)
    n = 1 << k
    cases = [all_equal(k, rng.randrange(2, R)), all_equal(k, 1, "all_equal(s=1)")]
    cases += [root_of_unity(k, i, name) for name, i in _roots(n)]
    cases += [delta(k, m, rng.randrange(1, R), name) for name, m in _deltas(n)]
    cases += [zeros(k), halves(k, 1, rng), halves(k, -1, rng), odd_zero(k, rng), random_case(k, rng)]
    if k <= UNKNOWN_DLOG_MAX_K:
        cases.append(unknown_dlog(k))
    assert [c.name for c in cases] == case_ids(k)
    return _frozen(cases)


@functools.lru_cache(maxsize=None)
def wide_families() -> Tuple[Case, ...]:
    """the families of WIDE_FAMILIES at k = 10"""
    k, n = K_WIDE, 1 << K_WIDE
    rng = random.Random(0xECF0 + k)
    cases = (all_equal(k, rng.randrange(2, R)), root_of_unity(k, 1, "root_of_unity(1)"), root_of_unity(k, n - 1, "root_of_unity(n-1)"),
             delta(k, n - 1, rng.randrange(1, R), "delta(n-1)"), odd_zero(k, rng))
    assert tuple(c.name for c in cases) == WIDE_FAMILIES
    return _frozen(cases)

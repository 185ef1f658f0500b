"""CPU: zk_host_accumulator_from_limbs, the host-only inverse of zk_host_accumulator_limbs (LimbsEncoding::from_repr as the
aggregation layers read an accumulator off a child snark's instances [REF aggregator/src/core.rs:120-135]).
  * it inverts zk_host_accumulator_limbs on random accumulators;
  * on the limbs the reference's own ChunkProof carries at its protocol's accumulator_indices it gives the oracle's
    accumulator_from_limbs, and that accumulator passes zk_host_accumulator_check under the fixture's s_g2;
  * a limb of 2^88 or more, a coordinate of p or more, a point off the curve, a cell that is no canonical Fr: ok = 0, points zeroed."""
import ctypes
import os
import random
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import zkevm_circuits_amd as z  # noqa: E402
from oracle import bn254 as b  # noqa: E402
from oracle import pairing as pr  # noqa: E402
from oracle import params_file  # noqa: E402
from oracle import snark_verifier as sv  # noqa: E402
from test_reference_chunk_proof import fx  # noqa: E402,F401

R, P = b.R_MOD, b.P_MOD
BITS = 88


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _limbs_of(acc):
    """the oracle's side of the encoding: [lhs.x, lhs.y, rhs.x, rhs.y] in 3 little-endian limbs of 88 bits"""
    return [(c >> (BITS * i)) & ((1 << BITS) - 1) for pt in acc for c in pt for i in range(3)]


def _decode(cref, limbs):
    lhs, rhs, ok = z.accumulator_from_limbs(cref.to_mont(list(limbs)))
    return lhs, rhs, ok


def test_from_limbs_inverts_limbs_on_random_accumulators(cref):
    rng = random.Random(88)
    for _ in range(16):
        acc = (b.g1_mul(b.G1_GEN, rng.randrange(1, R)), b.g1_mul(b.G1_GEN, rng.randrange(1, R)))
        lm, rm = cref.affine_to_mont([acc[0]]), cref.affine_to_mont([acc[1]])
        cells = np.zeros((12, 4), dtype=np.uint64)
        assert z.lib().zk_host_accumulator_limbs(_ptr(lm), _ptr(rm), _ptr(cells)) == 0
        assert cref.from_mont(cells) == _limbs_of(acc)
        lhs, rhs, ok = z.accumulator_from_limbs(cells)
        assert ok and np.array_equal(lhs, lm.reshape(8)) and np.array_equal(rhs, rm.reshape(8))


def test_reference_chunk_proof_accumulator(cref, fx):  # noqa: F811
    assert fx.protocol.accumulator_indices, "the fixture's protocol lists accumulator_indices"
    g2 = np.frombuffer(params_file.g2_raw_bytes(pr.G2_GEN), dtype=np.uint64).copy()
    s_g2 = np.frombuffer(params_file.g2_raw_bytes(fx.s_g2), dtype=np.uint64).copy()
    for indices in fx.protocol.accumulator_indices:
        limbs = [fx.instances[c][r] for c, r in indices]
        want = sv.accumulator_from_limbs(limbs)
        lhs, rhs, ok = _decode(cref, limbs)
        assert ok
        assert cref.affine_from_mont(np.stack([lhs, rhs])) == [want[0], want[1]]
        verdict = ctypes.c_int(-1)
        assert z.lib().zk_host_accumulator_check(_ptr(lhs), _ptr(rhs), _ptr(g2), _ptr(s_g2), ctypes.byref(verdict)) == 0
        assert verdict.value == 1


def _malformed_cases():
    rng = random.Random(7)
    acc = (b.g1_mul(b.G1_GEN, rng.randrange(1, R)), b.g1_mul(b.G1_GEN, rng.randrange(1, R)))
    good = _limbs_of(acc)
    cases = {}
    for cell in (0, 4, 8, 11):                      # a limb of 2^88 or more (also with the low 88 bits unchanged)
        bad = list(good)
        bad[cell] += 1 << BITS
        cases[f"limb {cell} + 2^88"] = bad
    bad = list(good)
    bad[1] = 1 << BITS
    cases["limb 1 = 2^88"] = bad
    for coord in range(4):                           # a coordinate of p or more: x + p still fits 3 limbs of 88 bits
        v = acc[coord // 2][coord % 2] + P
        if v >> (3 * BITS) == 0 and all(((v >> (BITS * i)) & ((1 << BITS) - 1)) < (1 << BITS) for i in range(3)):
            bad = list(good)
            bad[3 * coord:3 * coord + 3] = [(v >> (BITS * i)) & ((1 << BITS) - 1) for i in range(3)]
            cases[f"coordinate {coord} + p"] = bad
    top = list(good)                                 # 2^256 <= coordinate < 2^264: the top limb uses its bits 80..87
    top[2] |= 1 << 87
    cases["coordinate beyond 2^256"] = top
    off = list(good)                                 # not on the curve
    off[0] ^= 1
    cases["lhs off the curve"] = off
    off = list(good)
    off[9] ^= 1
    cases["rhs off the curve"] = off
    cases["identity"] = [0] * 12
    return good, cases


def test_malformed_limbs_give_ok_0(cref):
    good, cases = _malformed_cases()
    assert _decode(cref, good)[2]
    assert any(k.startswith("coordinate") and k.endswith("+ p") for k in cases)
    for what, limbs in cases.items():
        cells = cref.to_mont([v % R for v in limbs])
        # values of 2^88 and beyond are still canonical Fr cells (2^88 << r): the cell holds exactly the limb
        assert cref.from_mont(cells) == [v % R for v in limbs] == list(limbs), what
        lhs, rhs, ok = z.accumulator_from_limbs(cells)
        assert not ok, what
        assert not lhs.any() and not rhs.any(), what
        with pytest.raises(AssertionError):
            sv.accumulator_from_limbs(limbs)
    # a cell whose Montgomery limbs are not below r
    cells = cref.to_mont(good)
    cells[5] = np.array([0xFFFFFFFFFFFFFFFF] * 4, dtype=np.uint64)
    assert not z.accumulator_from_limbs(cells)[2]


def test_null_arguments_are_refused():
    cells = np.zeros((12, 4), dtype=np.uint64)
    out = np.zeros(8, dtype=np.uint64)
    ok = ctypes.c_int(-1)
    assert z.lib().zk_host_accumulator_from_limbs(None, _ptr(out), _ptr(out), ctypes.byref(ok)) == -1
    assert z.lib().zk_host_accumulator_from_limbs(_ptr(cells), _ptr(out), _ptr(out), None) == -1

"""The signed-digit recoding of the MSM (csrc/msm.hip: recode_wide for the merged-window path, recode_all / k_msm_digits for the
per-window path) restated in Python and run over the scalar families of msm_scalars.py, for every plan the library makes: the
digits must rebuild the scalar, no digit may exceed 2^(c-1) in magnitude (the top one included, after its carry and its
top_shift), and the families must really reach the edges the GPU tests rely on them to reach."""
import ctypes
import random

import pytest

from msm_scalars import R_MOD, families, plan_top_max, top_digit_max
from zkevm_circuits_amd import binding

CODE_ZERO = 0xFFFFFFFF          # recode_wide: zero digit; else bit 31 = sign, low bits = |d| - 1
NEG_BIT = 0x80000000
DIG_ZERO = 0xFFFF               # recode_all (k_msm_digits, u16): zero digit; else bit 15 = sign, low 15 bits = |d| - 1
DIG_NEG = 0x8000


def recode(s: int, c: int, W: int, top_shift: int, zero: int, neg: int):
    """Window codes of s as the kernels write them, and the digit each window saw after the carry of the one below (before the
    top window's shift).  A carry out of the top window is dropped, as in the kernels."""
    mask, half = (1 << c) - 1, 1 << (c - 1)
    carry, codes, raw = 0, [], []
    for w in range(W):
        d = ((s >> (c * w)) & mask) + carry
        raw.append(d)
        if w == W - 1:
            d <<= top_shift
        if d > half:
            carry, mag = 1, (1 << c) - d
            codes.append(neg | (mag - 1) if mag else zero)
        else:
            carry = 0
            codes.append(d - 1 if d else zero)
    return codes, raw


def decode(code: int, c: int, zero: int, neg: int) -> int:
    if code == zero:
        return 0
    mag = (code & ~neg) + 1
    assert mag <= 1 << (c - 1), f"bucket index {mag - 1} beyond the 2^(c-1) buckets of c = {c}"
    return -mag if code & neg else mag


def check_family_set(c: int, W: int, top_shift: int, zero: int, neg: int, fams: dict):
    """Assert the recoding invariants over every scalar of `fams`; returns which edges were met."""
    half = 1 << (c - 1)
    top_weight = c * (W - 1) - top_shift
    seen = {"half": False, "half_plus_one": False, "two_to_c": False, "top": set()}
    for name, vals in fams.items():
        for s in vals:
            codes, raw = recode(s, c, W, top_shift, zero, neg)
            digits = [decode(x, c, zero, neg) for x in codes]
            assert all(abs(d) <= half for d in digits), (c, W, top_shift, name, hex(s))
            assert digits[-1] >= 0, f"c = {c}, top_shift = {top_shift}: the top digit of {name} {hex(s)} went negative (its carry is lost)"
            rebuilt = sum(d << (c * w) for w, d in enumerate(digits[:-1])) + (digits[-1] << top_weight)
            assert rebuilt == s, f"c = {c}, W = {W}, top_shift = {top_shift}: {name} {hex(s)} rebuilds as {hex(rebuilt)}"
            seen["half"] |= half in raw[:-1]
            seen["half_plus_one"] |= (half + 1) in raw[:-1]
            seen["two_to_c"] |= (1 << c) in raw[:-1]
            seen["top"].add(raw[-1])
    return seen


def assert_edges(c: int, W: int, seen: dict, fams: dict):
    tmax = top_digit_max(c, W)
    assert seen["half"], f"c = {c}: no window at exactly 2^(c-1)"
    assert seen["half_plus_one"], f"c = {c}: no window at 2^(c-1) + 1"
    assert seen["two_to_c"], f"c = {c}: no all-ones window receiving a carry (d = 2^c)"
    assert max(seen["top"]) == tmax, f"c = {c}: top digits reach {max(seen['top'])}, the attainable maximum is {tmax}"
    fam_top = {recode(s, c, W, 0, CODE_ZERO, NEG_BIT)[1][-1] for s in fams["top_carry"]}
    assert fam_top == {tmax}, f"c = {c}: top_carry reaches {sorted(fam_top)}, not only {tmax}"
    # both ways of reaching it: through a carry from below (leading bits tmax - 1) and, where it exists, without one
    low = c * (W - 1)
    via = {(s >> low) for s in fams["top_carry"]}
    if tmax >= 1:
        assert tmax - 1 in via, f"c = {c}: no top_carry scalar reaches {tmax} through a carry"
    if tmax <= (R_MOD - 1) >> low:
        assert tmax in via, f"c = {c}: no top_carry scalar reaches {tmax} without a carry"
    # top_only is empty exactly where no canonical scalar has a non-zero leading part
    assert bool(fams["top_only"]) == ((R_MOD - 1) >> low >= 1), c
    assert all(s >> low and not s & ((1 << low) - 1) for s in fams["top_only"])
    assert all(1 <= s <= 1 << (c - 1) for s in fams["low_only"])


def _host_plan(lib, k):
    c, w, sh = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    assert lib.zk_host_msm_plan(ctypes.c_uint32(k), ctypes.byref(c), ctypes.byref(w), ctypes.byref(sh)) == 0
    return c.value, w.value, sh.value


def test_merged_plan_recoding_every_top_shift(monkeypatch):
    """recode_wide over every merged-window plan (k = 0 .. 28: c = 8 .. 22) and every top_shift the plan allows, each one also
    forced through ZK_MSM_TOP_SHIFT (the measurement knob the GPU tests flip); values above the plan's maximum are ignored."""
    lib = binding.lib()
    for var in ("ZK_MSM_C", "ZK_MSM_TOP_SHIFT"):
        monkeypatch.delenv(var, raising=False)
    plans = {}
    for k in range(29):
        plans.setdefault(_host_plan(lib, k), []).append(k)
    assert sorted({c for c, _, _ in plans}) == list(range(8, 23))
    for (c, W, sh_max), ks in plans.items():
        assert plan_top_max(c, W) << sh_max <= 1 << (c - 1)
        assert top_digit_max(c, W) <= plan_top_max(c, W), f"c = {c}: a top digit beyond the plan's bound"
        fams = families(c, W, sh_max, None, random.Random(c))
        for sh in range(sh_max + 1):
            monkeypatch.setenv("ZK_MSM_TOP_SHIFT", str(sh))
            assert _host_plan(lib, ks[0]) == (c, W, sh)
            seen = check_family_set(c, W, sh, CODE_ZERO, NEG_BIT, fams)
            assert_edges(c, W, seen, fams)
        monkeypatch.setenv("ZK_MSM_TOP_SHIFT", str(sh_max + 1))
        assert _host_plan(lib, ks[0]) == (c, W, sh_max)
        monkeypatch.delenv("ZK_MSM_TOP_SHIFT")


def test_merged_plan_window_knob(monkeypatch):
    """ZK_MSM_C picks the window size of the merged plan (8 .. 22, others ignored); the top_shift follows the window size."""
    lib = binding.lib()
    monkeypatch.delenv("ZK_MSM_TOP_SHIFT", raising=False)
    natural = {max(8, min(k, 22)): _host_plan(lib, k) for k in range(8, 23)}
    for c in range(8, 23):
        monkeypatch.setenv("ZK_MSM_C", str(c))
        assert _host_plan(lib, 12) == natural[c]
    for bad in ("7", "23", "0"):
        monkeypatch.setenv("ZK_MSM_C", bad)
        assert _host_plan(lib, 12) == natural[12]


@pytest.mark.parametrize("c", range(4, 17))
def test_per_window_plan_digit_codes(c):
    """k_msm_digits (recode_all, make_plan(n): c = clamp(log2 n - 4, 4, 16), no top shift) writes u16 codes: 0xFFFF for a zero
    digit, bit 15 the sign, |d| - 1 below; a non-zero digit never collides with 0xFFFF, and the top digit never goes negative."""
    W = (256 + c - 1) // c
    fams = families(c, W, 0, None, random.Random(100 + c))
    seen = check_family_set(c, W, 0, DIG_ZERO, DIG_NEG, fams)
    assert_edges(c, W, seen, fams)
    for vals in fams.values():
        for s in vals:
            codes, _ = recode(s, c, W, 0, DIG_ZERO, DIG_NEG)
            assert all(0 <= x <= 0xFFFF for x in codes)
            assert all((x == DIG_ZERO) == (decode(x, c, DIG_ZERO, DIG_NEG) == 0) for x in codes)

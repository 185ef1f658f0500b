"""Scalar families for the MSM tests, built per window plan so that the signed-digit recoding meets its edges.

The recoding (csrc/msm.hip: recode_wide, recode_all) reads a canonical scalar in W windows of c bits, lowest first; a window
digit d (plus the carry of the window below) above half = 2^(c-1) becomes d - 2^c and carries 1 into the next window; the top
window never goes negative.  The families below put windows at exactly half, at half + 1, at 2^c after a carry (an all-ones
window: the digit is zero and the carry moves on) and the top digit at the largest value a canonical scalar can give it.

Plain Python, no GPU: the CPU test (test_msm_recoding.py) checks that the families hit these edges, the GPU tests
(test_gpu_msm_paths.py) commit them."""
import random

R_MOD = 0x30644e72e131a029b85045b68181585d2833e84879b9709143e1f593f0000001


def canonical(x: int) -> int:
    """x with leading set bits cleared until it is below r (constructions that come out >= r)."""
    while x >= R_MOD:
        x &= ~(1 << (x.bit_length() - 1))
    return x


def carry_threshold(c: int, W: int) -> int:
    """The low c (W - 1) bits of a scalar carry into the top window exactly when they exceed this value: digits in
    (-half, half] over W - 1 windows represent [-(half - 1) S, half S] with S = sum 2^(c w), and the largest of them is half S."""
    return (1 << (c - 1)) * sum(1 << (c * w) for w in range(W - 1))


def top_digit(s: int, c: int, W: int) -> int:
    """The top window's digit of s (before any top_shift): its leading bits plus the carry of the windows below."""
    low = c * (W - 1)
    return (s >> low) + (1 if (s & ((1 << low) - 1)) > carry_threshold(c, W) else 0)


def top_digit_max(c: int, W: int) -> int:
    """The largest top digit any canonical scalar reaches (exact, by big integers): (r - 1) >> low plus one only if r - 1's own
    low bits carry -- otherwise r - 1 itself (no carry) and (((r - 1) >> low) - 1, carry) tie at (r - 1) >> low."""
    low = c * (W - 1)
    hmax = (R_MOD - 1) >> low
    return hmax + 1 if ((R_MOD - 1) & ((1 << low) - 1)) > carry_threshold(c, W) else hmax


def plan_top_max(c: int, W: int) -> int:
    """The plan's bound on the top digit (csrc/msm.hip make_plan_merged): the leading bits of r - 1 plus a carry."""
    low = c * (W - 1)
    return ((R_MOD - 1) >> low) + 1 if low < 254 else 1


def _tile(vals, n):
    if n is None or not vals:
        return list(vals)
    return [vals[i % len(vals)] for i in range(n)]


def families(c: int, W: int, top_shift: int, n, rng: random.Random) -> dict:
    """Named lists of canonical scalars for a plan of W windows of c bits whose top digit is scaled by 2^top_shift (the
    families do not depend on the shift; the scaled maximum must stay <= 2^(c-1), which the plan guarantees).  Every list is
    tiled (cycled) to n entries; n = None keeps the distinct values only.  A family that no canonical scalar can realise for
    this plan (`top_only` where the top window of every canonical scalar is zero) is an empty list."""
    half = 1 << (c - 1)
    low = c * (W - 1)
    assert (top_digit_max(c, W) << top_shift) <= half, (c, W, top_shift)
    fam = {
        "zero": [0],
        "one": [1],
        "r_minus_1": [R_MOD - 1],
        "r_minus_2": [R_MOD - 2],
        "one_hot": [1 << b for b in range(254)],
    }
    # every window at half (no window carries) -- all windows at once, and one window at a time; the top window of the
    # all-windows scalar is cut back by canonical() (r < 2^254)
    fam["half"] = [canonical(sum(half << (c * w) for w in range(W)))] + [canonical(half << (c * w)) for w in range(W)]
    # half + 1 goes negative and carries: all windows at once (the carry lifts the windows above to half + 2), and one at a time
    fam["half_plus_one"] = [canonical(sum((half + 1) << (c * w) for w in range(W)))] + [canonical((half + 1) << (c * w)) for w in range(W)]
    # 2^(c j) - 1: window 0 is all ones (-1, carry), windows 1 .. j-1 receive the carry as 2^c (zero digit, carry on), window j
    # takes 1; the longest chains exceed r and lose leading bits to canonical()
    fam["all_ones_runs"] = [canonical((1 << (c * j)) - 1) for j in range(1, W)]
    # the top digit at its attainable maximum, reached through a carry from below and without one
    tmax = top_digit_max(c, W)
    T = carry_threshold(c, W)
    lows = [0, T, T + 1, (1 << low) - 1, (R_MOD - 1) & ((1 << low) - 1), T + 1 + rng.randrange(max((1 << low) - T - 1, 1))]
    tc = []
    for hi in (tmax - 1, tmax):
        for lo in lows:
            s = (hi << low) | (lo & ((1 << low) - 1))
            if hi >= 0 and s < R_MOD and top_digit(s, c, W) == tmax and s not in tc:
                tc.append(s)
    fam["top_carry"] = tc
    # only the top window non-zero (leading bits only, no carry from below)
    hmax = (R_MOD - 1) >> low
    fam["top_only"] = sorted({h << low for h in [1, hmax] + [rng.randrange(1, hmax + 1) for _ in range(6)]}) if hmax >= 1 else []
    # only window 0 non-zero: digits 1 .. half never carry, every other window is empty
    fam["low_only"] = [1, half] + [rng.randrange(1, half + 1) for _ in range(30)]
    fam["all_equal"] = [rng.randrange(1, R_MOD)]
    fam["boolean"] = [rng.randrange(2) for _ in range(64)]
    fam["sparse"] = [rng.randrange(1, R_MOD) if rng.random() < 0.05 else 0 for _ in range(400)]
    fam["random"] = [rng.randrange(R_MOD) for _ in range(256)]
    for name, vals in fam.items():
        assert all(0 <= v < R_MOD for v in vals), name
    return {name: _tile(vals, n) for name, vals in fam.items()}

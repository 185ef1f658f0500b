"""CPU: the limb routine of the row RLC (csrc/ff29.hip.hpp: rlc29_mac / rlc29_carry / rlc29_reduce -- a sum of short integer products
in 64-bit column sums under ONE Montgomery reduction) compiled for the host as a stand-alone program (tests/host_row_rlc_harness.hip)
and compared with Python integers: the result of every case is canonical and equals (c + sum_j w_j x_j) 2^256 mod p, its limbs are
normalised and below 2p, and the carry passes that keep the column sums inside 64 bits happen when the bound says they must.  The
program is built twice, plain and with the address and undefined-behaviour sanitizers, and run directly."""
import os
import random
import shutil
import subprocess

import pytest

from oracle import bn254 as o

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = o.R_MOD                                  # the scalar field Fr
R256, R261, R517 = (1 << 256) % P, (1 << 261) % P, (1 << 517) % P
M29 = (1 << 29) - 1
LIMBS = {1: 1, 2: 1, 4: 2, 8: 3, 16: 5, 32: 9}
MAX_LOAD = 54                                # RLC29_MAX_LOAD: (54 + 9) 2^58 + 2^36 < 2^64
WIDTHS = (1, 2, 4, 8, 16, 32)


def top(width):
    """the largest cell: all ones for a narrow width, the Montgomery image of p - 1 for a field element"""
    return (1 << (8 * width)) - 1 if width < 32 else (P - 1) * R256 % P


def make_cases():
    """[(name, c, [(width, cell, w)])]: cell is the stored integer (a width-32 cell is a canonical Montgomery image), w and c plain"""
    rng = random.Random(0x520C)
    cases = [
        ("64 x 16-byte all-ones, weights p-1", P - 1, [(16, top(16), P - 1)] * 64),
        ("64 x Fr p-1, weights p-1", P - 1, [(32, top(32), P - 1)] * 64),
        ("64 x Fr largest stored value, weights p-1", P - 1, [(32, P - 1, P - 1)] * 64),
        ("64 bytes of 255", 0, [(1, 255, rng.randrange(P)) for _ in range(64)]),
        ("64 bytes of 255, weights p-1", P - 1, [(1, 255, P - 1)] * 64),
        ("all six widths", rng.randrange(P), [(w, rng.randrange(top(w) + 1) if w < 32 else rng.randrange(P), rng.randrange(P)) for w in WIDTHS * 3]),
        ("all six widths, largest cells", P - 1, [(w, top(w), P - 1) for w in WIDTHS * 10]),
        ("zero weights", 5, [(w, top(w), 0) for w in WIDTHS]),
        ("zero weights and constant", 0, [(w, top(w), 0) for w in WIDTHS]),
        ("zero cells", 7, [(w, 0, rng.randrange(P)) for w in WIDTHS]),
        ("count 0", rng.randrange(P), []),
        ("count 0, constant 0", 0, []),
        ("count 0, constant p-1", P - 1, []),
    ]
    for i in range(40):
        count = rng.choice([1, 2, 7, 33, 64])
        cols = []
        for _ in range(count):
            w = rng.choice(WIDTHS)
            cell = rng.choice([0, top(w), rng.randrange(top(w) + 1) if w < 32 else rng.randrange(P)])
            cols.append((w, cell, rng.choice([0, 1, P - 1, rng.randrange(P)])))
        cases.append((f"random {i}", rng.choice([0, P - 1, rng.randrange(P)]), cols))
    return cases


CASES = make_cases()


def expected(c, cols):
    """(c + sum w x) 2^256 mod p, x the plain value of the cell"""
    inv = pow(R256, -1, P)
    return (c + sum(w * (cell if width < 32 else cell * inv) for width, cell, w in cols)) * R256 % P


def carry_passes(cols):
    load, passes = 1, 0
    for width, _, _ in cols:
        if load + LIMBS[width] > MAX_LOAD:
            load, passes = 1, passes + 1
        load += LIMBS[width]
    return passes


def case_file(path):
    with open(path, "w") as f:
        for _, c, cols in CASES:
            f.write(f"case {len(cols)}\n{c * R517 % P:x}\n")
            for width, cell, w in cols:
                f.write(f"{width} {cell:x} {w * (R261 if width == 32 else R517) % P:x}\n")


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def outputs(request, tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    d = tmp_path_factory.mktemp("row_rlc_" + request.param)
    exe, cases = str(d / "host_row_rlc"), str(d / "cases.txt")
    flags = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all", "-g"] if request.param == "sanitized" else []
    subprocess.run([hipcc, "--cuda-host-only", "-O2", "-std=c++17", *flags, os.path.join(ROOT, "tests", "host_row_rlc_harness.hip"), "-o", exe], check=True, timeout=300)
    case_file(cases)
    run = subprocess.run([exe, cases], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stderr
    lines = run.stdout.splitlines()
    assert len(lines) == len(CASES)
    return [ln.split() for ln in lines]


def test_every_case_is_canonical_and_equal(outputs):
    for (name, c, cols), fields in zip(CASES, outputs):
        got = int(fields[0], 16)
        assert got < P, name
        assert got == expected(c, cols), name


def test_limbs_are_normalised_and_below_2p(outputs):
    for (name, c, cols), fields in zip(CASES, outputs):
        limbs = [int(x, 16) for x in fields[1:10]]
        assert all(x <= M29 for x in limbs[:8]), name
        v = sum(x << (29 * i) for i, x in enumerate(limbs))
        assert v < 2 * P and v % P == expected(c, cols), name


def test_carry_passes_follow_the_column_bound(outputs):
    for (name, _, cols), fields in zip(CASES, outputs):
        assert int(fields[10]) == carry_passes(cols), name
    by_name = {name: int(fields[10]) for (name, _, _), fields in zip(CASES, outputs)}
    assert by_name["64 x 16-byte all-ones, weights p-1"] == 6 and by_name["64 x Fr p-1, weights p-1"] == 12      # every 10 / every 5 terms
    assert by_name["64 bytes of 255"] == 1                                                                       # bytes: after 53 terms


def test_the_edge_cases_sit_where_the_bounds_say():
    """T < 2^261 p for 64 full-size terms and the constant; a column of MAX_LOAD products leaves room for the reduction's nine"""
    assert 64 * (P - 1) * (P - 1) + (P - 1) < (1 << 261) * P
    assert 170 * (P - 1) * (P - 1) > (1 << 261) * P > 169 * (P - 1) * (P - 1)      # Fr; the base field admits 147
    assert (MAX_LOAD + 9) * (M29 * M29) + (1 << 36) < 1 << 64

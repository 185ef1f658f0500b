"""CPU: the row step and the chunk fold of the typed running RLC (csrc/ff29.hip.hpp: scan_rlc29_step -- z <- (z M + x K) 2^-261, two
terms under ONE Montgomery reduction -- and scan_rlc29_fold, the same row as a map composed onto the rows before it) compiled for the
host as a stand-alone program (tests/host_scan_rlc_harness.hip) and compared with Python integers over chains of 64 rows and more, for
every cell width: after every row the walk's value is canonical once packed and equals the integer recurrence, every limb of the walk
and of the fold is normalised, every value is below 2p, and the folded map applied to the start value gives the walk's last value.
The program is built twice, plain and with the address and undefined-behaviour sanitizers, and run directly."""
import itertools
import os
import random
import shutil
import subprocess

import pytest

from oracle import bn254 as o

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = o.R_MOD                                  # the scalar field Fr
R256, R261, R517 = (1 << 256) % P, (1 << 261) % P, (1 << 517) % P
R256_INV = pow(R256, -1, P)
M29 = (1 << 29) - 1
WIDTHS = (1, 2, 4, 8, 16, 32)
STEPS = 64


def top(width):
    """the largest cell: all ones for a narrow width, the Montgomery image of p - 1 for a field element"""
    return (1 << (8 * width)) - 1 if width < 32 else (P - 1) * R256 % P


def make_chains():
    """[(name, width, z0, [(m, w)] * 4, [(kind, cell)])]: cell is the stored integer (a width-32 cell is a canonical Montgomery
    image), m, w and z0 plain"""
    rng = random.Random(0x5CA9)
    chains = []
    for width in WIDTHS:
        rnd_cell = (lambda: rng.randrange(top(width) + 1)) if width < 32 else (lambda: rng.randrange(P))
        # the largest operands: T = z M + x K at its bound in every row
        chains.append((f"width {width}: all-ones cells, m = w = z0 = p-1", width, P - 1, [(P - 1, P - 1)] * 4, [(j % 4, top(width)) for j in range(STEPS)]))
        # the table the circuits use: step (r, 1), start (0, 1), hold (1, 0), clear (0, 0)
        r = rng.randrange(P)
        chains.append((f"width {width}: step/start/hold/clear", width, rng.randrange(P), [(r, 1), (0, 1), (1, 0), (0, 0)],
                       [(rng.randrange(4), rng.choice([0, top(width), rnd_cell()])) for _ in range(2 * STEPS)]))
        # m, w, z0 over {0, 1, p-1, random}: every triple starts a chain, the other kinds' records rotate through the same values
        for a, b, c in itertools.product(range(4), repeat=3):
            vals = [0, 1, P - 1, rng.randrange(P)]
            table = [(vals[(a + s) % 4], vals[(b + 2 * s) % 4]) for s in range(4)]
            rows = [(rng.randrange(4) if j % 8 else j // 8 % 4, [0, top(width), rnd_cell()][(j + a) % 3]) for j in range(STEPS)]
            chains.append((f"width {width}: m {a} w {b} z0 {c}", width, vals[c], table, rows))
    return chains


CHAINS = make_chains()


def walk(width, z0, table, rows):
    """the Montgomery images of z after every row, and the map (A, B) of the whole chain, by Python integers"""
    z, A, B, out = z0, 1, 0, []
    for kind, cell in rows:
        m, w = table[kind]
        x = cell if width < 32 else cell * R256_INV % P
        z = (m * z + w * x) % P
        A, B = m * A % P, (m * B + w * x) % P
        out.append(z * R256 % P)
    return out, A * R256 % P, B * R256 % P


def chain_file(path):
    with open(path, "w") as f:
        for _, width, z0, table, rows in CHAINS:
            f.write(f"chain {width} {len(rows)}\n{z0 * R256 % P:x}\n")
            f.write(" ".join(f"{m * R261 % P:x} {w * (R261 if width == 32 else R517) % P:x}" for m, w in table) + "\n")
            for kind, cell in rows:
                f.write(f"{kind} {cell:x}\n")


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def outputs(request, tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    d = tmp_path_factory.mktemp("scan_rlc_" + request.param)
    exe, chains = str(d / "host_scan_rlc"), str(d / "chains.txt")
    flags = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all", "-g"] if request.param == "sanitized" else []
    subprocess.run([hipcc, "--cuda-host-only", "-O2", "-std=c++17", *flags, os.path.join(ROOT, "tests", "host_scan_rlc_harness.hip"), "-o", exe], check=True, timeout=300)
    chain_file(chains)
    run = subprocess.run([exe, chains], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stderr
    lines = iter(run.stdout.splitlines())
    out = []
    for _, _, _, _, rows in CHAINS:
        steps = [next(lines).split() for _ in rows]
        fold = next(lines).split()
        assert fold[0] == "fold" and all(len(s) == 28 for s in steps)
        out.append((steps, fold[1:]))
    assert next(lines, None) is None
    return out


def test_the_chains_cover_what_they_should():
    assert all(len(rows) >= STEPS for *_, rows in CHAINS)
    for width in WIDTHS:
        mine = [c for c in CHAINS if c[1] == width]
        assert {kind for c in mine for kind, _ in c[4]} == {0, 1, 2, 3}
        assert {0, top(width)} <= {cell for c in mine for _, cell in c[4]}
        z0s = {z0 for _, _, z0, _, _ in mine}
        ms = {m for *_, table, _ in mine for m, _ in table}
        ws = {w for *_, table, _ in mine for _, w in table}
        for seen in (z0s, ms, ws):                                     # 0, 1, p - 1 and random values in every position
            assert {0, 1, P - 1} < seen


def test_every_row_is_canonical_and_equal(outputs):
    for (name, width, z0, table, rows), (steps, fold) in zip(CHAINS, outputs):
        want, A, B = walk(width, z0, table, rows)
        for j, (fields, w) in enumerate(zip(steps, want)):
            got = int(fields[0], 16)
            assert got < P and got == w, (name, j)
        gotA, gotB = int(fold[0], 16), int(fold[1], 16)
        assert gotA < P and gotB < P and (gotA, gotB) == (A, B), name
        # the folded map applied to the start value is the walk's last value
        assert (gotA * R256_INV * z0 + gotB * R256_INV) % P * R256 % P == want[-1], name


def test_limbs_are_normalised_and_values_below_2p(outputs):
    for (name, width, z0, table, rows), (steps, _) in zip(CHAINS, outputs):
        want, _, _ = walk(width, z0, table, rows)
        for j, fields in enumerate(steps):
            for part in range(3):                                      # z, A, B
                limbs = [int(x, 16) for x in fields[1 + 9 * part:10 + 9 * part]]
                assert all(x <= M29 for x in limbs), (name, j, part)   # the top limb too: a value below 2p has fewer than 2^23 there
                v = sum(x << (29 * i) for i, x in enumerate(limbs))
                assert v < 2 * P, (name, j, part)
                if part == 0:
                    assert v % P == want[j], (name, j)


def test_the_bound_of_one_reduction():
    """T = z M + x K with z < 2p normalised, M, K < p, x < 2^128: below 2^261 p, what rlc29_reduce asks; a 32-byte cell (x < p) too;
    the fullest column holds 1 + 9 + 9 products, far below the 54 a column may take before a carry pass"""
    assert 2 * P * P + (1 << 128) * P < (1 << 261) * P
    assert 2 * P * (P - 1) + (P - 1) * (P - 1) < (1 << 261) * P
    assert 1 + 9 + 9 <= 54 and (54 + 9) * (M29 * M29) + (1 << 36) < 1 << 64

"""CPU: the per-lane arithmetic of ZK_OP_ROW_INV0 (csrc/ff29.hip.hpp: inv0_29_den -- the reduced sum to canonical limbs and the zero
test --, inv0_29_prefix, inv29_rp, inv0_29_back, inv0_29_out) compiled for the host as a stand-alone program
(tests/host_row_inv0_harness.hip) and compared bit for bit with Python integers, pow(x, -1, p): a lane's four rows (one tile) give
num * inv0(D) 2^256 mod p, canonical, with D = 0 giving 0; lanes of sixteen rows (the four tiles a wave of the kernel takes) too.
Every width; denominators 0, 1 and p - 1; sums that cancel only modulo p (the reduction then leaves the INTEGER p, which the zero
test must still see) and sums that reduce to 2p - small; a lane of zero rows, a lane with one live row in each position, rows past
n; numerators absent, narrow, 32-byte and zero.  The program is built twice, plain and with the address and undefined-behaviour
sanitizers, and run directly."""
import os
import random
import shutil
import subprocess

import pytest

from oracle import bn254 as o

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = o.R_MOD
R256, R261 = (1 << 256) % P, (1 << 261) % P
K_NARROW, K_FR = (1 << 522) % P, (1 << 266) % P          # the inverting launch's constants: w 2^522, w 2^266
CINV = {0: (1 << 778) % P, 1: (1 << 1039) % P, 2: (1 << 783) % P}
WIDTHS = (1, 2, 4, 8, 16, 32)
M29 = (1 << 29) - 1


def top(width):
    return (1 << (8 * width)) - 1 if width < 32 else (P - 1) * R256 % P


def plain(width, cell):
    """the value a stored cell stands for"""
    return cell if width < 32 else cell * pow(R256, -1, P) % P


def stored(width, value):
    return value if width < 32 else value * R256 % P


class Row:
    """one row of a lane: ("terms", c, [(width, stored cell, w)]) or ("raw", T), inside n or past it"""

    def __init__(self, kind, *, c=0, cols=(), T=0, in_range=True):
        self.kind, self.c, self.cols, self.T, self.in_range = kind, c, list(cols), T, in_range

    def total(self):
        """the unreduced sum T"""
        if self.kind == "raw":
            return self.T
        return self.c * K_NARROW % P + sum(cell * (w * (K_FR if width == 32 else K_NARROW) % P) for width, cell, w in self.cols)

    def den(self):
        """D mod p: T is D 2^522 as an integer sum (narrow cells and the constant) -- T 2^-261 is D in 2^261 form"""
        return self.total() * pow(1 << 522, -1, P) % P

    def reduced(self):
        """what rlc29_reduce leaves: (T + m p) / 2^261 with m = -T / p mod 2^261"""
        T = self.total()
        m = (-T * pow(P, -1, 1 << 261)) % (1 << 261)
        return (T + m * P) >> 261

    def write(self, f):
        if self.kind == "raw":
            f.write(f"raw {int(self.in_range)} {self.T:x}\n")
            return
        f.write(f"terms {int(self.in_range)} {len(self.cols)} {self.c * K_NARROW % P:x}\n")
        for width, cell, w in self.cols:
            f.write(f"{width} {cell:x} {w * (K_FR if width == 32 else K_NARROW) % P:x}\n")


def value_row(width, value, **kw):
    """value_inv of one cell: count = 1, w = 1"""
    return Row("terms", cols=[(width, stored(width, value), 1)], **kw)


def raw_for(v):
    """an unreduced sum T < 2^261 p that rlc29_reduce takes to exactly the integer v, p <= v < 2p: T = v 2^261 - (2^261 - 1) p"""
    T = (v << 261) - ((1 << 261) - 1) * P
    assert 0 <= T < (P << 261)
    return Row("raw", T=T)


def make_lanes():
    """[(name, num kind, [4 rows], [4 stored numerators])]"""
    rng = random.Random(0x1A70)
    rnd_num = {0: lambda: 0, 1: lambda: rng.randrange(1 << 128), 2: lambda: rng.randrange(P)}
    lanes = []
    for kind in (0, 1, 2):
        nums = lambda: [rnd_num[kind]() for _ in range(4)]
        for width in WIDTHS:
            hi = plain(width, top(width))
            lanes.append((f"width {width}: 1, largest, random, zero", kind, [value_row(width, 1), value_row(width, hi), value_row(width, rng.randrange(hi + 1)), value_row(width, 0)], nums()))
        lanes.append(("denominators 0, 1, p-1, 2", kind, [value_row(32, 0), value_row(32, 1), value_row(32, P - 1), value_row(32, 2)], nums()))
        lanes.append(("constant only: 0, 1, p-1, random", kind, [Row("terms", c=c) for c in (0, 1, P - 1, rng.randrange(P))], nums()))
        a, bb = rng.randrange(1 << 64), rng.randrange(1, 1 << 64)
        fr = rng.randrange(1, P)
        lanes.append(("zeros that arise only modulo p", kind, [
            Row("terms", cols=[(8, a, 1), (8, a, P - 1)]),                                       # a - a
            Row("terms", c=P - bb, cols=[(8, bb, 1)]),                                           # c + cell, c = p - cell
            Row("terms", cols=[(32, stored(32, fr), 1), (32, stored(32, P - fr), 1)]),           # an element against its negative
            Row("terms", cols=[(8, a, 1), (8, (a + 1) % (1 << 64), P - 1)]),                     # a - (a + 1) = -1
        ], nums()))
        lanes.append(("reduced sums p, p+1, 2p-1, 2p-7", kind, [raw_for(P), raw_for(P + 1), raw_for(2 * P - 1), raw_for(2 * P - 7)], nums()))
        lanes.append(("every row zero", kind, [value_row(1, 0), Row("terms", cols=[(8, a, 1), (8, a, P - 1)]), raw_for(P), Row("terms", c=0)], nums()))
        for s in range(4):
            rows = [value_row(2, 0) for _ in range(4)]
            rows[s] = value_row(16, rng.randrange(1, 1 << 128))
            lanes.append((f"one live row, position {s}", kind, rows, nums()))
        for s in range(4):
            rows = [value_row(4, rng.randrange(1, 1 << 32)) for _ in range(4)]
            rows[s].in_range = False
            lanes.append((f"row {s} past n", kind, rows, nums()))
        lanes.append(("every row past n", kind, [value_row(4, 5, in_range=False) for _ in range(4)], nums()))
        if kind:
            lanes.append(("zero numerators", kind, [value_row(8, rng.randrange(1, 1 << 64)) for _ in range(4)], [0, rnd_num[kind](), 0, 0]))
            lanes.append(("numerators on zero rows", kind, [value_row(1, 0), value_row(1, 3), raw_for(P), value_row(1, 255)], [rnd_num[kind]() or 1 for _ in range(4)]))
            big = (1 << 128) - 1 if kind == 1 else stored(32, P - 1)
            lanes.append(("largest numerators", kind, [value_row(32, P - 1), value_row(16, (1 << 128) - 1), value_row(1, 1), value_row(32, 1)], [big] * 4))
        for s in (0, 7, 15):
            rows = [value_row(1, 0) for _ in range(16)]
            rows[s] = value_row(8, rng.randrange(1, 1 << 64))
            lanes.append((f"sixteen rows, one live, position {s}", kind, rows, [rnd_num[kind]() for _ in range(16)]))
        rows = [Row("terms", cols=[(8, a, 1), (8, a if i % 3 == 0 else a ^ (i + 1), P - 1)], in_range=i != 14) for i in range(16)]
        lanes.append(("sixteen rows, every third cancels", kind, rows, [rnd_num[kind]() for _ in range(16)]))
        for i in range(12):
            rows = []
            for _ in range(4):
                cols = []
                for _ in range(rng.choice([1, 2, 7, 33, 64])):
                    w = rng.choice(WIDTHS)
                    cols.append((w, rng.choice([0, top(w), stored(w, rng.randrange(plain(w, top(w)) + 1))]), rng.choice([0, 1, P - 1, rng.randrange(P)])))
                rows.append(Row("terms", c=rng.choice([0, P - 1, rng.randrange(P)]), cols=cols, in_range=rng.random() < 0.9))
            lanes.append((f"random {i}", kind, rows, nums()))
    return lanes


LANES = make_lanes()


def expected(kind, row, num):
    d = row.den()
    if not row.in_range or d == 0:
        return 0
    n = 1 if kind == 0 else num if kind == 1 else num * pow(R256, -1, P) % P
    return n * pow(d, -1, P) % P * R256 % P


def case_file(path):
    with open(path, "w") as f:
        for _, kind, rows, nums in LANES:
            f.write(f"lane {kind} {len(rows)} {R261:x} {CINV[kind]:x}\n")
            for row in rows:
                row.write(f)
            f.write(" ".join(f"{n:x}" for n in nums) + "\n")


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def outputs(request, tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    d = tmp_path_factory.mktemp("row_inv0_" + request.param)
    exe, cases = str(d / "host_row_inv0"), str(d / "cases.txt")
    flags = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all", "-g"] if request.param == "sanitized" else []
    subprocess.run([hipcc, "--cuda-host-only", "-O2", "-std=c++17", *flags, os.path.join(ROOT, "tests", "host_row_inv0_harness.hip"), "-o", exe], check=True, timeout=300)
    case_file(cases)
    run = subprocess.run([exe, cases], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stderr
    assert run.stderr == "", run.stderr
    lines = run.stdout.splitlines()
    assert len(lines) == sum(len(rows) + 1 for _, _, rows, _ in LANES)
    out, at = [], 0
    for _, _, rows, _ in LANES:
        out.append([ln.split() for ln in lines[at:at + len(rows) + 1]])
        at += len(rows) + 1
    return out


def test_every_row_is_canonical_and_equal(outputs):
    for (name, kind, rows, nums), out in zip(LANES, outputs):
        for s, (row, num) in enumerate(zip(rows, nums)):
            got = int(out[s][0], 16)
            assert got < P, (name, kind, s)
            assert got == expected(kind, row, num), (name, kind, s)


def test_live_rows_are_the_nonzero_rows_inside_n(outputs):
    for (name, kind, rows, _), out in zip(LANES, outputs):
        assert out[len(rows)][0] == "live"
        want = sum(1 << s for s, row in enumerate(rows) if row.in_range and row.den() != 0)
        assert int(out[len(rows)][1], 16) == want, (name, kind)


def test_the_reduced_sums_are_what_the_cases_mean_them_to_be(outputs):
    """the harness prints rlc29_reduce's limbs: normalised, below 2p, the value the model computes -- and the cases that are there for
    the integer p and for 2p - small do produce them"""
    seen = {}
    for (name, kind, rows, _), out in zip(LANES, outputs):
        for s, row in enumerate(rows):
            limbs = [int(x, 16) for x in out[s][1:10]]
            assert all(x <= M29 for x in limbs[:8]), (name, s)
            v = sum(x << (29 * i) for i, x in enumerate(limbs))
            assert v == row.reduced() and v < 2 * P, (name, s)
            seen.setdefault(name, []).append(v)
    assert seen["reduced sums p, p+1, 2p-1, 2p-7"][:4] == [P, P + 1, 2 * P - 1, 2 * P - 7]
    assert seen["zeros that arise only modulo p"][:3] == [P, P, P]            # a cancelled sum arrives as the integer p, not as 0
    assert seen["zeros that arise only modulo p"][3] not in (0, P)


def test_the_forms_and_bounds_are_the_ones_the_code_states():
    """mul29 takes a 2^-261: [x]_e [y]_f -> [x y]_(e + f - 261); inv29_rp's constant c gives [1/B]_(e) for e = log2(c) - 522"""
    assert (CINV[0], CINV[1], CINV[2]) == (pow(2, 256 + 522, P), pow(2, 517 + 522, P), pow(2, 261 + 522, P))
    assert 4 * P * P < (1 << 261) * P                                         # every product of two values below 2p
    assert 64 * (P - 1) * (P - 1) + (P - 1) < (1 << 261) * P                  # 64 full-size terms and the constant, as for the row RLC

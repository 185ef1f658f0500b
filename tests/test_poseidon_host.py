"""CPU: the per-lane code of ZK_OP_POSEIDON (csrc/poseidon29.hip.hpp: psd_load -- the cell of every width as an integer, the 31-byte
cells big-endian --, psd_in, psd_enter -- the continue-row addition, reduced --, psd_rounds -- one permutation on 29-bit limbs --,
psd_out) compiled for the host as a stand-alone program (tests/host_poseidon_harness.hip) and compared bit for bit with Python
integers over oracle.hashes.poseidon_spec(3, 8, 57).  States (0, 0, 0) and (p-1, p-1, p-1), random states, every width for in0, in1
and the capacity, a continue row adding p-1 to a state word of p-1, 31-byte words of all 0xff, messages of several rows.  The table
of limb records is made here from the oracle's constants, in the layout the header states.  The program is built twice, plain and
with the address and undefined-behaviour sanitizers, and run directly."""
import os
import random
import shutil
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import poseidon_cases as pc  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = pc.P
R256 = pc.R256
C261, C266, C522 = (1 << 261) % P, (1 << 266) % P, (1 << 522) % P
M29 = (1 << 29) - 1
WIDTHS = (1, 2, 4, 8, 16, 31, 32)


def table_words():
    """204 records of nine limbs: round 0's constants as c 2^261, the others as c 2^522, then the MDS entries as M 2^261"""
    recs = []
    for r, row in enumerate(pc.SPEC.constants):
        recs += [c * (C522 if r else C261) % P for c in row]
    recs += [pc.SPEC.mds[i][j] * C261 % P for i in range(3) for j in range(3)]
    assert len(recs) == 204
    return [(v >> (29 * i)) & M29 for v in recs for i in range(9)]


def cell_bytes(width, value):
    """the cell in memory order and the value it stands for; width 32 stores the Montgomery image"""
    if width == 32:
        return (value * R256 % P).to_bytes(32, "little")
    return value.to_bytes(width, "big" if width == 31 else "little")


def top(width):
    return P - 1 if width == 32 else (1 << (8 * width)) - 1


class Row:
    def __init__(self, head, w0, v0, w1, v1, wc=0, vc=0, scale=1):
        self.head, self.w0, self.v0, self.w1, self.v1, self.wc, self.vc, self.scale = head, w0, v0, w1, v1, wc, vc, scale

    def write(self, f):
        k = lambda w, s=1: s * (C266 if w == 32 else C522) % P
        cap = f"{self.wc} {cell_bytes(self.wc, self.vc).hex()} {k(self.wc, self.scale):x}" if self.wc else "0 - 0"
        f.write(f"row {int(self.head)} {self.w0} {cell_bytes(self.w0, self.v0).hex()} {k(self.w0):x} {self.w1} {cell_bytes(self.w1, self.v1).hex()} {k(self.w1):x} {cap}\n")


def make_cases():
    """[(name, entering state or None, [rows])]"""
    rng = random.Random(0x9051D)
    cases = [("state (0, 0, 0)", None, [Row(True, 8, 0, 8, 0)]),
             ("state (p-1, p-1, p-1)", None, [Row(True, 32, P - 1, 32, P - 1, 32, P - 1)]),
             ("state (0, 0, 0) through a zero capacity cell", None, [Row(True, 32, 0, 1, 0, 1, 0)])]
    for i in range(6):
        cases.append((f"random state {i}", None, [Row(True, 32, rng.randrange(P), 32, rng.randrange(P), 32, rng.randrange(P), rng.choice([1, 1 << 64, rng.randrange(P)]))]))
    for w in WIDTHS:
        for v in (0, 1, top(w), rng.randrange(top(w) + 1)):
            cases.append((f"in0 width {w}", None, [Row(True, w, v, 8, rng.randrange(1 << 64), 8, rng.randrange(1 << 64), 1 << 64)]))
            cases.append((f"in1 width {w}", None, [Row(True, 4, rng.randrange(1 << 32), w, v)]))
            if w != 31:
                cases.append((f"cap width {w}", None, [Row(True, 1, rng.randrange(256), 2, rng.randrange(1 << 16), w, v, rng.choice([1, 1 << 64, P - 1]))]))
    cases.append(("31-byte words of all 0xff", None, [Row(True, 31, (1 << 248) - 1, 31, (1 << 248) - 1, 8, 62, 1 << 64), Row(False, 31, (1 << 248) - 1, 31, (1 << 248) - 1)]))
    cases.append(("continue adds p-1 to state words of p-1", [P - 1, P - 1, P - 1], [Row(False, 32, P - 1, 32, P - 1)]))
    cases.append(("continue adds 1 to state words of p-1", [P - 1, P - 1, P - 1], [Row(False, 1, 1, 32, 1)]))
    cases.append(("continue from the zero state", [0, 0, 0], [Row(False, 16, rng.randrange(1 << 128), 31, rng.randrange(1 << 248))]))
    for i in range(4):
        st = [rng.randrange(P) for _ in range(3)]
        cases.append((f"continue from a random state {i}", st, [Row(False, rng.choice(WIDTHS), 0, 32, rng.randrange(P))]))
    for i in range(3):
        rows = [Row(True, 31, rng.randrange(1 << 248), 31, rng.randrange(1 << 248), 8, rng.randrange(1 << 20), 1 << 64)]
        rows += [Row(False, 31, rng.randrange(1 << 248), 31, rng.randrange(1 << 248)) for _ in range(rng.choice([1, 4, 9]))]
        cases.append((f"message {i}", None, rows))
    for _, _, rows in cases:
        for row in rows:
            row.v0 %= top(row.w0) + 1
    return cases


CASES = make_cases()


def expected_rows():
    """per row: (out, word0, word1, state) as plain integers"""
    want = []
    for _, enter, rows in CASES:
        state = list(enter) if enter is not None else [0, 0, 0]
        for row in rows:
            if row.head:
                state = [row.scale * row.vc % P if row.wc else 0, 0, 0]
            state = pc.SPEC.permute([state[0], (state[1] + row.v0) % P, (state[2] + row.v1) % P])
            want.append((state[0], row.v0 % P, row.v1 % P, list(state)))
    return want


WANT = expected_rows()


def case_file(path):
    with open(path, "w") as f:
        f.write("tab " + " ".join(f"{w:x}" for w in table_words()) + "\n")
        for _, enter, rows in CASES:
            if enter is not None:
                f.write("state " + " ".join(f"{v * R256 % P:x}" for v in enter) + "\n")
            for row in rows:
                row.write(f)


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def outputs(request, tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    d = tmp_path_factory.mktemp("poseidon_" + request.param)
    exe, cases = str(d / "host_poseidon"), str(d / "cases.txt")
    flags = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all", "-g"] if request.param == "sanitized" else []
    subprocess.run([hipcc, "--cuda-host-only", "-O2", "-std=c++17", *flags, os.path.join(ROOT, "tests", "host_poseidon_harness.hip"), "-o", exe], check=True, timeout=300)
    case_file(cases)
    run = subprocess.run([exe, cases], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stderr
    assert run.stderr == "", run.stderr
    lines = [ln.split() for ln in run.stdout.splitlines()]
    assert len(lines) == len(WANT)
    return lines


def test_every_row_is_canonical_and_equal(outputs):
    names = [name for name, _, rows in CASES for _ in rows]
    for name, got, (out, w0, w1, _) in zip(names, outputs, WANT):
        vals = [int(x, 16) for x in got[:3]]
        assert all(v < P for v in vals), name
        assert vals == [out * R256 % P, w0 * R256 % P, w1 * R256 % P], name


def test_the_state_a_row_leaves_is_normalised_below_2p_and_equal(outputs):
    """what the next row of a message continues from: three words in 2^261 form"""
    names = [name for name, _, rows in CASES for _ in rows]
    for name, got, (_, _, _, state) in zip(names, outputs, WANT):
        limbs = [int(x, 16) for x in got[3:30]]
        assert len(limbs) == 27
        for i in range(3):
            word = limbs[9 * i:9 * i + 9]
            assert all(x <= M29 for x in word[:8]), name
            v = sum(x << (29 * j) for j, x in enumerate(word))
            assert v < 2 * P and v % P == state[i] * C261 % P, (name, i)


def test_the_cases_cover_what_they_name():
    assert any(name.startswith("31-byte words of all 0xff") for name, _, _ in CASES)
    assert {row.w0 for _, _, rows in CASES for row in rows} >= set(WIDTHS) and {row.w1 for _, _, rows in CASES for row in rows} >= set(WIDTHS)
    assert {row.wc for _, _, rows in CASES for row in rows} >= {1, 2, 4, 8, 16, 32}
    assert 9 * P * P < (1 << 261) * P and 3 * (3 * P) * P + P < (1 << 261) * P            # the bounds the header states
    assert 36 * (1 << 58) + (1 << 29) < 1 << 64

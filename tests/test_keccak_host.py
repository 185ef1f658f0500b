"""CPU: the per-lane code of ZK_OP_KECCAK (csrc/keccak64.hip.hpp: the range test, absorbing at any alignment, the permutation, the
RLCs eight bytes per reduction, the records made from a challenge) compiled for the host as a stand-alone program
(tests/host_keccak_harness.hip) and compared bit for bit with the model of tests/keccak_cases.py: digests, output_rlc and input_rlc.
Every length of the shared list at every start alignment 0-7, each message ending at the LAST byte of a heap block of exactly
total_bytes (so that a read past the message is the address sanitizer's to find), messages of all 0xff, r in {0, 1, p-1, random},
and the three out-of-range rows, which give zeros and read nothing.  The program is built twice, plain and with the address and
undefined-behaviour sanitizers, and run directly."""
import os
import random
import shutil
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import keccak_cases as kc  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = kc.P


def make_cases():
    """[(name, r_out, r_in, block bytes, [(off, len)])]"""
    rng = random.Random(0x6ECCA6)
    rnd = (rng.randrange(P), rng.randrange(P))
    cases = []
    for n in kc.LENGTHS:
        for align in range(8):
            block = bytes(rng.randrange(256) for _ in range(align + n))
            cases.append((f"len {n} align {align}", rnd[0], rnd[1], block, [(align, n)]))
    for r in (0, 1, P - 1):
        for n in kc.LENGTHS:
            align = rng.randrange(8)
            block = bytes(rng.randrange(256) for _ in range(align + n))
            cases.append((f"r {'p-1' if r > 1 else r} len {n}", r, r, block, [(align, n)]))
    for n in kc.LENGTHS:
        align = rng.randrange(1, 8)
        cases.append((f"0xff len {n}", rnd[0], P - 1, b"\xa5" * align + b"\xff" * n, [(align, n)]))
    # several rows of one block: overlapping, repeated, the whole block, the empty message at the very end
    block = bytes(rng.randrange(256) for _ in range(300))
    cases.append(("rows of one block", rnd[1], rnd[0], block, [(0, 300), (1, 299), (1, 299), (164, 136), (300, 0), (299, 1), (13, 137)]))
    # out of range: zeros, nothing read
    cases.append(("out of range", rnd[0], rnd[1], block, [(301, 0), (200, 101), ((1 << 64) - 1, 2), (0, 1 << 63), (100, 200)]))
    cases.append(("empty buffer", rnd[0], rnd[1], b"", [(0, 0), (0, 1), (1, 0)]))
    return cases


CASES = make_cases()


def expected_rows():
    want = []
    for _, r_out, r_in, block, rows in CASES:
        for off, n in rows:
            if off > len(block) or n > len(block) - off:
                want.append((0, bytes(32), 0, 0))
            else:
                d, o_, i_ = kc.expected([block[off:off + n]], r_out, r_in)
                want.append((1, d[0], o_[0], i_[0]))
    return want


WANT = expected_rows()


def case_file(path):
    with open(path, "w") as f:
        for _, r_out, r_in, block, rows in CASES:
            f.write(f"r {r_out * kc.R256 % P:x} {r_in * kc.R256 % P:x}\n")
            f.write(f"buf {len(block):x} {block.hex() if block else '-'}\n")
            for off, n in rows:
                f.write(f"row {off:x} {n:x}\n")


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def outputs(request, tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    d = tmp_path_factory.mktemp("keccak_" + request.param)
    exe, cases = str(d / "host_keccak"), str(d / "cases.txt")
    flags = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all", "-g"] if request.param == "sanitized" else []
    subprocess.run([hipcc, "--cuda-host-only", "-O2", "-std=c++17", *flags, os.path.join(ROOT, "tests", "host_keccak_harness.hip"), "-o", exe], check=True, timeout=300)
    case_file(cases)
    run = subprocess.run([exe, cases], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stderr
    assert run.stderr == "", run.stderr
    lines = [ln.split() for ln in run.stdout.splitlines()]
    assert len(lines) == len(WANT)
    return lines


def test_every_row_equals_the_model_bit_for_bit(outputs):
    names = [name for name, _, _, _, rows in CASES for _ in rows]
    for name, got, (ok, digest, out, inp) in zip(names, outputs, WANT):
        assert int(got[0]) == ok, name
        assert got[1] == digest.hex(), name
        vals = [int(got[2], 16), int(got[3], 16)]
        assert all(v < P for v in vals), name
        assert vals == [out * kc.R256 % P, inp * kc.R256 % P], name


def test_out_of_range_rows_give_zeros(outputs):
    at = 0
    seen = 0
    for name, _, _, block, rows in CASES:
        for off, n in rows:
            if off > len(block) or n > len(block) - off:
                assert outputs[at] == ["0", "00" * 32, "0" * 64, "0" * 64], (name, off, n)
                seen += 1
            at += 1
    assert seen == 6


def test_the_cases_cover_what_they_name():
    singles = {(rows[0][1], rows[0][0]) for name, _, _, _, rows in CASES if name.startswith("len ")}
    assert singles == {(n, a) for n in kc.LENGTHS for a in range(8)}
    for name, _, _, block, rows in CASES:
        if name.startswith(("len ", "r ", "0xff ")):
            assert rows[0][0] + rows[0][1] == len(block), name      # the message ends at the block's last byte
    assert {r for _, r, _, _, _ in CASES} >= {0, 1, P - 1}
    oor = [rows for name, _, _, _, rows in CASES if name == "out of range"][0]
    assert (301, 0) in oor and (200, 101) in oor and ((1 << 64) - 1, 2) in oor
    assert 2 * P * P + 8 * 256 * P < (1 << 261) * P and 1 + 9 + 8 <= 54             # the bounds the header states

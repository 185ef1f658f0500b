"""CPU: the per-lane code of ZK_OP_SHA256 (csrc/sha256_32.hip.hpp: the range test, blocks at any alignment, the padding with its
second block, the 64 unrolled rounds, the digest words under the RLC step of csrc/keccak64.hip.hpp, the records made from a
challenge) compiled for the host as a stand-alone program (tests/host_sha256_harness.hip) and compared bit for bit with the model
of tests/sha256_cases.py (hashlib.sha256 and Python integers): digests, output_rlc and input_rlc.  Every length of the shared list
at every start alignment 0-7, each message ending at the LAST byte of a heap block of exactly total_bytes (so that a read past the
message is the address sanitizer's to find), messages of all 0xff, r in {0, 1, p-1, random}, several rows of one block
(overlapping, repeated, empty at the very end) and the out-of-range rows, which give zeros and read nothing.  The program is built
twice, plain and with the address and undefined-behaviour sanitizers, and run directly."""
import hashlib
import os
import random
import shutil
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import sha256_cases as sc  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = sc.P
LONG = (1 << 29) + 3


def make_cases():
    """[(name, r_out, r_in, block bytes, [(off, len)])]"""
    rng = random.Random(0x5A256)
    rnd = (rng.randrange(P), rng.randrange(P))
    cases = []
    for n in sc.LENGTHS:
        for align in range(8):
            block = bytes(rng.randrange(256) for _ in range(align + n))
            cases.append((f"len {n} align {align}", rnd[0], rnd[1], block, [(align, n)]))
    for r in (0, 1, P - 1):
        for n in sc.LENGTHS:
            align = rng.randrange(8)
            block = bytes(rng.randrange(256) for _ in range(align + n))
            cases.append((f"r {'p-1' if r > 1 else r} len {n}", r, r, block, [(align, n)]))
    for n in sc.LENGTHS:
        align = rng.randrange(1, 8)
        cases.append((f"0xff len {n}", rnd[0], P - 1, b"\xa5" * align + b"\xff" * n, [(align, n)]))
    # several rows of one block: overlapping, repeated, the whole block, the empty message at the very end
    block = bytes(rng.randrange(256) for _ in range(300))
    cases.append(("rows of one block", rnd[1], rnd[0], block, [(0, 300), (1, 299), (1, 299), (236, 64), (300, 0), (299, 1), (13, 119), (245, 55), (244, 56)]))
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
                d, o_, i_ = sc.expected([block[off:off + n]], r_out, r_in)
                want.append((1, d[0], o_[0], i_[0]))
    return want


WANT = expected_rows()


def case_file(path):
    with open(path, "w") as f:
        for _, r_out, r_in, block, rows in CASES:
            f.write(f"r {r_out * sc.R256 % P:x} {r_in * sc.R256 % P:x}\n")
            f.write(f"buf {len(block):x} {block.hex() if block else '-'}\n")
            for off, n in rows:
                f.write(f"row {off:x} {n:x}\n")


BUILT = {}


def program(kind, tmp_path_factory):
    """the harness built plain or sanitized, once per kind"""
    if kind not in BUILT:
        hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
        if not os.path.exists(hipcc):
            pytest.skip("hipcc not available")
        exe = str(tmp_path_factory.mktemp("sha256_" + kind) / "host_sha256")
        flags = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all", "-g"] if kind == "sanitized" else []
        subprocess.run([hipcc, "--cuda-host-only", "-O2", "-std=c++17", *flags, os.path.join(ROOT, "tests", "host_sha256_harness.hip"), "-o", exe], check=True, timeout=300)
        BUILT[kind] = exe
    return BUILT[kind]


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def outputs(request, tmp_path_factory):
    exe = program(request.param, tmp_path_factory)
    cases = os.path.join(os.path.dirname(exe), "cases.txt")
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
        assert vals == [out * sc.R256 % P, inp * sc.R256 % P], name


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
    assert singles == {(n, a) for n in sc.LENGTHS for a in range(8)}
    for name, _, _, block, rows in CASES:
        if name.startswith(("len ", "r ", "0xff ")):
            assert rows[0][0] + rows[0][1] == len(block), name      # the message ends at the block's last byte
    assert {r for _, r, _, _, _ in CASES} >= {0, 1, P - 1}
    assert {n for name, _, _, _, rows in CASES if name.startswith("0xff ") for _, n in rows} == set(sc.LENGTHS)
    several = [rows for name, _, _, _, rows in CASES if name == "rows of one block"][0]
    assert several.count((1, 299)) == 2 and (300, 0) in several and (0, 300) in several
    oor = [rows for name, _, _, _, rows in CASES if name == "out of range"][0]
    assert (301, 0) in oor and (200, 101) in oor and ((1 << 64) - 1, 2) in oor and (0, 1 << 63) in oor


def test_a_message_of_2_pow_29_plus_3_bytes_has_the_digest_of_hashlib(tmp_path_factory):
    """The hash alone (no RLC) over 2^29 + 3 zero bytes, in the plain build only: the bit length is 2^32 + 24, so the HIGH word of
    the 64-bit length field is not zero.  No GPU test does this: one lane would walk the 2^23 blocks for tens of seconds."""
    exe = program("plain", tmp_path_factory)
    cases = os.path.join(os.path.dirname(exe), "long.txt")
    with open(cases, "w") as f:
        f.write(f"zeros {LONG:x}\n")
    run = subprocess.run([exe, cases], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and run.stderr == "", run.stderr
    h = hashlib.sha256()
    chunk = bytes(1 << 20)
    for _ in range(LONG >> 20):
        h.update(chunk)
    h.update(bytes(LONG & ((1 << 20) - 1)))
    assert (LONG * 8) >> 32 == 1
    assert run.stdout.split() == [h.hexdigest()]

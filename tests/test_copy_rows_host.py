"""CPU: the lane-free code of ZK_OP_COPY_ROWS and ZK_OP_COPY_RLC (csrc/copy_rows.hip.hpp) compiled for the host as a stand-alone
program (tests/host_copy_rows_harness.hip) and compared with the model of tests/copy_rows_cases.py: the saturating scan of the row
counts, every integer column of the rows replayed tile by tile, value_acc from the step maps composed in groups, and the word RLCs
carried along lanes that enter a word at any offset.  The program is built twice, plain and with the address and undefined-behaviour
sanitizers, and run directly; every buffer it reads is a heap block of its exact size."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import copy_rows_cases as cp  # noqa: E402
from oracle import bn254  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = 1024                                     # CP_TILE
R_WORD, R_IN = 0x1234567890ABCDEF1234567890ABCDEF % cp.R, cp.R - 0x0FEDCBA987654321


def make_cases():
    """[(name, n, events, heap)]"""
    rng = np.random.default_rng(0xC0B1)
    heap = bytes(rng.integers(0, 256, 3000, dtype=np.uint8))
    cases = []
    for seed in range(3):
        events = cp.random_events(np.random.default_rng(seed), 30, len(heap), max_len=120)
        cases.append((f"random {seed}", sum(2 * e["length"] for e in events) + 7, events, heap))
    big = cp.event(1500, cp.MEMORY, cp.BYTECODE, src_off=5, dst_off=900, prev_off=1400, src_front=3, src_back=40, dst_front=9, dst_back=0, src_addr=10, src_addr_end=1400)
    cases.append(("one event over three tiles", 3000, [big], heap))
    cases.append(("cut at an odd n", 2 * T + 1, [cp.event(5, cp.TX_CALLDATA, cp.TX_LOG, dst_addr_bias=cp.log_bias(4)), big], heap))
    cases.append(("no events", T + 5, [], heap))
    cases.append(("no rows", 0, [big], heap))
    cases.append(("more events than rows", 17, [cp.event(1, src_off=k) for k in range(40)], heap))
    good = cp.event(30, cp.MEMORY, cp.RLC_ACC, src_off=len(heap) - 30)
    bad = [dict(good, src_tag=0), dict(good, dst_tag=6), dict(good, flags=2), dict(good, reserved=9), dict(good, src_off=len(heap) - 29), dict(good, prev_off=2**64 - 1),
           dict(good, length=2**32 - 1, src_off=1)]
    cases.append(("events that do not count", 2 * 30 * 8 + 3, [good] + [x for e in bad for x in (e, good)], heap))
    cases.append(("wholly masked threads and a memory copy", 2 * (70 + 70 + 97) + 2,
                  [cp.event(70, src_front=70, dst_front=0, dst_back=70), cp.event(70, src_front=40, src_back=31, dst_front=69, dst_back=0),
                   cp.event(97, cp.MEMORY, cp.MEMORY, flags=1, src_front=2, dst_front=30, dst_off=100, prev_off=7, rw_counter=2**40)], heap))
    cases.append(("an empty heap", 9, [cp.event(0), cp.event(1)], b""))
    return cases


CASES = make_cases()


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def outputs(request, tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    d = tmp_path_factory.mktemp("copy_rows_" + request.param)
    exe, path = str(d / "host_copy_rows"), str(d / "cases.txt")
    flags = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all", "-g"] if request.param == "sanitized" else []
    subprocess.run([hipcc, "--cuda-host-only", "-O2", "-std=c++17", *flags, os.path.join(ROOT, "tests", "host_copy_rows_harness.hip"), "-o", exe], check=True, timeout=300)
    with open(path, "w") as f:
        for _, n, events, heap in CASES:
            f.write(f"case {n} {len(events)} {len(heap)} {heap.hex() or '-'} {bn254.mont_bytes(R_WORD, cp.R).hex()} {bn254.mont_bytes(R_IN, cp.R).hex()}\n")
            f.write("".join(bytes(cp.pack_events([e])).hex() + "\n" for e in events))
    run = subprocess.run([exe, path], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, (run.returncode, run.stdout[-300:], run.stderr)
    assert run.stderr == "", run.stderr
    per_case, cur = [], None
    for ln in run.stdout.splitlines():
        words = ln.split()
        if words[0] == "starts":
            cur = {"starts": [int(x) for x in words[1:]], "col": {}, "fr": {}}
            per_case.append(cur)
        elif words[0] == "col":
            cur["col"][words[1]] = [int(x) for x in words[2:]]
        else:
            cur["fr"][words[1]] = [bn254.from_mont_bytes(bytes.fromhex(x), cp.R) for x in words[2:]]
    assert len(per_case) == len(CASES)
    return per_case


def test_row_positions_saturate_at_n(outputs):
    for (name, n, events, heap), out in zip(CASES, outputs):
        lens = [e["length"] for e in cp.effective(events, len(heap))]
        assert out["starts"] == [min(2 * sum(lens[:e]), n) for e in range(len(events) + 1)], name


def test_every_integer_column_is_the_models(outputs):
    for (name, n, events, heap), out in zip(CASES, outputs):
        m = cp.assign(events, heap, n, R_WORD, R_IN)
        for col in cp.INT_COLUMNS:
            assert out["col"][col] == m[col], (name, col, [i for i, (a, b) in enumerate(zip(out["col"][col], m[col])) if a != b][:5])


def test_value_acc_and_the_word_rlcs_are_the_models(outputs):
    for (name, n, events, heap), out in zip(CASES, outputs):
        m = cp.assign(events, heap, n, R_WORD, R_IN)
        for col in ("value_acc", "word_rlc", "word_rlc_prev"):
            assert out["fr"][col] == m[col], (name, col, [i for i, (a, b) in enumerate(zip(out["fr"][col], m[col])) if a != b][:5])

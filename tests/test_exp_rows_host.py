"""CPU: the lane-free code of ZK_OP_EXP_ROWS (csrc/exp_rows.hip.hpp) compiled for the host as a stand-alone program
(tests/host_exp_rows_harness.hip) and compared cell for cell with the closed forms of tests/exp_rows_cases.py: the saturating sums of
the row counts, the chain of truncated 256-bit multiplies of every event, the search for the intermediate exponent, both MulAdd
witnesses with their carries and u16 digits, the padding steps and the zero rows.  The program is built twice, plain and with the
address and undefined-behaviour sanitizers, and run directly; every buffer it reads is a heap block of its exact size."""
import os
import shutil
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import exp_rows_cases as ex  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENARIOS = ex.scenarios()
CASES = [(name, *SCENARIOS[name]) for name in sorted(SCENARIOS) if len(SCENARIOS[name][0]) < 2000]   # the scan's levels are the device's


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def outputs(request, tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    d = tmp_path_factory.mktemp("exp_rows_" + request.param)
    exe, path = str(d / "host_exp_rows"), str(d / "cases.txt")
    flags = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all", "-g"] if request.param == "sanitized" else []
    subprocess.run([hipcc, "--cuda-host-only", "-O2", "-std=c++17", *flags, os.path.join(ROOT, "tests", "host_exp_rows_harness.hip"), "-o", exe], check=True, timeout=300)
    with open(path, "w") as f:
        for _, events, n in CASES:
            f.write(f"case {n} {len(events)}\n")
            f.write("".join(bytes(ex.pack_events([e])).hex() + "\n" for e in events))
    run = subprocess.run([exe, path], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, (run.returncode, run.stdout[-300:], run.stderr)
    assert run.stderr == "", run.stderr
    per_case, cur = [], None
    for ln in run.stdout.splitlines():
        words = ln.split()
        if words[0] == "starts":
            cur = {"starts": [int(x) for x in words[1:]], "col": {}}
            per_case.append(cur)
        elif words[0] == "needed":
            cur["needed"] = int(words[1])
        else:
            cur["col"][words[1]] = [int(x, 16) for x in words[2:]]
    assert len(per_case) == len(CASES)
    return per_case


def test_row_positions_saturate_at_n_and_the_rows_needed_do_not(outputs):
    for (name, events, n), out in zip(CASES, outputs):
        steps = [ex.steps_of(x) for _, x in events]
        assert out["starts"] == [min(8 * sum(steps[:e]), n) for e in range(len(events) + 1)], name
        assert out["needed"] == ex.rows_needed(events), name


def test_every_cell_is_the_closed_forms(outputs):
    for (name, events, n), out in zip(CASES, outputs):
        want = ex.closed(events, n)
        assert set(out["col"]) == set(ex.COLUMNS), name
        for col in ex.COLUMNS:
            assert out["col"][col] == want[col], (name, col, [i for i, (a, b) in enumerate(zip(out["col"][col], want[col])) if a != b][:5])

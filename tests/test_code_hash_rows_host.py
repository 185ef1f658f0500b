"""CPU: the lane-free code of ZK_OP_CODE_HASH_ROWS and ZK_OP_CODE_HASH_TABLE (csrc/code_hash_rows.hip.hpp) compiled for the host as
a stand-alone program (tests/host_code_hash_rows_harness.hip) and compared with the model of tests/code_hash_rows_cases.py: the
compile-time constants, the saturating scans of both row spaces, every column of the circuit's rows and of the table's rows found
tile by tile as a lane finds them, and every field read once more from a heap block in which its bytecode ends at the last byte.  The
program is built twice, plain and with the address and undefined-behaviour sanitizers, and run directly."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import code_hash_rows_cases as ch  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = 1024                                     # BC_TILE


def make_cases():
    """[(name, n, table n, buf, offs, lens)]"""
    rng = np.random.default_rng(0xC0DE)
    cases = []

    def add(name, codes, n=None, tn=None, gap=0):
        buf, offs, lens = ch.lay_out(codes, rng, gap)
        rows, blocks = sum(len(c) + 1 for c in codes), sum(-(-len(c) // 62) for c in codes)
        cases.append((name, rows + 13 if n is None else n, blocks + 3 if tn is None else tn, buf, offs, lens))

    add("the issue's lengths side by side, end to end", [ch.random_code(rng, k) for k in ch.LENGTHS])
    add("the same with filler between them", [ch.random_code(rng, k) for k in ch.LENGTHS], gap=3)
    for j in (0, 1, 29, 30, 31, 61, 62, 63, T - 63, T - 32, T - 31, T - 2, T - 1, T, T + 1, 2 * T - 31):
        add(f"a 130-byte code behind {j} bytes", [ch.random_code(rng, j), ch.random_code(rng, 130)], gap=1)
    add("one code over three tiles", [ch.random_code(rng, 3 * T + 11)])
    add("a hundred empty bytecodes", [ch.random_code(rng, 2)] + [b""] * 100 + [ch.random_code(rng, 63)])
    add("no bytecodes", [], n=T + 5, tn=5)
    add("no rows", [ch.random_code(rng, 70)], n=0, tn=0)
    for cut in (30, 31, 32, 33):                                         # a row before, at and behind a field border, and the next field's first row
        add(f"cut at {cut}", [ch.random_code(rng, 200), ch.random_code(rng, 5)], n=cut, tn=cut // 31)
    add("more bytecodes than rows", [ch.random_code(rng, 1)] * 40, n=17, tn=9)
    add("seventy table tiles of one-block codes", [ch.random_code(rng, int(k)) for k in rng.integers(0, 3, 3 * T)], tn=2 * T + 7)
    buf = np.frombuffer(ch.random_code(rng, 300), dtype=np.uint8)
    cases.append(("invalid entries", 400, 20, buf, [0, 301, 10, 2**64 - 1, 100, 2**64 - 4, 300, 0], [70, 0, 2**64 - 1, 1, 33, 8, 0, 301]))
    cases.append(("overlapping and repeated", 900, 30, buf, [1, 2, 1, 250, 299, 0, 238], [100, 99, 100, 50, 1, 300, 62]))
    return cases


CASES = make_cases()


def effective(buf, offs, lens):
    total = len(buf)
    return [bytes(buf[o:o + ln]) if o <= total and ln <= total - o else b"" for o, ln in zip(offs, lens)]


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def outputs(request, tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    d = tmp_path_factory.mktemp("code_hash_rows_" + request.param)
    exe, path = str(d / "host_code_hash_rows"), str(d / "cases.txt")
    flags = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all", "-g"] if request.param == "sanitized" else []
    subprocess.run([hipcc, "--cuda-host-only", "-O2", "-std=c++17", *flags, os.path.join(ROOT, "tests", "host_code_hash_rows_harness.hip"), "-o", exe], check=True, timeout=300)
    with open(path, "w") as f:
        for _, n, tn, buf, offs, lens in CASES:
            f.write(f"case {n} {tn} {len(offs)} {len(buf)} {bytes(buf).hex() or '-'}\n" + "".join(f"{o} {ln}\n" for o, ln in zip(offs, lens)))
    run = subprocess.run([exe, path], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, (run.stdout[-300:], run.stderr)
    assert run.stderr == "", run.stderr
    consts, per_case, cur = None, [], None
    for ln in run.stdout.splitlines():
        words = ln.split()
        vals = [int(x, 16) for x in words[2:]] if words[0] in ("col", "tab") else [int(x, 16) for x in words[1:]]
        if words[0] == "consts":
            consts = vals
        elif words[0] == "starts":
            cur = {"starts": vals, "col": {}, "tab": {}}
            per_case.append(cur)
        elif words[0] in ("col", "tab"):
            cur[words[0]][words[1]] = vals
        else:
            cur[words[0]] = vals
    assert len(per_case) == len(CASES)
    return consts, per_case


def test_the_compile_time_constants(outputs):
    consts, _ = outputs
    assert consts[:32] == [pow(256, k, ch.R) for k in range(32)]
    assert consts[32:] == [ch.inv0(k) for k in range(31)] and all(k * v % ch.R == 1 for k, v in enumerate(consts[32:]) if k)


def test_both_row_spaces_saturate_at_n(outputs):
    for (name, n, tn, buf, offs, lens), out in zip(CASES, outputs[1]):
        codes, m = effective(buf, offs, lens), min(len(offs), n)
        assert out["starts"] == [min(sum(len(c) + 1 for c in codes[:b]), n) for b in range(m + 1)], name
        assert out["tstarts"] == [min(sum(-(-len(c) // 62) for c in codes[:b]), tn) for b in range(len(codes) + 1)], name
        assert out["needed"] == [sum(-(-len(c) // 62) for c in codes)], name


def test_every_column_of_the_rows_is_the_models(outputs):
    for (name, n, tn, buf, offs, lens), out in zip(CASES, outputs[1]):
        codes = effective(buf, offs, lens)
        want = ch.assign(codes, n)
        for col in ch.ROW_COLUMNS:
            w = [v % 2**32 for v in want[col]] if col == "control_length" else want[col]
            assert out["col"].get(col, []) == w, (name, col, [i for i, (a, b) in enumerate(zip(out["col"].get(col, []), w)) if a != b][:5])


def test_every_column_of_the_table_is_the_models(outputs):
    for (name, n, tn, buf, offs, lens), out in zip(CASES, outputs[1]):
        codes = effective(buf, offs, lens)
        want, _ = ch.table_closed(codes, tn)
        loaded, _ = ch.dev_load(codes)
        for col in ch.TABLE_COLUMNS:
            assert out["tab"].get(col, []) == want[col], (name, col, [i for i, (a, b) in enumerate(zip(out["tab"].get(col, []), want[col])) if a != b][:5])
        for i, r in enumerate(loaded[:tn]):                              # and the transliteration itself
            assert (out["tab"]["input0"][i], out["tab"]["input1"][i], out["tab"]["control"][i], out["tab"]["heading_mark"][i]) == (r[0], r[1], r[2], r[4]), (name, i)

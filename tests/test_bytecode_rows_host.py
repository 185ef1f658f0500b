"""CPU: the lane-free code of ZK_OP_BYTECODE_ROWS (csrc/bytecode_rows.hip.hpp) compiled for the host as a stand-alone program
(tests/host_bytecode_rows_harness.hip) and compared with the model of tests/bytecode_rows_cases.py: the saturating scan of the row
counts, every tile's 33-state exit map against a direct simulation of the tile from each entry state, the composition of the maps up
the hierarchy against the simulation of all rows, the state that enters every tile, and every column of the rows replayed tile by tile.
The program is built twice, plain and with the address and undefined-behaviour sanitizers, and run directly."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import bytecode_rows_cases as bc  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = 1024                                     # BC_TILE
MIXED = bytes([0x60, 0x7f, 0x01, 0x7f]) + bytes(range(0x60, 0x80)) + bytes([0x00, 0x60, 0x60, 0x5b, 0x61, 0x7f, 0x7f, 0x02]) + bytes([0x7f] * 3) + bytes(range(0x10, 0x25)) + bytes([0x60, 0x7f])


def make_cases():
    """[(name, n, buf, offs, lens)]"""
    rng = np.random.default_rng(0xB7C0)
    cases = []

    def add(name, codes, n=None, gap=2):
        buf, offs, lens = bc.lay_out(codes, rng, gap)
        cases.append((name, sum(len(c) + 1 for c in codes) + 13 if n is None else n, buf, offs, lens))

    # T - 60: a PUSH32 in one tile, cut by the end of its code in the next
    for j in (0, 1, T - 72, T - 60, T - 40, T - 34, T - 33, T - 3, T - 2, T - 1, T, 2 * T - 36, 2 * T - 1):
        add(f"mixed code behind {j} bytes", [bytes(j), MIXED])
    add("200 x 0x7f", [bytes([0x7f] * 200)])
    add("200 x 0x60", [bytes([0x60] * 200)])
    add("pushes over three tiles", [bc.random_code(rng, 3 * T + 11, push_share=0.6)])
    add("PUSH32 truncated by the end, a header behind it", [bytes([0x7f, 0x60, 0x60]), bytes([0x61, 0xaa, 0xbb, 0x00]), b"", bytes([0x7f])], gap=0)
    add("a hundred empty bytecodes", [bytes([0x62, 0x01])] + [b""] * 100 + [bytes([0x60] * 3)])
    add("no bytecodes", [], n=T + 5)
    add("no rows", [MIXED], n=0)
    add("cut inside a push", [bc.random_code(rng, T), MIXED, MIXED], n=T + 1 + 50)
    add("more bytecodes than rows", [b"\x60"] * 40, n=17)
    add("65 tiles: two levels above the tiles", [bc.random_code(rng, 40 * T, push_share=0.5), MIXED, bc.random_code(rng, 25 * T - 200, push_share=0.2)], n=65 * T)
    buf = np.frombuffer(bc.random_code(rng, 300), dtype=np.uint8)
    cases.append(("invalid entries", 400, buf, [0, 301, 10, 2**64 - 1, 100, 2**64 - 4, 300, 0], [70, 0, 2**64 - 1, 1, 33, 8, 0, 301]))
    cases.append(("overlapping and repeated", 900, buf, [1, 2, 1, 250, 299, 0], [100, 99, 100, 50, 1, 300]))
    return cases


CASES = make_cases()


def effective(buf, offs, lens):
    total = len(buf)
    return [bytes(buf[o:o + ln]) if o <= total and ln <= total - o else b"" for o, ln in zip(offs, lens)]


def simulate(cols, lo, hi, state):
    """the state that leaves rows [lo, hi) when `state` enters row lo, by the reference's recurrence"""
    for i in range(lo, hi):
        if cols["tag"][i] != bc.BYTE:
            state = 0
        else:
            state = cols["push_data_size"][i] if state == 0 else state - 1
    return state


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def outputs(request, tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    d = tmp_path_factory.mktemp("bytecode_rows_" + request.param)
    exe, path = str(d / "host_bytecode_rows"), str(d / "cases.txt")
    flags = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all", "-g"] if request.param == "sanitized" else []
    subprocess.run([hipcc, "--cuda-host-only", "-O2", "-std=c++17", *flags, os.path.join(ROOT, "tests", "host_bytecode_rows_harness.hip"), "-o", exe], check=True, timeout=300)
    with open(path, "w") as f:
        for _, n, buf, offs, lens in CASES:
            f.write(f"case {n} {len(offs)} {len(buf)} {bytes(buf).hex() or '-'}\n" + "".join(f"{o} {ln}\n" for o, ln in zip(offs, lens)))
    run = subprocess.run([exe, path], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, (run.stdout[-300:], run.stderr)
    assert run.stderr == "", run.stderr
    per_case, cur = [], None
    for ln in run.stdout.splitlines():
        words = ln.split()
        if words[0] == "starts":
            cur = {"starts": [int(x) for x in words[1:]], "map": [], "col": {}}
            per_case.append(cur)
        elif words[0] == "map":
            assert int(words[1]) == len(cur["map"])
            cur["map"].append([int(x) for x in words[2:]])
        elif words[0] == "col":
            cur["col"][words[1]] = [int(x) for x in words[2:]]
        else:
            cur[words[0]] = [int(x) for x in words[1:]]
    assert len(per_case) == len(CASES)
    return per_case


def test_row_positions_saturate_at_n(outputs):
    for (name, n, buf, offs, lens), out in zip(CASES, outputs):
        codes, m = effective(buf, offs, lens), min(len(offs), n)
        exact = [sum(len(c) + 1 for c in codes[:b]) for b in range(m + 1)]
        assert out["starts"] == [min(s, n) for s in exact], name


def test_every_column_of_the_replayed_rows_is_the_models(outputs):
    for (name, n, buf, offs, lens), out in zip(CASES, outputs):
        codes = effective(buf, offs, lens)
        m = bc.assign(codes, [0] * len(codes), n, 0, fail_fast=False)
        for col in bc.INT_COLUMNS:
            want = [v % 2**32 for v in m[col]]
            assert out["col"].get(col, []) == want, (name, col, [i for i, (a, b) in enumerate(zip(out["col"].get(col, []), want)) if a != b][:5])


def test_tile_maps_composition_and_entry_states_are_the_recurrence(outputs):
    levels_seen = set()
    for (name, n, buf, offs, lens), out in zip(CASES, outputs):
        if not n:
            assert out["map"] == [] and out["root"] == [] and out["entry"] == []
            continue
        codes = effective(buf, offs, lens)
        cols = bc.assign(codes, [0] * len(codes), n, 0, fail_fast=False)
        tiles = (n + T - 1) // T
        assert len(out["map"]) == tiles == len(out["entry"])
        # rows at or after n are not written: the last tile treats them as padding, which resets
        exits = lambda t, s: simulate(cols, t * T, min(t * T + T, n), s) if t * T + T <= n else 0
        step = max(1, tiles // 12)
        for t in list(range(0, tiles, step)) + [tiles - 1]:
            assert out["map"][t] == [exits(t, s) for s in range(33)], (name, t)
        # the root: all rows from each entry state (a few of them where the rows are many)
        assert len(out["root"]) == 33
        for s in (range(33) if tiles <= 20 else (0, 1, 17, 32)):
            assert out["root"][s] == (0 if n % T else simulate(cols, 0, n, s)), (name, s)
        # the state that enters a tile is what the recurrence carries there from row 0
        entry, state = [], 0
        for t in range(tiles):
            entry.append(state)
            state = simulate(cols, t * T, min(t * T + T, n), state)
        assert out["entry"] == entry, name
        levels_seen.add(0 if tiles == 1 else 1 if tiles <= 64 else 2)
    assert levels_seen == {0, 1, 2}
    assert any(max(out["entry"], default=0) >= 20 for out in outputs) and any(1 <= min((e for e in out["entry"] if e), default=0) <= 3 for out in outputs)

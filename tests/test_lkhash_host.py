"""CPU: the hash of the lookup hash join (csrc/lkhash.hip.hpp) compiled for the host as a stand-alone program
(tests/host_lkhash_harness.hip) against the Python replica of tests/lookup_join_cases.py -- 0, 1, r - 1, the eight single-limb values
and 2000 random values, as Montgomery rows -- and the model and the case builders of that file against themselves.  The engineered
cases of tests/test_gpu_lookup_join.py (home slots that collide, probes that wrap) are chosen with the replica: were it wrong, they
would silently be random cases.  The program is built twice, plain and with the address and undefined-behaviour sanitizers, and run
directly."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import lookup_join_cases as lc  # noqa: E402
from oracle import bn254  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = bn254.R_MOD


def hash_values(cref):
    """(n, 4) uint64 rows"""
    named = cref.to_mont([0, 1, R - 1])
    single = np.zeros((8, 8), dtype=np.uint32)
    for j in range(8):
        single[j, j] = 0x2B3C4D5E + j
    return np.concatenate([named, single.view(np.uint64).reshape(8, 4), lc.random_rows(np.random.default_rng(0x1CA5), 2000)])


@pytest.fixture(scope="module")
def named(cref):
    return cref.to_mont([0, 1, R - 1])


@pytest.fixture(scope="module")
def cases(named):
    return lc.build_cases(named)


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def outputs(request, tmp_path_factory, cref):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    d = tmp_path_factory.mktemp("lkhash_" + request.param)
    exe, path = str(d / "host_lkhash"), str(d / "values.txt")
    flags = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all", "-g"] if request.param == "sanitized" else []
    subprocess.run([hipcc, "--cuda-host-only", "-O2", "-std=c++17", *flags, os.path.join(ROOT, "tests", "host_lkhash_harness.hip"), "-o", exe], check=True, timeout=300)
    values = hash_values(cref)
    with open(path, "w") as f:
        for v in cref.limbs_to_ints(values):
            f.write(f"{v:x}\n")
    run = subprocess.run([exe, path], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, (run.stdout[-500:], run.stderr)
    assert run.stderr == "", run.stderr
    lines = [ln.split() for ln in run.stdout.splitlines()]
    assert len(lines) == len(values) == 3 + 8 + 2000
    return values, lines


def test_the_replica_is_the_compiled_hash(outputs):
    values, lines = outputs
    got = [int(ln[0], 16) for ln in lines]
    assert got == [lc.fr_hash(lc.limbs_of(v)) for v in values]
    assert got == [int(h) for h in lc.fr_hash_rows(values)]
    assert len(set(got)) == len(got)                                           # 2011 values, 32 bits: a hash that dropped a limb would collide
    assert all(ln[1] == "1" and ln[2] == "0" for ln in lines)                  # fr_same: equal to itself, different from its neighbour


def test_the_kernels_use_the_header_the_harness_compiles():
    csrc = os.path.join(ROOT, "zkevm-circuits_amd", "csrc")
    unit, header = open(os.path.join(csrc, "lookup.hip")).read(), open(os.path.join(csrc, "lkhash.hip.hpp")).read()
    assert '#include "lkhash.hip.hpp"' in unit and "uint32_t fr_hash(" not in unit and "bool fr_same(" not in unit
    assert "__host__ __device__ __forceinline__ uint32_t fr_hash(" in header and "__host__ __device__ __forceinline__ bool fr_same(" in header
    assert "csrc/lkhash.hip.hpp" in open(os.path.join(ROOT, "zkevm-circuits_amd", "Makefile")).read().split("HDR :=")[1]
    assert '#include "../zkevm-circuits_amd/csrc/lkhash.hip.hpp"' in open(os.path.join(ROOT, "tests", "host_lkhash_harness.hip")).read()


def test_every_limb_reaches_the_hash():
    """a bit of each limb changes the hash.  (Bit 20, not bit 0: the first step is (l0 ^ l1) * c + (l0 >> 15), so the same low bit
    flipped in limb 0 or in limb 1 gives one hash -- a collision the join resolves by comparing limbs, fr_same.)"""
    base = lc.random_rows(np.random.default_rng(5), 1)[0]
    seen = {lc.fr_hash(lc.limbs_of(base))}
    for j in range(8):
        l = base.copy().view(np.uint32)
        l[j] ^= 1 << 20
        seen.add(lc.fr_hash(lc.limbs_of(l.view(np.uint64))))
    assert len(seen) == 9
    a, b = base.copy().view(np.uint32), base.copy().view(np.uint32)
    a[0] ^= 1
    b[1] ^= 1
    assert lc.fr_hash(lc.limbs_of(a.view(np.uint64))) == lc.fr_hash(lc.limbs_of(b.view(np.uint64)))


def test_slot_formulas():
    assert [lc.hash_cap(u) for u in (1, 8, 9, 16, 17, 32, 1000, 1024, 1025)] == [16, 16, 32, 32, 64, 64, 2048, 2048, 4096]
    assert lc.lds_home(0) == 0 and lc.lds_home(1) == 0x9E3779B1 >> 21 and max(lc.lds_home(r) for r in range(4096)) == 2047
    assert lc.LK_BLOCK_SLOTS == 2048 == 2 * lc.LK_COUNT_THREADS


def test_model_on_a_table_by_hand(named):
    zero, one, minus = named
    table = np.array([one, zero, one, minus, zero, minus])
    inputs = np.array([zero, one, one, minus, minus, one])
    assert lc.multiplicities(table, inputs, 6, 6) == ([0, 0, 3, 0, 1, 2], None)            # the last row holding a value owns it; input row 5 counts
    assert lc.multiplicities(table, inputs, 5, 6) == ([0, 0, 2, 2, 1, 0], None)            # row 5 of neither side counts
    assert lc.multiplicities(table, inputs, 3, 6) == ([0, 1, 2, 0, 0, 0], None)
    assert lc.multiplicities(table, inputs, 1, 6) == ([0] * 6, 0)                           # only `one` is usable: input row 0 is missing
    assert lc.multiplicities(table[2:], inputs[2:], 1, 4) == ([1, 0, 0, 0], None)
    assert lc.multiplicities(table, np.array([one, minus, zero, one, zero, one]), 3, 6) == ([0, 1, 1, 0, 0, 0], 1)


def test_the_cases_are_what_they_claim(cases):
    assert len(cases) == 2 * len(lc.SIZES) + 15 and len({c.name for c in cases}) == len(cases)
    for c in cases:
        results = [lc.multiplicities(*call) for call in c.calls]
        c.expect(results)
        for (table, inputs, usable, n), (m, bad) in zip(c.calls, results):
            assert len(m) == n and sum(m[usable:]) == 0
            held = {t.tobytes() for t in table[:usable]}
            missing = [r for r in range(usable) if inputs[r].tobytes() not in held]
            assert sum(m) == usable - len(missing) and bad == (missing[0] if missing else None)
    assert lc.runs_straddle()


def test_workgroup_owners_wrap_and_share():
    """Owner rows below 4096 spread over the 2048 LDS slots two a slot (the multiplier is the golden ratio's): only 16 have a home
    slot >= 2040 and at most 3 share one.  They still overflow the last 8 slots, so probes wrap; the 40 + 40 the cases ask for
    need the 2^17-row table."""
    for rows, wrap, share in ((4096, 16, 3), (1 << 17, 40, 40)):
        owners, a, b = lc.workgroup_owners(rows)
        assert len(set(owners.tolist())) == 1024 and a >= wrap and b >= share and a > 8
        homes = [lc.lds_home(int(r)) for r in owners]
        assert sum(1 for h in homes if h >= 2040) >= wrap and max(np.bincount([h for h in homes if h < 2040])) >= share


def test_global_clusters_wrap():
    """the clustered values fill the table's last slots and spill over slot 0; a value that is not in the table and starts inside the
    cluster is given up only after the probe has walked to the last slot, wrapped, and found the first empty slot behind the spill"""
    for cap, usable, count, lo in lc.WRAPS:
        case, absent = lc.global_wrap(cap, usable, count, lo)
        table, inputs, _, _ = case.calls[0]
        homes = lc.fr_hash_rows(table[:usable]) & np.uint32(cap - 1)
        assert int((homes >= lo).sum()) >= count > cap - lo
        used, cap_ = lc.occupied_slots(table, usable)
        assert cap_ == cap and len(used) == usable and set(range(lo, cap)) <= used and 0 in used
        hit = {r.tobytes() for r in inputs[:usable]}
        assert all(t.tobytes() in hit for t, h in zip(table[:usable], homes) if h >= lo)
        for a in absent:
            path = lc.probe_path(a, used, cap)
            assert path[0] >= lo and path[-1] < lo and cap - 1 in path and 0 in path and len(path) > count - (cap - lo)

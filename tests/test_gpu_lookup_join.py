"""GPU: the logUp multiplicity hash join (zk_lookup_multiplicities; csrc/lookup.hip: k_lk_insert, k_lk_count, k_lk_to_fr) against the
model of tests/lookup_join_cases.py on the engineered cases of that file, bit for bit and in full: every row of m -- those from
`usable` on must read 0, and m is filled with 0xFF bytes before each call -- and the bad row.  What the cases reach:

  sizes                      usable 1 .. 2049 around every wave, workgroup and `cap` boundary (cap doubles 8 -> 9, 16 -> 17, ...), with n = usable and
                             n a power of two above it; the rows from `usable` on hold values found nowhere else
  one value                  3000 equal rows: one slot, the ballot leaves one representative a wave, the top row owns; twice, equal results
  runs counted from the top  runs of 1, 63, 64, 65, 300 equal rows across wave and workgroup boundaries of k_lk_insert's own index, one value in two runs
  everything on one row      4090 inputs on one owner: one LDS entry a workgroup, one atomic each
  a full workgroup           1024 distinct owners in one workgroup of k_lk_count: the LDS table half full, home slots >= 2040 that wrap past
                             slot 2047 and a crowd on one home slot (16 and 3 of them among 4096 rows -- all there are; 64 and 40 among 2^17)
  global collisions          values whose home slots are the last of the table (cap 16, 64, 2048): probes wrap at `mask`; then three values that
                             are not in the table and start inside the cluster: missing only after the walk wraps, the lowest row is returned
  usable means usable        a value held by unusable table rows only is missing; a missing value in an unusable input row is not
  one limb apart             rows that differ in one bit of one limb, and two rows with the same hash: each credits its own row
  zero                       0 as a table value next to the idle lanes of a partial wave (their key is Fr::zero()); alone; with 1 and r - 1
  misses and reuse           misses at rows 0 and usable - 1; then good inputs; then a 16-row table on the scratch the 4096-row one left
  padded profile             n = 2^16: 200 rows, then the default row; 90 % of the inputs are the default

tests/test_lkhash_host.py holds the hash replica the cases are chosen with to the compiled hash, and checks on the CPU that the
cases are what this list says."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import lookup_join_cases as lc  # noqa: E402
from oracle import bn254  # noqa: E402

pytestmark = pytest.mark.gpu
NAMES = [c.name for c in lc.build_cases(np.zeros((3, 4), dtype=np.uint64))]       # the names do not depend on the named rows


@pytest.fixture(scope="module")
def cases(cref):
    return {c.name: c for c in lc.build_cases(cref.to_mont([0, 1, bn254.R_MOD - 1]))}


def run_call(ctx, table, inputs, usable, n):
    """-> (m as the (n, 4) array the device left, bad row or None)"""
    dT, dI, dM = ctx.to_device(table), ctx.to_device(inputs), ctx.to_device(np.full((n, 4), 0xFFFFFFFFFFFFFFFF, dtype=np.uint64))
    try:
        bad = ctx.lookup_multiplicities(dI, dT, usable, dM, n)
        return dM.download((n, 4)), bad
    finally:
        for buf in (dT, dI, dM):
            buf.free()


@pytest.mark.parametrize("name", NAMES)
def test_join_equals_the_model(ctx, cref, cases, name):
    case = cases[name]
    got = []
    for table, inputs, usable, n in case.calls:
        want_m, want_bad = lc.multiplicities(table, inputs, usable, n)
        m, bad = run_call(ctx, table, inputs, usable, n)
        print(f"{name}: usable {usable}, n {n}: bad row {bad} (model {want_bad}), sum m {sum(want_m)}")
        assert bad == want_bad
        diff = np.nonzero((m != cref.to_mont(want_m)).any(axis=1))[0]
        assert diff.size == 0, f"{diff.size} rows of m differ, the first at {diff[:8]}: got {cref.from_mont(m[diff[:8]])}, model {[want_m[i] for i in diff[:8]]}"
        assert not m[usable:].any()
        got.append(([int(v) for v in cref.from_mont(m)], bad))
    case.expect(got)

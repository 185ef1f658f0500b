"""GPU: every launch path of the NTT against the C oracle, bit for bit.  The cases are ntt_cases.GPU_CASES -- sizes, column counts
and geometry knobs (ZK_NTT_PASS_LOGTILE, ZK_NTT_LAST_LOGTILE, ZK_NTT_XCD, ZK_NTT_XCD_COLS, ZK_NTT_FIXED, ZK_NTT_BATCH, and domains
without inter-pass tables) chosen so that together they reach every launch signature the plans can produce up to 2^22
(test_ntt_plan.py checks that on a CPU).  Each case first asks zk_host_ntt_plan that it still takes the kernels it is listed for."""
import numpy as np
import pytest

import ntt_cases as nc
from oracle import bn254

pytestmark = pytest.mark.gpu

_columns, _forward, _coset = {}, {}, {}      # the oracle's work, once per (k, column) for the whole module; never modified


def coset_generator(k):
    return 0xC05E70 + k


def column(cref, k, i):
    if (k, i) not in _columns:
        _columns[k, i] = cref.rand_fr_stream(6100 + 37 * k + i, 1 << k)
    return _columns[k, i]


def forward(cref, k, i):
    if (k, i) not in _forward:
        _forward[k, i] = cref.best_fft(column(cref, k, i), bn254.omega_for_k(k), k)
    return _forward[k, i]


def coset(cref, k, i):
    if (k, i) not in _coset:
        _coset[k, i] = cref.best_fft(cref.distribute_powers(column(cref, k, i), coset_generator(k)), bn254.omega_for_k(k), k)
    return _coset[k, i]


def case_id(case):
    k, columns, knobs, tables = case
    short = "-".join(n[len("ZK_NTT_"):].lower() + v for n, v in sorted(knobs.items()))
    return f"k{k}-{columns}col" + ("-" + short if short else "") + ("" if tables else "-tableless")


def case_columns(index):
    """Which columns of its size's pool a case runs on: the pool is as large as the widest case of the size, and a case starts where
    the cases of the size before it stopped counting, so the oracle's work at the large sizes is spread over the cases."""
    k, columns = nc.GPU_CASES[index][:2]
    pool = max(c[1] for c in nc.GPU_CASES if c[0] == k)
    start = sum(1 for c in nc.GPU_CASES[:index] if c[0] == k)
    return [(start + j) % pool for j in range(columns)]


@pytest.mark.parametrize("index", range(len(nc.GPU_CASES)), ids=[case_id(c) for c in nc.GPU_CASES])
def test_case_matches_the_oracle(zk, ctx, cref, index):
    """ntt_batch forward and inverse and coeff_to_coset_batch out of place on the case's columns under its knobs: every forward
    column is best_fft, the inverse returns the input, every coset column is best_fft(distribute_powers(column, g))."""
    k, columns, knobs, tables = nc.GPU_CASES[index]
    n = 1 << k
    pl = nc.plan(zk, k, columns, knobs, tables)
    assert nc.launch_key(pl) == nc.GPU_CASE_LAUNCHES[index], "the case no longer takes the launches it is listed for"
    which = case_columns(index)
    cols = [column(cref, k, i) for i in which]
    g = cref.fr_const(coset_generator(k))
    held = []
    with nc.knobs_set(knobs, tables):
        c = ctx if tables else zk.Context(0)      # a cached domain keeps its tables: a tableless case gets a context of its own
        try:
            bufs = [c.to_device(col) for col in cols]
            held += bufs
            outs = [c.alloc(n * 32) for _ in cols]
            held += outs
            c.ntt_batch(bufs, k)
            fwd = [b.download((n, 4)) for b in bufs]
            c.ntt_batch(bufs, k, inverse=True)
            inv = [b.download((n, 4)) for b in bufs]
            c.coeff_to_coset_batch(bufs, k, g, outs)
            cos = [o.download((n, 4)) for o in outs]
        finally:
            for b in held:
                b.free()
            if not tables:
                c.close()
    for j, i in enumerate(which):
        assert np.array_equal(fwd[j], forward(cref, k, i)), f"forward, column {j}"
        assert np.array_equal(inv[j], cols[j]), f"inverse, column {j}"
        assert np.array_equal(cos[j], coset(cref, k, i)), f"coset, column {j}"

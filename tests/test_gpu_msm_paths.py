"""GPU parity of every MSM code path the plan and the measurement knobs can pick (csrc/msm.hip): each merged window size 8 .. 22
and each per-window size 4 .. 16, every top_shift, the sliced and the one-launch sorts, direct and LDS-staged scatter, the chunk
sizes, one and two pipelines, graph replay, the narrow (per-window and GM) paths and the table-less path -- over the edge scalar
families of msm_scalars.py, against best_multiexp (n <= 2^16) or the closed form f(s) G over g[i] = s^i G (above).  Every
comparison is bit-exact on the affine point.  The knobs are "speed only": no setting may change a result."""
import hashlib
import ctypes
import os
import random

import numpy as np
import pytest

from msm_scalars import families
from oracle import bn254
from zkevm_circuits_amd import binding

pytestmark = pytest.mark.gpu

S_SRS = 0x5A17ED
_WANT = {}            # oracle results, keyed by (column bytes, basis tag, n): many families do not depend on the plan


@pytest.fixture(autouse=True)
def _clean_msm_env(monkeypatch):
    for var in [v for v in os.environ if v.startswith("ZK_MSM_") and v != "ZK_MSM_TRACE"]:        # every path knob off; the trace is no knob
        monkeypatch.delenv(var)


@pytest.fixture(scope="module")
def srs12(ctx, cref):
    srs = ctx.srs_setup_with_s(12, cref.fr_const(S_SRS))
    yield srs
    srs.destroy()


@pytest.fixture(scope="module")
def bases12(srs12):
    """the two bases of srs12 on the host, by `lagrange`"""
    return {False: srs12.download_g(), True: srs12.download_g_lagrange()}


def _plan(k):
    """(c, W, top_shift) of the merged plan of an SRS of 2^k points under the current environment (ZK_MSM_C / ZK_MSM_TOP_SHIFT)."""
    c, w, sh = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    assert binding.lib().zk_host_msm_plan(ctypes.c_uint32(k), ctypes.byref(c), ctypes.byref(w), ctypes.byref(sh)) == 0
    return c.value, w.value, sh.value


def _cols(cref, c, n, seed, names=None):
    """The families of a c-bit plan as Montgomery columns of n rows (each family cycled); `random` is n independent scalars."""
    W = (256 + c - 1) // c
    out = {}
    for name, vals in families(c, W, 0, None, random.Random(seed)).items():
        if (names and name not in names) or not vals:
            continue
        out[name] = cref.rand_fr_stream(seed, n) if name == "random" else np.resize(cref.to_mont(vals), (n, 4))
    return out


def _want(cref, col, bases, tag, n):
    key = (hashlib.sha1(col[:n].tobytes()).digest(), tag, n)
    if key not in _WANT:
        _WANT[key] = cref.best_multiexp(np.ascontiguousarray(col[:n]), np.ascontiguousarray(bases[:n]))
    return _WANT[key]


def _closed_form(cref, col, s):
    """MSM(col, g) over g[i] = s^i G: (sum col_i s^i) G."""
    acc = cref.eval_polynomial(np.ascontiguousarray(col), s)
    return cref.g1_mul(cref.affine_to_mont([bn254.G1_GEN]), cref.to_mont([acc]))[0]


def _commit(ctx, srs, bufs, n, lagrange, narrow=None):
    """commit_batch with every column hinted dense unless hints are given: without hints the library sends small-valued columns
    (zero, one, boolean, low_only, ...) to the per-window path, and the merged plan under test would never see them"""
    return ctx.commit_batch(srs, [b_.ptr for b_ in bufs.values()], n, lagrange=lagrange, narrow=[0] * len(bufs) if narrow is None else narrow)


def _bad(names, got, want):
    return [nm for nm, g_, w_ in zip(names, got, want) if not np.array_equal(g_, w_)]


def test_window_table_follows_top_shift_and_window_size(ctx, cref, monkeypatch):
    """The merged path caches the SRS's window table; its top window is built with c - top_shift doublings, so a table built
    under one (c, top_shift) must not serve a commitment under another: default, ZK_MSM_TOP_SHIFT=0, default again, then
    ZK_MSM_C flipped and back, over one SRS -- every commitment = best_multiexp.  The batch of six takes graph replay, whose
    cached graphs carry the top_shift in their kernel arguments: they must not be replayed under another one either."""
    srs = ctx.srs_setup_with_s(12, cref.fr_const(S_SRS + 1))
    n = 1 << 12
    cols = {f"random{i}": cref.rand_fr_stream(900 + i, n) for i in range(3)}
    cols.update(_cols(cref, 12, n, 901, names={"top_carry", "top_only", "r_minus_1"}))
    bufs = {nm: ctx.to_device(col) for nm, col in cols.items()}
    names = list(cols)
    for lagrange in (False, True):
        bases = srs.download_g_lagrange() if lagrange else srs.download_g()
        want = [cref.best_multiexp(cols[nm], bases) for nm in names]
        for step, env in enumerate(({}, {"ZK_MSM_TOP_SHIFT": "0"}, {}, {"ZK_MSM_TOP_SHIFT": "1"}, {"ZK_MSM_C": "9"}, {},
                                    {"ZK_MSM_C": "9", "ZK_MSM_TOP_SHIFT": "0"}, {"ZK_MSM_C": "9"}, {})):
            for var in ("ZK_MSM_C", "ZK_MSM_TOP_SHIFT"):
                monkeypatch.delenv(var, raising=False)
            for var, val in env.items():
                monkeypatch.setenv(var, val)
            got = _commit(ctx, srs, bufs, n, lagrange)
            single = ctx.commit(srs, bufs["random0"], n, lagrange=lagrange)
            bad = _bad(names, got, want)
            assert not bad and np.array_equal(single, want[0]), \
                f"step {step} {env or 'default'} (plan {_plan(12)}), lagrange {lagrange}: {bad} differ from best_multiexp"
    for b_ in bufs.values():
        b_.free()
    srs.destroy()


@pytest.mark.parametrize("c", range(8, 23))
def test_every_merged_window_size(ctx, cref, srs12, bases12, monkeypatch, c):
    """ZK_MSM_C = c over an SRS of 2^12 points: every top_shift in {0, 1, max}, every family, both bases, n = 2^12, 2^12 - 3
    and 64 (the smallest MSM that takes the table); n = 63 goes to the per-window path.  ZK_MSM_TABLE_GB=0 routes the same
    columns to the table-less path: same points."""
    monkeypatch.setenv("ZK_MSM_C", str(c))
    cc, W, sh_max = _plan(12)
    assert cc == c
    cols = _cols(cref, c, 1 << 12, 1000 + c)
    names = list(cols)
    bufs = {nm: ctx.to_device(col) for nm, col in cols.items()}
    for n in (1 << 12, (1 << 12) - 3, 64, 63):
        assert ctx.msm_plan(srs12, n)["c"] == (c if n >= 64 else max(4, min(n.bit_length() - 5, 16)))
        for lagrange in (False, True):
            want = [_want(cref, cols[nm], bases12[lagrange], ("k12", lagrange), n) for nm in names]
            for sh in (sorted({0, min(1, sh_max), sh_max}) if n >= 64 else [sh_max]):
                monkeypatch.setenv("ZK_MSM_TOP_SHIFT", str(sh))
                bad = _bad(names, _commit(ctx, srs12, bufs, n, lagrange), want)
                assert not bad, f"c = {c}, top_shift = {sh}, n = {n}, lagrange {lagrange}: {bad} differ from best_multiexp"
            monkeypatch.delenv("ZK_MSM_TOP_SHIFT")
            if n == 1 << 12:
                monkeypatch.setenv("ZK_MSM_TABLE_GB", "0")
                bad = _bad(names, _commit(ctx, srs12, bufs, n, lagrange), want)
                monkeypatch.delenv("ZK_MSM_TABLE_GB")
                assert not bad, f"table-less path (c = {c} families), lagrange {lagrange}: {bad} differ from best_multiexp"
    for b_ in bufs.values():
        b_.free()


@pytest.mark.parametrize("k,n", [(18, 1 << 18), (21, 1 << 20)])
def test_natural_window_sizes_18_and_21(ctx, cref, k, n):
    """c = 18 and c = 21 at the SRS sizes that pick them (the Keccak and bundle proofs' plans), default knobs: the families of
    that plan against the closed form over the coefficient basis."""
    c = k
    srs = ctx.srs_setup_with_s(k, cref.fr_const(S_SRS + k))
    assert ctx.msm_plan(srs, n)["c"] == c
    cols = _cols(cref, c, n, 2000 + k, names={"half", "half_plus_one", "all_ones_runs", "top_carry", "top_only", "low_only", "r_minus_1", "random"})
    names = list(cols)
    bufs = {nm: ctx.to_device(col) for nm, col in cols.items()}
    want = [_closed_form(cref, cols[nm], S_SRS + k) for nm in names]
    bad = _bad(names, _commit(ctx, srs, bufs, n, False), want)
    assert not bad, f"c = {c} at 2^{k}: {bad} differ from the closed form"
    for b_ in bufs.values():
        b_.free()
    srs.destroy()


@pytest.mark.parametrize("c", [8, 12, 16, 19, 20, 21, 22])
def test_sort_and_scatter_paths(ctx, cref, srs12, bases12, monkeypatch, c):
    """ZK_MSM_BINSORT (one-launch partition sort / sliced count-scan-scatter) x ZK_MSM_STAGED (LDS-staged / direct scatter,
    c >= 19 only) x ZK_MSM_CHUNK (256, 1000, 2048, 65536 scalars per partition workgroup) at window size c: every combination
    = best_multiexp, hence the same bytes."""
    n = (1 << 12) - 3
    monkeypatch.setenv("ZK_MSM_C", str(c))
    cols = _cols(cref, c, n, 3000 + c, names={"half", "half_plus_one", "all_ones_runs", "top_carry", "one_hot", "all_equal", "sparse", "boolean", "random"})
    names = list(cols)
    bufs = {nm: ctx.to_device(col) for nm, col in cols.items()}
    want = [_want(cref, cols[nm], bases12[True], ("k12", True), n) for nm in names]
    for bs in ("0", "1"):
        for staged in ("0", "1"):
            for chunk in ("256", "1000", "2048", "65536"):
                monkeypatch.setenv("ZK_MSM_BINSORT", bs)
                monkeypatch.setenv("ZK_MSM_STAGED", staged)
                monkeypatch.setenv("ZK_MSM_CHUNK", chunk)
                bad = _bad(names, _commit(ctx, srs12, bufs, n, True), want)
                assert not bad, f"c = {c}, BINSORT={bs} STAGED={staged} CHUNK={chunk}: {bad} differ from best_multiexp"
    for b_ in bufs.values():
        b_.free()


def _mixed_batch(pool, count, offset):
    """count columns drawn from the family pool so that neighbours differ in bucket skew"""
    names = list(pool)
    return [names[(offset + 5 * i) % len(names)] for i in range(count)]


def _pipeline_settings():
    return [(p, g) for p in ("1", "2") for g in ("0", "1")]


def test_batches_pipelines_and_graph_replay(ctx, cref, srs12, bases12, monkeypatch, capfd):
    """Batches of 1, 2, 3, 4, 5 and 9 mixed columns under ZK_MSM_PIPES x ZK_MSM_GRAPH: each column = its own
    oracle.  Where graph replay is due (4+ columns, 1024 <= n <= 2^19) the trace must say it ran: the session's context keeps a
    graph failure for good, and the fallback alone would pass every comparison."""
    pool = _cols(cref, 12, 1 << 12, 4000)
    bufs = {nm: ctx.to_device(col) for nm, col in pool.items()}
    monkeypatch.setenv("ZK_MSM_TRACE", "1")
    for n in (1024, (1 << 12) - 5):
        for count in (1, 2, 3, 4, 5, 9):
            names = _mixed_batch(pool, count, count + n)
            want = [_want(cref, pool[nm], bases12[True], ("k12", True), n) for nm in names]
            for pipes, graph in _pipeline_settings():
                monkeypatch.setenv("ZK_MSM_PIPES", pipes)
                monkeypatch.setenv("ZK_MSM_GRAPH", graph)
                capfd.readouterr()
                got = ctx.commit_batch(srs12, [bufs[nm].ptr for nm in names], n, lagrange=True, narrow=[0] * count)
                err = capfd.readouterr().err
                label = f"n = {n}, {count} columns, PIPES={pipes} GRAPH={graph}"
                bad = [f"{i}:{nm}" for i, nm in enumerate(names) if not np.array_equal(got[i], want[i])]
                assert not bad, f"{label}: columns {bad} differ from best_multiexp"
                assert ("(graph replay)" in err) == (graph == "1" and count >= 4), f"{label}: graph replay expected {graph == '1' and count >= 4}, trace: {err!r}"
    for b_ in bufs.values():
        b_.free()


def test_batches_at_2_19(ctx, cref, monkeypatch, capfd):
    """The largest batch size of the graph mode (2^19 rows over an SRS of 2^19, c = 19): mixed columns under each of the
    four pipeline x graph settings, each against the closed form over the coefficient basis."""
    k = 19
    n = 1 << k
    s = S_SRS + 19
    srs = ctx.srs_setup_with_s(k, cref.fr_const(s))
    pool = _cols(cref, 19, n, 4019, names={"half", "half_plus_one", "all_ones_runs", "top_carry", "boolean", "all_equal", "random"})
    names = list(pool)
    want = {nm: _closed_form(cref, pool[nm], s) for nm in names}
    bufs = {nm: ctx.to_device(col) for nm, col in pool.items()}
    monkeypatch.setenv("ZK_MSM_TRACE", "1")
    for count, (pipes, graph) in ((5, ("2", "1")), (4, ("1", "1")), (5, ("2", "0")), (3, ("1", "0"))):
        monkeypatch.setenv("ZK_MSM_PIPES", pipes)
        monkeypatch.setenv("ZK_MSM_GRAPH", graph)
        batch = _mixed_batch(pool, count, count)
        capfd.readouterr()
        got = ctx.commit_batch(srs, [bufs[nm].ptr for nm in batch], n, narrow=[0] * count)
        err = capfd.readouterr().err
        label = f"2^19, {count} columns, PIPES={pipes} GRAPH={graph}"
        bad = [f"{i}:{nm}" for i, nm in enumerate(batch) if not np.array_equal(got[i], want[nm])]
        assert not bad, f"{label}: columns {bad} differ from the closed form"
        assert ("(graph replay)" in err) == (graph == "1" and count >= 4), f"{label}: trace {err!r}"
    for b_ in bufs.values():
        b_.free()
    srs.destroy()


@pytest.mark.parametrize("k", range(12, 21))
def test_narrow_and_gm_paths(ctx, cref, monkeypatch, k):
    """Columns hinted small-valued take the per-window plan of the SRS (c = k - 4: the GM partition instances 8 .. 16 at
    k = 12 .. 20), next to dense columns on the merged plan, n = 2^12 - 37.  Forced narrow on full-range columns, forced
    dense on small ones, the digit-matrix sort instead of GM, 1 / 2 / 4 bucket sets, groups of 1 / 5 / 16 and the table-less
    path: every commitment = best_multiexp over the first n Lagrange bases."""
    n = (1 << 12) - 37
    cn = k - 4
    srs = ctx.srs_setup_with_s(k, cref.fr_const(S_SRS + 100 + k))
    basis = srs.download_g_lagrange()[:n]
    rng = random.Random(5000 + k)
    cols, hints = {}, []
    edge = _cols(cref, cn, n, 5000 + k, names={"half", "half_plus_one", "all_ones_runs", "top_carry", "top_only", "low_only", "boolean"})
    dense = _cols(cref, k, n, 5100 + k, names={"random", "r_minus_1", "top_carry"})
    for bits in (1, 8, 16, 30, 64):
        cols[f"small{bits}"] = cref.to_mont([rng.randrange(1 << bits) if rng.random() < 0.7 else 0 for _ in range(n)])
        hints.append(1)
        if bits == 8:
            cols["dense_random"] = dense["random"]
            hints.append(0)
    for nm, col in edge.items():
        cols[f"pw_{nm}"] = col
        hints.append(1)
    for nm in ("r_minus_1", "top_carry"):
        cols[f"dense_{nm}"] = dense[nm]
        hints.append(0)
    names = list(cols)
    want = [cref.best_multiexp(cols[nm], basis) for nm in names]
    bufs = {nm: ctx.to_device(col) for nm, col in cols.items()}
    settings = [{}, {"ZK_MSM_NARROW": "1"}, {"ZK_MSM_NARROW": "0"}, {"ZK_MSM_NARROW_GM": "0"}, {"ZK_MSM_GM_SETS": "1"},
                {"ZK_MSM_GM_SETS": "4"}, {"ZK_MSM_NARROW_GROUP": "1"}, {"ZK_MSM_NARROW_GROUP": "5"}, {"ZK_MSM_NARROW_GROUP": "16"},
                {"ZK_MSM_NARROW_GROUP": "16", "ZK_MSM_GM_SETS": "4"}, {"ZK_MSM_TABLE_GB": "0"}]
    for env in settings:
        for var, val in env.items():
            monkeypatch.setenv(var, val)
        bad = _bad(names, _commit(ctx, srs, bufs, n, True, narrow=hints), want)
        for var in env:
            monkeypatch.delenv(var)
        assert not bad, f"SRS 2^{k} (per-window c = {cn}), {env or 'default'}: {bad} differ from best_multiexp"
    for b_ in bufs.values():
        b_.free()
    srs.destroy()


def test_graph_replay_mixes_the_three_step_kinds(ctx, cref, srs12, bases12, monkeypatch, capfd):
    """One batch of nine columns hinted 0 / 1 / 2 in turn over the Lagrange basis, n = 2^12 - 5: dense columns (one-launch sort),
    small-valued columns (per-window sort) and hint-2 columns that the run path leaves to the ordinary one (sliced sort: their
    scalars are independent, n random values have about n runs against the run path's cap of n / 16, and it takes no column
    below 4096 rows at all).  ZK_MSM_NARROW_GROUP=1 keeps the columns single, which graph mode asks for.  Under ZK_MSM_GRAPH x
    ZK_MSM_PIPES every commitment = best_multiexp, and the trace says "(graph replay)" exactly when graphs are on."""
    n, count = (1 << 12) - 5, 9
    rng = random.Random(8100)
    hints = [i % 3 for i in range(count)]
    cols = [cref.to_mont([rng.randrange(1 << 30) if rng.random() < 0.7 else 0 for _ in range(n)]) if h == 1 else cref.rand_fr_stream(8100 + i, n) for i, h in enumerate(hints)]
    want = [_want(cref, col, bases12[True], ("k12", True), n) for col in cols]
    bufs = [ctx.to_device(col) for col in cols]
    monkeypatch.setenv("ZK_MSM_NARROW_GROUP", "1")
    monkeypatch.setenv("ZK_MSM_TRACE", "1")
    for pipes, graph in _pipeline_settings():
        monkeypatch.setenv("ZK_MSM_PIPES", pipes)
        monkeypatch.setenv("ZK_MSM_GRAPH", graph)
        capfd.readouterr()
        got = ctx.commit_batch(srs12, [b_.ptr for b_ in bufs], n, lagrange=True, narrow=hints)
        err = capfd.readouterr().err
        bad = [i for i in range(count) if not np.array_equal(got[i], want[i])]
        assert not bad, f"PIPES={pipes} GRAPH={graph}: columns {bad} (hints {hints}) differ from best_multiexp"
        assert ("(graph replay)" in err) == (graph == "1"), f"PIPES={pipes} GRAPH={graph}: trace {err!r}"
    for b_ in bufs:
        b_.free()


@pytest.fixture(scope="module")
def random_bases(cref):
    """2^16 unstructured points with the identity, repeated points and P, -P pairs among them (test_msm_edge_cases)"""
    n = 1 << 16
    P = cref.g1_mul(cref.affine_to_mont([bn254.G1_GEN] * n), cref.rand_fr_stream(6000, n))
    for i in (5, 300, n - 1):
        P[i] = 0
    for i in (7, 1000, 40000):
        P[i + 1] = P[i]
    for i in (9, 2000, 50000):
        P[i + 1] = P[i]
        P[i + 1, 4:] = cref.to_mont([bn254.P_MOD - cref.from_mont(P[i, 4:].reshape(1, 4), 1)[0]], 1)[0]
    return P


@pytest.fixture(scope="module")
def srs21_g(ctx, cref):
    srs = ctx.srs_setup_with_s(21, cref.fr_const(S_SRS + 21))
    g = srs.download_g()
    srs.destroy()
    return g


EDGE_FAMILIES = ("half", "half_plus_one", "all_ones_runs", "top_carry", "top_only", "low_only")


def _mixed_scalars(cref, c, n, seed):
    """The families of a c-bit plan in one column of n rows: the edge families whole and first, then the others interleaved
    (one value of each in turn), cycled to n rows.  Every edge family must fit whole and every other family must have a value
    in the first n rows -- at n = 255 (c = 4) the bulky lists (one_hot, sparse, random) would otherwise crowd the edges out."""
    fams = families(c, (256 + c - 1) // c, 0, None, random.Random(seed))
    vals, rows = [], {}
    for name in EDGE_FAMILIES:
        rows[name] = range(len(vals), len(vals) + len(fams[name]))
        vals += fams[name]
    rest = [name for name in fams if name not in EDGE_FAMILIES]
    for i in range(max(len(fams[name]) for name in rest)):
        for name in rest:
            if i < len(fams[name]):
                rows.setdefault(name, range(len(vals), len(vals) + 1))
                vals.append(fams[name][i])
    for name in EDGE_FAMILIES:
        assert rows[name].stop <= n, f"c = {c}, n = {n}: {name} does not fit whole into the column"
    missing = [name for name in fams if fams[name] and rows[name].start >= n]
    assert not missing, f"c = {c}, n = {n}: families {missing} fall outside the column"
    return np.resize(cref.to_mont(vals), (n, 4))


@pytest.mark.parametrize("c", range(4, 17))
def test_arbitrary_base_path_every_window_size(ctx, cref, random_bases, srs21_g, c):
    """ctx.best_multiexp (make_plan(n): c = clamp(log2 n - 4, 4, 16)) at n = 2^(c+4), and 2^(c+4) +- 1 for c in {4, 9, 13, 16},
    on the edge families of that plan: best_multiexp over unstructured bases up to 2^16, the closed form over s^i G above."""
    n0 = 1 << (c + 4)
    for n in ([n0 - 1, n0, n0 + 1] if c in (4, 9, 13, 16) else [n0]):
        S = _mixed_scalars(cref, c, n, 7000 + c)
        if n <= 1 << 16:
            P = random_bases[:n]
            want = cref.best_multiexp(S, P)
        else:
            P = srs21_g[:n]
            want = _closed_form(cref, S, S_SRS + 21)
        got = ctx.best_multiexp(S, np.ascontiguousarray(P))
        assert np.array_equal(got, want), f"best_multiexp, n = {n} (plan c = {max(4, min(n.bit_length() - 5, 16))}): differs from the oracle"

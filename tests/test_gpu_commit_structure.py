"""GPU parity for the structure-reading commitment paths of csrc/runs.hip (hint 2: run ends against the prefix-sum table of the
basis; hint 3: first differences over the prefix basis) at their boundaries: the seams of the three-level prefix table, run ends
at chosen lanes and workgroup edges, run-end counts on both sides of every threshold, batches that cross the column groups, and
the byte digits of the common increment.

The reference is always best_multiexp of the column itself over the same basis, compared bit for bit on the affine point.  The
bases carry no structure (hash-to-curve points), so a wrong prefix entry cannot cancel.  Every fallback of runs.hip yields the
same point through the ordinary path, so each batch is committed with profiling off and again with profiling on, and the launch
counts of the scopes of runs.hip say which path ran."""
import os

import numpy as np
import pytest

from oracle import bn254

pytestmark = pytest.mark.gpu

R = bn254.R_MOD
K_MAX = 17
SCOPES = ("runs_prefix_table", "runs_collect", "runs_direct", "runs_ends_msm", "diff_fixed_table", "diff_mode", "diff_sparse")


@pytest.fixture(scope="module")
def points(cref):
    """Two sets of 2^17 points without structure, computed once; a test takes the first 2^k of each."""
    g = cref.hash_to_curve_points(0x5EA35, 1 << K_MAX)
    gl = cref.hash_to_curve_points(0x5EA35 + 1, 1 << K_MAX)
    g.flags.writeable = False
    gl.flags.writeable = False
    return g, gl


def _srs(ctx, points, k):
    g, gl = points
    return ctx.srs_create(k, g[:1 << k], gl[:1 << k])


def _commit(ctx, srs, bufs, n, hints, lagrange, profile):
    if profile:
        ctx.prof_enable(1)
        ctx.prof_reset()
    try:
        got = ctx.commit_batch(srs, [b_.ptr for b_ in bufs], n, lagrange=lagrange, narrow=hints)
        counts = {nm: ctx.prof_get(nm)[1] for nm in SCOPES} if profile else None
    finally:
        if profile:
            ctx.prof_enable(0)
    return got, counts


def _check(ctx, srs, bufs, n, hints, want, names, label, lagrange=True, first_profiled=False):
    """Commits the batch with profiling off, then on (first_profiled: once more before both, for what only a fresh SRS shows);
    every result against `want` each time.  Returns the scope counts of the first call (or None) and of the last."""
    first = None
    for profile in ([True] if first_profiled else []) + [False, True]:
        got, counts = _commit(ctx, srs, bufs, n, hints, lagrange, profile)
        bad = [nm for nm, g_, w_ in zip(names, got, want) if not np.array_equal(g_, w_)]
        assert not bad, f"{label}, profiling {'on' if profile else 'off'}: {bad} differ from best_multiexp"
        if first_profiled and first is None:
            first = counts
    return first, counts


def _run_ends(col):
    """Run ends the way k_runs_collect counts them: rows with z_i != z_{i+1}, z_n = 0."""
    nxt = np.vstack([col[1:], np.zeros((1, 4), dtype=np.uint64)])
    return np.flatnonzero(np.any(col != nxt, axis=1))


def _runs_ending_at(ends, values, n):
    """Runs of values[0], values[1], ... that end at the rows `ends`; zero after the last end."""
    col = np.zeros((n, 4), dtype=np.uint64)
    lo = 0
    for j, e in enumerate(ends):
        col[lo:e + 1] = values[j]
        lo = e + 1
    return col


def _random_runs(cref, rng, seed, n, count):
    """`count` runs of random lengths that cover every row, a random field element each: `count` run ends, the last at row n - 1."""
    cuts = np.sort(rng.choice(np.arange(1, n), size=count - 1, replace=False)) if count > 1 else np.array([], dtype=np.int64)
    lengths = np.diff(np.concatenate([[0], cuts, [n]]))
    return np.repeat(cref.rand_fr_stream(seed, count), lengths, axis=0)


def _free(bufs):
    for b_ in bufs:
        b_.free()


# ---- (a) one run end at every seam of the prefix table ---------------------------------------------------------------------------
@pytest.mark.parametrize("k", [13, 17])
def test_step_columns_probe_every_seam_of_the_prefix_table(ctx, cref, points, k):
    """v on rows 0..e and zero after has one run end: the commitment is v * P_e, one entry of the prefix-sum table.  e at every
    seam of the three levels of 64-point segments (64, 4096 and their neighbours, the first and last rows; at k = 17 also the
    second third-level entry and the middle of the table), v = 1, r - 1 and a random value: 36 columns at k = 13, 50 at k = 17
    (two launches of the collection kernel).  Both bases.  The table is built by the first call on a fresh SRS and not again."""
    n = 1 << k
    rows = [0, 1, 62, 63, 64, 65, 127, 128, 4094, 4095, 4096, 4097, n - 2, n - 1]
    if k == 17:
        rows += [8191, 8192, 65535, 65536]
    rnd = cref.rand_fr_stream(0xA0 + k, len(rows))
    values = {"one": cref.fr_const(1)[0], "r_minus_1": cref.fr_const(R - 1)[0]}
    cols, names = [], []
    for j, e in enumerate(rows):
        # a full-length column of a field-sized value costs the oracle half a second: the late rows take two of the three values
        for vn in ("one", "r_minus_1", "random") if e < n // 4 else ("one", ("r_minus_1", "random")[j % 2]):
            col = np.zeros((n, 4), dtype=np.uint64)
            col[:e + 1] = rnd[j] if vn == "random" else values[vn]
            assert list(_run_ends(col)) == [e]
            cols.append(col)
            names.append(f"e={e},v={vn}")
    srs = _srs(ctx, points, k)
    bufs = [ctx.to_device(c) for c in cols]
    hints = [2] * len(cols)
    for lagrange in (True, False):
        basis = points[1 if lagrange else 0][:n]
        want = [cref.best_multiexp(c, basis) for c in cols]
        first, again = _check(ctx, srs, bufs, n, hints, want, names, f"k {k}, lagrange {lagrange}", lagrange=lagrange, first_profiled=True)
        assert first["runs_prefix_table"] == 1 and again["runs_prefix_table"] == 0, (first, again)
        assert first["runs_direct"] >= 1 and again["runs_direct"] >= 1, (first, again)
    _free(bufs)
    srs.destroy()


# ---- (b) where a run end sits inside the collection kernel -----------------------------------------------------------------------
def test_run_ends_at_chosen_lanes_and_workgroup_edges(ctx, cref, points):
    """Run ends only at chosen rows of a 2^13 column: lane 0 and lane 63 of a wave, the last row of a workgroup and the first of
    the next, row n - 1 alone (one run over every row), row 0 alone, a workgroup whose 256 rows are all run ends (every wave's
    offset inside the workgroup's reservation), the same in the last workgroup, and a column that ends in a zero run.  Again at
    n = 2^13 - 37 on the same SRS, where z_n := 0 closes the last run at P_{n-1} inside the table and the last workgroup is
    partly empty.  Both bases."""
    k = 13
    srs = _srs(ctx, points, k)
    for n in (1 << k, (1 << k) - 37):
        uni = cref.rand_fr_stream(0xB0 + (n & 1), n)
        w = uni[7]
        last_wg = 256 * ((n - 1) // 256)
        cols = {
            "ends_0_63_64_255_256_last": _runs_ending_at([0, 63, 64, 255, 256, n - 1], uni[10:16], n),
            "only_row_last": np.repeat(uni[3:4], n, axis=0),
            "only_row_0": _runs_ending_at([0], uni[4:5], n),
            "rows_512_767_all_differ": np.repeat(w[None, :], n, axis=0),
            "last_workgroup_all_differ": np.repeat(w[None, :], n, axis=0),
            "ends_in_a_zero_run": _runs_ending_at([100, 4095, 4096, n - 300], uni[20:24], n),
        }
        cols["rows_512_767_all_differ"][512:768] = uni[512:768]
        cols["last_workgroup_all_differ"][last_wg:] = uni[last_wg:]
        ends = {nm: list(_run_ends(c)) for nm, c in cols.items()}
        assert ends["ends_0_63_64_255_256_last"] == [0, 63, 64, 255, 256, n - 1]
        assert ends["only_row_last"] == [n - 1] and ends["only_row_0"] == [0]
        assert ends["rows_512_767_all_differ"] == list(range(511, 768)) + [n - 1]
        assert ends["last_workgroup_all_differ"] == list(range(last_wg - 1, n))
        assert ends["ends_in_a_zero_run"] == [100, 4095, 4096, n - 300]
        assert max(len(e) for e in ends.values()) < n // 16                   # every column stays on the run-end path
        names = list(cols)
        bufs = [ctx.to_device(cols[nm]) for nm in names]
        for lagrange in (True, False):
            basis = points[1 if lagrange else 0][:n]
            want = [cref.best_multiexp(cols[nm], basis) for nm in names]
            _, counts = _check(ctx, srs, bufs, n, [2] * len(names), want, names, f"n {n}, lagrange {lagrange}", lagrange=lagrange)
            assert counts["runs_direct"] >= 1 and counts["runs_ends_msm"] == 0, counts
        _free(bufs)
    srs.destroy()


# ---- (c) run-end counts on both sides of every threshold -------------------------------------------------------------------------
def test_run_end_counts_around_the_direct_limit_and_the_cap_2_17(ctx, cref, points):
    """n = 2^17: cap = n / 16 = 8192 run ends, of which up to 4096 are summed directly.  Columns with exactly 4095 and 4096 ends
    (direct), 4097 and 8192 (the bucket method over the collected ends, one call each) and 8193 (not run-structured: the
    ordinary path, its list of ends cut off at the cap).  The column past the cap comes first, so the slot right after its
    list belongs to a column that is summed."""
    k, n = 17, 1 << 17
    rng = np.random.default_rng(0xC17)
    counts_wanted = [8193, 4095, 4096, 4097, 8192]
    cols = [_random_runs(cref, rng, 0xC0 + j, n, m) for j, m in enumerate(counts_wanted)]
    for c, m in zip(cols, counts_wanted):
        assert _run_ends(c).size == m
    names = [f"{m}_ends" for m in counts_wanted]
    srs = _srs(ctx, points, k)
    bufs = [ctx.to_device(c) for c in cols]
    want = [cref.best_multiexp(c, points[1]) for c in cols]
    _, counts = _check(ctx, srs, bufs, n, [2] * len(cols), want, names, "k 17")
    assert counts["runs_direct"] >= 1 and counts["runs_ends_msm"] == 2, counts
    _free(bufs)
    srs.destroy()


def test_run_end_counts_around_the_cap_2_12_zero_columns_and_no_table_for_nothing(ctx, cref, points):
    """n = 2^12, the smallest size the path accepts: cap = 256.  Columns with 255 and 256 run ends are summed directly, those
    with 257 take the ordinary path (each followed by a column that is summed); nothing reaches the bucket method over run
    ends.  A batch of all-zero columns has no run end at all: identity encodings, nothing multiplied.  On a fresh SRS a batch
    whose hinted columns all have a run end per row builds no prefix table: the counting sweep declines."""
    k, n = 12, 1 << 12
    rng = np.random.default_rng(0xC12)
    counts_wanted = [257, 255, 257, 256]
    cols = [_random_runs(cref, rng, 0xD0 + j, n, m) for j, m in enumerate(counts_wanted)]
    for c, m in zip(cols, counts_wanted):
        assert _run_ends(c).size == m
    names = [f"{m}_ends_{j}" for j, m in enumerate(counts_wanted)]
    basis = points[1][:n]
    srs = _srs(ctx, points, k)
    bufs = [ctx.to_device(c) for c in cols]
    want = [cref.best_multiexp(c, basis) for c in cols]
    _, counts = _check(ctx, srs, bufs, n, [2] * len(cols), want, names, "k 12")
    assert counts["runs_direct"] >= 1 and counts["runs_ends_msm"] == 0, counts
    _free(bufs)

    zero = np.zeros((n, 4), dtype=np.uint64)
    identity = np.zeros(8, dtype=np.uint64)                                    # 64 zero bytes
    assert np.array_equal(cref.best_multiexp(zero, basis), identity)
    bufs = [ctx.to_device(zero) for _ in range(3)]
    _, counts = _check(ctx, srs, bufs, n, [2, 2, 2], [identity] * 3, ["zero_0", "zero_1", "zero_2"], "k 12, all-zero batch")
    assert counts["runs_collect"] >= 1 and counts["runs_direct"] == 0 and counts["runs_ends_msm"] == 0, counts
    _free(bufs)
    srs.destroy()

    srs = _srs(ctx, points, k)
    cols = [cref.rand_fr_stream(0xE0 + j, n) for j in range(3)]
    for c in cols:
        assert _run_ends(c).size == n
    bufs = [ctx.to_device(c) for c in cols]
    want = [cref.best_multiexp(c, basis) for c in cols]
    first, again = _check(ctx, srs, bufs, n, [2, 2, 2], want, ["differs_0", "differs_1", "differs_2"], "k 12, a run end per row", first_profiled=True)
    for counts in (first, again):
        assert counts["runs_collect"] >= 1 and counts["runs_prefix_table"] == 0 and counts["runs_direct"] == 0, counts
    _free(bufs)
    srs.destroy()


# ---- (d) batches that cross the column groups ------------------------------------------------------------------------------------
def test_seventy_columns_cross_the_collection_groups(ctx, cref, points):
    """66 columns hinted 2 (three launches of the collection kernel: 32 + 32 + 2) with a dense, a small-valued, a running-sum and
    another dense column between them.  The kinds cycle through few runs, all zero, one run and a run end per row, shifted by one
    at every 32nd column, so that the 32nd, 33rd, 64th and 65th hinted columns are of four different kinds.  Also with the
    feature off."""
    k, n = 12, 1 << 12
    rng = np.random.default_rng(0xD12)
    kinds = ["few_runs", "zero", "one_run", "every_row_differs"]
    others = {5: (0, "dense"), 20: (1, "small"), 40: (3, "running_sum"), 60: (0, "dense")}
    cols, hints, names, hinted_kinds = [], [], [], []
    for pos in range(70):
        if pos in others:
            hint, kind = others[pos]
            if kind == "dense":
                col = cref.rand_fr_stream(0x100 + pos, n)
            elif kind == "small":
                col = cref.to_mont([int(v) for v in rng.integers(0, 1 << 16, size=n)])
            else:
                inc = np.repeat(cref.rand_fr_stream(0x100 + pos, 1), n, axis=0)
                active = rng.choice(n - 1, size=n // 12, replace=False)
                inc[active] = cref.rand_fr_stream(0x200 + pos, active.size)
                col = cref.prefix_sum(inc)
        else:
            i = len(hinted_kinds)
            hint, kind = 2, kinds[(i + i // 32) % 4]
            hinted_kinds.append(kind)
            if kind == "few_runs":
                col = _random_runs(cref, rng, 0x100 + pos, n, 11)
            elif kind == "zero":
                col = np.zeros((n, 4), dtype=np.uint64)
            elif kind == "one_run":
                col = np.repeat(cref.rand_fr_stream(0x100 + pos, 1), n, axis=0)
            else:
                col = cref.rand_fr_stream(0x100 + pos, n)
        cols.append(col)
        hints.append(hint)
        names.append(f"{pos}:{kind}")
    assert len(hinted_kinds) == 66 and len({hinted_kinds[i] for i in (31, 32, 63, 64)}) == 4
    basis = points[1][:n]
    want = [cref.best_multiexp(c, basis) for c in cols]
    srs = _srs(ctx, points, k)
    bufs = [ctx.to_device(c) for c in cols]
    _, counts = _check(ctx, srs, bufs, n, hints, want, names, "70 columns")
    assert counts["runs_collect"] >= 3 and counts["runs_direct"] >= 3, counts
    os.environ["ZK_MSM_RUNS"] = "0"
    try:
        _, counts = _check(ctx, srs, bufs, n, hints, want, names, "70 columns, ZK_MSM_RUNS=0")
    finally:
        os.environ.pop("ZK_MSM_RUNS", None)
    assert counts["runs_collect"] == 0 and counts["runs_direct"] == 0, counts
    _free(bufs)
    srs.destroy()


# ---- (e) first differences -------------------------------------------------------------------------------------------------------
C_FF_LOW = int.from_bytes(b"\xff\x00" * 16, "little")                             # 0x00FF00FF...00FF: bytes 0xFF, 0x00, 0xFF, ...
C_FF_HIGH = int.from_bytes(b"\x00\xff" * 16, "little") % R                       # 0xFF00FF00...FF00 reduced mod r
INCREMENTS = [("c=0", 0), ("c=1", 1), ("c=r-1", R - 1), ("c=00ff..", C_FF_LOW), ("c=ff00..", C_FF_HIGH), ("c=random", None)]


def _running_sum(cref, c_mont, n, active, seed, start=None, last_is_zero=False, blinding=False):
    """phi_0 = start, phi_{j+1} - phi_j = c except on the rows `active`, which carry random increments."""
    inc = np.repeat(c_mont[None, :], n, axis=0)
    active = np.asarray(active, dtype=np.int64)
    if active.size:
        inc[active] = cref.rand_fr_stream(seed, active.size)
    col = cref.prefix_sum(inc)
    if last_is_zero:
        start = cref.fe_binop("sub", 0, np.zeros((1, 4), dtype=np.uint64), col[n - 1:n])[0]
    if start is not None:
        col = cref.fe_binop("add", 0, col, np.repeat(start[None, :], n, axis=0))
    if blinding:
        col[n - 6:] = cref.rand_fr_stream(seed + 1, 6)
    return col


def _difference_columns(cref, n):
    """38 columns: 35 whose increments are mostly equal (they take the difference path: three chunks of 16, 16 and 3) and three
    that are turned away by the vote.  The 35 cycle through the six common increments and through five shapes (6 and 5 are
    coprime, so neighbours differ in both), which makes the 16th, 17th, 32nd and 33rd column four different kinds whether one
    counts all columns or only the kept ones."""
    rng = np.random.default_rng(0xE12)
    rnd = cref.rand_fr_stream(0xE0E0, 64)

    def spread(share):
        return rng.choice(n - 1, size=int(share * n), replace=False)
    shapes = ["no_active_rows", "twelfth_active", "active_pinned_0_and_last", "last_value_zero", "blinding_rows"]
    turned_away = {3: ("share_0.38", 0.38), 20: ("share_0.7", 0.7), 36: ("two_increments", None)}
    cols, names, kept = [], [], []
    for pos in range(38):
        seed = 0x300 + 2 * pos
        if pos in turned_away:
            nm, share = turned_away[pos]
            if share is None:                                                   # two increments on half the rows each
                inc = np.repeat(rnd[40:41], n, axis=0)
                inc[rng.choice(n, size=n // 2, replace=False)] = rnd[41]
                col = cref.prefix_sum(inc)
            else:
                col = _running_sum(cref, rnd[42 + pos % 2], n, spread(share), seed, start=rnd[44])
            names.append(f"{pos}:{nm}")
        else:
            i = len(kept)
            cname, c = INCREMENTS[i % 6]
            shape = shapes[i % 5]
            c_mont = rnd[i] if c is None else cref.fr_const(c)[0]
            if shape == "no_active_rows":
                col = _running_sum(cref, c_mont, n, [], seed)
            elif shape == "twelfth_active":
                col = _running_sum(cref, c_mont, n, spread(1 / 12), seed, start=rnd[45])
            elif shape == "active_pinned_0_and_last":
                col = _running_sum(cref, c_mont, n, np.union1d(spread(1 / 12), [0, n - 3, n - 2, n - 1]), seed, start=rnd[46])
            elif shape == "last_value_zero":
                col = _running_sum(cref, c_mont, n, spread(1 / 12), seed, last_is_zero=True)
                assert not col[n - 1].any()
            else:
                col = _running_sum(cref, c_mont, n, spread(1 / 12), seed, start=rnd[47], blinding=True)
            kept.append((cname, shape))
            names.append(f"{pos}:{cname},{shape}")
        cols.append(col)
    assert len(kept) == 35 and len({kept[i] for i in (15, 16, 31, 32)}) == 4
    assert len({names[i].split(":")[1] for i in (15, 16, 31, 32)}) == 4
    return cols, names


def test_running_sums_through_their_first_differences_2_12(ctx, cref, points):
    """Hint 3 over the Lagrange basis at n = 2^12.  Common increment c = 0, 1, r - 1, 0x00FF..00FF, 0xFF00..FF00 mod r and random
    (the 32 byte digits of k_fixed_mul at 0x00, 0x01 and 0xFF); no active rows, a twelfth of them, active rows pinned at both
    ends, phi_{n-1} = 0, six blinding rows; and columns with 38 % and 70 % active rows and with two increments on half the rows
    each, which the vote of the 256 sampled increments turns away wherever the samples fall (62 %, 30 % and 50 % agree, 75 % are
    asked): for those the result alone is asserted.  35 columns are kept: three chunks of difference images.  The same columns
    cut to n = 2^12 - 37, over the coefficient basis and with the feature off take the ordinary path."""
    k, n = 12, 1 << 12
    cols, names = _difference_columns(cref, n)
    hints = [3] * len(cols)
    srs = _srs(ctx, points, k)
    bufs = [ctx.to_device(c) for c in cols]
    want = [cref.best_multiexp(c, points[1][:n]) for c in cols]
    first, again = _check(ctx, srs, bufs, n, hints, want, names, "hint 3", first_profiled=True)
    for counts in (first, again):
        assert counts["diff_sparse"] >= 3 and counts["diff_mode"] >= 2, counts
    assert first["diff_fixed_table"] == 1 and again["diff_fixed_table"] == 0, (first, again)

    m = n - 37
    want_m = [cref.best_multiexp(c[:m], points[1][:m]) for c in cols]
    _, counts = _check(ctx, srs, bufs, m, hints, want_m, names, "hint 3, n below 2^k")
    assert counts["diff_sparse"] == 0, counts
    want_g = [cref.best_multiexp(c, points[0][:n]) for c in cols]
    _, counts = _check(ctx, srs, bufs, n, hints, want_g, names, "hint 3, coefficient basis", lagrange=False)
    assert counts["diff_sparse"] == 0, counts
    os.environ["ZK_MSM_DIFF"] = "0"
    try:
        _, counts = _check(ctx, srs, bufs, n, hints, want, names, "hint 3, ZK_MSM_DIFF=0")
    finally:
        os.environ.pop("ZK_MSM_DIFF", None)
    assert counts["diff_sparse"] == 0 and counts["diff_mode"] == 0, counts
    _free(bufs)
    srs.destroy()


def test_running_sums_through_their_first_differences_2_17(ctx, cref, points):
    """Four running sums at n = 2^17, where the prefix basis' own window tables are built at a size at which they are used: a
    twelfth of the rows active, the same starting elsewhere, every increment different (turned away), flat with steps (c = 0)."""
    k, n = 17, 1 << 17
    rng = np.random.default_rng(0xE17)
    rnd = cref.rand_fr_stream(0xE1E1, 4)
    active = rng.choice(n - 1, size=n // 12, replace=False)
    zero = np.zeros(4, dtype=np.uint64)
    cols = {
        "lookup_like": _running_sum(cref, rnd[0], n, active, 0x400, blinding=True),
        "starts_elsewhere": _running_sum(cref, rnd[0], n, active, 0x400, start=rnd[1], blinding=True),
        "all_increments_differ": cref.prefix_sum(cref.rand_fr_stream(0x402, n)),
        "flat_with_steps": _running_sum(cref, zero, n, np.arange(0, n, 97), 0x404),
    }
    names = list(cols)
    srs = _srs(ctx, points, k)
    bufs = [ctx.to_device(cols[nm]) for nm in names]
    want = [cref.best_multiexp(cols[nm], points[1]) for nm in names]
    _, counts = _check(ctx, srs, bufs, n, [3] * 4, want, names, "hint 3, k 17")
    assert counts["diff_sparse"] >= 1 and counts["diff_mode"] >= 2, counts
    _free(bufs)
    srs.destroy()


# ---- (f) both hints in one batch -------------------------------------------------------------------------------------------------
def test_run_and_difference_hints_in_one_batch(ctx, cref, points):
    """Hints [3, 2, 2, 3, 0, 1]: the first hint-2 column has a run end per row and is left over by the run-end path, the second
    has few runs and is taken, so the rest of the batch is submitted again -- and then once more, behind the difference path."""
    k, n = 12, 1 << 12
    rng = np.random.default_rng(0xF12)
    rnd = cref.rand_fr_stream(0xF0F0, 4)
    cols = {
        "running_sum": _running_sum(cref, rnd[0], n, rng.choice(n - 1, size=n // 12, replace=False), 0x500, start=rnd[1]),
        "every_row_differs": cref.rand_fr_stream(0x502, n),
        "few_runs": _random_runs(cref, rng, 0x504, n, 9),
        "running_sum_c_1": _running_sum(cref, cref.fr_const(1)[0], n, rng.choice(n - 1, size=n // 12, replace=False), 0x506, blinding=True),
        "dense": cref.rand_fr_stream(0x508, n),
        "small": cref.to_mont([int(v) for v in rng.integers(0, 1 << 16, size=n)]),
    }
    names = list(cols)
    srs = _srs(ctx, points, k)
    bufs = [ctx.to_device(cols[nm]) for nm in names]
    want = [cref.best_multiexp(cols[nm], points[1][:n]) for nm in names]
    _check(ctx, srs, bufs, n, [3, 2, 2, 3, 0, 1], want, names, "hints 3 2 2 3 0 1")
    _free(bufs)
    srs.destroy()

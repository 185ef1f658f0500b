"""CPU checks of the MSM batch plan (csrc/msm_plan.hpp: plan_batch, carve_sort_ws, carve_buckets) through the host-only view
zk_host_msm_batch_plan, over the grid of msm_batch_plan_cases.py: every k, size class, column count, hint pattern, blinded tail,
group cap and ZK_MSM_* setting.  The conditions are restated here from what the kernels of csrc/msm.hip need -- their constants and
comments -- and are not read back from the library."""
import pytest

from msm_batch_plan_cases import grid, msm_env
from zkevm_circuits_amd import binding

# the kernels' constants (csrc/msm_plan.hpp names them; csrc/msm.hip says what they bound)
SLICES = 4                     # slice workgroups per bucket range: [bucket][slice] counters, read as one uint4
SCAN_BLOCK = 1024 * 4          # counts per block of the scans
WFLAGS = 256                   # window flags of one sort
CLEARED = 256 + 4 + WFLAGS + (1 << 17)      # size bins, nmulti, window flags, done-counters: one memset
TASK_CAP, TASK_TARGET = 48, 1 << 18
RED_G_WIDE, RED_THREADS = 8, 256
M_STAGE = 15 * 1024            # indices of one partition in k_msm_m_binsort's LDS
M_CHUNK, M_SCHUNK = 2048, 1024
RANGE_MAX_BITS = 11
GM_MAX_COLS = 16
GRAPH_PIPES = 4


def ceil_div(a, b):
    return -(-a // b)


def knob(env, name):
    return int(env[name]) if name in env else None


@pytest.fixture(scope="module")
def plans():
    out = []
    for case in grid():
        env, k, n, count, hints, tail, table, cap, prof, broken = case
        with msm_env(env):
            out.append((case, binding.host_msm_batch_plan(k, n, count, hints, tail, bool(table), cap, bool(prof), bool(broken))))
    return out


def effective_hints(env, hints):
    forced = knob(env, "ZK_MSM_NARROW")
    return hints if forced is None else [1 if forced else 0] * len(hints)


def test_grid_is_whole():
    cases = grid()
    assert {c[1] for c in cases} >= set(range(8, 25)) | {27, 28}
    assert {c[3] for c in cases} == {1, 2, 3, 4, 5, 9, 33}
    assert {c[5] for c in cases} == {0, 6, 256, 257} and {c[6] for c in cases} == {0, 1} and {c[7] for c in cases} == {0, 8, 4, 2, 1}
    assert any(2 in c[4] for c in cases) and any(c[4][8:25] == [1] * 17 and c[4][7] == 0 for c in cases if len(c[4]) == 33)
    assert len(cases) < 30000


def check_regions(regs, total, label):
    """regions in the order given ascend, are disjoint and end within `total`"""
    end = 0
    for name, (off, length) in regs.items():
        assert off >= end, f"{label}: {name} at {off} overlaps the region in front of it (ends {end})"
        end = off + length
    assert end <= total, f"{label}: regions end at {end}, beyond {total}"


def test_unsupported_sizes_and_the_32_bit_give_up(plans):
    seen = 0
    for (env, k, n, count, hints, tail, table, cap, prof, broken), p in plans:
        unsupported = p["W"] * (1 << k) >= 1 << 31 or n * p["W"] >= 1 << 32
        assert (p["status"] == 1) == unsupported, f"k = {k}, n = {n}: status {p['status']}"
        if unsupported:
            seen += 1
            assert not p["steps"] and not p["sort"] and not p["buckets"]
        W_n = ceil_div(256, max(4, min(k - 4, 16)))
        if n * W_n >= 1 << 32:           # the per-window path is given up: no column's tail may be split off
            assert not p["any_narrow"] and p["tail_rows"] == 0 and p["n_narrow"] == n
    assert seen


def test_sort_layouts(plans):
    for (env, k, n, count, hints, tail, table, cap, prof, broken), p in plans:
        if p["status"]:
            continue
        label = f"{env} k = {k}, n = {n}, {count} columns"
        assert p["words"] % 64 == 0 and p["copies"] == (GRAPH_PIPES if p["graph"] else p["npipe"]), label
        B, W, B_n, W_n, NG, SG = 1 << (p["c"] - 1), p["W"], 1 << (p["c_n"] - 1), p["W_n"], p["NG"], p["SG"]
        assert p["n_pad"] % (16 * SLICES) == 0 and n <= p["n_pad"] < n + 16 * SLICES
        assert set(p["sort"]) == {"N", "G", "M"} and bool(p["sort"]["N"]["regions"]) == p["any_narrow"] and bool(p["sort"]["G"]["regions"]) == p["gm"]
        for name, lay in p["sort"].items():
            regs = lay["regions"]
            if not regs:
                assert lay["words"] == 0
                continue
            check_regions(regs, lay["words"], f"{label}, layout {name}")
            assert lay["words"] <= p["words"], label
            for r in ("slice_counts", "slice_off", "dig"):
                assert r not in regs or regs[r][0] % 4 == 0, f"{label}: {r} is not 16-B aligned"
            assert "entries" not in regs or regs["entries"][0] % 2 == 0, f"{label}: entries are not 8-B aligned"
            assert regs["cleared"][1] == CLEARED
        # what the kernels index: buckets, [bucket][slice] counters, partition histograms, worst-case entries, the digit matrix
        M, N, G = (p["sort"][x]["regions"] for x in "MNG")
        parts = B >> p["range_bits"]
        assert M["counts"][1] == B and M["slice_counts"][1] == B * SLICES and M["slice_off"][1] >= B * SLICES + 1 and M["hist"][1] == parts * p["nwg"] and M["hist_off"][1] == parts * p["nwg"] + 1
        assert M["idx"][1] == n * W and M["entries"][1] == 2 * n * W and M["block_tot_h"][1] >= ceil_div(parts * p["nwg"], SCAN_BLOCK) and M["block_tot"][1] >= ceil_div(B, SCAN_BLOCK)
        assert M["offsets"][1] == B + 1 and M["toff"][1] == B + 1 and M["order"][1] == B and M["ntasks"][1] == B
        assert parts * p["nwg"] < 1 << 32 and B * SLICES < 1 << 32
        if N:
            nb = NG * W_n * B_n
            assert N["counts"][1] == nb and N["slice_counts"][1] == nb * SLICES and N["idx"][1] == n * W_n * NG and 2 * N["dig"][1] >= p["n_pad"] * W_n * NG
            assert nb * SLICES < 1 << 32 and n * W_n * NG < 1 << 32 and N["block_tot_s"][1] >= ceil_div(nb * SLICES, SCAN_BLOCK)
        if G:
            assert SG <= 4 and G["counts"][1] == NG * SG * B_n and G["hist"][1] == NG * p["bpcG"] * p["nwgG"] and G["idx"][1] == n * W_n * NG and G["entries"][1] == 2 * n * W_n * NG
            assert p["bpcG"] << p["range_bits_G"] == SG * B_n and p["nwgG"] == ceil_div(p["n_narrow"], M_CHUNK) and NG * p["bpcG"] * p["nwgG"] < 1 << 32
            assert p["perm_G"] == (p["range_bits_G"] << 8 | (p["c_n"] - 1 - p["range_bits_G"]))


def test_bucket_buffer(plans):
    for (env, k, n, count, hints, tail, table, cap, prof, broken), p in plans:
        if p["status"]:
            continue
        label = f"{env} k = {k}, n = {n}, {count} columns"
        B, W, B_n, W_n, NG, SG = 1 << (p["c"] - 1), p["W"], 1 << (p["c_n"] - 1), p["W_n"], p["NG"], p["SG"]
        red_blocks_n = ceil_div(ceil_div(B_n, RED_G_WIDE), RED_THREADS)
        assert set(p["buckets"]) == {kind for _, _, kind in p["steps"]}, label
        assert p["npts29"] == max(b["points"] for b in p["buckets"].values()), label
        for kind, b in p["buckets"].items():
            regs = b["regions"]
            check_regions(regs, b["points"], f"{label}, {kind} step")
            if kind in ("dense", "dense_sliced"):
                nb, tasks = B, B + max(n * W // TASK_CAP, TASK_TARGET) + 1
                assert regs["partial"][1] >= max(B // 2048 + 1, B // 4 + 1024) and "folded" not in regs      # the one-launch reduction's partials; the levelled one's scratch
            elif kind == "gm":
                nb, tasks = NG * SG * B_n, NG * SG * B_n + max(n * NG * W_n // TASK_CAP, TASK_TARGET) + 1
                assert SG <= 4 and regs["partial"][1] >= red_blocks_n * NG * SG and "folded" not in regs
            else:
                nb, tasks = NG * W_n * B_n, NG * W_n * B_n + max(n * NG * W_n // TASK_CAP, TASK_TARGET) + 1
                assert regs["partial"][1] >= red_blocks_n * NG and regs["folded"][1] >= B_n * NG
            assert (b["nb"], b["tasks"]) == (nb, tasks), f"{label}, {kind} step"
            assert regs["buckets"][1] >= nb and regs["task_partial"][1] >= tasks, f"{label}, {kind} step"


def test_steps_groups_and_tails(plans):
    kinds_seen = set()
    for (env, k, n, count, hints, tail, table, cap, prof, broken), p in plans:
        if p["status"]:
            continue
        label = f"{env} k = {k}, n = {n}, hints {hints}, tail {tail}, table {table}, cap {cap}"
        hints = effective_hints(env, hints)
        c_n = max(4, min(k - 4, 16))
        W_n = ceil_div(256, c_n)
        narrow_possible = bool(table) and 1 in hints and n * W_n < 1 << 32
        assert p["any_narrow"] == narrow_possible, label
        assert p["tail_rows"] == (tail if narrow_possible and 0 < tail <= 256 and tail + 1024 <= n else 0) and p["n_narrow"] == n - p["tail_rows"], label
        NG = p["NG"]
        assert 1 <= NG <= GM_MAX_COLS and (not cap or NG <= cap), label
        if narrow_possible:
            assert (p["c_n"], p["W_n"]) == (c_n, W_n) and NG * W_n <= WFLAGS and n * W_n * NG < 1 << 32, label
            group = knob(env, "ZK_MSM_NARROW_GROUP")
            assert group is None or NG <= group, label
        else:
            assert NG == 1
        gm = narrow_possible and 8 <= c_n <= 16 and knob(env, "ZK_MSM_NARROW_GM") != 0
        assert p["gm"] == gm, label
        at = 0
        for first, cols, kind in p["steps"]:
            kinds_seen.add(kind)
            assert first == at and cols >= 1, label
            if narrow_possible and hints[first] == 1:
                assert kind == ("gm" if gm and not p["graph"] else "window") and cols <= NG and all(h == 1 for h in hints[first:first + cols]), label
                assert cols == NG or first + cols == count or hints[first + cols] != 1, f"{label}: the group at {first} is not maximal"
            else:
                assert cols == 1 and kind == ("dense_sliced" if hints[first] == 2 or not p["binsort"] else "dense"), label
            at += cols
        assert at == count, label
    assert kinds_seen == {"window", "dense", "dense_sliced", "gm"}


def test_merged_sort_and_modes(plans):
    for (env, k, n, count, hints, tail, table, cap, prof, broken), p in plans:
        if p["status"]:
            continue
        label = f"{env} k = {k}, n = {n}, {count} columns"
        c, W = p["c"], p["W"]
        assert c == (knob(env, "ZK_MSM_C") or max(8, min(k, 22))) and W == ceil_div(256, c), label
        B = 1 << (c - 1)
        rb = max(c - 1 - 10, 0)
        per = n * W // (B >> rb)
        binsort = knob(env, "ZK_MSM_BINSORT") != 0 and per + per // 8 <= M_STAGE
        assert p["binsort"] == binsort and p["range_bits"] == (rb if binsort else min(c - 1, RANGE_MAX_BITS)), label
        assert not binsort or B >> p["range_bits"] <= 1024, label
        staged = binsort and c >= 19 and (2 * 1024 + 16) * 4 + M_SCHUNK * W * 10 <= 150 * 1024 and knob(env, "ZK_MSM_STAGED") != 0
        chunk = knob(env, "ZK_MSM_CHUNK")
        chunk = M_SCHUNK if staged else chunk if chunk is not None and 256 <= chunk <= 65536 else M_CHUNK
        assert (p["staged_scatter"], p["chunk"], p["nwg"]) == (staged, chunk, ceil_div(n, chunk)), label
        pipes = knob(env, "ZK_MSM_PIPES")
        npipe = 1 if pipes == 1 else 2 if pipes == 2 and count >= 2 else 2 if n <= 1 << 19 and count >= 2 else 1
        assert p["npipe"] == npipe, label
        graph = 1024 <= n <= 1 << 19 and count >= 4 and knob(env, "ZK_MSM_GRAPH") != 0 and not prof and not broken and not (p["any_narrow"] and p["NG"] > 1)
        assert p["graph"] == graph, label


def test_cap_retry_shrinks_the_workspace(plans):
    followed, ended = 0, set()
    for (env, k, n, count, hints, tail, table, cap, prof, broken), p in plans:
        if p["status"] or cap or not p["smaller_cap"]:
            continue
        followed += 1
        with msm_env(env):
            words, NG = p["words"], p["NG"]
            while p["smaller_cap"]:
                assert p["smaller_cap"] == NG // 2
                p = binding.host_msm_batch_plan(k, n, count, hints, tail, bool(table), p["smaller_cap"], bool(prof), bool(broken))
                assert p["words"] <= words and p["NG"] <= NG // 2, f"{env} k = {k}, n = {n}"
                words, NG = p["words"], p["NG"]
            ended.add(NG)
        # it ends at single columns -- or earlier where smaller groups could not help any more: the merged layout, which no cap
        # shrinks, is then the larger one (a short MSM over a large SRS, n = 1024 at k = 22; small windows under ZK_MSM_C)
        assert p["smaller_cap"] == 0 and (NG == 1 or max(p["words_N"], p["words_G"]) <= p["words_M"]), f"{env} k = {k}, n = {n}: the retry ends at groups of {NG}"
        if n >= (1 << k) - 37 and "ZK_MSM_C" not in env:         # columns as long as the SRS, the plan's own window size: down to single columns
            assert NG == 1, f"{env} k = {k}, n = {n}: the retry ends at groups of {NG}"
    assert followed > 100 and 1 in ended


def test_graph_key_part_separates_plans(plans):
    by_fields = {}
    for (env, k, n, count, hints, tail, table, cap, prof, broken), p in plans:
        if p["status"]:
            continue
        fields = (n, p["c"], p["c_n"], p["top_shift"], p["nwg"], p["range_bits"], p["staged_scatter"], p["n_narrow"], 1 << k, p["words"])
        assert by_fields.setdefault(fields, p["key"]) == p["key"]
    keys = list(by_fields.values())
    assert len({tuple(k_) for k_ in keys}) == len(keys) > 1000, "two plans that differ in a baked-in value share a key part"


# profiles/r10_msm_host_refactor.md, "-> carve_sort_ws" column: words of the merged, per-window and GM layouts.  The note fixes k, the
# group size and the bucket sets; n = 2^k, every column hinted small-valued.  Its k = 19 row ("graph mode, no groups") does not say how the
# groups were turned off: ZK_MSM_NARROW_GROUP=1 here, four columns.
@pytest.mark.parametrize("k,env,count,NG,want", [(20, {}, 16, 16, (49939852, 511846928, 814875912)), (12, {}, 8, 8, (432656, 2130488, 3295754)),
                                                  (19, {"ZK_MSM_NARROW_GROUP": "1"}, 4, 1, (26608588, 18121592, 28738080))])
def test_word_counts_of_the_workspace_note(k, env, count, NG, want):
    with msm_env(env):
        p = binding.host_msm_batch_plan(k, 1 << k, count, [1] * count)
    assert (p["NG"], p["SG"]) == (NG, 2) and p["graph"] == (k == 19)
    assert (p["words_M"], p["words_N"], p["words_G"]) == want

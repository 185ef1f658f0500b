"""CPU: the launch plans of the NTT (csrc/ntt.hip: split_digits, columns_per_launch, plan_pass, plan_last, seen through the host-only
zk_host_ntt_plan) over the whole knob space and every size: structure, resources, the workgroup numberings of pass_tile / last_tile
(restated here from the kernels' comments; a numbering that is not one-to-one writes some tiles twice and others never, or reads
outside a column), what the plan conditions imply, and that the GPU cases of ntt_cases.py still reach every launch signature."""
import numpy as np
import pytest

import ntt_cases as nc

COLUMNS = (1, 2, 3, 16, 17)
NTT_PASS_MAX_LDS = 4096 * 36              # NTT_TILE elements of nine 4-byte limb planes
NTT_LAST_MAX_LDS = (4096 + 128) * 36      # plus 8 words of padding for each of at most 16 rows


@pytest.fixture(scope="module")
def plans(zk):
    """every plan of the knob space: [(k, columns, knobs, tables asked for, plan)]"""
    out = []
    for knobs in nc.knob_dicts():
        for tables in (True, False):
            with nc.knobs_set(knobs, tables):
                for k in range(1, 29):
                    for columns in COLUMNS:
                        out.append((k, columns, knobs, tables, zk.binding.host_ntt_plan(k, columns, tables)))
    assert len(out) == 128 * 2 * 28 * 5
    return out


def test_structure(plans):
    for k, columns, knobs, tables, pl in plans:
        where = (k, columns, knobs, tables)
        ls = pl["launches"]
        assert len(ls) == pl["passes"] == (1 if k <= 10 else 2 if k <= 20 else 3), where
        assert pl["tables"] == (tables and 11 <= k <= 24), where
        assert 1 <= pl["columns"] == min(columns, pl["per_launch"]) <= 16, where
        digits = [r["log_np"] for r in ls]
        assert sum(digits) == k and max(digits) <= 10 and digits == sorted(digits, reverse=True) and digits[0] - digits[-1] <= 1, where
        rem = k
        for i, r in enumerate(ls):
            rem -= r["log_np"]
            assert (r["pass"], r["passes"], r["log_m"]) == (i, len(ls), rem), where
            assert r["kind"] == ("last" if i == len(ls) - 1 else "strided"), where
            assert r["blocks"] << (r["log_np"] + r["log_t"]) == 1 << k, where
            if r["kind"] == "strided":
                assert r["log_np"] >= 3 and r["log_t"] <= r["log_m"], where
                assert (r["grid_x"], r["grid_y"]) == (r["blocks"] * pl["columns"], 1), where
            else:
                assert r["log_t"] <= (ls[0]["log_np"] if len(ls) > 1 else 0), where
                assert (r["grid_x"], r["grid_y"]) == (r["blocks"], pl["columns"]), where
                assert r["log_grp"] == 0, where


def test_a_coset_pass_of_its_own_goes_column_by_column(zk):
    for k in (5, 12, 21):
        pl = zk.binding.host_ntt_plan(k, 17, True, True)
        assert (pl["per_launch"], pl["columns"]) == (1, 1)
        assert all(r["grid_y"] == 1 and r["grid_x"] == r["blocks"] for r in pl["launches"])
    for bad in ((0, 1), (29, 1), (12, 0)):
        with pytest.raises(zk.ZkError):
            zk.binding.host_ntt_plan(*bad)


def test_resources(plans):
    top = 0
    for k, columns, knobs, tables, pl in plans:
        for r in pl["launches"]:
            where = (k, columns, knobs, tables, r)
            tile = 1 << (r["log_np"] + r["log_t"])
            assert tile <= 4096 and 64 <= r["threads"] <= 1024 and r["threads"] % 64 == 0, where
            if r["kind"] == "strided":
                assert r["lds"] == tile * 36 <= NTT_PASS_MAX_LDS, where
            else:
                pad = 8 if r["log_np"] >= 8 else 0      # ntt_row_pad
                assert r["lds"] == ((1 << r["log_np"]) + pad << r["log_t"]) * 36 <= NTT_LAST_MAX_LDS, where
                top = max(top, r["lds"])
            if r["fixed"]:
                assert r["threads"] == max(64, tile // 4), where
    assert top == NTT_LAST_MAX_LDS      # the attribute the last-pass kernels are given is reached, and not exceeded


def pass_tile(bx, ncols, xcd, log_grp):
    """csrc/ntt.hip pass_tile: blockIdx.x -> (tile of the column, column)"""
    if not xcd:
        return bx // ncols, bx % ncols
    slot = bx >> 3
    sub, s2 = slot & ((1 << log_grp) - 1), slot >> log_grp
    return ((((s2 // ncols) << 3) + (bx & 7)) << log_grp) + sub, s2 % ncols


def last_tile(bx, grid_x, xcd):
    """csrc/ntt.hip last_tile: blockIdx.x -> tile (the column is blockIdx.y)"""
    return (bx & 7) * (grid_x >> 3) + (bx >> 3) if xcd else bx


def test_workgroup_numberings_are_one_to_one(plans):
    """Every (tile, column) of a launch is worked on by exactly one workgroup, and every tile lies inside its column.  All workgroups
    of every plan up to 2^20; above, the plans with a renumbering (xcd or log_grp set) at three columns, the rest being the identity."""
    done = set()
    for k, columns, knobs, tables, pl in plans:
        ncols = pl["columns"]
        for r in pl["launches"]:
            if k > 20 and not ((r["xcd"] or r["log_grp"]) and columns == 3):
                continue
            geometry = (k, ncols, r["kind"], r["log_np"], r["log_m"], r["log_t"], r["blocks"], r["grid_x"], r["xcd"], r["log_grp"])
            if geometry in done:
                continue
            done.add(geometry)
            bx = np.arange(r["grid_x"], dtype=np.int64)
            if r["kind"] == "strided":
                tile, col = pass_tile(bx, ncols, r["xcd"], r["log_grp"])
                assert col.min() >= 0 and col.max() < ncols and tile.min() >= 0 and tile.max() < r["blocks"], geometry
                assert np.unique(tile * ncols + col).size == r["blocks"] * ncols == r["grid_x"], geometry
                # the elements of a tile: base + d * m + c, d < 2^log_np, c < T
                per_hi = (1 << r["log_m"]) >> r["log_t"]
                assert per_hi >= 1, geometry
                base = ((tile // per_hi) << (r["log_np"] + r["log_m"])) + ((tile % per_hi) << r["log_t"])
                assert (base + (((1 << r["log_np"]) - 1) << r["log_m"]) + (1 << r["log_t"]) - 1).max() < 1 << k, geometry
            else:
                tile = last_tile(bx, r["grid_x"], r["xcd"])
                assert tile.min() >= 0 and tile.max() < r["blocks"] and np.unique(tile).size == r["blocks"] == r["grid_x"], geometry
    assert any(g[2] == "strided" and g[9] == 2 for g in done) and any(g[2] == "strided" and g[9] == 1 and g[1] > 1 for g in done)
    assert any(g[2] == "last" and g[8] for g in done) and any(g[0] > 20 and g[8] for g in done)


def test_what_the_plan_conditions_imply(plans):
    for k, columns, knobs, tables, pl in plans:
        for r in pl["launches"]:
            where = (k, columns, knobs, tables, r)
            if r["fixed"]:
                assert knobs.get("ZK_NTT_FIXED") != "0" and pl["tables"] and 7 <= r["log_np"] <= 10, where
            if r["kind"] == "strided":
                if r["xcd"]:
                    assert r["blocks"] % (8 << r["log_grp"]) == 0 and knobs.get("ZK_NTT_XCD_COLS") != "0", where
                    assert pl["columns"] > 1 or r["log_grp"] > 0, where
                if r["log_grp"] > 0:
                    assert r["fixed"] and r["xcd"] and r["log_t"] < 2 and r["log_grp"] == 2 - r["log_t"], where
            else:
                if r["fixed"]:
                    assert r["passes"] > 1 and r["log_np"] >= 7, where
                if r["xcd"]:
                    assert knobs.get("ZK_NTT_XCD") == "1" and r["passes"] < 3 and r["blocks"] % 8 == 0 and r["blocks"] >= 16, where


def test_gpu_cases_reach_every_launch_signature(zk):
    """GPU_CASES is frozen data: its plans must still be the frozen ones (a GPU case that silently takes another kernel tests nothing),
    and must reach every signature any point of the knob space reaches for k <= 22 at 1 or 3 columns."""
    covered = set()
    for (k, columns, knobs, tables), launches in zip(nc.GPU_CASES, nc.GPU_CASE_LAUNCHES):
        pl = nc.plan(zk, k, columns, knobs, tables)
        assert nc.launch_key(pl) == launches, (k, columns, knobs, tables)
        covered |= nc.signatures(pl)
    reachable = nc.reachable_signatures(zk)
    missing = {s: at for s, at in reachable.items() if s not in covered}
    assert not missing, f"signatures no GPU case reaches (signature: a point that does): {missing}"
    assert len(reachable) > 100      # 163 when the list was made
    assert {knobs.get("ZK_NTT_BATCH") for _, _, knobs, _ in nc.GPU_CASES} >= {"1", "3", "16"}
    assert all(k <= 14 for k, columns, _, _ in nc.GPU_CASES if columns >= 16) and any(columns == 17 for _, columns, _, _ in nc.GPU_CASES)


def test_the_greedy_cover_is_a_cover(zk):
    """the function that made the list, kept callable: what it returns today reaches everything too"""
    cases = nc.greedy_cover(zk)
    covered = set().union(*(nc.signatures(nc.plan(zk, *c[:4])) for c in cases))
    assert covered == set(nc.reachable_signatures(zk)) and len(cases) <= 60

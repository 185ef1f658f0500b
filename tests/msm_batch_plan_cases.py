"""The grid of MSM batch shapes and ZK_MSM_* settings that test_msm_batch_plan.py sweeps, and its text form: one line per case for
tools/msm_batch_plan_check (which reads the lines and prints one record per case), `--records` prints the same records through
zk_host_msm_batch_plan.  A case is (env, k, n, count, hints, blinded_tail, window_table, group_cap, prof_on, graph_broken)."""
import itertools
import os
import sys
from contextlib import contextmanager

KS = range(8, 25)
COUNTS = (1, 2, 3, 4, 5, 9, 33)
TAILS = (0, 6, 256, 257)
CAPS = (0, 8, 4, 2, 1)
# each knob alone at the values test_gpu_msm_paths.py uses, then the pairs (and the sort triple) it uses
KNOB_SETTINGS = ([{}] + [{"ZK_MSM_C": str(c)} for c in range(8, 23)] + [{"ZK_MSM_TOP_SHIFT": v} for v in "01"] + [{"ZK_MSM_BINSORT": v} for v in "01"]
                 + [{"ZK_MSM_STAGED": v} for v in "01"] + [{"ZK_MSM_CHUNK": v} for v in ("256", "1000", "2048", "65536")] + [{"ZK_MSM_PIPES": v} for v in "12"]
                 + [{"ZK_MSM_GRAPH": v} for v in "01"] + [{"ZK_MSM_NARROW": v} for v in "01"] + [{"ZK_MSM_NARROW_GM": "0"}] + [{"ZK_MSM_GM_SETS": v} for v in "14"]
                 + [{"ZK_MSM_NARROW_GROUP": v} for v in ("1", "5", "16")]
                 + [{"ZK_MSM_C": "9", "ZK_MSM_TOP_SHIFT": "0"}, {"ZK_MSM_NARROW_GROUP": "16", "ZK_MSM_GM_SETS": "4"}]
                 + [{"ZK_MSM_PIPES": p, "ZK_MSM_GRAPH": g} for p in "12" for g in "01"]
                 + [{"ZK_MSM_NARROW_GROUP": "1", "ZK_MSM_PIPES": p, "ZK_MSM_GRAPH": g} for p in "12" for g in "01"]
                 + [{"ZK_MSM_C": c, "ZK_MSM_BINSORT": b, "ZK_MSM_STAGED": s, "ZK_MSM_CHUNK": ch} for c in ("12", "19", "22") for b in "01" for s in "01" for ch in ("256", "65536")])


def hint_patterns(count):
    """all 0, all 1, alternating, a run of 17 ones between zeros (as much of it as the batch holds), a mix with 2s"""
    run = ([0] * 8 + [1] * 17 + [0] * 8)[:count] if count > 9 else [0] + [1] * (count - 2) + [0] * (count > 1)
    pats = [[0] * count, [1] * count, [i & 1 for i in range(count)], run, [(0, 1, 2, 1, 1, 2, 0)[i % 7] for i in range(count)]]
    out = []
    for p in pats:
        if p not in out:
            out.append(p)
    return out


def sizes(k):
    return sorted({n for n in (1 << k, (1 << k) - 37, 1024, 64) if 0 < n <= 1 << k})


def grid():
    """Thinned by rotation, not by class: every (tail, table, cap) and every context-flag pair meets every k, size class, count and hint
    pattern many times, but not every combination of all of them."""
    combos = list(itertools.product(TAILS, (1, 0), CAPS))
    flags = [(0, 0), (0, 0), (0, 0), (1, 0), (0, 1)]
    turn = 0
    cases = []
    for k in KS:
        for n in sizes(k):
            for count in COUNTS:
                for hints in hint_patterns(count):
                    for _ in range(3):
                        tail, table, cap = combos[turn % len(combos)]
                        cases.append(({}, k, n, count, hints, tail, table, cap) + flags[turn % len(flags)])
                        turn += 7
    for env in KNOB_SETTINGS[1:]:
        for k in (8, 12, 16, 19, 20, 24):
            for n in ((1 << k), (1 << k) - 37):
                for count in (1, 4, 9, 33):
                    for hints in hint_patterns(count):
                        tail, table, cap = combos[turn % len(combos)]
                        cases.append((env, k, n, count, hints, tail, table, cap) + flags[turn % len(flags)])
                        turn += 7
    # the 32-bit limits
    for k in (27, 28):
        for hints in ([0] * 4, [1] * 4, [0, 1, 2, 1]):
            for tail in (0, 6):
                cases.append(({}, k, 1 << k, 4, hints, tail, 1, 0, 0, 0))
    return cases


def case_line(case):
    env, k, n, count, hints, tail, table, cap, prof, broken = case
    return " ".join(str(v) for v in (k, n, count, "".join(map(str, hints)), tail, table, cap, prof, broken, ",".join(f"{a}={b}" for a, b in sorted(env.items())) or "-"))


@contextmanager
def msm_env(env):
    """exactly `env` of the ZK_MSM_* variables (the trace, which is no knob, apart)"""
    saved = {v: os.environ.pop(v) for v in list(os.environ) if v.startswith("ZK_MSM_") and v != "ZK_MSM_TRACE"}
    os.environ.update(env)
    try:
        yield
    finally:
        for v in env:
            os.environ.pop(v, None)
        os.environ.update(saved)


def record(binding, case):
    env, k, n, count, hints, tail, table, cap, prof, broken = case
    with msm_env(env):
        return binding.host_msm_batch_plan_words(k, n, count, hints, tail, bool(table), cap, bool(prof), bool(broken))


if __name__ == "__main__":
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
    if sys.argv[1:] == ["--cases"]:
        for c in grid():
            print(case_line(c))
    elif sys.argv[1:] == ["--records"]:
        from zkevm_circuits_amd import binding
        for c in grid():
            print(" ".join(map(str, record(binding, c))))
    else:
        sys.exit("usage: msm_batch_plan_cases.py --cases | --records")

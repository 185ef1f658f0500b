"""What the NTT plan tests (test_ntt_plan.py, CPU) and the NTT path tests (test_gpu_ntt_paths.py, GPU) share: the knob space of
csrc/ntt.hip's launch plans, zk_host_ntt_plan under a set of knobs, the signatures of a launch, and GPU_CASES -- a frozen list of
(k, columns, knobs, tables) whose launches reach every signature that any point of the knob space reaches for k <= 22."""
import contextlib
import itertools
import os

KNOB_NAMES = ("ZK_NTT_PASS_LOGTILE", "ZK_NTT_LAST_LOGTILE", "ZK_NTT_XCD", "ZK_NTT_XCD_COLS", "ZK_NTT_FIXED", "ZK_NTT_BATCH", "ZK_NTT_OUT_TABLE")
KNOB_SPACE = {
    "ZK_NTT_PASS_LOGTILE": (None, "10", "11", "12"),
    "ZK_NTT_LAST_LOGTILE": (None, "10", "11", "12"),
    "ZK_NTT_XCD": (None, "1"),
    "ZK_NTT_XCD_COLS": (None, "0"),
    "ZK_NTT_FIXED": (None, "0"),
}


def knob_dicts():
    """every point of KNOB_SPACE as a dict of the knobs that are set"""
    names = list(KNOB_SPACE)
    for values in itertools.product(*(KNOB_SPACE[n] for n in names)):
        yield {n: v for n, v in zip(names, values) if v is not None}


@contextlib.contextmanager
def knobs_set(knobs, tables=True):
    """the NTT knobs of os.environ are exactly `knobs` (plus ZK_NTT_OUT_TABLE=0 when `tables` is false) inside, and as before after:
    the library reads them at every call"""
    env = dict(knobs)
    if not tables:
        env["ZK_NTT_OUT_TABLE"] = "0"
    saved = {n: os.environ.pop(n, None) for n in KNOB_NAMES}
    os.environ.update(env)
    try:
        yield
    finally:
        for n in KNOB_NAMES:
            os.environ.pop(n, None)
            if saved[n] is not None:
                os.environ[n] = saved[n]


def plan(zk, k, columns, knobs, tables, coset_pass=False):
    with knobs_set(knobs, tables):
        return zk.binding.host_ntt_plan(k, columns, tables, coset_pass)


def signatures(pl):
    """the three signatures of every launch of a plan, tagged 'A' / 'B' / 'C'"""
    out = set()
    for r in pl["launches"]:
        out.add(("A", r["kind"], r["passes"], r["log_np"], r["log_t"], r["fixed"]))
        out.add(("B", r["kind"], r["passes"], r["fixed"], r["xcd"], r["log_grp"], pl["columns"] > 1))
        out.add(("C", r["kind"], r["passes"], r["log_np"], r["fixed"], pl["tables"]))
    return out


def launch_key(pl):
    """what GPU_CASES freezes of a plan: per launch (kind, log_np, log_t, fixed, xcd, log_grp)"""
    return tuple((r["kind"][0], r["log_np"], r["log_t"], int(r["fixed"]), int(r["xcd"]), r["log_grp"]) for r in pl["launches"])


COVER_MAX_K, COVER_COLUMNS = 22, (1, 3)


def cover_space():
    for k in range(1, COVER_MAX_K + 1):
        for columns in COVER_COLUMNS:
            for tables in (True, False):
                for knobs in knob_dicts():
                    yield k, columns, knobs, tables


def reachable_signatures(zk):
    """signature -> the first point of the knob space (k <= 22, 1 or 3 columns) that reaches it"""
    seen = {}
    for k, columns, knobs, tables in cover_space():
        for s in signatures(plan(zk, k, columns, knobs, tables)):
            seen.setdefault(s, (k, columns, knobs, tables))
    return seen


def greedy_cover(zk):
    """The few lines that made GPU_CASES: repeatedly the point that reaches the most signatures not reached yet -- the smallest k,
    then the fewest knobs, among equals.  Returns [(k, columns, knobs, tables, launch_key)]."""
    points = [(c, signatures(plan(zk, *c))) for c in cover_space()]
    todo = set().union(*(s for _, s in points))
    cases = []
    while todo:
        (k, columns, knobs, tables), sigs = max(points, key=lambda p: (len(p[1] & todo), -p[0][0], -len(p[0][2]), p[0][3], -p[0][1]))
        cases.append((k, columns, knobs, tables, launch_key(plan(zk, k, columns, knobs, tables))))
        todo -= sigs
    return sorted(cases, key=lambda c: (c[0], c[1], sorted(c[2].items()), c[3]))


# Beyond the cover: the group boundary of a launch (NTT_BATCH = 16 columns, and ZK_NTT_BATCH = 1, 3, 16) at small sizes.
BATCH_CASES = [
    (5, 17, {}, True),
    (9, 16, {"ZK_NTT_BATCH": "3"}, True),
    (11, 3, {"ZK_NTT_BATCH": "1"}, True),
    (12, 17, {"ZK_NTT_BATCH": "16", "ZK_NTT_PASS_LOGTILE": "10"}, True),
    (14, 17, {}, True),
    (14, 16, {"ZK_NTT_BATCH": "3"}, False),
]

# greedy_cover() on the plans of the commit that added this file, then BATCH_CASES with their plans
FROZEN_CASES = [
    (1, 1, {}, True, (('l', 1, 0, 0, 0, 0),)),
    (2, 3, {}, True, (('l', 2, 0, 0, 0, 0),)),
    (3, 1, {}, True, (('l', 3, 0, 0, 0, 0),)),
    (4, 1, {}, True, (('l', 4, 0, 0, 0, 0),)),
    (5, 1, {}, True, (('l', 5, 0, 0, 0, 0),)),
    (6, 1, {}, True, (('l', 6, 0, 0, 0, 0),)),
    (7, 1, {}, True, (('l', 7, 0, 0, 0, 0),)),
    (8, 1, {}, True, (('l', 8, 0, 0, 0, 0),)),
    (9, 1, {}, True, (('l', 9, 0, 0, 0, 0),)),
    (10, 1, {}, True, (('l', 10, 0, 0, 0, 0),)),
    (11, 1, {}, True, (('s', 6, 5, 0, 0, 0), ('l', 5, 6, 0, 0, 0))),
    (11, 3, {'ZK_NTT_PASS_LOGTILE': '10', 'ZK_NTT_LAST_LOGTILE': '10'}, False, (('s', 6, 4, 0, 0, 0), ('l', 5, 5, 0, 0, 0))),
    (12, 1, {'ZK_NTT_LAST_LOGTILE': '10'}, False, (('s', 6, 6, 0, 0, 0), ('l', 6, 4, 0, 0, 0))),
    (13, 1, {'ZK_NTT_FIXED': '0'}, True, (('s', 7, 5, 0, 0, 0), ('l', 6, 5, 0, 0, 0))),
    (13, 1, {'ZK_NTT_PASS_LOGTILE': '10', 'ZK_NTT_LAST_LOGTILE': '12'}, True, (('s', 7, 3, 1, 0, 0), ('l', 6, 6, 0, 0, 0))),
    (14, 1, {}, True, (('s', 7, 5, 1, 0, 0), ('l', 7, 4, 1, 0, 0))),
    (14, 1, {'ZK_NTT_PASS_LOGTILE': '11', 'ZK_NTT_LAST_LOGTILE': '10'}, True, (('s', 7, 4, 1, 0, 0), ('l', 7, 3, 1, 0, 0))),
    (14, 1, {'ZK_NTT_PASS_LOGTILE': '11', 'ZK_NTT_LAST_LOGTILE': '12'}, False, (('s', 7, 4, 0, 0, 0), ('l', 7, 5, 0, 0, 0))),
    (14, 3, {'ZK_NTT_PASS_LOGTILE': '10', 'ZK_NTT_LAST_LOGTILE': '10', 'ZK_NTT_XCD': '1'}, False, (('s', 7, 3, 0, 1, 0), ('l', 7, 3, 0, 1, 0))),
    (15, 1, {'ZK_NTT_XCD': '1', 'ZK_NTT_FIXED': '0'}, True, (('s', 8, 4, 0, 0, 0), ('l', 7, 4, 0, 1, 0))),
    (15, 1, {'ZK_NTT_PASS_LOGTILE': '10', 'ZK_NTT_LAST_LOGTILE': '12'}, True, (('s', 8, 2, 1, 0, 0), ('l', 7, 5, 1, 0, 0))),
    (16, 1, {'ZK_NTT_PASS_LOGTILE': '11', 'ZK_NTT_LAST_LOGTILE': '10'}, True, (('s', 8, 3, 1, 0, 0), ('l', 8, 2, 1, 0, 0))),
    (16, 1, {'ZK_NTT_PASS_LOGTILE': '11', 'ZK_NTT_LAST_LOGTILE': '12'}, False, (('s', 8, 3, 0, 0, 0), ('l', 8, 4, 0, 0, 0))),
    (16, 1, {'ZK_NTT_PASS_LOGTILE': '10'}, False, (('s', 8, 2, 0, 0, 0), ('l', 8, 3, 0, 0, 0))),
    (16, 3, {}, True, (('s', 8, 4, 1, 1, 0), ('l', 8, 3, 1, 0, 0))),
    (17, 1, {'ZK_NTT_LAST_LOGTILE': '10', 'ZK_NTT_FIXED': '0'}, True, (('s', 9, 3, 0, 0, 0), ('l', 8, 2, 0, 0, 0))),
    (17, 1, {'ZK_NTT_LAST_LOGTILE': '12'}, True, (('s', 9, 3, 1, 0, 0), ('l', 8, 4, 1, 0, 0))),
    (17, 1, {'ZK_NTT_PASS_LOGTILE': '11'}, True, (('s', 9, 2, 1, 0, 0), ('l', 8, 3, 1, 0, 0))),
    (18, 1, {'ZK_NTT_PASS_LOGTILE': '11', 'ZK_NTT_LAST_LOGTILE': '12'}, False, (('s', 9, 2, 0, 0, 0), ('l', 9, 3, 0, 0, 0))),
    (18, 1, {'ZK_NTT_PASS_LOGTILE': '10'}, False, (('s', 9, 1, 0, 0, 0), ('l', 9, 2, 0, 0, 0))),
    (18, 1, {'ZK_NTT_PASS_LOGTILE': '10', 'ZK_NTT_XCD': '1'}, True, (('s', 9, 1, 1, 1, 1), ('l', 9, 2, 1, 1, 0))),
    (19, 1, {'ZK_NTT_LAST_LOGTILE': '10', 'ZK_NTT_FIXED': '0'}, True, (('s', 10, 2, 0, 0, 0), ('l', 9, 1, 0, 0, 0))),
    (19, 1, {'ZK_NTT_PASS_LOGTILE': '10', 'ZK_NTT_LAST_LOGTILE': '10'}, True, (('s', 10, 0, 1, 1, 2), ('l', 9, 1, 1, 0, 0))),
    (19, 3, {'ZK_NTT_PASS_LOGTILE': '11', 'ZK_NTT_LAST_LOGTILE': '12'}, True, (('s', 10, 1, 1, 1, 1), ('l', 9, 3, 1, 0, 0))),
    (20, 1, {'ZK_NTT_PASS_LOGTILE': '11', 'ZK_NTT_LAST_LOGTILE': '10', 'ZK_NTT_FIXED': '0'}, True, (('s', 10, 1, 0, 0, 0), ('l', 10, 0, 0, 0, 0))),
    (20, 1, {'ZK_NTT_LAST_LOGTILE': '12'}, False, (('s', 10, 2, 0, 0, 0), ('l', 10, 2, 0, 0, 0))),
    (20, 1, {'ZK_NTT_LAST_LOGTILE': '12'}, True, (('s', 10, 2, 1, 0, 0), ('l', 10, 2, 1, 0, 0))),
    (20, 1, {'ZK_NTT_PASS_LOGTILE': '10'}, False, (('s', 10, 0, 0, 0, 0), ('l', 10, 1, 0, 0, 0))),
    (20, 3, {'ZK_NTT_PASS_LOGTILE': '10', 'ZK_NTT_LAST_LOGTILE': '10'}, True, (('s', 10, 0, 1, 1, 2), ('l', 10, 0, 1, 0, 0))),
    (20, 3, {'ZK_NTT_XCD': '1', 'ZK_NTT_XCD_COLS': '0'}, True, (('s', 10, 2, 1, 0, 0), ('l', 10, 1, 1, 1, 0))),
    (22, 1, {}, False, (('s', 8, 3, 0, 0, 0), ('s', 7, 4, 0, 0, 0), ('l', 7, 4, 0, 0, 0))),
    (22, 1, {}, True, (('s', 8, 3, 1, 0, 0), ('s', 7, 4, 1, 0, 0), ('l', 7, 4, 1, 0, 0))),
    (22, 3, {'ZK_NTT_PASS_LOGTILE': '10', 'ZK_NTT_LAST_LOGTILE': '10', 'ZK_NTT_FIXED': '0'}, True, (('s', 8, 2, 0, 1, 0), ('s', 7, 3, 0, 1, 0), ('l', 7, 3, 0, 0, 0))),
    (22, 3, {'ZK_NTT_PASS_LOGTILE': '10', 'ZK_NTT_LAST_LOGTILE': '10'}, True, (('s', 8, 2, 1, 1, 0), ('s', 7, 3, 1, 1, 0), ('l', 7, 3, 1, 0, 0))),
    (22, 3, {'ZK_NTT_PASS_LOGTILE': '12', 'ZK_NTT_LAST_LOGTILE': '12', 'ZK_NTT_XCD_COLS': '0'}, False, (('s', 8, 4, 0, 0, 0), ('s', 7, 5, 0, 0, 0), ('l', 7, 5, 0, 0, 0))),
    (22, 3, {'ZK_NTT_PASS_LOGTILE': '12', 'ZK_NTT_LAST_LOGTILE': '12', 'ZK_NTT_XCD_COLS': '0'}, True, (('s', 8, 4, 1, 0, 0), ('s', 7, 5, 1, 0, 0), ('l', 7, 5, 1, 0, 0))),
    (5, 17, {}, True, (('l', 5, 0, 0, 0, 0),)),
    (9, 16, {'ZK_NTT_BATCH': '3'}, True, (('l', 9, 0, 0, 0, 0),)),
    (11, 3, {'ZK_NTT_BATCH': '1'}, True, (('s', 6, 5, 0, 0, 0), ('l', 5, 6, 0, 0, 0))),
    (12, 17, {'ZK_NTT_BATCH': '16', 'ZK_NTT_PASS_LOGTILE': '10'}, True, (('s', 6, 4, 0, 0, 0), ('l', 6, 5, 0, 0, 0))),
    (14, 17, {}, True, (('s', 7, 5, 1, 0, 0), ('l', 7, 4, 1, 0, 0))),
    (14, 16, {'ZK_NTT_BATCH': '3'}, False, (('s', 7, 5, 0, 0, 0), ('l', 7, 4, 0, 0, 0))),
]

GPU_CASES = [c[:4] for c in FROZEN_CASES]
GPU_CASE_LAUNCHES = [c[4] for c in FROZEN_CASES]

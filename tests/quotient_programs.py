"""Programs, column data and the big-int reference for the quotient evaluator's tests (csrc/quotient.hip) -- what msm_scalars.py is to
the MSM.

Programs.  The random postfix programs of test_quotient_lowering (random_program) and test_quotient_mac (random_horner_program, the
shapes that lower to K_MAC_COL), plus the shapes neither emits:
  * nested folds: a FOLD executed while values wait below it on the stack (PUSH a; PUSH b; FOLD c1; ...; FOLD c2);
  * parking edges: a PUSH_TMP right behind its TEE_TMP (the prefetch hazard the lowering pads with K_NOP), slots reused, and a program
    with a few hundred distinct slots;
  * deep programs: caller depth exactly 16 (the evaluator's Q_MAX_STACK), built so that the lowering cannot take operands from memory;
  * rotations at the edges of the domain and of the 32-bit word: 0, +-1, +-2, +-(n-1), +-n, +-(n+1), 0x7fffffff, 0x80000000;
  * sliceable sums: top-level fold sums long enough to cut under ZK_QUOTIENT_SLICES, with nested folds inside the terms.

Data.  Column values are the words stored in memory (R-form, canonical, below p) -- built from the integers themselves, not through a
conversion into Montgomery form, so that p - 1, 0, R mod p, p - 2 are what the kernel reads.  A column is laid out in segments of at
least 64 rows of one kind each, so rows near a segment boundary and rotated reads mix kinds.

Reference.  The original program over the integers mod p (test_quotient_lowering.run_plain), lifted to rows: row i reads column c at
(i + rot 2^(ext_k - k)) mod 2^ext_k, and the accumulator is multiplied by 1 / ((zeta w_ext^j)^n - 1), j = i mod 2^(ext_k - k), when
dividing.  One numpy object array per stack entry: 2^10 rows of a few hundred instructions take well under a second.
"""
import ctypes

import numpy as np

import test_quotient_lowering as tl
import test_quotient_mac as tm
from oracle import bn254
from test_quotient_lowering import (P, R, Q_ADD, Q_ADD_CONST, Q_DOUBLE, Q_FOLD, Q_MUL, Q_MUL_CONST, Q_NEG, Q_PUSH_COL, Q_PUSH_CONST,
                                    Q_PUSH_TMP, Q_SQUARE, Q_SUB, Q_TEE_TMP)

MAX_STACK = 16
M32 = 1 << 32
ONE = R % P
K_ADD_COL, K_SUB_COL, K_RSUB_COL, K_MUL_COL, K_FOLD_COL, K_NOP, K_MAC_COL = 16, 17, 18, 19, 20, 21, 22
K_SETTLE = 0x100 | 0x200
K_NORM = 0x400 | 0x800
K_SETTLE8 = 0x1000 | 0x2000
SEGMENT_KINDS = ("max", "zero", "one", "pm2", "random")


# ---- programs ------------------------------------------------------------------------------------------------------------------
def edge_rotations(k):
    """rotation words at the edges of a 2^k domain and of the 32-bit word"""
    n = 1 << k
    return sorted({r % M32 for r in (0, 1, -1, 2, -2, n - 1, -(n - 1), n, -n, n + 1, -(n + 1))} | {0x7fffffff, 0x80000000})


def with_rotations(rng, prog, k, share=0.35):
    """the program with a share of its column reads moved to edge rotations"""
    rots = edge_rotations(k)
    return [(op, a, rng.choice(rots)) if op == Q_PUSH_COL and rng.random() < share else (op, a, b) for op, a, b in prog]


def nested_fold_program(rng, ncols, nconsts, statements, depth):
    """statements of random_program, some of them folded while 1..3 values wait below them; those are folded later (sometimes combined
    first).  Starts with a nested fold; ends with the stack empty."""
    prog, defined, nxt = [], set(), [0]
    tl.random_expr(rng, ncols, nconsts, depth, defined, nxt, prog)
    pending = 1
    for _ in range(statements):
        if pending < 3 and rng.random() < 0.3:
            tl.random_expr(rng, ncols, nconsts, depth, defined, nxt, prog)
            pending += 1
            continue
        tl.random_expr(rng, ncols, nconsts, depth, defined, nxt, prog)
        prog.append((Q_FOLD, rng.randrange(nconsts), 0))
        if pending and rng.random() < 0.4:
            if pending >= 2 and rng.random() < 0.4:
                prog.append((rng.choice([Q_ADD, Q_SUB, Q_MUL]), 0, 0))
                pending -= 1
            prog.append((Q_FOLD, rng.randrange(nconsts), 0))
            pending -= 1
    prog += [(Q_FOLD, rng.randrange(nconsts), 0)] * pending
    return prog


def horner_program(rng, ncols, nconsts, items, depth, nested=False):
    """test_quotient_mac.random_horner_program (the sums that lower to K_MAC_COL); nested: run with a value waiting below, folded last"""
    prog = tm.random_horner_program(rng, ncols, nconsts, items, depth)
    if not nested:
        return prog
    return [(Q_PUSH_COL, rng.randrange(ncols), 0), (Q_SQUARE, 0, 0)] + prog + [(Q_FOLD, rng.randrange(nconsts), 0)]


def parking_program(rng, ncols, nconsts, slots):
    """`slots` distinct parking slots, each read back right behind its TEE_TMP in one of four ways (MUL_COL, SUB_COL, ADD_COL after a
    product, a nested FOLD_COL), then a sample of them read again much later, then slot 0 parked anew (reuse)"""
    col = lambda: (Q_PUSH_COL, rng.randrange(ncols), rng.choice([0, 1, M32 - 1]))
    cst = lambda: rng.randrange(nconsts)
    prog = []
    for s in range(slots):
        x = [col(), col(), (rng.choice([Q_ADD, Q_SUB]), 0, 0)]
        kind = s % 4
        if kind == 0:
            prog += x + [(Q_TEE_TMP, s, 0), (Q_PUSH_TMP, s, 0), (Q_MUL, 0, 0), (Q_FOLD, cst(), 0)]
        elif kind == 1:
            prog += x + [(Q_MUL_CONST, cst(), 0), (Q_TEE_TMP, s, 0), (Q_PUSH_TMP, s, 0), (Q_SUB, 0, 0), (Q_FOLD, cst(), 0)]
        elif kind == 2:
            prog += x + [(Q_TEE_TMP, s, 0), (Q_PUSH_TMP, s, 0), (Q_ADD, 0, 0), (Q_DOUBLE, 0, 0), (Q_FOLD, cst(), 0)]
        else:
            prog += x + [(Q_TEE_TMP, s, 0), (Q_PUSH_TMP, s, 0), (Q_FOLD, cst(), 0), (Q_FOLD, cst(), 0)]
    for s in rng.sample(range(slots), min(slots, 12)):
        prog += [(Q_PUSH_TMP, s, 0), col(), (Q_MUL, 0, 0), (Q_FOLD, cst(), 0)]
    prog += [col(), col(), (Q_MUL, 0, 0), (Q_TEE_TMP, 0, 0), (Q_PUSH_TMP, 0, 0), (Q_SUB, 0, 0), (Q_PUSH_TMP, 0, 0), (Q_ADD, 0, 0), (Q_FOLD, cst(), 0)]
    return prog


def deep_program(rng, ncols, nconsts, depth=MAX_STACK):
    """caller stack depth exactly `depth`: `depth` one-push sub-expressions (a column through a unary or constant operation, which the
    lowering cannot read from memory) combined right-nested,  e1 (e2 (... (e15 e16 op) ...) op) op,  then one FOLD"""
    prog = []
    for _ in range(depth):
        prog.append((Q_PUSH_COL, rng.randrange(ncols), rng.choice([0, 1, M32 - 1])))
        u = rng.choice([Q_SQUARE, Q_NEG, Q_DOUBLE, Q_MUL_CONST, Q_ADD_CONST])
        prog.append((u, rng.randrange(nconsts) if u in (Q_MUL_CONST, Q_ADD_CONST) else 0, 0))
    prog += [(rng.choice([Q_MUL, Q_MUL, Q_ADD, Q_SUB]), 0, 0) for _ in range(depth - 1)]
    prog.append((Q_FOLD, rng.randrange(nconsts), 0))
    return prog


def sliceable_program(rng, ncols, nconsts, terms):
    """a top-level fold sum of `terms` terms that zk_quotient_eval can cut (ZK_QUOTIENT_SLICES): each term parks and reads its values
    within itself (slot numbers reused from term to term), a third of them fold a statement while a value waits below (nested folds
    inside a slice), others are Horner sums"""
    prog = []
    nxt = [0]
    for t in range(terms):
        defined = set()                 # a term reads only what it parked itself
        if rng.random() < 0.5:
            nxt = [0]
        r = rng.random()
        if r < 0.35:
            tl.random_expr(rng, ncols, nconsts, 2, defined, nxt, prog)
            tl.random_expr(rng, ncols, nconsts, 3, defined, nxt, prog)
            prog += [(Q_FOLD, rng.randrange(nconsts), 0), (Q_FOLD, rng.randrange(nconsts), 0)]
        elif r < 0.55:
            prog += tm.random_horner_program(rng, ncols, nconsts, rng.randrange(1, 4), 2)      # slots from 0 again, each read behind its own TEE
        else:
            tl.random_expr(rng, ncols, nconsts, 3, defined, nxt, prog)
            prog.append((Q_FOLD, rng.randrange(nconsts), 0))
    return prog


def stack_depth(prog):
    sp = mx = 0
    for op, a, b in prog:
        if op in (Q_PUSH_COL, Q_PUSH_CONST, Q_PUSH_TMP):
            sp += 1
        elif op in (Q_ADD, Q_SUB, Q_MUL, Q_FOLD):
            sp -= 1
        mx = max(mx, sp)
    assert sp == 0
    return mx


def nested_folds(prog):
    """FOLDs that leave values on the stack"""
    sp = cnt = 0
    for op, a, b in prog:
        if op in (Q_PUSH_COL, Q_PUSH_CONST, Q_PUSH_TMP):
            sp += 1
        elif op in (Q_ADD, Q_SUB, Q_MUL):
            sp -= 1
        elif op == Q_FOLD:
            sp -= 1
            cnt += sp > 0
    return cnt


def num_cols_consts(prog):
    ncols = 1 + max([a for op, a, b in prog if op == Q_PUSH_COL], default=0)
    nconsts = 1 + max([a for op, a, b in prog if op in (Q_PUSH_CONST, Q_MUL_CONST, Q_ADD_CONST, Q_FOLD)], default=0)
    return ncols, nconsts


# ---- lowering and slicing (host entry points) ------------------------------------------------------------------------------------
def lower(prog, num_cols, fuse):
    """zk_host_quotient_lower: the lowered words and the lowered stack depth"""
    return tl.lower(prog, num_cols, fuse)


def slice_cuts(prog, ext_k):
    """zk_host_quotient_slices under the ZK_QUOTIENT_SLICES in force: the cut points, [] when the program stays whole"""
    from zkevm_circuits_amd import binding
    words = np.ascontiguousarray(np.array(prog, dtype=np.uint32).reshape(-1))
    out = np.zeros(len(prog) + 2, dtype=np.uint32)
    cnt = ctypes.c_uint32()
    assert binding.lib().zk_host_quotient_slices(words.ctypes.data_as(ctypes.c_void_p), ctypes.c_uint32(len(prog)), ctypes.c_uint32(ext_k),
                                                 out.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(out.size), ctypes.byref(cnt)) == 0
    return [int(x) for x in out[:cnt.value]]


def fuse_of(env):
    """the `fuse` argument of zk_host_quotient_lower that gives the stream zk_quotient_eval runs under the knobs `env`: the caller's sequence
    under ZK_QUOTIENT_FUSE=0; memory operands alone (1) for k_quotient_eval and under ZK_QUOTIENT_MAC=0; K_MAC_COL too (3) under
    ZK_QUOTIENT_MAC=1; every fused step (7) otherwise"""
    if env.get("ZK_QUOTIENT_FUSE") == "0":
        return 0
    if env.get("ZK_QUOTIENT_KERNEL") == "1" or env.get("ZK_QUOTIENT_MAC") == "0":
        return 1
    return 3 if env.get("ZK_QUOTIENT_MAC") == "1" else 7


def variant(prog, ncols, ext_k, env):
    """which kernel zk_quotient_eval launches for this program (packed columns) under the knobs `env` (ZK_QUOTIENT_KERNEL / MAC / FUSE /
    SLICES), restated from the rules of the launch: ("sliced",) or (kernel, FULL, ACC_MEM) with kernel "v2" (k_quotient_eval2) or "v1"
    (k_quotient_eval).  ZK_QUOTIENT_SLICES must be set in os.environ as in `env` (zk_host_quotient_slices reads it).
    tests/test_quotient_launch.py holds this against the library's launch plan on every (case, setting)."""
    v2 = env.get("ZK_QUOTIENT_KERNEL") != "1"
    ne = 1 << ext_k
    if v2 and ((ne // 256) & 7) == 0 and slice_cuts(prog, ext_k):
        return ("sliced",)
    words, _ = lower(prog, ncols, fuse_of(env))
    ops = [int(w) & 0xff for w in words[0::3]]
    folds = sum(1 for o in ops if o in (Q_FOLD, K_FOLD_COL))
    acc_mem = folds > 0 and folds * 16 <= len(ops)
    return ("v2" if v2 else "v1", ne >= 256, acc_mem)


# ---- column data -----------------------------------------------------------------------------------------------------------------
def segment_value(rng, kind):
    return {"max": P - 1, "zero": 0, "one": ONE, "pm2": P - 2}.get(kind) if kind != "random" else rng.randrange(P)


def column(rng, ne):
    """stored words of one column: segments of >= 64 rows (the whole column below 64 rows), one kind each"""
    vals = []
    while len(vals) < ne:
        kind = rng.choice(SEGMENT_KINDS)
        seg = min(ne - len(vals), rng.randrange(64, 257))
        vals += [segment_value(rng, kind) for _ in range(seg)]
    return vals


def constants(rng, nconsts):
    return [rng.choice([P - 1, P - 2, 0, 1, ONE, rng.randrange(P), rng.randrange(P)]) for _ in range(nconsts)]


def to_words(vals):
    """integers below 2^256 -> (len, 4) uint64, little-endian limbs"""
    m = (1 << 64) - 1
    return np.array([[(v >> (64 * j)) & m for j in range(4)] for v in vals], dtype=np.uint64).reshape(-1, 4)


def from_words(a):
    a = np.asarray(a, dtype=np.uint64).reshape(-1, 4)
    return [int(r[0]) | (int(r[1]) << 64) | (int(r[2]) << 128) | (int(r[3]) << 192) for r in a]


# ---- the reference ---------------------------------------------------------------------------------------------------------------
def vanishing_inverses(k, ext_k):
    """1 / ((zeta w_ext^j)^n - 1), j < 2^(ext_k - k) (plain values)"""
    zn, step = pow(bn254.FR_ZETA, 1 << k, P), pow(bn254.omega_for_k(ext_k), 1 << k, P)
    return [pow((zn * pow(step, j, P) - 1) % P, -1, P) for j in range(1 << (ext_k - k))]


def reference(prog, cols, consts, k, ext_k, divide, rows=None):
    """the original program over the integers mod p at the given rows (all by default), on stored words: products divide by R; the
    result is the stored word the kernel must write"""
    ne, scale = 1 << ext_k, 1 << (ext_k - k)
    idx = np.arange(ne, dtype=np.int64) if rows is None else np.asarray(rows, dtype=np.int64)
    cols = [np.array(c, dtype=object) for c in cols]
    rinv = pow(R, -1, P)
    full = lambda v: np.full(len(idx), v, dtype=object)
    st, tmp = [], {}
    acc = full(0)
    for op, a, b in prog:
        if op == Q_PUSH_COL:
            rot = b - M32 if b >= (1 << 31) else b
            st.append(cols[a][(idx + rot * scale) % ne])
        elif op == Q_PUSH_CONST: st.append(full(consts[a]))
        elif op == Q_PUSH_TMP: st.append(tmp[a])
        elif op == Q_TEE_TMP: tmp[a] = st[-1]
        elif op == Q_ADD: y = st.pop(); st[-1] = (st[-1] + y) % P
        elif op == Q_SUB: y = st.pop(); st[-1] = (st[-1] - y) % P
        elif op == Q_MUL: y = st.pop(); st[-1] = (st[-1] * y % P) * rinv % P
        elif op == Q_NEG: st[-1] = (-st[-1]) % P
        elif op == Q_SQUARE: st[-1] = (st[-1] * st[-1] % P) * rinv % P
        elif op == Q_DOUBLE: st[-1] = (2 * st[-1]) % P
        elif op == Q_MUL_CONST: st[-1] = (st[-1] * consts[a] % P) * rinv % P
        elif op == Q_ADD_CONST: st[-1] = (st[-1] + consts[a]) % P
        elif op == Q_FOLD: acc = ((acc * consts[a] % P) * rinv + st.pop()) % P
        else: raise AssertionError(f"opcode {op}")
    assert not st
    if divide:
        acc = acc * np.array(vanishing_inverses(k, ext_k), dtype=object)[idx % scale] % P
    return [int(v) for v in acc]


def sample_rows(ext_k):
    """every row up to 2^10, a fixed sample above: both ends of the domain and every 29th row"""
    ne = 1 << ext_k
    if ext_k <= 10:
        return None
    return sorted(set(range(80)) | set(range(ne - 80, ne)) | set(range(0, ne, 29)))


# ---- the corpus ------------------------------------------------------------------------------------------------------------------
SIZES_EXT_K = (0, 1, 3, 7, 8, 10, 11, 12)


class Case:
    def __init__(self, name, prog, k, ext_k, divide):
        self.name, self.prog, self.k, self.ext_k, self.divide = name, prog, k, ext_k, divide
        self.ncols, self.nconsts = num_cols_consts(prog)

    def __repr__(self):
        return f"{self.name}(k={self.k}, ext_k={self.ext_k}, divide={self.divide}, {len(self.prog)} instructions)"


def corpus(seed=20261016):
    """the programs of the device tests, with their sizes: every ext_k of SIZES_EXT_K with ext_k - k = 0 .. 3, two programs each (one
    that folds on most statements: accumulator in registers; one with long terms: accumulator in memory), dividing by the vanishing
    polynomial in one of the two; edge rotations throughout; two programs with 300 parking slots"""
    import random
    rng = random.Random(seed)
    reg = [lambda nc, nk: nested_fold_program(rng, nc, nk, rng.randrange(2, 7), rng.randrange(1, 4)),
           lambda nc, nk: tl.random_program(rng, nc, nk, statements=rng.randrange(2, 7), depth=rng.randrange(1, 3)),
           lambda nc, nk: parking_program(rng, nc, nk, rng.randrange(4, 17)),
           lambda nc, nk: nested_fold_program(rng, nc, nk, rng.randrange(3, 8), 2)]
    mem = [lambda nc, nk: deep_program(rng, nc, nk, rng.randrange(6, MAX_STACK + 1)),
           lambda nc, nk: horner_program(rng, nc, nk, rng.randrange(4, 7), rng.randrange(1, 4), nested=rng.random() < 0.5),
           lambda nc, nk: horner_program(rng, nc, nk, rng.randrange(4, 7), 2, nested=True)]
    cases = []
    i = 0
    for ext_k in SIZES_EXT_K:
        for e in range(min(3, ext_k) + 1):
            k = ext_k - e
            for fam, name in ((reg, "reg"), (mem, "mem")):
                nc, nk = rng.randrange(1, 7), rng.randrange(1, 5)
                prog = with_rotations(rng, fam[i % len(fam)](nc, nk), k)
                cases.append(Case(f"{name}{i % len(fam)}", prog, k, ext_k, (i + (name == "mem")) % 2 == 1))
            i += 1
    for k, ext_k in ((6, 8), (3, 3)):
        cases.append(Case("slots300", with_rotations(rng, parking_program(rng, 5, 3, 300), k), k, ext_k, ext_k > k))
    return cases


def sliceable_corpus(seed=20261017):
    """top-level fold sums for ZK_QUOTIENT_SLICES at ext_k >= 11"""
    import random
    rng = random.Random(seed)
    out = []
    for k, ext_k, divide in ((11, 11, False), (10, 12, True), (9, 12, False), (11, 12, True)):
        out.append(Case("sliceable", with_rotations(rng, sliceable_program(rng, 6, 4, 40), k), k, ext_k, divide))
    return out


def deep_case(depth, k, ext_k, seed=16):
    import random
    rng = random.Random(seed + depth)
    return Case(f"deep{depth}", with_rotations(rng, deep_program(rng, 5, 3, depth), k), k, ext_k, ext_k > k)


# ---- knob settings of the device tests and what they reach -----------------------------------------------------------------------
KNOBS = ("ZK_QUOTIENT_KERNEL", "ZK_QUOTIENT_MAC", "ZK_QUOTIENT_FUSE", "ZK_QUOTIENT_RELAXED", "ZK_QUOTIENT_SLICES")
SETTINGS = {"default": {}, "mac0": {"ZK_QUOTIENT_MAC": "0"}, "fuse0": {"ZK_QUOTIENT_FUSE": "0"}, "relaxed0": {"ZK_QUOTIENT_RELAXED": "0"},
            "kernel1": {"ZK_QUOTIENT_KERNEL": "1"}}
SLICE_SETTINGS = ("0", "2", "3", "64")
VARIANTS = [(kern, full, mem) for kern in ("v2", "v1") for full in (True, False) for mem in (True, False)] + [("sliced",)]
K_OPS = (K_ADD_COL, K_SUB_COL, K_RSUB_COL, K_MUL_COL, K_FOLD_COL, K_MAC_COL, K_NOP)


class knobs:
    """the evaluator's knobs set to exactly `env` (the others unset) inside the block, restored after it"""
    def __init__(self, env):
        self.env = env

    def __enter__(self):
        import os
        self.saved = {k: os.environ.get(k) for k in KNOBS}
        for k in KNOBS:
            os.environ.pop(k, None)
        os.environ.update(self.env)

    def __exit__(self, *a):
        import os
        for k, v in self.saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def setting_streams(case, env):
    """the lowered stream(s) zk_quotient_eval runs for the case under `env` (knobs must be in force): the whole program, or its slices"""
    v2 = env.get("ZK_QUOTIENT_KERNEL") != "1"
    fuse = fuse_of(env)
    cuts = slice_cuts(case.prog, case.ext_k) if v2 and (((1 << case.ext_k) // 256) & 7) == 0 else []
    if not cuts:
        return [lower(case.prog, case.ncols, fuse)[0]]
    return [lower(case.prog[x:y], case.ncols, fuse)[0] for x, y in zip(cuts, cuts[1:])]


def coverage():
    """over the device test's (case, setting) pairs: how often each kernel instantiation is launched (VARIANTS), how often each lowered
    opcode and each kind of settle / carry-propagation flag occurs"""
    from collections import Counter
    hits, ops, flags = Counter(), Counter(), Counter()
    runs = [(c, env) for c in corpus() for env in SETTINGS.values()]
    runs += [(c, {"ZK_QUOTIENT_SLICES": s}) for c in sliceable_corpus() for s in SLICE_SETTINGS]
    for c, env in runs:
        with knobs(env):
            hits[variant(c.prog, c.ncols, c.ext_k, env)] += 1
            for words in setting_streams(c, env):
                for w in words[0::3]:
                    w = int(w)
                    ops[w & 0xff] += 1
                    flags["settle"] += bool(w & K_SETTLE)
                    flags["settle8"] += bool(w & K_SETTLE8)
                    flags["norm"] += bool(w & K_NORM)
    return hits, ops, flags

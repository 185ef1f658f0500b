"""CPU: the corpus of tests/quotient_programs.py -- nested folds, Horner sums, parking edges, stacks 16 deep, edge rotations, sliceable
sums -- through the lowering (zk_host_quotient_lower at fuse = 0, 1 and 3, with ZK_QUOTIENT_RELAXED on and off) and the limb-level
executor of test_quotient_lowering / test_quotient_mac, against big-int evaluation of the original program.  Besides every precondition
the executor asserts for ff29.hip.hpp, every stack entry must stay within the value cap of the rule in force at every step: 8p relaxed,
4p with ZK_QUOTIENT_RELAXED=0 (round 5's (4, 4) rule, which never needs the 8p settle).  The device runs the same corpus in
tests/test_gpu_quotient_paths.py; the coverage it relies on (every kernel instantiation, every lowered opcode) is asserted here too."""
import random
from collections import Counter

import pytest

import quotient_programs as qp
import test_quotient_lowering as tl
import test_quotient_mac as tm
from test_quotient_lowering import P, val


def _entry_value(s):
    """the value of a stack entry; a top limb that borrowed counts as negative"""
    top = s[8] - (1 << 32) if s[8] >= (1 << 31) else s[8]
    return val(s[:8]) + (top << 232)


def run_checked(words, cols, consts, num_cols, cap_v):
    """tm.run_lowered_mac with the value cap asserted after every instruction: every stack entry in [0, cap_v p), limbs below 4 x 2^29"""
    consts_rp = [(c * 32) % P for c in consts]
    st, tmp = [], {}
    acc = tl.unpack(0)
    prev_tee = None
    for pc in range(len(words) // 3):
        w0, a, b = (int(x) for x in words[3 * pc:3 * pc + 3])
        op = w0 & 0xff
        if cap_v <= 4:
            assert not w0 & qp.K_SETTLE8, f"pc {pc}: an 8p settle under the (4, 4) rule"
        if op == qp.K_MAC_COL:
            if a >= num_cols:
                assert prev_tee != a - num_cols, "intermediate read back by the instruction right behind its TEE (prefetch hazard)"
                mem = tmp[a - num_cols]
            else:
                mem = cols[(a, b)]
            prev_tee = None
            assert w0 & 0x2a00 == 0
            tm._flags0(w0, st)
            x = st.pop()
            st[-1] = tm.mul2add29(x, tl.unpack_x32(mem), st[-1], tl.unpack(consts_rp[w0 >> 16]))
        else:
            acc, prev_tee = tm._step(w0, a, b, st, acc, tmp, prev_tee, cols, consts, consts_rp, num_cols)
        for s in st:
            assert all(x < (4 << 29) for x in s), f"pc {pc}: a limb reached 4 x 2^29"
            assert 0 <= _entry_value(s) < cap_v * P, f"pc {pc}: a stack entry reached {cap_v}p"
    assert not st
    acc = tl.normalize29(acc)
    assert val(acc) < 64 * P
    return val(acc) % P


def _row_values(rng, prog, kind):
    vals = tl.col_values(rng, prog, "mixed" if kind == "pm2" else kind)
    if kind == "pm2":
        vals = {key: P - 2 for key in vals}
    return vals


def _programs():
    return [c.prog for c in qp.corpus()] + [c.prog for c in qp.sliceable_corpus()] + [qp.deep_case(16, 8, 8).prog]


@pytest.mark.parametrize("relaxed", ["1", "0"])
@pytest.mark.parametrize("fuse", [0, 1, 3])
def test_corpus_lowers_within_every_bound(fuse, relaxed, monkeypatch):
    monkeypatch.setenv("ZK_QUOTIENT_RELAXED", relaxed)
    cap_v = 8 if relaxed == "1" else 4
    rng = random.Random(1000 * fuse + int(relaxed))
    for i, prog in enumerate(_programs()):
        ncols, nconsts = qp.num_cols_consts(prog)
        words, depth = tl.lower(prog, ncols, fuse)
        assert depth <= qp.stack_depth(prog) <= qp.MAX_STACK
        kinds = ("max", "zero", "one", "pm2", "mixed") if len(prog) < 1000 else ("max", "mixed")
        for kind in kinds:
            cols = _row_values(rng, prog, kind)
            consts = qp.constants(rng, nconsts)
            assert run_checked(words, cols, consts, ncols, cap_v) == tl.run_plain(prog, cols, consts), (i, kind, fuse, relaxed)


def test_the_strict_rule_settles_more_and_never_past_4p(monkeypatch):
    """the two rules really differ on the corpus: relaxed streams carry 8p settles and carry propagations, strict ones neither"""
    seen = Counter()
    for relaxed in ("1", "0"):
        monkeypatch.setenv("ZK_QUOTIENT_RELAXED", relaxed)
        for prog in _programs():
            for fuse in (0, 1, 3):
                for w in tl.lower(prog, qp.num_cols_consts(prog)[0], fuse)[0][0::3]:
                    w = int(w)
                    seen[relaxed, "settle8"] += bool(w & qp.K_SETTLE8)
                    seen[relaxed, "norm"] += bool(w & qp.K_NORM)
                    seen[relaxed, "settle"] += bool(w & qp.K_SETTLE)
    assert seen["1", "settle8"] > 0 and seen["1", "norm"] > 0
    assert seen["0", "settle8"] == 0 and seen["0", "norm"] == 0
    assert seen["0", "settle"] > seen["1", "settle"]


def test_nested_folds_lower_like_any_other_fold():
    """PUSH a; PUSH b; FOLD c1; FOLD c2 and the nested FOLD_COL of a value parked right before it"""
    col = lambda i: (qp.Q_PUSH_COL, i, 0)
    cases = [[col(0), col(1), (qp.Q_FOLD, 0, 0), (qp.Q_FOLD, 1, 0)],
             [col(0), col(1), (qp.Q_ADD, 0, 0), (qp.Q_TEE_TMP, 0, 0), (qp.Q_PUSH_TMP, 0, 0), (qp.Q_FOLD, 0, 0), (qp.Q_FOLD, 1, 0)],
             [col(0), (qp.Q_SQUARE, 0, 0), col(1), (qp.Q_MUL_CONST, 0, 0), col(2), col(0), (qp.Q_MUL, 0, 0), (qp.Q_ADD, 0, 0), (qp.Q_FOLD, 1, 0),
              (qp.Q_FOLD, 0, 0)]]
    rng = random.Random(4)
    for prog in cases:
        assert qp.nested_folds(prog) >= 1
        for fuse in (0, 1, 3):
            words, _ = tl.lower(prog, 3, fuse)
            for kind in ("max", "zero", "one", "pm2", "mixed"):
                cols = _row_values(rng, prog, kind)
                consts = qp.constants(rng, 2)
                assert run_checked(words, cols, consts, 3, 8) == tl.run_plain(prog, cols, consts), (prog, fuse, kind)
    ops = [int(w) & 0xff for w in tl.lower(cases[1], 3, 1)[0][0::3]]
    assert ops[ops.index(qp.Q_TEE_TMP) + 1] == qp.K_NOP and qp.K_FOLD_COL in ops
    ops = [int(w) & 0xff for w in tl.lower(cases[2], 3, 3)[0][0::3]]
    assert qp.K_MAC_COL in ops


def test_the_corpus_has_the_shapes_it_promises():
    progs = _programs()
    assert sum(qp.nested_folds(p) for p in progs) >= 100
    assert sum(1 for p in progs if qp.nested_folds(p)) >= 30
    assert max(len({a for op, a, b in p if op == qp.Q_TEE_TMP}) for p in progs) >= 300
    rots = {b for p in progs for op, a, b in p if op == qp.Q_PUSH_COL}
    assert {0x7fffffff, 0x80000000, 1, 2, qp.M32 - 1, qp.M32 - 2} <= rots
    for c in qp.corpus():
        assert all(b in set(qp.edge_rotations(c.k)) | {0, 1, 2, qp.M32 - 1} for op, a, b in c.prog if op == qp.Q_PUSH_COL)
    for k in (3, 8, 11):
        n = 1 << k
        assert {(n - 1), (-(n - 1)) % qp.M32, n, (-n) % qp.M32, n + 1, (-(n + 1)) % qp.M32} <= set(qp.edge_rotations(k))
    assert {c.ext_k - c.k for c in qp.corpus()} == {0, 1, 2, 3}
    assert {(c.ext_k, c.divide) for c in qp.corpus()} >= {(e, d) for e in qp.SIZES_EXT_K for d in (False, True)}


def test_stacks_at_the_limit():
    """caller depth exactly 16 stays 14 .. 16 deep after the lowering (its operands cannot come from memory); 17 is what the device refuses
    (tests/test_gpu_quotient_paths.py), and what the lowering reports as 17"""
    deep = qp.deep_case(16, 8, 8).prog
    assert qp.stack_depth(deep) == 16
    for fuse in (0, 1, 3):
        _, depth = tl.lower(deep, qp.num_cols_consts(deep)[0], fuse)
        assert 14 <= depth <= 16, fuse
    deeper = qp.deep_case(17, 8, 8).prog
    assert qp.stack_depth(deeper) == 17
    _, depth = tl.lower(deeper, qp.num_cols_consts(deeper)[0], 0)
    assert depth == 17


def test_the_corpus_reaches_every_kernel_instantiation_and_every_opcode():
    hits, ops, flags = qp.coverage()
    assert all(hits[v] >= 3 for v in qp.VARIANTS), hits
    assert set(qp.K_OPS) <= set(ops), ops
    assert all(flags[f] > 0 for f in ("settle", "settle8", "norm")), flags

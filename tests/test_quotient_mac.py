"""The evaluator's fused Horner steps (csrc/quotient_lower.hpp: lower_fuse with mac, K_MAC_COL; zk_host_quotient_lower with fuse & 2), checked on
the CPU.

A Horner step of a compiled class program,  S MUL_CONST y^gap <X> MUL_COL m [SUB_COL n ...] ADD,  becomes  S <X> MAC_COL(m, y^gap)
[SUB_COL n ...]:  t0 = X * 32 m + S * y^gap  under ONE Montgomery reduction (mul2add29), the chain of sums behind the product moved after
it.  The executor of test_quotient_lowering is extended with that instruction (every limb and column bound asserted, as it asserts them
for the others) and runs the fuse = 3 stream of random Horner-shaped programs and of the EVM-style class programs against plain big-int
evaluation.  The fuse = 1 stream -- what every existing test and the kernel with ZK_QUOTIENT_MAC=0 see -- must be what it was.
"""
import ctypes
import hashlib
import os
import random

import numpy as np
import pytest

import test_quotient_lowering as tl
from test_quotient_lowering import M, INV, MASK, P, R, val

K_MAC_COL = 22


def mul2add29(a, b, c, d):
    """(a b + c d) 2^-261 mod p as mul2add29_c / mul2add29_ub_ipa compute it: both products in the same column sums, one reduction"""
    assert all(x <= MASK + 8 for x in b[:8]) and all(x <= MASK + 8 for x in d[:8]), "the second factors must be normalised"
    assert val(a) * val(b) + val(c) * val(d) < (1 << 261) * P, "mul2add29: a b + c d must be below 2^261 p"
    m = [0] * 9
    t = [0] * 9
    acc = 0
    for k in range(17):
        lo, hi = (0, k) if k < 9 else (k - 8, 8)
        for i in range(lo, hi + 1):
            acc += a[i] * b[k - i] + c[i] * d[k - i]
        for i in range(lo, k if k < 9 else 9):
            acc += m[i] * M[k - i]
        assert acc < (1 << 64), "column overflow"
        if k < 9:
            m[k] = ((acc & 0xffffffff) * INV) & MASK
            acc += m[k] * M[0]
            assert acc < (1 << 64), "column overflow"
        else:
            t[k - 9] = acc & MASK
        acc >>= 29
    t[8] = acc
    assert acc < (1 << 32)
    assert val(t) < 2 * P and (val(t) << 261) % P == (val(a) * val(b) + val(c) * val(d)) % P
    return t


def run_lowered_mac(words, cols, consts, num_cols):
    """tl.run_lowered extended with MAC_COL: the other instructions run through the same primitives of test_quotient_lowering in the same
    order (_step), MAC_COL through mul2add29 above"""
    consts_rp = [(c * 32) % P for c in consts]
    st, tmp = [], {}
    acc = tl.unpack(0)
    prev_tee = None
    n = len(words) // 3
    for pc in range(n):
        w0, a, b = (int(x) for x in words[3 * pc:3 * pc + 3])
        op = w0 & 0xff
        if op != K_MAC_COL:
            acc, prev_tee = _step(w0, a, b, st, acc, tmp, prev_tee, cols, consts, consts_rp, num_cols)
            continue
        if a >= num_cols:
            assert prev_tee != a - num_cols, "intermediate read back by the instruction right behind its TEE (prefetch hazard)"
            mem = tmp[a - num_cols]
        else:
            mem = cols[(a, b)]
        assert mem < P
        prev_tee = None
        assert w0 & 0x2a00 == 0, "MAC_COL never asks for the entry below the top to be settled (the kernel has no step for it)"
        _flags0(w0, st)
        x = st.pop()                    # t0 = X; the entry below it, S, takes the result
        st[-1] = mul2add29(x, tl.unpack_x32(mem), st[-1], tl.unpack(consts_rp[w0 >> 16]))
        assert all(x < (1 << 31) for s2 in st for x in s2)
    assert not st
    acc = tl.normalize29(acc)
    assert val(acc) < 64 * P
    return val(acc) % P


def _flags0(w0, st):
    if w0 & 0x100:
        st[-1] = tl.settle(st[-1])
    if w0 & 0x400:
        st[-1] = tl.normalize29(st[-1])
    if w0 & 0x1000:
        st[-1] = tl.settle8(st[-1])


def _step(w0, a, b, st, acc, tmp, prev_tee, cols, consts, consts_rp, num_cols):
    """one lowered instruction other than MAC_COL, exactly as tl.run_lowered executes it (its loop body over the shared stack)"""
    op = w0 & 0xff
    has_mem = op == tl.Q_PUSH_COL or tl.K_ADD_COL <= op <= tl.K_FOLD_COL
    mem = None
    if has_mem:
        if a >= num_cols:
            assert prev_tee != a - num_cols, "intermediate read back by the instruction right behind its TEE (prefetch hazard)"
            mem = tmp[a - num_cols]
        else:
            mem = cols[(a, b)]
        assert mem < P
    prev_tee = a if op == tl.Q_TEE_TMP else None
    if w0 & 0x100:
        st[-1] = tl.settle(st[-1])
    if w0 & 0x200:
        st[-2] = tl.settle(st[-2])
    if w0 & 0x400:
        st[-1] = tl.normalize29(st[-1])
    if w0 & 0x800:
        st[-2] = tl.normalize29(st[-2])
    if w0 & 0x1000:
        st[-1] = tl.settle8(st[-1])
    if w0 & 0x2000:
        st[-2] = tl.settle8(st[-2])
    if op == tl.Q_PUSH_COL:
        st.append(tl.unpack(mem))
    elif op == tl.Q_PUSH_CONST:
        st.append(tl.unpack(consts[a]))
    elif op == tl.Q_ADD:
        y = st.pop(); st[-1] = tl.add29(st[-1], y)
    elif op == tl.Q_SUB:
        y = st.pop(); st[-1] = tl.normalize29(tl.sub29k(2, st[-1], y, normalised_after=True))
    elif op == tl.Q_MUL:
        y = st.pop(); st[-1] = tl.mul29(st[-1], tl.shl5(y))
    elif op == tl.Q_NEG:
        st[-1] = tl.normalize29(tl.sub29k(2, tl.unpack(0), st[-1], normalised_after=True))
    elif op == tl.Q_SQUARE:
        st[-1] = tl.mul29(st[-1], tl.shl5(st[-1]))
    elif op == tl.Q_DOUBLE:
        st[-1] = tl.add29(st[-1], st[-1])
    elif op == tl.Q_FOLD:
        acc = tl.add29(tl.mul29(acc, tl.unpack(consts_rp[a])), st.pop())
    elif op == tl.Q_MUL_CONST:
        st[-1] = tl.mul29(st[-1], tl.unpack(consts_rp[a]))
    elif op == tl.Q_ADD_CONST:
        st[-1] = tl.add29(st[-1], tl.unpack(consts[a]))
    elif op == tl.Q_TEE_TMP:
        tmp[a] = tl.pack_lt2p(st[-1])
    elif op == tl.K_ADD_COL:
        st[-1] = tl.add29(st[-1], tl.unpack(mem))
    elif op == tl.K_SUB_COL:
        st[-1] = tl.sub29k(2, st[-1], tl.unpack(mem), normalised_after=False)
    elif op == tl.K_RSUB_COL:
        st[-1] = tl.normalize29(tl.sub29k(2, tl.unpack(mem), st[-1], normalised_after=True))
    elif op == tl.K_MUL_COL:
        st[-1] = tl.mul29(st[-1], tl.unpack_x32(mem))
    elif op == tl.K_FOLD_COL:
        acc = tl.add29(tl.mul29(acc, tl.unpack(consts_rp[w0 >> 16])), tl.unpack(mem))
    elif op == tl.K_NOP:
        pass
    else:
        raise AssertionError(f"unknown lowered opcode {op}")
    assert all(x < (1 << 31) for s_ in st for x in s_), "stack limbs must stay below 2^31"
    return acc, prev_tee


def test_the_extended_executor_is_the_lowering_tests_executor_on_streams_without_mac():
    rng = random.Random(5)
    for trial in range(40):
        ncols, nconsts = rng.randrange(1, 6), rng.randrange(1, 4)
        prog = tl.random_program(rng, ncols, nconsts, statements=rng.randrange(1, 5), depth=rng.randrange(1, 5))
        words, _ = tl.lower(prog, ncols, 1)
        cols = tl.col_values(rng, prog, "mixed")
        consts = [rng.randrange(P) for _ in range(nconsts)]
        assert run_lowered_mac(words, cols, consts, ncols) == tl.run_lowered(words, cols, consts, ncols)


# ---- Horner-shaped random programs ---------------------------------------------------------------------------------------------
def random_horner_program(rng, ncols, nconsts, items, depth):
    """acc-style sums as the class compiler emits them:  S_0; S MUL_CONST c <term> ADD ...; FOLD -- terms X * m with chains of
    +- columns / + constants behind them (the fusable shape) mixed with arbitrary expressions (which must stay as they are)"""
    prog, defined, nxt = [], set(), [0]
    col = lambda: (tl.Q_PUSH_COL, rng.randrange(ncols), rng.choice([0, 0, 1, -1 & 0xffffffff]))
    for _ in range(rng.randrange(1, 4)):
        tl.random_expr(rng, ncols, nconsts, depth, defined, nxt, prog)
        for _ in range(items):
            prog.append((tl.Q_MUL_CONST, rng.randrange(nconsts), 0))
            if rng.random() < 0.75:
                if rng.random() < 0.5:                                   # X * m
                    tl.random_expr(rng, ncols, nconsts, depth - 1, defined, nxt, prog)
                    prog.append(col()); prog.append((tl.Q_MUL, 0, 0))
                else:                                                    # m * X
                    prog.append(col())
                    tl.random_expr(rng, ncols, nconsts, depth - 1, defined, nxt, prog)
                    prog.append((tl.Q_MUL, 0, 0))
                for _ in range(rng.randrange(0, 4)):
                    k = rng.random()
                    if k < 0.4:
                        prog.append(col()); prog.append((tl.Q_SUB, 0, 0))
                    elif k < 0.8:
                        prog.append(col()); prog.append((tl.Q_ADD, 0, 0))
                    else:
                        prog.append((tl.Q_ADD_CONST, rng.randrange(nconsts), 0))
            else:
                tl.random_expr(rng, ncols, nconsts, depth, defined, nxt, prog)
            prog.append((tl.Q_ADD, 0, 0))
        prog.append((tl.Q_FOLD, rng.randrange(nconsts), 0))
    return prog


def count_mac(words):
    return sum(1 for w in words[0::3] if int(w) & 0xff == K_MAC_COL)


def test_fused_horner_programs_match_plain_evaluation_and_keep_every_bound():
    rng = random.Random(20261016)
    fused = 0
    for trial in range(120):
        ncols, nconsts = rng.randrange(1, 7), rng.randrange(1, 4)
        prog = random_horner_program(rng, ncols, nconsts, items=rng.randrange(1, 7), depth=rng.randrange(1, 4))
        words, depth = tl.lower(prog, ncols, 3)
        assert depth <= 16
        words1, depth1 = tl.lower(prog, ncols, 1)
        assert depth <= depth1
        n_mac = count_mac(words)
        fused += n_mac
        # one instruction fewer per fused step: the ADD
        assert len(words) // 3 <= len(words1) // 3 - n_mac + sum(1 for w in words[0::3] if int(w) & 0xff == tl.K_NOP)
        for kind in ("max", "mixed", "mixed", "zero", "one"):
            cols = tl.col_values(rng, prog, kind)
            consts = [rng.choice([P - 1, 1, R % P, rng.randrange(P)]) for _ in range(nconsts)]
            assert run_lowered_mac(words, cols, consts, ncols) == tl.run_plain(prog, cols, consts), (trial, kind, prog)
    assert fused >= 150


@pytest.mark.parametrize("fuse", [3])
def test_random_programs_with_fuse_3_match_plain_evaluation(fuse):
    """the lowering test's own random programs (few Horner shapes) through the fused stream"""
    rng = random.Random(20260924)
    for trial in range(120):
        ncols, nconsts = rng.randrange(1, 7), rng.randrange(1, 4)
        prog = tl.random_program(rng, ncols, nconsts, statements=rng.randrange(1, 6), depth=rng.randrange(1, 6))
        words, depth = tl.lower(prog, ncols, fuse)
        for kind in ("max", "mixed", "zero"):
            cols = tl.col_values(rng, prog, kind)
            consts = [rng.choice([P - 1, 1, R % P, rng.randrange(P)]) for _ in range(nconsts)]
            assert run_lowered_mac(words, cols, consts, ncols) == tl.run_plain(prog, cols, consts), (trial, kind)


def test_fusion_needs_a_small_constant_index_and_a_product_by_memory():
    col = lambda i, r=0: (tl.Q_PUSH_COL, i, r)
    # S y^g + X * m - n: fused, the SUB_COL behind the MAC
    prog = [col(0), (tl.Q_MUL_CONST, 0, 0), col(1), col(2), (tl.Q_MUL, 0, 0), col(3), (tl.Q_SUB, 0, 0), (tl.Q_ADD, 0, 0), (tl.Q_FOLD, 0, 0)]
    words, _ = tl.lower(prog, 4, 3)
    assert [int(w) & 0xff for w in words[0::3]] == [tl.Q_PUSH_COL, tl.Q_PUSH_COL, K_MAC_COL, tl.K_SUB_COL, tl.Q_FOLD]
    assert int(words[6]) >> 16 == 0 and (int(words[7]), int(words[8])) == (2, 0)
    words1, _ = tl.lower(prog, 4, 1)
    assert [int(w) & 0xff for w in words1[0::3]] == [tl.Q_PUSH_COL, tl.Q_MUL_CONST, tl.Q_PUSH_COL, tl.K_MUL_COL, tl.K_SUB_COL, tl.Q_ADD, tl.Q_FOLD]
    # S y^g + (a + b): no product, nothing to fuse
    prog = [col(0), (tl.Q_MUL_CONST, 0, 0), col(1), col(2), (tl.Q_ADD, 0, 0), (tl.Q_ADD, 0, 0), (tl.Q_FOLD, 0, 0)]
    words, _ = tl.lower(prog, 3, 3)
    assert count_mac(words) == 0 and np.array_equal(words, tl.lower(prog, 3, 1)[0])
    # a constant index that does not fit next to the opcode: not fused
    prog = [col(0), (tl.Q_MUL_CONST, 1 << 16, 0), col(1), col(2), (tl.Q_MUL, 0, 0), (tl.Q_ADD, 0, 0), (tl.Q_FOLD, 0, 0)]
    words, _ = tl.lower(prog, 3, 3)
    assert count_mac(words) == 0


# ---- the fuse = 1 stream is what it was ------------------------------------------------------------------------------------------
def _evm_class_program(states=4, per_state=8, input_cols=4, cond_cols=2):
    import test_quotient_compile as tqc
    from zkevm_circuits_amd import binding
    c, spec, terms = tqc.evm_terms(states=states, per_state=per_state, input_cols=input_cols, cond_cols=cond_cols)
    K = len(terms)
    prog, last, st = tqc.compile_class(binding, terms, list(range(K)), K)
    return c, terms, prog, last


def _concretise(c, prog, y):
    import test_quotient_compile as tqc
    col_ix, const_ix, consts_tab = {}, {}, []

    def cst(a):
        if a not in const_ix:
            v = 1 if a == tqc.C_ONE else (pow(y, a - tqc.YPOW0, P) if a >= tqc.YPOW0 else c.consts[a] % P)
            const_ix[a] = len(consts_tab)
            consts_tab.append(v)
        return const_ix[a]
    conc = []
    for op, a, b in prog:
        if op == tqc.PUSH_COL:
            col_ix.setdefault((a, b), len(col_ix))
            conc.append((op, col_ix[(a, b)], 0))
        elif op in (tqc.PUSH_CONST, tqc.MUL_CONST, tqc.ADD_CONST, tqc.FOLD):
            conc.append((op, cst(a), 0))
        else:
            conc.append((op, a, b))
    return conc, col_ix, consts_tab


def _fuse1_digest():
    h = hashlib.sha256()
    rng = random.Random(99)
    for trial in range(60):
        ncols, nconsts = rng.randrange(1, 7), rng.randrange(1, 4)
        prog = random_horner_program(rng, ncols, nconsts, items=rng.randrange(1, 7), depth=rng.randrange(1, 4)) if trial % 2 else \
            tl.random_program(rng, ncols, nconsts, statements=rng.randrange(1, 6), depth=rng.randrange(1, 6))
        words, depth = tl.lower(prog, ncols, 1)
        h.update(np.asarray(words, dtype=np.uint32).tobytes()); h.update(bytes([depth]))
    c, terms, prog, last = _evm_class_program()
    conc, col_ix, _ = _concretise(c, prog, 3)
    words, depth = tl.lower(conc, len(col_ix), 1)
    h.update(np.asarray(words, dtype=np.uint32).tobytes()); h.update(bytes([depth]))
    return h.hexdigest()


# recorded with the lowering as it was before the fused forms existed
FUSE1_DIGEST = "c2fecf644d7bc25ba876241391760ed6791be935ec453115a068c7d262dd32df"


def test_the_fuse_1_stream_is_unchanged():
    assert _fuse1_digest() == FUSE1_DIGEST


# ---- the EVM-style class programs ------------------------------------------------------------------------------------------------
def test_evm_style_class_program_fused_keeps_the_value_and_every_bound():
    import test_quotient_compile as tqc
    c, terms, prog, last = _evm_class_program()
    rng = random.Random(8)
    y = rng.randrange(P)
    conc, col_ix, consts_tab = _concretise(c, prog, y)
    ncols = len(col_ix)
    words, depth = tl.lower(conc, ncols, 3)
    words1, depth1 = tl.lower(conc, ncols, 1)
    assert depth <= depth1 <= 16
    assert count_mac(words) >= 0.15 * sum(1 for op, a, b in conc if op == tqc.MUL_CONST)
    RR = 1 << 256
    rinv = pow(RR, -1, P)
    for trial in range(3):
        pick = [lambda: 0, lambda: 1, lambda: P - 1, lambda: rng.randrange(P)]
        vals = {key: (pick[rng.randrange(4)]() if trial else rng.randrange(P)) for key in col_ix}
        lowered_cols = {(i, 0): vals[key] for key, i in col_ix.items()}
        got = run_lowered_mac(words, lowered_cols, [v * RR % P for v in consts_tab], ncols)
        cols_plain = {key: v * rinv % P for key, v in vals.items()}
        want = 0
        for i, p_ in enumerate(terms):
            want = (want + pow(y, last - i, P) * tqc.evaluate_rot(p_, cols_plain, [x % P for x in c.consts])) % P
        assert got == want * RR % P


def _plan(blob, E, cap_classes_words):
    from zkevm_circuits_amd import binding
    lib = binding.lib()
    summ = np.zeros(8 + cap_classes_words * (E + 1), dtype=np.uint32)
    n_ = ctypes.c_uint32()
    assert lib.zk_host_quotient_plan(blob, ctypes.c_size_t(len(blob)), summ.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(summ.size),
                                     ctypes.c_uint32(0xFFFFFFFF), None, ctypes.c_size_t(0), ctypes.byref(n_)) == 0
    return summ


def _class_program(blob, e, n_hint=400000):
    from zkevm_circuits_amd import binding
    lib = binding.lib()
    summ = np.zeros(8 + 8 * (e + 8), dtype=np.uint32)
    out = np.zeros(3 * n_hint, dtype=np.uint32)
    n_ = ctypes.c_uint32()
    assert lib.zk_host_quotient_plan(blob, ctypes.c_size_t(len(blob)), summ.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(summ.size),
                                     ctypes.c_uint32(e), out.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(out.size), ctypes.byref(n_)) == 0
    return out[:3 * n_.value].reshape(-1, 3)


def _lowered_fused_count(prog):
    """MAC_COL instructions in the fuse = 3 stream of a plan's class program (columns and constants numbered densely, as the prover's
    concretisation does)"""
    prog = prog.copy()
    cols, consts = {}, {}
    for r in prog:
        if r[0] == tl.Q_PUSH_COL:
            r[1] = cols.setdefault((int(r[1]), int(r[2])), len(cols)); r[2] = 0
        elif r[0] in (tl.Q_PUSH_CONST, tl.Q_MUL_CONST, tl.Q_ADD_CONST, tl.Q_FOLD):
            r[1] = consts.setdefault(int(r[1]), len(consts))
    words, _ = tl.lower([tuple(int(x) for x in r) for r in prog], len(cols), 3)
    return count_mac(words)


@pytest.mark.parametrize("shape", ["evm", "plain"])
def test_plan_reports_the_fused_steps(shape):
    """zk_host_quotient_plan with room for them: reductions and fused multiply-accumulates per class; the fused count is what the lowering
    of that class's program makes; ZK_QUOTIENT_MAC=0 reports none.  The EVM-style block of the headline: at least 2 000 fused steps per
    row of its large class."""
    import bench_proof as bp
    from zkevm_circuits_amd import plonk
    if shape == "evm":
        p = dict(bp.EVM_DEFAULT)
        c = plonk.Circuit(10, num_fixed=1, num_advice=bp.evm_step_columns(p), num_instance=0, blinding_factors=5)
        bp.evm_block(c, 0, c.fixed_col(0), p)
    else:
        import plonk_fixtures
        c, _, _ = plonk_fixtures.build_circuit(6, seed=3, wide=True)
    blob = c.cs_blob()
    E = c.extended_k() - c.k
    s = _plan(blob, E, 10)
    base = 8 + 8 * (E + 1)
    assert np.array_equal(s[:base], _plan(blob, E, 8)), "the first 8 + 8 (E + 1) words do not depend on the room given"
    total = 0
    for e in range(E + 1):
        products, reductions, fused = int(s[8 + 8 * e + 2]), int(s[base + 2 * e]), int(s[base + 2 * e + 1])
        assert reductions + fused == products
        if s[8 + 8 * e]:
            assert fused == _lowered_fused_count(_class_program(blob, e))
        total += fused
    if shape == "evm":
        assert max(int(s[base + 2 * e + 1]) for e in range(E + 1)) >= 2000, s[base:]
    os.environ["ZK_QUOTIENT_MAC"] = "0"
    try:
        s0 = _plan(blob, E, 10)
    finally:
        os.environ.pop("ZK_QUOTIENT_MAC")
    assert np.array_equal(s0[:base], s[:base])
    assert all(int(s0[base + 2 * e + 1]) == 0 for e in range(E + 1))

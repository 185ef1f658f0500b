"""Sums of two column products and stack products under one reduction (csrc/quotient_lower.hpp: lower_fuse with mac2; PUSH_COL32, MAC2_COL,
MAC_STK; zk_host_quotient_lower with fuse & 4), checked on the CPU.

A Horner step over a sum of two column products,  S MUL_CONST c <X> MUL_COL m1 <Y> MUL_COL m2 ADD [chain] ADD,  becomes
S <X> PUSH_COL32 m1 <Y> MAC2_COL(m2, c) [chain]:  t0 = Y * 32 m2 + X * 32 m1 + S * c  under ONE Montgomery reduction; one over a product of
two computed values,  S MUL_CONST c <U> <V> MUL [chain] ADD,  becomes  S <U> <V> MAC_STK(c) [chain]:  t0 = U * 32 V + S * c.
test_quotient_mac's executor is extended with the three instructions: every value bound (169.3 p^2 < 2^261 p), every 64-bit column sum and
every limb bound is asserted while random programs rich in the two shapes run against plain big-int evaluation.  The fuse = 0 ... 3 streams
must be what they were."""
import ctypes
import hashlib
import os
import random

import numpy as np
import pytest

import test_quotient_lowering as tl
import test_quotient_mac as tm
from test_quotient_lowering import M, INV, MASK, P, R, val

K_MAC_COL, K_PUSH_COL32, K_MAC2_COL, K_MAC_STK = 22, 23, 24, 25
FLAGS0, FLAGS1 = 0x100 | 0x400 | 0x1000, 0x200 | 0x800 | 0x2000


def mulsum29(prods):
    """(sum of a b over the pairs) 2^-261 mod p as mul2add29_c / mul3add29_c and the generated in-place forms compute it: every product
    in the same column sums, one reduction"""
    assert all(x <= MASK + 8 for _, b in prods for x in b[:8]), "the second factors must be normalised"
    total = sum(val(a) * val(b) for a, b in prods)
    assert total < (1 << 261) * P, "the sum of the products must be below 2^261 p"
    m = [0] * 9
    t = [0] * 9
    acc = 0
    for k in range(17):
        lo, hi = (0, k) if k < 9 else (k - 8, 8)
        for a, b in prods:
            for i in range(lo, hi + 1):
                acc += a[i] * b[k - i]
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
    assert val(t) < 2 * P and (val(t) << 261) % P == total % P
    return t


def test_mulsum29_is_test_quotient_macs_product_on_two_pairs():
    rng = random.Random(3)
    for _ in range(20):
        a, c = ([rng.randrange(1 << 30) for _ in range(8)] + [rng.randrange(1 << 22)] for _ in range(2))
        b, d = (tl.unpack(rng.randrange(P)) for _ in range(2))
        assert mulsum29([(a, b), (c, d)]) == tm.mul2add29(a, b, c, d)


def run_lowered_mac2(words, cols, consts, num_cols, seen=None):
    """tm.run_lowered_mac extended with PUSH_COL32, MAC2_COL and MAC_STK; `seen` counts the settle requests the new instructions carried"""
    consts_rp = [(c * 32) % P for c in consts]
    st, tmp = [], {}
    acc = tl.unpack(0)
    prev_tee = None
    for pc in range(len(words) // 3):
        w0, a, b = (int(x) for x in words[3 * pc:3 * pc + 3])
        op = w0 & 0xff
        if op not in (K_MAC_COL, K_PUSH_COL32, K_MAC2_COL, K_MAC_STK):
            acc, prev_tee = tm._step(w0, a, b, st, acc, tmp, prev_tee, cols, consts, consts_rp, num_cols)
            continue
        mem = None
        if op != K_MAC_STK:
            if a >= num_cols:
                assert prev_tee != a - num_cols, "intermediate read back by the instruction right behind its TEE (prefetch hazard)"
                mem = tmp[a - num_cols]
            else:
                mem = cols[(a, b)]
            assert mem < P
        prev_tee = None
        if seen is not None and w0 & (FLAGS0 | FLAGS1) and op != K_MAC_COL:
            seen[op] = seen.get(op, 0) + 1
        if op == K_MAC_COL:
            assert w0 & FLAGS1 == 0
            tm._flags0(w0, st)
            x = st.pop()
            st[-1] = mulsum29([(x, tl.unpack_x32(mem)), (st[-1], tl.unpack(consts_rp[w0 >> 16]))])
        elif op == K_PUSH_COL32:
            # the kernel applies this instruction's bit-0 requests to the entry it spills (X), and has no other step for it
            assert w0 & FLAGS1 == 0 and w0 >> 16 == 0
            tm._flags0(w0, st)
            st.append(tl.unpack_x32(mem))
        elif op == K_MAC2_COL:
            # 32 m1, X and S are in LDS: only the top can be settled
            assert w0 & FLAGS1 == 0, "MAC2_COL never asks for an entry below the top to be settled (the kernel has no step for it)"
            tm._flags0(w0, st)
            y = st.pop(); m1 = st.pop(); x = st.pop()
            st[-1] = mulsum29([(y, tl.unpack_x32(mem)), (x, m1), (st[-1], tl.unpack(consts_rp[w0 >> 16]))])
        else:
            # the entry below the top is popped into registers (bit-1 requests reach it); S, below that, stays in LDS
            tm._flags0(w0, st)
            if w0 & 0x200:
                st[-2] = tl.settle(st[-2])
            if w0 & 0x800:
                st[-2] = tl.normalize29(st[-2])
            if w0 & 0x2000:
                st[-2] = tl.settle8(st[-2])
            v = st.pop(); u = st.pop()
            st[-1] = mulsum29([(u, tl.shl5(v)), (st[-1], tl.unpack(consts_rp[w0 >> 16]))])
        assert all(x < (1 << 31) for s2 in st for x in s2)
    assert not st
    acc = tl.normalize29(acc)
    assert val(acc) < 64 * P
    return val(acc) % P


# ---- random programs rich in the two shapes ---------------------------------------------------------------------------------------
def random_pair_program(rng, ncols, nconsts, items, depth):
    """acc-style sums as the class compiler emits them, the terms X * m1 + Y * m2 (either factor order, sometimes under a chain of +- columns /
    + constants), U * V with computed U and V, and test_quotient_mac's shapes mixed"""
    prog, defined, nxt = [], set(), [0]
    col = lambda: (tl.Q_PUSH_COL, rng.randrange(ncols), rng.choice([0, 0, 1, -1 & 0xffffffff]))
    expr = lambda d: tl.random_expr(rng, ncols, nconsts, max(d, 0), defined, nxt, prog)

    def product_by_column(d):
        if rng.random() < 0.5:
            expr(d); prog.append(col())
        else:
            prog.append(col()); expr(d)
        prog.append((tl.Q_MUL, 0, 0))

    def chain():
        for _ in range(rng.randrange(0, 3)):
            k = rng.random()
            if k < 0.4:
                prog.append(col()); prog.append((tl.Q_SUB, 0, 0))
            elif k < 0.8:
                prog.append(col()); prog.append((tl.Q_ADD, 0, 0))
            else:
                prog.append((tl.Q_ADD_CONST, rng.randrange(nconsts), 0))
    for _ in range(rng.randrange(1, 4)):
        expr(depth)
        for _ in range(items):
            prog.append((tl.Q_MUL_CONST, rng.randrange(nconsts), 0))
            r = rng.random()
            if r < 0.45:                                                 # X * m1 + Y * m2
                product_by_column(depth - 1)
                product_by_column(rng.choice([0, 0, depth - 1]))
                prog.append((tl.Q_ADD, 0, 0))
                chain()
            elif r < 0.65:                                               # U * V
                expr(depth); expr(depth)
                if prog[-1][0] in (tl.Q_PUSH_COL, tl.Q_PUSH_CONST, tl.Q_PUSH_TMP):      # keep V a computed value
                    prog.append((tl.Q_DOUBLE, 0, 0))
                prog.append((tl.Q_MUL, 0, 0))
                chain()
            elif r < 0.85:                                               # X * m (test_quotient_mac's shape)
                product_by_column(depth - 1)
                chain()
            else:
                expr(depth)
            prog.append((tl.Q_ADD, 0, 0))
        prog.append((tl.Q_FOLD, rng.randrange(nconsts), 0))
    return prog


def count_ops(words):
    ops = [int(w) & 0xff for w in words[0::3]]
    return {o: ops.count(o) for o in (K_MAC_COL, K_PUSH_COL32, K_MAC2_COL, K_MAC_STK, tl.K_NOP)}


def stream_depth(words):
    """stack entries the lowered stream holds at its peak"""
    d = mx = 0
    for w in words[0::3]:
        o = int(w) & 0xff
        d += {tl.Q_PUSH_COL: 1, tl.Q_PUSH_CONST: 1, K_PUSH_COL32: 1, tl.Q_ADD: -1, tl.Q_SUB: -1, tl.Q_MUL: -1, tl.Q_FOLD: -1, K_MAC_COL: -1,
              K_MAC_STK: -2, K_MAC2_COL: -3}.get(o, 0)
        mx = max(mx, d)
    assert d == 0
    return mx


SEED = 20261017
# what the generator yields with SEED on the CPU: 142 MAC2_COL and 135 MAC_STK over the 120 programs (small programs are often too shallow for
# MAC2_COL's extra entry, which is then declined); a lowering that fuses nothing, or only one of the shapes, cannot pass
MIN_MAC2, MIN_MAC_STK = 120, 110


def test_fused_pair_programs_match_plain_evaluation_and_keep_every_bound():
    rng = random.Random(SEED)
    mac2 = mac_stk = 0
    seen = {}
    for trial in range(120):
        ncols, nconsts = rng.randrange(1, 7), rng.randrange(1, 4)
        prog = random_pair_program(rng, ncols, nconsts, items=rng.randrange(1, 7), depth=rng.randrange(1, 4))
        words, depth = tl.lower(prog, ncols, 7)
        words3, depth3 = tl.lower(prog, ncols, 3)
        # the design allows NO extra depth: a fusion that would deepen the stack is declined (the LDS stack caps the launch's occupancy)
        assert depth <= depth3 <= 16 and stream_depth(words) == depth
        n = count_ops(words)
        assert n[K_PUSH_COL32] == n[K_MAC2_COL]
        mac2 += n[K_MAC2_COL]; mac_stk += n[K_MAC_STK]
        # per MAC2_COL: two MUL_COL and two ADD become PUSH_COL32 + MAC2_COL, the MUL_CONST goes; per MAC_STK: MUL_CONST and ADD go
        assert len(words) // 3 <= len(words3) // 3 + n[tl.K_NOP]
        for w0 in words[0::3]:
            if int(w0) & 0xff in (K_PUSH_COL32, K_MAC2_COL):
                assert int(w0) & FLAGS1 == 0
        for kind in ("max", "mixed", "mixed", "zero", "one"):
            cols = tl.col_values(rng, prog, kind)
            consts = [rng.choice([P - 1, 1, R % P, rng.randrange(P)]) for _ in range(nconsts)]
            assert run_lowered_mac2(words, cols, consts, ncols, seen) == tl.run_plain(prog, cols, consts), (trial, kind, prog)
    assert mac2 >= MIN_MAC2 and mac_stk >= MIN_MAC_STK, (mac2, mac_stk)
    # the settle requests riding on the new instructions are exercised, not only permitted
    assert seen.get(K_PUSH_COL32, 0) and seen.get(K_MAC2_COL, 0) and seen.get(K_MAC_STK, 0), seen


def test_the_other_random_programs_with_fuse_7_match_plain_evaluation():
    for gen, seed in ((tm.random_horner_program, 20261016), (None, 20260924)):
        rng = random.Random(seed)
        for trial in range(80):
            ncols, nconsts = rng.randrange(1, 7), rng.randrange(1, 4)
            prog = gen(rng, ncols, nconsts, items=rng.randrange(1, 7), depth=rng.randrange(1, 4)) if gen else \
                tl.random_program(rng, ncols, nconsts, statements=rng.randrange(1, 6), depth=rng.randrange(1, 6))
            words, depth = tl.lower(prog, ncols, 7)
            assert depth <= tl.lower(prog, ncols, 3)[1]
            for kind in ("max", "mixed", "zero"):
                cols = tl.col_values(rng, prog, kind)
                consts = [rng.choice([P - 1, 1, R % P, rng.randrange(P)]) for _ in range(nconsts)]
                assert run_lowered_mac2(words, cols, consts, ncols) == tl.run_plain(prog, cols, consts), (trial, kind)


def test_the_shapes_and_what_declines_them():
    col = lambda i, r=0: (tl.Q_PUSH_COL, i, r)
    ops = lambda words: [int(w) & 0xff for w in words[0::3]]
    # S c + a * m1 + b * m2 - n
    prog = [col(0), (tl.Q_MUL_CONST, 0, 0), col(1), col(2), (tl.Q_MUL, 0, 0), col(3), col(4), (tl.Q_MUL, 0, 0), (tl.Q_ADD, 0, 0), col(5), (tl.Q_SUB, 0, 0),
            (tl.Q_ADD, 0, 0), (tl.Q_FOLD, 0, 0)]
    # alone, the fuse = 3 stream of this program is 3 deep and MAC2_COL would need 4: declined, and the first product joins S c in a MAC_COL instead
    words, depth = tl.lower(prog, 6, 7)
    assert tl.lower(prog, 6, 3)[1] == 3 and depth == 2
    assert ops(words) == [tl.Q_PUSH_COL, tl.Q_PUSH_COL, K_MAC_COL, tl.Q_PUSH_COL, tl.K_MUL_COL, tl.Q_ADD, tl.K_SUB_COL, tl.Q_FOLD]
    # behind a statement that is 4 deep anyway it is fused: S, X, PUSH_COL32 m1, Y, MAC2_COL(m2, c), the chain behind
    deep = [col(0), (tl.Q_DOUBLE, 0, 0), col(1), (tl.Q_DOUBLE, 0, 0), col(2), (tl.Q_DOUBLE, 0, 0), col(3), (tl.Q_DOUBLE, 0, 0), (tl.Q_MUL, 0, 0), (tl.Q_MUL, 0, 0),
            (tl.Q_MUL, 0, 0), (tl.Q_FOLD, 0, 0)]
    words, depth = tl.lower(deep + prog, 6, 7)
    assert depth == 4 == tl.lower(deep + prog, 6, 3)[1]
    tail = ops(words)[-7:]
    assert tail == [tl.Q_PUSH_COL, tl.Q_PUSH_COL, K_PUSH_COL32, tl.Q_PUSH_COL, K_MAC2_COL, tl.K_SUB_COL, tl.Q_FOLD], tail
    w = words.reshape(-1, 3)[-5:]
    assert (int(w[0][1]), int(w[2][1])) == (2, 4) and int(w[2][0]) >> 16 == 0
    # S c + (a + b) * (c + d): a stack product, no deeper than before
    prog = [col(0), (tl.Q_MUL_CONST, 1, 0), col(1), col(2), (tl.Q_ADD, 0, 0), col(3), col(4), (tl.Q_ADD, 0, 0), (tl.Q_MUL, 0, 0), (tl.Q_ADD, 0, 0), (tl.Q_FOLD, 0, 0)]
    words, depth = tl.lower(prog, 5, 7)
    assert ops(words) == [tl.Q_PUSH_COL, tl.Q_PUSH_COL, tl.K_ADD_COL, tl.Q_PUSH_COL, tl.K_ADD_COL, K_MAC_STK, tl.Q_FOLD] and depth == 3
    assert int(words[15]) >> 16 == 1
    # bit 2 alone (fuse = 5) is the fuse = 1 stream: the new forms are extensions of the Horner fusion
    assert np.array_equal(tl.lower(prog, 5, 5)[0], tl.lower(prog, 5, 1)[0])


# ---- fuse = 0 ... 3 are what they were --------------------------------------------------------------------------------------------
def _digest(fuse):
    h = hashlib.sha256()
    rng = random.Random(77)
    for trial in range(60):
        ncols, nconsts = rng.randrange(1, 7), rng.randrange(1, 4)
        prog = random_pair_program(rng, ncols, nconsts, items=rng.randrange(1, 7), depth=rng.randrange(1, 4))
        words, depth = tl.lower(prog, ncols, fuse)
        h.update(np.asarray(words, dtype=np.uint32).tobytes()); h.update(bytes([depth]))
    return h.hexdigest()


# recorded with the library as it was before PUSH_COL32 / MAC2_COL / MAC_STK existed
PARENT_DIGESTS = {
    0: "1aa9c265d32108b8e859ea915ad42559d67897c5be07307ffdfb145b13e4e1cd",
    1: "de189f98f806f1aa58f7c29d01162f8efb4488dd9d6150f08d112aa8acf1dc97",
    2: "72d569dc05faab9ef34e3bc3ad778ea4730ddb54bf46570fad648ab2fc213741",
    3: "72d569dc05faab9ef34e3bc3ad778ea4730ddb54bf46570fad648ab2fc213741",
}


@pytest.mark.parametrize("fuse", [0, 1, 2, 3])
def test_the_streams_without_the_new_bit_are_the_parents(fuse):
    assert _digest(fuse) == PARENT_DIGESTS[fuse]
    assert tm._fuse1_digest() == tm.FUSE1_DIGEST


# ---- the plan's report --------------------------------------------------------------------------------------------------------------
def _lowered_counts(prog, fuse):
    prog = prog.copy()
    cols, consts = {}, {}
    for r in prog:
        if r[0] == tl.Q_PUSH_COL:
            r[1] = cols.setdefault((int(r[1]), int(r[2])), len(cols)); r[2] = 0
        elif r[0] in (tl.Q_PUSH_CONST, tl.Q_MUL_CONST, tl.Q_ADD_CONST, tl.Q_FOLD):
            r[1] = consts.setdefault(int(r[1]), len(consts))
    words, depth = tl.lower([tuple(int(x) for x in r) for r in prog], len(cols), fuse)
    return count_ops(words), words, depth


@pytest.mark.parametrize("shape", ["evm", "plain"])
def test_plan_reports_the_new_fused_steps(shape):
    """with room for 8 + 14 (E + 1) words: per class MAC2_COL, MAC_STK, declined, reductions of the stream in force -- equal to a recount of the
    lowered words; the words before them do not depend on the room; ZK_QUOTIENT_MAC=1 / 0 report none.  The EVM-style block of the headline: at
    least 1 800 reductions fewer per row of its large class than the fuse = 3 stream (the count that decided the kernel work)."""
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
    s = tm._plan(blob, E, 14)
    base = 8 + 10 * (E + 1)
    assert np.array_equal(s[:base], tm._plan(blob, E, 10)[:base]), "the first 8 + 10 (E + 1) words do not depend on the room given"
    for e in range(E + 1):
        products, red3, fused3 = int(s[8 + 8 * e + 2]), int(s[8 + 8 * (E + 1) + 2 * e]), int(s[8 + 8 * (E + 1) + 2 * e + 1])
        mac2, mac_stk, declined, reductions = (int(x) for x in s[base + 4 * e:base + 4 * e + 4])
        assert red3 + fused3 == products
        if s[8 + 8 * e]:
            n, _, _ = _lowered_counts(tm._class_program(blob, e), 7)
            assert (mac2, mac_stk) == (n[K_MAC2_COL], n[K_MAC_STK])
            assert reductions == products - n[K_MAC_COL] - 2 * mac2 - mac_stk
    if shape == "evm":
        # counted on the CPU before the kernel was written (profiles/r08_quotient_mac2.md): 395 MAC2_COL, 211 MAC_STK and 1 867 reductions fewer than
        # the fuse = 3 stream per row of the large class
        e = max(range(E + 1), key=lambda e: int(s[8 + 8 * e + 1]))
        assert int(s[base + 4 * e]) >= 350 and int(s[base + 4 * e + 1]) >= 200, s[base:]
        assert int(s[8 + 8 * (E + 1) + 2 * e]) - int(s[base + 4 * e + 3]) >= 1800, s[base:]
    for knob in ("1", "0"):
        os.environ["ZK_QUOTIENT_MAC"] = knob
        try:
            s1 = tm._plan(blob, E, 14)
        finally:
            os.environ.pop("ZK_QUOTIENT_MAC")
        assert np.array_equal(s1[:8 + 8 * (E + 1)], s[:8 + 8 * (E + 1)])
        for e in range(E + 1):
            assert tuple(int(x) for x in s1[base + 4 * e:base + 4 * e + 3]) == (0, 0, 0)
            assert int(s1[base + 4 * e + 3]) == int(s1[8 + 8 * e + 2]) - int(s1[8 + 8 * (E + 1) + 2 * e + 1])


def test_evm_style_class_program_with_fuse_7_keeps_the_value_and_every_bound():
    import test_quotient_compile as tqc
    c, terms, prog, last = tm._evm_class_program()
    rng = random.Random(8)
    y = rng.randrange(P)
    conc, col_ix, consts_tab = tm._concretise(c, prog, y)
    ncols = len(col_ix)
    words, depth = tl.lower(conc, ncols, 7)
    assert depth <= tl.lower(conc, ncols, 3)[1] <= 16
    RR = 1 << 256
    rinv = pow(RR, -1, P)
    for trial in range(3):
        pick = [lambda: 0, lambda: 1, lambda: P - 1, lambda: rng.randrange(P)]
        vals = {key: (pick[rng.randrange(4)]() if trial else rng.randrange(P)) for key in col_ix}
        lowered_cols = {(i, 0): vals[key] for key, i in col_ix.items()}
        got = run_lowered_mac2(words, lowered_cols, [v * RR % P for v in consts_tab], ncols)
        cols_plain = {key: v * rinv % P for key, v in vals.items()}
        want = 0
        for i, p_ in enumerate(terms):
            want = (want + pow(y, last - i, P) * tqc.evaluate_rot(p_, cols_plain, [x % P for x in c.consts])) % P
        assert got == want * RR % P

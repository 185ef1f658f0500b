"""The evaluator's record mode (csrc/quotient.hip: k_quotient_eval2 with REC), checked on the CPU.

A class program of a proof reads its coset operands as records: the nine canonical limbs of 32 v mod p, i.e. the R' = 2^261 form of
the value a packed column holds in R = 2^256 form.  The kernel then interprets the SAME lowered words (zk_host_quotient_lower at any
fuse level) with
  * memory operands taken as they arrive -- no unpacking, and no x 32 form: MUL_COL, MAC_COL, PUSH_COL32 and MAC2_COL read the plain limbs,
  * no shift by 5 in front of a stack product (MUL, SQUARE, MAC_STK),
  * additive constants (PUSH_CONST, ADD_CONST) in R' form like the multiplying ones,
  * a parked intermediate stored as the canonical limbs of its (R'-form) value.
Every value on the stack and in the accumulator is then in R' form, a product reduced by 2^261 is again, and the result is 32 x what
the packed program gives.  This test executes the words that way with the limb arithmetic of test_quotient_lowering -- every limb,
column and value bound the packed executors assert, asserted -- and compares with 32 x the plain big-int evaluation.  The bounds the
lowering derived for operands "up to 32 p" must hold for canonical ones; nothing here may lean on the packed executors' results.
"""
import random

import pytest

import quotient_programs as qp
import test_quotient_lowering as tl
import test_quotient_mac as tm
import test_quotient_mac2 as tm2
from test_quotient_corpus import _entry_value
from test_quotient_lowering import MASK, P, R, val

K_MAC_COL, K_PUSH_COL32, K_MAC2_COL, K_MAC_STK = 22, 23, 24, 25
MEM_OPS = {tl.Q_PUSH_COL, tl.K_ADD_COL, tl.K_SUB_COL, tl.K_RSUB_COL, tl.K_MUL_COL, tl.K_FOLD_COL, K_MAC_COL, K_PUSH_COL32, K_MAC2_COL}
ALL_ONES = val([MASK] * 8 + [0])            # 2^232 - 1: every limb below the top all ones (below p)
ALL_ONES_TOP = val([MASK] * 8 + [(P >> 232) - 1])       # the same under the largest top limb that keeps the value below p


def to_rp(v):
    """R form -> R' form, canonical"""
    return v * 32 % P


def settled(x):
    """what a product takes as its second factor without a shift: normalised, below 2p (q_shl5's precondition, kept although nothing shifts)"""
    assert all(v <= MASK for v in x[:8]) and val(x) < 2 * P
    return x


def run_records(words, cols, consts, num_cols, cap_v=8):
    """cols, consts: canonical R-form integers (as the packed executors take them); the record-mode kernel sees 32 x each.  Returns the
    canonical accumulator, which must be 32 x the plain value."""
    rec = {key: to_rp(v) for key, v in cols.items()}
    consts_rp = [to_rp(c) for c in consts]
    st, tmp = [], {}
    acc = tl.unpack(0)
    prev_tee = None
    for pc in range(len(words) // 3):
        w0, a, b = (int(x) for x in words[3 * pc:3 * pc + 3])
        op = w0 & 0xff
        mem = None
        if op in MEM_OPS:
            if a >= num_cols:
                assert prev_tee != a - num_cols, "intermediate read back by the instruction right behind its TEE (prefetch hazard)"
                mem = tmp[a - num_cols]
            else:
                mem = rec[(a, b)]
            assert mem < P
            mem = tl.unpack(mem)              # the record: canonical limbs, used as they are by every instruction
        prev_tee = a if op == tl.Q_TEE_TMP else None
        if op in (K_MAC_COL, K_PUSH_COL32, K_MAC2_COL):
            assert w0 & tm2.FLAGS1 == 0       # the kernel has no step for an entry in LDS
            tm._flags0(w0, st)
        else:
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
        if op == tl.Q_PUSH_COL or op == K_PUSH_COL32:
            st.append(mem)
        elif op == tl.Q_PUSH_CONST:
            st.append(tl.unpack(consts_rp[a]))
        elif op == tl.Q_ADD:
            y = st.pop(); st[-1] = tl.add29(st[-1], y)
        elif op == tl.Q_SUB:
            y = st.pop(); st[-1] = tl.normalize29(tl.sub29k(2, st[-1], y, normalised_after=True))
        elif op == tl.Q_MUL:
            y = st.pop(); st[-1] = tl.mul29(st[-1], settled(y))
        elif op == tl.Q_NEG:
            st[-1] = tl.normalize29(tl.sub29k(2, tl.unpack(0), st[-1], normalised_after=True))
        elif op == tl.Q_SQUARE:
            st[-1] = tl.mul29(st[-1], settled(st[-1]))
        elif op == tl.Q_DOUBLE:
            st[-1] = tl.add29(st[-1], st[-1])
        elif op == tl.Q_FOLD:
            acc = tl.add29(tl.mul29(acc, tl.unpack(consts_rp[a])), st.pop())
        elif op == tl.Q_MUL_CONST:
            st[-1] = tl.mul29(st[-1], tl.unpack(consts_rp[a]))
        elif op == tl.Q_ADD_CONST:
            st[-1] = tl.add29(st[-1], tl.unpack(consts_rp[a]))
        elif op == tl.Q_TEE_TMP:
            tmp[a] = tl.pack_lt2p(st[-1])     # canon29_lt2p: the canonical limbs of a normalised value below 2p
        elif op == tl.K_ADD_COL:
            st[-1] = tl.add29(st[-1], mem)
        elif op == tl.K_SUB_COL:
            st[-1] = tl.sub29k(2, st[-1], mem, normalised_after=False)
        elif op == tl.K_RSUB_COL:
            st[-1] = tl.normalize29(tl.sub29k(2, mem, st[-1], normalised_after=True))
        elif op == tl.K_MUL_COL:
            st[-1] = tl.mul29(st[-1], mem)
        elif op == tl.K_FOLD_COL:
            acc = tl.add29(tl.mul29(acc, tl.unpack(consts_rp[w0 >> 16])), mem)
        elif op == K_MAC_COL:
            x = st.pop()
            st[-1] = tm2.mulsum29([(x, mem), (st[-1], tl.unpack(consts_rp[w0 >> 16]))])
        elif op == K_MAC2_COL:
            y = st.pop(); m1 = st.pop(); x = st.pop()
            st[-1] = tm2.mulsum29([(y, mem), (x, m1), (st[-1], tl.unpack(consts_rp[w0 >> 16]))])
        elif op == K_MAC_STK:
            v = st.pop(); u = st.pop()
            st[-1] = tm2.mulsum29([(u, settled(v)), (st[-1], tl.unpack(consts_rp[w0 >> 16]))])
        elif op == tl.K_NOP:
            pass
        else:
            raise AssertionError(f"unknown lowered opcode {op}")
        for s in st:
            assert all(x < (1 << 31) for x in s), f"pc {pc}: stack limbs must stay below 2^31"
            assert all(x < (4 << 29) for x in s), f"pc {pc}: a limb reached 4 x 2^29"
            assert 0 <= _entry_value(s) < cap_v * P, f"pc {pc}: a stack entry reached {cap_v}p"
    assert not st
    acc = tl.normalize29(acc)
    assert val(acc) < 64 * P
    return val(acc) % P


def edge_rows(rng, prog):
    """one row per edge value in every column, then mixed rows.  The values are what the RECORDS hold (the kernel's operands); the
    R-form value handed to the executors is that / 32."""
    keys = sorted({(a, b) for op, a, b in prog if op == tl.Q_PUSH_COL})
    inv32 = pow(32, -1, P)
    edges = [0, 1, P - 1, ALL_ONES, ALL_ONES_TOP]
    rows = [{key: e * inv32 % P for key in keys} for e in edges]
    for _ in range(2):
        rows.append({key: rng.choice(edges + [rng.randrange(P), rng.randrange(P)]) * inv32 % P for key in keys})
    return rows


def check(prog, ncols, nconsts, fuse, rng, consts=None):
    words, depth = tl.lower(prog, ncols, fuse)
    assert depth <= 16
    for cols in edge_rows(rng, prog):
        cs = consts if consts is not None else [rng.choice([P - 1, 1, 0, R % P, ALL_ONES, rng.randrange(P)]) for _ in range(nconsts)]
        assert run_records(words, cols, cs, ncols) == to_rp(tl.run_plain(prog, cols, cs)), (fuse, prog[:12])


def test_the_edge_values_are_what_they_claim():
    assert ALL_ONES < ALL_ONES_TOP < P
    assert tl.unpack(ALL_ONES)[:8] == [MASK] * 8 and tl.unpack(ALL_ONES_TOP)[:8] == [MASK] * 8
    rng = random.Random(1)
    prog = [(tl.Q_PUSH_COL, 0, 0), (tl.Q_PUSH_COL, 1, 1), (tl.Q_MUL, 0, 0), (tl.Q_FOLD, 0, 0)]
    rows = edge_rows(rng, prog)
    assert [to_rp(r[(0, 0)]) for r in rows[:5]] == [0, 1, P - 1, ALL_ONES, ALL_ONES_TOP]


@pytest.mark.parametrize("fuse", [1, 3, 7])
def test_random_programs_in_record_mode(fuse):
    """the programs of test_quotient_lowering, of test_quotient_mac (Horner steps) and of test_quotient_mac2 (pairs of products)"""
    rng = random.Random(20261019 + fuse)
    for trial in range(60):
        ncols, nconsts = rng.randrange(1, 7), rng.randrange(1, 4)
        check(tl.random_program(rng, ncols, nconsts, statements=rng.randrange(1, 6), depth=rng.randrange(1, 6)), ncols, nconsts, fuse, rng)
        check(tm.random_horner_program(rng, ncols, nconsts, items=rng.randrange(1, 7), depth=rng.randrange(1, 4)), ncols, nconsts, fuse, rng)
        check(tm2.random_pair_program(rng, ncols, nconsts, items=rng.randrange(1, 7), depth=rng.randrange(1, 4)), ncols, nconsts, fuse, rng)


@pytest.mark.parametrize("fuse", [1, 3, 7])
def test_corpus_in_record_mode(fuse):
    rng = random.Random(3000 + fuse)
    progs = [c.prog for c in qp.corpus()] + [c.prog for c in qp.sliceable_corpus()] + [qp.deep_case(16, 8, 8).prog]
    for prog in progs:
        ncols, nconsts = qp.num_cols_consts(prog)
        if len(prog) < 1000:
            check(prog, ncols, nconsts, fuse, rng)
        else:                                     # the long ones: the all-(p - 1) row and a mixed one
            words, _ = tl.lower(prog, ncols, fuse)
            for cols in edge_rows(rng, prog)[2::3]:
                cs = qp.constants(rng, nconsts)
                assert run_records(words, cols, cs, ncols) == to_rp(tl.run_plain(prog, cols, cs))


def test_the_fused_forms_are_reached_in_record_mode():
    """fuse 7 streams of the pair programs carry MAC_COL, PUSH_COL32 / MAC2_COL and MAC_STK: the forms whose x 32 operand became a plain one"""
    rng = random.Random(tm2.SEED)
    seen = {K_MAC_COL: 0, K_PUSH_COL32: 0, K_MAC2_COL: 0, K_MAC_STK: 0}
    for _ in range(40):
        ncols, nconsts = rng.randrange(1, 7), rng.randrange(1, 4)
        prog = tm2.random_pair_program(rng, ncols, nconsts, items=rng.randrange(1, 7), depth=rng.randrange(1, 4))
        for w0 in tl.lower(prog, ncols, 7)[0][0::3]:
            if int(w0) & 0xff in seen:
                seen[int(w0) & 0xff] += 1
    assert all(seen.values()), seen

"""GPU: one proof over the ordering gadget of the state circuit, every advice column made on the device from RW rows handed over
UNSORTED: ZK_OP_KEY_SORT puts them in order, ONE ZK_OP_KEY_ORDER over that permutation makes limb_difference, its inverse, the five
bit columns of first_different_limb, not_first_access and the gathered limb columns, and zk_proof_advice_phase_typed_dev takes the
buffers as they are (2-byte limbs, 1-byte bits, 32-byte field elements).  The gates are the gadget's
(state_circuit/lexicographic_ordering.rs:109-189): q (1 - diff inv), booleanity of the bits, q [index = j] (diff - cur_j + prev_j)
for j in Tag, Address0, FieldTag, RwCounter1, RwCounter0 over the limb columns at rotations 0 and -1, and not_first_access tied to
the bits.  That route yields the proof bytes of the route on which every column comes from the Python model, which the oracle
verifier accepts and which equal the oracle prover's; both multi-open schemes.  One changed cell in any column fails check_witness."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import key_order_cases as kc  # noqa: E402
from oracle import bn254 as b  # noqa: E402
from oracle import pairing as pr  # noqa: E402
from oracle import plonk_prover as pp  # noqa: E402
from oracle import plonk_verifier as pv  # noqa: E402
from test_gpu_proof_typed import S_SECRET, SEED, Case  # noqa: E402
from zkevm_circuits_amd import plonk  # noqa: E402

pytestmark = pytest.mark.gpu
R = b.R_MOD
GATED = (0, 12, 13, 30, 31)                                            # Tag, Address0, FieldTag, RwCounter1, RwCounter0
LIMB = {j: c for c, j in enumerate(GATED)}                             # advice columns 0..4: the gathered limbs
BIT0, NOT_FIRST, DIFF, INV, ADVICE = 5, 10, 11, 12, 13                 # 5..9: bit planes 0..4 (plane 0 the most significant)
PUBLIC_ROW = 7


def ordering_circuit(k):
    circ = plonk.Circuit(k, num_fixed=1, num_advice=ADVICE, num_instance=1, blinding_factors=5)
    q = circ.fixed_col(0)
    bits = [circ.advice_col(BIT0 + i) for i in range(5)]
    not_first, diff, inv = circ.advice_col(NOT_FIRST), circ.advice_col(DIFF), circ.advice_col(INV)
    circ.add_gate(q * (1 - diff * inv))
    for bit in bits:
        circ.add_gate(q * bit * (bit - 1))
    for j in GATED:
        is_j = plonk.wrap(1)
        for i, bit in enumerate(bits):
            is_j = is_j * (bit if j >> (4 - i) & 1 else 1 - bit)
        cur = circ.advice_col(LIMB[j])
        circ.add_gate(q * is_j * (diff - cur + cur.rot(-1)))
    circ.add_gate(q * (not_first - bits[0] * bits[1] * bits[2] * bits[3]))  # index 30 or 31: only the counter differs
    for row in range(1, circ.u):                                         # row 0 has no predecessor
        circ.fixed[0][row] = 1
    circ.copy((plonk.ADVICE, NOT_FIRST, PUBLIC_ROW), (plonk.INSTANCE, 0, 0))
    return circ


def rw_rows(u):
    """u RW rows that differ in tag, the last address limb, field_tag and the counter only, so that every adjacent pair of the
    sorted order differs first in one of the five gated limbs; shuffled, with distinct counters"""
    rng = kc.rng(0x0DE5)
    groups = [(tag, low, ft) for tag in (1, 2, 4) for low in (0x0100, 0x01FF, 0xFFFE) for ft in (0, 3)]
    rows = []
    for serial in range(u):
        tag, low, ft = rng.choice(groups)
        counter = rng.randrange(3) << 16 | (serial + 1) * 7            # distinct; neighbours of a group differ in RwCounter1 or only in RwCounter0
        rows.append(kc.pack(tag, 9, (0xABCD << 144) + low, ft, 5, counter))
    rng.shuffle(rows)
    return rows


def model_columns(keys, n):
    """the advice columns as integers, n rows: the model over the model's sort"""
    perm = kc.sort_perm(keys)
    cols = kc.order_columns(keys, perm, 30)
    limbs = kc.gather(keys, [(2 * j, 2) for j in GATED], perm)
    pad = lambda col: list(col) + [0] * (n - len(col))
    return [pad(c) for c in limbs] + [pad(c) for c in cols["bits"]] + [pad(cols["not_first"]), pad(cols["diff"]), pad(cols["inv"])], cols["index"]


@pytest.fixture(scope="module")
def case(ctx, cref):
    circ = ordering_circuit(6)
    keys = rw_rows(circ.u)
    adv, index = model_columns(keys, circ.n)
    c = Case(ctx, cref, circ, lambda phase, ch: dict(enumerate(adv)), [[adv[NOT_FIRST][PUBLIC_ROW]] + [0] * (circ.n - 1)])
    c.keys, c.adv, c.index = keys, adv, index
    yield c
    c.close()


@pytest.mark.parametrize("scheme", ["gwc", "shplonk"])
def test_host_route_is_accepted_and_equals_the_oracle_prover(case, scheme):
    circ, adv, index = case.circ, case.adv, case.index
    assert set(index[1:]) == set(GATED) and 0 < sum(adv[NOT_FIRST]) < circ.u - 1       # every gated limb decides some pair
    assert kc.sort_perm(case.keys) != list(range(circ.u))                              # handed over unsorted
    assert all(0 < d < 65536 for d in adv[DIFF][1:circ.u])                             # in order: the circuit's range lookup would accept
    proof, per_phase = case.fr_proof(scheme)
    assert [len(c) for c in per_phase] == [0]
    assert pv.check_witness(circ, adv, case.inst) is None
    for col in range(ADVICE):
        row = index.index(GATED[col], 1) if col < 5 else 9                               # a limb column is pinned where its limb decides
        wrong = [list(c) for c in adv]
        wrong[col][row] = (wrong[col][row] + 2) % R
        assert pv.check_witness(circ, wrong, case.inst) is not None, (col, row)
    assert pv.verify(circ, case.vk_points, case.vk_repr, case.inst, proof, pr.ec_mul(pr.G2_GEN, S_SECRET), multiopen=scheme)
    assert proof == pp.create_proof(circ, pp.Srs(circ.k, S_SECRET), adv, case.inst, case.vk_repr, SEED, scheme)


@pytest.mark.parametrize("scheme", ["gwc", "shplonk"])
def test_device_route_gives_the_same_bytes(ctx, cref, case, scheme):
    circ, keys = case.circ, case.keys
    n, u = circ.n, circ.u
    want, _ = case.fr_proof(scheme)
    d_keys = ctx.to_device(np.frombuffer(b"".join(keys), dtype=np.uint8))               # what a witness kernel left in HBM, in execution order
    d_perm = ctx.to_device(np.zeros(u, dtype=np.uint32))
    d_limbs = [ctx.to_device(np.zeros(n, dtype=np.uint16)) for _ in GATED]
    d_bits = ctx.to_device(np.zeros(5 * u, dtype=np.uint8))
    d_nf = ctx.to_device(np.zeros(n, dtype=np.uint8))
    d_diff, d_inv = (ctx.to_device(np.zeros((n, 4), dtype=np.uint64)) for _ in range(2))  # rows from usable_rows on stay zero
    sess = case.session(scheme)
    try:
        ctx.key_sort(d_keys, u, d_perm)                                                 # no host step from here ...
        ctx.key_order(d_keys, u, d_inv, perm=d_perm, diff=d_diff, bits=d_bits, not_first=d_nf, group_limbs=30,
                      cols=[(2 * j, 2, d_limbs[LIMB[j]]) for j in GATED])
        columns = {LIMB[j]: (d_limbs[LIMB[j]], 2) for j in GATED}
        columns.update({BIT0 + i: (d_bits.ptr + i * u, 1) for i in range(5)})
        columns.update({NOT_FIRST: (d_nf, 1), DIFF: (d_diff, 32), INV: (d_inv, 32)})
        assert len(sess.advice_phase_typed_dev(columns)) == 0                           # ... to here
        assert d_perm.download(u, np.uint32).tolist() == kc.sort_perm(keys)
        assert cref.from_mont(d_diff.download((n, 4))) == case.adv[DIFF] and cref.from_mont(d_inv.download((n, 4))) == case.adv[INV]
        proof = sess.finish()
    except BaseException:
        sess.abort()
        raise
    finally:
        for buf in (d_keys, d_perm, *d_limbs, d_bits, d_nf, d_diff, d_inv):
            buf.free()
    assert proof == want

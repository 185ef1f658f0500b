"""GPU: one proof over the columns of a Poseidon table -- advice hash_id, input0, input1, control, heading -- whose hash columns are
made on the device by ONE ZK_OP_POSEIDON (31-byte cells straight from the padded bytecode bytes, the final flag: hash_id into d_out,
input0 / input1 into d_word0 / d_word1) and whose control column, the remaining length times 2^64, by ONE ZK_OP_ROW_RLC; the columns
are handed over in one zk_proof_advice_phase_typed_dev call.  hash_id at row 0 is copied to an instance cell that holds the
reference's code hash of [1; 32] (eth-types/src/utils/codehash.rs:98-102).  That route yields the proof bytes of the route on which
every column is made from Python integers, which in turn equal the oracle prover's; both multi-open schemes."""
import os
import random
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import poseidon_cases as pc  # noqa: E402
from oracle import bn254 as b  # noqa: E402
from oracle import pairing as pr  # noqa: E402
from oracle import plonk_prover as pp  # noqa: E402
from oracle import plonk_verifier as pv  # noqa: E402
from test_gpu_proof_typed import S_SECRET, SEED, Case  # noqa: E402
from zkevm_circuits_amd import plonk  # noqa: E402

pytestmark = pytest.mark.gpu
R = b.R_MOD
HASH_ID, INPUT0, INPUT1, CONTROL, HEADING = range(5)                  # advice columns


def poseidon_table_circuit(k):
    """q selects the rows whose successor is usable too:  q heading (heading - 1),  q (1 - heading[+1]) (hash_id[+1] - hash_id).
    hash_id[0] is public."""
    circ = plonk.Circuit(k, num_fixed=1, num_advice=5, num_instance=1, blinding_factors=5)
    q = circ.fixed_col(0)
    heading = circ.advice_col(HEADING)
    circ.add_gate(q * heading * (heading - 1))
    circ.add_gate(q * (1 - circ.advice_col(HEADING, 1)) * (circ.advice_col(HASH_ID, 1) - circ.advice_col(HASH_ID)))
    for row in range(circ.u - 1):
        circ.fixed[0][row] = 1
    circ.copy((plonk.ADVICE, HASH_ID, 0), (plonk.INSTANCE, 0, 0))
    return circ


def table_witness(circ):
    """the reference's small codes ([1; 32] first) and a few random ones, then off rows up to usable_rows"""
    n, u = circ.n, circ.u
    rng = random.Random(24)
    golden = pc.golden_vectors()
    codes = [golden[3][0], golden[0][0], golden[1][0], golden[2][0]] + [bytes(rng.randrange(256) for _ in range(size)) for size in (31, 62, 63, 200, 333)]
    data, kinds, lens = pc.code_rows(codes)
    rows = len(kinds)
    assert rows < u
    rem = []
    for code in codes:
        rem += [len(code) - 62 * j for j in range(len(pc.padded_bytes(code)) // 62)]
    data += bytes(62 * (u - rows))
    kinds += [pc.OFF] * (u - rows)
    lens += [0] * (u - rows)
    rem += [0] * (u - rows)
    in0, in1 = pc.rows_of_bytes(data, u)
    hash_id, w0, w1 = pc.expected(in0, in1, lens, kinds, pc.CAP_SCALE_CODE, final=True)
    pad = lambda col: list(col) + [0] * (n - u)
    adv = [pad(hash_id), pad(w0), pad(w1), pad([r * pc.CAP_SCALE_CODE % R for r in rem]), pad([int(kd != pc.CONT) for kd in kinds])]
    assert hash_id[0] == golden[3][1] and hash_id[1:4] == [h for _, h in golden[:3]]
    return adv, dict(data=data, kinds=kinds, lens=lens, rem=rem, rows=rows)


@pytest.fixture(scope="module")
def case(ctx, cref):
    circ = poseidon_table_circuit(6)
    adv, raw = table_witness(circ)

    def synth(phase, ch):
        return dict(enumerate(adv))
    c = Case(ctx, cref, circ, synth, [[adv[HASH_ID][0]] + [0] * (circ.n - 1)])
    c.adv, c.raw = adv, raw
    yield c
    c.close()


@pytest.mark.parametrize("scheme", ["gwc", "shplonk"])
def test_host_route_is_accepted_and_equals_the_oracle_prover(case, scheme):
    circ = case.circ
    proof, _ = case.fr_proof(scheme)
    assert 0 < sum(case.adv[HEADING]) < circ.u and case.raw["rows"] > 9 and any(kd == pc.CONT for kd in case.raw["kinds"])
    assert pv.check_witness(circ, case.adv, case.inst) is None
    assert pv.verify(circ, case.vk_points, case.vk_repr, case.inst, proof, pr.ec_mul(pr.G2_GEN, S_SECRET), multiopen=scheme)
    assert proof == pp.create_proof(circ, pp.Srs(circ.k, S_SECRET), case.adv, case.inst, case.vk_repr, SEED, scheme)


@pytest.mark.parametrize("scheme", ["gwc", "shplonk"])
def test_device_route_gives_the_same_bytes(zk, ctx, cref, case, scheme):
    circ, raw = case.circ, case.raw
    n, u = circ.n, circ.u
    want, _ = case.fr_proof(scheme)
    d_bytes = ctx.to_device(np.frombuffer(b"\xEE" + raw["data"], dtype=np.uint8))       # what a witness kernel left in HBM; the cells start at an odd address
    d_len = ctx.to_device(np.array(raw["lens"], dtype=np.uint64))
    d_rem = ctx.to_device(np.array(raw["rem"], dtype=np.uint64))
    d_kinds = ctx.to_device(np.array(raw["kinds"], dtype=np.uint8))
    d_heading = ctx.to_device(np.array(case.adv[HEADING][:u], dtype=np.uint8))
    d_cols = [ctx.to_device(np.zeros((n, 4), dtype=np.uint64)) for _ in range(4)]       # rows from usable_rows on stay zero
    sess = case.session(scheme)
    try:
        ctx.poseidon(d_bytes.ptr + 1, 31, d_bytes.ptr + 32, 31, u, d_cols[HASH_ID], cap=d_len, cap_width=8, cap_scale=cref.to_mont([pc.CAP_SCALE_CODE])[0], kinds=d_kinds, final=True,
                     word0=d_cols[INPUT0], word1=d_cols[INPUT1])
        ctx.row_rlc([d_rem], [8], cref.to_mont([pc.CAP_SCALE_CODE]), u, d_cols[CONTROL])
        for col in (HASH_ID, INPUT0, INPUT1, CONTROL):
            assert cref.from_mont(d_cols[col].download((n, 4))) == case.adv[col], col
        typed = {col: (d_cols[col], 32) for col in (HASH_ID, INPUT0, INPUT1, CONTROL)}
        typed[HEADING] = (d_heading, 1)
        assert len(sess.advice_phase_typed_dev(typed)) == 0
        proof = sess.finish()
    except BaseException:
        sess.abort()
        raise
    finally:
        for buf in [d_bytes, d_len, d_rem, d_kinds, d_heading] + d_cols:
            buf.free()
    assert proof == want

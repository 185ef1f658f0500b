"""GPU: one proof whose second-phase column is a row RLC, z = b_0 + b_1 r + b_2 r^2 + b_3 r^3 + v r^4 over four byte columns and one
16-byte column of the first phase -- rlc::value over the cells of a row -- made on the device by ONE ZK_OP_ROW_RLC straight from the
packed first-phase cells, between zk_proof_advice_phase_typed_dev and zk_proof_advice_phase_dev.  Only the five weights are computed
on the host (from the challenge the first phase returned); nothing of z is.  That route yields the challenge and the proof bytes of
the route on which every column is computed with Python integers, which in turn equal the oracle prover's; both multi-open schemes."""
import os
import random
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from oracle import bn254 as b  # noqa: E402
from oracle import pairing as pr  # noqa: E402
from oracle import plonk_prover as pp  # noqa: E402
from oracle import plonk_verifier as pv  # noqa: E402
from test_gpu_proof_typed import S_SECRET, SEED, Case  # noqa: E402
from zkevm_circuits_amd import plonk  # noqa: E402

pytestmark = pytest.mark.gpu
R = b.R_MOD
BYTES, V, Z = (0, 1, 2, 3), 4, 5                       # advice columns


def row_rlc_circuit(k):
    """phase 0: b_0 .. b_3 (bytes), v (16 bytes); the challenge r after it; phase 1: z.  q selects the usable rows.
    Gate: q (z - (b_0 + b_1 r + b_2 r^2 + b_3 r^3 + v r^4)).  b_0[0] is public."""
    circ = plonk.Circuit(k, num_fixed=1, num_advice=6, num_instance=1, blinding_factors=5)
    q, z = circ.fixed_col(0), circ.advice_col(Z)
    circ.advice_phase = [0, 0, 0, 0, 0, 1]
    r = circ.challenge_usable_after(0)
    rlc, rp = circ.advice_col(BYTES[0]), r
    for j in (1, 2, 3):
        rlc = rlc + circ.advice_col(BYTES[j]) * rp
        rp = rp * r
    rlc = rlc + circ.advice_col(V) * rp
    circ.add_gate(q * (z - rlc))
    for row in range(circ.u):
        circ.fixed[0][row] = 1
    circ.copy((plonk.ADVICE, BYTES[0], 0), (plonk.INSTANCE, 0, 0))
    return circ


@pytest.fixture(scope="module")
def case(ctx, cref):
    circ = row_rlc_circuit(6)
    n, u = circ.n, circ.u
    rng = random.Random(20)
    bv = [[rng.randrange(256) if i < u else 0 for i in range(n)] for _ in BYTES]
    vv = [rng.choice([0, (1 << 128) - 1, rng.randrange(1 << 128)]) if i < u else 0 for i in range(n)]

    def synth(phase, ch):
        if phase == 0:
            return {**{BYTES[j]: bv[j] for j in range(4)}, V: vv}
        r = ch[0]
        return {Z: [(sum(bv[j][i] * pow(r, j, R) for j in range(4)) + vv[i] * pow(r, 4, R)) % R if i < u else 0 for i in range(n)]}
    c = Case(ctx, cref, circ, synth, [[bv[0][0]] + [0] * (n - 1)])
    c.bv, c.vv = bv, vv
    yield c
    c.close()


@pytest.mark.parametrize("scheme", ["gwc", "shplonk"])
def test_host_route_is_accepted_and_equals_the_oracle_prover(case, scheme):
    circ = case.circ
    proof, per_phase = case.fr_proof(scheme)
    assert [len(c) for c in per_phase] == [1, 0]
    ch = case.cref.from_mont(per_phase[0])
    adv = case.bv + [case.vv, case.synth(1, ch)[Z]]
    assert any(adv[Z][i] >= 1 << 128 for i in range(circ.u)), "the challenge reached no cell of z"
    assert pv.check_witness(circ, adv, case.inst, challenges=ch) is None
    assert pv.verify(circ, case.vk_points, case.vk_repr, case.inst, proof, pr.ec_mul(pr.G2_GEN, S_SECRET), multiopen=scheme)
    assert proof == pp.create_proof(circ, pp.Srs(circ.k, S_SECRET), adv, case.inst, case.vk_repr, SEED, scheme)


@pytest.mark.parametrize("scheme", ["gwc", "shplonk"])
def test_device_route_gives_the_same_challenge_and_bytes(zk, ctx, cref, case, scheme):
    circ = case.circ
    n, u = circ.n, circ.u
    want, want_ch = case.fr_proof(scheme)
    d_b = [ctx.to_device(np.array(col[:u], dtype=np.uint8)) for col in case.bv]          # what a witness kernel left in HBM
    d_v = ctx.to_device(np.array([[x & (2 ** 64 - 1), x >> 64] for x in case.vv[:u]], dtype=np.uint64))
    d_z = ctx.to_device(np.zeros((n, 4), dtype=np.uint64))                              # rows from usable_rows on stay zero
    sess = case.session(scheme)
    try:
        got = sess.advice_phase_typed_dev({**{BYTES[j]: (d_b[j], 1) for j in range(4)}, V: (d_v, 16)})
        assert np.array_equal(got, want_ch[0])
        r = cref.from_mont(got)[0]
        ctx.row_rlc(d_b + [d_v], [1, 1, 1, 1, 16], cref.to_mont([pow(r, j, R) for j in range(5)]), u, d_z)
        z = cref.from_mont(d_z.download((n, 4)))
        assert any(x >= 1 << 128 for x in z[:u]) and not any(z[u:])
        assert len(sess.advice_phase_dev({Z: d_z})) == 0
        proof = sess.finish()
    except BaseException:
        sess.abort()
        raise
    finally:
        for buf in d_b + [d_v, d_z]:
            buf.free()
    assert proof == want

"""GPU: one proof whose second-phase column -- a running RLC with resets, z[i] = z[i-1] r (1 - first[i]) + x[i], the reference's
rlc_acc form -- is made on the device from packed first-phase cells: zk_fr_from_uint, ZK_OP_SUB, zk_fr_scale and one ZK_OP_SCAN_AFFINE
between zk_proof_advice_phase_typed_dev and zk_proof_advice_phase_dev.  Nothing of z is computed on the host on that route, and it
yields the challenge and the proof bytes of the route on which every column is computed with Python integers, which in turn equal the
oracle prover's; both multi-open schemes."""
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
X, FIRST, Z = 0, 1, 2                                  # advice columns


def running_rlc_circuit(k):
    """phase 0: x (bytes), first (0 / 1); the challenge r after it; phase 1: z.  q selects the usable rows.
    Gate: q (z - (z(-1) r (1 - first) + x)); at row 0 z(-1) is a blinding row, so first[0] = 1.  x[0] is public."""
    circ = plonk.Circuit(k, num_fixed=1, num_advice=3, num_instance=1, blinding_factors=5)
    q, x, first, z = circ.fixed_col(0), circ.advice_col(X), circ.advice_col(FIRST), circ.advice_col(Z)
    circ.advice_phase = [0, 0, 1]
    r = circ.challenge_usable_after(0)
    circ.add_gate(q * (z - (z.rot(-1) * r * (1 - first) + x)))
    for row in range(circ.u):
        circ.fixed[0][row] = 1
    circ.copy((plonk.ADVICE, X, 0), (plonk.INSTANCE, 0, 0))
    return circ


@pytest.fixture(scope="module")
def case(ctx, cref):
    circ = running_rlc_circuit(6)
    n, u = circ.n, circ.u
    rng = random.Random(18)
    xv = [rng.randrange(256) if i < u else 0 for i in range(n)]
    fv = [0] * n
    for row in (0, 5, 6, 23, 40, u - 1):                                   # two adjacent rows, the last usable row
        fv[row] = 1

    def synth(phase, ch):
        if phase == 0:
            return {X: xv, FIRST: fv}
        zv, z = [0] * n, 0
        for i in range(u):
            z = (z * ch[0] * (1 - fv[i]) + xv[i]) % R
            zv[i] = z
        return {Z: zv}
    c = Case(ctx, cref, circ, synth, [[xv[0]] + [0] * (n - 1)])
    c.xv, c.fv = xv, fv
    yield c
    c.close()


@pytest.mark.parametrize("scheme", ["gwc", "shplonk"])
def test_host_route_is_accepted_and_equals_the_oracle_prover(case, scheme):
    circ = case.circ
    proof, per_phase = case.fr_proof(scheme)
    assert [len(c) for c in per_phase] == [1, 0]
    ch = case.cref.from_mont(per_phase[0])
    adv = [case.xv, case.fv, case.synth(1, ch)[Z]]
    assert any(adv[Z][i] >= 1 << 128 for i in range(circ.u)), "the challenge reached no cell of z"
    assert pv.check_witness(circ, adv, case.inst, challenges=ch) is None
    assert pv.verify(circ, case.vk_points, case.vk_repr, case.inst, proof, pr.ec_mul(pr.G2_GEN, S_SECRET), multiopen=scheme)
    assert proof == pp.create_proof(circ, pp.Srs(circ.k, S_SECRET), adv, case.inst, case.vk_repr, SEED, scheme)


@pytest.mark.parametrize("scheme", ["gwc", "shplonk"])
def test_device_route_gives_the_same_challenge_and_bytes(zk, ctx, cref, case, scheme):
    circ = case.circ
    n, u = circ.n, circ.u
    want, want_ch = case.fr_proof(scheme)
    cells = lambda v: ctx.to_device(np.array(v[:u], dtype=np.uint8))
    d_x, d_first, d_one = cells(case.xv), cells(case.fv), cells([1] * u)   # what a witness kernel left in HBM, one byte per cell
    d_a, d_b, d_f = ctx.alloc(u * 32), ctx.alloc(u * 32), ctx.alloc(u * 32)
    d_z = ctx.to_device(np.zeros((n, 4), dtype=np.uint64))                  # rows from usable_rows on stay zero
    sess = case.session(scheme)
    try:
        got = sess.advice_phase_typed_dev({X: (d_x, 1), FIRST: (d_first, 1)})
        assert np.array_equal(got, want_ch[0])
        r_mont = np.ascontiguousarray(got[0])
        ctx.fr_from_uint(d_x, 1, u, d_b)                                    # b = x
        ctx.fr_from_uint(d_first, 1, u, d_f)
        ctx.fr_from_uint(d_one, 1, u, d_a)
        ctx.field_vec_op(zk.FIELD_FR, zk.OP_SUB, d_a, d_f, d_a, u)          # 1 - first
        ctx.fr_scale(d_a, r_mont, u)                                        # a = r (1 - first)
        ctx.field_vec_op(zk.FIELD_FR, zk.OP_SCAN_AFFINE, d_a, d_b, d_z, u)
        assert len(sess.advice_phase_dev({Z: d_z})) == 0
        proof = sess.finish()
    except BaseException:
        sess.abort()
        raise
    finally:
        for buf in (d_x, d_first, d_one, d_a, d_b, d_f, d_z):
            buf.free()
    assert proof == want

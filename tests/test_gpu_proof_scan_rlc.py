"""GPU: one proof whose second-phase column -- a running RLC with restarts and padding rows, the reference's Keccak data_rlc form
z[i] = pad ? z[i-1] : z[i-1] r (1 - first[i]) + x[i] -- is made on the device by ONE ZK_OP_SCAN_RLC straight from the packed byte
cells that went to zk_proof_advice_phase_typed_dev, plus a kind buffer first + 2 pad, and handed to zk_proof_advice_phase_dev.
Nothing of z is computed on the host on that route, and it yields the challenge and the proof bytes of the route on which every
column is computed with Python integers, which the oracle verifier accepts and which equal the oracle prover's; both multi-open
schemes; a second circuit runs the scan from the last usable row down (the copy circuit's rlc_acc form, z(+1) in the gate)."""
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
X, FIRST, PAD, Z = 0, 1, 2, 3                          # advice columns


def scan_rlc_circuit(k, reverse):
    """phase 0: x (bytes), first, pad (0 / 1); the challenge r after it; phase 1: z.  q selects the usable rows.
    Gate: q (z - (pad z(-1) + (1 - pad) (z(-1) r (1 - first) + x))), z(+1) in place of z(-1) when reversed.  The neighbour of the row
    the scan starts at is a blinding row, so that row has first = 1 and pad = 0.  x[0] is public."""
    circ = plonk.Circuit(k, num_fixed=1, num_advice=4, num_instance=1, blinding_factors=5)
    q, x, first, pad, z = circ.fixed_col(0), circ.advice_col(X), circ.advice_col(FIRST), circ.advice_col(PAD), circ.advice_col(Z)
    circ.advice_phase = [0, 0, 0, 1]
    r = circ.challenge_usable_after(0)
    prev = z.rot(1 if reverse else -1)
    circ.add_gate(q * (z - (pad * prev + (1 - pad) * (prev * r * (1 - first) + x))))
    for row in range(circ.u):
        circ.fixed[0][row] = 1
    circ.copy((plonk.ADVICE, X, 0), (plonk.INSTANCE, 0, 0))
    return circ


def host_z(xv, fv, pv_, r, u, n, reverse):
    zv, z = [0] * n, 0
    for j in range(u):
        i = u - 1 - j if reverse else j
        if not pv_[i]:
            z = (z * r * (1 - fv[i]) + xv[i]) % R
        zv[i] = z
    return zv


@pytest.fixture(scope="module", params=[False, True], ids=["forward", "reverse"])
def case(request, ctx, cref):
    reverse = request.param
    circ = scan_rlc_circuit(6, reverse)
    n, u = circ.n, circ.u
    rng = random.Random(22)
    xv = [rng.randrange(256) if i < u else 0 for i in range(n)]
    fv, pd = [0] * n, [0] * n
    start, end = (u - 1, 0) if reverse else (0, u - 1)
    fv[start] = 1                                                          # the row the scan starts at
    for row in (5, 6, 23, 40):                                             # two adjacent restarts
        fv[row] = 1
    for row in (10, 11, 12, 22, 23, 41, end):                              # adjacent holds; a hold beside and ON a restart (kind 3); the last row of the scan
        pd[row] = 1
    assert {fv[i] + 2 * pd[i] for i in range(u)} == {0, 1, 2, 3} and fv[start] + 2 * pd[start] == 1 and pd[end] == 1

    def synth(phase, ch):
        if phase == 0:
            return {X: xv, FIRST: fv, PAD: pd}
        return {Z: host_z(xv, fv, pd, ch[0], u, n, reverse)}
    c = Case(ctx, cref, circ, synth, [[xv[0]] + [0] * (n - 1)])
    c.xv, c.fv, c.pd, c.reverse = xv, fv, pd, reverse
    yield c
    c.close()


@pytest.mark.parametrize("scheme", ["gwc", "shplonk"])
def test_host_route_is_accepted_and_equals_the_oracle_prover(case, scheme):
    circ = case.circ
    proof, per_phase = case.fr_proof(scheme)
    assert [len(c) for c in per_phase] == [1, 0]
    ch = case.cref.from_mont(per_phase[0])
    adv = [case.xv, case.fv, case.pd, case.synth(1, ch)[Z]]
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
    d_x, d_first, d_pad = cells(case.xv), cells(case.fv), cells(case.pd)   # what a witness kernel left in HBM, one byte per cell
    d_kind = cells([f + 2 * p for f, p in zip(case.fv, case.pd)])          # first + 2 pad: step, start, hold, hold
    d_z = ctx.to_device(np.zeros((n, 4), dtype=np.uint64))                  # rows from usable_rows on stay zero
    sess = case.session(scheme)
    try:
        got = sess.advice_phase_typed_dev({X: (d_x, 1), FIRST: (d_first, 1), PAD: (d_pad, 1)})
        assert np.array_equal(got, want_ch[0])
        one, zero = cref.fr_const(1)[0], cref.fr_const(0)[0]
        table = [(got[0], one), (zero, one), (one, zero), (one, zero)]      # a hold on a restart row holds
        ctx.scan_rlc(d_x, 1, d_kind, np.array(table, dtype=np.uint64), u, d_z, reverse=case.reverse)      # the ONE call
        assert len(sess.advice_phase_dev({Z: d_z})) == 0
        proof = sess.finish()
    except BaseException:
        sess.abort()
        raise
    finally:
        for buf in (d_x, d_first, d_pad, d_kind, d_z):
            buf.free()
    assert proof == want

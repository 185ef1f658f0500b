"""GPU: one proof with an IsEqual gadget -- advice a, b (8-byte cells), inv = inv0(a - b), eq = 1 - (a - b) inv -- whose inverse
column is made on the device by ONE ZK_OP_ROW_INV0 with weights (1, -1), straight from the packed cells of a and b, and handed over
with them in one zk_proof_advice_phase_typed_dev call.  Nothing of inv is computed on the host on that route (the reference's
IsZeroChip leaves it to the prover's batch inversion as an Assigned::Rational).  That route yields the proof bytes of the route on
which every column is made from Python integers, which in turn equal the oracle prover's; both multi-open schemes."""
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
A, B, INV, EQ = 0, 1, 2, 3                             # advice columns


def is_equal_circuit(k):
    """one phase: a, b, inv, eq; q selects the usable rows.  With d = a - b:
    q d (1 - d inv),  q inv (1 - d inv),  q (eq - (1 - d inv)).  a[0] is public."""
    circ = plonk.Circuit(k, num_fixed=1, num_advice=4, num_instance=1, blinding_factors=5)
    q = circ.fixed_col(0)
    d = circ.advice_col(A) - circ.advice_col(B)
    inv, eq = circ.advice_col(INV), circ.advice_col(EQ)
    is_zero = 1 - d * inv
    circ.add_gate(q * d * is_zero)
    circ.add_gate(q * inv * is_zero)
    circ.add_gate(q * (eq - is_zero))
    for row in range(circ.u):
        circ.fixed[0][row] = 1
    circ.copy((plonk.ADVICE, A, 0), (plonk.INSTANCE, 0, 0))
    return circ


@pytest.fixture(scope="module")
def case(ctx, cref):
    circ = is_equal_circuit(6)
    n, u = circ.n, circ.u
    rng = random.Random(23)
    av = [rng.choice([0, (1 << 64) - 1, rng.randrange(1 << 64)]) if i < u else 0 for i in range(n)]
    same = {0, u - 1} | {i for i in range(u) if i % 3 == 1}          # about a third of the usable rows, the first and the last among them
    bv = [(av[i] if i in same else (av[i] + rng.randrange(1, 1 << 64)) % (1 << 64)) if i < u else 0 for i in range(n)]
    invv = [pow((av[i] - bv[i]) % R, -1, R) if i < u and av[i] != bv[i] else 0 for i in range(n)]
    eqv = [int(av[i] == bv[i]) if i < u else 0 for i in range(n)]

    def synth(phase, ch):
        return {A: av, B: bv, INV: invv, EQ: eqv}
    c = Case(ctx, cref, circ, synth, [[av[0]] + [0] * (n - 1)])
    c.av, c.bv, c.invv, c.eqv, c.same = av, bv, invv, eqv, same
    yield c
    c.close()


@pytest.mark.parametrize("scheme", ["gwc", "shplonk"])
def test_host_route_is_accepted_and_equals_the_oracle_prover(case, scheme):
    circ = case.circ
    proof, per_phase = case.fr_proof(scheme)
    adv = [case.av, case.bv, case.invv, case.eqv]
    assert sum(case.eqv) == len(case.same) and case.eqv[0] == 1 and case.eqv[circ.u - 1] == 1 and 0 < sum(case.eqv) < circ.u
    assert pv.check_witness(circ, adv, case.inst) is None
    assert pv.verify(circ, case.vk_points, case.vk_repr, case.inst, proof, pr.ec_mul(pr.G2_GEN, S_SECRET), multiopen=scheme)
    assert proof == pp.create_proof(circ, pp.Srs(circ.k, S_SECRET), adv, case.inst, case.vk_repr, SEED, scheme)


@pytest.mark.parametrize("scheme", ["gwc", "shplonk"])
def test_device_route_gives_the_same_bytes(zk, ctx, cref, case, scheme):
    circ = case.circ
    n, u = circ.n, circ.u
    want, _ = case.fr_proof(scheme)
    d_a = ctx.to_device(np.array(case.av[:u], dtype=np.uint64))                          # what a witness kernel left in HBM
    d_b = ctx.to_device(np.array(case.bv[:u], dtype=np.uint64))
    d_eq = ctx.to_device(np.array(case.eqv[:u], dtype=np.uint8))
    d_inv = ctx.to_device(np.zeros((n, 4), dtype=np.uint64))                            # rows from usable_rows on stay zero
    sess = case.session(scheme)
    try:
        ctx.row_inv0([d_a, d_b], [8, 8], cref.to_mont([1, R - 1]), u, d_inv)
        inv = cref.from_mont(d_inv.download((n, 4)))
        assert inv == case.invv and not any(inv[u:])
        assert len(sess.advice_phase_typed_dev({A: (d_a, 8), B: (d_b, 8), INV: (d_inv, 32), EQ: (d_eq, 1)})) == 0
        proof = sess.finish()
    except BaseException:
        sess.abort()
        raise
    finally:
        for buf in (d_a, d_b, d_eq, d_inv):
            buf.free()
    assert proof == want

"""GPU: the two lookup stages of zk_proof_finish with their fused path (ZK_LOOKUP_FUSED, default on): every recognised tuple of
the stage compressed by one launch (k_lk_compress_many), an argument's inputs counted by one launch, the denominators inverted out
of place and the running sums of a batch of arguments formed by one launch chain.  All of it is exact field arithmetic on
canonical values, so every proof here is compared byte for byte with the same session under ZK_LOOKUP_FUSED=0 and with the
oracle's big-int prover; the profiling scopes `lookup_compress_many` / `lookup_phi_fused` say which path ran, and the number of
`quotient_eval` launches says how many tuples went through a program of their own."""
import json
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from oracle import plonk_verifier as pv  # noqa: E402
from plonk_fixtures import build_evm_circuit, build_multi_lookup_circuit  # noqa: E402
from zkevm_circuits_amd import plonk  # noqa: E402

pytestmark = pytest.mark.gpu
S_SECRET = 0x5EC2E7
SEED = bytes(range(16))
R = plonk.R_MOD
FUSED_SCOPES = ("lookup_compress_many", "lookup_phi_fused")


class env:
    def __init__(self, kv): self.kv = kv
    def __enter__(self): os.environ.update(self.kv)
    def __exit__(self, *a):
        for k_ in self.kv:
            os.environ.pop(k_, None)


def tuples_of(circ):
    """compressions the multiplicities stage makes: every input tuple, and a table unless the argument before it has the same one"""
    count, prev = 0, None
    for lk in circ.lookups:
        ident = [circ.compile(e) for e in lk.table]
        count += len(lk.inputs) + (ident != prev)
        prev = ident
    return count


def prove(ctx, pk, adv, inst, knobs):
    """(proof, {scope: launches}) of one session under the knobs, profiling on"""
    with env(knobs):
        ctx.prof_enable(True)
        try:
            ctx.prof_reset()
            sess = ctx.proof_session(pk, [plonk.column_to_mont(c) for c in inst], SEED)
            sess.set_multiopen(1)
            sess.advice_phase({i: plonk.column_to_mont(c) for i, c in enumerate(adv)})
            proof = sess.finish()
            return proof, {name: ctx.prof_get(name)[1] for name in FUSED_SCOPES + ("quotient_eval",)}
        finally:
            ctx.prof_enable(False)


def check(ctx, cref, circ, adv, inst, declined=0, knobs=None):
    """fused == unfused == oracle; the scopes of the fused path recorded with it and only with it; `declined` tuples (of all the
    stage compresses) kept their own program under the fused path"""
    from oracle import plonk_prover as pp
    knobs = knobs or {}
    assert pv.check_witness(circ, adv, inst) is None
    srs = ctx.srs_setup_with_s(circ.k, cref.fr_const(S_SECRET))
    pk = ctx.pk_create(srs, circ.blob())
    try:
        _, rep = pk.vk(circ.F + len(circ.perm_cols))
        vk_repr = cref.from_mont(rep.reshape(1, 4))[0]
        fused, on = prove(ctx, pk, adv, inst, knobs)
        plain, off = prove(ctx, pk, adv, inst, dict(knobs, ZK_LOOKUP_FUSED="0"))
    finally:
        pk.destroy()
        srs.destroy()
    assert on["lookup_compress_many"] >= 1 and on["lookup_phi_fused"] >= 1, on
    assert off["lookup_compress_many"] == 0 and off["lookup_phi_fused"] == 0, off
    assert off["quotient_eval"] - on["quotient_eval"] == tuples_of(circ) - declined, (on, off)
    assert fused == plain
    want = pp.create_proof(circ, pp.Srs(circ.k, S_SECRET), adv, inst, vk_repr, SEED, "shplonk")
    first_diff = next((i for i, (x, y) in enumerate(zip(fused, want)) if x != y), None)
    assert len(fused) == len(want) and first_diff is None, f"proofs differ from byte {first_diff}"
    return on


def evm_with_wide_tuples(k):
    """build_evm_circuit's 4-column tuple and, beside it, a 6- and an 8-column tuple under the same q_lk and two arguments into
    ONE table, one behind the other (the second reads the first's compressed table and hash)"""
    circ, adv, inst = build_evm_circuit(k, seed=k, states=4, per_state=6)
    S = circ.A - 6
    q_lk, t_a, t_b, t_c = (circ.fixed_col(i) for i in (2, 3, 4, 5))
    a, b_, cc, a2, b2, c2 = (circ.advice_col(S + i) for i in range(6))
    for row in range(circ.u):
        if circ.fixed[2][row] == 1:                           # a lookup row: (a, b, c, a') hold (i, i^2 + 3, 7 i + 1, i); b', c' are free there
            adv[S + 4][row], adv[S + 5][row] = adv[S + 1][row], adv[S + 2][row]
    six = [t_a, t_b, t_c, t_a, t_b, t_c]
    circ.add_lookup([q_lk * x for x in (a, b_, cc, a2, b2, c2)], six)
    circ.add_lookup([q_lk * x for x in (a2, b2, c2, a, b_, cc)], six)          # the same table again
    circ.add_lookup([q_lk * x for x in (a, b_, cc, a2, b2, c2, a, b_)], six + [t_a, t_b])
    return circ, adv, inst


def test_one_segment_smaller_than_a_wave_batch(ctx, cref):
    """n = 64: less than one scan segment (2048 rows) and less than the 512 elements a wave inverts together"""
    circ, adv, inst = build_multi_lookup_circuit(6)
    check(ctx, cref, circ, adv, inst)


def test_degree_two_inputs_of_merged_arguments(ctx, cref):
    """`q x_i, q y_i` pairs, four of them merged and chunked by degree.  Each element is F * column with F one column read -- the
    shape the recogniser is specified to take, so these tuples ARE recognised (under the common factor q) and none falls back;
    the declined shapes are test_declined_tuples_keep_their_programs'."""
    circ, adv, inst = build_multi_lookup_circuit(6, n_inputs=4, input_degree=2, gate_degree=5)
    check(ctx, cref, circ, adv, inst)


def test_declined_tuples_keep_their_programs(ctx, cref):
    """tuples the recogniser declines -- an element that is a sum, a product of three reads -- run as programs of their own beside
    recognised ones of the same stage (a constant element, a rotated read, factors that differ between the elements)"""
    circ, adv, inst = build_multi_lookup_circuit(6, seed=3)
    q, t_a, t_b = (circ.fixed_col(i) for i in range(3))
    x0, y0, x1, y1 = (circ.advice_col(i) for i in range(4))
    circ.add_lookup([q * (x0 + x1 - x1), q * y0], [t_a, t_b])               # declined: a sum under the factor
    circ.add_lookup([q * x0 * q, y0 * q], [t_a, t_b])                       # declined: three reads under a product
    circ.add_lookup([x0 * q, q * y0, plonk.Const(5)], [t_a, t_b, plonk.Const(5)])      # recognised: the factor first and last, a constant element
    circ.add_lookup([x1, y1], [t_a.rot(1), t_b.rot(1)])                     # recognised: rotated reads (the table one row up; (0, 0) comes in from row u)
    check(ctx, cref, circ, adv, inst, declined=2)


def test_wide_tuples_under_a_common_factor_and_shared_tables(ctx, cref):
    circ, adv, inst = evm_with_wide_tuples(8)
    assert sorted(len(lk.inputs[0]) for lk in circ.lookups) == [4, 6, 6, 8]
    check(ctx, cref, circ, adv, inst)


def test_two_scan_segments_and_unusable_rows(ctx, cref):
    """k = 12: 4096 rows are two segments of the running sums (their totals scanned and added back), the last six rows unusable"""
    circ, adv, inst = build_multi_lookup_circuit(12, n_inputs=1)
    assert circ.u < circ.n == 4096
    check(ctx, cref, circ, adv, inst)


def test_several_inversion_batches_keep_a_table_with_its_sharer(ctx, cref):
    """ZK_LOOKUP_PHI_SLOTS=4: the four arguments need 2 + 2 + 1 + 2 slots (a table and one input each, the third sharing the
    second's table).  The first two fill the batch, the sharer stays with its owner beyond the cap, the fourth starts a new batch."""
    circ, adv, inst = evm_with_wide_tuples(8)
    on = check(ctx, cref, circ, adv, inst, knobs={"ZK_LOOKUP_PHI_SLOTS": "4"})
    assert on["lookup_phi_fused"] == 2


def test_single_input_arguments(ctx, cref):
    circ, adv, inst = build_multi_lookup_circuit(6, seed=4, n_inputs=1)
    assert all(len(lk.inputs) == 1 for lk in circ.lookups)
    check(ctx, cref, circ, adv, inst)


def test_arguments_into_one_table_that_are_not_neighbours(ctx, cref):
    """(pairs) (single) (pairs) (single): the fused path takes the arguments table by table, so the third and fourth read the
    compressed table, the hash and the inverted denominators of the first and second; commitments stay in argument order"""
    circ, adv, inst = build_multi_lookup_circuit(6, seed=6, n_inputs=1)
    t_a, t_b, t_c = (circ.fixed_col(i) for i in (1, 2, 3))
    tables = {len(lk.table): lk.table for lk in circ.lookups}
    first = len(circ.lookups[0].table)
    for width in (first, 3 - first):
        circ.add_lookup([circ.advice_col(0), circ.advice_col(1)] if width == 2 else [circ.advice_col(2)], tables[width])
    assert [len(lk.table) for lk in circ.lookups] == [first, 3 - first, first, 3 - first]
    check(ctx, cref, circ, adv, inst)


def test_input_missing_from_the_table_is_reported_alike(zk, ctx, cref):
    circ, adv, inst = build_multi_lookup_circuit(6, seed=2)
    bad = [list(col) for col in adv]
    row = 17
    bad[1][row] = (bad[1][row] + 1) % R                   # (x_0, y_0 + 1): in no table row
    srs = ctx.srs_setup_with_s(circ.k, cref.fr_const(S_SECRET))
    pk = ctx.pk_create(srs, circ.blob())
    try:
        errors = []
        for knobs in ({}, {"ZK_LOOKUP_FUSED": "0"}):
            with pytest.raises(zk.ZkError, match=f"input at row {row} is not in the table") as e:
                prove(ctx, pk, bad, inst, knobs)
            errors.append(str(e.value))
        assert errors[0] == errors[1]
    finally:
        pk.destroy()
        srs.destroy()


def test_two_ranks_share_the_arguments(ctx, cref, tmp_path):
    """a 2-rank session on one GPU (tests/test_gpu_sharded_proof.py's set-up) at k = 8, the arguments split over the ranks: each
    rank fuses its own arguments' stages; both ranks, either path and the unsharded session give the oracle prover's bytes"""
    from oracle import plonk_prover as pp
    from _launch import run_ranks
    res = run_ranks(2, os.path.join(HERE, "_lookup_stages_worker.py"), [tmp_path, 8], dict(os.environ, ZK_TEST_BACKEND="gloo", OMP_NUM_THREADS="1"))
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
    single = open(tmp_path / "proof_single.bin", "rb").read()
    for rank in range(2):
        for fused in ("1", "0"):
            assert open(tmp_path / f"proof_{rank}_{fused}.bin", "rb").read() == single, (rank, fused)
            scopes = json.load(open(tmp_path / f"scopes_{rank}_{fused}.json"))
            assert all((s in scopes) == (fused == "1") for s in FUSED_SCOPES), (rank, fused, scopes)
    circ, adv, inst = build_multi_lookup_circuit(8, seed=5, n_inputs=7, gate_degree=3)
    assert len(circ.lookups) >= 2
    srs = ctx.srs_setup_with_s(8, cref.fr_const(S_SECRET))
    pk = ctx.pk_create(srs, circ.blob())
    try:
        _, rep = pk.vk(circ.F + len(circ.perm_cols))
        vk_repr = cref.from_mont(rep.reshape(1, 4))[0]
    finally:
        pk.destroy()
        srs.destroy()
    assert single == pp.create_proof(circ, pp.Srs(8, S_SECRET), adv, inst, vk_repr, SEED, "shplonk")

"""GPU: the cosets of the columns as coset records (csrc/ff29.hip.hpp; written by the NTT's last pass and by k_powers, read by
k_quotient_eval2's record mode; csrc/prover.hip quotient_records).  ZK_QUOTIENT_RECORDS=0 keeps packed elements, and so does
ZK_QUOTIENT_KERNEL=1 (the older kernel has no record mode).

  * proofs are byte-equal between the default and ZK_QUOTIENT_RECORDS=0 on ONE key in one process, in both orders -- the key's coset
    cache outlives a session and has to change its format each time;
  * the same under the knobs that move coset buffers around: a forced additive split (the remainders' cosets), no cosets computed
    ahead, cosets computed beside the later stages, the key's cache running out of room, the older kernel, two sessions with their own blinding on one key;
  * every last-pass kernel writes records: k = 10 (single pass), 11 (two passes, run-time kernels), 14 (fixed instances 2^7 x 2^7),
    21 (three passes) -- one proof per k is checked by the oracle verifier.
"""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import pairing as pr  # noqa: E402
from oracle import plonk_verifier as pv  # noqa: E402
from plonk_fixtures import build_circuit, build_evm_circuit, build_multi_lookup_circuit, build_rotation_circuit  # noqa: E402
from zkevm_circuits_amd import plonk  # noqa: E402

pytestmark = pytest.mark.gpu
S_SECRET = 0x5EC2E7
PACKED = {"ZK_QUOTIENT_RECORDS": "0"}


class env:
    def __init__(self, *kvs):
        self.kv = {}
        for kv in kvs:
            self.kv.update(kv)

    def __enter__(self):
        os.environ.update(self.kv)

    def __exit__(self, *a):
        for name in self.kv:
            os.environ.pop(name, None)


@pytest.fixture(scope="module")
def srs_of(ctx, cref):
    made = {}

    def get(k):
        if k not in made:
            made[k] = ctx.srs_setup_with_s(k, cref.fr_const(S_SECRET))
        return made[k]
    yield get
    for s in made.values():
        s.destroy()


def session(ctx, pk, adv, inst, seed):
    sess = ctx.proof_session(pk, [plonk.column_to_mont(c) for c in inst], seed)
    sess.set_multiopen(1)
    return sess


def prove(ctx, pk, adv, inst, seed=bytes(range(7, 23))):
    sess = session(ctx, pk, adv, inst, seed)
    sess.advice_phase({i: plonk.column_to_mont(c) for i, c in enumerate(adv)})
    return sess.finish()


def accepted(cref, circ, pk, inst, proof):
    com, rep = pk.vk(circ.F + len(circ.perm_cols))
    return bool(pv.verify(circ, cref.affine_from_mont(com), cref.from_mont(rep.reshape(1, 4))[0], inst, proof, pr.ec_mul(pr.G2_GEN, S_SECRET), multiopen="shplonk"))


FIXTURES = {
    "circuit6": (lambda: build_circuit(6), {}),
    "rotation7": (lambda: build_rotation_circuit(7), {}),            # its rotations wrap
    "multi_lookup6": (lambda: build_multi_lookup_circuit(6), {}),
    "evm8": (lambda: build_evm_circuit(8, seed=8, states=12, per_state=24), {}),
    "evm8-slices4": (lambda: build_evm_circuit(8, seed=8, states=12, per_state=24), {"ZK_QUOTIENT_SLICES": "4"}),
    "evm8-one-class": (lambda: build_evm_circuit(8, seed=8, states=12, per_state=24), {"ZK_QUOTIENT_SPLIT": "0"}),
}


@pytest.mark.parametrize("name", list(FIXTURES))
def test_records_and_packed_cosets_give_the_same_proof_on_one_key(ctx, cref, srs_of, name):
    make, knobs = FIXTURES[name]
    circ, adv, inst = make()
    assert pv.check_witness(circ, adv, inst) is None
    pk = ctx.pk_create(srs_of(circ.k), circ.blob())
    try:
        with env(knobs):
            first = prove(ctx, pk, adv, inst)                    # records; fills the key's cache with records
            assert accepted(cref, circ, pk, inst, first)
            with env(PACKED):
                assert prove(ctx, pk, adv, inst) == first        # the cache is emptied and filled with packed cosets
                assert prove(ctx, pk, adv, inst) == first        # ... and read back
            assert prove(ctx, pk, adv, inst) == first            # and back to records
            assert prove(ctx, pk, adv, inst) == first
    finally:
        pk.destroy()
    pk = ctx.pk_create(srs_of(circ.k), circ.blob())               # the other order: a key whose first proof is the packed one
    try:
        with env(knobs):
            with env(PACKED):
                assert prove(ctx, pk, adv, inst) == first
            assert prove(ctx, pk, adv, inst) == first
            with env(PACKED):
                assert prove(ctx, pk, adv, inst) == first
    finally:
        pk.destroy()


def test_a_sliced_class_program_reads_records(ctx, cref, srs_of):
    """slices need 2^11 rows: the EVM-style fixture at k = 11, its large class cut in four (record operands, packed partial sums)"""
    circ, adv, inst = build_evm_circuit(11, seed=8, states=12, per_state=24)
    pk = ctx.pk_create(srs_of(circ.k), circ.blob())
    try:
        with env({"ZK_QUOTIENT_SLICES": "4"}):
            proof = prove(ctx, pk, adv, inst)
            with env(PACKED):
                assert prove(ctx, pk, adv, inst) == proof
        with env({"ZK_QUOTIENT_SLICES": "0"}):
            assert prove(ctx, pk, adv, inst) == proof
        assert accepted(cref, circ, pk, inst, proof)
    finally:
        pk.destroy()


KNOBS = {
    "additive-split": {"ZK_QUOTIENT_COSTGATE": "0"},                # the remainders of the split constraints are read on their cosets
    "none-ahead": {"ZK_ADVICE_COSET_GB": "0"},
    "late": {"ZK_ADVICE_COSET_LATE_GB": "1"},
    "cache-runs-out": {"ZK_PK_COSET_CACHE_FAIL_AFTER": "3"},
    "older-kernel": {"ZK_QUOTIENT_KERNEL": "1"},                    # falls back to packed buffers
}


@pytest.mark.parametrize("knob", list(KNOBS))
def test_the_knobs_that_move_coset_buffers(ctx, cref, srs_of, knob):
    circ, adv, inst = build_circuit(6, seed=3)
    want_pk = ctx.pk_create(srs_of(circ.k), circ.blob())
    try:
        with env(PACKED):
            want = prove(ctx, want_pk, adv, inst)
    finally:
        want_pk.destroy()
    with env(KNOBS[knob]):
        pk = ctx.pk_create(srs_of(circ.k), circ.blob())
        try:
            if knob == "additive-split":
                assert pk.quotient_plan()["remainders"] > 0
            assert prove(ctx, pk, adv, inst) == want
            assert prove(ctx, pk, adv, inst) == want              # the second proof finds what the first cached
            with env(PACKED):
                assert prove(ctx, pk, adv, inst) == want
            assert prove(ctx, pk, adv, inst) == want
        finally:
            pk.destroy()


def test_two_sessions_on_one_key(ctx, cref, srs_of):
    circ, adv, inst = build_circuit(6, seed=4)
    pk = ctx.pk_create(srs_of(circ.k), circ.blob())
    try:
        seed_a, seed_b = bytes(range(16)), bytes(range(1, 17))
        with env(PACKED):
            want_a, want_b = prove(ctx, pk, adv, inst, seed_a), prove(ctx, pk, adv, inst, seed_b)
        assert want_a != want_b
        assert prove(ctx, pk, adv, inst, seed_a) == want_a        # this session turns the key's cache into records and fills it
        assert prove(ctx, pk, adv, inst, seed_b) == want_b        # this one only reads it
    finally:
        pk.destroy()


@pytest.mark.parametrize("k", [10, 11, 14])
def test_every_last_pass_kernel_writes_records(ctx, cref, srs_of, k):
    circ, adv, inst = build_circuit(k, seed=k)
    pk = ctx.pk_create(srs_of(k), circ.blob())
    try:
        proof = prove(ctx, pk, adv, inst)
        with env(PACKED):
            assert prove(ctx, pk, adv, inst) == proof
        assert accepted(cref, circ, pk, inst, proof)
    finally:
        pk.destroy()


def test_three_pass_transforms_write_records(ctx, cref):
    """k = 21: the smallest fixture's structure with its witness built by numpy (bench_proof.build_large)"""
    import bench_proof as bp
    k = 21
    circ, blob, adv_m, inst_m, inst = bp.build_large(ctx, k, 1)
    npub = [int(np.flatnonzero(np.asarray(a).reshape(-1, 4).any(axis=1))[-1]) + 1 if np.asarray(a).any() else 0 for a in inst_m]
    inst = [list(col[:m]) for col, m in zip(inst, npub)]
    inst_m = [np.ascontiguousarray(a[:m]) for a, m in zip(inst_m, npub)]
    srs = ctx.srs_setup_with_s(k, cref.fr_const(S_SECRET))
    pk = ctx.pk_create(srs, blob)
    del blob
    try:
        def run():
            sess = ctx.proof_session(pk, inst_m, bytes(16), instance_slices=True)
            sess.set_multiopen(1)
            sess.advice_phase({i: c for i, c in enumerate(adv_m)})
            return sess.finish()
        proof = run()
        with env(PACKED):
            assert run() == proof
        assert accepted(cref, circ, pk, inst, proof)
    finally:
        pk.destroy()
        srs.destroy()

"""CPU: the verifying key object (zk_vk_create / zk_vk_proof_len / zk_vk_shape) -- host only, built from the constraint-system
part of a key blob by the same parser zk_pk_create uses.  The proof length it derives must be the length of what the prover
writes: the reference's own ChunkProof (k = 25, Poseidon, SHPLONK: 896 bytes) and the oracle prover's proofs of the suite's
circuits under every transcript kind and multi-open scheme."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import zkevm_circuits_amd as z  # noqa: E402
from oracle import cref, plonk_prover as pp, plonk_verifier as pv  # noqa: E402
from plonk_fixtures import build_circuit, build_evm_circuit, build_multi_lookup_circuit, build_rotation_circuit  # noqa: E402
from test_reference_chunk_proof import fx, halo2_circuit_of  # noqa: E402,F401  (fx: the fixture of the reference's proof)

TRANSCRIPTS = [(z.TRANSCRIPT_BLAKE2B, "blake2b"), (z.TRANSCRIPT_POSEIDON, "poseidon"), (z.TRANSCRIPT_EVM, "evm")]
MULTIOPEN = [(0, "gwc"), (1, "shplonk")]
CIRCUITS = {
    "plain": lambda: build_circuit(5, seed=3, wide=True),
    "rotation": lambda: build_rotation_circuit(6, seed=2),
    "multi_lookup": lambda: build_multi_lookup_circuit(5, seed=4, n_inputs=3, input_degree=2, gate_degree=4),
    "evm": lambda: build_evm_circuit(7, seed=5),
}


def _vk(circ, commitments=None, vk_repr=1):
    com = cref.affine_to_mont(commitments) if commitments is not None else np.zeros((circ.F + len(circ.perm_cols), 8), np.uint64)
    return z.VerifyingKey(circ.cs_blob(), com, cref.to_mont([vk_repr]).reshape(4))


def test_reference_chunk_proof_key_at_k25(fx):  # noqa: F811
    circ = halo2_circuit_of(fx.protocol)
    vk = _vk(circ, fx.protocol.preprocessed, fx.protocol.transcript_initial_state)
    try:
        sh = vk.shape()
        assert (sh["k"], sh["F"], sh["P"], sh["A"], sh["I"], sh["L"]) == (25, 4, 3, 1, 1, 1)
        assert vk.proof_len(z.TRANSCRIPT_POSEIDON, 1) == 896 == len(fx.proof)
        assert vk.proof_len(z.TRANSCRIPT_EVM, 1) > 896
    finally:
        vk.destroy()


@pytest.mark.parametrize("name", sorted(CIRCUITS))
def test_proof_len_equals_the_oracle_provers_proof(name):
    circ, adv, inst = CIRCUITS[name]()
    srs = pp.Srs(circ.k, 0x1234)
    vk = _vk(circ)
    try:
        for kind, tname in TRANSCRIPTS:
            for mo, mname in MULTIOPEN:
                proof = pp.create_proof(circ, srs, adv, inst, 7, bytes(16), mname, transcript=tname)
                assert vk.proof_len(kind, mo) == len(proof), (tname, mname)
    finally:
        vk.destroy()


def test_shape_from_the_constraint_system_alone():
    circ, _, _ = build_circuit(5, seed=3, wide=True)
    vk = _vk(circ)
    try:
        sh = vk.shape()
        assert (sh["k"], sh["degree"], sh["F"], sh["A"], sh["I"], sh["P"], sh["L"]) == (5, circ.degree(), circ.F, circ.A, circ.I, len(circ.perm_cols), 1)
        assert sh["advice_queries"] == len(circ.advice_queries) and sh["fixed_queries"] == len(circ.fixed_queries)
    finally:
        vk.destroy()


def test_truncated_or_garbled_blobs_are_refused():
    lib = z.lib()
    circ, _, _ = build_circuit(5, seed=3, wide=True)
    blob = circ.cs_blob()
    ncom = circ.F + len(circ.perm_cols)
    com = np.zeros((ncom, 8), np.uint64)
    rep = np.zeros(4, np.uint64)

    def create(data, ncommitments=ncom):
        buf = np.frombuffer(bytes(data), dtype=np.uint8).copy() if len(data) else np.zeros(1, np.uint8)
        h = ctypes.c_void_p()
        rc = lib.zk_vk_create(buf.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(len(data)), com.ctypes.data_as(ctypes.c_void_p),
                              ctypes.c_size_t(ncommitments), rep.ctypes.data_as(ctypes.c_void_p), ctypes.byref(h))
        if rc == 0:
            lib.zk_vk_destroy(h)
        return rc

    assert create(blob) == 0
    for cut in (0, 4, 8, 40, len(blob) // 3, len(blob) // 2, len(blob) - 12, len(blob) - 1):
        assert create(blob[:cut]) == -1, cut
    assert create(blob + bytes(32)) == -1                     # trailing bytes: not a constraint-system part
    assert create(blob, ncom - 1) == -1                       # F + P commitments expected
    bad_magic = bytearray(blob)
    bad_magic[0] ^= 1
    assert create(bad_magic) == -1
    huge_k = bytearray(blob)
    huge_k[8:12] = (28).to_bytes(4, "little")
    assert create(huge_k) == -1
    # a deterministic sweep of garbled words: refused or accepted, never a crash
    rng = np.random.default_rng(7)
    for _ in range(200):
        g = bytearray(blob)
        pos = int(rng.integers(0, len(blob) // 4)) * 4
        g[pos:pos + 4] = int(rng.integers(0, 1 << 32)).to_bytes(4, "little")
        assert create(g) in (0, -1)
    # a commitment off the curve is refused
    off = np.zeros((ncom, 8), np.uint64)
    off[0, 0] = 1
    h = ctypes.c_void_p()
    buf = np.frombuffer(blob, dtype=np.uint8).copy()
    assert lib.zk_vk_create(buf.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(len(blob)), off.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(ncom),
                            rep.ctypes.data_as(ctypes.c_void_p), ctypes.byref(h)) == -1


def test_default_repr_matches_the_oracle_on_a_shape_only_key():
    """a verifying key needs no column data: the oracle's default vk_repr is a function of cs_blob and the commitments alone"""
    circ, _, _ = build_circuit(5, seed=3, wide=True)
    srs = pp.Srs(circ.k, 0x1234)
    points = pp.vk_commitments(circ, srs)
    rep = pv.default_vk_repr(circ, points)
    vk = _vk(circ, points, rep)
    try:
        assert vk.proof_len(z.TRANSCRIPT_BLAKE2B, 0) == len(pp.create_proof(circ, srs, *build_circuit(5, seed=3, wide=True)[1:], rep, bytes(16), "gwc"))
    finally:
        vk.destroy()

"""GPU: key blob version 4 (typed fixed cells, sigma columns built on the device from halo2's permutation mapping) against the
untouched version 3 path of the same circuit.  The version 3 columns come from plonk.py's big-int `sigma_columns()`, which shares
nothing with the device code: the two keys must have the same commitments and `transcript_repr`, write the same proofs, report
the same MockProver failures, and a malformed version 4 blob must be refused with a status and a message."""
import os
import random
import struct
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from oracle import pairing as pr  # noqa: E402
from oracle import plonk_verifier as pv  # noqa: E402
from plonk_fixtures import build_circuit, build_evm_circuit  # noqa: E402
from test_blob_v4 import widths_circuit  # noqa: E402
from test_gpu_cpp_caller import _dump, exe  # noqa: E402,F401  (exe: the compiled examples/prove_from_files.cpp)
from zkevm_circuits_amd import plonk  # noqa: E402

pytestmark = pytest.mark.gpu
R = plonk.R_MOD
S_SECRET = 0x5EC2E7
FX, AD, IN = plonk.FIXED, plonk.ADVICE, plonk.INSTANCE


@pytest.fixture(scope="module")
def srs_by_k(ctx, cref):
    class PerK(dict):
        def __missing__(self, k):
            self[k] = ctx.srs_setup_with_s(k, cref.fr_const(S_SECRET))
            return self[k]
    cache = PerK()
    yield cache
    for s in cache.values():
        s.destroy()


def _tie(circ, a, b):
    """a copy constraint on any row (Circuit.copy keeps to the usable rows; key generation has no such limit)"""
    for c in (a, b):
        circ.enable_equality(c[0], c[1])
    circ.copies.append((a, b))


def corners_circuit():
    """k = 5: a cycle through a fixed, an advice and an instance column; a cycle through row 0 and row n - 1; advice column 1 as
    ONE cycle, so that no cell of it maps to its own row"""
    c = plonk.Circuit(5, num_fixed=2, num_advice=2, num_instance=1)
    n = c.n
    c.fixed[0][4], c.fixed[1][9] = 77, R - 2
    _tie(c, (FX, 0, 4), (AD, 0, 11))
    _tie(c, (AD, 0, 11), (IN, 0, 2))
    _tie(c, (IN, 0, 2), (AD, 0, 30))
    _tie(c, (AD, 0, 0), (AD, 0, n - 1))
    _tie(c, (IN, 0, n - 1), (FX, 0, 0))
    for i in range(n - 1):
        _tie(c, (AD, 1, i), (AD, 1, i + 1))
    assert all(i2 != i for i, (_, i2) in enumerate(c.permutation_mapping()[c.perm_cols.index((AD, 1))]))
    return c


def one_column_circuit():
    """P = 1: a single permutation column, wholly one cycle"""
    c = plonk.Circuit(5, num_fixed=1, num_advice=1, num_instance=0)
    for i in range(c.n - 1):
        _tie(c, (AD, 0, (i * 7) % c.n), (AD, 0, (i * 7 + 7) % c.n))
    assert len(c.perm_cols) == 1
    return c


def no_permutation_circuit():
    c = plonk.Circuit(5, num_fixed=2, num_advice=1, num_instance=0)
    c.fixed[0] = [i % 2 for i in range(c.n)]
    c.fixed[1][3] = R - 5
    c.add_gate(c.fixed_col(0) * c.advice_col(0) * c.fixed_col(1))
    return c


def no_fixed_circuit():
    c = plonk.Circuit(5, num_fixed=0, num_advice=2, num_instance=1)
    _tie(c, (AD, 0, 1), (AD, 1, 2))
    _tie(c, (AD, 1, 2), (IN, 0, 0))
    _tie(c, (AD, 0, 31), (AD, 0, 0))
    return c


def random_copies_circuit(k, fixed, perm_fixed, advice, copies, seed):
    """the first `perm_fixed` fixed columns and every advice column in the permutation, `copies` random copy constraints over all
    of them and all rows"""
    rng = random.Random(seed)
    c = plonk.Circuit(k, num_fixed=fixed, num_advice=advice, num_instance=0)
    cols = [(FX, i) for i in range(perm_fixed)] + [(AD, i) for i in range(advice)]
    for i in range(fixed):
        for _ in range(4):
            c.fixed[i][rng.randrange(c.n)] = rng.randrange(1 << rng.choice((1, 8, 16, 60, 120, 254))) % R
    for col in cols:
        c.enable_equality(*col)
    for _ in range(copies):
        _tie(c, rng.choice(cols) + (rng.randrange(c.n),), rng.choice(cols) + (rng.randrange(c.n),))
    return c


KEY_CIRCUITS = {
    "wide_k6": lambda: build_circuit(6, seed=3, wide=True)[0],
    "wide_k8": lambda: build_circuit(8, seed=4, wide=True)[0],
    "evm_k7": lambda: build_evm_circuit(7, seed=5)[0],
    "corners_k5": corners_circuit,
    "one_column": one_column_circuit,
    "no_permutation": no_permutation_circuit,
    "no_fixed": no_fixed_circuit,
    "seventeen_each": lambda: random_copies_circuit(5, 17, 0, 17, 60, seed=8),     # F = 17, P = 17: one past the 16-column launch group, both kinds
    "k13_twenty_columns": lambda: random_copies_circuit(13, 2, 2, 18, 3000, seed=9),  # 32 workgroups per column, j' over all 20 columns
    "widths": widths_circuit,
}


def _key_bytes(ctx, srs, circ, blob):
    pk = ctx.pk_create(srs, blob)
    try:
        com, rep = pk.vk(circ.F + len(circ.perm_cols))
        return com.tobytes(), rep.tobytes(), pk.shape()
    finally:
        pk.destroy()


@pytest.mark.parametrize("name", sorted(KEY_CIRCUITS))
def test_v4_key_equals_v3_key(ctx, srs_by_k, name):
    circ = KEY_CIRCUITS[name]()
    srs = srs_by_k[circ.k]
    want = _key_bytes(ctx, srs, circ, circ.blob())
    got = _key_bytes(ctx, srs, circ, circ.blob(version=4))
    assert got[2] == want[2]                      # zk_pk_shape
    assert got[0] == want[0]                      # all F + P commitments
    assert got[1] == want[1]                      # transcript_repr
    if name == "widths":
        assert plonk.Circuit.blob_v4_parts(circ.blob(version=4))[0] == [1, 2, 4, 8, 16, 32, 1]
    if name == "k13_twenty_columns":
        mapping = circ.permutation_mapping()
        assert len(mapping) == 20 and {j2 for col in mapping for j2, _ in col} == set(range(20))


def _session_proof(ctx, pk, adv, inst, seed, multiopen):
    sess = ctx.proof_session(pk, [plonk.column_to_mont(c) for c in inst], seed)
    sess.set_multiopen(1 if multiopen == "shplonk" else 0)
    sess.advice_phase({i: plonk.column_to_mont(c) for i, c in enumerate(adv)})
    return sess.finish()


@pytest.mark.parametrize("shape,multiopen", [("wide_k6", "gwc"), ("wide_k6", "shplonk"), ("evm_k7", "gwc"), ("evm_k7", "shplonk")])
def test_v4_key_writes_the_v3_keys_proof(ctx, cref, srs_by_k, shape, multiopen):
    circ, adv, inst = build_circuit(6, seed=3, wide=True) if shape == "wide_k6" else build_evm_circuit(7, seed=5)
    seed = bytes((7 * i + 3) & 0xFF for i in range(16))
    proofs = []
    for version in (3, 4):
        pk = ctx.pk_create(srs_by_k[circ.k], circ.blob(version=version))
        try:
            com, rep = pk.vk(circ.F + len(circ.perm_cols))
            proofs.append(_session_proof(ctx, pk, adv, inst, seed, multiopen))
        finally:
            pk.destroy()
    assert proofs[1] == proofs[0]
    s_g2 = pr.ec_mul(pr.G2_GEN, S_SECRET)
    assert pv.verify(circ, cref.affine_from_mont(com), cref.from_mont(rep.reshape(1, 4))[0], inst, proofs[1], s_g2, multiopen=multiopen)


def test_mock_verify_reports_a_broken_copy_under_both_keys(ctx, srs_by_k):
    circ, adv, inst = build_circuit(6, seed=7, wide=True)
    a = next(c[0] for c in circ.copies if c[0][0] == AD)
    bad = [list(col) for col in adv]
    bad[a[1]][a[2]] = (bad[a[1]][a[2]] + 1) % R
    want = pv.mock_failures(circ, bad, inst)
    assert any(f[0] == pv.MOCK_PERMUTATION for f in want)
    reports = []
    for version in (3, 4):
        pk = ctx.pk_create(srs_by_k[circ.k], circ.blob(version=version))
        try:
            assert ctx.mock_verify(pk, [plonk.column_to_mont(c) for c in adv], [plonk.column_to_mont(c) for c in inst]) == ([], 0)
            reports.append(ctx.mock_verify(pk, [plonk.column_to_mont(c) for c in bad], [plonk.column_to_mont(c) for c in inst]))
        finally:
            pk.destroy()
    assert reports[1] == reports[0] == (want, len(want))


def test_malformed_v4_blobs_are_refused_and_the_context_goes_on(zk, ctx, srs_by_k):
    circ = build_circuit(6, seed=3, wide=True)[0]
    srs = srs_by_k[circ.k]
    blob = circ.blob(version=4)
    good = _key_bytes(ctx, srs, circ, blob)
    cs_len, n, P = plonk.Circuit.cs_blob_len(blob), circ.n, len(circ.perm_cols)
    map_at = len(blob) - 8 * P * n

    def patched(at, word):
        b = bytearray(blob)
        b[at:at + 4] = struct.pack("<I", word)
        return bytes(b)

    cases = [
        ("cell width", patched(cs_len + 4 * 2, 3)),                                 # width 3
        ("cell width", patched(cs_len, 64)),
        ("out of range", patched(map_at + 8 * (n + 5), P)),                         # j' = P in column 1
        ("out of range", patched(map_at + 8 * ((P - 1) * n + n - 1) + 4, n)),       # i' = n in the last cell of the last column
        ("out of range", patched(map_at + 4, 0xFFFFFFFF)),
        ("truncated|exceed the blob", blob[:-1]),                                                   # one byte short
        ("truncated|exceed the blob", blob[:map_at + 8]),
        ("truncated|exceed the blob", blob[:cs_len + 4 * circ.F + 5]),
        ("truncated|exceed the blob", blob[:cs_len + 6]),                                                    # inside the width table
        ("version", patched(4, 5)),
        ("version", patched(4, 2)),
    ]
    for message, bad in cases:
        with pytest.raises(zk.ZkError, match=message):
            ctx.pk_create(srs, bad)
        assert _key_bytes(ctx, srs, circ, blob) == good                             # the context still makes the good key


def test_cpp_caller_writes_the_same_proof_from_a_v4_blob_file(zk, ctx, cref, exe, tmp_path):  # noqa: F811
    circ, adv, inst = build_circuit(6, 2, True)
    srs = _dump(zk, ctx, cref, str(tmp_path), circ, adv, inst, 77, bytes(range(16)))
    srs.destroy()
    proofs = []
    for version in (3, 4):
        open(tmp_path / "blob.bin", "wb").write(circ.blob(version=version))
        res = subprocess.run([exe, str(tmp_path), "shplonk"], capture_output=True, text=True, timeout=300)
        assert res.returncode == 0 and "mock checks passed" in res.stdout, res.stdout + res.stderr
        proofs.append(open(tmp_path / "proof_cpp.bin", "rb").read())
        os.remove(tmp_path / "proof_cpp.bin")
    assert proofs[1] == proofs[0] and len(proofs[0]) > 0

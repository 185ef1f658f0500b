"""GPU: the library's own halo2 verify_proof (zk_verify_proofs; KZG with GWC / SHPLONK, Blake2b / Poseidon / EVM transcripts).
  * one parser: the shape zk_vk_create derives from cs_blob() is zk_pk_shape of the key zk_pk_create builds from the full blob;
  * the reference's own ChunkProof (k = 25, Poseidon, SHPLONK) is accepted, and every single-bit flip the oracle tests flip is
    rejected;
  * on the prover's matrix (circuits, schemes, transcripts, vanishing kinds, three phases) every GPU proof is accepted and the
    native verdict equals oracle/plonk_verifier.verify's on the proof and on a fixed set of mutations;
  * AccumulatorStrategy: a batch of 8 proofs of one key in one call, any one of them mutated, a batch of 1, two keys in one call;
  * the EVM-style k = 20 proof; a C++ caller through include/zkmi355_halo2.hpp."""
import os
import random
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import zkevm_circuits_amd as z  # noqa: E402
from oracle import bn254 as b  # noqa: E402
from oracle import pairing as pr  # noqa: E402
from oracle import params_file  # noqa: E402
from oracle import plonk_verifier as pv  # noqa: E402
from plonk_fixtures import build_circuit, build_evm_circuit, build_multi_lookup_circuit, build_rotation_circuit  # noqa: E402
from test_reference_chunk_proof import fx, halo2_circuit_of  # noqa: E402,F401
from zkevm_circuits_amd import plonk  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S_SECRET = 0x5EC2E7
R = b.R_MOD
KIND = {"blake2b": z.TRANSCRIPT_BLAKE2B, "poseidon": z.TRANSCRIPT_POSEIDON, "evm": z.TRANSCRIPT_EVM}
MO = {"gwc": 0, "shplonk": 1}
VANISH = {"one": 1, "uniform": 0}
G2 = params_file.g2_raw_bytes(pr.G2_GEN)


@pytest.fixture(scope="module")
def s_g2():
    return pr.ec_mul(pr.G2_GEN, S_SECRET)


@pytest.fixture(scope="module")
def srs(ctx, cref):
    class PerK(dict):
        def __missing__(self, k):
            self[k] = ctx.srs_setup_with_s(k, cref.fr_const(S_SECRET))
            return self[k]
    cache = PerK()
    yield cache
    for s_ in cache.values():
        s_.destroy()


def _mont_cols(cols):
    return [plonk.column_to_mont(c) for c in cols]


def three_phase(k=6, seed=5):
    """The SuperCircuit's phase structure (tests/test_gpu_proof.py has the commentary): challenges after phases 0 and 1, advice
    in all three, a third-phase lookup into a second-phase column.  Fixed columns depend on k only, so every seed gives a
    witness of the same key.  Returns (circuit, synth(phase, challenges) -> {column: values}, instance)."""
    circ = plonk.Circuit(k, num_fixed=3, num_advice=7, num_instance=1, blinding_factors=5)
    q, q5, ql = circ.fixed_col(0), circ.fixed_col(1), circ.fixed_col(2)
    a, b_, w, kk, t, s_, lk = (circ.advice_col(i) for i in range(7))
    circ.advice_phase = [0, 0, 1, 1, 2, 2, 2]
    evm_word, keccak_input = circ.challenge_usable_after(0), circ.challenge_usable_after(0)
    lookup_input = circ.challenge_usable_after(1)
    circ.add_gate(q * (a + evm_word * b_ - w))
    circ.add_gate(q * (b_ + keccak_input * a - kk))
    circ.add_gate(q * (w + lookup_input * kk - t))
    circ.add_gate(q5 * (t * t * lookup_input - s_.rot(1) * w))
    circ.lookup_any("lk in w", [ql * lk], [w])
    circ.chunk_lookups()
    n, u = circ.n, circ.u
    for row in range(u):
        circ.fixed[0][row] = 1
    for row in range(0, u - 3, 2):
        circ.fixed[1][row] = 1
    picks = [(3 * j + 1, (7 * j + 2) % (u - 1)) for j in range(6)]
    for row, src in picks:
        circ.fixed[2][row] = 1
        circ.copy((plonk.ADVICE, 6, row), (plonk.ADVICE, 2, src))
    circ.copy((plonk.ADVICE, 0, 0), (plonk.INSTANCE, 0, 0))
    rng = random.Random(seed)
    av = [rng.randrange(1, R) if i < u - 1 else 0 for i in range(n)]
    bv = [rng.randrange(1, R) if i < u - 1 else 0 for i in range(n)]

    def synth(phase, ch):
        if phase == 0:
            return {0: av, 1: bv}
        wv = [(av[i] + ch[0] * bv[i]) % R if i < u else 0 for i in range(n)]
        kv = [(bv[i] + ch[1] * av[i]) % R if i < u else 0 for i in range(n)]
        if phase == 1:
            return {2: wv, 3: kv}
        tv = [(wv[i] + ch[2] * kv[i]) % R if i < u else 0 for i in range(n)]
        sv, lv = [0] * n, [0] * n
        for row in range(u):
            if circ.fixed[1][row]:
                sv[row + 1] = tv[row] * tv[row] % R * ch[2] % R * b.fr_inv(wv[row]) % R
        for row, src in picks:
            lv[row] = wv[src]
        return {4: tv, 5: sv, 6: lv}
    return circ, synth, [[av[0]] + [0] * (n - 1)]


def _prove(ctx, cref, pk, circ, adv_or_synth, inst, seed, multiopen, transcript, vanishing):
    sess = ctx.proof_session(pk, _mont_cols(inst), seed)
    sess.set_transcript_kind(KIND[transcript])
    sess.set_multiopen(MO[multiopen])
    sess.set_vanishing_random(VANISH[vanishing])
    if callable(adv_or_synth):
        ch = []
        for ph in range(3):
            got = sess.advice_phase({i: plonk.column_to_mont(c) for i, c in adv_or_synth(ph, ch).items()})
            ch += cref.from_mont(got)
    else:
        sess.advice_phase({i: plonk.column_to_mont(c) for i, c in enumerate(adv_or_synth)})
    return sess.finish()


def _oracle(circ, vk_points, vk_repr, inst, proof, s_g2, multiopen, transcript):
    try:
        return bool(pv.verify(circ, vk_points, vk_repr, inst, proof, s_g2, multiopen=multiopen, transcript=transcript))
    except (AssertionError, ValueError, KeyError, IndexError):
        return False


def _native(ctx, vk, inst, proofs, s_g2, multiopen, transcript):
    if isinstance(proofs, (bytes, bytearray)):
        proofs, inst = [bytes(proofs)], [inst]
    return ctx.verify_proofs(vk, proofs, [_mont_cols(i) for i in inst], KIND[transcript], MO[multiopen], G2, params_file.g2_raw_bytes(s_g2))


CIRCUITS = {
    "plain": lambda: build_circuit(5, seed=3, wide=True),
    "rotation": lambda: build_rotation_circuit(6, seed=2),
    "multi_lookup": lambda: build_multi_lookup_circuit(5, seed=4, n_inputs=3, input_degree=2, gate_degree=4),
    "evm": lambda: build_evm_circuit(6, seed=6, states=6, per_state=16),
    "three_phase": lambda: three_phase(6, 5),
}


# ------------------------------------------------------------------------------------ one parser
@pytest.mark.parametrize("name", sorted(CIRCUITS))
def test_vk_shape_equals_the_proving_keys(ctx, srs, name):
    circ = CIRCUITS[name]()[0]
    pk = ctx.pk_create(srs[circ.k], circ.blob())
    try:
        com, rep = pk.vk(circ.F + len(circ.perm_cols))
        want = pk.shape()
        for blob in (circ.cs_blob(), circ.blob()):
            vk = z.VerifyingKey(blob, com, rep)
            assert vk.shape() == want
            vk.destroy()
        vk = z.VerifyingKey.from_pk(pk, circ.cs_blob())
        assert vk.shape() == want
        vk.destroy()
    finally:
        pk.destroy()


# ------------------------------------------------------------------------------------ the reference's proof
def test_reference_chunk_proof_is_accepted_and_bit_flips_rejected(ctx, cref, fx):  # noqa: F811
    circ = halo2_circuit_of(fx.protocol)
    vk = z.VerifyingKey(circ.cs_blob(), cref.affine_to_mont(fx.protocol.preprocessed), cref.to_mont([fx.protocol.transcript_initial_state]).reshape(4))
    s_g2 = params_file.g2_raw_bytes(fx.s_g2)
    inst = [cref.to_mont(list(col)) for col in fx.instances]

    def verify(proof, instances):
        return ctx.verify_proofs(vk, [proof], [instances], z.TRANSCRIPT_POSEIDON, 1, G2, s_g2)
    assert verify(fx.proof, inst)
    for word in [0, 1, 2, 4, 5, 9, 13, 17, 21, 25, 26, 27]:
        bad = bytearray(fx.proof)
        bad[32 * word + 3] ^= 0x10
        assert not verify(bytes(bad), inst), word
    for cell in [0, 11, 12, 43]:
        ins = [list(fx.instances[0])]
        ins[0][cell] ^= 1
        assert not verify(fx.proof, [cref.to_mont(ins[0])]), cell
    # the wrong SRS, the GWC reading of a SHPLONK proof, another transcript: rejected
    assert not ctx.verify_proofs(vk, [fx.proof], [inst], z.TRANSCRIPT_POSEIDON, 1, G2, params_file.g2_raw_bytes(pr.ec_mul(pr.G2_GEN, 1234)))
    assert not ctx.verify_proofs(vk, [fx.proof], [inst], z.TRANSCRIPT_POSEIDON, 0, G2, s_g2)
    assert not ctx.verify_proofs(vk, [fx.proof], [inst], z.TRANSCRIPT_BLAKE2B, 1, G2, s_g2)
    vk.destroy()


# ------------------------------------------------------------------------------------ agreement with the oracle verifier
MATRIX = [
    ("plain", "gwc", "blake2b", "one"), ("plain", "shplonk", "blake2b", "uniform"), ("plain", "shplonk", "poseidon", "one"),
    ("plain", "gwc", "poseidon", "uniform"), ("plain", "shplonk", "evm", "uniform"), ("plain", "gwc", "evm", "one"),
    ("rotation", "gwc", "blake2b", "one"), ("rotation", "shplonk", "poseidon", "uniform"),
    ("multi_lookup", "shplonk", "blake2b", "one"), ("multi_lookup", "gwc", "evm", "uniform"),
    ("evm", "gwc", "blake2b", "uniform"), ("evm", "shplonk", "poseidon", "one"),
    ("three_phase", "shplonk", "blake2b", "one"), ("three_phase", "gwc", "evm", "uniform"),
]


@pytest.mark.parametrize("name,multiopen,transcript,vanishing", MATRIX)
def test_native_verdicts_equal_the_oracles(ctx, cref, srs, s_g2, name, multiopen, transcript, vanishing):
    circ, adv, inst = CIRCUITS[name]()
    pk = ctx.pk_create(srs[circ.k], circ.blob())
    try:
        com, rep = pk.vk(circ.F + len(circ.perm_cols))
        proof = _prove(ctx, cref, pk, circ, adv, inst, bytes(range(7, 23)), multiopen, transcript, vanishing)
        other = _prove(ctx, cref, pk, circ, adv, inst, bytes(range(7, 23)), "gwc" if multiopen == "shplonk" else "shplonk", transcript, vanishing)
    finally:
        pk.destroy()
    vk_points, vk_repr = cref.affine_from_mont(com), cref.from_mont(rep.reshape(1, 4))[0]
    vk = z.VerifyingKey(circ.cs_blob(), com, rep)
    wrong_vk = z.VerifyingKey(circ.cs_blob(), com, cref.to_mont([(vk_repr + 1) % R]).reshape(4))
    assert vk.proof_len(KIND[transcript], MO[multiopen]) == len(proof)
    try:
        assert _native(ctx, vk, inst, proof, s_g2, multiopen, transcript)
        assert _oracle(circ, vk_points, vk_repr, inst, proof, s_g2, multiopen, transcript)
        plen = 64 if transcript == "evm" else 32
        first_scalar = vk.shape()["commitments"] * plen
        cases = {
            "point bit": (bytes(proof[:3]) + bytes([proof[3] ^ 0x10]) + proof[4:], inst, vk, vk_repr, multiopen),
            "scalar bit": (proof[:first_scalar + 1] + bytes([proof[first_scalar + 1] ^ 0x04]) + proof[first_scalar + 2:], inst, vk, vk_repr, multiopen),
            "short": (proof[:-32], inst, vk, vk_repr, multiopen),
            "wrong repr": (proof, inst, wrong_vk, (vk_repr + 1) % R, multiopen),
            "other scheme": (other, inst, vk, vk_repr, multiopen),
            "checked as the other scheme": (proof, inst, vk, vk_repr, "gwc" if multiopen == "shplonk" else "shplonk"),
        }
        if inst:
            cases["instance value"] = (proof, [[(inst[0][0] + 1) % R] + list(inst[0][1:])] + [list(c) for c in inst[1:]], vk, vk_repr, multiopen)
        for what, (p_, ins, key, rep_int, mo) in cases.items():
            native = _native(ctx, key, ins, p_, s_g2, mo, transcript)
            oracle = _oracle(circ, vk_points, rep_int, ins, p_, s_g2, mo, transcript)
            assert native == oracle, (what, native, oracle)
            assert not native, what
    finally:
        vk.destroy()
        wrong_vk.destroy()


# ------------------------------------------------------------------------------------ AccumulatorStrategy
@pytest.fixture(scope="module")
def batch8(ctx, cref, srs):
    """8 proofs of the three-phase key: different witnesses (seeds 1..8), different blinding seeds; SHPLONK, Poseidon"""
    circ, _, _ = three_phase(6, 1)
    pk = ctx.pk_create(srs[circ.k], circ.blob())
    proofs, insts = [], []
    try:
        com, rep = pk.vk(circ.F + len(circ.perm_cols))
        for s_ in range(1, 9):
            c2, synth, inst = three_phase(6, s_)
            proofs.append(_prove(ctx, cref, pk, c2, synth, inst, bytes([s_] * 16), "shplonk", "poseidon", "one"))
            insts.append(inst)
    finally:
        pk.destroy()
    vk = z.VerifyingKey(circ.cs_blob(), com, rep)
    yield circ, vk, proofs, insts
    vk.destroy()


def test_batch_of_8_is_accepted_in_one_call(ctx, s_g2, batch8):
    circ, vk, proofs, insts = batch8
    assert len(set(proofs)) == 8
    assert _native(ctx, vk, insts, proofs, s_g2, "shplonk", "poseidon")
    # a batch of 1 gives the single call's verdict
    for i in (0, 5):
        assert _native(ctx, vk, [insts[i]], [proofs[i]], s_g2, "shplonk", "poseidon") == _native(ctx, vk, insts[i], proofs[i], s_g2, "shplonk", "poseidon") is True


@pytest.mark.parametrize("which,pos", [(0, 3), (3, 200), (7, -1), (5, 32 * 9 + 1), (2, -40)])
def test_batch_with_one_mutated_proof_is_rejected(ctx, s_g2, batch8, which, pos):
    circ, vk, proofs, insts = batch8
    bad = [bytearray(p_) for p_ in proofs]
    bad[which][pos] ^= 0x02
    bad = [bytes(p_) for p_ in bad]
    assert not _native(ctx, vk, insts, bad, s_g2, "shplonk", "poseidon")
    assert not _native(ctx, vk, insts[which], bad[which], s_g2, "shplonk", "poseidon")


def test_batch_with_a_mutated_instance_is_rejected(ctx, s_g2, batch8):
    circ, vk, proofs, insts = batch8
    ins = [[list(c) for c in i] for i in insts]
    ins[4][0][0] = (ins[4][0][0] + 1) % R
    assert not _native(ctx, vk, ins, proofs, s_g2, "shplonk", "poseidon")


def test_proofs_of_two_keys_in_one_call_are_rejected(ctx, cref, srs, s_g2):
    """same shape, different fixed columns (build_circuit's layout follows its seed): a proof of key B in a batch verified under
    key A is rejected (zkmi355.h: rejected, never accepted), and so is the batch verified under key B"""
    keys, proofs, insts = [], [], []
    for seed in (2, 3):
        circ, adv, inst = build_circuit(5, seed=seed, wide=True)
        pk = ctx.pk_create(srs[circ.k], circ.blob())
        try:
            com, rep = pk.vk(circ.F + len(circ.perm_cols))
            keys.append(z.VerifyingKey(circ.cs_blob(), com, rep))
            for s_ in range(2):
                proofs.append(_prove(ctx, cref, pk, circ, adv, inst, bytes([s_ + 1] * 16), "gwc", "blake2b", "one"))
                insts.append(inst)
        finally:
            pk.destroy()
    try:
        assert keys[0].shape() == keys[1].shape()
        assert _native(ctx, keys[0], insts[:2], proofs[:2], s_g2, "gwc", "blake2b")
        assert _native(ctx, keys[1], insts[2:], proofs[2:], s_g2, "gwc", "blake2b")
        for key in keys:
            assert not _native(ctx, key, insts, proofs, s_g2, "gwc", "blake2b")
    finally:
        for k_ in keys:
            k_.destroy()


def test_bad_arguments_are_refused(ctx, batch8, s_g2):
    circ, vk, proofs, insts = batch8
    with pytest.raises(z.ZkError):
        ctx.verify_proofs(vk, proofs[:1], [[]], z.TRANSCRIPT_POSEIDON, 1, G2, params_file.g2_raw_bytes(s_g2))       # wrong instance column count
    with pytest.raises(z.ZkError):
        ctx.verify_proofs(vk, proofs[:1], [_mont_cols(insts[0])], 7, 1, G2, params_file.g2_raw_bytes(s_g2))          # unknown transcript kind
    # too many instance values for the usable rows: a reject, not an error
    long = [list(insts[0][0][:circ.u]) + [1]]
    assert not ctx.verify_proofs(vk, proofs[:1], [_mont_cols(long)], z.TRANSCRIPT_POSEIDON, 1, G2, params_file.g2_raw_bytes(s_g2))


# ------------------------------------------------------------------------------------ size
def test_evm_style_k20_proof_is_accepted(ctx, cref):
    from test_gpu_headline_config import require_host_memory
    require_host_memory(64)
    import bench_proof as bp
    shape = (20, 1000, 150, 150, 100, 9)
    circ, blob, adv_m, inst_m, inst, rlc = bp.build_shape(ctx, *shape, dist="survey", phases=True, evm=dict(bp.EVM_DEFAULT))
    npub = [int(np.flatnonzero(np.asarray(a).reshape(-1, 4).any(axis=1))[-1]) + 1 if np.asarray(a).any() else 0 for a in inst_m]
    inst_m = [np.ascontiguousarray(a[:m]) for a, m in zip(inst_m, npub)]
    s_ = ctx.srs_setup_with_s(circ.k, cref.fr_const(S_SECRET))
    pk = ctx.pk_create(s_, blob)
    del blob
    adv_dev = [ctx.to_device(a) for a in adv_m]
    driver = bp.PhaseDriver(ctx, circ, adv_dev, rlc)
    try:
        com, rep = pk.vk(circ.F + len(circ.perm_cols))
        sess = ctx.proof_session(pk, inst_m, bytes(16), instance_slices=True)
        sess.set_multiopen(1)
        driver.run(sess)
        proof = sess.finish()
    finally:
        driver.free()
        for b_ in adv_dev:
            b_.free()
        pk.destroy()
        s_.destroy()
    vk = z.VerifyingKey(circ.cs_blob(), com, rep)
    s_g2 = params_file.g2_raw_bytes(pr.ec_mul(pr.G2_GEN, S_SECRET))
    try:
        assert ctx.verify_proofs(vk, [proof], [inst_m], z.TRANSCRIPT_BLAKE2B, 1, G2, s_g2)
        bad = bytearray(proof)
        bad[len(bad) // 3] ^= 4
        assert not ctx.verify_proofs(vk, [bytes(bad)], [inst_m], z.TRANSCRIPT_BLAKE2B, 1, G2, s_g2)
    finally:
        vk.destroy()


# ------------------------------------------------------------------------------------ C++
CPP_VERIFY = r'''
#include "zkmi355_halo2.hpp"
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iterator>
#include <string>
using namespace zk::halo2;
static std::vector<uint8_t> slurp(const std::string& p) {
    std::ifstream f(p, std::ios::binary);
    if (!f) throw std::runtime_error("cannot read " + p);
    return std::vector<uint8_t>((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}
int main(int argc, char** argv) {
    const std::string dir = argv[1];
    const bool shplonk = std::string(argv[2]) == "shplonk";
    try {
        Context ctx(0);
        ParamsKZG params = ParamsKZG::read_custom(ctx, slurp(dir + "/params.bin"), ParamsKZG::SerdeFormat::RawBytesUnchecked);
        const std::vector<uint8_t> blob = slurp(dir + "/blob.bin"), repr_b = slurp(dir + "/repr.bin");
        Fr repr;
        std::memcpy(repr.data(), repr_b.data(), 32);
        ProvingKey pk(ctx, params, blob);
        pk.set_transcript_repr(repr);
        VerifyingKey vk = VerifyingKey::from_pk(ctx, pk, blob);
        uint32_t shape[16];
        if (zk_vk_shape(vk.raw(), shape)) return 5;
        const size_t n = size_t(1) << shape[0], I = shape[5], usable = n - shape[11] - 1;
        const std::vector<uint8_t> instance = slurp(dir + "/instance.bin");
        std::vector<std::vector<Fr>> inst(I, std::vector<Fr>(usable));
        for (size_t c = 0; c < I; ++c) std::memcpy(inst[c].data(), instance.data() + c * n * 32, usable * 32);
        std::vector<uint8_t> proof = slurp(dir + "/proof_cpp.bin");
        const bool ok = verify_proof(ctx, vk, {proof}, {inst}, ZK_TRANSCRIPT_BLAKE2B, shplonk, params.g2(), params.s_g2());
        proof[proof.size() / 2] ^= 1;
        const bool bad = verify_proof(ctx, vk, {proof}, {inst}, ZK_TRANSCRIPT_BLAKE2B, shplonk, params.g2(), params.s_g2());
        std::printf("len %zu/%zu verify %d tampered %d\n", proof.size(), vk.proof_len(ZK_TRANSCRIPT_BLAKE2B, shplonk), (int)ok, (int)bad);
        return 0;
    } catch (const std::exception& e) {
        std::printf("error: %s\n", e.what());
        return 3;
    }
}
'''


@pytest.mark.parametrize("multiopen", ["shplonk", "gwc"])
def test_cpp_caller_verifies_what_prove_from_files_wrote(zk, ctx, cref, tmp_path, multiopen):
    libdir = os.path.dirname(zk.binding.LIB_PATH)
    flags = ["-L", libdir, "-lzkmi355", f"-Wl,-rpath,{libdir}", "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"]
    prover, verifier = tmp_path / "prove_from_files", tmp_path / "verify_from_files"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "prove_from_files.cpp"), "-o", str(prover)] + flags)
    src = tmp_path / "verify_from_files.cpp"
    src.write_text(CPP_VERIFY)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(verifier)] + flags)
    circ, adv, inst = build_circuit(6, 2, True)
    d = tmp_path / "files"
    d.mkdir()
    s_ = ctx.srs_setup_with_s(circ.k, cref.fr_const(S_SECRET))
    try:
        g2, s_g2 = zk.binding.g2_setup(cref.fr_const(S_SECRET))
        (d / "params.bin").write_bytes(bytes(ctx.params_write(s_, g2, s_g2, 2)))
    finally:
        s_.destroy()
    (d / "blob.bin").write_bytes(circ.blob())
    (d / "advice.bin").write_bytes(b"".join(plonk.column_to_mont(c).tobytes() for c in adv))
    (d / "instance.bin").write_bytes(b"".join(plonk.column_to_mont(c).tobytes() for c in inst))
    (d / "repr.bin").write_bytes(plonk.fr_mont_bytes(12345))
    (d / "seed.bin").write_bytes(bytes(range(16)))
    res = subprocess.run([str(prover), str(d), multiopen], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    res = subprocess.run([str(verifier), str(d), multiopen], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    n = len((d / "proof_cpp.bin").read_bytes())
    assert f"len {n}/{n} verify 1 tampered 0" in res.stdout, res.stdout

"""GPU: one proof over the columns of a SHA-256 table in its dev_load form, one row per message -- phase 0: enable (1-byte cells) and
input_len, which is the 4-byte d_lens buffer of the call itself; ONE challenge after phase 0 (the reference takes both RLCs of the
SHA256Table under keccak_input, zkevm-circuits/src/table.rs:1657-1662); phase 1: input_rlc and output_rlc, both made on the device
by ONE ZK_OP_SHA256 from the message bytes, with that challenge as r_out and as r_in, and handed to zk_proof_advice_phase_dev.
The gates pin the empty message's row and the row of "abc" to the digests the reference holds
(sha256_circuit/circuit.rs:1198-1227, tests/golden/sha256_reference.json) in Horner form in the challenge, the input_rlc of "abc" to
0x61 r^2 + 0x62 r + 0x63, and the one-byte message's input_rlc to a public byte, so a wrong hash column fails check_witness.  That
route yields the challenge and the proof bytes of the route on which every column is made from Python integers, which the oracle
verifier accepts and which equal the oracle prover's; both multi-open schemes."""
import os
import random
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import sha256_cases as sc  # noqa: E402
from oracle import bn254 as b  # noqa: E402
from oracle import pairing as pr  # noqa: E402
from oracle import plonk_prover as pp  # noqa: E402
from oracle import plonk_verifier as pv  # noqa: E402
from test_gpu_proof_typed import S_SECRET, SEED, Case  # noqa: E402
from zkevm_circuits_amd import plonk  # noqa: E402

pytestmark = pytest.mark.gpu
R = b.R_MOD
ENABLE, INPUT_LEN, INPUT_RLC, OUTPUT_RLC = range(4)                    # advice columns
EMPTY_ROW, BYTE_ROW, ABC_ROW = 0, 1, 2


def horner_in(challenge, data):
    """sum_k data[k] challenge^(len-1-k) as an expression in the challenge"""
    h = plonk.wrap(data[0])
    for byte in data[1:]:
        h = h * challenge + byte
    return h


def sha256_table_circuit(k):
    """q selects the usable rows, q_0 the row of the empty message, q_1 the row of "abc":
      q enable (enable - 1),
      q_0 input_rlc,   q_0 input_len,   q_0 (output_rlc - H_nil(r)),
      q_1 (output_rlc - H_abc(r)),   q_1 (input_rlc - (0x61 r^2 + 0x62 r + 0x63)),
    H_nil and H_abc the Horner forms of the reference-held digests in the ONE challenge r.  input_rlc of the one-byte message's row
    is copied to an instance cell that holds the byte."""
    circ = plonk.Circuit(k, num_fixed=3, num_advice=4, num_instance=1, blinding_factors=5)
    q, q0, q1 = circ.fixed_col(0), circ.fixed_col(1), circ.fixed_col(2)
    enable, input_len, input_rlc, output_rlc = (circ.advice_col(i) for i in range(4))
    circ.advice_phase = [0, 0, 1, 1]
    r = circ.challenge_usable_after(0)
    vectors = sc.reference_vectors()
    circ.add_gate(q * enable * (enable - 1))
    circ.add_gate(q0 * input_rlc)
    circ.add_gate(q0 * input_len)
    circ.add_gate(q0 * (output_rlc - horner_in(r, vectors["empty"][1])))
    circ.add_gate(q1 * (output_rlc - horner_in(r, vectors["abc"][1])))
    circ.add_gate(q1 * (input_rlc - horner_in(r, b"abc")))
    for row in range(circ.u):
        circ.fixed[0][row] = 1
    circ.fixed[1][EMPTY_ROW] = 1
    circ.fixed[2][ABC_ROW] = 1
    circ.copy((plonk.ADVICE, INPUT_RLC, BYTE_ROW), (plonk.INSTANCE, 0, 0))
    return circ


def table_messages(circ):
    """the empty message, one byte, abc, the lengths around the padding boundary and one block, a few random ones; then off rows
    (enable 0, length 0, an offset outside the bytes, so that they write zeros and not the digest of the empty message) up to
    usable_rows"""
    rng = random.Random(26)
    messages = [b"", bytes([rng.randrange(1, 256)]), b"abc"] + [bytes(rng.randrange(256) for _ in range(size)) for size in (55, 56, 63, 64, 65, 31, 119, 200, 333, 500)]
    data, offs = bytearray(), []
    for m in messages:
        data += bytes(rng.randrange(256) for _ in range(rng.randrange(4)))
        offs.append(len(data))
        data += m
    rows = len(messages)
    assert rows < circ.u
    off_rows = circ.u - rows
    return dict(messages=messages, data=bytes(data), offs=offs + [len(data) + 1 + i for i in range(off_rows)], lens=[len(m) for m in messages] + [0] * off_rows,
                enable=[1] * rows + [0] * off_rows, rows=rows)


def phase1(raw, n, r):
    """input_rlc and output_rlc as integers, both under the one challenge r"""
    _, out, inp = sc.expected(raw["messages"], r, r)
    pad = lambda col: list(col) + [0] * (n - len(col))
    return pad(inp), pad(out)


@pytest.fixture(scope="module")
def case(ctx, cref):
    circ = sha256_table_circuit(6)
    raw = table_messages(circ)
    n = circ.n
    pad = lambda col: list(col) + [0] * (n - len(col))

    def synth(phase, ch):
        if phase == 0:
            return {ENABLE: pad(raw["enable"]), INPUT_LEN: pad(raw["lens"])}
        inp, out = phase1(raw, n, ch[0])
        return {INPUT_RLC: inp, OUTPUT_RLC: out}
    c = Case(ctx, cref, circ, synth, [[raw["messages"][BYTE_ROW][0]] + [0] * (n - 1)])
    c.raw = raw
    yield c
    c.close()


@pytest.mark.parametrize("scheme", ["gwc", "shplonk"])
def test_host_route_is_accepted_and_equals_the_oracle_prover(case, scheme):
    circ = case.circ
    proof, per_phase = case.fr_proof(scheme)
    assert [len(c) for c in per_phase] == [1, 0]                       # ONE challenge after phase 0
    ch = case.cref.from_mont(per_phase[0])
    adv = [case.synth(0, [])[ENABLE], case.synth(0, [])[INPUT_LEN], *phase1(case.raw, circ.n, ch[0])]
    vectors = sc.reference_vectors()
    assert adv[OUTPUT_RLC][EMPTY_ROW] == sc.horner(vectors["empty"][1], ch[0]) and adv[OUTPUT_RLC][ABC_ROW] == sc.horner(vectors["abc"][1], ch[0])
    assert adv[INPUT_RLC][ABC_ROW] == (0x61 * ch[0] * ch[0] + 0x62 * ch[0] + 0x63) % R and adv[INPUT_RLC][BYTE_ROW] == case.raw["messages"][BYTE_ROW][0]
    assert pv.check_witness(circ, adv, case.inst, challenges=ch) is None
    for col, row in ((OUTPUT_RLC, EMPTY_ROW), (INPUT_RLC, EMPTY_ROW), (INPUT_LEN, EMPTY_ROW), (OUTPUT_RLC, ABC_ROW), (INPUT_RLC, ABC_ROW), (INPUT_RLC, BYTE_ROW), (ENABLE, 3)):
        wrong = [list(c) for c in adv]
        wrong[col][row] = (wrong[col][row] + 2) % R
        assert pv.check_witness(circ, wrong, case.inst, challenges=ch) is not None, (col, row)
    assert pv.verify(circ, case.vk_points, case.vk_repr, case.inst, proof, pr.ec_mul(pr.G2_GEN, S_SECRET), multiopen=scheme)
    assert proof == pp.create_proof(circ, pp.Srs(circ.k, S_SECRET), adv, case.inst, case.vk_repr, SEED, scheme)


@pytest.mark.parametrize("scheme", ["gwc", "shplonk"])
def test_device_route_gives_the_same_challenges_and_bytes(zk, ctx, cref, case, scheme):
    circ, raw = case.circ, case.raw
    n, u = circ.n, circ.u
    want, want_ch = case.fr_proof(scheme)
    d_bytes = ctx.to_device(np.frombuffer(b"\xEE" + raw["data"], dtype=np.uint8))       # what a witness kernel left in HBM, at an odd address
    d_offs = ctx.to_device(np.array(raw["offs"], dtype=np.uint32))
    d_lens = ctx.to_device(np.array(raw["lens"], dtype=np.uint32))                      # the call's lengths ARE the input_len column
    d_enable = ctx.to_device(np.array(raw["enable"], dtype=np.uint8))
    d_in, d_out = (ctx.to_device(np.zeros((n, 4), dtype=np.uint64)) for _ in range(2))  # rows from usable_rows on stay zero
    sess = case.session(scheme)
    try:
        got = sess.advice_phase_typed_dev({ENABLE: (d_enable, 1), INPUT_LEN: (d_lens, 4)})
        assert np.array_equal(got, want_ch[0]) and len(got) == 1
        ctx.sha256(d_bytes.ptr + 1, len(raw["data"]), d_offs, d_lens, 4, u, d_out, got[0], r_in=got[0], input_rlc=d_in)        # the ONE call
        inp, out = phase1(raw, n, cref.from_mont(got)[0])
        assert cref.from_mont(d_in.download((n, 4))) == inp and cref.from_mont(d_out.download((n, 4))) == out
        assert len(sess.advice_phase_dev({INPUT_RLC: d_in, OUTPUT_RLC: d_out})) == 0
        proof = sess.finish()
    except BaseException:
        sess.abort()
        raise
    finally:
        for buf in (d_bytes, d_offs, d_lens, d_enable, d_in, d_out):
            buf.free()
    assert proof == want

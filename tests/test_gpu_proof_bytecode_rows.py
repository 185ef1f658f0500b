"""GPU: one proof at k = 7 over the gates of the bytecode circuit (bytecode_circuit/circuit.rs:143-460), every advice column made on
the device from code bytes: ZK_OP_BYTECODE_ROWS (tag, index, value, is_code, push_data_left, push_data_size, length, the code hash and
the two kind columns), ZK_OP_ROW_INV0 twice (push_data_left_inv; index_length_diff_inv over index + 1 - length), and, under the two
challenges squeezed after the first phase, ZK_OP_SCAN_RLC for value_rlc (kinds = tag) and push_acc, ZK_OP_SCAN_RLC_REV for push_rlc;
zk_proof_advice_phase_typed_dev takes the typed buffers as they stand.  The gates: the two IsZero gadgets, first and last row, tag
boolean, header row, byte row (is_code == push_data_left_is_zero, push_acc 0 on code), header to header, header to byte, byte to byte
(length, index, hash, value_rlc, push_data_left, the push_rlc copy-forward and the push_acc accumulation), last byte, byte to header,
and the lookup of (value, push_data_size) into a fixed table that holds the byte values these bytecodes use (256 rows do not fit).
The code hash is the Poseidon build's: a first-phase cell per bytecode, the constant of the empty code on padding.  The bytecodes
include an empty one, a truncated PUSH32, a push at the very end and push data that holds push opcodes.  That route yields the proof
bytes of the route on which every column comes from the Python model, which the oracle verifier accepts and which equal the oracle
prover's; both multi-open schemes.  One changed cell in any column fails check_witness."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import bytecode_rows_cases as bc  # noqa: E402
from oracle import bn254 as b  # noqa: E402
from oracle import pairing as pr  # noqa: E402
from oracle import plonk_prover as pp  # noqa: E402
from oracle import plonk_verifier as pv  # noqa: E402
from test_gpu_proof_typed import S_SECRET, SEED, Case  # noqa: E402
from zkevm_circuits_amd import plonk  # noqa: E402

pytestmark = pytest.mark.gpu
R = b.R_MOD
TAG, INDEX, VALUE, IS_CODE, LEFT, SIZE, LENGTH, HASH, LEFT_INV, DIFF_INV, VALUE_RLC, PUSH_ACC, PUSH_RLC, ADVICE = range(14)
NAMES = {TAG: "tag", INDEX: "index", VALUE: "value", IS_CODE: "is_code", LEFT: "push_data_left", SIZE: "push_data_size", LENGTH: "length", HASH: "code_hash",
         LEFT_INV: "push_data_left_inv", DIFF_INV: "index_length_diff_inv", VALUE_RLC: "value_rlc", PUSH_ACC: "push_acc", PUSH_RLC: "push_rlc"}
WIDTHS = {TAG: 1, INDEX: 4, VALUE: 4, IS_CODE: 1, LEFT: 1, SIZE: 1, LENGTH: 4}
Q_ENABLE, Q_FIRST, Q_LAST, T_VALUE, T_SIZE = range(5)
EMPTY_HASH = 0x2098f5fb9e239eab3ceac3f27b81e481dc3124d55ffed523a839ee8446b64864   # POSEIDON_CODE_HASH_EMPTY (tests/golden/poseidon_code_hash.json)
CODES = [
    bytes([0x61, 0x60, 0x7f, 0x01, 0x60, 0x05, 0x00]),                  # PUSH2 whose data are push opcodes, ADD, PUSH1, STOP
    b"",
    bytes([0x5b, 0x7f]) + bytes([0x7f, 0x60, 0x61] * 10 + [0x11, 0x22]) + bytes([0x02]),   # a full PUSH32 of push opcodes, then code
    bytes([0x01, 0x7f, 0xaa, 0xbb, 0x60]),                              # PUSH32 cut by the end after three bytes
    bytes([0x60]),                                                      # a push at the very end: no data row
    bytes([0x62, 0x01, 0x02, 0x03, 0x00]),
]
HASHES = [(0x1111 * (i + 3)) ** 9 % R if code else EMPTY_HASH for i, code in enumerate(CODES)]   # the gates pin the hash of the empty code


def bytecode_circuit(k):
    circ = plonk.Circuit(k, num_fixed=5, num_advice=ADVICE, num_instance=1, blinding_factors=5)
    circ.advice_phase = [0] * 10 + [1] * 3
    keccak_input, evm_word = circ.challenge_usable_after(0), circ.challenge_usable_after(0)
    q, q_first, q_last = (circ.fixed_col(i) for i in (Q_ENABLE, Q_FIRST, Q_LAST))
    a = lambda col, rot=0: circ.advice_col(col, rot)
    tag, index, value, is_code, left, size, length, code_hash = (a(c) for c in (TAG, INDEX, VALUE, IS_CODE, LEFT, SIZE, LENGTH, HASH))
    value_rlc, push_acc, push_rlc = a(VALUE_RLC), a(PUSH_ACC), a(PUSH_RLC)
    nxt = lambda col: a(col, 1)
    not_last = 1 - q_last
    # :145-160 the IsZero gadgets
    left_is_zero = 1 - left * a(LEFT_INV)
    diff = index + 1 - length
    diff_is_zero = 1 - diff * a(DIFF_INV)
    circ.add_gate(q * left * left_is_zero)
    circ.add_gate(q * diff * diff_is_zero)
    # :165-192 first and last row, tag boolean
    circ.add_gate(q * (q_first + q_last - q_first * q_last) * tag)
    circ.add_gate(q * tag * (tag - 1))
    # :197-216 header row
    header = q * not_last * (1 - tag)
    circ.add_gate(header * index)
    circ.add_gate(header * (value - length))
    # :221-264 byte row and the push table
    byte = q * not_last * tag
    circ.add_gate(byte * (is_code - left_is_zero))
    circ.add_gate(byte * is_code * push_acc)
    circ.add_lookup([byte * value, byte * size], [circ.fixed_col(T_VALUE), circ.fixed_col(T_SIZE)])
    # :269-299 header to header, or the last row
    h2h = (1 - tag) * (1 - nxt(TAG))
    pad = q * (h2h + q_last - h2h * q_last)
    circ.add_gate(pad * length)
    circ.add_gate(pad * (code_hash - EMPTY_HASH))
    # :307-344 header to byte
    h2b = q * not_last * (1 - tag) * nxt(TAG)
    circ.add_gate(h2b * (nxt(LENGTH) - length))
    circ.add_gate(h2b * nxt(INDEX))
    circ.add_gate(h2b * (nxt(IS_CODE) - 1))
    circ.add_gate(h2b * (nxt(HASH) - code_hash))
    circ.add_gate(h2b * (nxt(VALUE_RLC) - nxt(VALUE)))
    # :355-424 byte to byte
    b2b = q * not_last * tag * nxt(TAG)
    circ.add_gate(b2b * (nxt(LENGTH) - length))
    circ.add_gate(b2b * (nxt(INDEX) - index - 1))
    circ.add_gate(b2b * (nxt(HASH) - code_hash))
    circ.add_gate(b2b * (nxt(VALUE_RLC) - (value_rlc * keccak_input + nxt(VALUE))))
    circ.add_gate(b2b * (nxt(LEFT) - (is_code * size + (1 - is_code) * (left - 1))))
    circ.add_gate(b2b * (push_rlc - (nxt(IS_CODE) * push_acc + (1 - nxt(IS_CODE)) * nxt(PUSH_RLC))))
    circ.add_gate(b2b * (1 - nxt(IS_CODE)) * (nxt(PUSH_ACC) - (push_acc * evm_word + nxt(VALUE))))
    # :428-441 the last byte is followed by a header
    circ.add_gate(q * tag * diff_is_zero * nxt(TAG))
    # :446-462 byte to header
    b2h = q * not_last * tag * (1 - nxt(TAG))
    circ.add_gate(b2h * (index + 1 - length))
    circ.add_gate(b2h * (push_rlc - push_acc))
    for row in range(circ.u):
        circ.fixed[Q_ENABLE][row] = 1
    circ.fixed[Q_FIRST][0] = 1
    circ.fixed[Q_LAST][circ.u - 1] = 1
    used = sorted({v for code in CODES for v in code})
    assert len(used) + 1 <= circ.u
    for row, v in enumerate(used, 1):                                   # row 0 stays (0, 0): what a row that is no byte row looks up
        circ.fixed[T_VALUE][row], circ.fixed[T_SIZE][row] = v, bc.get_push_size(v)
    circ.copy((plonk.ADVICE, VALUE, 0), (plonk.INSTANCE, 0, 0))
    return circ


def model_columns(circ, ch):
    """every advice column from the Python model: u rows of the assignment loop, zeros behind them"""
    keccak_input, evm_word = ch if ch else (0, 0)
    m = bc.assign(CODES, HASHES, circ.u, EMPTY_HASH, evm_word=evm_word, keccak_input=keccak_input)
    return {col: m[name] + [0] * (circ.n - circ.u) for col, name in NAMES.items()}


@pytest.fixture(scope="module")
def case(ctx, cref):
    circ = bytecode_circuit(7)
    assert sum(len(c) + 1 for c in CODES) < circ.u                       # the last usable row is a padding row

    def synth(phase, ch):
        cols = model_columns(circ, ch)
        return {col: v for col, v in cols.items() if circ.advice_phase[col] == phase}
    c = Case(ctx, cref, circ, synth, [[len(CODES[0])] + [0] * (circ.n - 1)])
    yield c
    c.close()


@pytest.mark.parametrize("scheme", ["gwc", "shplonk"])
def test_host_route_is_accepted_and_equals_the_oracle_prover(case, scheme):
    circ = case.circ
    proof, per_phase = case.fr_proof(scheme)
    assert [len(c) for c in per_phase] == [2, 0]
    ch = case.cref.from_mont(per_phase[0])
    cols = model_columns(circ, ch)
    adv = [cols[col] for col in range(ADVICE)]
    assert set(adv[LEFT]) >= {0, 1, 2, 32} and set(bc.assign(CODES, HASHES, circ.u, EMPTY_HASH)["rlc_kinds"]) == {0, 1, 2}
    assert any(v >= 1 << 128 for v in adv[PUSH_RLC]) and any(v >= 1 << 128 for v in adv[VALUE_RLC]), "a challenge reached no cell"
    assert pv.check_witness(circ, adv, case.inst, challenges=ch) is None
    row = 2                                                             # index 1 of the first code: push data, push_data_left 2
    assert adv[TAG][row] == 1 and adv[LEFT][row] == 2 and adv[IS_CODE][row] == 0
    for col in range(ADVICE):
        wrong = [list(c) for c in adv]
        wrong[col][row] = (wrong[col][row] + 2) % R
        assert pv.check_witness(circ, wrong, case.inst, challenges=ch) is not None, NAMES[col]
    assert pv.verify(circ, case.vk_points, case.vk_repr, case.inst, proof, pr.ec_mul(pr.G2_GEN, S_SECRET), multiopen=scheme)
    assert proof == pp.create_proof(circ, pp.Srs(circ.k, S_SECRET), adv, case.inst, case.vk_repr, SEED, scheme)


@pytest.mark.parametrize("scheme", ["gwc", "shplonk"])
def test_device_route_gives_the_same_challenges_and_bytes(ctx, cref, case, scheme):
    circ = case.circ
    n, u = circ.n, circ.u
    want, want_ch = case.fr_proof(scheme)
    buf, offs, lens = bc.lay_out(CODES, gap=1)                           # what the block's code database left in HBM
    d_bytes, d_offs, d_lens = ctx.to_device(buf), ctx.to_device(np.array(offs, dtype=np.uint32)), ctx.to_device(np.array(lens, dtype=np.uint32))
    d_hashes = ctx.to_device(bc.to_mont(HASHES))
    typed = {col: ctx.to_device(np.zeros(n * w, dtype=np.uint8)) for col, w in WIDTHS.items()}       # rows from usable_rows on stay zero
    d_acc_kinds, d_rlc_kinds = (ctx.to_device(np.zeros(n, dtype=np.uint8)) for _ in range(2))
    fr = {col: ctx.to_device(np.zeros((n, 4), dtype=np.uint64)) for col in (HASH, LEFT_INV, DIFF_INV, VALUE_RLC, PUSH_ACC, PUSH_RLC)}
    one, zero, minus_one = cref.fr_const(1)[0], cref.fr_const(0)[0], cref.fr_const(R - 1)[0]
    sess = case.session(scheme)
    try:
        # phase 1 of the reference's numbering: nothing here depends on a challenge
        ctx.bytecode_rows(d_bytes, len(buf), d_offs, d_lens, 4, len(CODES), u, fr[HASH], bc.to_mont([EMPTY_HASH])[0], hashes=d_hashes, tag=typed[TAG], index=typed[INDEX],
                          value=typed[VALUE], is_code=typed[IS_CODE], push_data_left=typed[LEFT], push_data_size=typed[SIZE], length=typed[LENGTH],
                          acc_kinds=d_acc_kinds, rlc_kinds=d_rlc_kinds)
        ctx.row_inv0([typed[LEFT]], [1], [one], u, fr[LEFT_INV])
        ctx.row_inv0([typed[INDEX], typed[LENGTH]], [4, 4], [one, minus_one], u, fr[DIFF_INV], constant=one)
        columns = {col: (typed[col], w) for col, w in WIDTHS.items()}
        columns.update({col: (fr[col], 32) for col in (HASH, LEFT_INV, DIFF_INV)})
        got = sess.advice_phase_typed_dev(columns)
        assert np.array_equal(got, want_ch[0])
        keccak_input, evm_word = got[0], got[1]
        # phase 2: the three RLC columns
        ctx.scan_rlc(typed[VALUE], 4, typed[TAG], np.array([(zero, zero), (keccak_input, one), (zero, zero), (zero, zero)], dtype=np.uint64), u, fr[VALUE_RLC])
        ctx.scan_rlc(typed[VALUE], 4, d_acc_kinds, np.array([(zero, zero), (evm_word, one), (zero, zero), (zero, zero)], dtype=np.uint64), u, fr[PUSH_ACC])
        ctx.scan_rlc(fr[PUSH_ACC], 32, d_rlc_kinds, np.array([(zero, zero), (zero, one), (one, zero), (zero, zero)], dtype=np.uint64), u, fr[PUSH_RLC], reverse=True)
        assert len(sess.advice_phase_dev({col: fr[col] for col in (VALUE_RLC, PUSH_ACC, PUSH_RLC)})) == 0
        cols = model_columns(circ, cref.from_mont(got))
        for col, d in fr.items():
            assert cref.from_mont(d.download((n, 4))) == cols[col], NAMES[col]
        proof = sess.finish()
    except BaseException:
        sess.abort()
        raise
    finally:
        for d in (d_bytes, d_offs, d_lens, d_hashes, d_acc_kinds, d_rlc_kinds, *typed.values(), *fr.values()):
            d.free()
    assert proof == want

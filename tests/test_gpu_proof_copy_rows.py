"""GPU: one proof at k = 8 over the gates of the copy circuit (copy_circuit.rs:250-420 with copy_circuit/copy_gadgets.rs, the access
list and dual-bytecode parts left out), every advice column made on the device from five copy events: ZK_OP_COPY_ROWS (the integer
columns), ZK_OP_ROW_INV0 three times (is_src_end over addr - src_addr_end with d_num = src_end_rows, is_word_end over word_index - 31,
is_id_unchange over id - id_other), ZK_OP_COPY_RLC under the two challenges squeezed after the first phase (value_acc, both word
RLCs, rlc_acc, the ids); zk_proof_advice_phase_typed_dev takes the typed buffers as they stand.  The gates: the tag bits against the
type columns, first and last, must-terminate, the forwarded parameters, is_pad with its IsEqual, mask and front_mask, non_pad_non_mask,
masked values, value_acc, rlc_acc on the last row, both word RLCs, word_index, real_bytes_left, the address, the rw counters with the
memory-copy rules, is_memory_copy with its IsEqual, and the word that an RW type must complete.  The events: a memory copy whose
reader is masked at the front and whose writer is masked at the back over overlapping runs, a calldata read that runs past
src_addr_end, a log, a copy both of whose threads are wholly masked, and a bytecode read into an RLC.  That route yields the proof
bytes of the route on which every column comes from the Python model, which the oracle verifier accepts and which equal the oracle
prover's; both multi-open schemes.  One changed cell in any column fails check_witness."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import copy_rows_cases as cp  # noqa: E402
from oracle import bn254 as b  # noqa: E402
from oracle import pairing as pr  # noqa: E402
from oracle import plonk_prover as pp  # noqa: E402
from oracle import plonk_verifier as pv  # noqa: E402
from test_gpu_proof_typed import S_SECRET, SEED, Case  # noqa: E402
from zkevm_circuits_amd import plonk  # noqa: E402

pytestmark = pytest.mark.gpu
R = b.R_MOD
FIRST_PHASE = ("is_first", "is_last", "tag_bits0", "tag_bits1", "tag_bits2", "value", "value_prev", "mask", "front_mask", "word_index", "addr", "src_addr_end", "is_pad",
               "non_pad_non_mask", "real_bytes_left", "rw_counter", "rwc_inc_left", "types0", "types1", "types2", "types3", "types4", "src_end_inv", "word_end_inv")
SECOND_PHASE = ("id", "id_inv", "value_acc", "word_rlc", "word_rlc_prev", "rlc_acc")
NAMES = FIRST_PHASE + SECOND_PHASE
COL = {name: i for i, name in enumerate(NAMES)}
ADVICE = len(NAMES)
WIDTHS = {name: 8 if name in cp.WORD_COLUMNS else 1 for name in FIRST_PHASE[:-2]}
Q_ENABLE, Q_STEP = range(2)

# the heap: 0 .. 63 the memory the copy reads, 64 .. 95 what lay at the destination before, 96 .. 127 calldata, 128 .. 159 the calldata
# as it arrives (zeros behind its end), 160 .. 191 log data, 192 .. 199 code
HEAP = bytearray(np.random.default_rng(0xC0).integers(1, 256, 200, dtype=np.uint8).tobytes())
HEAP[64 + 29:64 + 32] = HEAP[3 + 29:3 + 32]                              # the bytes the masked writer rows leave in place
HEAP[128:148] = HEAP[96:116]
HEAP[148:160] = bytes(12)
HEAP = bytes(HEAP)
EVENTS = [
    # MCOPY inside one call: the reader skips three bytes, the writer's last three are masked; the writer's bytes are the reader's
    cp.event(32, cp.MEMORY, cp.MEMORY, src_addr=0x40 - 3, src_addr_end=0x1000, dst_addr=0x80, rw_counter=9, src_off=0, dst_off=3, prev_off=64, src_front=3, src_back=0,
             dst_front=0, dst_back=3, flags=cp.MEMORY_COPY, src_id=5, dst_id=5),
    # CALLDATACOPY past the end of the calldata: twenty bytes, then zeros
    cp.event(32, cp.TX_CALLDATA, cp.MEMORY, src_addr=100, src_addr_end=120, dst_addr=0, rw_counter=11, src_off=96, dst_off=128, prev_off=128, src_id=1, dst_id=6),
    # LOG: the address column of the writer carries the field tag and the log id
    cp.event(32, cp.MEMORY, cp.TX_LOG, src_addr=0x20, src_addr_end=0x1000, dst_addr=0, dst_addr_bias=cp.log_bias(3), rw_counter=12, src_off=160, src_id=6, dst_id=1),
    # both threads wholly masked, the writer by counts that add up to more than the length
    cp.event(5, cp.TX_CALLDATA, cp.BYTECODE, src_addr=7, src_addr_end=12, dst_addr=0, rw_counter=14, src_off=96, dst_off=10, prev_off=10, src_front=5, src_back=0, dst_front=2,
             dst_back=4, src_id=1, dst_id=0x1234567),
    # SHA3-shaped: bytecode bytes into an RLC
    cp.event(7, cp.BYTECODE, cp.RLC_ACC, src_addr=1, src_addr_end=8, dst_addr=0, rw_counter=14, src_off=192, src_id=0x7654321, dst_id=8),
]
ROWS = sum(2 * e["length"] for e in EVENTS)


def copy_circuit(k):
    circ = plonk.Circuit(k, num_fixed=2, num_advice=ADVICE, num_instance=1, blinding_factors=5)
    circ.advice_phase = [0] * len(FIRST_PHASE) + [1] * len(SECOND_PHASE)
    keccak_input, evm_word = circ.challenge_usable_after(0), circ.challenge_usable_after(0)
    q, is_reader = circ.fixed_col(Q_ENABLE), circ.fixed_col(Q_STEP)
    cur = lambda name: circ.advice_col(COL[name], 0)                    # noqa: E731  CURRENT
    nrow = lambda name: circ.advice_col(COL[name], 1)                   # noqa: E731  NEXT_ROW
    nstep = lambda name: circ.advice_col(COL[name], 2)                  # noqa: E731  NEXT_STEP
    gate = lambda e: circ.add_gate(q * e)                               # noqa: E731
    boolean = lambda e: e * (1 - e)                                     # noqa: E731
    select = lambda c, x, y: c * x + (1 - c) * y                        # noqa: E731

    def tag_value(at):
        return 4 * at("tag_bits0") + 2 * at("tag_bits1") + at("tag_bits2")

    def tag_equals(t, at):
        e = 1
        for bit in range(3):
            e = e * (at(f"tag_bits{bit}") if t >> (2 - bit) & 1 else 1 - at(f"tag_bits{bit}"))
        return e

    # copy_circuit.rs:213-234 the three IsEqual chips
    id_diff = cur("id") - nrow("id")
    is_id_unchange = 1 - id_diff * cur("id_inv")
    circ.add_gate(is_reader * (1 - cur("is_last")) * id_diff * is_id_unchange)
    src_end = lambda at: 1 - (at("addr") - at("src_addr_end")) * at("src_end_inv")   # noqa: E731
    circ.add_gate(is_reader * (cur("addr") - cur("src_addr_end")) * src_end(cur))
    is_word_end = 1 - (cur("word_index") - 31) * cur("word_end_inv")
    gate((cur("word_index") - 31) * is_word_end)
    # copy_gadgets.rs:14-49 constrain_tag, and the bits are bits
    for bit in range(3):
        gate(boolean(cur(f"tag_bits{bit}")))
    for plane, t in enumerate((cp.BYTECODE, cp.MEMORY, cp.TX_CALLDATA, cp.TX_LOG)):
        gate(cur(f"types{plane}") - tag_equals(t, cur))
    is_bytecode, is_memory, is_tx_log, is_memory_copy = (lambda at: at("types0")), (lambda at: at("types1")), cur("types3"), cur("types4")
    is_first, is_last = cur("is_first"), cur("is_last")
    is_last_step = cur("is_last") + nrow("is_last")                     # copy_circuit.rs:259-263
    is_continue = 1 - is_last_step
    # :52-68 constrain_first_last
    gate(boolean(is_first))
    gate(boolean(is_last))
    gate((1 - is_reader) * is_first)
    gate(is_last * is_reader)
    # :71-91 constrain_must_terminate
    gate(tag_value(cur) * (circ.fixed_col(Q_ENABLE, 2) - 1))
    # :94-120 constrain_forward_parameters
    gate(is_continue * (cur("id") - nstep("id")))
    gate(is_continue * (tag_value(cur) - tag_value(nstep)))
    gate(is_continue * (cur("src_addr_end") - nstep("src_addr_end")))
    # :125-170 constrain_is_pad
    gate(boolean(cur("is_pad")))
    gate(is_reader * nrow("is_pad"))
    gate(is_first * (cur("is_pad") - src_end(cur)))
    gate(is_reader * (1 - nrow("is_last")) * (select(src_end(nstep), 1, cur("is_pad")) - nstep("is_pad")))
    # :174-239 constrain_mask (copy_circuit.rs:292-307: no front mask at a word end or in a log)
    for at in (cur, nrow):
        gate(is_first * (at("mask") - at("front_mask")))
    back_mask, back_mask_next = cur("mask") - cur("front_mask"), nstep("mask") - nstep("front_mask")
    gate(boolean(cur("mask")))
    gate(boolean(cur("front_mask")))
    gate(boolean(back_mask))
    gate(is_continue * boolean(cur("front_mask") - nstep("front_mask")))
    gate(is_continue * boolean(back_mask_next - back_mask))
    gate(is_continue * cur("front_mask") * back_mask_next)
    gate((is_word_end + is_tx_log) * cur("front_mask"))
    # :242-273 constrain_non_pad_non_mask, constrain_masked_value
    gate(cur("non_pad_non_mask") - (1 - cur("is_pad")) * (1 - cur("mask")))
    gate(cur("mask") * (cur("value") - cur("value_prev")))
    # :277-325 constrain_value_rlc
    for at in (cur, nrow):
        gate(is_first * (at("value_acc") - at("value") * at("non_pad_non_mask")))
    accumulated = cur("value_acc") * keccak_input + nstep("value") * (1 - nstep("is_pad"))
    gate(is_continue * (select(nstep("mask"), cur("value_acc"), accumulated) - nstep("value_acc")))
    gate(nrow("is_last") * (cur("value_acc") - nrow("value_acc")))
    # :329-368 constrain_event_rlc_acc
    gate((1 - is_last) * (cur("rlc_acc") - nrow("rlc_acc")))
    rlc_acc_cond = tag_equals(cp.RLC_ACC, cur) + tag_equals(cp.RLC_ACC, nrow) + is_bytecode(nrow)
    gate(rlc_acc_cond * nrow("is_last") * (nrow("value_acc") - nrow("rlc_acc")))
    # :372-409 constrain_word_rlc, before and after the write
    for word_rlc, value in (("word_rlc", "value"), ("word_rlc_prev", "value_prev")):
        for at in (cur, nrow):
            gate(is_first * (at(word_rlc) - at(value)))
        gate(is_continue * (select(is_word_end, 0, cur(word_rlc)) * evm_word + nstep(value) - nstep(word_rlc)))
    # :412-441 constrain_word_index
    for at in (cur, nrow):
        gate(is_first * at("word_index"))
    gate(is_continue * (select(is_word_end, 0, cur("word_index") + 1) - nstep("word_index")))
    # :444-469 constrain_bytes_left
    gate(is_first * (cur("real_bytes_left") - nrow("real_bytes_left")))
    gate(cur("real_bytes_left") - (1 - cur("mask")) - is_continue * nstep("real_bytes_left"))
    # :472-490 constrain_address
    gate(is_continue * (cur("addr") + (1 - cur("front_mask")) - nstep("addr")))
    # :494-569 constrain_rw_counter (copy_circuit.rs:367-390: memory and log are the RW types, a row ends at a word end)
    new_value = cur("rwc_inc_left") - (is_memory(cur) + is_tx_log) * is_word_end
    gate((1 - is_memory_copy) * (new_value - (1 - is_last) * nrow("rwc_inc_left")))
    gate(is_memory_copy * (1 - nrow("is_last")) * (1 - is_last) * (new_value - nstep("rwc_inc_left")))
    gate(is_memory_copy * is_last * (cur("rwc_inc_left") - 1))
    gate(is_memory_copy * is_first * (cur("rwc_inc_left") - 2 * nrow("rwc_inc_left")))
    gate((1 - is_last) * (cur("rw_counter") + cur("rwc_inc_left") - nrow("rw_counter") - nrow("rwc_inc_left")))
    # :572-593 constrain_is_memory_copy, :596-610 constrain_rw_word_complete
    gate(boolean(is_memory_copy))
    gate((1 - is_last) * (is_memory_copy - is_memory(cur) * is_memory(nrow) * is_id_unchange))
    gate(is_last_step * (is_memory(cur) + is_tx_log) * (1 - is_word_end))
    # copy_circuit.rs:927-937: the last two usable rows are disabled rows
    for row in range(circ.u - 2):
        circ.fixed[Q_ENABLE][row] = 1
        circ.fixed[Q_STEP][row] = 1 - row % 2
    circ.copy((plonk.ADVICE, COL["value"], 0), (plonk.INSTANCE, 0, 0))
    return circ


def inv0(v):
    return pow(v % R, R - 2, R)


def model_columns(circ, ch):
    """every advice column from the Python model: u rows of the assignment loop, zeros behind them"""
    keccak_input, evm_word = ch if ch else (0, 0)
    u = circ.u
    m = cp.assign(EVENTS, HEAP, u, evm_word, keccak_input)
    m["src_end_inv"] = [m["src_end_rows"][i] * inv0(m["addr"][i] - m["src_addr_end"][i]) % R for i in range(u)]   # copy_circuit.rs:749-757, :1112-1117
    m["word_end_inv"] = [inv0(m["word_index"][i] - 31) for i in range(u)]                                        # :773-778, :1118-1123
    m["id_inv"] = [inv0(m["id"][i] - m["id_other"][i]) for i in range(u)]                                        # :759-771, :1106-1111
    return {COL[name]: m[name] + [0] * (circ.n - u) for name in NAMES}


@pytest.fixture(scope="module")
def case(ctx, cref):
    circ = copy_circuit(8)
    assert circ.u % 2 == 0 and ROWS + 4 <= circ.u                       # padding rows in front of the two disabled rows

    def synth(phase, ch):
        cols = model_columns(circ, ch)
        return {col: v for col, v in cols.items() if circ.advice_phase[col] == phase}
    c = Case(ctx, cref, circ, synth, [[HEAP[0]] + [0] * (circ.n - 1)])
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
    m = cp.assign(EVENTS, HEAP, circ.u, ch[1], ch[0])
    c = cp.closed(EVENTS, HEAP, circ.u, ch[1], ch[0])
    assert all(m[name] == c[name] for name in cp.INT_COLUMNS + cp.FR_COLUMNS), "on these events the reference's rlc_acc is the op's"
    assert sum(m["is_pad"]) == 12 and sum(m["front_mask"][:64]) == 3 and all(m["front_mask"][192:202]) and m["addr"][129] == cp.log_bias(3) and m["rlc_acc"][202] >= 1 << 128
    assert any(v >= 1 << 128 for v in adv[COL["word_rlc"]]) and any(v >= 1 << 128 for v in adv[COL["value_acc"]]), "a challenge reached no cell"
    assert pv.check_witness(circ, adv, case.inst, challenges=ch) is None
    row = 74                                                            # step 5 of the calldata read: a reader row in the middle of a word, ids that differ
    for col in range(ADVICE):
        wrong = [list(x) for x in adv]
        wrong[col][row] = (wrong[col][row] + 2) % R
        assert pv.check_witness(circ, wrong, case.inst, challenges=ch) is not None, NAMES[col]
    assert pv.verify(circ, case.vk_points, case.vk_repr, case.inst, proof, pr.ec_mul(pr.G2_GEN, S_SECRET), multiopen=scheme)
    assert proof == pp.create_proof(circ, pp.Srs(circ.k, S_SECRET), adv, case.inst, case.vk_repr, SEED, scheme)


@pytest.mark.parametrize("scheme", ["gwc", "shplonk"])
def test_device_route_gives_the_same_challenges_and_bytes(ctx, cref, case, scheme):
    circ = case.circ
    n, u = circ.n, circ.u
    want, want_ch = case.fr_proof(scheme)
    d_events, d_heap, d_ids = ctx.to_device(cp.pack_events(EVENTS)), ctx.to_device(np.frombuffer(HEAP, dtype=np.uint8)), ctx.to_device(cp.pack_ids(EVENTS))
    typed = {name: ctx.to_device(np.zeros(n * 8 if name in cp.WORD_COLUMNS else n, dtype=np.uint8)) for name in cp.BYTE_COLUMNS + cp.WORD_COLUMNS}   # rows from usable_rows on stay zero
    planes = {name: ctx.to_device(np.zeros(n * count, dtype=np.uint8)) for name, count in cp.PLANE_COLUMNS.items()}
    fr = {name: ctx.to_device(np.zeros((n, 4), dtype=np.uint64)) for name in ("src_end_inv", "word_end_inv", "id_other") + SECOND_PHASE}
    one, minus_one, minus_31 = cref.fr_const(1)[0], cref.fr_const(R - 1)[0], cref.fr_const(R - 31)[0]
    sess = case.session(scheme)
    try:
        # phase 1 of the reference's numbering: nothing here depends on a challenge
        ctx.copy_rows(d_events, len(EVENTS), d_heap, len(HEAP), u, typed["addr"], tag_bits=planes["tag_bits"], types=planes["types"],
                      **{name: typed[name] for name in cp.BYTE_COLUMNS + cp.WORD_COLUMNS if name != "addr"})
        ctx.row_inv0([typed["addr"], typed["src_addr_end"]], [8, 8], [one, minus_one], u, fr["src_end_inv"], num=typed["src_end_rows"], num_width=1)
        ctx.row_inv0([typed["word_index"]], [1], [one], u, fr["word_end_inv"], constant=minus_31)
        columns = {COL[name]: (typed[name], w) for name, w in WIDTHS.items() if name in typed}
        columns.update({COL[f"{name}{p}"]: (planes[name].ptr + p * u, 1) for name, count in cp.PLANE_COLUMNS.items() for p in range(count)})
        columns.update({COL[name]: (fr[name], 32) for name in ("src_end_inv", "word_end_inv")})
        assert sorted(columns) == list(range(len(FIRST_PHASE)))
        got = sess.advice_phase_typed_dev(columns)
        assert np.array_equal(got, want_ch[0])
        keccak_input, evm_word = got[0], got[1]
        # phase 2: the columns under the challenges
        ctx.copy_rlc(d_events, len(EVENTS), d_heap, len(HEAP), u, fr["value_acc"], evm_word, keccak_input, ids=d_ids, id=fr["id"], id_other=fr["id_other"], rlc_acc=fr["rlc_acc"],
                     word_rlc=fr["word_rlc"], word_rlc_prev=fr["word_rlc_prev"])
        ctx.row_inv0([fr["id"], fr["id_other"]], [32, 32], [one, minus_one], u, fr["id_inv"])
        assert len(sess.advice_phase_dev({COL[name]: fr[name] for name in SECOND_PHASE})) == 0
        cols = model_columns(circ, cref.from_mont(got))
        for name in ("src_end_inv", "word_end_inv") + SECOND_PHASE:
            assert cref.from_mont(fr[name].download((n, 4))) == cols[COL[name]], name
        proof = sess.finish()
    except BaseException:
        sess.abort()
        raise
    finally:
        for d in (d_events, d_heap, d_ids, *typed.values(), *planes.values(), *fr.values()):
            d.free()
    assert proof == want

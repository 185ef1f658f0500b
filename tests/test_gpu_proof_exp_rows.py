"""GPU: one proof at k = 8 over the gates of the exponentiation circuit (exp_circuit.rs:95-308: all but the last step, all rows, all
steps), the mul-add gate of both MulAddChips (gadgets mul_add.rs:168-217), both range-composition gates of each (range.rs:68-83) and
the parity chip's overflow, every one of the 36 advice columns made on the device by ONE ZK_OP_EXP_ROWS call from four events;
zk_proof_advice_phase_typed_dev takes the typed buffers as they stand.  The u16 lookups are left out: 2-byte cells are in range by
construction.  The fixed columns q_enable, is_step and is_final_step are key material.  The events: (3, 13), (2^200 + 5, 6), (7, 1)
-- no steps --, (2^256 - 1, 37): 15 steps, then padding steps up to the ten unusable rows, with max_exp_rows the circuit's 250 usable
rows (no multiple of 8).  That route yields the challenges and the proof bytes of the route on which every column comes from the Python
model, which the oracle verifier accepts and which equal the oracle prover's; both multi-open schemes.  One changed cell in any column
on the first row of a step that is not a last step fails check_witness."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import exp_rows_cases as ex  # noqa: E402
from oracle import bn254 as b  # noqa: E402
from oracle import pairing as pr  # noqa: E402
from oracle import plonk_prover as pp  # noqa: E402
from oracle import plonk_verifier as pv  # noqa: E402
from test_gpu_proof_typed import S_SECRET, SEED, Case  # noqa: E402
from zkevm_circuits_amd import plonk  # noqa: E402

pytestmark = pytest.mark.gpu
R = b.R_MOD
NAMES = ex.COLUMNS
COL = {name: i for i, name in enumerate(NAMES)}
ADVICE = len(NAMES)
Q_ENABLE, IS_STEP, IS_FINAL_STEP = range(3)
EVENTS = [(3, 13), ((1 << 200) + 5, 6), (7, 1), (ex.M256, 37)]
STEPS = sum(ex.steps_of(x) for _, x in EVENTS)
OFFSET_INCREMENT = 8


def exp_circuit(k):
    circ = plonk.Circuit(k, num_fixed=3, num_advice=ADVICE, num_instance=1, blinding_factors=5)
    q_enable, is_step, is_final_step = circ.fixed_col(Q_ENABLE), circ.fixed_col(IS_STEP), circ.fixed_col(IS_FINAL_STEP)
    adv = lambda name, rot=0: circ.advice_col(COL[name], rot)           # noqa: E731
    boolean = lambda e: e * (1 - e)                                     # noqa: E731
    step = q_enable * is_step                                           # exp_circuit.rs:70-89: the q_enable of both chips
    two64, two128 = 1 << 64, 1 << 128

    def chip(prefix):
        """mul_add.rs:124-253 MulAddChip::configure without the lookups: the cells by name, the two checks, the range gates"""
        col = lambda i, rot: adv(f"{prefix}_cols.{i}", rot)             # noqa: E731
        a, bb = [col(i, 0) for i in range(4)], [col(i, 1) for i in range(4)]
        c_lo, c_hi, d_lo, d_hi = (col(i, 2) for i in range(4))
        from_u16 = lambda cells: sum(cell * (1 << 16 * i) for i, cell in enumerate(cells))   # noqa: E731  expr_from_u16
        carry_lo = from_u16([col(0, 3), col(1, 3), col(2, 3), col(3, 3), col(0, 4)])          # mul_add.rs:130-134
        carry_hi = from_u16([col(0, 5), col(1, 5), col(2, 5), col(3, 5), col(0, 6)])          # :136-140
        t0 = a[0] * bb[0]                                                                    # :187-196
        t1 = a[0] * bb[1] + a[1] * bb[0]
        t2 = a[0] * bb[2] + a[1] * bb[1] + a[2] * bb[0]
        t3 = a[0] * bb[3] + a[1] * bb[2] + a[2] * bb[1] + a[3] * bb[0]
        overflow = carry_hi + a[1] * bb[3] + a[2] * bb[2] + a[2] * bb[3] + a[3] * bb[1] + a[3] * bb[2] + a[3] * bb[3]   # :197-203
        circ.add_gate(step * (t0 + t1 * two64 + c_lo - (d_lo + carry_lo * two128)))           # :207-208 check_a
        circ.add_gate(step * (t2 + t3 * two64 + c_hi + carry_lo - (d_hi + carry_hi * two128)))   # :211-212 check_b
        # range.rs:68-83 over mul_add.rs:220-241: a and b on the first two rows against four u16 cells, c and d on the third against eight
        for row_idx, expr in enumerate(a + bb):
            circ.add_gate(step * (expr - from_u16([adv(f"{prefix}_u16_64.{c}", row_idx) for c in range(4)])))
        for row_idx, expr in enumerate((c_lo, c_hi, d_lo, d_hi)):
            circ.add_gate(step * (expr - from_u16([adv(f"{prefix}_u16_128.{c}", row_idx) for c in range(8)])))
        return {"a": a, "b": bb, "c": (c_lo, c_hi), "d": (d_lo, d_hi), "d_next": (col(2, 2 + 8), col(3, 2 + 8)), "overflow": overflow}

    mul, parity = chip("mul"), chip("parity")
    is_last = adv("is_last")
    base = lambda rot: adv("base_limb", rot)                            # noqa: E731
    exponent = lambda rot: adv("exponent_lo_hi", rot)                   # noqa: E731
    # exp_circuit.rs:95-140 "verify all but the last step"
    not_last = step * (1 - is_last)
    for i in range(4):
        circ.add_gate(not_last * (base(i) - base(i + OFFSET_INCREMENT)))
    circ.add_gate(not_last * (mul["a"][0] + mul["a"][1] * two64 - mul["d_next"][0]))
    circ.add_gate(not_last * (mul["a"][2] + mul["a"][3] * two64 - mul["d_next"][1]))
    circ.add_gate(not_last * is_final_step)
    # :142-158 "verify all rows"
    circ.add_gate(q_enable * boolean(is_step))
    circ.add_gate(q_enable * boolean(is_last))
    # :160-308 "verify all steps"
    circ.add_gate(step * (adv("exponentiation_lo_hi", 0) - mul["d"][0]))
    circ.add_gate(step * (adv("exponentiation_lo_hi", 1) - mul["d"][1]))
    circ.add_gate(step * mul["c"][0])
    circ.add_gate(step * mul["c"][1])
    is_odd, remainder_hi = parity["c"]
    circ.add_gate(step * remainder_hi)
    circ.add_gate(step * boolean(is_odd))
    circ.add_gate(step * (parity["a"][0] - 2))
    for limb in parity["a"][1:]:
        circ.add_gate(step * limb)
    circ.add_gate(step * parity["overflow"])
    odd = step * (1 - is_last) * is_odd                                 # :205-233
    circ.add_gate(odd * (exponent(OFFSET_INCREMENT) - (exponent(0) - 1)))
    circ.add_gate(odd * (exponent(1 + OFFSET_INCREMENT) - exponent(1)))
    for i in range(4):
        circ.add_gate(odd * (base(i) - mul["b"][i]))
    even = step * (1 - is_last) * (1 - is_odd)                          # :235-272
    circ.add_gate(even * (exponent(0) - parity["d"][0]))
    circ.add_gate(even * (exponent(1) - parity["d"][1]))
    circ.add_gate(even * (exponent(OFFSET_INCREMENT) - (parity["b"][0] + parity["b"][1] * two64)))
    circ.add_gate(even * (exponent(1 + OFFSET_INCREMENT) - (parity["b"][2] + parity["b"][3] * two64)))
    for i in range(4):
        circ.add_gate(even * (mul["a"][i] - mul["b"][i]))
    last = step * is_last                                               # :275-302
    circ.add_gate(last * (exponent(0) - 2))
    circ.add_gate(last * exponent(1))
    for i in range(4):
        circ.add_gate(last * (base(i) - mul["a"][i]))
        circ.add_gate(last * (base(i) - mul["b"][i]))
    # the fixed columns as assign_exp_events leaves them for max_exp_rows = the usable rows (exp_circuit.rs:362-381, :428-441, :462-469)
    offset = 0
    while offset + OFFSET_INCREMENT <= circ.u - ex.UNUSABLE_EXP_ROWS:
        for i in range(OFFSET_INCREMENT):
            circ.fixed[Q_ENABLE][offset + i] = 1
        circ.fixed[IS_STEP][offset] = 1
        offset += OFFSET_INCREMENT
    circ.fixed[IS_FINAL_STEP][offset - OFFSET_INCREMENT] = 1
    circ.copy((plonk.ADVICE, COL["exponentiation_lo_hi"], 0), (plonk.INSTANCE, 0, 0))
    return circ


def model_columns(circ):
    """every advice column from the Python model of the reference's loop: u rows, zeros behind them"""
    m = ex.assign(EVENTS, circ.u)
    return {COL[name]: m[name] + [0] * (circ.n - circ.u) for name in NAMES}


@pytest.fixture(scope="module")
def case(ctx, cref):
    circ = exp_circuit(8)
    assert circ.u % 8 and ex.rows_needed(EVENTS) + 8 <= circ.u and STEPS == 15   # padding steps in front of the unusable rows
    c = Case(ctx, cref, circ, lambda phase, ch: model_columns(circ), [[pow(3, 13) & ex.M128] + [0] * (circ.n - 1)])
    yield c
    c.close()


@pytest.mark.parametrize("scheme", ["gwc", "shplonk"])
def test_host_route_is_accepted_and_equals_the_oracle_prover(case, scheme):
    circ = case.circ
    proof, per_phase = case.fr_proof(scheme)
    assert [len(c) for c in per_phase] == [0]
    cols = model_columns(circ)
    adv = [cols[col] for col in range(ADVICE)]
    m, c = ex.assign(EVENTS, circ.u), ex.closed(EVENTS, circ.u)
    assert all(m[name] == c[name] for name in NAMES)
    assert sum(m["is_last"]) == 3 + (circ.u - 10 - 8 * STEPS) // 8 and any(m["mul_cols.0"][4::8]), "pad steps, and a carry of more than 64 bits"
    assert pv.check_witness(circ, adv, case.inst) is None
    row = 8 * 6                                                         # step 1 of (2^200 + 5, 6): x = 3 is odd, not the last step
    assert m["is_last"][row] == 0 and m["exponent_lo_hi"][row] == 3
    for col in range(ADVICE):
        wrong = [list(x) for x in adv]
        wrong[col][row] = (wrong[col][row] + 2) % R
        assert pv.check_witness(circ, wrong, case.inst) is not None, NAMES[col]
    assert pv.verify(circ, case.vk_points, case.vk_repr, case.inst, proof, pr.ec_mul(pr.G2_GEN, S_SECRET), multiopen=scheme)
    assert proof == pp.create_proof(circ, pp.Srs(circ.k, S_SECRET), adv, case.inst, case.vk_repr, SEED, scheme)


@pytest.mark.parametrize("scheme", ["gwc", "shplonk"])
def test_device_route_gives_the_same_challenges_and_bytes(ctx, case, scheme):
    circ = case.circ
    n, u = circ.n, circ.u
    want, want_ch = case.fr_proof(scheme)
    d_events = ctx.to_device(ex.pack_events(EVENTS))
    out = {name: ctx.to_device(np.zeros(n * width * planes, dtype=np.uint8)) for name, width, planes in ex.OUTPUTS}   # rows from usable_rows on stay zero
    d_needed = ctx.to_device(np.zeros(1, dtype=np.uint64))
    sess = case.session(scheme)
    try:
        ctx.exp_rows(d_events, len(EVENTS), u, out["exponentiation_lo_hi"], rows_needed=d_needed, **{name: out[name] for name, _, _ in ex.OUTPUTS[1:]})
        columns = {}
        for name, width, planes in ex.OUTPUTS:
            if planes == 1:
                columns[COL[name]] = (out[name], width)
            else:
                prefix, kind = name.split("_", 1)
                columns.update({COL[f"{prefix}_{kind}.{p}"]: (out[name].ptr + p * u * width, width) for p in range(planes)})
        assert sorted(columns) == list(range(ADVICE))
        got = sess.advice_phase_typed_dev(columns)
        assert len(got) == 0 and len(want_ch[0]) == 0
        assert int(d_needed.download(1, np.uint64)[0]) == ex.rows_needed(EVENTS) <= u    # the check the reference asserts
        proof = sess.finish()
    except BaseException:
        sess.abort()
        raise
    finally:
        for d in (d_events, d_needed, *out.values()):
            d.free()
    assert proof == want

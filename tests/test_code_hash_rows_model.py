"""CPU: the closed forms of ZK_OP_CODE_HASH_ROWS and ZK_OP_CODE_HASH_TABLE (tests/code_hash_rows_cases.py) against the line-by-line
transliteration of the reference's assign_extended_row / set_header_row with its carried row_input and of PoseidonTable::dev_load
with unroll_to_hash_input, and the reference's own bytecode_unrolling_to_input assertions through the transliteration."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import code_hash_rows_cases as ch  # noqa: E402
import poseidon_cases as pc  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "code_hash_rows_reference.json")


def code_of(length, seed=0):
    return ch.random_code(np.random.default_rng(1000 * seed + length), length)


def test_closed_forms_equal_the_transliteration_for_every_length_up_to_190():
    for length in range(191):
        code = code_of(length)
        n = length + 3
        assert ch.rows_closed([code], n) == ch.assign([code], n), length
        rows, owner = ch.dev_load([code])
        cols, needed = ch.table_closed([code], len(rows) + 1)
        assert needed == len(rows) == -(-length // 62), length
        for i, (in0, in1, control, domain, mark) in enumerate(rows):
            assert (cols["input0"][i], cols["input1"][i], cols["control"][i], cols["heading_mark"][i], cols["cap"][i]) == (in0, in1, control, mark, length) and domain == 0
            assert cols["kinds"][i] == (ch.HEAD if mark else ch.CONT)
        assert [cols[name][-1] for name in ch.TABLE_COLUMNS] == [0, 0, 0, 0, ch.OFF, 0]


def test_closed_forms_equal_the_transliteration_for_random_codes_side_by_side_and_cut():
    rng = np.random.default_rng(7)
    for trial in range(20):
        codes = [ch.random_code(rng, int(k)) for k in rng.integers(0, 200, int(rng.integers(1, 7)))]
        total = sum(len(c) + 1 for c in codes)
        for n in (total + 5, total, total - 1, max(1, total // 2), 1):
            assert ch.rows_closed(codes, n) == ch.assign(codes, n), (trial, n)
        rows, owner = ch.dev_load(codes)
        for n in (len(rows) + 3, len(rows), max(len(rows) - 1, 0)):
            cols, needed = ch.table_closed(codes, n)
            assert needed == len(rows)
            for i in range(min(n, len(rows))):
                assert (cols["input0"][i], cols["input1"][i], cols["control"][i], cols["heading_mark"][i]) == (rows[i][0], rows[i][1], rows[i][2], rows[i][4])
                assert cols["cap"][i] == len(codes[owner[i]])


def test_the_issue_lengths():
    codes = [code_of(k, 3) for k in ch.LENGTHS]
    n = sum(len(c) + 1 for c in codes) + 4
    assert ch.rows_closed(codes, n) == ch.assign(codes, n)


def test_a_border_row_holds_the_table_input():
    """on a row with is_field_border the circuit looks (field_input, field_index, control_length) up in the table: field_input must be
    input0 or input1 of the block, by field_index"""
    for length in list(range(0, 130)) + [500]:
        code = code_of(length, 5)
        cols = ch.rows_closed([code], length + 1)
        table, _ = ch.table_closed([code], -(-length // 62))
        seen = 0
        for p in range(length):
            row = p + 1
            if not cols["is_field_border"][row]:
                continue
            j = p // 62
            want = table["input0"][j] if cols["field_index"][row] == 1 else table["input1"][j]
            assert cols["field_input"][row] == want and cols["control_length"][row] * ch.HASHABLE_DOMAIN_SPEC == table["control"][j], (length, p)
            seen += 1
        assert seen == -(-length // 31)


def test_the_vectorised_columns_are_the_closed_forms():
    rng = np.random.default_rng(9)
    codes = [ch.random_code(rng, k) for k in (0, 1, 30, 31, 32, 61, 62, 63, 124, 700)]
    for n in (sum(len(c) + 1 for c in codes) + 9, 800, 1):
        want, got = ch.rows_closed(codes, n), ch.rows_numpy(codes, n)
        for name in ch.ROW_COLUMNS:
            assert np.array_equal(got[name].view(np.uint8).reshape(-1), ch.cells(name, want[name], ch.ROW_WIDTHS)), (n, name)
    for n in (sum(-(-len(c) // 62) for c in codes) + 2, 17, 3, 0):
        (want, needed), (got, got_needed) = ch.table_closed(codes, n), ch.table_numpy(codes, n)
        assert needed == got_needed
        for name in ch.TABLE_COLUMNS:
            assert np.array_equal(got[name].view(np.uint8).reshape(-1), ch.cells(name, want[name], ch.TABLE_WIDTHS)), (n, name)


def test_the_table_inputs_hash_to_the_code_hash():
    """the sponge of poseidon_cases over the closed-form rows (cap = L, scale 2^64, head / continue kinds, FINAL) is the code hash"""
    for code, digest in pc.golden_vectors():
        if not code:
            continue                                                     # an empty bytecode owns no table row
        cols, needed = ch.table_closed([code], -(-len(code) // 62))
        out, _, _ = pc.expected(cols["input0"], cols["input1"], cap=cols["cap"], kinds=cols["kinds"], cap_scale=pc.CAP_SCALE_CODE, final=True)
        assert set(out) == {digest} and pc.code_hash(code) == digest


def test_the_references_own_unrolling_assertions():
    """to_poseidon_hash.rs:688-727 (fn bytecode_unrolling_to_input), recorded in the fixture with file:line, through the
    transliteration with its field width as a parameter"""
    recorded = json.load(open(GOLDEN))["unrolling_assertions"]
    assert len(recorded) == 5 and all(a["ref"].startswith("bytecode_circuit/circuit/to_poseidon_hash.rs:") for a in recorded)
    bt = bytes(range(1, 16))
    for a in recorded:
        out = ch.unroll_to_hash_input(bt[:a["take"]], a["bytes_in_field"], a["input_len"])
        assert out == [[int(x, 16) for x in row] for row in a["out"]], a["ref"]
        # and the circuit side of the same widths: a border row's field_input is that input
        cols = ch.assign([bt[:a["take"]]], a["take"] + 1, a["bytes_in_field"], a["input_len"])
        borders = [cols["field_input"][r] for r in range(a["take"] + 1) if cols["is_field_border"][r]]
        flat = [x for row in out for x in row]
        assert borders == flat[:len(borders)] and not any(flat[len(borders):]), a["ref"]

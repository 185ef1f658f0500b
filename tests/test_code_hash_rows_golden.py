"""CPU: the model of tests/code_hash_rows_cases.py against tests/golden/code_hash_rows_reference.json -- the three contract codes of
bytecode_rows_reference.json and the five byte strings of the Poseidon code hash fixture: for every column of the Poseidon-hash
extension and of the table the first 64 rows and a SHA-256 over the whole column as the device writes it, the closed forms and the
vectorised columns against the same records, and the recorded code hash.  Reads the JSON only."""
import hashlib
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import code_hash_rows_cases as ch  # noqa: E402
import poseidon_cases as pc  # noqa: E402

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GOLDEN = os.path.join(HERE, "code_hash_rows_reference.json")


def records():
    ref = json.load(open(GOLDEN))
    base = json.load(open(os.path.join(HERE, "bytecode_rows_reference.json")))
    pos = json.load(open(os.path.join(HERE, "poseidon_code_hash.json")))["vectors"]
    codes = [bytes.fromhex(c["code"]) for c in base["contracts"]] + [bytes.fromhex(v["code"]) for v in pos]
    return ref, list(zip(ref["contracts"] + ref["poseidon_vectors"], codes))


def first(name, vals, widths):
    return [hex(v) if widths[name] >= 16 else v for v in vals[:64]]


def test_the_fixture_is_what_it_says():
    ref, recs = records()
    assert os.path.getsize(GOLDEN) < 256 * 1024
    assert [r["entry"] for r in ref["contracts"]] == [8, 6, 1] and len(ref["poseidon_vectors"]) == 5 and len(ref["unrolling_assertions"]) == 5
    assert [r["bytes"] for r in ref["contracts"]] == [74, 1852, 5871] and 5036 in [r["bytes"] for r in ref["poseidon_vectors"]]
    for r, code in recs:
        assert len(code) == r["bytes"] and hashlib.sha256(code).hexdigest() == r["code_sha256"]
        assert r["rows"] == r["bytes"] + 2 and r["table_rows"] == -(-r["bytes"] // 62) + 1
        assert set(r["columns"]) == set(ch.ROW_COLUMNS) and set(r["table"]) == set(ch.TABLE_COLUMNS)
    for r in ref["poseidon_vectors"]:
        assert int(r["hash"], 16) == int(r["code_hash"], 16), "the model's code hash is the reference-held one"


def test_the_models_assign_the_recorded_columns():
    _, recs = records()
    for r, code in recs:
        line, closed, fast = ch.assign([code], r["rows"]), ch.rows_closed([code], r["rows"]), ch.rows_numpy([code], r["rows"])
        for name in ch.ROW_COLUMNS:
            want = r["columns"][name]
            assert first(name, line[name], ch.ROW_WIDTHS) == want["first"] == first(name, closed[name], ch.ROW_WIDTHS), (r["bytes"], name)
            assert hashlib.sha256(ch.cells(name, line[name], ch.ROW_WIDTHS).tobytes()).hexdigest() == want["sha256"], (r["bytes"], name)
            assert hashlib.sha256(fast[name].tobytes()).hexdigest() == want["sha256"], (r["bytes"], name)
        table, needed = ch.table_closed([code], r["table_rows"])
        assert needed == r["table_rows"] - 1
        for name in ch.TABLE_COLUMNS:
            want = r["table"][name]
            assert first(name, table[name], ch.TABLE_WIDTHS) == want["first"], (r["bytes"], name)
            assert hashlib.sha256(ch.cells(name, table[name], ch.TABLE_WIDTHS).tobytes()).hexdigest() == want["sha256"], (r["bytes"], name)
        assert pc.code_hash(code) == int(r["code_hash"], 16)


def test_real_code_meets_every_kind_of_row():
    _, recs = records()
    r, code = recs[2]
    cols = ch.assign([code], r["rows"])
    assert set(cols["field_index"]) == {1, 2} and set(cols["bytes_in_field_index"]) == set(range(32)) and set(cols["is_field_border"]) == {0, 1}
    assert cols["control_length"][1] == 5871 and min(cols["control_length"][1:-1]) == 5871 - 62 * (5870 // 62)

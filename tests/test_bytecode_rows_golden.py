"""CPU: the model of tests/bytecode_rows_cases.py against tests/golden/bytecode_rows_reference.json -- three real contract codes out
of a block trace of the reference's test data and the five byte strings of the Poseidon code hash fixture: for every integer column of
the bytecode circuit the first 64 rows, a SHA-256 over the whole column and the number of is_code rows, and the vectorised columns
(rows_numpy, what the large GPU case and the timing tool compare with) against the same records.  Reads the JSON only."""
import hashlib
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import bytecode_rows_cases as bc  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bytecode_rows_reference.json")
DTYPE = {1: "<u1", 4: "<u4"}


def records():
    ref = json.load(open(GOLDEN))
    return ref, ref["contracts"] + ref["poseidon_vectors"]


def test_the_fixture_is_what_it_says():
    ref, recs = records()
    assert os.path.getsize(GOLDEN) < 40 * 1024
    assert "trace_v2_5224657.json" in ref["source"] and [r["entry"] for r in ref["contracts"]] == [8, 6, 1] and len(ref["poseidon_vectors"]) == 5
    assert [r["bytes"] for r in ref["contracts"]] == [74, 1852, 5871] and [r["bytes"] for r in ref["poseidon_vectors"]][:4] == [0, 1, 2, 32]
    pos = json.load(open(os.path.join(os.path.dirname(GOLDEN), "poseidon_code_hash.json")))["vectors"]
    assert [r["code"] for r in ref["poseidon_vectors"]] == [v["code"] for v in pos]
    for r in recs:
        assert len(bytes.fromhex(r["code"])) == r["bytes"] and r["rows"] == r["bytes"] + 2 and set(r["columns"]) == set(bc.INT_COLUMNS)


def test_the_model_assigns_the_recorded_columns():
    _, recs = records()
    for r in recs:
        code = bytes.fromhex(r["code"])
        m = bc.assign([code], [0], r["rows"], 0)
        w = bc.rows_numpy([code], r["rows"])
        assert sum(m["is_code"]) == r["is_code_rows"] == int(w["is_code"].sum())
        for name in bc.INT_COLUMNS:
            want = r["columns"][name]
            assert m[name][:64] == want["first"], (r["bytes"], name)
            cells = np.array(m[name], dtype=DTYPE[bc.INT_WIDTHS[name]])
            assert hashlib.sha256(cells.tobytes()).hexdigest() == want["sha256"], (r["bytes"], name)
            assert hashlib.sha256(w[name].astype(DTYPE[bc.INT_WIDTHS[name]]).tobytes()).hexdigest() == want["sha256"], (r["bytes"], name)


def test_real_code_has_pushes_of_every_kind_of_row():
    _, recs = records()
    big = recs[2]
    m = bc.assign([bytes.fromhex(big["code"])], [0], big["rows"], 0)
    assert set(m["rlc_kinds"]) == {0, 1, 2} and set(m["acc_kinds"]) == {0, 1} and max(m["push_data_left"]) == 32 and 0 < big["is_code_rows"] < big["bytes"]

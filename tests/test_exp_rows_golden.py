"""CPU: tests/golden/exp_rows_reference.json -- the reference's own exponentiation vectors (23^123 and the five steps of 3^13 of
bus-mapping's test_exp_by_squaring, the 129-bit exponent of exp_circuit_big, the default padding event) with the 36 columns of the
exponentiation circuit as recorded from the line-by-line model -- against the model as it stands and against the closed forms that
the device op evaluates.  The file is data: nothing in it is executed."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import exp_rows_cases as ex  # noqa: E402

GOLDEN = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "exp_rows_reference.json")))
EVENTS, N = [(int(b, 16), int(x, 16)) for b, x in GOLDEN["events"]], GOLDEN["rows"]


def check(cols):
    assert set(GOLDEN["columns"]) == set(ex.COLUMNS)
    for name, rec in GOLDEN["columns"].items():
        first = [int(v, 16) for v in rec["first"]]
        assert len(first) == 64 and cols[name][:64] == first, name
        assert ex.column_digest(cols[name]) == rec["sha256"], name


def test_the_vectors_are_the_references():
    v = GOLDEN["exp_by_squaring"]
    steps = []
    assert ex.exp_by_squaring(v["base"], v["exponent"], steps) == int(v["result"]) == pow(23, 123, 1 << 256) and len(steps) == ex.steps_of(123)
    steps = []
    assert ex.exp_by_squaring(3, 13, steps) == 1594323 and [list(s) for s in steps] == GOLDEN["steps_3_13"]
    assert EVENTS == [(23, 123), (3, 13), (2, int(GOLDEN["big_exponent"], 16))] and int(GOLDEN["big_exponent"], 16) == (1 << 129) - 2
    assert GOLDEN["steps"] == [ex.steps_of(x) for _, x in EVENTS] == [11, 5, 255] and N == 8 * sum(GOLDEN["steps"]) + 10 + 8 * 2 + 3
    assert GOLDEN["pad_event"] == [2, 2]


def test_the_recorded_rows_hold_the_vectors():
    cols = GOLDEN["columns"]
    lo = int(cols["exponentiation_lo_hi"]["first"][0], 16), int(cols["exponentiation_lo_hi"]["first"][1], 16)
    assert lo[0] + (lo[1] << 128) == int(GOLDEN["exp_by_squaring"]["result"])
    # 3^13 starts behind the 11 steps of 23^123, outside the first 64 rows: its d column is checked through the model below
    m = ex.assign(EVENTS, N)
    o = 8 * 11
    assert [m["exponentiation_lo_hi"][o + 8 * j] for j in range(5)] == [s[2] for s in reversed(GOLDEN["steps_3_13"])]
    assert [m["mul_cols.0"][o + 8 * j] for j in range(5)] == [s[0] for s in reversed(GOLDEN["steps_3_13"])]
    pad = 8 * sum(GOLDEN["steps"])
    assert [m[c][pad] for c in ("is_last", "base_limb", "exponent_lo_hi", "exponentiation_lo_hi")] == [1, 2, 2, 4] and m["is_last"][pad + 8] == 1
    assert not any(m[c][pad + 16 + i] for c in ex.COLUMNS for i in range(13))


def test_the_line_by_line_model_gives_the_recorded_columns():
    check(ex.assign(EVENTS, N))


def test_the_closed_forms_give_the_recorded_columns():
    check(ex.closed(EVENTS, N))

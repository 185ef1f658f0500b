"""CPU: tests/golden/copy_rows_reference.json -- three copy events over real contract codes (a CODECOPY that starts in the middle of
a memory word, a RETURN that deploys a code, a SHA3 whose source runs past src_addr_end) with the columns of the copy circuit as
recorded from the line-by-line model -- against the model as it stands and against the closed forms that the device ops evaluate.
The file is data: nothing in it is executed."""
import hashlib
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import copy_rows_cases as cp  # noqa: E402

GOLDEN = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "copy_rows_reference.json")))
EVENTS, HEAP, N = GOLDEN["events"], bytes.fromhex(GOLDEN["heap"]), GOLDEN["rows"]
R_WORD, R_IN = int(GOLDEN["r_word"], 16), int(GOLDEN["r_in"], 16)


def digest(name, values):
    if name in cp.FR_COLUMNS:
        return hashlib.sha256(b"".join(v.to_bytes(32, "little") for v in values)).hexdigest()
    return hashlib.sha256(np.array(values, dtype="<u8" if name in cp.WORD_COLUMNS else "<u1").tobytes()).hexdigest()


def check(cols):
    assert set(GOLDEN["columns"]) == set(cp.INT_COLUMNS + cp.FR_COLUMNS)
    for name, rec in GOLDEN["columns"].items():
        first = [int(v, 16) for v in rec["first"]] if name in cp.FR_COLUMNS else rec["first"]
        assert len(first) == 64 and cols[name][:64] == first, name
        assert digest(name, cols[name]) == rec["sha256"], name


def test_the_events_are_the_three_shapes():
    assert [(e["src_tag"], e["dst_tag"], e["length"]) for e in EVENTS] == [(cp.BYTECODE, cp.MEMORY, 608), (cp.MEMORY, cp.BYTECODE, 96), (cp.MEMORY, cp.RLC_ACC, 160)]
    assert EVENTS[0]["dst_addr"] % 32 == 5 == EVENTS[0]["dst_front"] and N == 2 * (608 + 96 + 160) + 6
    assert EVENTS[2]["src_addr"] + 160 > EVENTS[2]["src_addr_end"] and GOLDEN["pad_rows"] == 160 - (5888 - 5792) and GOLDEN["masked_rows"] == 2 * (8 + 22) + 6
    assert all(cp.counts(e, len(HEAP)) and cp.rlc_is_the_references(e) for e in EVENTS)
    codes = [bytes.fromhex(c["code"]) for c in json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bytecode_rows_reference.json")))["contracts"]]
    small, middle, large = sorted(codes, key=len)
    assert HEAP[5:605] == middle[37:637] and HEAP[1216:1290] == small and HEAP[1312:1312 + 79] == large[5792:] and not any(HEAP[1312 + 79:])


def test_the_line_by_line_model_gives_the_recorded_columns():
    check(cp.assign(EVENTS, HEAP, N, R_WORD, R_IN))


def test_the_closed_forms_give_the_recorded_columns():
    check(cp.closed(EVENTS, HEAP, N, R_WORD, R_IN))

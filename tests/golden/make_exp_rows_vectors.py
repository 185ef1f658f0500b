"""Writes tests/golden/exp_rows_reference.json: the reference's own exponentiation vectors and the columns of the exponentiation
circuit for them, as the line-by-line model of tests/exp_rows_cases.py (assign) gives them.

usage: python tests/golden/make_exp_rows_vectors.py

The vectors: 23^123 and the five steps of 3^13 as bus-mapping/src/evm/opcodes/exp.rs:75-99 (test_exp_by_squaring) states them; the
exponent 0x1FFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFE to the base 2 of zkevm-circuits/src/exp_circuit/test.rs:91-97 (exp_circuit_big); the
default event (base 2, exponent 2) that assign_exp_events pads with.  The rows: those three events in that order in max_exp_rows =
8 x steps + 10 + 8 x 2 + 3 rows, so that two padding steps and thirteen zero rows follow.  The file holds data only: the events, and
for each of the 36 columns the first 64 rows in full and a SHA-256 over the whole column (every cell as 16 little-endian bytes).
tests/test_exp_rows_golden.py reads the JSON only."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import exp_rows_cases as ex  # noqa: E402

FIRST = 64
BIG = 0x1FFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFE


def main():
    events = [(23, 123), (3, 13), (2, BIG)]
    n = ex.rows_needed(events) + 8 * 2 + 3
    m = ex.assign(events, n)
    steps = []
    ex.exp_by_squaring(3, 13, steps)
    out = {
        "source": "bus-mapping/src/evm/opcodes/exp.rs:75-99 test_exp_by_squaring; zkevm-circuits/src/exp_circuit/test.rs:91-97 exp_circuit_big; ExpEvent::default()",
        "pins": "exp_circuit.rs:325-522 assign_exp_events, table.rs:2207-2271 ExpTable::assignments, gadgets mul_add.rs:261-415 MulAddChip::assign, range.rs:108-136: "
                "eight rows per step, last step of exp_by_squaring first, padding steps, ten unusable rows; every cell a canonical integer below 2^128",
        "exp_by_squaring": {"base": 23, "exponent": 123, "result": "87180413255890732361416772728849128389641993872302935967571352892955279939527"},
        "steps_3_13": [[3, 3, 9], [9, 3, 27], [27, 27, 729], [729, 729, 531441], [531441, 3, 1594323]],
        "big_exponent": hex(BIG), "pad_event": [2, 2],
        "events": [[hex(b), hex(x)] for b, x in events], "rows": n, "steps": [ex.steps_of(x) for _, x in events],
        "columns": {name: {"first": [hex(v) for v in m[name][:FIRST]], "sha256": ex.column_digest(m[name])} for name in ex.COLUMNS},
    }
    assert [list(s) for s in steps] == out["steps_3_13"]
    with open(os.path.join(HERE, "exp_rows_reference.json"), "w") as f:
        json.dump(out, f, separators=(",", ":"))
        f.write("\n")


if __name__ == "__main__":
    main()

"""Writes tests/golden/code_hash_rows_reference.json: for the three contract codes of bytecode_rows_reference.json and the five byte
strings of poseidon_code_hash.json, the eight columns of the bytecode circuit's Poseidon-hash extension and the code-hash rows of the
Poseidon table, as the line-by-line model of tests/code_hash_rows_cases.py assigns them, and the reference's own
bytecode_unrolling_to_input assertions with file:line.

usage: python tests/golden/make_code_hash_rows_vectors.py

The file holds data only: per column the first 64 rows in full (field elements and 16-byte cells as hex) and a SHA-256 over the whole
column as the device writes it (Montgomery Fr at 32 bytes, little-endian integers below).  The codes themselves are not repeated:
a record names its source record.  tests/test_code_hash_rows_golden.py reads the JSON only."""
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import code_hash_rows_cases as ch  # noqa: E402
import poseidon_cases as pc  # noqa: E402

FIRST = 64
REF = "bytecode_circuit/circuit/to_poseidon_hash.rs"
# fn bytecode_unrolling_to_input: unroll_to_hash_input::<Fr, bytes_in_field, input_len>(bt.take(take)) over bt = 1 .. 15
UNROLLING = [
    (f"{REF}:691-694", 4, 2, 6, [["0x01020304", "0x05060000"]]),
    (f"{REF}:696-701", 3, 2, 9, [["0x010203", "0x040506"], ["0x070809", "0x0"]]),
    (f"{REF}:703-708", 3, 2, 12, [["0x010203", "0x040506"], ["0x070809", "0x0a0b0c"]]),
    (f"{REF}:710-717", 3, 3, 12, [["0x010203", "0x040506", "0x070809"], ["0x0a0b0c", "0x0", "0x0"]]),
    (f"{REF}:719-726", 3, 3, 14, [["0x010203", "0x040506", "0x070809"], ["0x0a0b0c", "0x0d0e00", "0x0"]]),
]


def column(name, vals, widths):
    wide = widths[name] >= 16
    return {"first": [hex(v) if wide else v for v in vals[:FIRST]], "sha256": hashlib.sha256(ch.cells(name, vals, widths).tobytes()).hexdigest()}


def record(code, **about):
    n = len(code) + 2                                                    # header, bytes, one padding row
    rows = ch.assign([code], n)
    loaded, _ = ch.dev_load([code])
    k = len(loaded) + 1                                                  # and one row that is off
    table, needed = ch.table_closed([code], k)
    assert needed == len(loaded) and all((table["input0"][i], table["input1"][i], table["control"][i], table["heading_mark"][i]) == (r[0], r[1], r[2], r[4]) for i, r in enumerate(loaded))
    return dict(about, bytes=len(code), rows=n, table_rows=k, code_sha256=hashlib.sha256(code).hexdigest(), code_hash=hex(pc.code_hash(code)),
                columns={name: column(name, rows[name], ch.ROW_WIDTHS) for name in ch.ROW_COLUMNS},
                table={name: column(name, table[name], ch.TABLE_WIDTHS) for name in ch.TABLE_COLUMNS})


def main():
    base = json.load(open(os.path.join(HERE, "bytecode_rows_reference.json")))
    pos = json.load(open(os.path.join(HERE, "poseidon_code_hash.json")))["vectors"]
    out = {
        "source": "the codes of bytecode_rows_reference.json contracts[] and of poseidon_code_hash.json vectors[], in that order",
        "pins": REF + ":412-645 (assign_internal, set_header_row, assign_extended_row), bytecode_unroller.rs:68-124, table.rs:1081-1139; rows = header, "
                "one per byte, one padding row; table rows = ceil(bytes / 62) and one that is off; widths " + json.dumps({**ch.ROW_WIDTHS, **ch.TABLE_WIDTHS}, sort_keys=True),
        "contracts": [record(bytes.fromhex(c["code"]), entry=c["entry"]) for c in base["contracts"]],
        "poseidon_vectors": [record(bytes.fromhex(v["code"]), ref=v["ref"], hash=v["hash"]) for v in pos],
        "unrolling_assertions": [dict(ref=ref, bytes_in_field=f, input_len=w, take=take, out=rows) for ref, f, w, take, rows in UNROLLING],
    }
    with open(os.path.join(HERE, "code_hash_rows_reference.json"), "w") as f:
        json.dump(out, f, separators=(",", ":"))
        f.write("\n")


if __name__ == "__main__":
    main()

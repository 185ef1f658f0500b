"""Writes tests/golden/bytecode_rows_reference.json: real contract codes out of a block trace of the reference's test data and the
bytecode circuit's integer columns for each of them, as the line-by-line model of tests/bytecode_rows_cases.py assigns them.

usage: python tests/golden/make_bytecode_rows_vectors.py <reference checkout>/eth-types/src/testdata/trace_v2_5224657.json

The file holds data only: the code bytes, for every integer column the first 64 rows in full and a SHA-256 over the whole column (its
cells little-endian at the column's width), and the number of is_code rows.  The five byte strings of poseidon_code_hash.json ride
along with the same records.  tests/test_bytecode_rows_golden.py reads the JSON only."""
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import bytecode_rows_cases as bc  # noqa: E402

ENTRIES = (8, 6, 1)                          # codes[] of the trace: 74, 1852 and 5871 bytes
FIRST = 64


def record(code, **about):
    n = len(code) + 2                        # header, bytes, one padding row
    m = bc.assign([code], [0], n, 0)
    cols = {}
    for name in bc.INT_COLUMNS:
        cells = np.array(m[name], dtype={1: np.uint8, 4: np.uint32}[bc.INT_WIDTHS[name]])
        cols[name] = {"first": m[name][:FIRST], "sha256": hashlib.sha256(cells.astype(cells.dtype.newbyteorder("<")).tobytes()).hexdigest()}
    return dict(about, code=code.hex(), bytes=len(code), rows=n, is_code_rows=sum(m["is_code"]), columns=cols)


def main(trace_path):
    trace = json.load(open(trace_path))
    codes = trace.get("result", trace)["codes"]
    out = {
        "source": "eth-types/src/testdata/trace_v2_5224657.json, codes[] entries " + ", ".join(map(str, ENTRIES)),
        "pins": "bytecode_circuit/bytecode_unroller.rs:32-60 and circuit.rs:666-835: rows = header, one per byte, one padding row; widths "
                + json.dumps(bc.INT_WIDTHS, sort_keys=True),
        "contracts": [record(bytes.fromhex(codes[i]["code"][2:]), entry=i, hash=codes[i]["hash"]) for i in ENTRIES],
        "poseidon_vectors": [record(bytes.fromhex(v["code"]), ref=v["ref"]) for v in json.load(open(os.path.join(HERE, "poseidon_code_hash.json")))["vectors"]],
    }
    with open(os.path.join(HERE, "bytecode_rows_reference.json"), "w") as f:
        json.dump(out, f, separators=(",", ":"))
        f.write("\n")


if __name__ == "__main__":
    main(sys.argv[1])

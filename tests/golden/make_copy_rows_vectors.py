"""Writes tests/golden/copy_rows_reference.json: three copy events built from the real contract codes of
tests/golden/bytecode_rows_reference.json and the columns of the copy circuit for them, as the line-by-line model of
tests/copy_rows_cases.py (assign) gives them under two fixed challenges.

usage: python tests/golden/make_copy_rows_vectors.py

The events: a CODECOPY-shaped Bytecode -> Memory copy of 600 bytes of the 1 852-byte code to memory address 0x45, which starts in the
middle of a word (five masked steps at the front, three at the back); a RETURN-shaped Memory -> Bytecode copy that deploys the 74-byte
code out of three memory words (22 masked steps at the back); a SHA3-shaped Memory -> RlcAcc read of 160 bytes from address 5 792 of a
memory that holds the 5 871-byte code and ends at 5 888, so that the source runs past src_addr_end.  The file holds data only: the
event records and the byte heap, the two challenges, and for every column the first 64 rows in full and a SHA-256 over the whole
column (integer cells little-endian at the column's width, field elements as 32 little-endian bytes of the canonical integer).
tests/test_copy_rows_golden.py reads the JSON only."""
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import copy_rows_cases as cp  # noqa: E402

FIRST = 64
R_WORD = 0x1F2E3D4C5B6A79880796A5B4C3D2E1F00112233445566778899AABBCCDDEEFF % cp.R
R_IN = 0x0123456789ABCDEFFEDCBA98765432100F1E2D3C4B5A69788796A5B4C3D2E1F % cp.R
WIDTHS = {name: 8 if name in cp.WORD_COLUMNS else 1 for name in cp.INT_COLUMNS}


def build():
    contracts = json.load(open(os.path.join(HERE, "bytecode_rows_reference.json")))["contracts"]
    small, middle, large = (bytes.fromhex(c["code"]) for c in sorted(contracts, key=lambda c: c["bytes"]))
    assert (len(small), len(middle), len(large)) == (74, 1852, 5871)
    rng = np.random.default_rng(0x31)
    # CODECOPY: memory words 0x40 .. 0x2a0 after the write, and before it
    before = bytes(rng.integers(0, 256, 608, dtype=np.uint8))
    after = before[:5] + middle[37:637] + before[605:]
    # RETURN: three memory words that hold the 74 bytes of the code to deploy
    words = small + bytes(rng.integers(0, 256, 22, dtype=np.uint8))
    # SHA3: the last words of a memory that holds the large code, zeros behind its end
    tail = large[5792:] + bytes(160 - (5871 - 5792))
    heap = after + before + words + tail
    events = [
        cp.event(608, cp.BYTECODE, cp.MEMORY, src_addr=37, src_addr_end=1852, dst_addr=0x45, rw_counter=1001, src_off=0, dst_off=0, prev_off=608, src_front=5, src_back=3,
                 src_id=int(sorted(contracts, key=lambda c: c["bytes"])[1]["hash"], 16) % cp.R, dst_id=7),
        cp.event(96, cp.MEMORY, cp.BYTECODE, src_addr=0x20, src_addr_end=0x1000, dst_addr=0, rw_counter=1020, src_off=1216, dst_off=1216, prev_off=1216, src_back=22,
                 src_id=7, dst_id=int(sorted(contracts, key=lambda c: c["bytes"])[0]["hash"], 16) % cp.R),
        cp.event(160, cp.MEMORY, cp.RLC_ACC, src_addr=5792, src_addr_end=5888, dst_addr=0, rw_counter=1023, src_off=1312, dst_off=1312, prev_off=1312, src_id=9, dst_id=1023),
    ]
    return events, heap


def main():
    events, heap = build()
    n = sum(2 * e["length"] for e in events) + 6
    m = cp.assign(events, heap, n, R_WORD, R_IN)
    cols = {}
    for name in cp.INT_COLUMNS:
        cells = np.array(m[name], dtype={1: "<u1", 8: "<u8"}[WIDTHS[name]])
        cols[name] = {"first": m[name][:FIRST], "sha256": hashlib.sha256(cells.tobytes()).hexdigest()}
    for name in cp.FR_COLUMNS:
        cols[name] = {"first": [hex(v) for v in m[name][:FIRST]], "sha256": hashlib.sha256(b"".join(v.to_bytes(32, "little") for v in m[name])).hexdigest()}
    out = {
        "source": "the codes of tests/golden/bytecode_rows_reference.json (eth-types/src/testdata/trace_v2_5224657.json, codes[] entries 8, 6, 1)",
        "pins": "table.rs:1802-2065 CopyTable::assignments, copy_circuit.rs:676-841 assign_copy_event, :944-1151 assign_padding_row: two rows per step, then padding rows; "
                "integer cells little-endian at widths " + json.dumps(WIDTHS, sort_keys=True) + "; field elements as canonical integers",
        "events": events, "heap": heap.hex(), "rows": n, "r_word": hex(R_WORD), "r_in": hex(R_IN),
        "pad_rows": sum(m["is_pad"]), "masked_rows": sum(m["mask"]), "columns": cols,
    }
    with open(os.path.join(HERE, "copy_rows_reference.json"), "w") as f:
        json.dump(out, f, separators=(",", ":"))
        f.write("\n")


if __name__ == "__main__":
    main()

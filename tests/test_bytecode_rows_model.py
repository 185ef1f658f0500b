"""CPU: the model of tests/bytecode_rows_cases.py against itself.  The two kind columns that ZK_OP_BYTECODE_ROWS writes, run through
the scans ZK_OP_SCAN_RLC and ZK_OP_SCAN_RLC_REV compute (z_i = m z_(i-1) + w cell_i under the tables of the cases file), reproduce
push_acc and push_rlc of the reference's assignment loop -- make_push_rlc's accumulator and the value held on every row of the
instruction -- on random sets of bytecodes and on the edges: truncated pushes, empty codes, headers directly behind push data, pushes
inside push data.  value_rlc is the plain forward scan with tag as the kind.  The vectorised integer columns (rows_numpy) are the
assignment loop's."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import bytecode_rows_cases as bc  # noqa: E402

R = bc.R
EVM_WORD, KECCAK_INPUT = 0x1234567890ABCDEF1234567890ABCDEF % R, (R - 3)
EDGES = [
    [bytes([0x7f])],
    [bytes([0x7f, 0x01])],
    [bytes([0x7f] + [0x60] * 31)],
    [bytes([0x7f] + [0x60] * 32)],
    [bytes([0x7f] + [0x60] * 33)],
    [bytes([0x7f] * 200)],
    [bytes([0x60] * 200)],
    [bytes([0x60])],
    [b""],
    [b"", b"", b""],
    [bytes([0x7f, 0x60, 0x60]), bytes([0x61, 0xaa, 0xbb, 0x00]), b"", bytes([0x7f])],
    [bytes([0x61, 0x7f]), bytes([0x7f, 0x7f])],
    [bytes([0x00, 0x5f, 0x80, 0x60, 0x7f, 0x7f])],
]


def check(codes, extra=0):
    n = sum(len(c) + 1 for c in codes) + extra
    m = bc.assign(codes, list(range(100, 100 + len(codes))), n, 77, evm_word=EVM_WORD, keccak_input=KECCAK_INPUT)
    acc = bc.scan(m["acc_kinds"], m["value"], bc.acc_table(EVM_WORD))
    assert acc == m["push_acc"]
    assert bc.scan(m["rlc_kinds"], acc, bc.rlc_table(), reverse=True) == m["push_rlc"]
    assert bc.scan(m["tag"], m["value"], {bc.HEADER: (0, 0), bc.BYTE: (KECCAK_INPUT, 1)}) == m["value_rlc"]
    assert m["is_code"] == [int(t == bc.BYTE and left == 0) for t, left in zip(m["tag"], m["push_data_left"])]
    for v, inv in zip(m["push_data_left"], m["push_data_left_inv"]):
        assert v * inv % R == (1 if v else 0)
    for i, ln, inv in zip(m["index"], m["length"], m["index_length_diff_inv"]):
        assert (i + 1 - ln) * inv % R == (1 if (i + 1 - ln) % R else 0)
    assert m["code_hash"] == [h for b, c in enumerate(codes) for h in [100 + b] * (len(c) + 1)] + [77] * extra
    w = bc.rows_numpy(codes, n)
    for name in bc.INT_COLUMNS:
        assert w[name].tolist() == m[name], name
    return m


def test_kind_values_and_tables():
    assert (bc.ACC_NONE, bc.ACC_DATA, bc.RLC_NONE, bc.RLC_TAKE, bc.RLC_COPY) == (0, 1, 0, 1, 2)
    assert bc.acc_table(5) == {0: (0, 0), 1: (5, 1)} and bc.rlc_table() == {0: (0, 0), 1: (0, 1), 2: (1, 0)}
    assert [bc.get_push_size(v) for v in (0x5f, 0x60, 0x7f, 0x80, 0, 255)] == [0, 1, 32, 0, 0, 0]


def test_edges():
    for codes in EDGES:
        check(codes)
        check(codes, extra=5)
    m = check([bytes([0x61, 0xaa])], extra=1)                            # PUSH2 with one byte: push_rlc is the RLC of that byte
    assert m["push_rlc"] == [0, 0xaa, 0xaa, 0] and m["push_acc"] == [0, 0, 0xaa, 0] and m["rlc_kinds"] == [0, 2, 1, 0]
    m = check([bytes([0x60])])                                          # a push at the very end has no data row
    assert m["push_rlc"] == [0, 0] and m["rlc_kinds"] == [0, 0]


def test_random_sets_of_bytecodes():
    rng = np.random.default_rng(0xC0DE)
    for t in range(300):
        codes = [bc.random_code(rng, int(k), push_share=float(rng.choice([0.1, 0.4, 0.9]))) for k in rng.integers(0, 120, int(rng.integers(1, 7)))]
        check(codes, extra=int(rng.integers(0, 4)))


def test_a_cut_bytecode_keeps_the_rows_below_n():
    rng = np.random.default_rng(3)
    codes = [bc.random_code(rng, 90), bc.random_code(rng, 90)]
    full = bc.assign(codes, [1, 2], 182, 9)
    for n in (0, 1, 50, 91, 92, 150, 181):
        cut = bc.assign(codes, [1, 2], n, 9, fail_fast=False)
        for name in bc.INT_COLUMNS + ("code_hash",):
            assert cut[name] == full[name][:n], (n, name)
        try:
            bc.assign(codes, [1, 2], n, 9)
            assert False, "Error::Synthesis"
        except OverflowError:
            pass

"""The Poseidon-hash extension of the bytecode circuit and the code-hash rows of the Poseidon table in Python: line by line after the
reference, and beside it the closed forms that ZK_OP_CODE_HASH_ROWS and ZK_OP_CODE_HASH_TABLE evaluate.  No GPU, no library.

assign restates zkevm-circuits/src/bytecode_circuit/circuit/to_poseidon_hash.rs:412-494 (assign_internal) with set_header_row
(:497-543) and assign_extended_row (:547-645) and its carried row_input; unroll_to_hash_input restates
bytecode_circuit/bytecode_unroller.rs:68-124, dev_load restates table.rs:1081-1139 (PoseidonTable::dev_load).  The field width and the
input width are parameters there, because the reference's own assertions (to_poseidon_hash.rs:688-727) use 3- and 4-byte fields;
everything else uses 31 and 2.
"""
import functools

import numpy as np

from oracle import bn254

R = bn254.R_MOD
F, INPUT_WIDTH = 31, 2                                   # HASHBLOCK_BYTES_IN_FIELD, PoseidonTable::INPUT_WIDTH
W = F * INPUT_WIDTH
HASHABLE_DOMAIN_SPEC = 1 << 64
HEADER, BYTE = 0, 1
HEAD, CONT, OFF = 0, 1, 2                                # the kinds of ZK_OP_POSEIDON

ROW_COLUMNS = ("control_length", "field_input", "bytes_in_field_index", "bytes_in_field_inv", "is_field_border", "padding_shift", "field_index", "field_index_inv")
ROW_WIDTHS = {"control_length": 4, "field_input": 32, "bytes_in_field_index": 1, "bytes_in_field_inv": 32, "is_field_border": 1, "padding_shift": 32,
              "field_index": 1, "field_index_inv": 1}
TABLE_COLUMNS = ("input0", "input1", "control", "heading_mark", "kinds", "cap")
TABLE_WIDTHS = {"input0": 32, "input1": 32, "control": 16, "heading_mark": 1, "kinds": 1, "cap": 8}
LENGTHS = (0, 1, 30, 31, 32, 61, 62, 63, 93, 124, 125, 500)


def inv0(v):
    return pow(v % R, -1, R) if v % R else 0


# ---- the reference, line by line ------------------------------------------------------------------------------------------------------
def assign(codes, n, bytes_in_field=F, input_width=INPUT_WIDTH):
    """to_poseidon_hash.rs:412-494 over n rows without fail_fast: a dict of the eight columns, each a list of n Python ints.  The
    rows at or after n are dropped (:464: only offsets up to last_row_offset are assigned), which is what the device op does."""
    cols = {name: [0] * n for name in ROW_COLUMNS}

    def set_header_row(code_length, offset):                             # :497-543
        for name in ("field_input", "bytes_in_field_index", "bytes_in_field_inv", "is_field_border", "field_index_inv"):   # :503-519
            cols[name][offset] = 0
        cols["control_length"][offset] = code_length                     # :522-526
        cols["padding_shift"][offset] = pow(256, bytes_in_field, R)      # :527-531
        cols["field_index"][offset] = 1                                  # :532

    def assign_extended_row(offset, tag, code_index, value, input_prev, code_length):   # :547-645
        if tag == BYTE:                                                  # :558
            block_size = bytes_in_field * input_width                    # :559
            prog_block = code_index // block_size                        # :561
            control_length = code_length - prog_block * block_size       # :562
            bytes_in_field_index = (code_index + 1) % bytes_in_field     # :563
            field_border = bytes_in_field_index == 0                     # :564
            if field_border:                                             # :565-569
                bytes_in_field_index = bytes_in_field
            bytes_in_field_index_inv_f = inv0(bytes_in_field - bytes_in_field_index)   # :570-573
            padding_shift_f = pow(256, bytes_in_field - bytes_in_field_index, R)       # :574-575
            input_f = (value * padding_shift_f + input_prev) % R         # :576
            field_border = field_border or code_index + 1 == code_length   # :578
            field_index = (code_index % block_size) // bytes_in_field + 1   # :580
            field_index_inv_f = inv0(input_width - field_index)          # :581-583
            cols["control_length"][offset] = control_length              # :596-628
            cols["field_input"][offset] = input_f
            cols["bytes_in_field_index"][offset] = bytes_in_field_index
            cols["bytes_in_field_inv"][offset] = bytes_in_field_index_inv_f
            cols["is_field_border"][offset] = int(field_border)
            cols["padding_shift"][offset] = padding_shift_f
            cols["field_index"][offset] = field_index
            cols["field_index_inv"][offset] = field_index_inv_f
            return 0 if field_border else input_f                        # :630-634
        set_header_row(code_length, offset)                              # :636-639
        return 0

    offset = 0                                                           # :443
    row_input = 0                                                        # :444
    for code in codes:                                                   # :445
        begin = offset                                                   # :446
        rows = [(HEADER, 0, len(code))] + [(BYTE, i, v) for i, v in enumerate(code)]   # the unroller's rows
        offset = min(begin + len(rows), n)                               # :447-457: assign_bytecode without fail_fast stops at the last row
        for idx, (tag, index, value) in enumerate(rows):                 # :459
            if begin + idx < n:                                          # :464
                row_input = assign_extended_row(begin + idx, tag, index, value, row_input, len(code))   # :465-471
    for idx in range(offset, n):                                         # :477
        set_header_row(0, idx)                                           # :486
    return cols


def unroll_to_hash_input(code, bytes_in_field=F, input_len=INPUT_WIDTH):
    """bytecode_unroller.rs:68-124: rows of input_len field elements"""
    code = bytes(code)
    fl_cnt = len(code) // bytes_in_field                                 # :71
    if len(code) % bytes_in_field:                                       # :72-76
        fl_cnt += 1
    padded = code + bytes(fl_cnt * bytes_in_field - len(code))           # :78-80
    msgs = [int.from_bytes(padded[i:i + bytes_in_field], "big") % R for i in range(0, len(padded), bytes_in_field)]   # :81-90
    input_cnt = len(msgs) // input_len                                   # :92
    if len(msgs) % input_len:                                            # :93-97
        input_cnt += 1
    if input_cnt == 0:                                                   # :98-100
        return []
    msgs += [0] * (input_cnt * input_len - len(msgs))                    # :102-105
    return [msgs[i:i + input_len] for i in range(0, len(msgs), input_len)]   # :106-123


def dev_load(codes):
    """table.rs:1081-1139 behind the two leading rows: rows of (input0, input1, control, domain_spec, heading_mark) per code, and the
    index of the code each row belongs to.  hash_id is the caller's (poseidon_cases.code_hash)."""
    rows, owner = [], []
    for b, code in enumerate(codes):                                     # :1081
        control_len = len(code)                                          # :1082
        first_row = True                                                 # :1083
        for row in unroll_to_hash_input(code):                           # :1090
            assert control_len != 0, "must have enough len left"         # :1091-1096
            block_size = F * len(row)                                    # :1097
            control_len_as_flag = HASHABLE_DOMAIN_SPEC * control_len     # :1098-1099
            rows.append((row[0], row[1], control_len_as_flag, 0, int(first_row)))   # :1107-1117
            owner.append(b)
            first_row = False                                            # :1126
            control_len = control_len - block_size if control_len > block_size else 0   # :1128-1132
        assert control_len == 0, "should have exhaust all bytes"         # :1134-1139
    return rows, owner


# ---- the closed forms -------------------------------------------------------------------------------------------------------------------
def header_row(length):
    return dict(control_length=length, field_input=0, bytes_in_field_index=0, bytes_in_field_inv=0, is_field_border=0, padding_shift=pow(256, F, R), field_index=1,
                field_index_inv=0)


def byte_row(code, p):
    m, length = p % F, len(code)
    return dict(control_length=length - W * (p // W), field_input=sum(code[p - m + t] * 256**(F - 1 - t) for t in range(m + 1)), bytes_in_field_index=m + 1,
                bytes_in_field_inv=inv0(F - 1 - m), is_field_border=int(m == F - 1 or p + 1 == length), padding_shift=pow(256, F - 1 - m, R),
                field_index=p // F % 2 + 1, field_index_inv=1 - p // F % 2)


def rows_closed(codes, n):
    """the eight columns by the closed forms, cut at n"""
    cols = {name: [] for name in ROW_COLUMNS}
    for code in codes:
        for row in [header_row(len(code))] + [byte_row(code, p) for p in range(len(code))]:
            if len(cols["field_input"]) < n:
                for name in ROW_COLUMNS:
                    cols[name].append(row[name])
    while len(cols["field_input"]) < n:
        for name, v in header_row(0).items():
            cols[name].append(v)
    return cols


def table_closed(codes, n):
    """the table's columns by the closed forms over n rows, and the unsaturated number of rows"""
    cols = {name: [] for name in TABLE_COLUMNS}
    needed = 0
    for code in codes:
        length = len(code)
        blocks = -(-length // W)
        needed += blocks
        for j in range(blocks):
            if len(cols["input0"]) >= n:
                break
            cols["input0"].append(int.from_bytes(bytes(code[W * j:W * j + F]).ljust(F, b"\0"), "big"))
            cols["input1"].append(int.from_bytes(bytes(code[W * j + F:W * j + W]).ljust(F, b"\0"), "big"))
            cols["control"].append((length - W * j) * HASHABLE_DOMAIN_SPEC)
            cols["heading_mark"].append(int(j == 0))
            cols["kinds"].append(HEAD if j == 0 else CONT)
            cols["cap"].append(length)
    while len(cols["input0"]) < n:
        for name in TABLE_COLUMNS:
            cols[name].append(OFF if name == "kinds" else 0)
    return cols, needed


# ---- as the device writes them --------------------------------------------------------------------------------------------------------------
def to_mont(vals):
    """(len, 4) uint64 Montgomery Fr of Python ints"""
    return np.array([[(v % R << 256) % R >> (64 * j) & (2**64 - 1) for j in range(4)] for v in vals], dtype=np.uint64).reshape(len(vals), 4)


def cells(name, vals, widths):
    """the column as the bytes the device writes: Montgomery Fr at 32, little-endian integers below (control_length mod 2^32)"""
    width = widths[name]
    if width == 32:
        return to_mont(vals).view(np.uint8).reshape(-1)
    if width == 16:
        return np.array([[v & (2**64 - 1), v >> 64] for v in vals], dtype="<u8").reshape(-1).view(np.uint8)
    return np.array([v % 2**(8 * width) for v in vals], dtype={1: "<u1", 4: "<u4", 8: "<u8"}[width]).view(np.uint8)


@functools.lru_cache(maxsize=1 << 17)
def field_mont(chunk):
    """the bytes of a field up to a row's own (or a whole field of the table, cut at the end of the code) as the 32 bytes of the
    Montgomery image of their big-endian integer, left-aligned in 31 bytes"""
    return ((int.from_bytes(chunk.ljust(F, b"\0"), "big") << 256) % R).to_bytes(32, "little")


_TABLES = None


def rows_numpy(codes, n):
    """the eight columns as device bytes for large inputs, vectorised over the rows where the structure allows it (the timing tool's
    host route, the alignment sweeps and the large GPU case); checked against rows_closed on the CPU"""
    global _TABLES
    if _TABLES is None:
        _TABLES = (to_mont([pow(256, k, R) for k in range(F + 1)]), to_mont([inv0(k) for k in range(F)]))
    pow_tab, inv_tab = _TABLES
    kind = np.zeros(n, np.uint8); pos = np.zeros(n, np.int64); length = np.zeros(n, np.int64)
    fields, at = [], 0
    for code in codes:
        if at >= n:
            break
        code = bytes(code)
        ln = len(code)
        take = min(ln, n - at - 1)
        kind[at] = 1
        length[at:at + 1 + take] = ln
        kind[at + 1:at + 1 + take] = 2
        pos[at + 1:at + 1 + take] = np.arange(take, dtype=np.int64)
        fields.append(bytes(32))
        fields += [field_mont(code[p - p % F:p + 1]) for p in range(take)]   # the serial part a host has
        at += 1 + take
    fields.append(bytes(32 * (n - at)))
    byte = kind == 2
    m = pos % F
    second = pos // F % 2
    out = {}
    out["field_input"] = np.frombuffer(b"".join(fields), dtype=np.uint8)
    out["control_length"] = np.where(byte, length - W * (pos // W), np.where(kind == 1, length, 0)).astype("<u4").view(np.uint8)
    out["bytes_in_field_index"] = np.where(byte, m + 1, 0).astype(np.uint8)
    out["is_field_border"] = (byte & ((m == F - 1) | (pos + 1 == length))).astype(np.uint8)
    out["field_index"] = np.where(byte, second + 1, 1).astype(np.uint8)
    out["field_index_inv"] = np.where(byte, 1 - second, 0).astype(np.uint8)
    out["padding_shift"] = pow_tab[np.where(byte, F - 1 - m, F)].view(np.uint8).reshape(-1)
    out["bytes_in_field_inv"] = inv_tab[np.where(byte, F - 1 - m, 0)].view(np.uint8).reshape(-1)
    return out


def table_numpy(codes, n):
    """the table's columns as device bytes, and the unsaturated number of rows; checked against table_closed on the CPU"""
    in0, in1, lens, js = [], [], [], []
    needed = 0
    for code in codes:
        code = bytes(code)
        blocks = -(-len(code) // W)
        needed += blocks
        take = min(blocks, n - len(lens))
        in0 += [field_mont(code[W * j:W * j + F]) for j in range(take)]
        in1 += [field_mont(code[W * j + F:W * j + W]) for j in range(take)]
        lens += [len(code)] * take
        js += list(range(take))
    used = len(lens)
    ln = np.array(lens + [0] * (n - used), dtype=np.uint64)
    j = np.array(js + [0] * (n - used), dtype=np.uint64)
    owned = np.arange(n) < used
    out = {}
    out["input0"] = np.frombuffer(b"".join(in0) + bytes(32 * (n - used)), dtype=np.uint8)
    out["input1"] = np.frombuffer(b"".join(in1) + bytes(32 * (n - used)), dtype=np.uint8)
    control = np.zeros((n, 2), dtype="<u8")
    control[:, 1] = np.where(owned, ln - np.uint64(W) * j, 0)
    out["control"] = control.reshape(-1).view(np.uint8)
    out["heading_mark"] = (owned & (j == 0)).astype(np.uint8)
    out["kinds"] = np.where(owned, np.where(j == 0, HEAD, CONT), OFF).astype(np.uint8)
    out["cap"] = ln.astype("<u8").view(np.uint8)
    return out, needed


def lay_out(codes, rng=None, gap=0):
    """codes laid end to end (gap bytes of filler between them): the byte buffer, offsets, lengths"""
    buf, offs, lens = bytearray(), [], []
    for code in codes:
        if gap:
            buf += bytes(rng.integers(0, 256, gap, dtype=np.uint8)) if rng is not None else bytes(gap)
        offs.append(len(buf))
        lens.append(len(code))
        buf += bytes(code)
    return np.frombuffer(bytes(buf), dtype=np.uint8).copy(), offs, lens


def random_code(rng, length):
    """random bytes without a zero, so that a byte read from the wrong place or a padding byte taken for code shows"""
    return bytes(rng.integers(1, 256, length, dtype=np.uint8))

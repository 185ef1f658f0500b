"""The bytecode circuit's witness in Python, line by line after the reference, and what ZK_OP_BYTECODE_ROWS adds to it: the two kind
columns and the scan tables from which ZK_OP_SCAN_RLC and ZK_OP_SCAN_RLC_REV make push_acc and push_rlc.  No GPU, no library.

unroll_with_codehash restates zkevm-circuits/src/bytecode_circuit/bytecode_unroller.rs:32-60, assign restates
bytecode_circuit/circuit.rs:666-835 (assign_bytecode, make_push_rlc, set_padding_row) with the padding loop of circuit.rs:594-604.  The
two are the reference's two independent formulations of is_code -- the unroller's push_rindex and the assignment loop's push_data_left
-- and assign asserts on every byte row that they agree.
"""
import numpy as np

from oracle import bn254

R = bn254.R_MOD
HEADER, BYTE = 0, 1                                    # table.rs: BytecodeFieldTag

# the kinds of d_acc_kinds and d_rlc_kinds and the (m, w) tables of the scans: z_i = m * z_(i-1) + w * cell_i (reverse: z_(i+1))
ACC_NONE, ACC_DATA = 0, 1
RLC_NONE, RLC_TAKE, RLC_COPY = 0, 1, 2
INT_COLUMNS = ("tag", "index", "value", "is_code", "push_data_left", "push_data_size", "length", "acc_kinds", "rlc_kinds")
INT_WIDTHS = {"tag": 1, "index": 4, "value": 4, "is_code": 1, "push_data_left": 1, "push_data_size": 1, "length": 4, "acc_kinds": 1, "rlc_kinds": 1}


def acc_table(r):
    """push_acc = ZK_OP_SCAN_RLC over the value column, z0 = 0"""
    return {ACC_NONE: (0, 0), ACC_DATA: (r % R, 1)}


def rlc_table():
    """push_rlc = ZK_OP_SCAN_RLC_REV over the push_acc column, z0 = 0"""
    return {RLC_NONE: (0, 0), RLC_TAKE: (0, 1), RLC_COPY: (1, 0)}


def get_push_size(byte):
    """util.rs get_push_size: PUSH1 .. PUSH32 are 0x60 .. 0x7f"""
    return byte - 0x5f if 0x60 <= byte <= 0x7f else 0


def unroll_with_codehash(code_hash, code):
    """bytecode_unroller.rs:32-60: rows of (code_hash, tag, index, is_code, value)"""
    rows = [(code_hash, HEADER, 0, 0, len(code))]                        # :33-39
    push_rindex = 0                                                     # :41
    for index, byte in enumerate(code):                                 # :42
        is_code = push_rindex == 0                                      # :44
        push_rindex = get_push_size(byte) if is_code else push_rindex - 1   # :45-49
        rows.append((code_hash, BYTE, index, int(is_code), byte))       # :51-57
    return rows


def make_push_rlc(rand, values):
    """circuit.rs:795-805: the RLC of a slice of byte values and the accumulator after each"""
    acc, inter = 0, []
    for v in values:
        acc = (acc * rand + v) % R                                      # :800
        inter.append(acc)
    return acc, inter


def assign(codes, hashes, n, empty_hash, evm_word=0, keccak_input=0, fail_fast=True):
    """circuit.rs:579-604 with assign_bytecode (:666-792) and set_padding_row (:807-835) over n rows: a dict of columns, each a list
    of n Python ints.  hashes[b]: the code hash cell of bytecode b as a field element (the caller's build decides what it is).  A
    bytecode that does not fit raises with fail_fast (:698-705, Error::Synthesis); without it the rows at or after n are dropped, which
    is what the device op does."""
    names = ("code_hash", "tag", "index", "is_code", "value", "push_data_left", "push_acc", "push_rlc", "value_rlc", "length", "push_data_size")
    cols = {name: [] for name in names}

    def set_row(*cells):                                                # :838-: the advice cells of one row
        for name, cell in zip(names, cells):
            cols[name].append(cell)

    for code, code_hash in zip(codes, hashes):
        rows = unroll_with_codehash(code_hash, code)
        push_data_left = next_push_data_left = push_data_size = 0       # :679-681
        push_acc_iter = iter(())                                        # :682
        push_rlc = 0                                                    # :683
        value_rlc = 0                                                   # :684
        length = len(code)                                              # :685
        for idx, (_, tag, index, row_is_code, value) in enumerate(rows):    # :697
            if len(cols["tag"]) >= n:                                   # :698
                if fail_fast:
                    raise OverflowError("Error::Synthesis: the bytecodes do not fit")
                break
            push_acc = next(push_acc_iter, 0)                           # :707
            if idx > 0:                                                 # :709
                is_code = push_data_left == 0                           # :710
                assert int(is_code) == row_is_code, "the unroller's is_code is push_data_left == 0"
                push_data_size = get_push_size(value)                   # :712
                next_push_data_left = push_data_size if is_code else push_data_left - 1   # :714-718
                if is_code:                                             # :720
                    start = idx + 1                                     # :722
                    end = min(start + push_data_size, len(rows))        # :723
                    push_rlc, inter = make_push_rlc(evm_word, [r[4] for r in rows[start:end]])   # :724-727
                    push_acc_iter = iter(inter)                         # :729
                value_rlc = (value_rlc * keccak_input + value) % R      # :732-735
            set_row(code_hash % R, tag, index, row_is_code, value, push_data_left, push_acc, push_rlc, value_rlc, length, push_data_size)   # :740-758
            push_data_left = next_push_data_left                        # :777
    while len(cols["tag"]) < n:                                         # :595-604
        set_row(empty_hash % R, HEADER, 0, 0, 0, 0, 0, 0, 0, 0, 0)      # :816-834
    # the two IsZero gadgets (circuit.rs set_row: push_data_left_inv, index_length_diff_inv over index + 1 - length)
    cols["push_data_left_inv"] = [pow(v, -1, R) if v % R else 0 for v in cols["push_data_left"]]
    cols["index_length_diff_inv"] = [pow((i + 1 - ln) % R, -1, R) if (i + 1 - ln) % R else 0 for i, ln in zip(cols["index"], cols["length"])]
    cols["acc_kinds"], cols["rlc_kinds"] = kinds(cols)
    return cols


def kinds(cols):
    """the kind columns, defined on the columns of the assignment alone"""
    acc, rlc = [], []
    for tag, index, length, left, size in zip(cols["tag"], cols["index"], cols["length"], cols["push_data_left"], cols["push_data_size"]):
        data = tag == BYTE and left > 0
        last = index == length - 1
        acc.append(ACC_DATA if data else ACC_NONE)
        if data:
            rlc.append(RLC_TAKE if left == 1 or last else RLC_COPY)
        elif tag == BYTE and size > 0 and not last:
            rlc.append(RLC_COPY)
        else:
            rlc.append(RLC_NONE)
    return acc, rlc


def scan(kinds_col, cells, table, reverse=False, z0=0):
    """ZK_OP_SCAN_RLC / ZK_OP_SCAN_RLC_REV: z_i = m(kind_i) * z_(i-1) + w(kind_i) * cell_i, from z0"""
    out, z = [0] * len(cells), z0 % R
    order = range(len(cells) - 1, -1, -1) if reverse else range(len(cells))
    for i in order:
        m, w = table[kinds_col[i]]
        z = (m * z + w * cells[i]) % R
        out[i] = z
    return out


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


def random_code(rng, length, push_share=0.3):
    """bytes with many pushes: every byte is a PUSH1 .. PUSH32 with probability push_share"""
    code = rng.integers(0, 256, length, dtype=np.uint8)
    push = rng.random(length) < push_share
    code[push] = rng.integers(0x60, 0x80, int(push.sum()), dtype=np.uint8)
    return bytes(code)


def to_mont(vals):
    """(len, 4) uint64 Montgomery Fr of Python ints"""
    return np.array([[(v % R << 256) % R >> (64 * j) & (2**64 - 1) for j in range(4)] for v in vals], dtype=np.uint64).reshape(len(vals), 4)


def from_mont(a):
    inv = pow(1 << 256, -1, R)
    return [sum(int(w) << (64 * j) for j, w in enumerate(row)) * inv % R for row in np.asarray(a).reshape(-1, 4)]


def rows_numpy(codes, n):
    """the integer columns for large inputs, vectorised where the structure allows it (the timing tool's host route and the large GPU
    case): the same columns as assign(), as numpy arrays, without the field columns"""
    tag = np.zeros(n, np.uint8); index = np.zeros(n, np.uint32); value = np.zeros(n, np.uint32); length = np.zeros(n, np.uint32)
    is_code = np.zeros(n, np.uint8); left = np.zeros(n, np.uint8); size = np.zeros(n, np.uint8); owner = np.full(n, -1, np.int64)
    at = 0
    for b, code in enumerate(codes):
        if at >= n:
            break
        ln = len(code)
        take = min(ln, n - at - 1)
        value[at] = ln % 2**32
        length[at:at + 1 + take] = ln % 2**32
        owner[at:at + 1 + take] = b
        v = np.frombuffer(bytes(code[:take]), dtype=np.uint8)
        tag[at + 1:at + 1 + take] = 1
        index[at + 1:at + 1 + take] = np.arange(take, dtype=np.uint32)
        value[at + 1:at + 1 + take] = v
        p = np.where((v >= 0x60) & (v <= 0x7f), v - 0x5f, 0).astype(np.uint8)
        size[at + 1:at + 1 + take] = p
        s, pl = 0, p.tolist()
        state = [0] * take
        for i in range(take):                                           # the serial part a host has
            state[i] = s
            s = pl[i] if s == 0 else s - 1
        st = np.array(state, dtype=np.uint8)
        left[at + 1:at + 1 + take] = st
        is_code[at + 1:at + 1 + take] = st == 0
        at += 1 + take
    data = (tag == 1) & (left > 0)
    last = (tag == 1) & (index.astype(np.int64) == length.astype(np.int64) - 1)
    acc = data.astype(np.uint8)
    rlc = np.where(data, np.where((left == 1) | last, RLC_TAKE, RLC_COPY), np.where((tag == 1) & (size > 0) & ~last, RLC_COPY, RLC_NONE)).astype(np.uint8)
    return dict(tag=tag, index=index, value=value, is_code=is_code, push_data_left=left, push_data_size=size, length=length, acc_kinds=acc, rlc_kinds=rlc, owner=owner)

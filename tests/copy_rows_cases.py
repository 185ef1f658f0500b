"""The copy circuit's witness in Python, line by line after the reference, and the closed forms that ZK_OP_COPY_ROWS and ZK_OP_COPY_RLC
evaluate per row.  No GPU, no library.

assign restates zkevm-circuits/src/table.rs:1802-2065 (CopyTable::assignments) inside the loops of copy_circuit.rs:676-841
(assign_copy_event) and :944-1151 (assign_padding_row); closed holds the formulas of include/zkmi355.h, a function of (event, row) with
no state carried from row to row except the three running RLCs, which it writes as sums.  tests/test_copy_rows_model.py holds the two
against each other; the GPU tests compare the device with closed.

An event is a dict with the members of zk_copy_event (src_addr, src_addr_end, dst_addr, dst_addr_bias, rw_counter, src_off, dst_off,
prev_off, length, src_front, src_back, dst_front, dst_back, src_tag, dst_tag, flags, reserved) and, optionally, src_id and dst_id as
field elements.  The byte heap is a bytes object.  The reference's per-step (value, mask) pairs are the runs and the mask counts
spread out again: step s of a thread is masked if s < front or s >= length - back.
"""
import struct

import numpy as np

from oracle import bn254

R = bn254.R_MOD
M64 = 2**64
BYTECODE, MEMORY, TX_CALLDATA, TX_LOG, RLC_ACC = 1, 2, 3, 4, 5          # table.rs: CopyDataType (Padding is 0)
MEMORY_COPY = 1                                                         # ZK_COPY_MEMORY_COPY
TX_LOG_DATA = 6                                                         # TxLogFieldTag::Data
EVENT_BYTES = 88
BYTE_COLUMNS = ("is_first", "is_last", "tag", "value", "value_prev", "mask", "front_mask", "word_index", "is_pad", "non_pad_non_mask", "src_end_rows")
WORD_COLUMNS = ("addr", "src_addr_end", "real_bytes_left", "rw_counter", "rwc_inc_left")
PLANE_COLUMNS = {"tag_bits": 3, "types": 5}
INT_COLUMNS = BYTE_COLUMNS + WORD_COLUMNS + tuple(f"{name}{b}" for name, planes in PLANE_COLUMNS.items() for b in range(planes))
FR_COLUMNS = ("value_acc", "word_rlc", "word_rlc_prev", "rlc_acc", "id", "id_other")


def log_bias(log_id):
    """build_tx_log_address of the data field: (TxLogFieldTag::Data << 32) + (log_id << 48)"""
    return (TX_LOG_DATA << 32) + (log_id << 48)


def event(length, src_tag=MEMORY, dst_tag=MEMORY, src_addr=0, src_addr_end=None, dst_addr=0, dst_addr_bias=0, rw_counter=1, src_off=0, dst_off=None, prev_off=None,
          src_front=0, src_back=0, dst_front=None, dst_back=None, flags=0, reserved=0, src_id=0, dst_id=0):
    """an event; what is left out is what the reference leaves out: no aux bytes (the writer reads the reader's run with the reader's
    masks), no bytes_write_prev (value_prev is the writer's value), a source that ends behind the copied range"""
    dst_off = src_off if dst_off is None else dst_off
    return dict(src_addr=src_addr, src_addr_end=src_addr + length if src_addr_end is None else src_addr_end, dst_addr=dst_addr, dst_addr_bias=dst_addr_bias,
                rw_counter=rw_counter, src_off=src_off, dst_off=dst_off, prev_off=dst_off if prev_off is None else prev_off, length=length,
                src_front=src_front, src_back=src_back, dst_front=src_front if dst_front is None else dst_front, dst_back=src_back if dst_back is None else dst_back,
                src_tag=src_tag, dst_tag=dst_tag, flags=flags, reserved=reserved, src_id=src_id, dst_id=dst_id)


def pack_events(events):
    """count records of 88 little-endian bytes (zk_copy_event)"""
    out = bytearray()
    for e in events:
        out += struct.pack("<8Q5I4B", *(e[k] % M64 for k in ("src_addr", "src_addr_end", "dst_addr", "dst_addr_bias", "rw_counter", "src_off", "dst_off", "prev_off")),
                           *(e[k] for k in ("length", "src_front", "src_back", "dst_front", "dst_back")), e["src_tag"], e["dst_tag"], e["flags"], e["reserved"])
    assert len(out) == EVENT_BYTES * len(events)
    return np.frombuffer(bytes(out), dtype=np.uint8).copy()


def pack_ids(events):
    """count x 2 Montgomery Fr as (count * 2, 4) uint64: src id, then dst id"""
    return fr_numpy([e[k] % R for e in events for k in ("src_id", "dst_id")])


def counts(e, total):
    """the rule that makes an event an empty one"""
    runs = all(0 <= e[k] <= total and e["length"] <= total - e[k] for k in ("src_off", "dst_off", "prev_off"))
    return 1 <= e["src_tag"] <= 5 and 1 <= e["dst_tag"] <= 5 and e["reserved"] == 0 and e["flags"] & ~1 == 0 and runs


def effective(events, total):
    """what the ops take every event for: one that does not count has no steps"""
    return [e if counts(e, total) else dict(e, length=0) for e in events]


def empty_columns(n):
    cols = {name: [0] * n for name in INT_COLUMNS + FR_COLUMNS}
    return cols


def put_tag(cols, i, tag, memory_copy):
    """BinaryNumberChip::assign (most significant bit first) and the type columns of copy_circuit.rs:790-835"""
    cols["tag"][i] = tag
    for b in range(3):
        cols[f"tag_bits{b}"][i] = tag >> (2 - b) & 1
    for b, t in enumerate((BYTECODE, MEMORY, TX_CALLDATA, TX_LOG)):     # is_bytecode :796, is_memory :802, is_tx_calldata :790, is_tx_log :818
        cols[f"types{b}"][i] = int(tag == t)
    cols["types4"][i] = int(memory_copy)                                # :808-816


def padding_row(cols, i):
    """copy_circuit.rs:944-1151 assign_padding_row"""
    cols["is_last"][i] = i % 2                                          # :983-988
    cols["src_addr_end"][i] = 1                                         # :1004-1009
    cols["mask"][i] = 1                                                 # :1053-1058
    cols["front_mask"][i] = 1                                           # :1060-1065
    put_tag(cols, i, 0, 0)                                              # :1104 Padding, :1131-1146
    cols["id_other"][i] = 1                                             # :1106-1111 is_id_unchange.assign(0, 1)
    cols["src_end_rows"][i] = 1                                         # :1112-1117 is_src_end.assign(0, 1)
    # every other column 0


def assign(events, heap, n, r_word=0, r_in=0):
    """copy_circuit.rs:887-937 over n rows: every event through assign_copy_event (:676-841) around CopyTable::assignments
    (table.rs:1802-2065), then padding rows.  A dict of columns, each a list of n Python ints; rows at or after n are dropped."""
    cols = empty_columns(n)
    offset = 0
    for e in effective(events, len(heap)):
        L = e["length"]
        masked = lambda s, f, b: s < f or s >= L - b                    # noqa: E731
        read_steps = [(heap[e["src_off"] + s], masked(s, e["src_front"], e["src_back"])) for s in range(L)]
        write_steps = [(heap[e["dst_off"] + s], masked(s, e["dst_front"], e["dst_back"])) for s in range(L)]   # table.rs:1832-1837
        prev_write = [heap[e["prev_off"] + s] for s in range(L)]        # :1839-1843
        has_rlc = e["src_tag"] == RLC_ACC or e["dst_tag"] == RLC_ACC or e["dst_tag"] == BYTECODE
        rlc_acc = 0
        if has_rlc:                                                     # :1816-1830: rlc::value over the reversed values is Horner from the first
            for v, m in read_steps:
                if not m:
                    rlc_acc = (rlc_acc * r_in + v) % R
        is_source_rw = e["src_tag"] == MEMORY
        is_destination_rw = e["dst_tag"] in (MEMORY, TX_LOG)
        rw_counter = e["rw_counter"]                                    # :1845
        rwc_inc_left = (is_source_rw + is_destination_rw) * (L // 32)   # :1846 rw_counter_delta()
        rw_counter_write = rw_counter + rwc_inc_left // 2               # :1849
        rwc_inc_left_write = rwc_inc_left - rwc_inc_left // 2           # :1850
        is_memory_copy = bool(e["flags"] & MEMORY_COPY)                 # :1852-1854, as the caller states it
        copy_length = sum(1 for _, m in read_steps if not m)
        reader = dict(tag=e["src_tag"], is_rw=is_source_rw, id=e["src_id"], front_mask=True, addr=e["src_addr"], addr_end=e["src_addr_end"],
                      bytes_left=copy_length, value_acc=0, word_rlc=0, word_rlc_prev=0)                        # :1856-1867
        writer = dict(tag=e["dst_tag"], is_rw=is_destination_rw, id=e["dst_id"], front_mask=True, addr=e["dst_addr"], addr_end=e["dst_addr"] + L,
                      bytes_left=copy_length, value_acc=0, word_rlc=0, word_rlc_prev=0)                        # :1869-1880
        for step_idx in range(2 * L):                                   # :1884-1899
            is_read_step = step_idx % 2 == 0
            value, mask = (read_steps if is_read_step else write_steps)[step_idx // 2]
            prev_value = value if is_read_step else prev_write[step_idx // 2]   # :1902-1904
            thread = reader if is_read_step else writer                 # :1907-1911
            is_first = step_idx == 0                                    # :1913
            is_last = step_idx == 2 * L - 1                             # :1914
            is_pad = is_read_step and thread["addr"] >= thread["addr_end"]   # :1916
            value_or_pad = 0 if is_pad else value                       # :1936-1940
            if not mask:                                                # :1942-1945
                thread["front_mask"] = False
                thread["value_acc"] = (thread["value_acc"] * r_in + value_or_pad) % R
            if (step_idx // 2) % 32 == 0:                               # :1946-1950
                thread["word_rlc"] = 0
                thread["word_rlc_prev"] = 0
            thread["word_rlc"] = (thread["word_rlc"] * r_word + value) % R   # :1951
            thread["word_rlc_prev"] = thread["word_rlc"] if is_read_step else (thread["word_rlc_prev"] * r_word + prev_value) % R   # :1952-1956
            word_index = (step_idx // 2) % 32                           # :1970
            addr = thread["addr"]
            if not is_read_step:                                        # :1973-1979: the caller's bias is build_tx_log_address for a log, 0 otherwise
                addr += e["dst_addr_bias"]
            if is_memory_copy and not is_read_step:                     # :1982-1987
                rw_col, left_col = rw_counter_write, rwc_inc_left_write
            else:
                rw_col, left_col = rw_counter, rwc_inc_left
            i = offset
            if i < n:
                cols["is_first"][i] = int(is_first)                     # :2010
                cols["id"][i] = thread["id"] % R                        # :2011
                cols["addr"][i] = addr % M64                            # :2012
                cols["src_addr_end"][i] = thread["addr_end"] % M64      # :2013
                cols["real_bytes_left"][i] = thread["bytes_left"] % M64  # :2014
                cols["rlc_acc"][i] = rlc_acc                            # :2015
                cols["rw_counter"][i] = rw_col % M64                    # :2016
                cols["rwc_inc_left"][i] = left_col % M64                # :2017-2020
                cols["is_last"][i] = int(is_last)                       # :2023
                cols["value"][i] = value                                # :2024
                cols["value_prev"][i] = prev_value                      # :2025
                cols["word_rlc"][i] = thread["word_rlc"]                # :2026
                cols["word_rlc_prev"][i] = thread["word_rlc_prev"]      # :2027
                cols["value_acc"][i] = thread["value_acc"]              # :2028
                cols["is_pad"][i] = int(is_pad)                         # :2029
                cols["mask"][i] = int(mask)                             # :2030
                cols["front_mask"][i] = int(thread["front_mask"])       # :2031
                cols["word_index"][i] = word_index                      # :2032
                put_tag(cols, i, thread["tag"], is_memory_copy)         # copy_circuit.rs:746, :790-835
                cols["src_end_rows"][i] = int(is_read_step)             # copy_circuit.rs:749-757: is_src_end is assigned on reader rows
                cols["id_other"][i] = (e["dst_id"] if is_read_step else e["src_id"]) % R   # copy_circuit.rs:759-771
                cols["non_pad_non_mask"][i] = int(not is_pad and not mask)   # copy_circuit.rs:780-788
            if not thread["front_mask"]:                                # :2043-2045
                thread["addr"] += 1
            if not mask:                                                # :2047-2049
                thread["bytes_left"] -= 1
            is_row_end = (step_idx // 2) % 32 == 31                     # :2051
            if is_row_end and thread["is_rw"]:                          # :2053-2062
                if is_memory_copy and not is_read_step:
                    rw_counter_write += 1
                    rwc_inc_left_write -= 1
                else:
                    rw_counter += 1
                    rwc_inc_left -= 1
            offset += 1
    for i in range(offset, n):                                          # copy_circuit.rs:914-937
        padding_row(cols, i)
    return cols


def closed(events, heap, n, r_word=0, r_in=0):
    """the formulas of ZK_OP_COPY_ROWS and ZK_OP_COPY_RLC, row by row.  rlc_acc is the writer's value_acc at the event's last step where
    the event has an RLC and lies inside the n rows."""
    cols = empty_columns(n)
    start = 0
    for e in effective(events, len(heap)):
        L = e["length"]
        if start >= n:
            break
        acc = [0, 0]
        word = [0, 0]
        prev = 0
        cut = start + 2 * L > n
        for j in range(min(2 * L, n - start)):
            i, s, t = start + j, j >> 1, j & 1
            f, b = (e["dst_front"], e["dst_back"]) if t else (e["src_front"], e["src_back"])
            if f + b >= L:
                f, b = L, 0
            R_, W_ = int(e["src_tag"] == MEMORY), int(e["dst_tag"] in (MEMORY, TX_LOG))
            delta, cl, q = (R_ + W_) * (L // 32), max(L - e["src_front"] - e["src_back"], 0), s // 32
            adv = max(0, s - f)
            tag = e["dst_tag"] if t else e["src_tag"]
            value = heap[(e["dst_off"] if t else e["src_off"]) + s]
            value_prev = heap[e["prev_off"] + s] if t else value
            mask = int(s < f or s >= L - b)
            is_pad = int(t == 0 and (e["src_addr"] + adv) % M64 >= e["src_addr_end"])
            cols["is_first"][i], cols["is_last"][i] = int(j == 0), int(j == 2 * L - 1)
            cols["value"][i], cols["value_prev"][i] = value, value_prev
            cols["mask"][i], cols["front_mask"][i] = mask, int(s < f)
            cols["word_index"][i] = s % 32
            cols["addr"][i] = ((e["dst_addr"] + e["dst_addr_bias"] if t else e["src_addr"]) + adv) % M64
            cols["src_addr_end"][i] = (e["dst_addr"] + L) % M64 if t else e["src_addr_end"]
            cols["is_pad"][i], cols["non_pad_non_mask"][i] = is_pad, int(not is_pad and not mask)
            cols["real_bytes_left"][i] = (cl - min(adv, L - f - b)) % M64
            memory_copy = e["flags"] & MEMORY_COPY
            if memory_copy:
                rw, left = (e["rw_counter"] + delta // 2 + q, delta - delta // 2 - q) if t else (e["rw_counter"] + q, delta - q)
            else:
                inc = q * (R_ + W_) + (R_ if t == 1 and s % 32 == 31 else 0)
                rw, left = e["rw_counter"] + inc, delta - inc
            cols["rw_counter"][i], cols["rwc_inc_left"][i] = rw % M64, left % M64
            put_tag(cols, i, tag, memory_copy)
            cols["src_end_rows"][i] = int(t == 0)
            # the challenge-phase columns
            if s % 32 == 0:
                word[t] = 0
                if t:
                    prev = 0
            if s == 0:
                acc[t] = 0
            if not mask:
                acc[t] = (acc[t] * r_in + (0 if is_pad else value)) % R
            word[t] = (word[t] * r_word + value) % R
            if t:
                prev = (prev * r_word + value_prev) % R
            cols["value_acc"][i], cols["word_rlc"][i], cols["word_rlc_prev"][i] = acc[t], word[t], prev if t else word[t]
            cols["id"][i], cols["id_other"][i] = (e["dst_id"], e["src_id"]) if t else (e["src_id"], e["dst_id"])
            cols["id"][i] %= R
            cols["id_other"][i] %= R
        if not cut and L and (e["src_tag"] == RLC_ACC or e["dst_tag"] == RLC_ACC or e["dst_tag"] == BYTECODE):
            for j in range(2 * L):
                cols["rlc_acc"][start + j] = acc[1]
        start += 2 * L
    for i in range(min(start, n), n):
        padding_row(cols, i)
    return cols


def rlc_is_the_references(e):
    """the events on which rlc_acc, the writer's last value_acc, is the reference's sum over the reader's unmasked bytes: the writer's
    run and masks are the reader's.  Every event with an RLC that the reference builds is one."""
    return e["dst_off"] == e["src_off"] and e["dst_front"] == e["src_front"] and e["dst_back"] == e["src_back"]


def random_events(rng, count, heap_len, max_len=80, whole=True):
    """random events over a heap of heap_len bytes, every tag pair, masks, pads, memory copies, log biases"""
    out = []
    for _ in range(count):
        L = int(rng.choice([0, 1, 2, 31, 32, 33, 64, int(rng.integers(1, max_len + 1))]))
        L = min(L, heap_len)
        src_tag, dst_tag = int(rng.integers(1, 6)), int(rng.integers(1, 6))
        pick = lambda: [int(x) for x in rng.integers(0, L + 2, 2)] if rng.integers(0, 3) == 0 else [int(rng.integers(0, 4)) % (L + 1), int(rng.integers(0, 4)) % (L + 1)]   # noqa: E731
        (sf, sb), (df, db) = pick(), pick()
        same = rng.integers(0, 2) == 0
        src_off = int(rng.integers(0, heap_len - L + 1))
        dst_off = src_off if same else int(rng.integers(0, heap_len - L + 1))
        prev_off = dst_off if rng.integers(0, 2) else int(rng.integers(0, heap_len - L + 1))
        src_addr = int(rng.integers(0, 1 << 20))
        memory_copy = src_tag == MEMORY and dst_tag == MEMORY and rng.integers(0, 2) == 0
        out.append(event(L, src_tag, dst_tag, src_addr=src_addr, src_addr_end=src_addr + int(rng.integers(0, L + 8)), dst_addr=int(rng.integers(0, 1 << 20)),
                         dst_addr_bias=log_bias(int(rng.integers(0, 9))) if dst_tag == TX_LOG else 0, rw_counter=int(rng.integers(1, 1 << 30)),
                         src_off=src_off, dst_off=dst_off, prev_off=prev_off, src_front=sf, src_back=sb, dst_front=sf if same else df, dst_back=sb if same else db,
                         flags=int(memory_copy), src_id=int(rng.integers(1, 1 << 62)), dst_id=int(rng.integers(1, 1 << 62))))
        if memory_copy:
            out[-1]["dst_id"] = out[-1]["src_id"]
    return out


def columns_numpy(cols, n):
    """the integer columns as the arrays the op writes (planes joined), the Fr columns as (n, 4) uint64 Montgomery limbs"""
    out = {name: np.array(cols[name], dtype=np.uint8) for name in BYTE_COLUMNS}
    out.update({name: np.array(cols[name], dtype=np.uint64) for name in WORD_COLUMNS})
    for name, planes in PLANE_COLUMNS.items():
        out[name] = np.concatenate([np.array(cols[f"{name}{b}"], dtype=np.uint8) for b in range(planes)]) if n else np.zeros(0, np.uint8)
    return out


def fr_numpy(values):
    return np.frombuffer(b"".join(bn254.mont_bytes(v, R) for v in values), dtype=np.uint64).reshape(len(values), 4).copy()

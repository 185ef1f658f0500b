"""Helper (not collected): the model of ZK_OP_KEY_SORT and ZK_OP_KEY_ORDER in Python integers.
1. Record packing: an RW row (tag, id, address, field_tag, storage_key, rw_counter) as the 64 bytes that the reference's
   rw_to_be_limbs packs (zkevm-circuits/src/state_circuit/lexicographic_ordering.rs:297-312).
2. The sort: sorted(range(n), key=lambda i: (masked(keys[i]), i)) -- stable, over the bytes the mask keeps.
3. The order columns of adjacent rows (first_different_limb, its five bits, limb_difference, its inverse, not_first_access) and the
   gathered typed columns, with the state circuit's gather map: its 48 sort-key columns (tag, field_tag, 2 id limbs, 10 address limbs,
   32 storage-key bytes, 2 rw_counter limbs) and the RW table's own rw_counter and id, 50 columns in one call."""
import json
import os
import random

from oracle import bn254 as o

P = o.R_MOD
R256 = (1 << 256) % P
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "key_order_reference.json")
RECORD = 64
LIMBS = 32
TILE = 2048                                  # places per workgroup of a sort pass: KS_TILE of csrc/keyorder.hip.hpp
FULL_MASK = bytes([1]) * 64
NO_COUNTER_MASK = bytes([1]) * 60 + bytes(4)  # Rw::as_key: everything but the rw_counter


def reference():
    return json.load(open(GOLDEN))


# ---- 1. packing
def pack(tag, rw_id, address, field_tag, storage_key, rw_counter):
    """one 64-byte key record"""
    assert 0 <= tag < 256 and 0 <= rw_id < 1 << 32 and 0 <= address < 1 << 160 and 0 <= field_tag < 256 and 0 <= storage_key < 1 << 256 and 0 <= rw_counter < 1 << 32
    rec = bytes([0, tag]) + rw_id.to_bytes(4, "big") + address.to_bytes(20, "big") + bytes([0, field_tag]) + storage_key.to_bytes(32, "big") + rw_counter.to_bytes(4, "big")
    assert len(rec) == RECORD
    return rec


def limbs(rec):
    return [int.from_bytes(rec[2 * j:2 * j + 2], "big") for j in range(LIMBS)]


def realistic_rows(rng, n):
    """RW rows as a block has them: few tags, ids below 50, 8 addresses, 4 storage keys, distinct counters, in counter order"""
    addresses = [rng.randrange(1 << 160) for _ in range(8)]
    storage = [0] + [rng.randrange(1 << 256) for _ in range(3)]
    return [pack(rng.choice((1, 2, 3, 4, 5, 9)), rng.randrange(50), rng.choice(addresses), rng.randrange(4), rng.choice(storage), c + 1) for c in range(n)]


# ---- 2. the sort
def masked(rec, mask):
    return rec if all(mask) else bytes(b for b, m in zip(rec, mask) if m)


def sort_perm(keys, mask=None):
    mask = FULL_MASK if mask is None else mask
    assert len(mask) == RECORD
    return sorted(range(len(keys)), key=lambda i: (masked(keys[i], mask), i))


# ---- 3. the order columns and the gathers
def order_columns(keys, perm=None, group_limbs=30):
    """{index, bits (5 planes), diff, inv, not_first} of n rows; diff and inv as integers mod P (not Montgomery).  Row i is record
    perm[i]; row 0, and a row whose index or whose predecessor's index is >= n, holds zeros."""
    n = len(keys) if perm is None else len(perm)
    perm = list(range(n)) if perm is None else perm
    out = {"index": [0] * n, "bits": [[0] * n for _ in range(5)], "diff": [0] * n, "inv": [0] * n, "not_first": [0] * n}
    for i in range(1, n):
        if perm[i] >= len(keys) or perm[i - 1] >= len(keys):
            continue
        cur, prev = limbs(keys[perm[i]]), limbs(keys[perm[i - 1]])
        j = next((j for j in range(LIMBS) if cur[j] != prev[j]), LIMBS - 1)
        d = (cur[j] - prev[j]) % P
        out["index"][i] = j
        for b in range(5):
            out["bits"][b][i] = j >> (4 - b) & 1
        out["diff"][i] = d
        out["inv"][i] = pow(d, -1, P) if d else 0
        out["not_first"][i] = int(j >= group_limbs)
    return out


def gather(keys, cols, perm=None):
    """[column][row]: the big-endian integer of key bytes [offset, offset + width) of row i's record; 0 for an index >= n"""
    n = len(keys) if perm is None else len(perm)
    perm = list(range(n)) if perm is None else perm
    return [[int.from_bytes(keys[p][off:off + width], "big") if p < len(keys) else 0 for p in perm] for off, width in cols]


def state_circuit_cols():
    """the state circuit's 48 sort-key columns, then the RW table's own rw_counter and id: (name, offset, width)"""
    cols = [("tag", 1, 1), ("field_tag", 27, 1), ("id_limb1", 2, 2), ("id_limb0", 4, 2)]
    cols += [(f"address_limb{9 - k}", 6 + 2 * k, 2) for k in range(10)]
    cols += [(f"storage_key_byte{31 - k}", 28 + k, 1) for k in range(32)]
    cols += [("rw_counter_limb1", 60, 2), ("rw_counter_limb0", 62, 2)]
    assert len(cols) == 48
    return cols + [("rw_counter", 60, 4), ("id", 2, 4)]


def mont(values):
    return [v * R256 % P for v in values]


def random_keys(rng, n):
    return [rng.randbytes(RECORD) for _ in range(n)]


def rng(seed):
    return random.Random(seed)

"""CPU: the model of tests/key_order_cases.py against what the reference holds about the state circuit's row order
(tests/golden/key_order_reference.json: the 32 LimbIndex names in order, the byte layout of rw_to_be_limbs, hand-worked row pairs):
the packing puts every field where the layout says, the limb numbers are the reference's, the hand-worked pairs give the stated
first_different_limb and limb_difference, the bits follow AsBits<5>, and the masked stable sort is sort_by_cached_key(Rw::as_key)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import key_order_cases as kc  # noqa: E402

P = kc.P


def _fields(f):
    return f["tag"], f["id"], int(f["address"], 16), f["field_tag"], int(f["storage_key"], 16), f["rw_counter"]


def test_the_fixture_lists_the_32_limbs_in_order():
    ref = kc.reference()
    names = [e["name"] for e in ref["limb_index"]]
    assert [e["value"] for e in ref["limb_index"]] == list(range(32))
    assert names[:3] == ["Tag", "Id1", "Id0"] and names[3:13] == [f"Address{9 - k}" for k in range(10)] and names[13] == "FieldTag"
    assert names[14:30] == [f"StorageKey{15 - k}" for k in range(16)] and names[30:] == ["RwCounter1", "RwCounter0"]
    assert all(e["at"].startswith("zkevm-circuits/src/state_circuit/lexicographic_ordering.rs:") for e in ref["limb_index"])
    assert ref["not_first_access"]["group_limbs"] == names.index("RwCounter1") == 30


def test_packing_follows_the_layout():
    ref = kc.reference()
    spans = [tuple(f["bytes"]) for f in ref["layout"]["fields"]]
    assert spans == [(0, 0), (1, 1), (2, 5), (6, 25), (26, 26), (27, 27), (28, 59), (60, 63)]
    assert [hi + 1 for _, hi in spans[:-1]] == [lo for lo, _ in spans[1:]] and spans[-1][1] == kc.RECORD - 1
    tag, rw_id, address, field_tag, key, counter = 0xA1, 0xB2B3B4B5, int.from_bytes(bytes(range(0x10, 0x24)), "big"), 0xC6, int.from_bytes(bytes(range(0x40, 0x60)), "big"), 0xD7D8D9DA
    rec = kc.pack(tag, rw_id, address, field_tag, key, counter)
    content = {f["content"]: rec[f["bytes"][0]:f["bytes"][1] + 1] for f in ref["layout"]["fields"] if f["content"] != "zero"}
    assert rec[0] == 0 and rec[26] == 0
    assert content == {"tag": bytes([tag]), "id, big-endian": rw_id.to_bytes(4, "big"), "address": address.to_bytes(20, "big"), "field_tag": bytes([field_tag]),
                       "storage_key, big-endian": key.to_bytes(32, "big"), "rw_counter, big-endian": counter.to_bytes(4, "big")}
    names = [e["name"] for e in ref["limb_index"]]
    limbs = dict(zip(names, kc.limbs(rec)))
    assert limbs["Tag"] == tag and limbs["Id1"] == rw_id >> 16 and limbs["Id0"] == rw_id & 0xFFFF and limbs["FieldTag"] == field_tag
    assert limbs["Address9"] == address >> 144 and limbs["Address0"] == address & 0xFFFF
    assert limbs["StorageKey15"] == key >> 240 and limbs["StorageKey0"] == key & 0xFFFF
    assert limbs["RwCounter1"] == counter >> 16 and limbs["RwCounter0"] == counter & 0xFFFF


def test_the_hand_worked_pairs():
    ref = kc.reference()
    names = [e["name"] for e in ref["limb_index"]]
    pairs = ref["pairs"]
    assert {"Tag", "Address0", "StorageKey15", "RwCounter1", "RwCounter0"} <= {p["name"] for p in pairs}
    for p in pairs:
        prev, cur = kc.pack(*_fields(p["prev"])), kc.pack(*_fields(p["cur"]))
        assert prev.hex() == p["prev"]["record"] and cur.hex() == p["cur"]["record"], p["name"]
        cols = kc.order_columns([prev, cur])
        j, d = p["index"], p["diff"]
        assert names[j] == p["name"].split(",")[0]
        assert cols["index"] == [0, j] and cols["diff"] == [0, d % P] and cols["inv"][0] == 0 and cols["inv"][1] * d % P == 1, p["name"]
        assert [cols["bits"][b][1] for b in range(5)] == [int(c) for c in format(j, "05b")], p["name"]      # plane 0: the most significant bit
        assert cols["not_first"] == [0, int(j >= 30)], p["name"]
        # the sort puts the smaller record first; an out-of-order pair is the one with the negative difference
        assert kc.sort_perm([prev, cur]) == ([0, 1] if d > 0 else [1, 0]), p["name"]


def test_equal_records_and_row_zero():
    rec = kc.pack(3, 1, 2, 3, 4, 5)
    cols = kc.order_columns([rec, rec, rec], group_limbs=30)
    assert cols["index"] == [0, 31, 31] and cols["diff"] == [0, 0, 0] and cols["inv"] == [0, 0, 0] and cols["not_first"] == [0, 1, 1]
    assert kc.order_columns([rec, rec], group_limbs=32)["not_first"] == [0, 0]
    assert kc.sort_perm([rec, rec, rec]) == [0, 1, 2]


def test_the_masked_sort_is_sort_by_cached_key():
    """(tag, id, address, field_tag, storage_key) with the rw_counter breaking ties: rows handed over in counter order, sorted stably
    without the counter bytes, stand as the tuple sort puts them -- and so does the full mask while the counters are distinct"""
    ref = kc.reference()
    assert ref["sort_key"]["order"] == ["tag", "id", "address", "field_tag", "storage_key"] and ref["sort_key"]["tie"] == "rw_counter"
    rng = kc.rng(5)
    rows = [(rng.choice((1, 2, 5)), rng.randrange(4), rng.choice((7, 1 << 159, 99)), rng.randrange(3), rng.choice((0, 1 << 255, 12)), c + 1) for c in range(400)]
    keys = [kc.pack(*r) for r in rows]
    want = sorted(range(len(rows)), key=lambda i: (rows[i][:5], rows[i][5]))
    assert kc.sort_perm(keys, kc.NO_COUNTER_MASK) == want == kc.sort_perm(keys, kc.FULL_MASK)
    assert kc.sort_perm(keys, bytes(64)) == list(range(len(keys)))
    # the gather map: 48 state-circuit columns over disjoint key bytes that cover everything but the two zero bytes
    cols = kc.state_circuit_cols()
    assert len(cols) == 50 and cols[48:] == [("rw_counter", 60, 4), ("id", 2, 4)]
    covered = sorted(b for _, off, width in cols[:48] for b in range(off, off + width))
    assert covered == [b for b in range(64) if b not in (0, 26)]
    got = kc.gather(keys[:3], [(off, width) for _, off, width in cols])
    by_name = {name: col for (name, _, _), col in zip(cols, got)}
    assert by_name["tag"] == [r[0] for r in rows[:3]] and by_name["id"] == [r[1] for r in rows[:3]] and by_name["rw_counter"] == [1, 2, 3]
    assert by_name["address_limb0"] == [r[2] & 0xFFFF for r in rows[:3]] and by_name["storage_key_byte31"] == [r[4] >> 248 for r in rows[:3]]

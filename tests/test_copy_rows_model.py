"""CPU: the closed forms that ZK_OP_COPY_ROWS and ZK_OP_COPY_RLC evaluate (copy_rows_cases.closed) against the line-by-line restatement
of the reference's serial loop (copy_rows_cases.assign), on random events and on the edges.  rlc_acc is compared on the events on which
the writer's run and masks are the reader's: there the writer's last value_acc is the reference's sum over the reader's unmasked
bytes; elsewhere the op's value is the one constrain_event_rlc_acc forces and the reference's own sum would not satisfy the gate."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import copy_rows_cases as cp  # noqa: E402

R_WORD, R_IN = 0x1234567890ABCDEF1234567890ABCDEF % cp.R, (cp.R - 0x0FEDCBA987654321)


def heap_of(n, seed=1):
    return bytes(np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8))


def agree(events, heap, n=None, slack=5):
    rows = sum(2 * e["length"] for e in cp.effective(events, len(heap)))
    n = rows + slack if n is None else n
    a, c = cp.assign(events, heap, n, R_WORD, R_IN), cp.closed(events, heap, n, R_WORD, R_IN)
    same = all(cp.rlc_is_the_references(e) for e in events) and n >= rows
    for name in cp.INT_COLUMNS + cp.FR_COLUMNS:
        if name == "rlc_acc" and not same:
            continue
        assert a[name] == c[name], (name, [i for i in range(n) if a[name][i] != c[name][i]][:5])
    return a


@pytest.mark.parametrize("seed", range(12))
def test_random_events(seed):
    rng = np.random.default_rng(seed)
    heap = heap_of(400, seed)
    agree(cp.random_events(rng, 25, len(heap)), heap)


@pytest.mark.parametrize("seed", range(4))
def test_random_events_whose_writer_is_the_reader_have_the_references_rlc_acc(seed):
    rng = np.random.default_rng(100 + seed)
    heap = heap_of(400, seed)
    events = [e for e in cp.random_events(rng, 60, len(heap)) if cp.rlc_is_the_references(e)]
    assert any(e["src_tag"] == cp.RLC_ACC or e["dst_tag"] in (cp.RLC_ACC, cp.BYTECODE) for e in events)
    a = agree(events, heap)
    assert any(a["rlc_acc"])


@pytest.mark.parametrize("L", [1, 31, 32, 33, 64])
def test_lengths_around_a_word(L):
    heap = heap_of(200)
    for src_tag in range(1, 6):
        for dst_tag in range(1, 6):
            agree([cp.event(L, src_tag, dst_tag, src_off=3, src_addr=7, dst_addr=100)], heap)


@pytest.mark.parametrize("L", [1, 5, 33])
def test_masks_that_cover_the_whole_thread(L):
    """f + b == L and f + b > L: the thread keeps front_mask = 1 and never advances its address"""
    heap = heap_of(200)
    for f in range(L + 2):
        for b in (L - f, L - f + 1, L + 3):
            if b < 0:
                continue
            a = agree([cp.event(L, src_front=f, src_back=b, dst_front=0, dst_back=0, src_addr=50, dst_addr=9)], heap)
            assert all(a["front_mask"][0:2 * L:2]) and len(set(a["addr"][0:2 * L:2])) == 1
            agree([cp.event(L, src_front=0, src_back=0, dst_front=f, dst_back=b, src_addr=50, dst_addr=9)], heap)
            agree([cp.event(L, cp.MEMORY, cp.BYTECODE, src_front=f, src_back=b)], heap)


@pytest.mark.parametrize("end", [990, 1000, 1001, 1010, 1037, 1038, 1039, 1100])
def test_src_addr_end_before_inside_and_behind_the_range(end):
    """40 steps from address 1000 with two front-masked steps: the reader's address runs from 1000 to 1037"""
    heap = heap_of(200)
    a = agree([cp.event(40, cp.TX_CALLDATA, cp.MEMORY, src_addr=1000, src_addr_end=end, src_front=2, dst_front=2)], heap)
    assert sum(a["is_pad"]) == sum(1 for s in range(40) if 1000 + max(0, s - 2) >= end)


@pytest.mark.parametrize("L", [32, 96, 97, 160])
def test_memory_copy_with_odd_and_even_delta(L):
    heap = heap_of(400)
    a = agree([cp.event(L, cp.MEMORY, cp.MEMORY, flags=cp.MEMORY_COPY, src_id=5, dst_id=5, rw_counter=77, dst_off=100, prev_off=200, src_front=3, dst_front=9)], heap)
    delta = 2 * (L // 32)
    assert a["rw_counter"][1] == 77 + delta // 2 and a["rwc_inc_left"][1] == delta - delta // 2 and all(a["types4"][:2 * L])


def test_log_bias_is_on_writer_rows_only():
    heap = heap_of(200)
    a = agree([cp.event(40, cp.MEMORY, cp.TX_LOG, dst_addr=4, dst_addr_bias=cp.log_bias(3), src_addr=64)], heap)
    assert a["addr"][0] == 64 and a["addr"][1] == 4 + (6 << 32) + (3 << 48) and a["addr"][3] == a["addr"][1] + 1


def test_a_reader_with_rlc_acc_and_a_writer_with_bytecode():
    heap = heap_of(200)
    a = agree([cp.event(37, cp.RLC_ACC, cp.MEMORY, src_front=1, src_back=2), cp.event(37, cp.MEMORY, cp.BYTECODE, src_front=4), cp.event(5, cp.MEMORY, cp.MEMORY)], heap)
    assert a["rlc_acc"][0] and a["rlc_acc"][74] and a["rlc_acc"][0] != a["rlc_acc"][74] and not any(a["rlc_acc"][148:])


def test_aux_bytes_with_masks_that_differ_from_the_readers():
    heap = heap_of(300)
    agree([cp.event(70, cp.MEMORY, cp.MEMORY, src_off=0, dst_off=100, prev_off=200, src_front=5, src_back=3, dst_front=11, dst_back=0),
           cp.event(33, cp.BYTECODE, cp.MEMORY, src_off=10, dst_off=150, prev_off=20, src_front=0, src_back=0, dst_front=0, dst_back=31)], heap)


def test_events_that_do_not_count_are_empty_and_a_cut_event_has_no_rlc_acc():
    heap = heap_of(100)
    good = cp.event(10, cp.MEMORY, cp.RLC_ACC)
    bad = [dict(good, src_tag=0), dict(good, dst_tag=6), dict(good, reserved=1), dict(good, flags=2), dict(good, src_off=91), dict(good, prev_off=2**63)]
    for e in bad:
        assert not cp.counts(e, len(heap))
    assert cp.counts(dict(good, src_off=90), len(heap))
    a = agree(bad + [good], heap)
    assert a["is_first"][0] == 1 and a["tag"][20] == 0
    c = cp.closed([good], heap, 19, R_WORD, R_IN)
    assert not any(c["rlc_acc"]) and c["value_acc"][:19] == a["value_acc"][:19]


def test_the_packer_writes_the_c_layout():
    e = cp.event(0x01020304, 2, 5, src_addr=1, src_addr_end=2, dst_addr=3, dst_addr_bias=4, rw_counter=5, src_off=6, dst_off=7, prev_off=8, src_front=9, src_back=10,
                 dst_front=11, dst_back=12, flags=1)
    raw = cp.pack_events([e])
    assert len(raw) == 88 and raw[:8].view(np.uint64)[0] == 1 and raw[56:64].view(np.uint64)[0] == 8
    assert raw[64:84].view(np.uint32).tolist() == [0x01020304, 9, 10, 11, 12] and raw[84:].tolist() == [2, 5, 1, 0]


@pytest.mark.parametrize("seed", range(3))
def test_the_tight_loop_of_value_acc_is_the_closed_form(seed):
    """copy_rows_device.value_acc_only, which the one large GPU case is compared with"""
    import copy_rows_device as dev
    heap = heap_of(400, seed)
    events = cp.random_events(np.random.default_rng(200 + seed), 40, len(heap))
    rows = sum(2 * e["length"] for e in events)
    for n in (rows + 5, rows - 7, rows - 8):
        want = cp.closed(events, heap, n, dev.R_WORD, dev.R_IN)["value_acc"]
        for t in range(2):
            assert dev.value_acc_only(events, heap, n, t) == want[t::2], (n, t)

"""GPU: ZK_OP_COPY_ROWS of zk_field_vec_op -- every output byte for byte against the closed forms of tests/copy_rows_cases.py (which
tests/test_copy_rows_model.py holds against the reference's serial loop), through the C ABI, with sentinels in front of and behind
every buffer.  T = 1024 rows is the implementation's tile; the scenarios are those of tests/copy_rows_device.py."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import copy_rows_cases as cp  # noqa: E402
import copy_rows_device as dev  # noqa: E402
from copy_rows_device import GUARD, INVALID_ARG, OK, ROWS_OUTPUTS, SENT, T, Device, busy_event, heap_of, sweep, want_arrays  # noqa: E402
from oracle import bn254  # noqa: E402

pytestmark = pytest.mark.gpu
SCENARIOS = dev.scenarios()
NAMES = ("addr",) + ROWS_OUTPUTS


def checked(ctx, events, heap, n, **kw):
    d = Device(ctx, events, heap, n, rlc_outputs=(), **kw)
    try:
        return d.check(d.run_rows())
    finally:
        d.free()


@pytest.mark.parametrize("name", sorted(SCENARIOS))
def test_scenario(ctx, name):
    events, heap, n = SCENARIOS[name]
    got = checked(ctx, events, heap, n)
    if name == "no_events":
        assert got["mask"].all() and got["src_end_rows"].all() and not got["tag"].any() and (got["src_addr_end"] == 1).all()


def test_an_event_boundary_at_every_even_offset_of_a_tiles_first_64_rows(ctx):
    """events own an even number of rows, so a boundary falls on the even rows T, T + 2, .., T + 64"""
    heap = heap_of(3000, 7)
    firsts = [busy_event(T // 2 + k, len(heap), dst_tag=cp.TX_LOG, dst_addr_bias=cp.log_bias(1)) for k in range(33)]
    sweep(ctx, firsts, busy_event(70, len(heap), src_tag=cp.TX_CALLDATA), heap, "run_rows", NAMES)


def test_a_tile_edge_at_every_word_index_of_an_event(ctx):
    """a first event of k steps pushes a 600-step memory copy along: row T is its step 512 - k, every s mod 32 for k = 0 .. 33"""
    heap = heap_of(3000, 8)
    firsts = [cp.event(k, cp.BYTECODE, cp.MEMORY, src_off=k, src_front=k // 2) for k in range(34)]
    tail = busy_event(600, len(heap), src_tag=cp.MEMORY, dst_tag=cp.MEMORY, flags=cp.MEMORY_COPY, dst_id=11)
    sweep(ctx, firsts, tail, heap, "run_rows", NAMES)


def test_no_rows_writes_nothing(ctx):
    heap = heap_of(100)
    d = Device(ctx, [busy_event(20, len(heap))], heap, 0, n_alloc=8, rlc_outputs=())
    try:
        assert (d.run_rows() == SENT).all()
    finally:
        d.free()


def test_events_that_do_not_count_are_empty_events(ctx):
    """a bad tag, bad flags, a nonzero reserved byte, and runs that end one byte past total_bytes, between events that count; the heap
    on the device is longer than total_bytes says, and a run that ends exactly at total_bytes counts"""
    heap = heap_of(500, 9)
    total = 400
    good = busy_event(30, total, src_off=370, dst_off=0, prev_off=370)
    bad = [dict(good, src_tag=0), dict(good, dst_tag=6), dict(good, src_tag=255), dict(good, flags=2), dict(good, flags=0x81), dict(good, reserved=1),
           dict(good, src_off=371), dict(good, dst_off=371), dict(good, prev_off=371), dict(good, src_off=2**64 - 1), dict(good, prev_off=2**63), dict(good, length=2**32 - 1, src_off=1)]
    events = [good] + [x for e in bad for x in (e, good)]
    assert all(not cp.counts(e, total) for e in bad) and cp.counts(good, total)
    got = checked(ctx, events, heap, 2 * 30 * (len(bad) + 1) + 20, total=total)
    assert int(got["is_first"].sum()) == len(bad) + 1


@pytest.mark.parametrize("name", ROWS_OUTPUTS + ("none",))
def test_each_output_alone(ctx, name):
    events, heap, n = SCENARIOS["mixed_random_events"]
    checked(ctx, events[:20], heap, 2 * T + 77, rows_outputs=() if name == "none" else (name,))


def test_the_call_without_a_byte_output_reads_no_byte(ctx):
    """d_bytes points at a buffer that is shorter than total_bytes says; no output holds a byte value, so it is never touched"""
    events, heap, n = SCENARIOS["mixed_random_events"]
    outputs = tuple(x for x in ROWS_OUTPUTS if x not in ("value", "value_prev"))
    d = Device(ctx, events, heap, n, rows_outputs=outputs, rlc_outputs=())
    short = ctx.to_device(np.full(2 * GUARD + 16, SENT, np.uint8))
    try:
        ctx.copy_rows(d.d_events, d.count, short.ptr + GUARD, d.total, n, d.ptr("addr"), **{x: d.ptr(x) for x in outputs})
        ctx.sync()
        d.written = {"addr", *outputs}
        d.check(d.image())
        assert (short.download(2 * GUARD + 16, np.uint8) == SENT).all()
    finally:
        short.free()
        d.free()


def test_one_byte_outputs_at_odd_addresses(ctx):
    events, heap, _ = SCENARIOS["mixed_random_events"]
    for n in (1, 3, 70, T + 7, 2 * T + 3):
        checked(ctx, events, heap, n, odd=True)


def test_the_profilers_byte_count(ctx):
    events, heap, n = SCENARIOS["mixed_random_events"]
    d = Device(ctx, events, heap, n, rows_outputs=("tag", "tag_bits", "value", "rw_counter", "types"), rlc_outputs=())
    try:
        ctx.prof_enable(True)
        ctx.prof_reset()
        d.run_rows()
        assert ctx.prof_get("copy_rows")[1] == 1
        assert ctx.prof_get_bytes("copy_rows") == 88 * len(events) + len(heap) + n * (8 + 1 + 3 + 1 + 8 + 5)
        d.free()
        d = Device(ctx, events, heap, n, rows_outputs=("mask",), rlc_outputs=())
        ctx.prof_reset()
        d.run_rows()
        assert ctx.prof_get_bytes("copy_rows") == 88 * len(events) + n * (8 + 1)
    finally:
        ctx.prof_enable(False)
        d.free()


def test_the_same_call_twice_gives_the_same_bytes(ctx):
    events, heap, n = SCENARIOS["overlapping_and_repeated_runs"]
    d = Device(ctx, events, heap, n, rlc_outputs=())
    try:
        first = d.run_rows()
        assert np.array_equal(first, d.run_rows())
    finally:
        d.free()


def test_refusals_leave_the_outputs_untouched_and_the_context_usable(zk, ctx):
    b = zk.binding
    rng = np.random.default_rng(12)
    n = 150
    heap = heap_of(300, 12)
    d = Device(ctx, [busy_event(40, len(heap)), busy_event(20, len(heap))], heap, n, rlc_outputs=())
    vals = [[int.from_bytes(rng.bytes(31), "little") for _ in range(4)] for _ in range(2)]
    x, y = (ctx.to_device(cp.fr_numpy(v)) for v in vals)
    add_out = ctx.alloc(128)
    host = np.zeros(8, np.uint64)

    def desc(**change):
        f = dict(d_events=d.d_events, count=d.count, d_bytes=d.d_bytes, total_bytes=d.total, flags=0)
        f.update({"d_" + name: d.ptr(name) for name in ROWS_OUTPUTS})
        f.update(change)
        return b._CopyRows(*[f[name] for name, _ in b._CopyRows._fields_])

    def call(ds, field=0, op=28, rows=n, out=None, d_b=None):
        return zk.lib().zk_field_vec_op(ctx.h, field, op, ctypes.byref(ds), d_b, ctypes.c_void_p(d.ptr("addr") if out is None else out), ctypes.c_size_t(rows))

    def refused(ds, why, **kw):
        rc = call(ds, **kw)
        ctx.sync()
        assert rc == INVALID_ARG, why
        assert (d.image() == SENT).all(), why
        # a valid call follows every refusal
        assert zk.lib().zk_field_vec_op(ctx.h, 0, 0, ctypes.c_void_p(x.ptr), ctypes.c_void_p(y.ptr), ctypes.c_void_p(add_out.ptr), ctypes.c_size_t(4)) == OK, why
        ctx.sync()
        assert [bn254.from_mont_bytes(bytes(r), cp.R) for r in add_out.download((4, 32), np.uint8)] == [(u + v) % cp.R for u, v in zip(*vals)], why

    try:
        refused(desc(), "Fq", field=1)
        refused(desc(), "Fq is looked at before n", field=1, rows=0)
        refused(desc(flags=1), "flags")
        refused(desc(flags=1), "validated before n is looked at", rows=0)
        refused(desc(d_events=None), "NULL d_events")
        refused(desc(d_events=d.d_events + 4), "misaligned d_events")
        refused(desc(d_bytes=None), "NULL d_bytes with bytes")
        refused(desc(total_bytes=2**61), "total_bytes = 2^61")
        refused(desc(), "n = 2^32", rows=2**32)
        refused(desc(), "d_out at 4", out=d.ptr("addr") + 4)
        for name in ("src_addr_end", "real_bytes_left", "rw_counter", "rwc_inc_left"):
            refused(desc(**{"d_" + name: d.ptr(name) + 4}), f"misaligned {name}")
        refused(desc(), "a second operand", d_b=host.ctypes.data_as(ctypes.c_void_p))
        refused(desc(), "a second operand, before n", d_b=host.ctypes.data_as(ctypes.c_void_p), rows=0)
        # overlaps: an output with an input, with d_out, with another output
        refused(desc(d_tag=d.d_bytes + 10), "d_tag inside d_bytes")
        refused(desc(d_mask=d.d_events + 87), "d_mask over the last byte of d_events")
        refused(desc(d_value=d.ptr("addr") + 8 * n - 1), "d_value over the last byte of d_out")
        refused(desc(d_is_pad=d.ptr("tag_bits") + 3 * n - 1), "d_is_pad over the last byte of the third plane of d_tag_bits")
        refused(desc(d_is_last=d.ptr("types") + 5 * n - 1), "d_is_last over the last byte of d_types")
        refused(desc(d_rw_counter=d.ptr("rwc_inc_left")), "d_rw_counter is d_rwc_inc_left")
        refused(desc(d_front_mask=d.ptr("mask")), "d_front_mask is d_mask")
        for op in (27, 29):
            assert zk.lib().zk_field_vec_op(ctx.h, 0, op, ctypes.c_void_p(x.ptr), ctypes.c_void_p(y.ptr), ctypes.c_void_p(d.ptr("addr")), ctypes.c_size_t(4)) == INVALID_ARG, op
            refused(desc(), f"op {op}", op=op, rows=4, d_b=host.ctypes.data_as(ctypes.c_void_p))
        # and the accepted neighbours: n = 0 with a valid descriptor, count = 0 without events, no bytes without a heap
        assert call(desc(), rows=0) == OK
        ctx.sync()
        assert (d.image() == SENT).all()
        assert call(desc(d_events=None, count=0, d_bytes=None, total_bytes=0)) == OK
        ctx.sync()
        d.written = {"addr", *ROWS_OUTPUTS}
        d.check(d.image(), want_arrays([], b"", n, NAMES))
        d.clear()
        d.check(d.run_rows())
    finally:
        for buf_ in (x, y, add_out):
            buf_.free()
        d.free()

"""GPU: ZK_OP_COPY_RLC of zk_field_vec_op -- value_acc, the two word RLCs, rlc_acc and the ids, every Fr canonical and bit for bit
against the closed forms of tests/copy_rows_cases.py, through the C ABI, with sentinels around every buffer.  A workgroup of the scan
takes STEP_BLOCK = 2048 steps of one thread, 4096 rows; the scenarios are those of tests/copy_rows_device.py."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import copy_rows_cases as cp  # noqa: E402
import copy_rows_device as dev  # noqa: E402
from copy_rows_device import GUARD, INVALID_ARG, OK, R_IN, R_WORD, RLC_OUTPUTS, SENT, STEP_BLOCK, Device, busy_event, heap_of, sweep, want_arrays  # noqa: E402
from oracle import bn254  # noqa: E402

pytestmark = pytest.mark.gpu
SCENARIOS = dev.scenarios()
NAMES = ("value_acc",) + RLC_OUTPUTS


def checked(ctx, events, heap, n, **kw):
    d = Device(ctx, events, heap, n, rows_outputs=(), **kw)
    try:
        return d.check(d.run_rlc())
    finally:
        d.free()


@pytest.mark.parametrize("name", sorted(SCENARIOS))
def test_scenario(ctx, name):
    events, heap, n = SCENARIOS[name]
    got = checked(ctx, events, heap, n)
    if name == "no_events":
        assert not got["value_acc"].any() and not got["id"].any() and (got["id_other"] == cp.fr_numpy([1])[0]).all()
    if name == "an_event_cut_at_n":
        assert got["rlc_acc"][:100].any() and not got["rlc_acc"][100:].any()


def test_an_event_boundary_at_every_even_offset_behind_a_block_of_steps(ctx):
    """a boundary on the even rows 2 STEP_BLOCK, .., 2 STEP_BLOCK + 64: the first steps of the second workgroup of each thread"""
    heap = heap_of(5000, 7)
    firsts = [busy_event(STEP_BLOCK + k, len(heap), dst_tag=cp.TX_LOG) for k in range(33)]
    sweep(ctx, firsts, busy_event(70, len(heap), src_tag=cp.TX_CALLDATA), heap, "run_rlc", NAMES)


def test_a_block_edge_at_every_word_index_of_an_event(ctx):
    """a first event of k steps pushes a 2200-step event along: step STEP_BLOCK of the call is its step 2048 - k, every s mod 32, and
    the lanes of eight steps enter its words at every offset"""
    heap = heap_of(5000, 8)
    firsts = [cp.event(k, cp.BYTECODE, cp.MEMORY, src_off=k, src_front=k // 2, src_id=3, dst_id=4) for k in range(34)]
    sweep(ctx, firsts, busy_event(2200, len(heap), src_back=100, dst_front=2100), heap, "run_rlc", NAMES)


def test_masks_of_every_kind_across_a_block_edge(ctx):
    """wholly masked threads, masks that meet, a padded read from the first step on: identity maps and constant maps at the edge"""
    heap = heap_of(5000, 9)
    L = STEP_BLOCK + 40
    events = [busy_event(L, len(heap), src_front=L, src_back=0, dst_front=0, dst_back=L), busy_event(L, len(heap), src_front=STEP_BLOCK - 1, src_back=41, dst_front=STEP_BLOCK, dst_back=39),
              busy_event(100, len(heap), src_addr_end=0, dst_tag=cp.RLC_ACC), busy_event(L, len(heap), src_front=0, src_back=0, dst_front=0, dst_back=0, src_addr_end=40 + STEP_BLOCK - 3)]
    checked(ctx, events, heap, 2 * (3 * L + 100) + 5)


def test_value_acc_across_the_windows_of_the_block_maps(ctx):
    """WINDOW_N = 2 x 256 x 2048 + 1 rows, the one case above 2^14: 257 workgroups of steps per thread, so that k_affine_b carries a
    value from its first window of 256 block maps into a second one.  value_acc alone, against A_t(s) as a tight loop that the
    closed forms confirm on the first rows."""
    heap = heap_of(9000, 10)
    events = [busy_event(8000 + 13 * k, len(heap), seed=k, src_addr_end=40 + 7000) for k in range(64)]
    n = dev.WINDOW_N
    assert sum(2 * e["length"] for e in events) > n
    d = Device(ctx, events, heap, n, rows_outputs=(), rlc_outputs=())
    try:
        got = d.split(d.run_rlc())["value_acc"]
        want = np.zeros((n, 4), np.uint64)
        for t in range(2):
            column = dev.value_acc_only(events, heap, n, t)
            assert column[:2048] == cp.closed(events, heap, 4096, R_WORD, R_IN)["value_acc"][t::2]
            want[t::2] = cp.fr_numpy(column)
        diff = (got != want).any(axis=1)
        assert not diff.any(), np.argwhere(diff)[:5].ravel().tolist()
    finally:
        d.free()


def test_no_rows_writes_nothing(ctx):
    heap = heap_of(100)
    d = Device(ctx, [busy_event(20, len(heap))], heap, 0, n_alloc=8, rows_outputs=())
    try:
        assert (d.run_rlc() == SENT).all()
    finally:
        d.free()


def test_events_that_do_not_count_are_empty_events(ctx):
    heap = heap_of(500, 9)
    total = 400
    good = busy_event(30, total, src_off=370, dst_off=0, prev_off=370, dst_tag=cp.RLC_ACC)
    bad = [dict(good, src_tag=0), dict(good, dst_tag=6), dict(good, flags=2), dict(good, reserved=1), dict(good, src_off=371), dict(good, dst_off=371), dict(good, prev_off=371),
           dict(good, src_off=2**64 - 1), dict(good, length=2**32 - 1, src_off=1)]
    events = [good] + [x for e in bad for x in (dict(e, src_id=77), good)]
    got = checked(ctx, events, heap, 2 * 30 * (len(bad) + 1) + 20, total=total)
    assert not (got["id"] == cp.fr_numpy([77])[0]).all(axis=1).any()


@pytest.mark.parametrize("name", RLC_OUTPUTS + ("none",))
def test_each_output_alone(ctx, name):
    events, heap, n = SCENARIOS["mixed_random_events"]
    checked(ctx, events, heap, n, rlc_outputs=() if name == "none" else (name,))


def test_without_ids_the_rows_of_events_hold_zero(ctx):
    events, heap, n = SCENARIOS["mixed_random_events"]
    got = checked(ctx, events, heap, n, ids=False)
    assert not got["id"].any() and (got["id_other"][-11:] == cp.fr_numpy([1])[0]).all() and not got["id_other"][:-11].any()


def test_challenges_that_are_not_reduced_are_taken_mod_r(zk, ctx):
    """r_word + r and r_in + r as limbs (both below 2^256): the same columns"""
    events, heap, n = SCENARIOS["an_event_cut_at_n"]
    d = Device(ctx, events, heap, n, rows_outputs=())
    try:
        mont = lambda v: np.frombuffer(((v * 2**256 % cp.R) + cp.R).to_bytes(32, "little"), dtype=np.uint64)   # noqa: E731
        ctx.copy_rlc(d.d_events, d.count, d.d_bytes, d.total, n, d.ptr("value_acc"), mont(R_WORD), mont(R_IN), ids=d.ids.ptr, **{x: d.ptr(x) for x in RLC_OUTPUTS})
        ctx.sync()
        d.written = set(NAMES)
        d.check(d.image())
    finally:
        d.free()


def test_the_profilers_byte_count(ctx):
    events, heap, n = SCENARIOS["mixed_random_events"]
    d = Device(ctx, events, heap, n, rows_outputs=(), rlc_outputs=("rlc_acc", "word_rlc"))
    try:
        ctx.prof_enable(True)
        ctx.prof_reset()
        d.run_rlc()
        assert ctx.prof_get("copy_rlc")[1] == 1
        assert ctx.prof_get_bytes("copy_rlc") == (88 + 64) * len(events) + len(heap) + n * 32 * 3
    finally:
        ctx.prof_enable(False)
        d.free()


def test_the_same_call_twice_gives_the_same_bytes(ctx):
    events, heap, n = SCENARIOS["overlapping_and_repeated_runs"]
    d = Device(ctx, events, heap, n, rows_outputs=())
    try:
        first = d.run_rlc()
        assert np.array_equal(first, d.run_rlc())
    finally:
        d.free()


def test_refusals_leave_the_outputs_untouched_and_the_context_usable(zk, ctx):
    b = zk.binding
    rng = np.random.default_rng(13)
    n = 150
    heap = heap_of(300, 12)
    d = Device(ctx, [busy_event(40, len(heap)), busy_event(20, len(heap))], heap, n, rows_outputs=())
    vals = [[int.from_bytes(rng.bytes(31), "little") for _ in range(4)] for _ in range(2)]
    x, y = (ctx.to_device(cp.fr_numpy(v)) for v in vals)
    add_out = ctx.alloc(128)
    ch = np.ascontiguousarray(np.concatenate([cp.fr_numpy([R_WORD])[0], cp.fr_numpy([R_IN])[0]]))

    def desc(**change):
        f = dict(d_events=d.d_events, count=d.count, d_bytes=d.d_bytes, total_bytes=d.total, flags=0, d_ids=d.ids.ptr)
        f.update({"d_" + name: d.ptr(name) for name in RLC_OUTPUTS})
        f.update(change)
        return b._CopyRlc(*[f[name] for name, _ in b._CopyRlc._fields_])

    def call(ds, field=0, op=30, rows=n, out=None, d_b=ch.ctypes.data_as(ctypes.c_void_p)):
        return zk.lib().zk_field_vec_op(ctx.h, field, op, ctypes.byref(ds), d_b, ctypes.c_void_p(d.ptr("value_acc") if out is None else out), ctypes.c_size_t(rows))

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
        refused(desc(), "no challenges", d_b=None)
        refused(desc(flags=1), "flags")
        refused(desc(flags=1), "validated before n is looked at", rows=0)
        refused(desc(d_events=None), "NULL d_events")
        refused(desc(d_events=d.d_events + 4), "misaligned d_events")
        refused(desc(d_bytes=None), "NULL d_bytes with bytes")
        refused(desc(total_bytes=2**61), "total_bytes = 2^61")
        refused(desc(), "n = 2^32", rows=2**32)
        refused(desc(), "d_out at 8", out=d.ptr("value_acc") + 8)
        for name in RLC_OUTPUTS:
            refused(desc(**{"d_" + name: d.ptr(name) + 8}), f"misaligned {name}")
        # overlaps: an output with an input, with d_out, with another output
        refused(desc(d_id=d.ids.ptr + 16), "d_id inside d_ids")
        refused(desc(d_word_rlc=d.d_events + 80), "d_word_rlc over the end of d_events")
        refused(desc(d_rlc_acc=d.src.ptr + GUARD + 16 - (d.src.ptr + GUARD) % 16), "d_rlc_acc inside d_bytes")
        refused(desc(d_id_other=d.ptr("value_acc") + 32 * n - 16), "d_id_other over the last bytes of d_out")
        refused(desc(d_word_rlc_prev=d.ptr("word_rlc")), "d_word_rlc_prev is d_word_rlc")
        assert call(desc(), rows=0) == OK
        ctx.sync()
        assert (d.image() == SENT).all()
        assert call(desc(d_events=None, count=0, d_bytes=None, total_bytes=0, d_ids=None)) == OK
        ctx.sync()
        d.written = set(NAMES)
        d.check(d.image(), want_arrays([], b"", n, NAMES))
        d.clear()
        d.check(d.run_rlc())
    finally:
        for buf_ in (x, y, add_out):
            buf_.free()
        d.free()

"""GPU: ZK_OP_EXP_ROWS of zk_field_vec_op -- every output byte for byte against the closed forms of tests/exp_rows_cases.py (which
tests/test_exp_rows_model.py holds against the reference's serial loop), through the C ABI, with sentinels in front of and behind
every buffer.  1024 rows (128 steps) is the implementation's tile, 2048 entries its scan tile; no call runs more than 2^15 rows."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import exp_rows_cases as ex  # noqa: E402
from exp_rows_device import GUARD, INVALID_ARG, OK, OUT, OUTPUTS, SCENARIOS, SENT, Device, scenario_want, want_bytes  # noqa: E402
from oracle import bn254  # noqa: E402

pytestmark = pytest.mark.gpu
R = bn254.R_MOD
FEW = "n_one_step_more"                      # four events, 15 steps and one pad step: the scenario of the small tests


def checked(ctx, events, n, want=None, **kw):
    d = Device(ctx, events, n, **kw)
    try:
        return d.check(d.run(), want)
    finally:
        d.free()


@pytest.mark.parametrize("name", sorted(SCENARIOS))
def test_scenario(ctx, name):
    """every output, d_rows_needed exact (also where n cuts the events), nothing outside the outputs written"""
    events, n = SCENARIOS[name]
    checked(ctx, events, n, scenario_want(name))


@pytest.mark.parametrize("name", OUTPUTS + ("none", "all_but_the_u16_planes"))
def test_each_output_alone(ctx, name):
    events, n = SCENARIOS["mixed_random_events"]
    outputs = () if name == "none" else tuple(o for o in OUTPUTS if o not in ex.U16_OUTPUTS) if name == "all_but_the_u16_planes" else (name,)
    checked(ctx, events, n, scenario_want("mixed_random_events"), outputs=outputs, rows_needed=name != "none")


def test_small_cells_at_addresses_that_are_no_multiple_of_four(ctx):
    """is_last at an odd address, the u16 planes at 2 mod 4, with n odd, even and 2 mod 4 so that every plane starts differently"""
    events, _ = SCENARIOS["mixed_random_events"]
    for n in (19, 70, 1024 + 27, 2048 + 18):
        checked(ctx, events, n, odd=True)
        checked(ctx, events, n, outputs=("mul_u16_64", "is_last"), odd=False)


def test_no_rows_writes_nothing(ctx):
    events, _ = SCENARIOS[FEW]
    d = Device(ctx, events, 0, n_alloc=8)
    try:
        assert (d.run() == SENT).all()
    finally:
        d.free()


def test_garbage_records_read_nothing_else_and_are_a_pure_function(ctx):
    """random 64-byte records: whatever they hold they are a base and an exponent; two calls give identical bytes"""
    rng = np.random.default_rng(77)
    events = [(int.from_bytes(rng.bytes(32), "little"), int.from_bytes(rng.bytes(int(rng.integers(0, 5))), "little")) for _ in range(300)]
    d = Device(ctx, events, 3000)
    try:
        first = d.check(d.run())
        assert np.array_equal(first, d.run())
    finally:
        d.free()


def test_the_same_call_twice_gives_the_same_bytes(ctx):
    events, n = SCENARIOS["one_510_step_event_across_four_tiles"]
    d = Device(ctx, events, n)
    try:
        first = d.run()
        d.clear()
        assert np.array_equal(first, d.check(d.run(), scenario_want("one_510_step_event_across_four_tiles")))
    finally:
        d.free()


def test_the_profilers_byte_count(ctx):
    events, n = SCENARIOS[FEW]
    d = Device(ctx, events, n, outputs=("is_last", "mul_cols", "parity_u16_128"))
    try:
        ctx.prof_enable(True)
        ctx.prof_reset()
        d.run()
        assert ctx.prof_get("exp_rows")[1] == 1
        assert ctx.prof_get_bytes("exp_rows") == 64 * len(events) + n * (16 + 1 + 64 + 16)
        d.free()
        d = Device(ctx, events, n)
        ctx.prof_reset()
        d.run()
        assert ctx.prof_get_bytes("exp_rows") == 64 * len(events) + n * (16 + 1 + 8 + 16 + 2 * (64 + 8 + 16))
    finally:
        ctx.prof_enable(False)
        d.free()


def test_refusals_leave_the_outputs_untouched_and_the_context_usable(zk, ctx):
    b = zk.binding
    rng = np.random.default_rng(12)
    events, n = SCENARIOS[FEW]
    d = Device(ctx, events, n)
    vals = [[int.from_bytes(rng.bytes(31), "little") for _ in range(4)] for _ in range(2)]
    fr = lambda vs: np.frombuffer(b"".join(bn254.mont_bytes(v, R) for v in vs), dtype=np.uint64).reshape(len(vs), 4).copy()   # noqa: E731
    x, y = (ctx.to_device(fr(v)) for v in vals)
    add_out = ctx.alloc(128)
    host = np.zeros(8, np.uint64)

    def desc(**change):
        f = dict(d_events=d.d_events, count=d.count, flags=0, d_rows_needed=d.ptr("rows_needed"))
        f.update({"d_" + name: d.ptr(name) for name in OUTPUTS})
        f.update(change)
        return b._ExpRows(*[f[name] for name, _ in b._ExpRows._fields_])

    def call(ds, field=0, op=32, rows=n, out=None, d_b=None):
        return zk.lib().zk_field_vec_op(ctx.h, field, op, ctypes.byref(ds), d_b, ctypes.c_void_p(d.ptr(OUT) if out is None else out), ctypes.c_size_t(rows))

    def refused(ds, why, **kw):
        rc = call(ds, **kw)
        ctx.sync()
        assert rc == INVALID_ARG, why
        assert (d.image() == SENT).all(), why
        # a valid ZK_OP_ADD follows every refusal
        assert zk.lib().zk_field_vec_op(ctx.h, 0, 0, ctypes.c_void_p(x.ptr), ctypes.c_void_p(y.ptr), ctypes.c_void_p(add_out.ptr), ctypes.c_size_t(4)) == OK, why
        ctx.sync()
        assert [bn254.from_mont_bytes(bytes(r), R) for r in add_out.download((4, 32), np.uint8)] == [(u + v) % R for u, v in zip(*vals)], why

    try:
        refused(desc(), "Fq", field=1)
        refused(desc(), "Fq is looked at before n", field=1, rows=0)
        refused(desc(flags=1), "flags")
        refused(desc(flags=1), "validated before n is looked at", rows=0)
        refused(desc(d_events=None), "NULL d_events")
        refused(desc(d_events=d.d_events + 4), "misaligned d_events")
        refused(desc(), "n = 2^32", rows=2**32)
        refused(desc(), "d_out at 8", out=d.ptr(OUT) + 8)
        for name, off in (("exponent_lo_hi", 8), ("mul_cols", 8), ("parity_cols", 8), ("base_limb", 4), ("rows_needed", 4), ("mul_u16_64", 1), ("mul_u16_128", 1), ("parity_u16_64", 1),
                          ("parity_u16_128", 1)):
            refused(desc(**{"d_" + name: d.ptr(name) + off}), f"misaligned {name}")
        refused(desc(), "a second operand", d_b=host.ctypes.data_as(ctypes.c_void_p))
        refused(desc(), "a second operand, before n", d_b=host.ctypes.data_as(ctypes.c_void_p), rows=0)
        # overlaps: an output with the events, with d_out, with another output
        refused(desc(d_is_last=d.d_events + 64 * d.count - 1), "d_is_last over the last byte of d_events")
        refused(desc(d_rows_needed=d.d_events), "d_rows_needed over the first event")
        refused(desc(d_is_last=d.ptr(OUT) + 16 * n - 1), "d_is_last over the last byte of d_out")
        refused(desc(d_base_limb=d.ptr("mul_cols") + 64 * n - 8), "d_base_limb over the last cell of the fourth plane of d_mul_cols")
        refused(desc(d_mul_u16_64=d.ptr("parity_u16_128") + 16 * n - 2), "d_mul_u16_64 over the last cell of the eighth plane of d_parity_u16_128")
        refused(desc(d_parity_cols=d.ptr("mul_cols")), "d_parity_cols is d_mul_cols")
        refused(desc(d_is_last=d.ptr("rows_needed") + 7), "d_is_last over the last byte of d_rows_needed")
        assert zk.lib().zk_field_vec_op(ctx.h, 0, 31, ctypes.c_void_p(x.ptr), ctypes.c_void_p(y.ptr), ctypes.c_void_p(d.ptr(OUT)), ctypes.c_size_t(4)) == INVALID_ARG
        refused(desc(), "op 31", op=31, rows=4, d_b=host.ctypes.data_as(ctypes.c_void_p))
        # and the accepted neighbours: n = 0 with a valid descriptor, count = 0 without events
        assert call(desc(), rows=0) == OK
        ctx.sync()
        assert (d.image() == SENT).all()
        assert call(desc(d_events=None, count=0, d_rows_needed=None)) == OK
        ctx.sync()
        image = d.image()
        want = want_bytes([], n)
        for name in (OUT,) + OUTPUTS:
            assert np.array_equal(image[d.at[name]:d.at[name] + len(want[name])], want[name]), name
        d.clear()
        d.check(d.run(), scenario_want(FEW))
    finally:
        for buf_ in (x, y, add_out):
            buf_.free()
        d.free()

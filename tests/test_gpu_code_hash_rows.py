"""GPU: ZK_OP_CODE_HASH_ROWS of zk_field_vec_op -- every output byte for byte against the model of tests/code_hash_rows_cases.py (the
reference's assign_extended_row and set_header_row in Python), with sentinels in front of and behind every buffer.

T = 1024 is the implementation's tile: a workgroup takes T rows.  The alignment sweep puts a 130-byte code behind a first bytecode
of every length in 0 .. 70, T - 70 .. T + 70 and 2 T - 35 .. 2 T + 35 with n = 3 T, so that every phase of the 31- and 62-byte
periods of both codes, and the up to 30 bytes a row needs in front of its own, meet a tile boundary; the large case fills 2^19 rows
with one random code beside small ones."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import code_hash_rows_cases as ch  # noqa: E402
from code_hash_rows_device import GUARD, INVALID_ARG, OK, SENT, Call, T, checked  # noqa: E402
from oracle import bn254  # noqa: E402

pytestmark = pytest.mark.gpu
OUTPUTS = tuple(c for c in ch.ROW_COLUMNS if c != "field_input")
SWEEPS = {"0..70": range(0, 71), "T-70..T+70": range(T - 70, T + 71), "2T-35..2T+35": range(2 * T - 35, 2 * T + 36)}


@pytest.mark.parametrize("span", list(SWEEPS))
def test_alignment_sweep_of_a_130_byte_code_against_the_tile_boundaries(ctx, span):
    """one arena and one n for all lengths: only the first length changes, on the device"""
    rng = np.random.default_rng(130)
    n = 3 * T
    buf, offs, lens = ch.lay_out([ch.random_code(rng, 2 * T + 35), ch.random_code(rng, 130)], rng, 3)
    call = Call(ctx, "rows", n, buf, offs, lens)
    try:
        for j in SWEEPS[span]:
            call.set_lens([j, 130])
            call.compare(call.split(call.run()), call.want(), j)
    finally:
        call.free()


def test_the_lengths_around_one_and_two_fields_side_by_side(ctx):
    rng = np.random.default_rng(1)
    got = checked(ctx, "rows", [ch.random_code(rng, k) for k in (0, 1, 30, 31, 32, 61, 62, 63, 124)])
    assert int(got["is_field_border"].sum()) == sum(-(-k // 31) for k in (0, 1, 30, 31, 32, 61, 62, 63, 124))


@pytest.mark.parametrize("n", [31, 32, 33, T + 61, T + 62, T + 63])
def test_a_bytecode_cut_at_n_around_a_field_border(ctx, n):
    """byte p stands on row p + 1 and p = 30 and p = T + 60 end a field: the last row written is the row before the border, the
    border row, the row behind it"""
    assert 30 % 31 == 30 and (T + 60) % 31 == 30
    rng = np.random.default_rng(n)
    checked(ctx, "rows", [ch.random_code(rng, T + 300), ch.random_code(rng, 40)], n=n)


def test_n_smaller_than_the_first_header_of_the_second_bytecode_and_of_everything(ctx):
    rng = np.random.default_rng(2)
    codes = [ch.random_code(rng, 100), ch.random_code(rng, 100)]
    for n in (1, 100, 101, 102):
        checked(ctx, "rows", codes, n=n)
    checked(ctx, "rows", [ch.random_code(rng, 1)] * 40, n=17)           # more bytecodes than rows


def test_no_bytecodes_is_all_header_rows_of_length_zero(ctx):
    call = Call(ctx, "rows", T + 500, np.zeros(0, np.uint8), [], [])
    try:
        got = call.check()
        assert not got["field_input"].any() and not got["control_length"].any() and (got["field_index"] == 1).all()
    finally:
        call.free()


def test_no_rows(ctx):
    buf, offs, lens = ch.lay_out([bytes(range(1, 71))])
    call = Call(ctx, "rows", 0, buf, offs, lens, n_alloc=8)
    try:
        assert (call.run() == SENT).all()
    finally:
        call.free()


@pytest.mark.parametrize("iw", [4, 8])
def test_invalid_entries_between_valid_ones_count_as_empty(ctx, iw):
    rng = np.random.default_rng(iw)
    buf = np.frombuffer(ch.random_code(rng, 400), dtype=np.uint8)
    top = 2**(8 * iw)
    offs = [0, 401, 10, 390, top - 1, 100, top - 4, 400, 0, 50]
    lens = [70, 0, top - 1, 11, 1, 33, 8, 0, 401, top - 50]
    call = Call(ctx, "rows", 70 + 33 + 10 + 40, buf, offs, lens, iw=iw)
    try:
        call.check()
    finally:
        call.free()


def test_unaligned_overlapping_and_repeated_bytecodes(ctx):
    rng = np.random.default_rng(5)
    buf = np.frombuffer(ch.random_code(rng, 600), dtype=np.uint8)
    offs = [1, 2, 3, 1, 1, 250, 251, 599, 0, 7]
    lens = [100, 99, 98, 100, 599, 77, 77, 1, 600, 5]
    call = Call(ctx, "rows", sum(lens) + len(lens) + 9, buf, offs, lens)
    try:
        call.check()
    finally:
        call.free()


def test_one_byte_outputs_at_odd_addresses(ctx):
    rng = np.random.default_rng(6)
    for n in (3, 70, T + 7, 2 * T + 3):
        checked(ctx, "rows", [ch.random_code(rng, 2 * T + 200), ch.random_code(rng, 70)], n=n, odd=True)


@pytest.mark.parametrize("name", ("none",) + OUTPUTS)
def test_each_output_alone(ctx, name):
    rng = np.random.default_rng(8)
    checked(ctx, "rows", [ch.random_code(rng, 70), ch.random_code(rng, T + 50), b"", ch.random_code(rng, 63)], outputs=() if name == "none" else (name,))


def test_one_bytecode_that_fills_2_19_rows_beside_small_ones(ctx):
    rng = np.random.default_rng(19)
    small = [ch.random_code(rng, int(k)) for k in rng.integers(0, 70, 6)]
    n = 1 << 19
    big = ch.random_code(rng, n - sum(len(c) + 1 for c in small) - 1 - 2)
    checked(ctx, "rows", small[:3] + [big] + small[3:], n=n)


def test_the_same_call_twice_gives_the_same_bytes(ctx):
    rng = np.random.default_rng(10)
    buf, offs, lens = ch.lay_out([ch.random_code(rng, 5 * T), ch.random_code(rng, 70), b"", ch.random_code(rng, 700)])
    call = Call(ctx, "rows", sum(lens) + 4 + 50, buf, offs, lens)
    try:
        first = call.run()
        assert np.array_equal(first, call.run())
        call.check()
    finally:
        call.free()


def test_refusals_leave_the_outputs_untouched_and_the_context_usable(zk, ctx):
    b = zk.binding
    rng = np.random.default_rng(12)
    n = 150
    buf, offs, lens = ch.lay_out([ch.random_code(rng, 70), ch.random_code(rng, 70)])
    call = Call(ctx, "rows", n, buf, offs, lens)
    vals = [[int.from_bytes(rng.bytes(31), "little") for _ in range(4)] for _ in range(2)]
    x, y = (ctx.to_device(ch.to_mont(v)) for v in vals)
    add_out = ctx.alloc(128)
    some = np.zeros(4, dtype=np.uint64)

    def desc(**change):
        kw = call.kwargs()
        f = dict(d_bytes=kw["data"], total_bytes=kw["total_bytes"], d_offsets=kw["offsets"], d_lens=kw["lens"], count=call.count, index_width=4, flags=0)
        f.update({"d_" + name: kw[name] for name in OUTPUTS})
        f.update(change)
        return b._CodeHashRows(*[f[name] for name, _ in b._CodeHashRows._fields_])

    def refused(d, field=0, op=34, rows=n, out=None, d_b=None, why=""):
        rc = zk.lib().zk_field_vec_op(ctx.h, field, op, ctypes.byref(d), d_b, ctypes.c_void_p(call.ptr("field_input") if out is None else out), ctypes.c_size_t(rows))
        ctx.sync()
        assert rc == INVALID_ARG, why
        assert (call.arena.download(call.size, np.uint8) == SENT).all(), why
        assert zk.lib().zk_field_vec_op(ctx.h, 0, 0, ctypes.c_void_p(x.ptr), ctypes.c_void_p(y.ptr), ctypes.c_void_p(add_out.ptr), ctypes.c_size_t(4)) == OK, why
        ctx.sync()
        got = add_out.download((4, 4))
        assert np.array_equal(got, ch.to_mont([(u + v) % bn254.R_MOD for u, v in zip(*vals)])), why

    try:
        refused(desc(), field=1, why="Fq")
        refused(desc(), field=1, rows=0, why="Fq is looked at before n")
        refused(desc(), d_b=some.ctypes.data_as(ctypes.c_void_p), why="a second operand")
        for iw in (0, 1, 2, 3, 5, 16):
            refused(desc(index_width=iw), why=f"index_width {iw}")
        refused(desc(flags=1), why="flags")
        refused(desc(flags=1), rows=0, why="validated before n is looked at")
        refused(desc(d_offsets=None), why="NULL d_offsets")
        refused(desc(d_lens=None), why="NULL d_lens")
        refused(desc(d_offsets=call.d_offs.ptr + 2), why="misaligned d_offsets")
        refused(desc(d_lens=call.d_lens.ptr + 1), why="misaligned d_lens")
        refused(desc(d_bytes=None), why="NULL d_bytes with bytes")
        refused(desc(), out=call.ptr("field_input") + 8, why="d_out at 8")
        for name in ("bytes_in_field_inv", "padding_shift"):
            refused(desc(**{"d_" + name: call.ptr(name) + 8}), why=f"{name} at 8")
        refused(desc(d_control_length=call.ptr("control_length") + 2), why="misaligned control_length")
        refused(desc(), rows=2**32, why="n = 2^32")
        refused(desc(total_bytes=2**61), why="total_bytes = 2^61")
        # overlaps: an output with an input, with d_out, with another output
        refused(desc(d_field_index=call.src.ptr + GUARD + 10), why="d_field_index inside d_bytes")
        refused(desc(d_is_field_border=call.d_lens.ptr), why="d_is_field_border over d_lens")
        refused(desc(d_control_length=call.d_offs.ptr + 4), why="d_control_length over d_offsets")
        refused(desc(d_field_index_inv=call.ptr("field_input") + 32 * n - 1), why="d_field_index_inv over the last byte of d_out")
        refused(desc(d_bytes_in_field_index=call.ptr("field_index") + n - 1), why="d_bytes_in_field_index over the last byte of d_field_index")
        refused(desc(d_padding_shift=call.ptr("bytes_in_field_inv")), why="d_padding_shift is d_bytes_in_field_inv")
        for op in (33, 35):
            rc = zk.lib().zk_field_vec_op(ctx.h, 0, op, ctypes.c_void_p(x.ptr), ctypes.c_void_p(y.ptr), ctypes.c_void_p(call.ptr("field_input")), ctypes.c_size_t(4))
            assert rc == INVALID_ARG, op
            refused(desc(), op=op, rows=4, d_b=some.ctypes.data_as(ctypes.c_void_p), why=f"op {op}")
        # and the accepted neighbours of some refusals: n = 0 with a valid descriptor
        assert zk.lib().zk_field_vec_op(ctx.h, 0, 34, ctypes.byref(desc()), None, ctypes.c_void_p(call.ptr("field_input")), ctypes.c_size_t(0)) == OK
        ctx.sync()
        assert (call.arena.download(call.size, np.uint8) == SENT).all()
        call.check()
    finally:
        for buf_ in (x, y, add_out):
            buf_.free()
        call.free()

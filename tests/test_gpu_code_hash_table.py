"""GPU: ZK_OP_CODE_HASH_TABLE of zk_field_vec_op -- every output byte for byte against the model of tests/code_hash_rows_cases.py (the
reference's PoseidonTable::dev_load over unroll_to_hash_input in Python), with sentinels in front of and behind every buffer, and its
outputs through ZK_OP_POSEIDON against the reference-held code hashes.

T = 1024 is the implementation's tile, in table rows: a bytecode of K blocks of 62 bytes owns K rows.  The sweep puts a 130-byte code
(three rows) behind a first bytecode of K = 0 .. 70, T - 70 .. T + 70 and 2 T - 35 .. 2 T + 35 blocks with n = 3 T, each K at the
lengths 62 K - 1, 62 K and 62 K + 1."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import code_hash_rows_cases as ch  # noqa: E402
import poseidon_cases as pc  # noqa: E402
from code_hash_rows_device import GUARD, INVALID_ARG, OK, SENT, Call, T, checked  # noqa: E402

pytestmark = pytest.mark.gpu
OUTPUTS = ("input1", "control", "heading_mark", "kinds", "cap", "rows_needed")
SWEEPS = {"0..70": range(0, 71), "T-70..T+70": range(T - 70, T + 71), "2T-35..2T+35": range(2 * T - 35, 2 * T + 36)}


@pytest.mark.parametrize("span", list(SWEEPS))
def test_alignment_sweep_in_block_space(ctx, span):
    """one arena and one n for all lengths: only the first length changes, on the device"""
    rng = np.random.default_rng(62)
    n = 3 * T
    buf, offs, lens = ch.lay_out([ch.random_code(rng, 62 * (2 * T + 35) + 1), ch.random_code(rng, 130)], rng, 3)
    call = Call(ctx, "table", n, buf, offs, lens)
    try:
        for k in SWEEPS[span]:
            for length in (62 * k - 1, 62 * k, 62 * k + 1):
                if length >= 0:
                    call.set_lens([length, 130])
                    call.compare(call.split(call.run()), call.want(), length)
    finally:
        call.free()


def test_the_lengths_around_one_and_two_fields_side_by_side(ctx):
    rng = np.random.default_rng(1)
    lengths = (0, 1, 30, 31, 32, 61, 62, 63, 93, 124, 125, 500)
    got = checked(ctx, "table", [ch.random_code(rng, k) for k in lengths])
    assert int(got["heading_mark"].sum()) == len(lengths) - 1 and int(got["rows_needed"].view("<u8")[0]) == sum(-(-k // 62) for k in lengths)


@pytest.mark.parametrize("delta", [-1, 0, 1])
def test_n_below_at_and_above_the_rows_needed(ctx, delta):
    """d_rows_needed is exact and unsaturated in all three, also where most bytecodes do not fit"""
    rng = np.random.default_rng(3)
    codes = [ch.random_code(rng, int(k)) for k in rng.integers(0, 400, 60)] + [ch.random_code(rng, 62 * T)]
    needed = sum(-(-len(c) // 62) for c in codes)
    got = checked(ctx, "table", codes, n=needed + delta)
    assert int(got["rows_needed"].view("<u8")[0]) == needed
    got = checked(ctx, "table", codes, n=7)
    assert int(got["rows_needed"].view("<u8")[0]) == needed


def test_no_bytecodes_and_only_empty_ones_are_all_off(ctx):
    for codes in ([], [b""] * 300):
        buf, offs, lens = ch.lay_out(codes)
        call = Call(ctx, "table", T + 5, buf, offs, lens)
        try:
            got = call.check()
            assert (got["kinds"] == ch.OFF).all() and not got["input0"].any() and not got["rows_needed"].any()
        finally:
            call.free()


def test_no_rows_writes_nothing(ctx):
    buf, offs, lens = ch.lay_out([bytes(range(1, 71))])
    call = Call(ctx, "table", 0, buf, offs, lens, n_alloc=8)
    try:
        image = call.run()
        call.split(image, written=False)
        assert (image == SENT).all()
    finally:
        call.free()


@pytest.mark.parametrize("iw", [4, 8])
def test_invalid_entries_between_valid_ones_own_no_row(ctx, iw):
    rng = np.random.default_rng(iw)
    buf = np.frombuffer(ch.random_code(rng, 400), dtype=np.uint8)
    top = 2**(8 * iw)
    offs = [0, 401, 10, 390, top - 1, 100, top - 4, 400, 0, 50]
    lens = [70, 0, top - 1, 11, 1, 33, 8, 0, 401, top - 50]
    call = Call(ctx, "table", 9, buf, offs, lens, iw=iw)
    try:
        got = call.check()
        assert int(got["rows_needed"].view("<u8")[0]) == 2 + 1          # the 70 bytes at 0 and the 33 at 100; 390 + 11 leaves the buffer
    finally:
        call.free()


def test_unaligned_overlapping_and_repeated_bytecodes_at_odd_addresses(ctx):
    rng = np.random.default_rng(5)
    buf = np.frombuffer(ch.random_code(rng, 600), dtype=np.uint8)
    offs = [1, 2, 3, 1, 1, 250, 251, 599, 0, 7, 538]
    lens = [100, 99, 98, 100, 599, 77, 77, 1, 600, 5, 62]
    for odd in (False, True):
        call = Call(ctx, "table", 40, buf, offs, lens, odd=odd)
        try:
            call.check()
        finally:
            call.free()


@pytest.mark.parametrize("name", ("none",) + OUTPUTS)
def test_each_output_alone(ctx, name):
    rng = np.random.default_rng(8)
    checked(ctx, "table", [ch.random_code(rng, 70), ch.random_code(rng, 62 * T + 50), b"", ch.random_code(rng, 63)], outputs=() if name == "none" else (name,))


def test_2_19_rows_of_one_long_code_beside_small_ones(ctx):
    rng = np.random.default_rng(19)
    small = [ch.random_code(rng, int(k)) for k in rng.integers(0, 200, 6)]
    n = 1 << 19
    big = ch.random_code(rng, 62 * (n - sum(-(-len(c) // 62) for c in small) - 2) - 17)
    got = checked(ctx, "table", small[:3] + [big] + small[3:], n=n)
    assert int(got["rows_needed"].view("<u8")[0]) == n - 2


def mont_words(vals):
    return ch.to_mont(vals)


def test_the_reference_code_hashes_through_the_table_op_and_the_poseidon_op(ctx):
    """each of the five codes of poseidon_code_hash.json through ZK_OP_CODE_HASH_TABLE and then ZK_OP_POSEIDON (FINAL, widths 32,
    cap_width 8, cap_scale 2^64, the kinds): the reference-held hash on every row of the code -- no host re-packing -- and input0,
    input1 are the word0, word1 that ZK_OP_POSEIDON makes from the padded width-31 layout of the same codes"""
    vectors = pc.golden_vectors()
    codes = [code for code, _ in vectors]
    assert [len(c) for c in codes][:4] == [0, 1, 2, 32] and 5036 in [len(c) for c in codes]
    buf, offs, lens = ch.lay_out(codes)
    needed = sum(-(-len(c) // 62) for c in codes)
    n = needed + 2
    call = Call(ctx, "table", n, buf, offs, lens)
    hash_id = ctx.to_device(np.full((n + 2, 4), 0xC3C3C3C3C3C3C3C3, dtype=np.uint64))
    # the padded layout of the codes that own a row, for the poseidon op's width 31
    data, kinds, caps = pc.code_rows([c for c in codes if c])
    assert len(kinds) == needed
    padded = ctx.to_device(np.frombuffer(b"\xee" + data, dtype=np.uint8))
    d_cap = ctx.to_device(np.array(caps, dtype=np.uint64))
    d_kinds = ctx.to_device(np.array(kinds, dtype=np.uint8))
    words = [ctx.to_device(np.zeros((needed, 4), dtype=np.uint64)) for _ in range(3)]
    scale = mont_words([pc.CAP_SCALE_CODE])[0]
    try:
        got = call.check()
        ctx.poseidon(call.ptr("input0"), 32, call.ptr("input1"), 32, n, hash_id.ptr + 32, cap=call.ptr("cap"), cap_width=8, cap_scale=scale, kinds=call.ptr("kinds"), final=True)
        ctx.sync()
        out = hash_id.download((n + 2, 4))
        assert (out[0] == 0xC3C3C3C3C3C3C3C3).all() and (out[n + 1] == 0xC3C3C3C3C3C3C3C3).all()
        want = [h for code, h in vectors for _ in range(-(-len(code) // 62))] + [0, 0]
        assert np.array_equal(out[1:n + 1], mont_words(want)), "hash_id"
        ctx.poseidon(padded.ptr + 1, 31, padded.ptr + 32, 31, needed, words[0], cap=d_cap, cap_width=8, cap_scale=scale, kinds=d_kinds, final=True, word0=words[1], word1=words[2])
        ctx.sync()
        assert np.array_equal(words[0].download((needed, 4)), out[1:needed + 1])
        assert np.array_equal(words[1].download((needed, 4)).view(np.uint8).reshape(-1), got["input0"][:32 * needed])
        assert np.array_equal(words[2].download((needed, 4)).view(np.uint8).reshape(-1), got["input1"][:32 * needed])
    finally:
        for b in [hash_id, padded, d_cap, d_kinds] + words:
            b.free()
        call.free()


def test_refusals_leave_the_outputs_untouched(zk, ctx):
    b = zk.binding
    rng = np.random.default_rng(12)
    n = 20
    buf, offs, lens = ch.lay_out([ch.random_code(rng, 70), ch.random_code(rng, 700)])
    call = Call(ctx, "table", n, buf, offs, lens)
    some = np.zeros(4, dtype=np.uint64)

    def desc(**change):
        kw = call.kwargs()
        f = dict(d_bytes=kw["data"], total_bytes=kw["total_bytes"], d_offsets=kw["offsets"], d_lens=kw["lens"], count=call.count, index_width=4, flags=0)
        f.update({"d_" + name: kw[name] for name in OUTPUTS})
        f.update(change)
        return b._CodeHashTable(*[f[name] for name, _ in b._CodeHashTable._fields_])

    def refused(d, field=0, op=36, rows=n, out=None, d_b=None, why=""):
        rc = zk.lib().zk_field_vec_op(ctx.h, field, op, ctypes.byref(d), d_b, ctypes.c_void_p(call.ptr("input0") if out is None else out), ctypes.c_size_t(rows))
        ctx.sync()
        assert rc == INVALID_ARG, why
        assert (call.arena.download(call.size, np.uint8) == SENT).all(), why

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
        refused(desc(), out=call.ptr("input0") + 8, why="d_out at 8")
        refused(desc(d_input1=call.ptr("input1") + 8), why="d_input1 at 8")
        refused(desc(d_control=call.ptr("control") + 8), why="d_control at 8")
        refused(desc(d_cap=call.ptr("cap") + 4), why="d_cap at 4")
        refused(desc(d_rows_needed=call.ptr("rows_needed") + 4), why="d_rows_needed at 4")
        refused(desc(), rows=2**32, why="n = 2^32")
        refused(desc(total_bytes=2**61), why="total_bytes = 2^61")
        refused(desc(d_kinds=call.src.ptr + GUARD + 10), why="d_kinds inside d_bytes")
        refused(desc(d_heading_mark=call.d_lens.ptr), why="d_heading_mark over d_lens")
        refused(desc(d_cap=call.d_offs.ptr), why="d_cap over d_offsets")
        refused(desc(d_kinds=call.ptr("input0") + 32 * n - 1), why="d_kinds over the last byte of d_out")
        refused(desc(d_rows_needed=call.ptr("cap") + 8), why="d_rows_needed inside d_cap")
        refused(desc(d_input1=call.ptr("input0")), why="d_input1 is d_out")
        refused(desc(), op=35, d_b=some.ctypes.data_as(ctypes.c_void_p), why="op 35")
        assert zk.lib().zk_field_vec_op(ctx.h, 0, 36, ctypes.byref(desc()), None, ctypes.c_void_p(call.ptr("input0")), ctypes.c_size_t(0)) == OK
        ctx.sync()
        assert (call.arena.download(call.size, np.uint8) == SENT).all()
        call.check()
    finally:
        call.free()

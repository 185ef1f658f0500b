"""GPU: zk_fr_from_uint (packed little-endian unsigned cells of 1, 2, 4, 8 or 16 bytes -> Montgomery Fr on the device) against
the oracle's to_mont, bit for bit: every width at sizes around a wave, below and above a workgroup's share, with the extreme
cell values; a source that starts one cell into its allocation; a multi-workgroup launch with a ragged end; refused arguments
leave the output alone; the profiler books the stated bytes."""
import functools

import numpy as np
import pytest

from oracle import bn254 as b
from oracle import cref

pytestmark = pytest.mark.gpu
WIDTHS = (1, 2, 4, 8, 16)
SIZES = (1, 63, 64, 65, 255, 4099)       # 4099: prime, more than one workgroup (1024 cells), a tail for every per-lane packing
PATTERN = 0xA5C3A5C3A5C3A5C3


@functools.lru_cache(maxsize=None)
def cells(width: int, n: int):
    """n cells of `width` bytes: all ones, 0, 1, all ones minus 1, then a splitmix64 stream -- and their Montgomery images (oracle)"""
    top = (1 << (8 * width)) - 1
    vals, state = [top, 0, 1, top - 1][:n], 0x1234 + width
    while len(vals) < n:
        state, lo = b.splitmix64(state)
        state, hi = b.splitmix64(state)
        vals.append((lo | hi << 64) & top)
    want = cref.to_mont(vals)
    want.setflags(write=False)
    return tuple(vals), want


def pack(vals, width: int) -> np.ndarray:
    if width == 16:
        return np.array([[v & (2 ** 64 - 1), v >> 64] for v in vals], dtype=np.uint64).reshape(-1, 2)
    return np.array(vals, dtype={1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[width])


def expand(ctx, packed: np.ndarray, width: int, n: int, offset_cells: int = 0) -> np.ndarray:
    src, out = ctx.to_device(packed), ctx.alloc(max(n, 1) * 32)
    try:
        ctx.fr_from_uint(src, width, n, out, offset_bytes=offset_cells * width)
        return out.download((n, 4))
    finally:
        src.free()
        out.free()


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("width", WIDTHS)
def test_every_width_and_size_equals_the_oracle(ctx, width, n):
    vals, want = cells(width, n)
    assert np.array_equal(expand(ctx, pack(vals, width), width, n), want)
    assert cref.from_mont(want[:1])[0] == vals[0] and b.to_mont(vals[-1], b.R_MOD) == cref.limbs_to_ints(want[-1:])[0]      # the two oracles agree on what is asked


@pytest.mark.parametrize("width", WIDTHS)
def test_source_one_cell_into_its_allocation(ctx, width):
    """aligned to the cell width only: the packed loads of the narrow widths start in the middle of a word"""
    vals, want = cells(width, 4099)
    assert np.array_equal(expand(ctx, pack(vals, width), width, 4098, offset_cells=1), want[1:])


def test_many_workgroups_with_a_ragged_end(ctx):
    n = (1 << 16) + 1
    table = cref.to_mont(list(range(256)))
    state, vals = 7, np.empty(n, dtype=np.uint8)
    for i in range(0, n, 8):
        state, z = b.splitmix64(state)
        chunk = np.frombuffer(z.to_bytes(8, "little"), dtype=np.uint8)
        vals[i:i + 8] = chunk[:min(8, n - i)]
    vals[-1] = 255
    assert np.array_equal(expand(ctx, vals, 1, n), table[vals])


@pytest.mark.parametrize("width,offset_bytes", [(0, 0), (3, 0), (32, 0), (2, 1), (4, 2), (8, 4), (16, 8)])
def test_refused_arguments_leave_the_output_alone(zk, ctx, width, offset_bytes):
    n = 64
    src = ctx.to_device(np.arange(n * 34, dtype=np.uint8))
    out = ctx.to_device(np.full((n, 4), PATTERN, dtype=np.uint64))
    try:
        with pytest.raises(zk.ZkError, match="status -1"):
            ctx.fr_from_uint(src, width, n, out, offset_bytes=offset_bytes)
        assert (out.download((n, 4)) == PATTERN).all()
    finally:
        src.free()
        out.free()


def test_profiler_books_the_algorithmic_bytes(ctx):
    launches = [(1, 4099), (2, 255), (16, 65), (8, 1)]
    ctx.prof_enable(True)
    try:
        ctx.prof_reset()
        for width, n in launches:
            vals, want = cells(width, n)
            assert np.array_equal(expand(ctx, pack(vals, width), width, n), want)
        assert ctx.prof_get("fr_from_uint")[1] == len(launches)
        assert ctx.prof_get_bytes("fr_from_uint") == sum(n * (w + 32) for w, n in launches)
    finally:
        ctx.prof_enable(False)
        ctx.prof_reset()

"""GPU: ZK_OP_KEY_SORT of zk_field_vec_op -- the stable sort of 64-byte key records as a permutation, and the records in sorted
order -- byte for byte against the model of tests/key_order_cases.py (sorted(range(n), key=(masked record, i))).  Sizes around a
wave, a workgroup and a tile of the passes; random records; realistic RW rows under the full mask and without the counter bytes;
equal records; a difference at each single byte position; 4 distinct records over 2^16 rows; sorted and reversed input; masks of
zeros and of one byte; records at an address that is 8 mod 16; two calls giving identical bytes; every refusal with canaries around
the outputs; ops 19 and 21 still refused."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import key_order_cases as kc  # noqa: E402

pytestmark = pytest.mark.gpu
TILE = 2048                                  # KS_TILE of csrc/keyorder.hip.hpp: the places one workgroup of a pass takes
GUARD = 6                                    # sentinel entries in front of and behind every output (d_out stays 8-byte aligned)
SENT32, SENT8 = 0xA5C3A5C3, 0xC3
INVALID_ARG = -1
assert TILE == kc.TILE


class Sort:
    """one input on the device (optionally at an address that is 8 mod 16) and guarded outputs"""

    def __init__(self, ctx, keys, odd_half=False):
        self.ctx, self.keys, self.n = ctx, list(keys), len(keys)
        self.image = np.frombuffer(b"".join(self.keys), dtype=np.uint8) if self.n else np.zeros(0, dtype=np.uint8)
        self.src = ctx.alloc(64 * self.n + 32)
        self.at = self.src.ptr + (8 - self.src.ptr % 16) % 16 if odd_half else self.src.ptr
        if self.n:
            zk_upload(ctx, self.at, self.image)
        self.perm = ctx.to_device(np.full(self.n + 2 * GUARD, SENT32, dtype=np.uint32))
        self.sorted = ctx.to_device(np.full((self.n + 2 * GUARD) * 64, SENT8, dtype=np.uint8))

    def perm_ptr(self):
        return self.perm.ptr + 4 * GUARD

    def sorted_ptr(self):
        return self.sorted.ptr + 64 * GUARD

    def run(self, mask=None, with_sorted=True):
        self.ctx.key_sort(self.at, self.n, self.perm_ptr(), mask=mask, sorted_keys=self.sorted_ptr() if with_sorted else None)
        return self.results(with_sorted)

    def results(self, with_sorted=True):
        perm = self.perm.download(self.n + 2 * GUARD, np.uint32)
        assert (perm[:GUARD] == SENT32).all() and (perm[GUARD + self.n:] == SENT32).all(), "d_out: an entry outside [0, n) was written"
        rec = self.sorted.download((self.n + 2 * GUARD) * 64, np.uint8)
        assert (rec[:64 * GUARD] == SENT8).all() and (rec[64 * (GUARD + self.n):] == SENT8).all(), "d_sorted: a record outside [0, n) was written"
        body = rec[64 * GUARD:64 * (GUARD + self.n)]
        if not with_sorted:
            assert (body == SENT8).all(), "d_sorted was not given"
        return perm[GUARD:GUARD + self.n].tolist(), body.tobytes()

    def check(self, mask=None, want=None):
        perm, rec = self.run(mask)
        want = kc.sort_perm(self.keys, mask) if want is None else want
        assert perm == want, ("first differing places", [i for i in range(self.n) if perm[i] != want[i]][:5])
        assert rec == b"".join(self.keys[i] for i in want)
        assert self.input_intact()
        return perm

    def input_intact(self):
        return not self.n or np.array_equal(zk_download(self.ctx, self.at, 64 * self.n), self.image)

    def untouched(self):
        return (self.perm.download(self.n + 2 * GUARD, np.uint32) == SENT32).all() and (self.sorted.download((self.n + 2 * GUARD) * 64, np.uint8) == SENT8).all() and self.input_intact()

    def free(self):
        for b in (self.src, self.perm, self.sorted):
            b.free()


def zk_upload(ctx, ptr, a):
    import zkevm_circuits_amd as z
    a = np.ascontiguousarray(a)
    ctx._ck(z.lib().zk_h2d(ctx.h, ctypes.c_void_p(ptr), a.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(a.nbytes)))


def zk_download(ctx, ptr, nbytes):
    import zkevm_circuits_amd as z
    out = np.empty(nbytes, dtype=np.uint8)
    ctx._ck(z.lib().zk_d2h(ctx.h, out.ctypes.data_as(ctypes.c_void_p), ctypes.c_void_p(ptr), ctypes.c_size_t(nbytes)))
    return out


def checked(ctx, keys, mask=None, want=None, **kw):
    s = Sort(ctx, keys, **kw)
    try:
        return s.check(mask, want)
    finally:
        s.free()


# ---- 1. sizes: a wave, a workgroup, a tile of the passes, several tiles
@pytest.mark.parametrize("n", [0, 1, 2, 63, 64, 65, 255, 256, 257, TILE - 1, TILE, TILE + 1, 3 * TILE + 5, (1 << 17) + 1])
def test_random_records(ctx, n):
    checked(ctx, kc.random_keys(kc.rng(n), n))


@pytest.fixture(scope="module")
def realistic():
    keys = kc.realistic_rows(kc.rng(0x5EA1), 3 * TILE + 77)
    return keys, kc.sort_perm(keys, kc.NO_COUNTER_MASK)


@pytest.mark.parametrize("mask", ["full", "no counter"])
def test_realistic_rows_sort_the_same_with_and_without_the_counter_bytes(ctx, realistic, mask):
    keys, want = realistic
    assert want == kc.sort_perm(keys, kc.FULL_MASK)                        # distinct counters
    checked(ctx, keys, None if mask == "full" else kc.NO_COUNTER_MASK, want)


def test_equal_records_give_the_identity(ctx):
    rec = kc.rng(1).randbytes(64)
    assert checked(ctx, [rec] * (2 * TILE + 3)) == list(range(2 * TILE + 3))


def test_a_difference_at_each_single_byte_position(ctx):
    rng = kc.rng(0xB17E)
    base = bytearray(rng.randbytes(64))
    for j in range(64):
        keys = []
        for _ in range(300):
            rec = bytearray(base)
            rec[j] = rng.randrange(256)
            keys.append(bytes(rec))
        want = sorted(range(300), key=lambda i: (keys[i][j], i))
        assert want == kc.sort_perm(keys)
        checked(ctx, keys, None, want)


def test_four_distinct_records_over_many_workgroups_stay_stable(ctx):
    rng = kc.rng(4)
    four = kc.random_keys(rng, 4)
    keys = [four[rng.randrange(4)] for _ in range(1 << 16)]
    perm = checked(ctx, keys)
    runs = [perm[i] < perm[i + 1] for i in range(len(perm) - 1) if keys[perm[i]] == keys[perm[i + 1]]]
    assert len(runs) == (1 << 16) - 4 and all(runs)


def test_sorted_and_reversed_input(ctx):
    keys = sorted(kc.random_keys(kc.rng(6), TILE + 100))
    assert checked(ctx, keys) == list(range(len(keys)))
    assert checked(ctx, keys[::-1]) == list(range(len(keys)))[::-1]


def test_masks(ctx):
    keys = kc.random_keys(kc.rng(7), TILE + 50)
    assert checked(ctx, keys, bytes(64)) == list(range(len(keys)))        # nothing compared: the identity
    one = bytes(33) + b"\x80" + bytes(30)                                 # any nonzero byte keeps its position
    perm = checked(ctx, keys, one)
    assert perm == sorted(range(len(keys)), key=lambda i: (keys[i][33], i))
    few = [rec[:1] + bytes(1) + rec[2:] for rec in keys[:500]]
    checked(ctx, few, bytes([1, 1]) + bytes(62))                          # two kept bytes, one of which no record differs in
    s = Sort(ctx, keys)
    try:
        s.ctx.key_sort(s.at, s.n, s.perm_ptr())                           # no d_sorted
        perm, _ = s.results(with_sorted=False)
        assert perm == kc.sort_perm(keys)
    finally:
        s.free()


def test_records_at_an_address_that_is_8_mod_16(ctx):
    keys = kc.random_keys(kc.rng(8), 1000)
    s = Sort(ctx, keys, odd_half=True)
    try:
        assert s.at % 16 == 8
        s.check()
    finally:
        s.free()


def test_two_calls_give_identical_bytes(ctx):
    rng = kc.rng(9)
    four = kc.random_keys(rng, 4)
    keys = [four[rng.randrange(4)] for _ in range(5 * TILE + 1)]
    s = Sort(ctx, keys)
    try:
        first = s.run()
        second = s.run()
        assert first == second and first[0] == kc.sort_perm(keys)
    finally:
        s.free()


# ---- 2. refusals
class _KeySortFlags(ctypes.Structure):
    _fields_ = [("d_keys", ctypes.c_void_p), ("d_sorted", ctypes.c_void_p), ("flags", ctypes.c_uint8)]


def raw_call(zk, ctx, s, field=0, op=20, keys="own", sorted_keys="own", flags=0, mask=None, out="own", n=None, desc=True, b=None):
    d = _KeySortFlags(s.at if keys == "own" else keys, s.sorted_ptr() if sorted_keys == "own" else sorted_keys, flags)
    m = None if mask is None else (ctypes.c_uint8 * 64)(*mask)
    second = b if b is not None else (ctypes.cast(m, ctypes.c_void_p) if m is not None else None)
    return zk.lib().zk_field_vec_op(ctx.h, field, op, ctypes.byref(d) if desc else None, second, ctypes.c_void_p(s.perm_ptr() if out == "own" else out),
                                    ctypes.c_size_t(s.n if n is None else n))


def test_refused_calls_write_nothing_and_leave_the_context_usable(zk, ctx):
    keys = kc.random_keys(kc.rng(10), 300)
    s = Sort(ctx, keys)
    want = kc.sort_perm(keys)
    refusals = []

    def refused(what, **kw):
        assert raw_call(zk, ctx, s, **kw) == INVALID_ARG, what
        ctx.sync()
        assert s.untouched(), what
        refusals.append(what)
    try:
        refused("Fq", field=zk.FIELD_FQ)
        for bits in (1, 2, 128, 255):
            refused(f"flags {bits}", flags=bits)
        refused("NULL descriptor", desc=False)
        refused("NULL d_keys", keys=None)
        refused("NULL d_out", out=None)
        refused("d_keys at an address that is 4 mod 8", keys=s.at + 4)
        refused("d_sorted at an address that is 4 mod 8", sorted_keys=s.sorted_ptr() + 4)
        refused("d_out at an address that is 2 mod 4", out=s.perm_ptr() + 2)
        refused("n = 2^32", n=1 << 32)
        refused("n = 2^64 - 1", n=(1 << 64) - 1)
        refused("d_sorted is d_keys", sorted_keys=s.at)
        refused("d_sorted one record into d_keys", sorted_keys=s.at + 64)
        refused("d_sorted ends inside d_keys", sorted_keys=s.at - 64 * s.n + 8)
        refused("d_out inside d_keys", out=s.at + 64)
        refused("d_out inside d_sorted", out=s.sorted_ptr() + 128)
        refused("d_sorted inside d_out", sorted_keys=s.perm_ptr() + 8 - 64 * s.n + 64)
        for op in (19, 21):
            refused(f"op {op}", op=op, b=ctypes.c_void_p(s.at))
            refused(f"op {op} with a NULL second operand", op=op)
            refused(f"op {op} over Fq", op=op, field=zk.FIELD_FQ, b=ctypes.c_void_p(s.at))
        refused("flags with n = 0", flags=1, n=0)
        refused("NULL d_keys with n = 0", keys=None, n=0)
        refused("a misaligned d_out with n = 0", out=s.perm_ptr() + 1, n=0)
        refused("Fq with n = 0", field=zk.FIELD_FQ, n=0)
        refused("d_sorted is d_keys with n = 0", sorted_keys=s.at, n=0)
        assert len(refusals) == 30
        assert raw_call(zk, ctx, s, n=0) == 0                               # n = 0: ZK_OK, nothing written
        assert raw_call(zk, ctx, s, n=0, sorted_keys=None) == 0
        ctx.sync()
        assert s.untouched()
        assert s.check(None, want) == want                                  # the context still works
    finally:
        s.free()


def test_the_call_books_its_launches_and_bytes(ctx):
    keys = kc.random_keys(kc.rng(11), 777)
    s = Sort(ctx, keys)
    try:
        ctx.sync()
        ctx.prof_reset()
        ctx.prof_enable(True)
        try:
            s.check(kc.NO_COUNTER_MASK)
            ms, launches = ctx.prof_get("key_sort")
            assert ms > 0 and launches == 1
            assert ctx.prof_get_bytes("key_sort") == 777 * (76 + 14 * 60 + 128)
        finally:
            ctx.prof_enable(False)
            ctx.prof_reset()
    finally:
        s.free()

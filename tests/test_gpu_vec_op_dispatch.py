"""GPU: which calls of zk_field_vec_op are refused before anything runs, stated as a table.

The expectations below were read off the chain of `if`s that zk_field_vec_op was before it looked its descriptor ops up in a table; they
are data of this file and are not derived from that table.  In the order in which the function applies them:

  * d_a and d_out are never NULL; d_b is required, optional (the key sort's mask) or must be NULL (the key order);
  * a descriptor op looks at the field before it looks at n, and then hands over to its own checks -- a valid descriptor is accepted
    for n = 0 and for n = 4;
  * every other op returns ZK_OK for n = 0 once its three pointers are there, WHATEVER the op and the field are (that is how the
    function has always been; an op value without a #define is refused only when there is something to do);
  * the affine scans are defined over Fr only, the plain ops over Fr and Fq, any other op value or field is refused.

Every refused call must leave a sentinel-filled output as it was and the context usable: a valid ZK_OP_ADD follows each of them.
Buffers of four elements; one context, a few hundred calls, well under a second.
"""
import ctypes
import itertools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from oracle import bn254  # noqa: E402

pytestmark = pytest.mark.gpu

N = 4
OK, INVALID_ARG = 0, -1
FR, FQ, NO_FIELD = 0, 1, 7
MOD = {FR: bn254.R_MOD, FQ: bn254.P_MOD}
SENT = 0xA5

# op value -> (d_b rule, Fr only, the field is looked at before n: the op takes a descriptor)
REQUIRED, OPTIONAL, MUST_BE_NULL = "required", "optional", "must be NULL"
DEFINED = {
    0: (REQUIRED, False, False),        # ZK_OP_ADD
    1: (REQUIRED, False, False),        # ZK_OP_SUB
    2: (REQUIRED, False, False),        # ZK_OP_MUL
    3: (REQUIRED, True, False),         # ZK_OP_SCAN_AFFINE
    4: (REQUIRED, True, False),         # ZK_OP_SCAN_AFFINE_REV
    8: (REQUIRED, True, True),          # ZK_OP_ROW_RLC
    9: (REQUIRED, True, True),          # ZK_OP_SCAN_RLC
    10: (REQUIRED, True, True),         # ZK_OP_SCAN_RLC_REV
    12: (REQUIRED, True, True),         # ZK_OP_ROW_INV0
    14: (REQUIRED, True, True),         # ZK_OP_POSEIDON
    16: (REQUIRED, True, True),         # ZK_OP_KECCAK
    18: (REQUIRED, True, True),         # ZK_OP_SHA256
    20: (OPTIONAL, True, True),         # ZK_OP_KEY_SORT
    22: (MUST_BE_NULL, True, True),     # ZK_OP_KEY_ORDER
}
OPS = range(25)                         # 5, 6, 7 and the odd values from 11 on have no #define


def expected(op, field, n, null):
    """null: which of "a", "b", "out" is NULL, or None"""
    b_rule, fr_only, descriptor = DEFINED.get(op, (REQUIRED, False, False))
    if null in ("a", "out"):
        return INVALID_ARG
    if b_rule == REQUIRED and null == "b":
        return INVALID_ARG
    if b_rule == MUST_BE_NULL and null != "b":
        return INVALID_ARG
    if descriptor:
        return OK if field == FR else INVALID_ARG
    if n == 0:
        return OK
    if fr_only and field != FR:
        return INVALID_ARG
    return OK if op in DEFINED and field in (FR, FQ) else INVALID_ARG


def mont(vals, field):
    return np.array([[(v << 256) % MOD[field] >> (64 * j) & (2**64 - 1) for j in range(4)] for v in vals], dtype=np.uint64)


def unmont(a, field):
    inv = pow(1 << 256, -1, MOD[field])
    return [sum(int(w) << (64 * j) for j, w in enumerate(row)) * inv % MOD[field] for row in a]


class Operands:
    """everything a valid call of any op needs, on four rows; the descriptors are kept alive here"""

    def __init__(self, zk, ctx):
        b = zk.binding
        rng = np.random.default_rng(0xD15)
        self.vals = {f: [[int.from_bytes(rng.bytes(32), "little") % MOD[f] for _ in range(N)] for _ in range(2)] for f in (FR, FQ)}
        self.vals[NO_FIELD] = self.vals[FR]
        self.elems = {f: [ctx.to_device(mont(v, f if f in MOD else FR)) for v in self.vals[f]] for f in (FR, FQ, NO_FIELD)}
        self.out = ctx.alloc(32 * N + 64)                                  # the sentinel-filled output of the call under test
        self.add_out = ctx.alloc(32 * N)                                   # the output of the ZK_OP_ADD that follows a refusal
        self.cells = ctx.to_device(rng.integers(0, 2**63, 2 * N, dtype=np.uint64))        # two columns of 8-byte cells
        self.keys = ctx.to_device(rng.integers(0, 256, 64 * N, dtype=np.uint8))
        self.bytes = ctx.to_device(rng.integers(0, 256, 64, dtype=np.uint8))
        self.offsets = ctx.to_device(np.array([0, 3, 17, 40], dtype=np.uint32))
        self.lens = ctx.to_device(np.array([0, 5, 23, 24], dtype=np.uint32))
        self.host = np.zeros((9, 4), dtype=np.uint64)                      # constants, weights, challenges: zeros are valid for every op
        self.mask = np.ones(64, dtype=np.uint8)
        self.col_ptrs = (ctypes.c_void_p * 1)(self.cells.ptr)
        self.col_widths = (ctypes.c_uint8 * 1)(8)
        cols, widths = ctypes.cast(self.col_ptrs, ctypes.POINTER(ctypes.c_void_p)), ctypes.cast(self.col_widths, ctypes.POINTER(ctypes.c_uint8))
        hash_fields = (self.bytes.ptr, 64, self.offsets.ptr, self.lens.ptr, None, None, 4, 0)
        self.desc = {
            8: b._RowRlc(1, cols, widths),
            9: b._ScanRlc(self.cells.ptr, 8, None),
            10: b._ScanRlc(self.cells.ptr, 8, None),
            12: b._RowInv0(1, cols, widths, None, 0),
            14: b._Poseidon(self.cells.ptr, self.cells.ptr + 8 * N, None, None, None, None, 8, 8, 0, 0),
            16: b._Keccak(*hash_fields),
            18: b._Sha256(*hash_fields),
            20: b._KeySort(self.keys.ptr, None, 0),
            22: b._KeyOrder(self.keys.ptr, None, None, None, None, None, 30, 0, None, None, 0),
        }
        self.fill()

    def fill(self):
        self.out.upload(np.full(32 * N + 64, SENT, dtype=np.uint8))

    def untouched(self):
        return bool((self.out.download(32 * N + 64, np.uint8) == SENT).all())

    def args(self, op, field, null):
        """d_a, d_b, d_out of a call that is valid but for `null`"""
        if op in self.desc:
            a = ctypes.cast(ctypes.byref(self.desc[op]), ctypes.c_void_p)
            b = self.mask.ctypes.data_as(ctypes.c_void_p) if op in (20, 22) else self.host.ctypes.data_as(ctypes.c_void_p)
        else:
            a, b = (ctypes.c_void_p(e.ptr) for e in self.elems[field])
        return (None if null == "a" else a), (None if null == "b" else b), (None if null == "out" else ctypes.c_void_p(self.out.ptr + 32))


@pytest.fixture(scope="module")
def operands(zk, ctx):
    return Operands(zk, ctx)


def valid_add(zk, ctx, t):
    a, b = (ctypes.c_void_p(e.ptr) for e in t.elems[FR])
    return zk.lib().zk_field_vec_op(ctx.h, FR, 0, a, b, ctypes.c_void_p(t.add_out.ptr), ctypes.c_size_t(N))


def test_every_op_field_n_and_null_operand_is_refused_or_accepted_as_the_table_says(zk, ctx, operands):
    t = operands
    wrong, refused, accepted = [], 0, 0
    for op, field, n, null in itertools.product(OPS, (FR, FQ, NO_FIELD), (0, N), (None, "a", "b", "out")):
        a, b, out = t.args(op, field, null)
        rc = zk.lib().zk_field_vec_op(ctx.h, field, op, a, b, out, ctypes.c_size_t(n))
        want = expected(op, field, n, null)
        ctx.sync()
        if rc != want:
            wrong.append((op, field, n, null, rc, want))
        if rc == OK:
            accepted += 1
            if n:
                t.fill()
            continue
        refused += 1
        if not t.untouched():
            wrong.append((op, field, n, null, "a refused call wrote to d_out"))
            t.fill()
        if valid_add(zk, ctx, t) != OK:
            wrong.append((op, field, n, null, "ZK_OP_ADD failed after the refusal"))
    ctx.sync()
    assert not wrong, wrong[:20]
    # accepted: 8 descriptor ops that take a d_b over Fr, n = 0 and 4 (16), the key ops with a NULL d_b (4), the 16 other op values
    # with n = 0 whatever the field (48), the plain ops over both fields and the scans over Fr with n = 4 (8)
    assert (refused, accepted) == (25 * 3 * 2 * 4 - 76, 76)
    want = mont([(x + y) % MOD[FR] for x, y in zip(*t.vals[FR])], FR)
    assert (t.add_out.download((N, 4)) == want).all()                      # the last of the additions that followed the refusals


def test_the_key_sort_takes_no_mask_and_the_key_order_takes_no_second_operand(zk, ctx, operands):
    t = operands
    a, _, out = t.args(20, FR, "b")
    assert zk.lib().zk_field_vec_op(ctx.h, FR, 20, a, None, out, ctypes.c_size_t(N)) == OK
    ctx.sync()
    keys = t.keys.download((N, 64), np.uint8)
    order = sorted(range(N), key=lambda i: (bytes(keys[i]), i))
    got = t.out.download(32 * N + 64, np.uint8)
    assert got[32:32 + 4 * N].view(np.uint32).tolist() == order and (got[:32] == SENT).all() and (got[32 + 4 * N:] == SENT).all()
    t.fill()
    a, b, out = t.args(22, FR, None)
    assert zk.lib().zk_field_vec_op(ctx.h, FR, 22, a, b, out, ctypes.c_size_t(N)) == INVALID_ARG
    assert "no second operand" in zk.lib().zk_last_error(ctx.h).decode()
    ctx.sync()
    assert t.untouched()
    assert zk.lib().zk_field_vec_op(ctx.h, FR, 22, a, None, out, ctypes.c_size_t(N)) == OK
    ctx.sync()
    t.fill()


@pytest.mark.parametrize("field", [FR, FQ])
def test_the_plain_ops_match_the_host(zk, ctx, operands, field):
    t = operands
    x, y = t.vals[field]
    p = MOD[field]
    for op, f in ((0, lambda u, v: (u + v) % p), (1, lambda u, v: (u - v) % p), (2, lambda u, v: u * v % p)):
        a, b, out = t.args(op, field, None)
        assert zk.lib().zk_field_vec_op(ctx.h, field, op, a, b, out, ctypes.c_size_t(N)) == OK
        ctx.sync()
        got = t.out.download(32 * N + 64, np.uint8)
        assert unmont(got[32:32 + 32 * N].view(np.uint64).reshape(N, 4), field) == [f(u, v) for u, v in zip(x, y)], op
        assert (got[:32] == SENT).all() and (got[32 + 32 * N:] == SENT).all()
        t.fill()

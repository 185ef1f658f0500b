"""GPU: ZK_OP_KEY_ORDER of zk_field_vec_op -- first_different_limb, its five bit planes, limb_difference, its inverse,
not_first_access and the gathered typed columns of adjacent key records -- bit for bit against the model of
tests/key_order_cases.py, converted by the oracle (cref.to_mont).  With and without d_perm and with every subset of the optional
outputs; a difference in each limb, equal and out-of-order neighbours, row 0, a d_perm entry >= n; group_limbs 0, 30 and 32; the
state circuit's gather map; n across the wave and workgroup edges and 2^16 + 3; sort and order chained on the device; every refusal
with canaries around the outputs."""
import ctypes
import itertools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import key_order_cases as kc  # noqa: E402
from oracle import cref  # noqa: E402

pytestmark = pytest.mark.gpu
P = kc.P
GUARD = 4                                    # sentinel rows in front of and behind every output
SENT64, SENT8 = 0xA5C3A5C3A5C3A5C3, 0xC3
INVALID_ARG = -1
OPTIONAL = ("diff", "index", "bits", "not_first")
DTYPE = {1: np.uint8, 2: np.uint16, 4: np.uint32}


def mont(vals):
    return cref.to_mont(list(vals)) if len(vals) else np.zeros((0, 4), dtype=np.uint64)


class Order:
    """one call: records (and optionally a permutation) on the device, every output inside GUARD sentinel rows"""

    def __init__(self, ctx, keys, perm=None, outputs=OPTIONAL, group_limbs=30, cols=()):
        self.ctx, self.keys, self.perm, self.group_limbs, self.cols = ctx, list(keys), None if perm is None else list(perm), group_limbs, list(cols)
        self.n = len(self.keys) if perm is None else len(self.perm)
        n = self.n
        self.image = np.frombuffer(b"".join(self.keys), dtype=np.uint8) if self.keys else np.zeros(0, dtype=np.uint8)
        self.src = ctx.to_device(self.image)
        self.d_perm = ctx.to_device(np.array(self.perm, dtype=np.uint32)) if self.perm is not None else None
        self.fr = {name: ctx.to_device(np.full((n + 2 * GUARD, 4), SENT64, dtype=np.uint64)) for name in ("inv", "diff") if name == "inv" or name in outputs}
        self.by = {name: ctx.to_device(np.full((n + 2 * GUARD) * 16, SENT8, dtype=np.uint8)) for name in ("index", "not_first") if name in outputs}
        self.bits = ctx.to_device(np.full(5 * n + 2 * GUARD * 16, SENT8, dtype=np.uint8)) if "bits" in outputs else None
        self.cells = [ctx.to_device(np.full((n + 2 * GUARD) * 16, SENT8, dtype=np.uint8)) for _ in self.cols]

    def ptr(self, name):
        if name in self.fr:
            return self.fr[name].ptr + 32 * GUARD
        if name in self.by:
            return self.by[name].ptr + 16 * GUARD
        if name == "bits" and self.bits is not None:
            return self.bits.ptr + 16 * GUARD
        return None

    def cell_ptr(self, c):
        return self.cells[c].ptr + 16 * GUARD

    def args(self):
        return dict(keys=self.src.ptr, n=self.n, inv_out=self.ptr("inv"), perm=None if self.d_perm is None else self.d_perm.ptr, diff=self.ptr("diff"), index=self.ptr("index"),
                    bits=self.ptr("bits"), not_first=self.ptr("not_first"), group_limbs=self.group_limbs,
                    cols=[(off, width, self.cell_ptr(c)) for c, (off, width) in enumerate(self.cols)])

    def got(self):
        """every output's n rows, after checking that nothing around them was written"""
        n, out = self.n, {}
        for name, buf in self.fr.items():
            a = buf.download((n + 2 * GUARD, 4))
            assert (a[:GUARD] == SENT64).all() and (a[GUARD + n:] == SENT64).all(), f"{name}: a row outside [0, n) was written"
            out[name] = a[GUARD:GUARD + n]
        for name, buf in self.by.items():
            a = buf.download((n + 2 * GUARD) * 16, np.uint8)
            assert (a[:16 * GUARD] == SENT8).all() and (a[16 * GUARD + n:] == SENT8).all(), f"{name}: a byte outside [0, n) was written"
            out[name] = a[16 * GUARD:16 * GUARD + n]
        if self.bits is not None:
            a = self.bits.download(5 * n + 2 * GUARD * 16, np.uint8)
            assert (a[:16 * GUARD] == SENT8).all() and (a[16 * GUARD + 5 * n:] == SENT8).all(), "bits: a byte outside the five planes was written"
            out["bits"] = a[16 * GUARD:16 * GUARD + 5 * n].reshape(5, n)
        for c, (off, width) in enumerate(self.cols):
            a = self.cells[c].download((n + 2 * GUARD) * 16, np.uint8)
            assert (a[:16 * GUARD] == SENT8).all() and (a[16 * GUARD + width * n:] == SENT8).all(), f"column {c}: a byte outside its n cells was written"
            out[("col", c)] = a[16 * GUARD:16 * GUARD + width * n].view(DTYPE[width])
        return out

    def want(self):
        m = kc.order_columns(self.keys, self.perm, self.group_limbs)
        w = {"inv": mont(m["inv"]), "diff": mont(m["diff"]), "index": np.array(m["index"], dtype=np.uint8), "not_first": np.array(m["not_first"], dtype=np.uint8),
             "bits": np.array(m["bits"], dtype=np.uint8).reshape(5, self.n)}
        for c, col in enumerate(kc.gather(self.keys, self.cols, self.perm)):
            w[("col", c)] = np.array(col, dtype=DTYPE[self.cols[c][1]])
        return w

    def check(self, want=None):
        self.ctx.key_order(**self.args())
        got, want = self.got(), self.want() if want is None else want
        for name, a in got.items():
            assert np.array_equal(a, want[name]), (name, "first differing rows", np.argwhere(np.asarray(a != want[name]).reshape(len(a), -1).any(axis=1))[:5].ravel().tolist() if name != "bits" else "")
        for name in self.fr:                                             # canonical
            assert all(sum(int(x) << (64 * j) for j, x in enumerate(row)) < P for row in got[name][:300]), name
        assert self.inputs_intact()
        return got

    def inputs_intact(self):
        return (not self.keys or np.array_equal(self.src.download(self.image.shape, np.uint8), self.image)) and (self.d_perm is None or not self.n or self.d_perm.download(self.n, np.uint32).tolist() == self.perm)

    def buffers(self):
        return [self.src, *self.fr.values(), *self.by.values(), *self.cells] + [b for b in (self.d_perm, self.bits) if b is not None]

    def untouched(self):
        return (all((b.download((self.n + 2 * GUARD, 4)) == SENT64).all() for b in self.fr.values())
                and all((b.download(b.nbytes, np.uint8) == SENT8).all() for b in [*self.by.values(), *self.cells] + ([self.bits] if self.bits is not None else []))
                and self.inputs_intact())

    def free(self):
        for b in self.buffers():
            b.free()


def checked(ctx, keys, **kw):
    t = Order(ctx, keys, **kw)
    try:
        return t.check()
    finally:
        t.free()


@pytest.fixture(scope="module")
def main_case():
    """333 rows: runs of equal records, out-of-order neighbours, differences at every limb"""
    rng = kc.rng(0x0DE2)
    keys = kc.realistic_rows(rng, 200)
    base = rng.randbytes(64)
    for j in range(32):
        rec = bytearray(base)
        rec[2 * j + rng.randrange(2)] ^= 1 + rng.randrange(255)
        keys += [bytes(rec), base]
    keys += [base] * 5 + kc.random_keys(rng, 333 - len(keys) - 5)
    perm = list(range(333))
    rng.shuffle(perm)
    return keys, perm


@pytest.mark.parametrize("with_perm", [False, True])
@pytest.mark.parametrize("outputs", [c for k in range(5) for c in itertools.combinations(OPTIONAL, k)], ids=lambda c: "+".join(c) or "none")
def test_every_subset_of_the_optional_outputs(ctx, main_case, with_perm, outputs):
    keys, perm = main_case
    got = checked(ctx, keys, perm=perm if with_perm else None, outputs=outputs)
    if not with_perm and "index" in outputs:
        assert set(got["index"][1:].tolist()) == set(range(32))           # a difference in each limb, and equal neighbours (31)
    if "diff" in outputs:
        assert not got["diff"][0].any() and not got["inv"][0].any()       # row 0


def test_equal_and_out_of_order_neighbours(ctx):
    a, b = kc.pack(4, 7, 99, 2, 5, 12), kc.pack(4, 7, 99, 2, 5, 7)
    got = checked(ctx, [a, a, b, a, b, b])
    assert got["index"].tolist() == [0, 31, 31, 31, 31, 31] and got["not_first"].tolist() == [0, 1, 1, 1, 1, 1]
    five = mont([0, 0, P - 5, 5, P - 5, 0])                              # equal: 0; 7 after 12: r - 5
    assert np.array_equal(got["diff"], five)
    assert np.array_equal(got["inv"], mont([0, 0, P - pow(5, -1, P), pow(5, -1, P), P - pow(5, -1, P), 0]))


@pytest.mark.parametrize("group_limbs", [0, 30, 32])
def test_group_limbs(ctx, main_case, group_limbs):
    keys, _ = main_case
    got = checked(ctx, keys, group_limbs=group_limbs)
    nf = got["not_first"]
    assert nf[0] == 0 and (nf[1:].all() if group_limbs == 0 else not nf.any() if group_limbs == 32 else 0 < nf.sum() < len(nf) - 1)


def test_a_perm_entry_out_of_range_zeroes_its_row_and_the_next(ctx):
    keys = kc.random_keys(kc.rng(21), 100)
    perm = list(range(100))
    kc.rng(22).shuffle(perm)
    for at, bad in ((40, 100), (0, 0xFFFFFFFF), (99, 1 << 31), (64, 100)):
        perm[at] = bad
    cols = [(0, 4), (61, 1), (30, 2)]
    got = checked(ctx, keys, perm=perm, cols=cols)
    for at in (40, 41, 0, 1, 99, 64, 65):
        assert not got["inv"][at].any() and not got["diff"][at].any() and got["index"][at] == 0 and got["not_first"][at] == 0 and not got["bits"][:, at].any()
    for at in (40, 0, 99, 64):
        assert all(got[("col", c)][at] == 0 for c in range(3))
    assert got[("col", 0)][41] == int.from_bytes(keys[perm[41]][:4], "big")   # the row behind it still has a record of its own
    assert got["inv"][42].any()


def test_the_state_circuit_gather_map(ctx):
    rng = kc.rng(23)
    keys = kc.realistic_rows(rng, 700)
    perm = kc.sort_perm(keys)
    cols = kc.state_circuit_cols()
    got = checked(ctx, keys, perm=perm, cols=[(off, width) for _, off, width in cols])
    by_name = {name: got[("col", c)] for c, (name, _, _) in enumerate(cols)}
    assert len(cols) == 50 and by_name["rw_counter"].dtype == np.uint32 and by_name["tag"].dtype == np.uint8 and by_name["address_limb0"].dtype == np.uint16
    assert sorted(by_name["rw_counter"].tolist()) == list(range(1, 701))
    assert (by_name["rw_counter"] == (by_name["rw_counter_limb1"].astype(np.uint32) << 16 | by_name["rw_counter_limb0"])).all()
    assert (np.diff(by_name["tag"].astype(int)) >= 0).all()               # sorted rows
    assert got["diff"].any() and all(int(x) < 65536 for x in cref.from_mont(got["diff"])[:50])   # in order: small positive differences


@pytest.mark.parametrize("n", [0, 1, 2, 63, 64, 65, 255, 256, 257, (1 << 16) + 3])
def test_sizes(ctx, n):
    rng = kc.rng(n + 1)
    four = kc.random_keys(rng, 4)
    keys = [rng.choice(four) if rng.random() < 0.3 else rng.randbytes(64) for _ in range(n)]
    checked(ctx, keys, cols=[(1, 1), (60, 4)])


def test_sort_and_order_chained_on_the_device(ctx):
    rng = kc.rng(24)
    keys = kc.realistic_rows(rng, 5000)
    rng.shuffle(keys)
    t = Order(ctx, keys, perm=list(range(5000)), cols=[(60, 4), (1, 1)])
    try:
        ctx.key_sort(t.src.ptr, t.n, t.d_perm.ptr, mask=kc.NO_COUNTER_MASK)   # the permutation never leaves the device
        t.perm = kc.sort_perm(keys, kc.NO_COUNTER_MASK)
        got = t.check()
        assert got["not_first"].sum() > 0 and got[("col", 0)].tolist() == [int.from_bytes(keys[i][60:], "big") for i in t.perm]
    finally:
        t.free()


# ---- refusals
class _Col(ctypes.Structure):
    _fields_ = [("offset", ctypes.c_uint8), ("width", ctypes.c_uint8)]


class _Desc(ctypes.Structure):
    _fields_ = [("d_keys", ctypes.c_void_p), ("d_perm", ctypes.c_void_p), ("d_diff", ctypes.c_void_p), ("d_index", ctypes.c_void_p), ("d_bits", ctypes.c_void_p),
                ("d_not_first", ctypes.c_void_p), ("group_limbs", ctypes.c_uint32), ("count", ctypes.c_uint32), ("cols", ctypes.POINTER(_Col)),
                ("d_cols", ctypes.POINTER(ctypes.c_void_p)), ("flags", ctypes.c_uint8)]


def raw_call(zk, ctx, t, field=0, op=22, flags=0, n=None, b=None, desc=True, count=None, null_cols=False, null_d_cols=False, col_specs=None, col_ptrs=None, out="own", **over):
    a = t.args()
    specs = [(off, width) for off, width, _ in a["cols"]] if col_specs is None else col_specs
    ptrs = [p for _, _, p in a["cols"]] if col_ptrs is None else col_ptrs
    table = (_Col * max(1, len(specs)))(*[_Col(off, width) for off, width in specs])
    dptrs = (ctypes.c_void_p * max(1, len(ptrs)))(*ptrs)
    f = dict(keys=a["keys"], perm=a["perm"], diff=a["diff"], index=a["index"], bits=a["bits"], not_first=a["not_first"], group_limbs=a["group_limbs"])
    f.update(over)
    d = _Desc(f["keys"], f["perm"], f["diff"], f["index"], f["bits"], f["not_first"], f["group_limbs"], len(specs) if count is None else count,
              None if null_cols else table, None if null_d_cols else dptrs, flags)
    return zk.lib().zk_field_vec_op(ctx.h, field, op, ctypes.byref(d) if desc else None, b, ctypes.c_void_p(a["inv_out"] if out == "own" else out), ctypes.c_size_t(t.n if n is None else n))


def test_refused_calls_write_nothing_and_leave_the_context_usable(zk, ctx):
    keys = kc.random_keys(kc.rng(25), 200)
    perm = list(range(200))
    kc.rng(26).shuffle(perm)
    t = Order(ctx, keys, perm=perm, cols=[(0, 4), (10, 2), (63, 1)])
    a = t.args()
    n, inv, diff, index, bits, nf = t.n, a["inv_out"], a["diff"], a["index"], a["bits"], a["not_first"]
    c0, c1, c2 = (p for _, _, p in a["cols"])
    refusals = []

    def refused(what, **kw):
        assert raw_call(zk, ctx, t, **kw) == INVALID_ARG, what
        ctx.sync()
        assert t.untouched(), what
        refusals.append(what)
    try:
        refused("Fq", field=zk.FIELD_FQ)
        for f in (1, 2, 128, 255):
            refused(f"flags {f}", flags=f)
        refused("NULL descriptor", desc=False)
        refused("NULL d_keys", keys=None)
        refused("NULL d_out", out=None)
        refused("a second operand", b=ctypes.c_void_p(a["keys"]))
        refused("d_keys at an address that is 4 mod 8", keys=a["keys"] + 4)
        refused("d_perm at an address that is 2 mod 4", perm=a["perm"] + 2)
        refused("d_out at an address that is 8 mod 16", out=inv + 8)
        refused("d_diff at an address that is 8 mod 16", diff=diff + 8)
        refused("a 4-byte column at an address that is 2 mod 4", col_ptrs=[c0 + 2, c1, c2])
        refused("a 2-byte column at an odd address", col_ptrs=[c0, c1 + 1, c2])
        refused("n = 2^32", n=1 << 32)
        refused("n = 2^64 - 1", n=(1 << 64) - 1)
        for width in (0, 3, 5, 8, 255):
            refused(f"width {width}", col_specs=[(0, 4), (10, width), (63, 1)])
        refused("offset 61 with width 4", col_specs=[(61, 4), (10, 2), (63, 1)])
        refused("offset 63 with width 2", col_specs=[(0, 4), (63, 2), (63, 1)])
        refused("offset 64", col_specs=[(0, 4), (10, 2), (64, 1)])
        refused("count 65", count=65)
        refused("NULL cols", null_cols=True)
        refused("NULL d_cols", null_d_cols=True)
        refused("a NULL entry in d_cols", col_ptrs=[c0, None, c2])
        refused("group_limbs 33", group_limbs=33)
        refused("d_diff AT d_out", diff=inv)
        refused("d_index inside d_out", index=inv + 5)
        refused("d_bits ends inside d_diff", bits=diff - 5 * n + 1)
        refused("d_not_first inside d_bits", not_first=bits + 2 * n)
        refused("a column inside d_out", col_ptrs=[inv + 32, c1, c2])
        refused("two columns at one address", col_ptrs=[c0, c1, c0 + 3])
        refused("d_out inside d_keys", out=a["keys"] + 64)
        refused("d_index AT d_perm", index=a["perm"])
        refused("a column inside d_keys", col_ptrs=[c0, c1, a["keys"] + 7])
        refused("flags with n = 0", flags=1, n=0)
        refused("a bad width with n = 0", col_specs=[(0, 4), (10, 3), (63, 1)], n=0)
        refused("group_limbs 33 with n = 0", group_limbs=33, n=0)
        refused("a second operand with n = 0", b=ctypes.c_void_p(a["keys"]), n=0)
        refused("Fq with n = 0", field=zk.FIELD_FQ, n=0)
        assert len(refusals) == 44
        assert raw_call(zk, ctx, t, n=0) == 0                               # n = 0: ZK_OK, nothing written
        assert raw_call(zk, ctx, t, n=0, diff=inv) == 0                     # nothing to overlap
        assert raw_call(zk, ctx, t, count=0, null_cols=True, null_d_cols=True, n=0) == 0
        ctx.sync()
        assert t.untouched()
        t.check()                                                           # the context still works
    finally:
        t.free()


def test_the_call_books_one_launch_and_its_bytes(ctx):
    keys = kc.random_keys(kc.rng(27), 500)

    def booked(t):
        ctx.sync()
        ctx.prof_reset()
        ctx.prof_enable(True)
        try:
            t.check()
            ms, launches = ctx.prof_get("key_order")
            assert ms > 0 and launches == 1
            return ctx.prof_get_bytes("key_order")
        finally:
            ctx.prof_enable(False)
            ctx.prof_reset()
            t.free()
    assert booked(Order(ctx, keys, outputs=())) == 500 * 192
    assert booked(Order(ctx, keys, perm=list(range(500)), cols=[(0, 4), (9, 1)])) == 500 * (192 + 8 + 32 + 1 + 5 + 1 + 5)

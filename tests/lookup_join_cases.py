"""The logUp multiplicity hash join (csrc/lookup.hip: k_lk_insert, k_lk_count) restated for the tests: a replica of its hash
(csrc/lkhash.hip.hpp, held to the compiled code by tests/test_lkhash_host.py), of its two slot formulas, a model of what the join
must return, and the engineered cases of tests/test_gpu_lookup_join.py.

Rows are Montgomery residues as the kernels see them: (n, 4) uint64 arrays, i.e. eight little-endian 32-bit limbs a row.  The join
compares limbs, so the cases build limbs directly (top limb <= 0x2FFFFFFF: below r, hence canonical) and never convert.

A case is a name and a list of calls (table, inputs, usable, n) made one after the other on one context, plus what must hold for
the list of results [(m as integers, lowest bad row or None)]: the model's results are checked against it on the CPU, the device's
against the model in full."""
import numpy as np

R_TOP_LIMB = 0x30644E72                    # the top limb of r: a row whose top limb is below it is canonical
TOP_LIMB_MASK = 0x2FFFFFFF
M32 = 0xFFFFFFFF
LK_COUNT_THREADS, LK_BLOCK_SLOT_BITS = 1024, 11
LK_BLOCK_SLOTS = 1 << LK_BLOCK_SLOT_BITS
INSERT_THREADS = 256


# ---- the hash
def limbs_of(row):
    """the eight 32-bit limbs of one row (4 x uint64), least significant first"""
    return [int(x) for x in np.ascontiguousarray(row, dtype=np.uint64).view(np.uint32)]


def fr_hash(limbs):
    """fr_hash of csrc/lkhash.hip.hpp on Python integers"""
    h = limbs[0]
    for i in range(1, 8):
        h = (((h ^ limbs[i]) * 0x9E3779B1) + (h >> 15)) & M32
    h ^= h >> 16
    h = h * 0x85EBCA6B & M32
    h ^= h >> 13
    h = h * 0xC2B2AE35 & M32
    h ^= h >> 16
    return h


def fr_hash_rows(rows):
    """fr_hash of every row of an (n, 4) uint64 array -> uint32 array (the same steps in wrapping uint32 arithmetic)"""
    l = np.ascontiguousarray(rows, dtype=np.uint64).view(np.uint32).reshape(-1, 8)
    h = l[:, 0].copy()
    for i in range(1, 8):
        h = (h ^ l[:, i]) * np.uint32(0x9E3779B1) + (h >> np.uint32(15))
    h ^= h >> np.uint32(16)
    h *= np.uint32(0x85EBCA6B)
    h ^= h >> np.uint32(13)
    h *= np.uint32(0xC2B2AE35)
    h ^= h >> np.uint32(16)
    return h


def hash_cap(usable):
    """slots of the global table: lookup_multiplicities_enqueue"""
    cap = 16
    while cap < 2 * usable:
        cap <<= 1
    return cap


def lds_home(row):
    """home slot of owner row `row` in the per-workgroup table of k_lk_count"""
    return (row * 0x9E3779B1 & M32) >> (32 - LK_BLOCK_SLOT_BITS)


def occupied_slots(table, usable):
    """the slots the global table holds once table[:usable] is inserted: with linear probing the SET of occupied slots does not
    depend on the order of insertion, so a serial insertion gives what the concurrent one leaves"""
    cap = hash_cap(usable)
    used, seen = set(), set()
    for i, h in enumerate(fr_hash_rows(table[:usable])):
        key = table[i].tobytes()
        if key in seen:
            continue
        seen.add(key)
        s = int(h) & (cap - 1)
        while s in used:
            s = (s + 1) & (cap - 1)
        used.add(s)
    return used, cap


def probe_path(row, used, cap):
    """the slots a probe for a value that is NOT in the table reads, up to and including the empty one that ends it"""
    s = fr_hash(limbs_of(row)) & (cap - 1)
    path = [s]
    while s in used:
        s = (s + 1) & (cap - 1)
        path.append(s)
    return path


# ---- the model
def multiplicities(table, inputs, usable, n):
    """-> (m, lowest bad row or None): m[i] = number of usable input rows whose value is the value of table row i, for the LAST
    usable row i that holds the value; m is n long, zero from `usable` on; an input row below `usable` whose value no usable table
    row holds is bad (and counts nowhere)"""
    owner = {}
    for i in range(usable):
        owner[table[i].tobytes()] = i
    m, bad = [0] * n, None
    for r in range(usable):
        i = owner.get(inputs[r].tobytes())
        if i is None:
            bad = r if bad is None else min(bad, r)
        else:
            m[i] += 1
    return m, bad


# ---- rows
def random_rows(rng, count):
    rows = rng.integers(0, 1 << 32, size=(count, 8), dtype=np.uint32)
    rows[:, 7] &= TOP_LIMB_MASK
    return np.ascontiguousarray(rows).view(np.uint64).reshape(count, 4)


def distinct_rows(rng, count, avoid=()):
    rows = random_rows(rng, count)
    keys = {r.tobytes() for r in rows} | {np.ascontiguousarray(a).tobytes() for a in avoid}
    assert len(keys) == count + len(avoid)
    return rows


def rows_with_home(rng, count, cap, lo, hi=None):
    """`count` distinct random rows whose home slot in a table of `cap` slots lies in [lo, hi]"""
    hi = cap - 1 if hi is None else hi
    found, tried = [], 0
    while len(found) < count:
        cand = random_rows(rng, 4096)
        tried += 4096
        home = fr_hash_rows(cand) & np.uint32(cap - 1)
        found += list(cand[(home >= lo) & (home <= hi)])
        assert tried < 1 << 22, "the search for clustered rows does not end"
    rows = np.array(found[:count], dtype=np.uint64)
    assert len({r.tobytes() for r in rows}) == count
    return rows


def next_pow2(v):
    p = 1
    while p < v:
        p <<= 1
    return p


class Case:
    def __init__(self, name, calls, expect=None):
        self.name, self.calls, self.expect = name, calls, expect or (lambda results: None)

    def __repr__(self):
        return self.name


def call(table, inputs, usable, n):
    table, inputs = np.ascontiguousarray(table, dtype=np.uint64), np.ascontiguousarray(inputs, dtype=np.uint64)
    assert table.shape == inputs.shape == (n, 4) and 0 < usable <= n
    assert int(table.view(np.uint32).reshape(-1, 8)[:, 7].max()) <= R_TOP_LIMB and int(inputs.view(np.uint32).reshape(-1, 8)[:, 7].max()) <= R_TOP_LIMB
    return (table, inputs, usable, n)


def padded(rng, table_usable, inputs_usable, n):
    """rows from `usable` on: table values and input values that occur nowhere else"""
    usable = len(table_usable)
    if n == usable:
        return np.array(table_usable), np.array(inputs_usable)
    extra = distinct_rows(rng, 2 * (n - usable))
    return np.concatenate([table_usable, extra[:n - usable]]), np.concatenate([inputs_usable, extra[n - usable:]])


# ---- the cases
SIZES = [1, 2, 7, 8, 9, 16, 17, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2049]


def size_cases():
    out = []
    for usable in SIZES:
        for n in (usable, next_pow2(usable + 6)):
            rng = np.random.default_rng(1000 * usable + n)
            table = distinct_rows(rng, usable)
            inputs = table[rng.integers(0, usable, size=usable)]
            t, i = padded(rng, table, inputs, n)
            out.append(Case(f"sizes: usable {usable}, n {n}", [call(t, i, usable, n)], _all_found))
    return out


def _all_found(results):
    for m, bad in results:
        assert bad is None


def one_value():
    rng = np.random.default_rng(3000)
    usable, n = 3000, 4096
    table = np.repeat(random_rows(rng, 1), n, axis=0)
    c = call(table, table.copy(), usable, n)

    def expect(res):
        assert res[0] == res[1] and res[0][1] is None
        assert res[0][0][usable - 1] == usable and sum(res[0][0]) == usable
    return Case("one value, twice", [c, c], expect)


RUNS_USABLE = 1500
# (first index, length, value) in the insert kernel's own index rows - 1 - row; value 0 occurs in two runs
RUNS = [(33, 63, 0), (128, 1, 1), (160, 64, 2), (230, 300, 3), (600, 65, 4), (700, 70, 0)]


def runs_from_the_top():
    rng = np.random.default_rng(1500)
    usable, n = RUNS_USABLE, 2048
    table = distinct_rows(rng, usable)
    values = distinct_rows(rng, 5, avoid=table)
    for start, length, v in RUNS:
        for idx in range(start, start + length):
            table[usable - 1 - idx] = values[v]
    inputs = table[rng.permutation(usable)]                                  # every row's value once: m[owner] = rows of the value
    t, i = padded(rng, table, inputs, n)

    def expect(res):
        m, bad = res[0]
        assert bad is None and sum(m) == usable
        assert m[usable - 1 - 33] == 63 + 70 and m[usable - 1 - 128] == 1 and m[usable - 1 - 160] == 64 and m[usable - 1 - 230] == 300 and m[usable - 1 - 600] == 65
        assert sorted(v for v in m if v > 1) == [64, 65, 133, 300]
    return Case("runs counted from the top", [call(t, i, usable, n)], expect)


def runs_straddle():
    """what the layout of RUNS claims: each run longer than one row straddles a multiple of 64, one a multiple of 256"""
    wave = [any(idx % 64 == 0 for idx in range(s + 1, s + l)) for s, l, _ in RUNS if l > 1]
    group = [any(idx % INSERT_THREADS == 0 for idx in range(s + 1, s + l)) for s, l, _ in RUNS if l > 1]
    return all(wave) and any(group) and {1, 63, 64, 65, 300} <= {l for _, l, _ in RUNS}


def everything_on_one_row():
    rng = np.random.default_rng(1777)
    n, usable = 4096, 4090
    table = distinct_rows(rng, n)
    inputs = np.repeat(table[1777:1778], n, axis=0)

    def expect(res):
        m, bad = res[0]
        assert bad is None and m[1777] == usable and sum(m) == usable
    return Case("everything on one row", [call(table, inputs, usable, n)], expect)


def workgroup_owners(rows, wrap_from=2040, shared=40):
    """1024 owner rows below `rows` for the first workgroup of k_lk_count: every row whose LDS home slot is >= wrap_from (up to 64
    of them), the `shared` rows of the most crowded home slot, the rest at random -> (owners, number that wrap, number that share)"""
    homes = np.array([lds_home(r) for r in range(rows)])
    top = [r for r in range(rows) if homes[r] >= wrap_from][:64]
    counts = np.bincount(homes, minlength=LK_BLOCK_SLOTS)
    counts[wrap_from:] = 0
    slot = int(counts.argmax())
    same = [r for r in range(rows) if homes[r] == slot][:shared]
    chosen = top + same
    rng = np.random.default_rng(rows)
    rest = [r for r in rng.permutation(rows) if r not in set(chosen)][:LK_COUNT_THREADS - len(chosen)]
    owners = np.array(chosen + [int(r) for r in rest])
    assert len(set(owners.tolist())) == LK_COUNT_THREADS
    return owners[rng.permutation(LK_COUNT_THREADS)], len(top), len(same)


def full_workgroup(rows):
    """a distinct table; input rows 0 .. 1023 -- one workgroup of k_lk_count -- hit 1024 different owner rows"""
    rng = np.random.default_rng(40 + rows)
    table = distinct_rows(rng, rows)
    owners, _, _ = workgroup_owners(rows)
    inputs = table[rng.integers(0, rows, size=rows)]
    inputs[:LK_COUNT_THREADS] = table[owners]
    return Case(f"a full workgroup of distinct owners, {rows} rows", [call(table, inputs, rows, rows)], _all_found)


WRAPS = [(16, 8, 8, 14), (64, 32, 20, 62), (2048, 1000, 24, 2044)]        # cap, usable, clustered values, their lowest home slot


def global_wrap(cap, usable, count, lo):
    rng = np.random.default_rng(cap)
    assert hash_cap(usable) == cap
    n = next_pow2(usable + 6)
    cluster = rows_with_home(rng, count, cap, lo)
    table = np.concatenate([cluster, distinct_rows(rng, usable - count, avoid=cluster)])
    table = table[rng.permutation(usable)]
    inputs = table[rng.integers(0, usable, size=usable)]
    cluster = table[(fr_hash_rows(table) & np.uint32(cap - 1)) >= lo]          # with the other rows that happen to start there
    inputs[rng.permutation(usable)[:len(cluster)]] = cluster                  # every clustered value is looked up
    t, good = padded(rng, table, inputs, n)
    absent = rows_with_home(rng, 3, cap, lo)
    assert not {a.tobytes() for a in absent} & {r.tobytes() for r in table}
    bad_rows = [usable - 1, 1, usable // 2]
    missing = good.copy()
    missing[bad_rows] = absent

    def expect(res):
        assert res[0][1] is None and sum(res[0][0]) == usable
        assert res[1][1] == 1 and sum(res[1][0]) == usable - 3
    return Case(f"global collisions that wrap, cap {cap}", [call(t, good, usable, n), call(t, missing, usable, n)], expect), absent


def usable_means_usable():
    rng = np.random.default_rng(40)
    n, usable = 64, 40
    table = distinct_rows(rng, n)
    inputs = table[rng.integers(0, usable, size=n)]
    w = distinct_rows(rng, 1, avoid=table)[0]
    inputs[50] = w                                                            # absent, in an unusable input row: ignored
    first = call(table, inputs, usable, n)
    inputs = inputs.copy()
    inputs[10] = table[usable + 3]                                            # present in an unusable table row only: missing
    inputs[30] = table[n - 1]

    def expect(res):
        assert res[0][1] is None and sum(res[0][0]) == usable
        assert res[1][1] == 10 and sum(res[1][0]) == usable - 2
    return Case("usable means usable", [first, call(table, inputs, usable, n)], expect)


def one_limb_apart():
    rng = np.random.default_rng(8)
    n, usable = 64, 40
    table = distinct_rows(rng, n)
    rows = rng.permutation(usable)[:18]
    for j in range(8):
        a, b = int(rows[2 * j]), int(rows[2 * j + 1])
        l = table[a].copy().view(np.uint32)
        l[j] ^= np.uint32(1 << int(rng.integers(0, 28)))                     # below bit 28: the top limb stays below r's
        table[b] = l.view(np.uint64)
    # and two rows with ONE hash: the same low bit flipped in limb 0 and in limb 1 (the first step of fr_hash takes l0 ^ l1 and l0 >> 15)
    la, lb = table[int(rows[16])].view(np.uint32), table[int(rows[17])].view(np.uint32)
    lb[:] = la
    la[0] ^= np.uint32(1)
    lb[1] ^= np.uint32(1)
    assert fr_hash(limbs_of(table[int(rows[16])])) == fr_hash(limbs_of(table[int(rows[17])]))
    assert len({r.tobytes() for r in table}) == n
    inputs = table[rng.integers(0, usable, size=n)]
    inputs[:18] = table[rows]
    inputs[18:27] = table[rows[0::2]]                                         # the first of each pair twice, the second once

    def expect(res):
        m, bad = res[0]
        assert bad is None and sum(m) == usable
        for j in range(9):
            assert m[int(rows[2 * j])] >= 2 and m[int(rows[2 * j + 1])] >= 1
    return Case("one limb apart", [call(table, inputs, usable, n)], expect)


def zero_cases(named):
    """named: the Montgomery rows of 0, 1 and r - 1"""
    zero = named[0]
    assert not zero.any()
    rng = np.random.default_rng(65)
    usable, n = 65, 128
    table = distinct_rows(rng, usable)
    table[0] = zero                                                           # index 64 from the top: alone in a partial wave
    inputs = table[rng.integers(0, usable, size=usable)]
    inputs[[3, 17, 64]] = zero
    t, i = padded(rng, table, inputs, n)
    count = int(sum(1 for r in inputs if not r.any()))

    def expect_a(res):
        assert res[0][1] is None and res[0][0][0] == count >= 3
    one = np.zeros((1, 4), dtype=np.uint64)

    def expect_b(res):
        assert res[0] == ([1], None)
    usable, n = 20, 32
    table = distinct_rows(rng, n)
    table[[4, 11, 19]] = named
    inputs = table[rng.integers(0, usable, size=n)]
    inputs[:6] = np.concatenate([named, named[::-1]])

    def expect_c(res):
        m, bad = res[0]
        assert bad is None and min(m[4], m[11], m[19]) >= 2
    return [Case("zero in a partial wave", [call(t, i, 65, 128)], expect_a), Case("zero alone", [call(one, one.copy(), 1, 1)], expect_b),
            Case("0, 1 and r - 1 in one table", [call(table, inputs, usable, n)], expect_c)]


def misses_and_reuse():
    rng = np.random.default_rng(4096)
    n, usable = 4096, 4090
    table = distinct_rows(rng, n)
    good = table[rng.integers(0, usable, size=n)]
    missing = good.copy()
    missing[[0, usable - 1]] = distinct_rows(rng, 2, avoid=table)
    small = distinct_rows(rng, 16)
    small_in = small[rng.integers(0, 16, size=16)]

    def expect(res):
        assert res[0][1] == 0 and sum(res[0][0]) == usable - 2
        assert res[1][1] is None and sum(res[1][0]) == usable
        assert res[2][1] is None and sum(res[2][0]) == 16
    return Case("misses, then reuse, then a small table on stale scratch",
                [call(table, missing, usable, n), call(table, good, usable, n), call(small, small_in, 16, 16)], expect)


def padded_profile():
    rng = np.random.default_rng(16)
    n, usable, distinct = 1 << 16, (1 << 16) - 6, 200
    rows = distinct_rows(rng, distinct + 1)
    table = np.repeat(rows[distinct:], n, axis=0)
    table[:distinct] = rows[:distinct]
    pick = rng.integers(0, distinct, size=n)
    inputs = np.where((rng.random(n) < 0.9)[:, None], rows[distinct], rows[pick])

    def expect(res):
        m, bad = res[0]
        assert bad is None and sum(m) == usable and m[usable - 1] > 0.85 * usable and sum(m[distinct:usable - 1]) == 0
    return Case("padded profile", [call(table, inputs, usable, n)], expect)


def build_cases(named):
    """every case; named = the Montgomery rows of 0, 1 and r - 1 (the only values that are meant as integers)"""
    cases = size_cases() + [one_value(), runs_from_the_top(), everything_on_one_row(), full_workgroup(4096), full_workgroup(1 << 17)]
    cases += [global_wrap(*w)[0] for w in WRAPS]
    cases += [usable_means_usable(), one_limb_apart()] + zero_cases(np.ascontiguousarray(named, dtype=np.uint64)) + [misses_and_reuse(), padded_profile()]
    return cases

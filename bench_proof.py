#!/usr/bin/env python
"""bench_proof.py -- wall-clock of a FULL proof (keygen_pk + create_proof) on one MI355X for a
synthetic-shape PLONKish circuit, verified afterwards by the oracle's pairing-based verifier.

BASELINE.json's metric is "SuperCircuit proof-gen wall-clock (s) at k"; a real SuperCircuit /
Keccak witness needs the reference's Rust + Go toolchain (absent here), so this uses a
synthetic circuit with the same ingredients (custom gates with rotations up to degree 5, a chunked
permutation argument over every advice column, logUp lookups) and labels every number
"synthetic-shape".  Not the driver's bench (that is bench.py); prints one JSON line.

usage: python bench_proof.py [--k 16] [--groups 10] [--no-verify]
"""
import argparse
import ctypes
import json
import os
import random
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import zkevm_circuits_amd as z  # noqa: E402
from zkevm_circuits_amd import plonk  # noqa: E402

R = plonk.R_MOD


def build(k: int, groups: int, seed: int = 1):
    """groups x (a, b, c) advice triples; gates per group: q_mul (a b - c), q_add (a + b - c.next);
    one degree-5 gate on group 0; one 2-column lookup on group 0; every advice column is in the
    permutation, with a chain of copy constraints per group."""
    rng = random.Random(seed)
    A, F = 3 * groups, 6
    c = plonk.Circuit(k, num_fixed=F, num_advice=A, num_instance=1, blinding_factors=5)
    n, u = c.n, c.u
    q_mul, q_add, q_cube, q_lk, t_a, t_b = (c.fixed_col(i) for i in range(F))
    for g in range(groups):
        a, b_, cc = (c.advice_col(3 * g + i) for i in range(3))
        c.add_gate(q_mul * (a * b_ - cc))
        c.add_gate(q_add * (a + b_ - cc.rot(1)))
    a0, b0, c0 = c.advice_col(0), c.advice_col(1), c.advice_col(2)
    c.add_gate(q_cube * (a0 * a0 * a0 * b0 + 7 - c0.rot(-1)))
    c.add_lookup([q_lk * a0, q_lk * b0], [t_a, t_b])
    tab_n = min(4096, u)
    for row in range(u):
        if 0 < row < tab_n:
            c.fixed[4][row], c.fixed[5][row] = row, (row * row + 3) % R
    adv = [[0] * n for _ in range(A)]
    inst = [[0] * n]
    kinds = [rng.randrange(4) for _ in range(u // 3)]
    for ri, kind in enumerate(kinds):
        row = 1 + 3 * ri
        if row + 3 >= u:
            break
        if kind == 0:
            c.fixed[0][row] = 1
            for g in range(groups):
                x, y = rng.getrandbits(60), rng.getrandbits(60)
                adv[3 * g][row], adv[3 * g + 1][row], adv[3 * g + 2][row] = x, y, x * y % R
        elif kind == 1:
            c.fixed[1][row] = 1
            for g in range(groups):
                x, y = rng.getrandbits(60), rng.getrandbits(60)
                adv[3 * g][row], adv[3 * g + 1][row], adv[3 * g + 2][row + 1] = x, y, x + y
        elif kind == 2:
            c.fixed[2][row + 1] = 1
            x, y = rng.getrandbits(60), rng.getrandbits(60)
            adv[0][row + 1], adv[1][row + 1] = x, y
            adv[2][row] = (x * x * x * y + 7) % R
        else:
            c.fixed[3][row] = 1
            i = rng.randrange(1, tab_n)
            adv[0][row], adv[1][row] = i, (i * i + 3) % R
    for col in range(A):
        c.enable_equality(plonk.ADVICE, col)
    # copy constraints: c of one mul row feeds a of a later mul row (same group); a few public inputs
    mul_rows = [1 + 3 * ri for ri, kd in enumerate(kinds) if kd == 0 and 1 + 3 * ri + 3 < u]
    for g in range(groups):
        for r0, r1 in list(zip(mul_rows[:-1:2], mul_rows[1::2]))[:256]:
            x = adv[3 * g + 2][r0]
            adv[3 * g][r1] = x
            adv[3 * g + 2][r1] = x * adv[3 * g + 1][r1] % R
            c.copy((plonk.ADVICE, 3 * g + 2, r0), (plonk.ADVICE, 3 * g, r1))
    for j, r0 in enumerate(mul_rows[:4]):
        inst[0][j] = adv[1][r0]
        c.copy((plonk.ADVICE, 1, r0), (plonk.INSTANCE, 0, j))
    return c, adv, inst


def to_mont_gpu(ctx, canon: np.ndarray) -> np.ndarray:
    """(n, 4) u64 canonical integers -> Montgomery form on the device: Montgomery-multiplying by the
    plain integer R^2 mod r gives a*R (big-int conversion in Python takes seconds per 2^20 column)."""
    r2 = np.frombuffer(plonk.fr_mont_bytes((1 << 256) % R), dtype=np.uint64).copy()
    buf = ctx.to_device(np.ascontiguousarray(canon))
    ctx.fr_scale(buf, r2, canon.shape[0])
    out = buf.download(canon.shape)
    buf.free()
    return out


def small_to_limbs(v: np.ndarray) -> np.ndarray:
    out = np.zeros((v.shape[0], 4), dtype=np.uint64)
    out[:, 0] = v
    return out


def build_large(ctx, k: int, groups: int, seed: int = 1):
    """Vectorised (numpy + device-side Montgomery conversion) version of `build` for k = 18..22:
    same gate / lookup / permutation structure, witness values < 2^30 so products fit 64 bits.
    Returns (circuit shell for the verifier, blob, advice arrays (Montgomery), instance arrays)."""
    rng = np.random.default_rng(seed)
    A, F = 3 * groups, 6
    c = plonk.Circuit(k, num_fixed=F, num_advice=A, num_instance=1, blinding_factors=5)
    n, u = c.n, c.u
    q_mul, q_add, q_cube, q_lk, t_a, t_b = (c.fixed_col(i) for i in range(F))
    for g in range(groups):
        a, b_, cc = (c.advice_col(3 * g + i) for i in range(3))
        c.add_gate(q_mul * (a * b_ - cc))
        c.add_gate(q_add * (a + b_ - cc.rot(1)))
    a0, b0, c0 = c.advice_col(0), c.advice_col(1), c.advice_col(2)
    c.add_gate(q_cube * (a0 * a0 + b0 - c0.rot(-1)) * (a0 + 1) * (b0 + 2))      # degree 5
    c.add_lookup([q_lk * a0, q_lk * b0], [t_a, t_b])
    for col in range(A):
        c.enable_equality(plonk.ADVICE, col)
    c.enable_equality(plonk.INSTANCE, 0)
    # row pattern: regions of 3 rows, kind = region index mod 4 shuffled
    nreg = (u - 4) // 3
    kinds = rng.integers(0, 4, size=nreg)
    rows = 1 + 3 * np.arange(nreg)
    fixed = np.zeros((F, n), dtype=np.uint64)
    fixed[0, rows[kinds == 0]] = 1
    fixed[1, rows[kinds == 1]] = 1
    fixed[2, rows[kinds == 2] + 1] = 1
    fixed[3, rows[kinds == 3]] = 1
    tab_n = min(4096, u)
    ti = np.arange(tab_n, dtype=np.uint64)
    fixed[4, 1:tab_n] = ti[1:]
    fixed[5, 1:tab_n] = ti[1:] * ti[1:] + 3
    adv = np.zeros((A, n), dtype=np.uint64)
    r_mul, r_add, r_cube, r_lk = rows[kinds == 0], rows[kinds == 1], rows[kinds == 2] + 1, rows[kinds == 3]
    for g in range(groups):
        x = rng.integers(0, 1 << 30, size=r_mul.size, dtype=np.uint64)
        y = rng.integers(0, 1 << 30, size=r_mul.size, dtype=np.uint64)
        adv[3 * g, r_mul], adv[3 * g + 1, r_mul], adv[3 * g + 2, r_mul] = x, y, x * y
        x = rng.integers(0, 1 << 30, size=r_add.size, dtype=np.uint64)
        y = rng.integers(0, 1 << 30, size=r_add.size, dtype=np.uint64)
        adv[3 * g, r_add], adv[3 * g + 1, r_add], adv[3 * g + 2, r_add + 1] = x, y, x + y
    x = rng.integers(0, 1 << 20, size=r_cube.size, dtype=np.uint64)
    y = rng.integers(0, 1 << 20, size=r_cube.size, dtype=np.uint64)
    adv[0, r_cube], adv[1, r_cube], adv[2, r_cube - 1] = x, y, x * x + y
    i = rng.integers(1, tab_n, size=r_lk.size, dtype=np.uint64)
    adv[0, r_lk], adv[1, r_lk] = i, i * i + 3
    # copy constraints: disjoint pairs -- product of a mul row feeds `a` of the next mul row (per group)
    npairs = min(256, r_mul.size // 2)
    src, dst = r_mul[0:2 * npairs:2], r_mul[1:2 * npairs:2]
    copies = []
    for g in range(groups):
        adv[3 * g, dst] = adv[3 * g + 2, src] % np.uint64(1 << 30)          # keep products inside 64 bits
        adv[3 * g + 2, src] = adv[3 * g, dst]                                 # ... so make the source cell equal
        # re-satisfy the mul gate at src (a*b = c): set a = c, b = 1;  and at dst: c = a*b
        adv[3 * g, src], adv[3 * g + 1, src] = adv[3 * g + 2, src], 1
        adv[3 * g + 2, dst] = adv[3 * g, dst] * adv[3 * g + 1, dst]
        copies += [((plonk.ADVICE, 3 * g + 2, int(s)), (plonk.ADVICE, 3 * g, int(d))) for s, d in zip(src, dst)]
    inst = np.zeros((1, n), dtype=np.uint64)
    pub = r_add[:4]
    inst[0, :pub.size] = adv[1, pub]
    copies += [((plonk.ADVICE, 1, int(r0)), (plonk.INSTANCE, 0, j)) for j, r0 in enumerate(pub)]
    c.copies = copies
    # ---- Montgomery forms via the device
    fixed_m = [to_mont_gpu(ctx, small_to_limbs(fixed[i])) for i in range(F)]
    adv_m = [to_mont_gpu(ctx, small_to_limbs(adv[i])) for i in range(A)]
    inst_m = [to_mont_gpu(ctx, small_to_limbs(inst[0]))]
    # sigma columns: identity delta^j * omega^i generated on the device, then the 2-cycles swapped in
    P = len(c.perm_cols)
    pos = {pc: j for j, pc in enumerate(c.perm_cols)}
    omega_m = np.frombuffer(plonk.fr_mont_bytes(c.omega()), dtype=np.uint64).copy()
    sig = []
    tmp = ctx.alloc(n * 32)
    for j in range(P):
        ctx.fr_powers(omega_m, np.frombuffer(plonk.fr_mont_bytes(pow(plonk.FR_DELTA, j, R)), dtype=np.uint64).copy(), tmp, n)
        sig.append(tmp.download((n, 4)))
    tmp.free()
    for (ta, ia, ra), (tb, ib, rb) in copies:
        ja, jb = pos[(ta, ia)], pos[(tb, ib)]
        sig[ja][ra], sig[jb][rb] = sig[jb][rb].copy(), sig[ja][ra].copy()
    # the Circuit object keeps Python-int fixed columns only for the verifier's instance / gate evaluation: not needed
    # there (the verifier reads evaluations from the proof), so serialise the blob directly from the arrays
    parts = [c.cs_blob()]
    parts += [f.tobytes() for f in fixed_m] + [s_.tobytes() for s_ in sig]
    inst_int = [[int(v) for v in inst[0]]]
    return c, b"".join(parts), adv_m, inst_m, inst_int


def assemble_blob(ctx, c, F: int, fixed_of, copies):
    """key blob of circuit `c` with F fixed columns given as Montgomery arrays (fixed_of(i)) and the
    sigma columns of `copies`, written in place (no Python-side copies of the columns)"""
    n = c.n
    Pn = len(c.perm_cols)
    head = c.cs_blob(cse=os.environ.get("ZK_BENCH_CSE") == "1")
    col_bytes = n * 32
    total = len(head) + (F + Pn) * col_bytes
    raw = np.empty(total + 8, dtype=np.uint8)
    shift = (-(raw.ctypes.data + len(head))) % 8       # columns 8-byte aligned in memory (u64 views below)
    blob = raw[shift:shift + total]
    blob[:len(head)] = np.frombuffer(head, dtype=np.uint8)
    off = len(head)
    for i in range(F):
        blob[off:off + col_bytes] = fixed_of(i).view(np.uint8).reshape(-1)
        off += col_bytes
    pos = {pc: j for j, pc in enumerate(c.perm_cols)}
    omega_m = np.frombuffer(plonk.fr_mont_bytes(c.omega()), dtype=np.uint64).copy()
    sig_view = [blob[off + j * col_bytes: off + (j + 1) * col_bytes].view(np.uint64).reshape(n, 4) for j in range(Pn)]
    tmp = ctx.alloc(col_bytes)
    for j in range(Pn):
        ctx.fr_powers(omega_m, np.frombuffer(plonk.fr_mont_bytes(pow(plonk.FR_DELTA, j, R)), dtype=np.uint64).copy(), tmp, n)
        ctx._ck(z.binding.lib().zk_d2h(ctx.h, sig_view[j].ctypes.data_as(ctypes.c_void_p), ctypes.c_void_p(tmp.ptr), ctypes.c_size_t(col_bytes)))
    tmp.free()
    for (ta_, ia, ra), (tb_, ib, rb) in copies:
        ja, jb = pos[(ta_, ia)], pos[(tb_, ib)]
        va, vb = sig_view[ja][ra].copy(), sig_view[jb][rb].copy()
        sig_view[ja][ra], sig_view[jb][rb] = vb, va
    return blob


def build_keccak_shape(ctx, k: int, pairs: int = 48, window: int = 12, lookups: int = 7, d: int = 9, seed: int = 1):
    """SURVEY 8d config 3 stand-in (Keccak circuit, k = 18): the packed-multi Keccak circuit at 12
    rows per round has 59 unusable rows [REF zkevm-circuits/src/keccak_circuit/keccak_packed_multi.rs:59-68]
    -- i.e. some column is queried at dozens of rotations --, maximum degree 9
    [REF zkevm-circuits/src/keccak_circuit/param.rs:1] and a handful of table lookups.  Shape used
    here: `pairs` column pairs (a_j, b_j), all with distinct data;
        q_sum * (a + a.rot(1) + ... + a.rot(window-1) - b.rot(-3))        window + 1 rotations of a_j
        q_far * (a.rot(-5) * a.rot(window-5) - b)
        q_hi * (a_0^2 - b_0.rot(1)) * (a_0 + 1)...(a_0 + d - 3)           degree d
        `lookups` lookups (q_lk * a_j) in a 4096-row table
    58 blinding factors (59 unusable rows), copy constraints into the instance column."""
    rng = np.random.default_rng(seed)
    A, F = 2 * pairs, 5
    c = plonk.Circuit(k, num_fixed=F, num_advice=A, num_instance=1, blinding_factors=58)
    c.fixed = None
    n, u = c.n, c.u
    q_sum, q_far, q_lk, t_a, q_hi = (c.fixed_col(i) for i in range(F))
    for j in range(pairs):
        a, b_ = c.advice_col(2 * j), c.advice_col(2 * j + 1)
        acc = a
        for i in range(1, window):
            acc = acc + a.rot(i)
        c.add_gate(q_sum * (acc - b_.rot(-3)))
        c.add_gate(q_far * (a.rot(-5) * a.rot(window - 5) - b_))
    a0, b0 = c.advice_col(0), c.advice_col(1)
    hi = q_hi * (a0 * a0 - b0.rot(1))
    for i in range(d - 3):
        hi = hi * (a0 + (i + 1))
    c.add_gate(hi)
    for l in range(lookups):
        c.add_lookup([q_lk * c.advice_col(2 * (l % pairs))], [t_a])
    for j in range(min(6, pairs)):
        c.enable_equality(plonk.ADVICE, 2 * j + 1)
    c.enable_equality(plonk.INSTANCE, 0)
    assert c.degree() == d, (c.degree(), d)
    tab_n = min(4096, u)
    rows = np.arange(8, u - window - 2)
    r0, r2, r3 = rows[rows % 4 == 0], rows[rows % 4 == 2], rows[rows % 4 == 3]
    a_v = np.zeros((pairs, n), dtype=np.uint64)
    a_v[:, :u] = rng.integers(0, tab_n, size=(pairs, u), dtype=np.uint64)
    b_v = np.zeros((pairs, n), dtype=np.uint64)
    for i in range(window):
        b_v[:, r0 - 3] += a_v[:, r0 + i]
    b_v[:, r2] = a_v[:, r2 - 5] * a_v[:, r2 + window - 5]
    b_v[0, r3 + 1] = a_v[0, r3] * a_v[0, r3]                  # the degree-d gate reads pair 0 only
    inst = np.zeros((1, n), dtype=np.uint64)
    pub = r2[:4]
    inst[0, :pub.size] = b_v[0, pub]
    copies = [((plonk.ADVICE, 1, int(r_)), (plonk.INSTANCE, 0, j)) for j, r_ in enumerate(pub)]
    for j in range(1, min(6, pairs)):                         # tie equal cells of different columns together
        b_v[j, r2[10 + j]] = b_v[0, r2[10]]
        a_v[j, r2[10 + j] - 5], a_v[j, r2[10 + j] + window - 5] = a_v[0, r2[10] - 5], a_v[0, r2[10] + window - 5]
        copies.append(((plonk.ADVICE, 1, int(r2[10])), (plonk.ADVICE, 2 * j + 1, int(r2[10 + j]))))
    # the changed a cells feed rotation sums: recompute the sums of the touched pairs
    for j in range(1, min(6, pairs)):
        b_v[j, r0 - 3] = 0
        for i in range(window):
            b_v[j, r0 - 3] += a_v[j, r0 + i]
        b_v[j, r2] = a_v[j, r2 - 5] * a_v[j, r2 + window - 5]
    c.copies = copies
    if ctx is None:
        # host-only variant (the restated CPU prover's input, bench.py cpu_baseline leg): fixed and advice columns as
        # Montgomery arrays made by the oracle's C conversion, nothing touches a device
        from oracle import cref
        import ctypes

        def host_mont(v):
            canon = np.ascontiguousarray(small_to_limbs(v))
            out = np.empty_like(canon)
            cref.lib().orc_fe_to_mont_vec(0, canon.ctypes.data_as(ctypes.c_void_p), out.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(canon.shape[0]))
            return out

        def sel_h(rows_):
            v = np.zeros(n, dtype=np.uint64)
            v[rows_] = 1
            return host_mont(v)
        ta_h = np.zeros(n, dtype=np.uint64)
        ta_h[:tab_n] = np.arange(tab_n, dtype=np.uint64)
        c.fixed = [sel_h(r0), sel_h(r2), sel_h(np.arange(u)), host_mont(ta_h), sel_h(r3)]
        adv_h = []
        for j in range(pairs):
            adv_h += [host_mont(a_v[j]), host_mont(b_v[j])]
        return c, adv_h, [[int(v) for v in inst[0, :pub.size]]]
    adv_m = []
    for j in range(pairs):
        adv_m.append(to_mont_gpu(ctx, small_to_limbs(a_v[j])))
        adv_m.append(to_mont_gpu(ctx, small_to_limbs(b_v[j])))
    inst_m = [to_mont_gpu(ctx, small_to_limbs(inst[0]))]

    def sel(rows_):
        v = np.zeros(n, dtype=np.uint64)
        v[rows_] = 1
        return to_mont_gpu(ctx, small_to_limbs(v))
    ta = np.zeros(n, dtype=np.uint64)
    ta[:tab_n] = np.arange(tab_n, dtype=np.uint64)
    fixed_m = [sel(r0), sel(r2), sel(np.arange(u)), to_mont_gpu(ctx, small_to_limbs(ta)), sel(r3)]
    blob = assemble_blob(ctx, c, F, lambda i: fixed_m[i], copies)
    inst_int = [[int(v) for v in inst[0]]]
    return c, blob, adv_m, inst_m, inst_int


def build_halo2_base_shape(ctx, k: int, num_advice: int, num_lookup_advice: int = 1, lookup_bits: int = 20, seed: int = 1):
    """An aggregation-layer circuit as halo2-base's FlexGate / RangeChip lay it out, sized by the reference's own config files
    [REF aggregator/configs/bundle_circuit.config] (degree 21, 5 advice + 1 lookup advice, 1 fixed), `compression_wide.config`
    (22, 8 + 1, 1), `compression_thin.config` (26, 1 + 1, 1).  The constraint system is the one the reference-held ChunkProof's protocol
    spells out (tests/golden/reference_chunk_proof.json: `quotient.numerator`): per basic-gate advice column a selector q_i and the
    gate q_i * (a + a.rot(1) * a.rot(2) - a.rot(3)); one logUp lookup of the lookup-advice column into a fixed range table
    [0, 2^lookup_bits); a permutation over the constants column, every advice column and the instance column; blinding_factors = 6.
    Witness: disjoint 4-row gate instances over 88-bit-limb-sized operands (field-sized products), range-checked copies below
    2^lookup_bits in the lookup column."""
    rng = np.random.default_rng(seed)
    A = num_advice + num_lookup_advice
    F = 2 + num_advice                              # range table | constants | one selector per basic-gate column
    c = plonk.Circuit(k, num_fixed=F, num_advice=A, num_instance=1, blinding_factors=6)
    c.fixed = None
    n, u = c.n, c.u
    table, consts = c.fixed_col(0), c.fixed_col(1)
    c.enable_equality(plonk.FIXED, 1)
    for i in range(num_advice):
        a = c.advice_col(i)
        c.add_gate(c.fixed_col(2 + i) * (a + a.rot(1) * a.rot(2) - a.rot(3)))
    for j in range(num_lookup_advice):
        c.lookup_any("range", [c.advice_col(num_advice + j)], [table])
    c.chunk_lookups()
    for i in range(A):
        c.enable_equality(plonk.ADVICE, i)
    c.enable_equality(plonk.INSTANCE, 0)
    assert c.halo2_blinding_factors() == c.bf, (c.halo2_blinding_factors(), c.bf)
    rows = np.arange(0, u - 8, 4)
    tab_n = min(1 << lookup_bits, u)
    mont = lambda limbs: to_mont_gpu(ctx, np.ascontiguousarray(limbs))

    def rand_limbs(m, bits):                         # canonical integers below 2^bits as (m, 4) u64
        out = np.zeros((m, 4), dtype=np.uint64)
        full, rest = divmod(bits, 64)
        for w in range(full):
            out[:, w] = rng.integers(0, 1 << 63, size=m, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=m, dtype=np.uint64)
        if rest:
            out[:, full] = rng.integers(0, 1 << rest, size=m, dtype=np.uint64)
        return out
    adv_m, fixed_m = [], []
    ta = np.zeros((n, 4), dtype=np.uint64)
    ta[:tab_n, 0] = np.arange(tab_n, dtype=np.uint64)
    fixed_m.append(mont(ta))
    fixed_m.append(np.zeros((n, 4), dtype=np.uint64))          # constants column (zeros; the copy constraints below use advice cells)
    sel = np.zeros((n, 4), dtype=np.uint64)
    sel[rows, 0] = 1
    sel_m = mont(sel)
    one = np.frombuffer(plonk.fr_mont_bytes(1), dtype=np.uint64)
    first_d = None
    for i in range(num_advice):
        fixed_m.append(sel_m)
        # a, b, c at rows r, r+1, r+2 (88-bit limbs), d = a + b * c at r+3: computed on the device (Montgomery product of the
        # Montgomery images is the image of the product)
        col = np.zeros((n, 4), dtype=np.uint64)
        col[rows], col[rows + 1], col[rows + 2] = rand_limbs(rows.size, 88), rand_limbs(rows.size, 88), rand_limbs(rows.size, 88)
        col_m = mont(col)
        bbuf, cbuf, abuf = ctx.to_device(np.ascontiguousarray(col_m[rows + 1])), ctx.to_device(np.ascontiguousarray(col_m[rows + 2])), ctx.to_device(np.ascontiguousarray(col_m[rows]))
        ctx.field_vec_op(0, 2, bbuf, cbuf, bbuf, rows.size)
        ctx.field_vec_op(0, 0, bbuf, abuf, bbuf, rows.size)
        col_m[rows + 3] = bbuf.download((rows.size, 4))
        for b_ in (abuf, bbuf, cbuf):
            b_.free()
        adv_m.append(col_m)
        if first_d is None:
            first_d = col_m[rows[:4] + 3].copy()
    copies = []
    for j in range(num_lookup_advice):
        lk = np.zeros((n, 4), dtype=np.uint64)
        lk[:u, 0] = rng.integers(0, tab_n, size=u, dtype=np.uint64)
        lk_m = mont(lk)
        # a few range-checked cells are copies of cells of the first gate column (what RangeChip does: copy, then look up):
        # make those gate operands small and recompute their d
        adv_m.append(lk_m)
    inst = np.zeros((1, n), dtype=np.uint64)
    inst_m_full = np.zeros((n, 4), dtype=np.uint64)
    inst_m_full[:4] = first_d                       # public inputs = the first four gate outputs of column 0
    copies += [((plonk.ADVICE, 0, int(rows[j] + 3)), (plonk.INSTANCE, 0, j)) for j in range(4)]
    for i in range(1, num_advice):                  # equal cells across columns: outputs of column i - 1 feed operand a of column i (same row block)
        for r_ in rows[4:36]:
            adv_m[i][r_] = adv_m[i - 1][r_ + 3]
            copies.append(((plonk.ADVICE, i - 1, int(r_ + 3)), (plonk.ADVICE, i, int(r_))))
        # operand a changed: recompute d on those rows
        sub = rows[4:36]
        abuf, bbuf, cbuf = (ctx.to_device(np.ascontiguousarray(adv_m[i][sub + o])) for o in (0, 1, 2))
        ctx.field_vec_op(0, 2, bbuf, cbuf, bbuf, sub.size)
        ctx.field_vec_op(0, 0, bbuf, abuf, bbuf, sub.size)
        adv_m[i][sub + 3] = bbuf.download((sub.size, 4))
        for b_ in (abuf, bbuf, cbuf):
            b_.free()
    c.copies = copies
    blob = assemble_blob(ctx, c, F, lambda i: fixed_m[i], copies)
    rinv = pow(1 << 256, -1, R)
    inst_int = [[(int(v[0]) | int(v[1]) << 64 | int(v[2]) << 128 | int(v[3]) << 192) * rinv % R for v in inst_m_full[:4]] + [0] * (n - 4)]
    return c, blob, adv_m, [inst_m_full], inst_int


def build_reference_cs_shape(ctx, k: int, seed: int = 1, table_bits: int = 16):
    """The constraint system of the reference-held ChunkProof (tests/golden/reference_chunk_proof.json: `protocol`; a halo2-base
    circuit as [REF aggregator/data/batch-task.json] carries it) at any k, built with numpy: fixed 0 = lookup table, 1 = constants
    (equality-enabled), 2 = q_gate, 3 = q_lookup; ONE advice column a under q_gate * (a + a.rot(1) * a.rot(2) - a.rot(3)); the lookup
    (q_lookup * a) in the table; permutation over (fixed 1, advice 0, instance 0); blinding_factors = 6; queries registered in the order
    of the fixture's evaluation list -- the same object tests/test_gpu_reference_protocol.build_reference_cs builds cell by cell at k = 8,
    so that a proof at an aggregation layer's size (k = 21 .. 25) can be put in front of the verifier driven by the reference's own
    protocol object."""
    rng = np.random.default_rng(seed)
    c = plonk.Circuit(k, num_fixed=4, num_advice=1, num_instance=1, blinding_factors=6)
    c.fixed = None
    table, consts, q_gate, q_lookup = (c.fixed_col(i) for i in range(4))
    a = c.advice_col(0)
    c.enable_equality(plonk.FIXED, 1)
    c.add_gate(q_gate * (a + a.rot(1) * a.rot(2) - a.rot(3)))
    c.lookup_any("range", [q_lookup * a], [table])
    c.chunk_lookups()
    c.enable_equality(plonk.ADVICE, 0)
    c.enable_equality(plonk.INSTANCE, 0)
    c.fixed_queries = [(1, 0), (0, 0), (2, 0), (3, 0)]
    assert c.advice_queries == [(0, 0), (0, 1), (0, 2), (0, 3)] and c.degree() == 5 and c.halo2_blinding_factors() == 6
    n, u = c.n, c.u
    tab_n = min(1 << table_bits, u // 4)
    n_lk = min(u // 4, 1 << 18) & ~3                 # range-checked cells below the gates
    gates = np.arange(0, u - n_lk - 8, 4)
    lk_rows = np.arange(u - n_lk - 4, u - 4)
    mont = lambda limbs: to_mont_gpu(ctx, np.ascontiguousarray(limbs))

    def rand_limbs(m, bits):
        out = np.zeros((m, 4), dtype=np.uint64)
        full, rest = divmod(bits, 64)
        for w in range(full):
            out[:, w] = rng.integers(0, 1 << 63, size=m, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=m, dtype=np.uint64)
        if rest:
            out[:, full] = rng.integers(0, 1 << rest, size=m, dtype=np.uint64)
        return out
    col = np.zeros((n, 4), dtype=np.uint64)
    col[gates], col[gates + 1], col[gates + 2] = rand_limbs(gates.size, 250), rand_limbs(gates.size, 250), rand_limbs(gates.size, 250)
    col[lk_rows, 0] = rng.integers(0, tab_n, size=lk_rows.size, dtype=np.uint64)
    col[lk_rows[3]] = col[lk_rows[2]]
    col_m = mont(col)
    abuf, bbuf, cbuf = (ctx.to_device(np.ascontiguousarray(col_m[gates + o])) for o in (0, 1, 2))
    ctx.field_vec_op(0, 2, bbuf, cbuf, bbuf, gates.size)          # d = a + b c on the device (Montgomery images)
    ctx.field_vec_op(0, 0, bbuf, abuf, bbuf, gates.size)
    col_m[gates + 3] = bbuf.download((gates.size, 4))
    for b_ in (abuf, bbuf, cbuf):
        b_.free()
    ta = np.zeros((n, 4), dtype=np.uint64); ta[:tab_n, 0] = np.arange(tab_n, dtype=np.uint64)
    kon = np.zeros((n, 4), dtype=np.uint64); kon[0], kon[1] = col[lk_rows[0]], col[lk_rows[1]]
    qg = np.zeros((n, 4), dtype=np.uint64); qg[gates, 0] = 1
    ql = np.zeros((n, 4), dtype=np.uint64); ql[lk_rows, 0] = 1
    fixed_m = [mont(ta), mont(kon), mont(qg), mont(ql)]
    copies = [((plonk.FIXED, 1, 0), (plonk.ADVICE, 0, int(lk_rows[0]))), ((plonk.FIXED, 1, 1), (plonk.ADVICE, 0, int(lk_rows[1]))),
              ((plonk.ADVICE, 0, int(lk_rows[2])), (plonk.ADVICE, 0, int(lk_rows[3]))),
              ((plonk.ADVICE, 0, int(gates[0] + 3)), (plonk.INSTANCE, 0, 0)), ((plonk.ADVICE, 0, int(gates[1] + 3)), (plonk.INSTANCE, 0, 1))]
    c.copies = copies
    blob = assemble_blob(ctx, c, 4, lambda i: fixed_m[i], copies)
    inst_m_full = np.zeros((n, 4), dtype=np.uint64)
    inst_m_full[0], inst_m_full[1] = col_m[gates[0] + 3], col_m[gates[1] + 3]
    rinv = pow(1 << 256, -1, R)
    to_int = lambda v: (int(v[0]) | int(v[1]) << 64 | int(v[2]) << 128 | int(v[3]) << 192) * rinv % R
    inst_int = [[to_int(inst_m_full[0]), to_int(inst_m_full[1])] + [0] * (n - 2)]
    return c, blob, [col_m], [inst_m_full], inst_int


# ---------------------------------------------------------------------------------------------------------------- EVM-style block
EVM_DEFAULT = {"states": 80, "per_state": 64, "cond_cols": 8, "input_cols": 77, "seed": 7}


def evm_step_columns(p: dict) -> int:
    """advice columns an EVM-style block with these parameters occupies: q_step | pair bits | odd | condition bits | inputs |
    outputs | rw_counter"""
    pairs = (p["states"] + 1) // 2
    return 1 + pairs + 1 + p["cond_cols"] + p["input_cols"] + (p["per_state"] + 1) // 2 + 1


def evm_block(c, first_col: int, q_usable, p: dict):
    """The constraint system of an EVM-circuit-like state machine over S = evm_step_columns(p) advice columns starting at `first_col`
    (what the reference's ExecutionConfig emits, restated as a generator -- the circuit itself needs the Rust workspace):

      * a step is 2 rows high; `q_step` (an ADVICE column, as in [REF zkevm-circuits/src/evm_circuit/execution.rs:265,410]) marks
        its first row; a step's cells are its columns at rotations 0 and 1, the next step's at rotation 2;
      * the execution state is a DynamicSelectorHalf [REF zkevm-circuits/src/evm_circuit/step.rs:624-631]: ceil(states/2) pair bits
        and one `odd` bit, state_selector_s = pair[s/2] * (odd or 1 - odd): degree 2;
      * every constraint of state s is the polynomial  q_usable * q_step * state_selector_s * (constraint * condition)
        [REF execution.rs:839-851]: implicit degree 4 [REF util/constraint_builder.rs:33-34], constraint * condition of degree 1 .. 5
        (the builder splits only above that [REF util/constraint_builder.rs:322-341]), so the polynomials have degree 5 .. 9;
      * `per_state` constraints per state in gadget blocks of eight that share one condition (a product of up to two condition
        cells: the builder's condition stack), eight constraint forms (multiply-add, byte composition, triple product, select,
        ...), each defining one output cell of the step from its input cells; one state-transition constraint per state
        (rw_counter(next) = rw_counter + delta_s); booleanity of every selector / condition bit and "exactly one pair bit" under
        q_usable * q_step.
    Adds the gates to `c` and returns the spec `evm_witness` fills the columns from."""
    import random as _random
    rng = _random.Random(p["seed"])
    ns, per = p["states"], p["per_state"]
    pairs = (ns + 1) // 2
    col = first_col
    q_step_c = col; col += 1
    pair_c = list(range(col, col + pairs)); col += pairs
    odd_c = col; col += 1
    cond_c = list(range(col, col + p["cond_cols"])); col += p["cond_cols"]
    in_c = list(range(col, col + p["input_cols"])); col += p["input_cols"]
    out_c = list(range(col, col + (per + 1) // 2)); col += (per + 1) // 2
    ctr_c = col; col += 1
    assert col - first_col == evm_step_columns(p)
    adv = c.advice_col
    q_step = adv(q_step_c)
    enable = q_usable * q_step
    odd = adv(odd_c)
    cond_cells = [(cc, r) for cc in cond_c for r in (0, 1)]
    in_cells = [(ic, r) for ic in in_c for r in (0, 1)]
    out_cells = [(oc, r) for oc in out_c for r in (0, 1)][:per]
    cell = lambda cr: adv(cr[0], cr[1])
    # booleanity and one-hot of the selector bits, booleanity of the condition bits
    for b_ in [adv(pc) for pc in pair_c] + [odd] + [cell(cr) for cr in cond_cells]:
        c.add_gate(enable * (b_ * (1 - b_)))
    tot = adv(pair_c[0])
    for pc in pair_c[1:]:
        tot = tot + adv(pc)
    c.add_gate(enable * (tot - 1))
    spec = {"q_step": q_step_c, "pair": pair_c, "odd": odd_c, "cond": cond_cells, "in": in_cells, "out": out_cells, "ctr": ctr_c, "states": []}
    for s_ in range(ns):
        sel = adv(pair_c[s_ // 2]) * (odd if s_ % 2 else (1 - odd))
        delta = 1 + s_ % 5
        c.add_gate(enable * sel * (adv(ctr_c, 2) - adv(ctr_c) - delta))
        cons = []
        for j in range(per):
            if j % 8 == 0:      # a new gadget block: its condition (shared by the block's constraints)
                nc = (j // 8 + s_) % 3
                cc_ = rng.sample(range(len(cond_cells)), nc)
            a_, b_, c_, d_ = (rng.randrange(len(in_cells)) for _ in range(4))
            if j % 8 == 3 and cons:                # reuses the product a*b of the block's first constraint (what a gadget's cached expressions look like)
                a_, b_ = cons[j - 3]["in"][0], cons[j - 3]["in"][1]
            form = j % 8
            sel_bit = rng.randrange(len(cond_cells))
            a, b, cx, dx, o = cell(in_cells[a_]), cell(in_cells[b_]), cell(in_cells[c_]), cell(in_cells[d_]), cell(out_cells[j])
            if form == 0: e = a * b + cx - o
            elif form == 1: e = a + b * 256 + cx * 65536 - o
            elif form == 2: e = a * b * cx - o
            elif form == 3: e = a * b * dx - o
            elif form == 4: e = cell(cond_cells[sel_bit]) * a + (1 - cell(cond_cells[sel_bit])) * b - o
            elif form == 5: e = a * (b + cx) - o
            elif form == 6: e = a - b + 255 - o
            else: e = a * a + b - o
            if cc_:
                cnd = cell(cond_cells[cc_[0]])
                for x in cc_[1:]:
                    cnd = cnd * cell(cond_cells[x])
                e = e * cnd
            c.add_gate(enable * sel * e)
            cons.append({"form": form, "in": (a_, b_, c_, d_), "sel_bit": sel_bit, "cond": list(cc_)})
        spec["states"].append({"delta": delta, "cons": cons})
    return spec


def evm_witness(spec: dict, n: int, u: int, seed: int = 3):
    """a satisfying assignment of the block's columns: {column: uint64 array of n canonical values}, and the q_usable column.
    Steps on the even rows below u - 4 with a random execution state each; inputs are bytes, outputs what the step's state defines
    them to be where the gadget's condition holds and arbitrary bytes where it does not."""
    rng = np.random.default_rng(seed)
    rows = np.arange(0, u - 4, 2)
    ns = len(spec["states"])
    state = rng.integers(0, ns, size=rows.size)
    cols = {}
    z = lambda: np.zeros(n, dtype=np.uint64)
    q_usable = z(); q_usable[:rows[-1] + 2] = 1
    cols[spec["q_step"]] = z(); cols[spec["q_step"]][rows] = 1
    for j, pc in enumerate(spec["pair"]):
        cols[pc] = z(); cols[pc][rows[state // 2 == j]] = 1
    cols[spec["odd"]] = z(); cols[spec["odd"]][rows] = (state % 2).astype(np.uint64)
    getc = lambda cidx: cols[cidx] if cidx in cols else cols.setdefault(cidx, z())
    cval = {}
    for (cc, r) in spec["cond"]:
        v = rng.integers(0, 2, size=rows.size, dtype=np.uint64)
        getc(cc)[rows + r] = v
        cval[(cc, r)] = v
    ival = {}
    for (ic, r) in spec["in"]:
        v = rng.integers(0, 256, size=rows.size, dtype=np.uint64)
        getc(ic)[rows + r] = v
        ival[(ic, r)] = v
    delta = np.array([st["delta"] for st in spec["states"]], dtype=np.uint64)
    ctr = np.concatenate([[0], np.cumsum(delta[state])]).astype(np.uint64)       # one more cell: the last step's "next"
    getc(spec["ctr"])[np.concatenate([rows, [rows[-1] + 2]])] = ctr
    garbage = rng.integers(0, 256, size=(len(spec["out"]), rows.size), dtype=np.uint64)
    for s_, st in enumerate(spec["states"]):
        m = np.flatnonzero(state == s_)          # the steps in state s_; an operand is gathered once per state, not once per constraint
        rows_m, iv, cv = rows[m], {}, {}
        inp = lambda i: iv[i] if i in iv else iv.setdefault(i, ival[spec["in"][i]][m])
        cnd = lambda x: cv[x] if x in cv else cv.setdefault(x, cval[spec["cond"][x]][m])
        for j, cn in enumerate(st["cons"]):
            a, b, cx, dx = (inp(i) for i in cn["in"])
            f = cn["form"]
            if f == 0: o = a * b + cx
            elif f == 1: o = a + b * np.uint64(256) + cx * np.uint64(65536)
            elif f == 2: o = a * b * cx
            elif f == 3: o = a * b * dx
            elif f == 4: sb = cnd(cn["sel_bit"]); o = sb * a + (np.uint64(1) - sb) * b
            elif f == 5: o = a * (b + cx)
            elif f == 6: o = a + np.uint64(255) - b
            else: o = a * a + b
            holds = np.ones(o.size, dtype=bool)
            for x in cn["cond"]:
                holds &= cnd(x) == 1
            o = np.where(holds, o, garbage[j][m])
            oc, r = spec["out"][j]
            getc(oc)[rows_m + r] = o
    return cols, q_usable


def build_shape(ctx, k: int, A: int, F: int, P: int, L: int, d: int, distinct: int = 8, seed: int = 1, dist: str = None, phases: bool = False, evm: dict = None):
    """SURVEY 8d config 4 stand-in: a circuit with the SuperCircuit's *shape* (A advice, F fixed,
    P permutation columns, L lookups, max degree d).  Same ingredients as `build_large`; to keep
    the host side small only `distinct` advice triples hold distinct data (the other triples
    alias them -- same gates, same witness, separate columns / commitments on the device) and the
    selector classes share their content.  Returns (circuit shell, blob as a uint8 array,
    advice arrays, instance arrays, instance ints).

    dist -- the witness's value distribution:
      "small"   every cell below 2^60, two thirds of them zero (rounds 1-3)
      "survey"  SURVEY 8d's witness-like columns: ~60 % zero / ~30 % below 2^16 / 10 % uniform field elements PER CELL
      "dense"   a third of the cells uniform field elements (the row of every 3-row region that no constraint reads)
    phases -- the SuperCircuit's three advice phases [REF zkevm-circuits/src/util.rs:120-133]: `evm_word`, `keccak_input` usable after
      the first phase, `lookup_input` after the second; as in the EVM circuit [REF zkevm-circuits/src/evm_circuit/execution.rs:418-431]
      ~8 % of the columns are third-phase and a handful second-phase.  The last two advice columns are RLCs that need the challenges:
      w = q_lk * (a_0 + evm_word * b_0) (second phase), t = q_lk * (w + lookup_input * b_0) (third phase); the caller computes them
      between the phases (`phase_columns`).  With phases the function returns a sixth value: that callback's ingredients.
    evm -- parameters of an EVM-style block (`evm_block`, EVM_DEFAULT): evm_step_columns(evm) of the A advice columns become the step
      columns of an execution-state machine whose >= 5 000 constraints of degree 5 .. 9 read them at rotations 0 / 1 / 2 -- every one of
      them on all 8 cosets --; the other columns keep the triple gates, and the lookups become 4- / 6- / 8-column tuples (three
      neighbouring triples' a, b, c on a lookup row, into (t_a, t_b, t_c) repeated).  The adverse degree structure of the two shapes
      (round-5 review: the plain shape has ONE degree-9 gate on three columns)."""
    import struct
    rng = np.random.default_rng(seed)
    if dist is None:
        dist = "dense" if os.environ.get("ZK_BENCH_DENSE") == "1" else "small"
    assert dist in ("small", "survey", "dense")
    vbits = 8 if dist == "survey" else 30            # operand size: products below 2^16 / 2^60
    n_step = evm_step_columns(evm) if evm else 0
    groups = (A - 2 - n_step) // 3 if phases else (A - n_step) // 3
    S = max(1, (F - (6 if evm else 4)) // 2)       # selector classes: q_mul[j], q_add[j]
    assert F >= 2 * S + (6 if evm else 4) and groups >= (3 if evm else 1) and d >= 5 and P >= 2
    c = plonk.Circuit(k, num_fixed=F, num_advice=A, num_instance=1, blinding_factors=5)
    c.fixed = None                                  # fixed columns live in the blob only (numpy), not as Python ints
    n, u = c.n, c.u
    q_hi, q_lk, t_a, t_b = (c.fixed_col(2 * S + i) for i in range(4))
    for g in range(groups):
        a, b_, cc = (c.advice_col(3 * g + i) for i in range(3))
        c.add_gate(c.fixed_col(2 * (g % S)) * (a * b_ - cc))
        c.add_gate(c.fixed_col(2 * (g % S) + 1) * (a + b_ - cc.rot(1)))
        if os.environ.get("ZK_BENCH_SHARED") == "1":      # gates that reuse the products of the first one (what an EVM-style circuit is full of)
            c.add_gate((c.fixed_col(2 * (g % S)) * (a * b_ - cc)) * (a * b_ + 3))
            c.add_gate(c.fixed_col(2 * (g % S)) * ((a * b_ - cc) * (a * b_ - cc)) * (a * b_ + 5))
    a0, b0, c0 = c.advice_col(0), c.advice_col(1), c.advice_col(2)
    hi = q_hi * (a0 * a0 + b0 - c0.rot(-1))          # degree 3, then one linear factor per extra degree
    for i in range(d - 3):
        hi = hi * ((a0 if i % 2 == 0 else b0) + (i + 1))
    c.add_gate(hi)
    if phases:
        c.advice_phase = [2 if col % 12 == 11 else (1 if col % 150 == 7 else 0) for col in range(A)]
        c.advice_phase[A - 2], c.advice_phase[A - 1] = 1, 2
        evm_word, keccak_input = c.challenge_usable_after(0), c.challenge_usable_after(0)
        lookup_input = c.challenge_usable_after(1)
        w_, t_ = c.advice_col(A - 2), c.advice_col(A - 1)
        c.add_gate(q_lk * (a0 + evm_word * b0 - w_))                       # selector-gated: the blinding rows of w and t are free
        c.add_gate(q_lk * (w_ + lookup_input * b0 + keccak_input * 0 - t_))
    evm_spec = None
    if evm:
        q_usable, t_c = c.fixed_col(2 * S + 4), c.fixed_col(2 * S + 5)
        evm_spec = evm_block(c, 3 * groups, q_usable, evm)
    for j in range(L):
        g = j % groups
        if evm:      # tuples of 4 / 6 / 8 cells: a, b, c of this triple and of its neighbours, all holding (i, i^2 + 3, 7 i + 1) of ONE i on a lookup row
            width = (4, 6, 8)[j % 3]
            cells = [c.advice_col(3 * ((g + t) % groups) + i) for t in range(3) for i in range(3)][:width]
            c.add_lookup([q_lk * x for x in cells], [(t_a, t_b, t_c)[i % 3] for i in range(width)])
        else:
            c.add_lookup([q_lk * c.advice_col(3 * g), q_lk * c.advice_col(3 * g + 1)], [t_a, t_b])
    for col in range(min(P - 1, A)):
        c.enable_equality(plonk.ADVICE, col)
    c.enable_equality(plonk.INSTANCE, 0)
    assert c.degree() == d, (c.degree(), d)
    nreg = (u - 4) // 3
    kinds = rng.integers(0, 4, size=nreg)
    rows = 1 + 3 * np.arange(nreg)
    r_mul, r_add, r_hi, r_lk = rows[kinds == 0], rows[kinds == 1], rows[kinds == 2] + 1, rows[kinds == 3]
    tab_n = min(250 if dist == "survey" else 4096, u)          # survey: table values i, i^2 + 3 below 2^16
    ti = np.arange(tab_n, dtype=np.uint64)
    D = min(distinct, groups)
    data = np.zeros((D, 3, n), dtype=np.uint64)
    npairs = min(256, r_mul.size // 2)
    src, dst = r_mul[0:2 * npairs:2], r_mul[1:2 * npairs:2]
    for t in range(D):
        x = rng.integers(0, 1 << vbits, size=r_mul.size, dtype=np.uint64)
        y = rng.integers(0, 1 << vbits, size=r_mul.size, dtype=np.uint64)
        data[t, 0, r_mul], data[t, 1, r_mul], data[t, 2, r_mul] = x, y, x * y
        x = rng.integers(0, 1 << vbits, size=r_add.size, dtype=np.uint64)
        y = rng.integers(0, 1 << vbits, size=r_add.size, dtype=np.uint64)
        data[t, 0, r_add], data[t, 1, r_add], data[t, 2, r_add + 1] = x, y, x + y
        if not (evm and t):
            i = rng.integers(1, tab_n, size=r_lk.size, dtype=np.uint64)   # every triple may be a lookup input (evm: the SAME i in every triple of a row -- the tuples span triples)
        data[t, 0, r_lk], data[t, 1, r_lk] = i, i * i + 3
        if evm:
            data[t, 2, r_lk] = i * np.uint64(7) + np.uint64(1)
        # copy pairs (product of a mul row feeds `a` of the next one), same pattern in every triple
        data[t, 0, dst] = data[t, 2, src] % np.uint64(1 << vbits)
        data[t, 2, src] = data[t, 0, dst]
        data[t, 0, src], data[t, 1, src] = data[t, 2, src], 1
        data[t, 2, dst] = data[t, 0, dst] * data[t, 1, dst]
    # the degree-d gate lives on triple 0: rows r_hi hold (x, y) with c[row-1] = x^2 + y
    x = rng.integers(0, 1 << min(20, vbits), size=r_hi.size, dtype=np.uint64)
    y = rng.integers(0, 1 << min(20, vbits), size=r_hi.size, dtype=np.uint64)
    data[0, 0, r_hi], data[0, 1, r_hi], data[0, 2, r_hi - 1] = x, y, x * x + y
    copies = []
    for g in range(groups):
        if 3 * g + 2 < min(P - 1, A):
            copies += [((plonk.ADVICE, 3 * g + 2, int(s_)), (plonk.ADVICE, 3 * g, int(d_))) for s_, d_ in zip(src, dst)]
    inst = np.zeros((1, n), dtype=np.uint64)
    pub = r_add[:4]
    inst[0, :pub.size] = data[0, 1, pub]
    copies += [((plonk.ADVICE, 1, int(r0)), (plonk.INSTANCE, 0, j)) for j, r0 in enumerate(pub)]
    c.copies = copies
    data_m = [[to_mont_gpu(ctx, small_to_limbs(data[t, i])) for i in range(3)] for t in range(D)]
    if dist in ("dense", "survey"):
        # field-sized cells: the third row of every 3-row region is read by no constraint.  "dense" fills it (one row in three of
        # every column) with uniform field elements; "survey" fills 30 % of those rows, i.e. 10 % of all cells, chosen cell by cell
        free = rows + 2
        for t in range(D):
            for i in range(3):
                pick = free if dist == "dense" else free[rng.random(free.size) < 0.30]
                limbs = rng.integers(0, 1 << 63, size=(pick.size, 4), dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=(pick.size, 4), dtype=np.uint64)
                limbs[:, 3] &= np.uint64((1 << 60) - 1)
                data_m[t][i][pick] = limbs
    zero_col = np.zeros((n, 4), dtype=np.uint64)
    adv_m = [data_m[(col // 3) % D][col % 3] if col < 3 * groups else zero_col for col in range(A)]
    # the same witness as the integers it was made from (--typed), for the columns that hold nothing else: "small" cells only, no
    # column that a phase computes from a challenge, no step column of the EVM block (those are converted further down)
    zero_ints = np.zeros(n, dtype=np.uint64)
    c.advice_ints = [None] * A
    if dist == "small":
        for col in range(A - 2 if phases else A):
            c.advice_ints[col] = data[(col // 3) % D, col % 3] if col < 3 * groups else (None if evm and col < 3 * groups + n_step else zero_ints)
    f_usable = f_tc = zero_col
    if evm:
        step_cols, usable = evm_witness(evm_spec, n, u, seed + 2)
        for col, v in step_cols.items():
            adv_m[col] = to_mont_gpu(ctx, small_to_limbs(v))
        f_usable = to_mont_gpu(ctx, small_to_limbs(usable))
        tc = np.zeros(n, dtype=np.uint64); tc[1:tab_n] = ti[1:] * np.uint64(7) + np.uint64(1)
        f_tc = to_mont_gpu(ctx, small_to_limbs(tc))
    inst_m = [to_mont_gpu(ctx, small_to_limbs(inst[0]))]

    def sel(rows_):
        v = np.zeros(n, dtype=np.uint64)
        v[rows_] = 1
        return to_mont_gpu(ctx, small_to_limbs(v))
    f_mul, f_add, f_hi, f_lk = sel(r_mul), sel(r_add), sel(r_hi), sel(r_lk)
    ta = np.zeros(n, dtype=np.uint64); ta[1:tab_n] = ti[1:]
    tb = np.zeros(n, dtype=np.uint64); tb[1:tab_n] = ti[1:] * ti[1:] + 3
    f_ta, f_tb = to_mont_gpu(ctx, small_to_limbs(ta)), to_mont_gpu(ctx, small_to_limbs(tb))
    fixed_of = lambda i: (f_mul if i % 2 == 0 else f_add) if i < 2 * S else ([f_hi, f_lk, f_ta, f_tb, f_usable, f_tc][i - 2 * S] if i < 2 * S + 6 else zero_col)
    blob = assemble_blob(ctx, c, F, fixed_of, copies)
    inst_int = [[int(v) for v in inst[0]]]
    if phases:
        return c, blob, adv_m, inst_m, inst_int, {"q_lk": f_lk, "a0": adv_m[0], "b0": adv_m[1], "w": A - 2, "t": A - 1}
    return c, blob, adv_m, inst_m, inst_int


def cell_distribution(adv_m, sample_cols: int = 24):
    """share of zero / below-2^16 / larger cells over a sample of the witness columns (Montgomery images: zero stays zero, the
    image of a small value is judged through the device-free inverse map on a row sample)"""
    from zkevm_circuits_amd import plonk as _p
    rinv = pow(1 << 256, -1, R)
    zero = small = total = 0
    step = max(1, len(adv_m) // sample_cols)
    for col in adv_m[::step]:
        a = np.asarray(col).reshape(-1, 4)
        rows_ = np.arange(0, a.shape[0], max(1, a.shape[0] // 4096))
        for r_ in rows_:
            v = int(a[r_, 0]) | int(a[r_, 1]) << 64 | int(a[r_, 2]) << 128 | int(a[r_, 3]) << 192
            total += 1
            if v == 0:
                zero += 1
            elif v * rinv % R < (1 << 16):
                small += 1
    return {"zero": round(zero / total, 3), "below_2^16": round(small / total, 3), "larger": round(1 - (zero + small) / total, 3), "cells_sampled": total}


def owned_columns(circ, rank: int, world: int) -> set:
    """advice columns rank `rank` of a `world`-rank sharded session owns: position j of each phase's columns (ascending column
    index), j % world == rank -- the rule of zk_proof_advice_phase_dev (include/zkmi355.h)"""
    out = set()
    for ph in range(circ.num_phases()):
        cols = [i for i in range(circ.A) if circ.advice_phase[i] == ph]
        out.update(cols[rank::world])
    return out


class PhaseDriver:
    """The host side of a three-phase proof over device-resident witness columns: what the Rust shim does by calling
    `Circuit::synthesize` once per phase [REF zkevm-circuits/src/super_circuit.rs:728-736], here with the two challenge-dependent
    columns computed on the device between the phases (w = q_lk (a_0 + evm_word b_0), t = q_lk (w + lookup_input b_0)).
    adv_dev: list or {column: DeviceBuffer}.  owned (sharded sessions): the columns this rank hands over; the others go in as None
    and arrive from their owner (a_0, b_0, w, t are held by every rank: the two RLC columns are recomputed everywhere)."""

    def __init__(self, ctx, circ, adv_dev, rlc, in_place=True, owned=None):
        self.ctx, self.circ, self.rlc, self.in_place, self.owned = ctx, circ, rlc, in_place, owned
        self.adv = adv_dev if isinstance(adv_dev, dict) else dict(enumerate(adv_dev))
        self.n = circ.n
        self.q = ctx.to_device(rlc["q_lk"])
        self.tmp = ctx.alloc(self.n * 32)

    def _rlc(self, base_col, ch_mont, out_col):
        """out = q_lk * (base + ch * b_0), all on the device"""
        ctx, n = self.ctx, self.n
        FR, ADD, MUL = 0, 0, 2
        ctx.field_vec_op(FR, ADD, self.adv[1], self.zero(), self.tmp, n)       # tmp = b_0
        ctx.fr_scale(self.tmp, ch_mont, n)                                       # tmp = ch * b_0
        ctx.field_vec_op(FR, ADD, self.tmp, self.adv[base_col], self.tmp, n)
        ctx.field_vec_op(FR, MUL, self.tmp, self.q, self.adv[out_col], n)

    def zero(self):
        if not hasattr(self, "_zero"):
            self._zero = self.ctx.to_device(np.zeros((self.n, 4), dtype=np.uint64))
        return self._zero

    def run(self, sess, before_phase=None):
        """three advice phases of `sess`; returns the challenges.  before_phase(p): called ahead of phase p (sharding.EmulatedRank)"""
        phase_of = self.circ.advice_phase
        mine = lambda i: self.owned is None or i in self.owned
        cols = lambda ph: {i: (self.adv[i] if mine(i) else None) for i in range(self.circ.A) if phase_of[i] == ph}
        hook = before_phase or (lambda p_: None)
        hook(0)
        ch0 = sess.advice_phase_dev(cols(0), in_place=self.in_place)      # evm_word, keccak_input
        self._rlc(0, ch0[0], self.rlc["w"])
        hook(1)
        ch1 = sess.advice_phase_dev(cols(1), in_place=self.in_place)      # lookup_input
        self._rlc(self.rlc["w"], ch1[0], self.rlc["t"])
        hook(2)
        sess.advice_phase_dev(cols(2), in_place=self.in_place)
        return list(ch0) + list(ch1)

    def free(self):
        for b_ in (self.q, self.tmp, getattr(self, "_zero", None)):
            if b_ is not None:
                b_.free()


def narrowest_cells(ints: np.ndarray) -> np.ndarray:
    """a column of integers below 2^64 in the narrowest cell type that holds every value (ProofSession.advice_phase_typed)"""
    top = int(ints.max()) if ints.size else 0
    return ints.astype(next(dt for bits, dt in ((8, np.uint8), (16, np.uint16), (32, np.uint32), (64, np.uint64)) if top < 1 << bits))


def proof_bench(ctx, k, circ, blob, adv_m, inst_m, inst, shplonk=True, repeat=3, verify=True, pinned=False, t_build=0.0,
                session_hook=None, barrier=None, report=True, world=1, transcript_kind=None, profiled_extra=False, resident=False, typed=False):
    """keygen_pk + `repeat` proving sessions of one circuit; returns the result record (None on
    ranks that do not report).  Verified afterwards by the oracle's pairing verifier.
    resident: the witness columns are uploaded BEFORE the sessions (one device buffer per column) and handed over as device
    pointers (zk_proof_advice_phase_dev): inputs resident in HBM when the timed region starts."""
    # halo2 hands create_proof the public inputs themselves, not an n-row column: keep the slice that
    # holds them (the rest of the column is zero) so the transcript absorbs a handful of scalars
    npub = [int(np.flatnonzero(np.asarray(a).reshape(-1, 4).any(axis=1))[-1]) + 1 if np.asarray(a).any() else 0 for a in inst_m]
    inst = [list(col[:m]) for col, m in zip(inst, npub)]
    inst_m = [np.ascontiguousarray(a[:m]) for a, m in zip(inst_m, npub)]
    if typed:           # every column the generator knows as integers goes over in its narrowest cell type; the others stay Montgomery
        ints = getattr(circ, "advice_ints", None) or [None] * len(adv_m)
        narrow = {}
        for v in ints:
            if v is not None and id(v) not in narrow:
                narrow[id(v)] = narrowest_cells(v)
        adv_m = [a if v is None else narrow[id(v)] for a, v in zip(adv_m, ints)]
    if pinned:          # what a host integration would do: witness columns in page-locked memory
        pin = {}
        for a in adv_m:
            if id(a) not in pin:
                pin[id(a)] = ctx.host_alloc(a.shape, a.dtype)
                pin[id(a)][:] = a
        adv_m = [pin[id(a)] for a in adv_m]
    S = 0x5EC2E7
    s_mont = np.frombuffer(plonk.fr_mont_bytes(S), dtype=np.uint64).copy()
    t0 = time.perf_counter()
    srs = ctx.srs_setup_with_s(k, s_mont)
    ctx.sync()
    t_srs = time.perf_counter() - t0
    t0 = time.perf_counter()
    pk = ctx.pk_create(srs, blob)
    ctx.sync()
    t_keygen = time.perf_counter() - t0
    times = []
    proof = b""
    adv_dev = [ctx.to_device(a) for a in adv_m] if resident else None
    if resident:
        ctx.sync()
    for it in range(repeat + (1 if profiled_extra else 0)):
        if it == repeat:            # one more proof with the per-scope HIP events on (not timed: the events cost host time)
            ctx.prof_reset()
            ctx.prof_enable(True)
        t0 = time.perf_counter()
        if barrier:
            barrier()
            t0 = time.perf_counter()
        sess = ctx.proof_session(pk, inst_m, bytes(16), instance_slices=True)
        if transcript_kind is not None:
            sess.set_transcript_kind(transcript_kind)
        sess.set_multiopen(1 if shplonk else 0)
        keep = session_hook(sess) if session_hook else None
        if resident:
            sess.advice_phase_dev({i: c for i, c in enumerate(adv_dev)}, in_place=True)
        elif typed:
            sess.advice_phase_typed({i: c for i, c in enumerate(adv_m)})
        else:
            sess.advice_phase({i: c for i, c in enumerate(adv_m)})
        proof = sess.finish()
        del keep
        if barrier:
            barrier()
        if it < repeat:
            times.append(time.perf_counter() - t0)
        else:
            ctx.prof_enable(False)
    if adv_dev:
        for b_ in adv_dev:
            b_.free()
    if not report:
        pk.destroy(); srs.destroy()
        return None
    ok = None
    if verify:
        from oracle import cref, pairing as pr, plonk_verifier as pv
        com, rep = pk.vk(circ.F + len(circ.perm_cols))
        kinds = {None: "blake2b", 0: "blake2b", 1: "poseidon", 2: "evm"}
        ok = bool(pv.verify(circ, cref.affine_from_mont(com), cref.from_mont(rep.reshape(1, 4))[0], inst, proof, pr.ec_mul(pr.G2_GEN, S),
                            multiopen="shplonk" if shplonk else "gwc", transcript=kinds[transcript_kind]))
    pk.destroy(); srs.destroy()
    d = circ.degree()
    extra = {}
    if typed:           # what crosses PCIe per proof: the usable rows of every column at its cell width, plus the blinding rows
        cell = [z.binding.typed_cell_width(a) for a in adv_m]
        extra = {"typed_columns_by_cell_bytes": {str(w): cell.count(w) for w in sorted(set(cell))},
                 "witness_upload_bytes": sum(circ.u * w + (circ.n - circ.u) * 32 for w in cell), "witness_upload_bytes_as_fr": len(cell) * circ.n * 32}
        if profiled_extra:
            extra["fr_from_uint_ms"] = round(ctx.prof_get("fr_from_uint")[0], 3)
    return {**extra,
        "metric": "synthetic-shape full proof wall-clock (s), 1x MI355X",
        "value": round(min(times), 4), "unit": "s", "higher_is_better": False,
        "k": k, "advice": circ.A, "fixed": circ.F, "instance": circ.I, "permutation_columns": len(circ.perm_cols),
        "lookups": len(circ.lookups), "gates": len(circ.gates), "degree": d, "extended_k": circ.extended_k(),
        "advice_queries": len(circ.advice_queries), "fixed_queries": len(circ.fixed_queries), "blinding_factors": circ.bf,
        "proof_bytes": len(proof), "create_proof_s": [round(t, 4) for t in times], "keygen_pk_s": round(t_keygen, 4),
        "srs_setup_s": round(t_srs, 4), "host_circuit_build_s": round(t_build, 2), "verified_by_oracle": ok,
        "msm_count": circ.A + 2 * len(circ.lookups) + (len(circ.perm_cols) + d - 3) // (d - 2) + 1 + (d - 1) + (2 if shplonk else 0),
        "multiopen": "shplonk" if shplonk else "gwc", "data": "synthetic-shape",
        "witness_residency": "HBM (zk_proof_advice_phase_dev)" if resident else ("page-locked host memory" if pinned else "pageable host memory"), "n_gpus": world,
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, default=16)
    ap.add_argument("--groups", type=int, default=10)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--no-verify", action="store_true")
    ap.add_argument("--large", action="store_true", help="vectorised builder (k >= 18, many columns)")
    ap.add_argument("--shplonk", action="store_true", help="SHPLONK multi-open instead of GWC")
    ap.add_argument("--host-upload", action="store_true", help="sharded runs: every rank uploads every advice column (no device all-gather)")
    ap.add_argument("--rccl", action="store_true", help="sharded runs: exchange through the library's own RCCL communicator (zk_comm_init) instead of torch.distributed callbacks")
    ap.add_argument("--pinned", action="store_true", help="advice columns in page-locked host memory (zk_host_alloc)")
    ap.add_argument("--typed", action="store_true", help="with --pinned: advice columns whose generated values are all below 2^64 go over as integers of "
                    "their narrowest cell width (zk_proof_advice_phase_typed) instead of 32-byte Montgomery elements")
    ap.add_argument("--cpu-baseline", action="store_true", help="time the C oracle's MSM / NTT at 2^k on the host and scale by the prover's counts")
    ap.add_argument("--keccak", action="store_true", help="Keccak-circuit stand-in (SURVEY 8d config 3): 59 unusable rows, 13-rotation gates, degree 9")
    ap.add_argument("--shape", default="", help="A,F,P,L,d: circuit with this many advice / fixed / permutation columns, lookups and "
                    "max degree (SURVEY 8d config 4 stand-in: 1000,150,150,100,9)")
    args = ap.parse_args()

    # multi-GPU: launched with `python -m torch.distributed.run --nproc-per-node N bench_proof.py ...`
    # -> one rank per GPU, sharded proving session (zk_proof_set_sharding), rank 0 reports.
    world, rank, shard = int(os.environ.get("WORLD_SIZE", "1")), int(os.environ.get("RANK", "0")), None
    device = 0
    dist = None
    if world > 1 and args.rccl:
        # the library's own communicator, joined from the launcher's environment: no torch in a prover rank
        from zkevm_circuits_amd import rendezvous
        device = int(os.environ.get("LOCAL_RANK", "0"))
    elif world > 1:
        import torch
        import torch.distributed as dist
        from zkevm_circuits_amd import sharding as shard
        device = int(os.environ.get("LOCAL_RANK", "0")) % max(torch.cuda.device_count(), 1)
        torch.cuda.set_device(device)
        # fewer GPUs than ranks (single-GPU test box): ranks share a device and exchange over gloo
        dist.init_process_group(backend="nccl" if torch.cuda.device_count() >= world else "gloo")
    ctx = z.Context(device)
    t0 = time.perf_counter()
    if args.keccak:
        circ, blob, adv_m, inst_m, inst = build_keccak_shape(ctx, args.k)
    elif args.shape:
        sa, sf, sp, sl, sd = (int(v) for v in args.shape.split(","))
        circ, blob, adv_m, inst_m, inst = build_shape(ctx, args.k, sa, sf, sp, sl, sd)
    elif args.large:
        circ, blob, adv_m, inst_m, inst = build_large(ctx, args.k, args.groups)
    else:
        circ, adv, inst = build(args.k, args.groups)
        blob = circ.blob()
        adv_m = [plonk.column_to_mont(c) for c in adv]
        inst_m = [plonk.column_to_mont(c) for c in inst]
    t_build = time.perf_counter() - t0
    hook = None
    barrier = None
    if world > 1 and args.rccl:
        rendezvous.comm_init_from_env(ctx)
        hook = lambda sess: sess.set_sharding_comm()
        barrier = lambda: rendezvous.comm_barrier(ctx, rank, world)
    elif world > 1:    # device all-gather of the advice columns unless --host-upload asks every rank to upload everything
        hook = (lambda sess: shard.shard_session(sess)) if args.host_upload else (lambda sess: shard.shard_session_device(sess))
    out = proof_bench(ctx, args.k, circ, blob, adv_m, inst_m, inst, shplonk=args.shplonk, repeat=args.repeat, verify=not args.no_verify, pinned=args.pinned,
                      t_build=t_build, session_hook=hook, barrier=barrier or (dist.barrier if world > 1 else None), report=(rank == 0), world=world,
                      **({"typed": True, "profiled_extra": True} if args.typed and args.pinned else {}))
    if world > 1 and rank != 0:
        if dist is not None:
            dist.destroy_process_group()
        return
    d = circ.degree()
    if args.cpu_baseline:
        # The reference prover (Rust / Rayon) cannot be built here, and the oracle has no full prover
        # at this size.  What can be timed on the host is what dominates halo2's create_proof: one
        # best_multiexp and one best_fft of size 2^k in the C / OpenMP restatement, times the number
        # of each the prover performs for this shape.  Quotient evaluation, the running products and
        # witness synthesis are left out, so the figure is a LOWER bound for the restated CPU prover.
        from oracle import bn254, cref
        n = 1 << args.k
        sc, bases = cref.rand_fr_stream(7, n), cref.srs_powers(3, min(n, 1 << 12))
        bases = np.ascontiguousarray(np.tile(bases, (n // bases.shape[0], 1)))
        t0 = time.perf_counter()
        cref.best_multiexp(sc, bases, cref.usable_cpus())
        t_msm = time.perf_counter() - t0
        t0 = time.perf_counter()
        cref.best_fft(sc, bn254.omega_for_k(args.k), args.k)
        t_ntt = time.perf_counter() - t0
        cosets = 1 << (circ.extended_k() - args.k)
        polys = out["msm_count"] - (d - 1)                       # committed columns: advice, m / phi, Z, random
        ntt_count = polys * (1 + cosets) + cosets               # lagrange_to_coeff + extended cosets, plus h back to coefficients
        out["cpu_baseline"] = {
            "kind": "port-estimate", "cores": cref.usable_cpus(), "msm_s": round(t_msm, 3), "ntt_s": round(t_ntt, 4),
            "msm_count": out["msm_count"], "ntt_count_size_n": ntt_count,
            "estimated_proof_s": round(out["msm_count"] * t_msm + ntt_count * t_ntt, 1),
            "note": "C/OpenMP restatement of best_multiexp / best_fft timed once at 2^k, multiplied by the prover's MSM and "
                    "size-n NTT counts for this shape; excludes quotient evaluation, products and synthesis (lower bound)",
        }
    if world > 1:
        out["metric"] = f"synthetic-shape full proof wall-clock (s), {world} ranks (sharded session)"
        if dist is not None:
            dist.destroy_process_group()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()

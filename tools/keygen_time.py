"""Key generation from a version 3 and from a version 4 key blob of the same circuit, in one process.

The circuit has no gates: F fixed columns (two thirds 0/1 selectors, the rest 16-bit tables but for `--field-columns` columns of
field-sized cells) and P advice columns in the permutation, tied by random 2-cycles as bench_proof.py ties its columns (one cell
in `--copy-every` takes part).  Both blobs are put together here with numpy, the way a caller at this size has to:

  version 3   every fixed column converted to Montgomery form (on the device), every sigma column as delta^j * omega^i from
              zk_fr_powers, downloaded, its copy cycles swapped in on the host
  version 4   fixed cells at their narrowest width, the permutation as the (j', i') mapping -- no field arithmetic

Reported per k as one JSON line: blob bytes and host seconds to build either blob, zk_pk_create wall seconds (a host clock around
the call, device drained before and after; one untimed call of either version first, then `--repeat` timed calls of each,
alternating), whether the two keys' commitments and transcript_repr are equal, and from one more version 4 call under
zk_prof_enable the device time of k_sigma_from_mapping and of the fixed-cell expansion per launch of up to sixteen columns.

usage: python tools/keygen_time.py [--k 18,20] [--fixed 150] [--perm 150] [--repeat 3]"""
import argparse
import ctypes
import json
import os
import struct
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import zkevm_circuits_amd as z  # noqa: E402
from zkevm_circuits_amd import plonk  # noqa: E402

R = plonk.R_MOD


def to_mont(ctx, canon):
    """(n, 4) u64 canonical integers -> Montgomery form, by a Montgomery product with the plain integer R^2 on the device"""
    r2 = np.frombuffer(plonk.fr_mont_bytes((1 << 256) % R), dtype=np.uint64).copy()
    buf = ctx.to_device(np.ascontiguousarray(canon))
    ctx.fr_scale(buf, r2, canon.shape[0])
    out = buf.download(canon.shape)
    buf.free()
    return out


def make_circuit(k, F, P, field_columns, copy_every, seed):
    rng = np.random.default_rng(seed)
    c = plonk.Circuit(k, num_fixed=F, num_advice=P, num_instance=0, shape_only=True)
    n = c.n
    for j in range(P):
        c.enable_equality(plonk.ADVICE, j)
    selectors = F - F // 3
    fixed = []
    for i in range(F):
        if i < selectors:
            fixed.append((rng.random(n) < 0.3).astype(np.uint8))
        elif i < F - field_columns:
            fixed.append(rng.integers(0, 1 << 16, size=n, dtype=np.uint16))
        else:
            limbs = rng.integers(0, 1 << 63, size=(n, 4), dtype=np.uint64)
            limbs[:, 3] >>= np.uint64(2)              # below 2^253 < r: canonical
            fixed.append(limbs)
    # random 2-cycles: distinct cells of the P x n grid, paired in the order drawn
    cells = np.unique(rng.integers(0, P * n, size=max(2, P * n // copy_every), dtype=np.int64))
    rng.shuffle(cells)
    cells = cells[:len(cells) // 2 * 2].reshape(-1, 2)
    return c, fixed, cells


def blob_v3(ctx, c, fixed, pairs):
    n, F, P = c.n, len(fixed), len(c.perm_cols)
    head = c.cs_blob()
    blob = np.empty(len(head) + (F + P) * n * 32, dtype=np.uint8)
    blob[:len(head)] = np.frombuffer(head, dtype=np.uint8)
    off = len(head)
    for col in fixed:
        if col.ndim == 1:
            limbs = np.zeros((n, 4), dtype=np.uint64)
            limbs[:, 0] = col
        else:
            limbs = col
        blob[off:off + n * 32] = to_mont(ctx, limbs).view(np.uint8).reshape(-1)
        off += n * 32
    sigma = np.empty((P * n, 4), dtype=np.uint64)
    omega = np.frombuffer(plonk.fr_mont_bytes(c.omega()), dtype=np.uint64).copy()
    tmp = ctx.alloc(n * 32)
    for j in range(P):
        ctx.fr_powers(omega, np.frombuffer(plonk.fr_mont_bytes(pow(plonk.FR_DELTA, j, R)), dtype=np.uint64).copy(), tmp, n)
        ctx._ck(z.lib().zk_d2h(ctx.h, sigma[j * n:(j + 1) * n].ctypes.data_as(ctypes.c_void_p), ctypes.c_void_p(tmp.ptr), ctypes.c_size_t(n * 32)))
    tmp.free()
    a, b = sigma[pairs[:, 0]].copy(), sigma[pairs[:, 1]].copy()
    sigma[pairs[:, 0]], sigma[pairs[:, 1]] = b, a
    blob[off:] = sigma.view(np.uint8).reshape(-1)
    return blob


def blob_v4(ctx, c, fixed, pairs):
    n, F, P = c.n, len(fixed), len(c.perm_cols)
    head = c.cs_blob(version=4)
    widths = [col.dtype.itemsize if col.ndim == 1 else 32 for col in fixed]
    blob = np.empty(len(head) + 4 * F + n * sum(widths) + 8 * P * n, dtype=np.uint8)
    blob[:len(head)] = np.frombuffer(head, dtype=np.uint8)
    off = len(head)
    blob[off:off + 4 * F] = np.frombuffer(struct.pack(f"<{F}I", *widths), dtype=np.uint8)
    off += 4 * F
    for col, w in zip(fixed, widths):
        blob[off:off + n * w] = (to_mont(ctx, col) if w == 32 else col).view(np.uint8).reshape(-1)
        off += n * w
    mapping = np.empty((P * n, 2), dtype=np.uint32)
    mapping[:, 0] = np.repeat(np.arange(P, dtype=np.uint32), n)
    mapping[:, 1] = np.tile(np.arange(n, dtype=np.uint32), P)
    a, b = mapping[pairs[:, 0]].copy(), mapping[pairs[:, 1]].copy()
    mapping[pairs[:, 0]], mapping[pairs[:, 1]] = b, a
    blob[off:] = mapping.view(np.uint8).reshape(-1)
    return blob


def timed_key(ctx, srs, blob, ncom):
    ctx.sync()
    t0 = time.perf_counter()
    pk = ctx.pk_create(srs, blob)
    ctx.sync()
    dt = time.perf_counter() - t0
    com, rep = pk.vk(ncom)
    key = com.tobytes() + rep.tobytes()
    pk.destroy()
    return dt, key


def run(ctx, k, args):
    c, fixed, pairs = make_circuit(k, args.fixed, args.perm, args.field_columns, args.copy_every, args.seed)
    ncom = args.fixed + args.perm
    srs = ctx.srs_setup_with_s(k, np.frombuffer(plonk.fr_mont_bytes(0x5EC2E7), dtype=np.uint64).copy())
    blobs, build_s = {}, {}
    for version, make in ((3, blob_v3), (4, blob_v4)):
        ctx.sync()
        t0 = time.perf_counter()
        blobs[version] = make(ctx, c, fixed, pairs)
        ctx.sync()
        build_s[version] = time.perf_counter() - t0
    keys = {v: timed_key(ctx, srs, blobs[v], ncom)[1] for v in (3, 4)}         # untimed: first call of either path
    times = {3: [], 4: []}
    for _ in range(args.repeat):
        for v in (3, 4):
            times[v].append(timed_key(ctx, srs, blobs[v], ncom)[0])
    ctx.prof_reset()
    ctx.prof_enable(True)
    timed_key(ctx, srs, blobs[4], ncom)
    ctx.prof_enable(False)
    sig_ms, sig_launches = ctx.prof_get("sigma_from_mapping")
    fu_ms, fu_launches = ctx.prof_get("fr_from_uint_batch")
    print(json.dumps({
        "k": k, "fixed_columns": args.fixed, "permutation_columns": args.perm, "cells_in_copy_cycles": int(pairs.size),
        "fixed_cell_bytes": {str(w): n_ for w, n_ in zip(*np.unique([col.dtype.itemsize if col.ndim == 1 else 32 for col in fixed], return_counts=True))},
        "blob_bytes_v3": int(blobs[3].nbytes), "blob_bytes_v4": int(blobs[4].nbytes),
        "blob_build_s_v3": round(build_s[3], 3), "blob_build_s_v4": round(build_s[4], 3),
        "pk_create_s_v3": [round(t, 4) for t in times[3]], "pk_create_s_v4": [round(t, 4) for t in times[4]],
        "pk_create_s_min_v3": round(min(times[3]), 4), "pk_create_s_min_v4": round(min(times[4]), 4),
        "keys_equal": keys[3] == keys[4],
        "sigma_from_mapping_ms_per_launch": round(sig_ms / max(sig_launches, 1), 4), "sigma_from_mapping_launches": sig_launches,
        "sigma_from_mapping_algorithmic_bytes": ctx.prof_get_bytes("sigma_from_mapping"),
        "fr_from_uint_batch_ms_per_launch": round(fu_ms / max(fu_launches, 1), 4), "fr_from_uint_batch_launches": fu_launches}, default=int), flush=True)
    srs.destroy()
    if keys[3] != keys[4]:
        sys.exit("the two blobs made different keys")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", default="18,20")
    ap.add_argument("--fixed", type=int, default=150)
    ap.add_argument("--perm", type=int, default=150)
    ap.add_argument("--field-columns", type=int, default=6)
    ap.add_argument("--copy-every", type=int, default=16, help="one cell in this many is drawn for a 2-cycle")
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--seed", type=int, default=1)
    args = ap.parse_args()
    ctx = z.Context(0)
    for k in (int(v) for v in args.k.split(",")):
        run(ctx, k, args)
    ctx.close()


if __name__ == "__main__":
    main()

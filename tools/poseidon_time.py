"""ZK_OP_POSEIDON on one device, beside the only route there was before it: zk_host_poseidon_permute_width3 per row on one host
thread, then the upload of the n x 32 B result (zk_h2d).

Dense: head-only calls (d_kinds = NULL) of 2^17 and 2^20 rows from 32-byte cells and from 8-byte cells, capacity column included.  The
host route is timed at 2^14 rows (wall clock, the permutation called through ctypes on consecutive states of one array, then the
upload) and SCALED LINEARLY to the row counts of the op: `host_route_ms_scaled`.  Skewed: 2^17 rows of 31-byte cells under a kinds
column with the final flag, as 1-row messages, as messages of 82 rows, and as one message of 397 rows (a 24 KB contract) in every
workgroup-sized stretch of 1-row messages and in one place only -- what lane-per-message divergence costs.  The cells are random
bytes (32-byte columns random field elements) made on the device by zk_fr_random; one process, nothing else on the device.  A call is
timed with the context's HIP-event timer, the stream drained before (zk_ctx_sync); --warmup untimed calls, then --repeat timed ones.
Prints one JSON line per shape: median, minimum and maximum in ms, rows and permutations per second, field products per second
(828 per permutation; the conversions are not counted) beside the 169 G products/s of tools/ubench.hip, and the booked bytes.  The
first 64 rows of every dense result are compared with the host permutation.

usage: python tools/poseidon_time.py [--repeat 10] [--warmup 2] [--host-log-n 14]"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PRODUCTS = 828
UBENCH_PEAK = 169e9


def timed(ctx, call, warmup, repeat):
    ms = []
    for it in range(warmup + repeat):
        ctx.sync()
        ctx.timer_start()
        call()
        t = ctx.timer_stop_ms()
        if it >= warmup:
            ms.append(t)
    return ms


def summary(ms):
    return {"ms_median": round(statistics.median(ms), 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--host-log-n", type=int, default=14)
    args = ap.parse_args()
    import zkevm_circuits_amd as z
    from oracle import cref
    ctx = z.Context(0)
    device = ctx.device_info()[0].strip()
    key = bytes(range(32))
    lib = z.lib()

    # ---- the host route at 2^host_log_n rows
    hn = 1 << args.host_log_n
    src = [ctx.alloc(hn * 32) for _ in range(3)]
    for j, buf in enumerate(src):
        ctx.fr_random(key, 70 + j, 0, buf, hn)
    states = np.ascontiguousarray(np.stack([buf.download((hn, 4)) for buf in src], axis=1))            # (hn, 3, 4): cap, in0, in1
    work = states.copy()
    base = work.ctypes.data
    host_out = ctx.alloc(hn * 32)
    t0 = time.perf_counter()
    for i in range(hn):
        lib.zk_host_poseidon_permute_width3(ctypes.c_void_p(base + 96 * i))
    t1 = time.perf_counter()
    column = np.ascontiguousarray(work[:, 0, :])
    host_out.upload(column)
    ctx.sync()
    t2 = time.perf_counter()
    host_ms, upload_ms = (t1 - t0) * 1e3, (t2 - t1) * 1e3
    print(json.dumps({"device": device, "shape": "host_route", "rows": hn, "permute_ms": round(host_ms, 2), "upload_ms": round(upload_ms, 3),
                      "us_per_row": round((host_ms + upload_ms) * 1e3 / hn, 3)}), flush=True)
    for buf in src + [host_out]:
        buf.free()

    # ---- dense
    for log_n in (17, 20):
        n = 1 << log_n
        cols = [ctx.alloc(n * 32) for _ in range(3)]                   # a width-w column uses the first n * w bytes
        for j, buf in enumerate(cols):
            ctx.fr_random(key, 70 + j, 0, buf, n)
        out = ctx.alloc(n * 32)
        for width in (32, 8):
            call = lambda: ctx.poseidon(cols[1], width, cols[2], width, n, out, cap=cols[0], cap_width=width)
            ms = timed(ctx, call, args.warmup, args.repeat)
            med = statistics.median(ms)
            res = {"device": device, "shape": f"dense_{width}", "log_n": log_n, "n": n, "timed_calls": args.repeat, "warmup_calls": args.warmup}
            res.update(summary(ms))
            res["hashes_per_s"] = round(n / med * 1e3)
            res["products_per_s"] = round(n * PRODUCTS / med * 1e3)
            res["of_ubench_peak"] = round(n * PRODUCTS / med * 1e3 / UBENCH_PEAK, 3)
            res["booked_bytes"] = n * (3 * width + 32)
            res["host_route_ms_scaled"] = round((host_ms + upload_ms) * n / hn, 1)
            res["host_route_over_op"] = round((host_ms + upload_ms) * n / hn / med, 1)
            if width == 32 and log_n == 17:                            # the same inputs as the host route's first rows (same random streams)
                res["same_as_host_first_rows"] = bool(np.array_equal(out.download((n, 4))[:64], column[:64]))
            print(json.dumps(res), flush=True)
        for buf in cols + [out]:
            buf.free()

    # ---- skewed: 2^17 rows of 31-byte cells under a kinds column, final flag
    n = 1 << 17
    data = ctx.alloc(n * 64)
    ctx.fr_random(key, 80, 0, data, 2 * n)
    lens = ctx.alloc(n * 32)
    ctx.fr_random(key, 81, 0, lens, n)
    out = ctx.alloc(n * 32)
    ones = np.zeros(n, dtype=np.uint8)
    m82 = np.ones(n, dtype=np.uint8)
    m82[::82] = 0
    one397 = np.zeros(n, dtype=np.uint8)
    one397[1000:1000 + 396] = 1                                         # head at 999
    per_group = np.zeros(n, dtype=np.uint8)
    for g in range(0, n - 1024, 1024):                                  # one 397-row message per 1024 rows, the rest 1-row messages
        per_group[g + 1:g + 397] = 1
    for name, kinds in (("kinds_1_row_messages", ones), ("kinds_82_row_messages", m82), ("kinds_one_397_row_message", one397), ("kinds_397_row_message_per_1024_rows", per_group)):
        d_kinds = ctx.to_device(kinds)
        messages = int((kinds == 0).sum())
        call = lambda: ctx.poseidon(data.ptr, 31, data.ptr + 31, 31, n, out, cap=lens, cap_width=8, kinds=d_kinds, final=True)
        ms = timed(ctx, call, args.warmup, args.repeat)
        med = statistics.median(ms)
        res = {"device": device, "shape": name, "n": n, "messages": messages, "longest_message": int(np.diff(np.flatnonzero(np.append(kinds == 0, True))).max()), "timed_calls": args.repeat,
               "warmup_calls": args.warmup}
        res.update(summary(ms))
        res["hashes_per_s"] = round(n / med * 1e3)
        res["products_per_s"] = round(n * PRODUCTS / med * 1e3)
        res["booked_bytes"] = n * (31 + 31 + 8 + 1 + 32)
        print(json.dumps(res), flush=True)
        d_kinds.free()
    ctx.sync()
    ctx.prof_reset()
    ctx.prof_enable(True)
    d_kinds = ctx.to_device(m82)
    ctx.poseidon(data.ptr, 31, data.ptr + 31, 31, n, out, cap=lens, cap_width=8, kinds=d_kinds, final=True)
    prof_ms, prof_calls = ctx.prof_get("fr_poseidon")
    print(json.dumps({"prof_fr_poseidon": {"calls": prof_calls, "ms": round(prof_ms, 4), "bytes": ctx.prof_get_bytes("fr_poseidon")}}), flush=True)
    ctx.prof_enable(False)
    for buf in (data, lens, out, d_kinds):
        buf.free()
    ctx.close()


if __name__ == "__main__":
    main()

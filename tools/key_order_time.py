"""ZK_OP_KEY_SORT and ZK_OP_KEY_ORDER on one device at 2^20 key records, beside the host route a caller had before them:
numpy.lexsort over the 64 key bytes (stable, one thread -- numpy sorts on one), the first differing limb and the difference in numpy,
and the inverse column through the oracle's C batch inversion (cref.batch_invert) -- then it would still have to upload ~50 columns.
A yardstick, not a threshold.

Cases: `rw`, 2^20 realistic RW rows (6 tags, ids below 50, 8 addresses, 4 storage keys, distinct counters, handed over in counter
order; sorted under the full mask and under the mask without bytes 60..63); `random`, 2^20 random records (all 64 passes live).
Every case times key_sort without and with d_sorted, and key_order over the sorted permutation: the inverse alone, every output, and
every output with the state circuit's 50 gathered columns.  For key_sort it also prints the live passes (kept byte positions at
which the records differ, counted on the host) and the time per live pass against the bytes a pass moves (14 n algorithmic: index
and key byte read twice, index written).  One process per case, nothing else on the device.  A call is timed with the context's
HIP-event timer, the stream drained before (zk_ctx_sync); --warmup untimed calls, then --repeat timed ones; the median, minimum and
maximum are printed.  The device's permutation is compared with lexsort's and its inverse column with the host's, all rows.

Without --case this is the driver: it runs every case as a child process of its own under `timeout -k 10 SECONDS`, one after the
other, and stops at the first that fails -- nothing follows a failed step.  Prints one JSON line per case.

usage: python tools/key_order_time.py [--repeat 10] [--warmup 2] [--case rw|random] [--log-n 20] [--step-timeout 300]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

CASES = ("rw", "random")


def records(case, n):
    """(n, 64) uint8"""
    rng = np.random.default_rng(28)
    if case == "random":
        return rng.integers(0, 256, size=(n, 64), dtype=np.uint8)
    keys = np.zeros((n, 64), dtype=np.uint8)
    keys[:, 1] = rng.choice(np.array([1, 2, 3, 4, 5, 9], dtype=np.uint8), size=n)
    keys[:, 5] = rng.integers(0, 50, size=n, dtype=np.uint8)                                  # id below 50: its last byte
    keys[:, 6:26] = rng.integers(0, 256, size=(8, 20), dtype=np.uint8)[rng.integers(0, 8, size=n)]
    keys[:, 27] = rng.integers(0, 4, size=n, dtype=np.uint8)
    storage = rng.integers(0, 256, size=(4, 32), dtype=np.uint8)
    storage[0] = 0
    keys[:, 28:60] = storage[rng.integers(0, 4, size=n)]
    keys[:, 60:64] = (np.arange(1, n + 1, dtype=">u4")).view(np.uint8).reshape(n, 4)          # rw_counter, big-endian, in order
    return keys


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


def run_case(case, log_n, warmup, repeat):
    import key_order_cases as kc
    import zkevm_circuits_amd as z
    from oracle import cref
    ctx = z.Context(0)
    n = 1 << log_n
    keys = records(case, n)
    res = {"device": ctx.device_info()[0].strip(), "case": case, "n": n, "timed_calls": repeat, "warmup_calls": warmup}

    # ---- the host route
    t0 = time.perf_counter()
    perm = np.lexsort(keys.T[::-1]).astype(np.uint32)                   # the last key is the primary one: byte 0
    t1 = time.perf_counter()
    srt = keys[perm]
    limbs = srt.view(">u2").astype(np.int64)                            # (n, 32)
    differs = limbs[1:] != limbs[:-1]
    first = np.where(differs.any(axis=1), differs.argmax(axis=1), 31)
    diff = np.concatenate([[0], (limbs[1:] - limbs[:-1])[np.arange(n - 1), first]])
    t2 = time.perf_counter()
    res.update(host_lexsort_ms=round((t1 - t0) * 1e3, 1), host_first_limb_ms=round((t2 - t1) * 1e3, 1))

    # ---- the ops
    d_keys = ctx.to_device(keys)
    d_perm, d_sorted = ctx.alloc(4 * n), ctx.alloc(64 * n)
    vary = (keys != keys[0]).any(axis=0)
    masks = [("full", None)] + ([("no_counter", kc.NO_COUNTER_MASK)] if case == "rw" else [])
    for name, mask in masks:
        live = int(vary[:60].sum() if mask is not None else vary.sum())
        for tag, target in (("", None), ("_with_sorted", d_sorted)):
            ms = timed(ctx, lambda: ctx.key_sort(d_keys, n, d_perm, mask=mask, sorted_keys=target), warmup, repeat)
            med = statistics.median(ms)
            res[f"key_sort_{name}{tag}"] = dict(summary(ms), live_passes=live, us_per_live_pass=round(med * 1e3 / max(live, 1), 2), pass_bytes=14 * n,
                                                GBps_per_pass=round(14 * n * max(live, 1) / med / 1e6, 1))
        res[f"key_sort_{name}"]["perm_equals_lexsort"] = bool(np.array_equal(d_perm.download(n, np.uint32), perm))
    res["sorted_records_equal"] = bool(np.array_equal(d_sorted.download((n, 64), np.uint8), srt))

    d_inv, d_diff, d_index, d_bits, d_nf = ctx.alloc(32 * n), ctx.alloc(32 * n), ctx.alloc(n), ctx.alloc(5 * n), ctx.alloc(n)
    cols = kc.state_circuit_cols()
    d_cols = [ctx.alloc(width * n) for _, _, width in cols]
    forms = (("inverse_only", {}), ("every_output", dict(diff=d_diff, index=d_index, bits=d_bits, not_first=d_nf)),
             ("every_output_and_50_columns", dict(diff=d_diff, index=d_index, bits=d_bits, not_first=d_nf, cols=[(off, width, buf) for (_, off, width), buf in zip(cols, d_cols)])))
    for name, kw in forms:
        ms = timed(ctx, lambda: ctx.key_order(d_keys, n, d_inv, perm=d_perm, **kw), warmup, repeat)
        res[f"key_order_{name}"] = dict(summary(ms), ns_per_row=round(statistics.median(ms) * 1e6 / n, 3))
    got_index = d_index.download(n, np.uint8)
    res["index_equals_host"] = bool(np.array_equal(got_index[1:], first.astype(np.uint8)))
    got_diff, got_inv = d_diff.download((n, 4)), d_inv.download((n, 4))
    t3 = time.perf_counter()
    safe = got_diff.copy()
    zero = ~safe.any(axis=1)
    safe[zero] = cref.to_mont([1])[0]
    host_inv = cref.batch_invert(safe)
    host_inv[zero] = 0
    t4 = time.perf_counter()
    res.update(host_batch_invert_ms=round((t4 - t3) * 1e3, 1), inverse_equals_host=bool(np.array_equal(host_inv, got_inv)),
               diff_sample_equals_host=bool(cref.from_mont(got_diff[:2000]) == [int(d) % kc.P for d in diff[:2000]]))
    res["host_route_ms"] = round(res["host_lexsort_ms"] + res["host_first_limb_ms"] + res["host_batch_invert_ms"], 1)
    res["device_route_ms"] = round(res["key_sort_full"]["ms_median"] + res["key_order_every_output_and_50_columns"]["ms_median"], 3)
    print(json.dumps(res), flush=True)
    ok = all(v for k, v in res.items() if k.endswith("_host") or k == "sorted_records_equal") and all(res[f"key_sort_{name}"]["perm_equals_lexsort"] for name, _ in masks)
    for buf in (d_keys, d_perm, d_sorted, d_inv, d_diff, d_index, d_bits, d_nf, *d_cols):
        buf.free()
    ctx.close()
    return 0 if ok else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--case", choices=CASES)
    ap.add_argument("--log-n", type=int, default=20)
    ap.add_argument("--step-timeout", type=int, default=300)
    args = ap.parse_args()
    if args.case:
        return run_case(args.case, args.log_n, args.warmup, args.repeat)
    for case in CASES:                                                  # every GPU step under its own time limit; nothing follows a failed one
        cmd = ["timeout", "-k", "10", str(args.step_timeout), sys.executable, os.path.abspath(__file__), "--case", case, "--repeat", str(args.repeat), "--warmup", str(args.warmup),
               "--log-n", str(args.log_n)]
        rc = subprocess.run(cmd).returncode
        if rc != 0:
            print(json.dumps({"case": case, "failed_with_status": rc, "stopped": True}), flush=True)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())

"""The affine scan ops of zk_field_vec_op beside the scan of the same shape that was there before, zk_fr_prefix_product.

For n = 2^20 and 2^24 (--log-sizes): ZK_OP_SCAN_AFFINE, ZK_OP_SCAN_AFFINE_REV and zk_fr_prefix_product on the same random columns
(filled on the device by zk_fr_random), in one process, nothing else on the device.  Every call is timed by itself with the
context's HIP-event timer (zk_timer_start / zk_timer_stop_ms around one call, the stream drained before); --warmup untimed calls of
each, then --repeat timed ones, the three kernels taking turns so that a drift of the clocks meets all of them alike.  Prints one JSON
line per size: median, minimum and maximum in ms, the ratio of the medians to the prefix product's, and the rate of each over its
algorithmic bytes -- n x 96 B for the affine scan (what its zk_prof scope books: a and b read, out written), n x 64 B for the prefix
product.  A last profiled call of each op confirms the scope and its bytes (zk_prof_get / zk_prof_get_bytes).

usage: python tools/scan_time.py [--log-sizes 20,24] [--repeat 20] [--warmup 3]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-sizes", default="20,24")
    ap.add_argument("--repeat", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    assert args.repeat >= 10, "the record wants the median of at least ten calls"
    import zkevm_circuits_amd as z
    ctx = z.Context(0)
    device = ctx.device_info()
    key = bytes(range(32))
    for k in (int(v) for v in args.log_sizes.split(",")):
        n = 1 << k
        a, b, out = ctx.alloc(n * 32), ctx.alloc(n * 32), ctx.alloc(n * 32)
        ctx.fr_random(key, 1, 0, a, n)
        ctx.fr_random(key, 2, 0, b, n)
        calls = {
            "scan_affine": lambda: ctx.field_vec_op(z.FIELD_FR, z.OP_SCAN_AFFINE, a, b, out, n),
            "scan_affine_rev": lambda: ctx.field_vec_op(z.FIELD_FR, z.OP_SCAN_AFFINE_REV, a, b, out, n),
            "prefix_product": lambda: ctx.fr_prefix_product(a, out, n),
        }
        ms = {name: [] for name in calls}
        for it in range(args.warmup + args.repeat):
            for name, call in calls.items():
                ctx.sync()
                ctx.timer_start()
                call()
                t = ctx.timer_stop_ms()
                if it >= args.warmup:
                    ms[name].append(t)
        med = {name: statistics.median(v) for name, v in ms.items()}
        booked = {"scan_affine": n * 96, "scan_affine_rev": n * 96, "prefix_product": n * 64}
        res = {"device": device[0].strip(), "log_n": k, "n": n, "timed_calls": args.repeat, "warmup_calls": args.warmup}
        for name in calls:
            res[f"{name}_ms_median"] = round(med[name], 4)
            res[f"{name}_ms_min"] = round(min(ms[name]), 4)
            res[f"{name}_ms_max"] = round(max(ms[name]), 4)
            res[f"{name}_algorithmic_GB_per_s"] = round(booked[name] / med[name] / 1e6, 1)
        res["scan_affine_over_prefix_product"] = round(med["scan_affine"] / med["prefix_product"], 3)
        res["scan_affine_rev_over_prefix_product"] = round(med["scan_affine_rev"] / med["prefix_product"], 3)
        ctx.sync()
        ctx.prof_reset()
        ctx.prof_enable(True)
        calls["scan_affine"]()
        calls["scan_affine_rev"]()
        prof_ms, prof_calls = ctx.prof_get("fr_scan_affine")
        res["prof_fr_scan_affine"] = {"calls": prof_calls, "ms": round(prof_ms, 4), "bytes": ctx.prof_get_bytes("fr_scan_affine")}
        ctx.prof_enable(False)
        assert prof_calls == 2 and res["prof_fr_scan_affine"]["bytes"] == 2 * n * 96
        print(json.dumps(res), flush=True)
        for buf in (a, b, out):
            buf.free()
    ctx.close()


if __name__ == "__main__":
    main()

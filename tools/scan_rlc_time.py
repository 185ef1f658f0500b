"""ZK_OP_SCAN_RLC beside the composition of calls that gave the same column before it: zk_fr_from_uint of the cells, zk_fr_from_uint
of a flag column, ZK_OP_SUB against a column of ones, zk_fr_scale by r, ZK_OP_SCAN_AFFINE.

At n = 2^20 (--log-n), for two columns: byte cells with a kind column (kinds step and start, a restart every 32 rows on average: what
the composition can express -- a hold row would cost it one more column), and 16-byte cells without kinds (the plain Horner running
RLC).  The cells are random bytes made on the device by zk_fr_random; one process, nothing else on the device.  The composition is
given every advantage the old interface allowed: its three n x 32 B temporaries and the column of ones exist beforehand, and without
kinds it runs as four calls instead of five (the ones copied by zk_d2d and scaled by r; no flag column, no subtraction).  Both routes
are checked once to give the same bytes.  Every route is timed by itself with the context's HIP-event timer around the whole
sequence of calls, the stream drained before; --warmup untimed runs of each, then --repeat timed ones, the routes taking turns.
Prints one JSON line per case: median, minimum and maximum in ms, the op's rate over its booked bytes n x (width + kinds + 32), the
composition's time over the op's, and what a last profiled call booked.

usage: python tools/scan_rlc_time.py [--log-n 20] [--repeat 20] [--warmup 3]"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = {"bytes_with_kinds": (1, True), "u128_without_kinds": (16, False)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-n", type=int, default=20)
    ap.add_argument("--repeat", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    assert args.repeat >= 10, "the record wants the median of at least ten calls"
    import zkevm_circuits_amd as z
    from oracle import bn254, cref
    ctx = z.Context(0)
    device = ctx.device_info()
    key = bytes(range(32))
    n = 1 << args.log_n
    P = bn254.R_MOD
    r = 0x2B7E151628AED2A6ABF7158809CF4F3C762E7160F38B4DA56A784D9045190CFE % P
    r_mont, one, zero = cref.to_mont([r])[0], cref.to_mont([1])[0], cref.to_mont([0])[0]
    table = np.array([(r_mont, one), (zero, one), (one, zero), (zero, zero)], dtype=np.uint64)      # step, start, hold, clear
    for name, (width, with_kinds) in CASES.items():
        cells = ctx.alloc(n * 32)                                   # the first n * width bytes are the column
        ctx.fr_random(key, 10 + width, 0, cells, n)
        kinds = None
        if with_kinds:
            kinds = ctx.to_device((np.random.default_rng(5).integers(0, 32, n) == 0).astype(np.uint8))     # the flag column and the kind column
        out = ctx.alloc(n * 32)
        t_a, t_b, t_f, t_out = (ctx.alloc(n * 32) for _ in range(4))       # the composition's temporaries and its result
        ones_bytes = ctx.to_device(np.ones(n, dtype=np.uint8))
        ones = ctx.alloc(n * 32)
        ctx.fr_from_uint(ones_bytes, 1, n, ones)

        def op():
            ctx.scan_rlc(cells, width, kinds, table, n, out)

        def composition():
            ctx.fr_from_uint(cells, width, n, t_b)                  # b = x
            if with_kinds:
                ctx.fr_from_uint(kinds, 1, n, t_f)
                ctx.field_vec_op(z.FIELD_FR, z.OP_SUB, ones, t_f, t_a, n)      # 1 - first
            else:
                ctx._ck(z.lib().zk_d2d(ctx.h, ctypes.c_void_p(t_a.ptr), ctypes.c_void_p(ones.ptr), ctypes.c_size_t(n * 32)))
            ctx.fr_scale(t_a, r_mont, n)                            # a = r (1 - first)
            ctx.scan_affine(t_a, t_b, t_out, n)

        routes = {"scan_rlc": op, "composition": composition}
        ms = {k: [] for k in routes}
        for it in range(args.warmup + args.repeat):
            for k, call in routes.items():
                ctx.sync()
                ctx.timer_start()
                call()
                t = ctx.timer_stop_ms()
                if it >= args.warmup:
                    ms[k].append(t)
        same = bool(np.array_equal(out.download((n, 4)), t_out.download((n, 4))))
        med = {k: statistics.median(v) for k, v in ms.items()}
        booked = n * (width + (1 if with_kinds else 0) + 32)
        res = {"device": device[0].strip(), "case": name, "width": width, "kinds": with_kinds, "log_n": args.log_n, "n": n, "timed_calls": args.repeat,
               "warmup_calls": args.warmup, "composition_calls": 5 if with_kinds else 4}
        for k in routes:
            res[f"{k}_ms_median"] = round(med[k], 4)
            res[f"{k}_ms_min"] = round(min(ms[k]), 4)
            res[f"{k}_ms_max"] = round(max(ms[k]), 4)
        res["scan_rlc_booked_bytes"] = booked
        res["scan_rlc_algorithmic_GB_per_s"] = round(booked / med["scan_rlc"] / 1e6, 1)
        res["composition_over_scan_rlc"] = round(med["composition"] / med["scan_rlc"], 2)
        res["same_bytes"] = same
        ctx.sync()
        ctx.prof_reset()
        ctx.prof_enable(True)
        op()
        prof_ms, prof_calls = ctx.prof_get("fr_scan_rlc")
        res["prof_fr_scan_rlc"] = {"calls": prof_calls, "ms": round(prof_ms, 4), "bytes": ctx.prof_get_bytes("fr_scan_rlc")}
        ctx.prof_enable(False)
        print(json.dumps(res), flush=True)
        assert same and prof_calls == 1 and res["prof_fr_scan_rlc"]["bytes"] == booked
        for buf in [cells, out, t_a, t_b, t_f, t_out, ones_bytes, ones] + ([kinds] if kinds is not None else []):
            buf.free()
    ctx.close()


if __name__ == "__main__":
    main()

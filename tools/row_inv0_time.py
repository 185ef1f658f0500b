"""ZK_OP_ROW_INV0 beside the composition of calls that gave the same column before it: ZK_OP_ROW_RLC into a temporary, then
zk_fr_batch_invert on it, then ZK_OP_MUL by the numerator where there is one.

At n = 2^20 (--log-n), for three shapes: IsZeroChip's value_inv of a byte column; IsEqual's inverse of the difference of two 8-byte
columns, w = (1, -1); a rational cell with a 32-byte denominator and a 32-byte numerator.  The cells are random bytes (the 32-byte
columns random field elements) made on the device by zk_fr_random, so a byte column has a zero in one row of 256 and the others have
practically none; one process, nothing else on the device.  The composition's temporary exists beforehand.  Both routes are checked
once to give the same bytes.  Every route is timed by itself with the context's HIP-event timer around the whole sequence of calls, the
stream drained before; --warmup untimed runs of each, then --repeat timed ones, the routes taking turns.  Prints one JSON line per
shape: median, minimum and maximum in ms, the op's rate over its booked bytes n x (sum of widths + num_width + 32), the
composition's time over the op's, and what a last profiled call booked.

usage: python tools/row_inv0_time.py [--log-n 20] [--repeat 20] [--warmup 3]"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# name: (denominator widths, weights as plain integers with -1 for r - 1, numerator width or None)
SHAPES = {"value_inv_byte": ([1], [1], None), "is_equal_8_8": ([8, 8], [1, -1], None), "rational_32_over_32": ([32], [1], 32)}


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
    for name, (widths, ws, num_width) in SHAPES.items():
        w_mont = cref.to_mont([w % P for w in ws])
        cols = [ctx.alloc(n * 32) for _ in widths]                   # column j uses the first n * widths[j] bytes
        for j, buf in enumerate(cols):
            ctx.fr_random(key, 40 + j, 0, buf, n)
        num = None
        if num_width:
            num = ctx.alloc(n * 32)
            ctx.fr_random(key, 60, 0, num, n)
        out, tmp = ctx.alloc(n * 32), ctx.alloc(n * 32)

        def op():
            ctx.row_inv0(cols, widths, w_mont, n, out, num=num, num_width=num_width or 32)

        def composition():
            ctx.row_rlc(cols, widths, w_mont, n, tmp)
            ctx.fr_batch_invert(tmp, n)
            if num is not None:
                ctx.field_vec_op(z.FIELD_FR, z.OP_MUL, tmp, num, tmp, n)

        routes = {"row_inv0": op, "composition": composition}
        ms = {k: [] for k in routes}
        for it in range(args.warmup + args.repeat):
            for k, call in routes.items():
                ctx.sync()
                ctx.timer_start()
                call()
                t = ctx.timer_stop_ms()
                if it >= args.warmup:
                    ms[k].append(t)
        same = bool(np.array_equal(out.download((n, 4)), tmp.download((n, 4))))
        med = {k: statistics.median(v) for k, v in ms.items()}
        booked = n * (sum(widths) + (num_width or 0) + 32)
        res = {"device": device[0].strip(), "shape": name, "widths": widths, "num_width": num_width, "log_n": args.log_n, "n": n, "timed_calls": args.repeat, "warmup_calls": args.warmup}
        for k in routes:
            res[f"{k}_ms_median"] = round(med[k], 4)
            res[f"{k}_ms_min"] = round(min(ms[k]), 4)
            res[f"{k}_ms_max"] = round(max(ms[k]), 4)
        res["row_inv0_booked_bytes"] = booked
        res["row_inv0_algorithmic_GB_per_s"] = round(booked / med["row_inv0"] / 1e6, 1)
        res["composition_over_row_inv0"] = round(med["composition"] / med["row_inv0"], 2)
        res["same_bytes"] = same
        ctx.sync()
        ctx.prof_reset()
        ctx.prof_enable(True)
        op()
        prof_ms, prof_calls = ctx.prof_get("fr_row_inv0")
        res["prof_fr_row_inv0"] = {"calls": prof_calls, "ms": round(prof_ms, 4), "bytes": ctx.prof_get_bytes("fr_row_inv0")}
        ctx.prof_enable(False)
        print(json.dumps(res), flush=True)
        assert same and prof_calls == 1 and res["prof_fr_row_inv0"]["bytes"] == booked
        for buf in cols + [out, tmp] + ([num] if num is not None else []):
            buf.free()
    ctx.close()


if __name__ == "__main__":
    main()

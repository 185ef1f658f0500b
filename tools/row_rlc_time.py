"""ZK_OP_ROW_RLC beside the composition of calls that gave the same column before it: zk_fr_from_uint_batch, then zk_fr_scale and
ZK_OP_ADD per column.

At n = 2^20 (--log-n), for two tables: the 32 byte columns of a word RLC (w_j = r^j, no constant), and the eleven columns of
RwRow::rlc (widths 8, 1, 1, 4, 16, 1, 32, 32, 32, 16, 16; constant r^11, descending powers).  The cells are random bytes (the
32-byte columns random field elements) made on the device by zk_fr_random; one process, nothing else on the device.  The composition
is given every advantage the old interface allowed: its buffers exist beforehand, the first column's product starts the sum (no
addition for it), the constant column is prepared outside the timed region and costs one addition; a 32-byte column, which
zk_fr_scale would overwrite, is copied first (zk_d2d).  Both routes are checked once to give the same bytes.  Every route is timed
by itself with the context's HIP-event timer around the whole sequence of calls, the stream drained before; --warmup untimed runs of
each, then --repeat timed ones, the routes taking turns.  Prints one JSON line per table: median, minimum and maximum in ms, the
op's rate over its booked bytes n x (sum of widths + 32), the composition's time over the op's, and what a last profiled call booked.

usage: python tools/row_rlc_time.py [--log-n 20] [--repeat 20] [--warmup 3]"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

TABLES = {"word_32_bytes": [1] * 32, "rw_row": [8, 1, 1, 4, 16, 1, 32, 32, 32, 16, 16]}


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
    for name, widths in TABLES.items():
        count = len(widths)
        if name == "rw_row":
            const, ws = pow(r, 11, P), [pow(r, 10 - j, P) for j in range(count)]
        else:
            const, ws = 0, [pow(r, j, P) for j in range(count)]
        w_mont, c_mont = cref.to_mont(ws), cref.to_mont([const])[0]
        cols = [ctx.alloc(n * 32) for _ in widths]                   # column j uses the first n * widths[j] bytes
        for j, buf in enumerate(cols):
            ctx.fr_random(key, 10 + j, 0, buf, n)
        out, const_col = ctx.alloc(n * 32), ctx.alloc(n * 32)
        expanded = [ctx.alloc(n * 32) for _ in widths]
        ones = ctx.to_device(np.ones(n, dtype=np.uint8))
        ctx.fr_from_uint(ones, 1, n, const_col)
        ctx.fr_scale(const_col, c_mont, n)
        narrow = [j for j, w in enumerate(widths) if w < 32]

        def op():
            ctx.row_rlc(cols, widths, w_mont, n, out, constant=c_mont)

        def composition():
            ctx.fr_from_uint_batch([cols[j] for j in narrow], [widths[j] for j in narrow], n, [expanded[j] for j in narrow])
            for j, w in enumerate(widths):
                if w == 32:
                    ctx._ck(z.lib().zk_d2d(ctx.h, ctypes.c_void_p(expanded[j].ptr), ctypes.c_void_p(cols[j].ptr), ctypes.c_size_t(n * 32)))
                ctx.fr_scale(expanded[j], np.ascontiguousarray(w_mont[j]), n)
                if j:
                    ctx.field_vec_op(z.FIELD_FR, z.OP_ADD, expanded[0], expanded[j], expanded[0], n)
            if const:
                ctx.field_vec_op(z.FIELD_FR, z.OP_ADD, expanded[0], const_col, expanded[0], n)

        routes = {"row_rlc": op, "composition": composition}
        ms = {k: [] for k in routes}
        for it in range(args.warmup + args.repeat):
            for k, call in routes.items():
                ctx.sync()
                ctx.timer_start()
                call()
                t = ctx.timer_stop_ms()
                if it >= args.warmup:
                    ms[k].append(t)
        same = bool(np.array_equal(out.download((n, 4)), expanded[0].download((n, 4))))
        med = {k: statistics.median(v) for k, v in ms.items()}
        booked = n * (sum(widths) + 32)
        res = {"device": device[0].strip(), "table": name, "widths": widths, "log_n": args.log_n, "n": n, "timed_calls": args.repeat, "warmup_calls": args.warmup}
        for k in routes:
            res[f"{k}_ms_median"] = round(med[k], 4)
            res[f"{k}_ms_min"] = round(min(ms[k]), 4)
            res[f"{k}_ms_max"] = round(max(ms[k]), 4)
        res["row_rlc_booked_bytes"] = booked
        res["row_rlc_algorithmic_GB_per_s"] = round(booked / med["row_rlc"] / 1e6, 1)
        res["composition_over_row_rlc"] = round(med["composition"] / med["row_rlc"], 2)
        res["same_bytes"] = same
        ctx.sync()
        ctx.prof_reset()
        ctx.prof_enable(True)
        op()
        prof_ms, prof_calls = ctx.prof_get("fr_row_rlc")
        res["prof_fr_row_rlc"] = {"calls": prof_calls, "ms": round(prof_ms, 4), "bytes": ctx.prof_get_bytes("fr_row_rlc")}
        ctx.prof_enable(False)
        print(json.dumps(res), flush=True)
        assert same and prof_calls == 1 and res["prof_fr_row_rlc"]["bytes"] == booked
        for buf in cols + expanded + [out, const_col, ones]:
            buf.free()
    ctx.close()


if __name__ == "__main__":
    main()

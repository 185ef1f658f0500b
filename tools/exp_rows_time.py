"""ZK_OP_EXP_ROWS on one device at 2^15 and 2^19 rows, beside the host route a caller had before it, stated as ONE Python thread: the
closed forms of tests/exp_rows_cases.py (closed: the formulas the op evaluates, in Python) for all 36 columns, their Montgomery form,
and the upload of 36 columns of 32-byte Fr.  A yardstick, not a threshold.

Cases, all filling the rows in front of the ten unusable ones: `one_step`, events of exponent 2 only; `mixed`, random bases with random
exponents of 1 .. 256 bits; `long`, exponent 2^256 - 1 only, 510 steps each -- the longest chain and, beside a `mixed` wave, the worst
divergence.  Every case times the call with every output and without the u16 planes, and reads k_exp_chain and k_exp_rows on their own
from zk_prof ("exp_rows_chain", "exp_rows_tiles"); it prints the booked algorithmic bytes (zk_prof's figure for the call) and the bytes
per second they make at the median.  One process per case and size, nothing else on the device.  A call is timed with the context's
HIP-event timer, the stream drained before (zk_ctx_sync); --warmup untimed calls, then --repeat timed ones; the median, minimum and
maximum are printed.  The host route is timed at --host-log-n rows (2^15: at 2^19 one Python thread needs minutes) and every column the
device wrote is compared with it there; at a larger size the rows of the events that the smaller size holds are compared.

Without --case this is the driver: it runs every case and size as a child process of its own under `timeout -k 10 SECONDS`, one after
the other, and stops at the first that fails -- nothing follows a failed step.  Prints one JSON line per case.

usage: python tools/exp_rows_time.py [--repeat 10] [--warmup 2] [--case one_step|mixed|long] [--log-n 15] [--host-log-n 15] [--step-timeout 400]"""
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

CASES = ("one_step", "mixed", "long")
SIZES = (15, 19)


def events_of(case, n, ex):
    """events whose steps fill the n - 10 rows in use, in an order that does not depend on n: a smaller n holds a prefix"""
    rng = np.random.default_rng(32)
    word = lambda bits: int.from_bytes(rng.bytes(32), "little") >> (256 - bits)   # noqa: E731
    out, left = [], (n - 10) // 8
    while left:
        if case == "one_step":
            e = (word(256), 2)
        elif case == "long":
            e = (word(256) | 1, ex.M256)
        else:
            e = (word(int(rng.integers(1, 257))), word(int(rng.integers(1, 257))))
        steps = ex.steps_of(e[1])
        if steps > left:
            if case == "long":
                break                                                   # padding steps take the rest
            e, steps = (e[0], 2), 1
        if steps:
            out.append(e)
            left -= steps
    return out


def timed(ctx, call, warmup, repeat, names):
    """the call's time on the context's timer and, per profiler name, its time in that call"""
    ms, prof = [], {name: [] for name in names}
    for it in range(warmup + repeat):
        ctx.sync()
        ctx.prof_reset()
        ctx.timer_start()
        call()
        t = ctx.timer_stop_ms()
        ctx.sync()
        if it >= warmup:
            ms.append(t)
            for name in names:
                prof[name].append(ctx.prof_get(name)[0])
    return ms, prof


def spread(ms):
    return {"ms_median": round(statistics.median(ms), 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4)}


def summary(ms, nbytes):
    med = statistics.median(ms)
    return dict(spread(ms), booked_bytes=int(nbytes), GBps=round(nbytes / med / 1e6, 1))


def run_case(case, log_n, host_log_n, warmup, repeat):
    import exp_rows_cases as ex
    import zkevm_circuits_amd as z
    from zkevm_circuits_amd import plonk
    b = z.binding
    ctx = z.Context(0)
    n = 1 << log_n
    events = events_of(case, n, ex)
    count = len(events)
    res = {"device": ctx.device_info()[0].strip(), "case": case, "n": n, "events": count, "steps": sum(ex.steps_of(x) for _, x in events), "timed_calls": repeat, "warmup_calls": warmup}

    # the host route at min(n, 2^host_log_n) rows: the events of that size are a prefix of these
    hn = min(n, 1 << host_log_n)
    h_events = events_of(case, hn, ex)
    t0 = time.perf_counter()
    host = ex.closed(h_events, hn)
    res["host_rows"] = hn
    res["host_closed_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
    t0 = time.perf_counter()
    mont = [plonk.column_to_mont(host[name]) for name in ex.COLUMNS]
    res["host_montgomery_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
    t0 = time.perf_counter()
    uploaded = [ctx.to_device(a) for a in mont]
    ctx.sync()
    res["host_upload_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
    for buf in uploaded:
        buf.free()

    d_events = ctx.to_device(ex.pack_events(events))
    width = {name: w * p for name, w, p in ex.OUTPUTS}
    d = {name: ctx.alloc(n * width[name]) for name in width}
    d_needed = ctx.alloc(8)
    outs = tuple(name for name, _, _ in ex.OUTPUTS[1:])
    call = lambda names: ctx.exp_rows(d_events, count, n, d["exponentiation_lo_hi"], rows_needed=d_needed, **{name: d[name] for name in names})   # noqa: E731
    ctx.prof_enable(True)
    kernels = ("exp_rows_chain", "exp_rows_tiles")
    for label, names in (("every_output", outs), ("without_u16_planes", tuple(x for x in outs if x not in ex.U16_OUTPUTS))):
        ms, prof = timed(ctx, lambda: call(names), warmup, repeat, kernels)
        res[label] = summary(ms, 64 * count + n * (16 + sum(width[x] for x in names)))
        res[label]["k_exp_chain"], res[label]["k_exp_rows"] = spread(prof["exp_rows_chain"]) if count else None, spread(prof["exp_rows_tiles"])
    ctx.prof_enable(False)
    call(outs)
    ctx.sync()
    res["rows_needed"] = int(d_needed.download(1, np.uint64)[0])
    # every column against the host's: all rows at the host's size, else the rows of the events the host's size holds
    shared = next((i for i, (p, q) in enumerate(zip(h_events, events)) if p != q), len(h_events))
    rows = hn if hn == n else 8 * sum(ex.steps_of(x) for _, x in h_events[:shared])
    equal = res["rows_needed"] == ex.rows_needed(events)
    for name, w, planes in ex.OUTPUTS:
        got = d[name].download(n * w * planes, np.uint8).reshape(planes, n * w)[:, :rows * w]
        want = np.frombuffer(ex.output_bytes(host, hn, name), dtype=np.uint8).reshape(planes, hn * w)[:, :rows * w]
        equal = equal and bool(np.array_equal(got, want))
    res["compared_rows"], res["columns_equal_host"] = rows, equal
    res["host_over_device"] = round((res["host_closed_ms"] + res["host_montgomery_ms"] + res["host_upload_ms"]) * (n / hn) / res["every_output"]["ms_median"], 1)
    print(json.dumps(res), flush=True)
    for buf in (d_events, d_needed, *d.values()):
        buf.free()
    ctx.close()
    return 0 if equal else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--case", choices=CASES)
    ap.add_argument("--log-n", type=int)
    ap.add_argument("--host-log-n", type=int, default=15)
    ap.add_argument("--step-timeout", type=int, default=400)
    args = ap.parse_args()
    if args.case:
        return run_case(args.case, args.log_n or 15, args.host_log_n, args.warmup, args.repeat)
    for log_n in ((args.log_n,) if args.log_n else SIZES):
        for case in CASES:                                              # every GPU step under its own time limit; nothing follows a failed one
            cmd = ["timeout", "-k", "10", str(args.step_timeout), sys.executable, os.path.abspath(__file__), "--case", case, "--repeat", str(args.repeat), "--warmup", str(args.warmup),
                   "--log-n", str(log_n), "--host-log-n", str(args.host_log_n)]
            rc = subprocess.run(cmd).returncode
            if rc != 0:
                print(json.dumps({"case": case, "log_n": log_n, "failed_with_status": rc, "stopped": True}), flush=True)
                return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())

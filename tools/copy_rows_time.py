"""ZK_OP_COPY_ROWS and ZK_OP_COPY_RLC on one device at 2^19 rows, beside the host route a caller had before them: the row-by-row model
of tests/copy_rows_cases.py (closed: the formulas the ops evaluate, in Python) for every column, then the upload of the columns it
made.  A yardstick, not a threshold.

Cases, all filling 2^19 rows: `single`, one event that owns every row; `tiny`, 2^18 events of one step; `mixed`, events of 1 .. 24 576
steps in the proportions of a block (many short CALLDATACOPY / LOG / SHA3 ranges, a few CODECOPY and RETURN of whole contracts), with
masks, padded reads, memory copies and log biases.  Every case times ZK_OP_COPY_ROWS with every output and with the 8-byte columns
alone, and ZK_OP_COPY_RLC with every output and with value_acc alone; it prints the booked algorithmic bytes (zk_prof's figure for the
call) and the bytes per second they make at the median.  One process per case, nothing else on the device.  A call is timed with the
context's HIP-event timer, the stream drained before (zk_ctx_sync); --warmup untimed calls, then --repeat timed ones; the median,
minimum and maximum are printed.  Every column the device wrote is compared with the host's, all rows.

Without --case this is the driver: it runs every case as a child process of its own under `timeout -k 10 SECONDS`, one after the
other, and stops at the first that fails -- nothing follows a failed step.  Prints one JSON line per case.

usage: python tools/copy_rows_time.py [--repeat 10] [--warmup 2] [--case single|tiny|mixed] [--log-n 19] [--step-timeout 400]"""
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

CASES = ("single", "tiny", "mixed")
HEAP = 1 << 16
R_WORD, R_IN = 0x1234567890ABCDEF1234567890ABCDEF, 0x0FEDCBA987654321FEDCBA9876543210


def events_of(case, n, cp):
    rng = np.random.default_rng(31)
    steps = n // 2
    if case == "single":
        lengths = [steps]
    elif case == "tiny":
        lengths = [1] * steps
    else:
        lengths, left = [], steps
        while left:
            length = min(int(rng.integers(1, 24577)) if rng.random() < 0.05 else int(rng.integers(1, 400)), left)
            lengths.append(length)
            left -= length
    out = []
    for k, length in enumerate(lengths):
        span = min(length, HEAP)
        src_tag, dst_tag = [(cp.MEMORY, cp.MEMORY), (cp.TX_CALLDATA, cp.MEMORY), (cp.BYTECODE, cp.MEMORY), (cp.MEMORY, cp.TX_LOG), (cp.MEMORY, cp.RLC_ACC), (cp.MEMORY, cp.BYTECODE)][k % 6]
        off = lambda: int(rng.integers(0, HEAP - span + 1))              # noqa: E731
        src_off = off()
        front = int(rng.integers(0, 32)) % (length + 1)
        src_addr = int(rng.integers(0, 1 << 24))
        out.append(cp.event(span, src_tag, dst_tag, src_addr=src_addr, src_addr_end=src_addr + max(0, span - int(rng.integers(0, 40))), dst_addr=int(rng.integers(0, 1 << 24)),
                            dst_addr_bias=cp.log_bias(k % 7) if dst_tag == cp.TX_LOG else 0, rw_counter=1 + 3 * k, src_off=src_off,
                            dst_off=src_off if dst_tag in (cp.RLC_ACC, cp.BYTECODE) else off(), prev_off=off(), src_front=front, dst_front=front, flags=int(k % 12 == 0),
                            src_id=k + 1, dst_id=k + 1 if k % 12 == 0 else k + 2))
    if case == "single":                                                 # one event of n / 2 steps over a heap of that size
        out = [cp.event(steps, cp.MEMORY, cp.BYTECODE, src_addr=64, src_addr_end=64 + steps - 9, dst_addr=0, rw_counter=5, src_off=0, dst_off=0, prev_off=0, src_front=3, src_back=2, src_id=1, dst_id=2)]
    return out


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


def summary(ms, nbytes):
    med = statistics.median(ms)
    return {"ms_median": round(med, 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4), "booked_bytes": int(nbytes), "GBps": round(nbytes / med / 1e6, 1)}


def run_case(case, log_n, warmup, repeat):
    import copy_rows_cases as cp
    import zkevm_circuits_amd as z
    b = z.binding
    ctx = z.Context(0)
    n = 1 << log_n
    events = events_of(case, n, cp)
    heap_len = n // 2 if case == "single" else HEAP
    heap = bytes(np.random.default_rng(2).integers(0, 256, heap_len, dtype=np.uint8))
    count = len(events)
    res = {"device": ctx.device_info()[0].strip(), "case": case, "n": n, "events": count, "heap_bytes": heap_len, "longest": max(e["length"] for e in events),
           "timed_calls": repeat, "warmup_calls": warmup}

    t0 = time.perf_counter()
    host = cp.closed(events, heap, n, R_WORD % cp.R, R_IN % cp.R)        # the host route: every column, row by row
    ints = cp.columns_numpy(host, n)
    frs = {name: cp.fr_numpy(host[name]) for name in cp.FR_COLUMNS}
    res["host_model_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
    t0 = time.perf_counter()
    uploaded = [ctx.to_device(a) for a in list(ints.values()) + list(frs.values())]
    ctx.sync()
    res["host_upload_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
    for buf in uploaded:
        buf.free()

    d_events, d_heap, d_ids = ctx.to_device(cp.pack_events(events)), ctx.to_device(np.frombuffer(heap, dtype=np.uint8)), ctx.to_device(cp.pack_ids(events))
    width = {name: 1 for name in cp.BYTE_COLUMNS}
    width.update({name: 8 for name in cp.WORD_COLUMNS})
    width.update(cp.PLANE_COLUMNS)
    d = {name: ctx.alloc(n * width[name]) for name in ("addr",) + b.COPY_ROWS_OUTPUTS}
    f = {name: ctx.alloc(n * 32) for name in ("value_acc",) + b.COPY_RLC_OUTPUTS}
    r_word, r_in = cp.fr_numpy([R_WORD % cp.R])[0], cp.fr_numpy([R_IN % cp.R])[0]
    rows = lambda outs: ctx.copy_rows(d_events, count, d_heap, heap_len, n, d["addr"], **{name: d[name] for name in outs})                      # noqa: E731
    rlc = lambda outs: ctx.copy_rlc(d_events, count, d_heap, heap_len, n, f["value_acc"], r_word, r_in, ids=d_ids, **{name: f[name] for name in outs})   # noqa: E731
    words = tuple(name for name in b.COPY_ROWS_OUTPUTS if width[name] == 8)
    for label, outs in (("rows_every_output", b.COPY_ROWS_OUTPUTS), ("rows_8_byte_columns", words)):
        reads = "value" in outs
        res[label] = summary(timed(ctx, lambda: rows(outs), warmup, repeat), 88 * count + (heap_len if reads else 0) + n * (8 + sum(width[name] for name in outs)))
    for label, outs in (("rlc_every_output", b.COPY_RLC_OUTPUTS), ("rlc_value_acc_alone", ())):
        res[label] = summary(timed(ctx, lambda: rlc(outs), warmup, repeat), (88 + 64) * count + heap_len + n * 32 * (1 + len(outs)))
    rows(b.COPY_ROWS_OUTPUTS)
    rlc(b.COPY_RLC_OUTPUTS)
    ctx.sync()
    equal = {name: bool(np.array_equal(d[name].download(n * width[name] // (8 if width[name] == 8 else 1), np.uint64 if width[name] == 8 else np.uint8), ints[name])) for name in d}
    equal.update({name: bool(np.array_equal(f[name].download((n, 4)), frs[name])) for name in f})
    res["columns_equal_host"] = all(equal.values())
    res["host_over_device"] = round((res["host_model_ms"] + res["host_upload_ms"]) / (res["rows_every_output"]["ms_median"] + res["rlc_every_output"]["ms_median"]), 1)
    print(json.dumps(res), flush=True)
    for buf in (d_events, d_heap, d_ids, *d.values(), *f.values()):
        buf.free()
    ctx.close()
    return 0 if res["columns_equal_host"] else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--case", choices=CASES)
    ap.add_argument("--log-n", type=int, default=19)
    ap.add_argument("--step-timeout", type=int, default=400)
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

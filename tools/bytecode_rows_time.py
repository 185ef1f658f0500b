"""ZK_OP_BYTECODE_ROWS on one device at 2^19 rows, beside the host route a caller had before it: the Python/numpy unroll of
tests/bytecode_rows_cases.py (rows_numpy: the columns vectorised per bytecode, push_data_left by the serial loop a host has), after
which it would still have to upload nine integer columns and a hash column.  A yardstick, not a threshold.

Cases, all filling 2^19 rows: `mixed`, about 150 codes of 0 .. 24 576 bytes; `single`, one code that fills every row; `tiny`, 2^18
one-byte codes.  Every case times the call with every output, with only the outputs that need no push state (tag, index, value,
push_data_size, length), and the hashes-only call of the challenge phase; it prints the booked algorithmic bytes (zk_prof's figure for
the call) and the bytes per second they make at the median.  One process per case, nothing else on the device.  A call is timed with
the context's HIP-event timer, the stream drained before (zk_ctx_sync); --warmup untimed calls, then --repeat timed ones; the median,
minimum and maximum are printed.  Every integer column the device wrote is compared with the host's, all rows.

Without --case this is the driver: it runs every case as a child process of its own under `timeout -k 10 SECONDS`, one after the
other, and stops at the first that fails -- nothing follows a failed step.  Prints one JSON line per case.

usage: python tools/bytecode_rows_time.py [--repeat 10] [--warmup 2] [--case mixed|single|tiny] [--log-n 19] [--step-timeout 300]"""
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

CASES = ("mixed", "single", "tiny")
WIDTHS = {"tag": 1, "index": 4, "value": 4, "is_code": 1, "push_data_left": 1, "push_data_size": 1, "length": 4, "acc_kinds": 1, "rlc_kinds": 1}
STATELESS = ("tag", "index", "value", "push_data_size", "length")


def codes_of(case, n, bc):
    rng = np.random.default_rng(30)
    if case == "single":
        return [bc.random_code(rng, n - 1)]
    if case == "tiny":
        return [bytes([v]) for v in rng.integers(0, 256, n // 2, dtype=np.uint8)]
    codes, left = [], n
    while left > 1:
        length = min(int(rng.integers(0, 24577)) if rng.random() < 0.25 else int(rng.integers(0, 2000)), left - 1)
        codes.append(bc.random_code(rng, length))
        left -= length + 1
    return codes


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
    import bytecode_rows_cases as bc
    import zkevm_circuits_amd as z
    ctx = z.Context(0)
    n = 1 << log_n
    codes = codes_of(case, n, bc)
    buf, offs, lens = bc.lay_out(codes)
    count, total = len(codes), len(buf)
    res = {"device": ctx.device_info()[0].strip(), "case": case, "n": n, "bytecodes": count, "code_bytes": total, "longest": max(lens), "timed_calls": repeat, "warmup_calls": warmup}

    t0 = time.perf_counter()
    host = bc.rows_numpy(codes, n)                                      # the host route
    res["host_numpy_ms"] = round((time.perf_counter() - t0) * 1e3, 1)

    d_bytes, d_offs, d_lens = ctx.to_device(buf if total else np.zeros(1, np.uint8)), ctx.to_device(np.array(offs, dtype=np.uint32)), ctx.to_device(np.array(lens, dtype=np.uint32))
    d_hashes = ctx.to_device(np.random.default_rng(1).integers(0, 2**62, (count, 4), dtype=np.uint64))
    d_out = ctx.alloc(32 * n)
    d = {name: ctx.alloc(n * w) for name, w in WIDTHS.items()}
    empty = np.arange(1, 5, dtype=np.uint64)
    call = lambda outs: ctx.bytecode_rows(d_bytes, total, d_offs, d_lens, 4, count, n, d_out, empty, hashes=d_hashes, **{name: d[name] for name in outs})
    entries = count * (8 + 32)
    for label, outs, reads in (("every_output", tuple(WIDTHS), True), ("no_push_state", STATELESS, True), ("hashes_only", (), False)):
        ms = timed(ctx, lambda: call(outs), warmup, repeat)
        res[label] = summary(ms, entries + (total if reads else 0) + n * (32 + sum(WIDTHS[name] for name in outs)))
    call(tuple(WIDTHS))
    ctx.sync()
    equal = {name: bool(np.array_equal(d[name].download(n, np.uint8 if w == 1 else np.uint32), host[name])) for name, w in WIDTHS.items()}
    res["columns_equal_host"] = all(equal.values())
    res["host_over_device"] = round(res["host_numpy_ms"] / res["every_output"]["ms_median"], 1)
    print(json.dumps(res), flush=True)
    for b in (d_bytes, d_offs, d_lens, d_hashes, d_out, *d.values()):
        b.free()
    ctx.close()
    return 0 if res["columns_equal_host"] else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--case", choices=CASES)
    ap.add_argument("--log-n", type=int, default=19)
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

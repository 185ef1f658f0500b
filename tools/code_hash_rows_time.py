"""ZK_OP_CODE_HASH_ROWS and ZK_OP_CODE_HASH_TABLE on one device at 2^19 rows, beside ZK_OP_BYTECODE_ROWS on the same inputs (the
sibling op, the yardstick) and beside the host route a caller had before them: the Python model of tests/code_hash_rows_cases.py
(rows_numpy and table_numpy: one cached big-integer conversion per row, the serial part a host has), after which it would still have
to upload three 32-byte columns and five narrow ones.  A yardstick, not a threshold.

Cases, the inputs of tools/bytecode_rows_time.py, all filling 2^19 circuit rows: `mixed`, about 150 codes of 0 .. 24 576 bytes;
`single`, one code that fills every row; `tiny`, 2^18 one-byte codes.  Every case times the row op with every output and with
field_input alone, the table op with every output over 2^19 table rows (the codes own only the first rows_needed of them, the rest
are off rows) and, in `single`, over one code of 62 x 2^19 bytes that owns every table row, and the sibling op with every output.  It
prints the booked algorithmic bytes (zk_prof's figure for the call) and the bytes per second they make at the median.  One process
per case, nothing else on the device.  A call is timed with the context's HIP-event timer, the stream drained before (zk_ctx_sync);
--warmup untimed calls, then --repeat timed ones; the median, minimum and maximum are printed.  Every column the device wrote is
compared with the host's, all rows.

Without --case this is the driver: it runs every case as a child process of its own under `timeout -k 10 SECONDS`, one after the
other, and stops at the first that fails -- nothing follows a failed step.  Prints one JSON line per case.

usage: python tools/code_hash_rows_time.py [--repeat 10] [--warmup 2] [--case mixed|single|tiny] [--log-n 19] [--step-timeout 300]"""
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

CASES = ("mixed", "single", "tiny")


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
    import code_hash_rows_cases as ch
    import zkevm_circuits_amd as z
    from bytecode_rows_time import WIDTHS as BC_WIDTHS, codes_of
    ctx = z.Context(0)
    n = 1 << log_n
    codes = codes_of(case, n, bc)
    buf, offs, lens = bc.lay_out(codes)
    count, total = len(codes), len(buf)
    res = {"device": ctx.device_info()[0].strip(), "case": case, "n": n, "bytecodes": count, "code_bytes": total, "longest": max(lens), "timed_calls": repeat, "warmup_calls": warmup}

    t0 = time.perf_counter()
    host = ch.rows_numpy(codes, n)                                      # the host route
    res["host_rows_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
    t0 = time.perf_counter()
    host_table, needed = ch.table_numpy(codes, n)
    res["host_table_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
    res["table_rows_needed"] = needed

    d_bytes, d_offs, d_lens = ctx.to_device(buf if total else np.zeros(1, np.uint8)), ctx.to_device(np.array(offs, dtype=np.uint32)), ctx.to_device(np.array(lens, dtype=np.uint32))
    row_w = {name: w for name, w in ch.ROW_WIDTHS.items() if name != "field_input"}
    tab_w = dict({name: w for name, w in ch.TABLE_WIDTHS.items() if name != "input0"}, rows_needed=8)
    d_out = ctx.alloc(32 * n)
    d = {name: ctx.alloc(n * w) for name, w in row_w.items()}
    t = {name: ctx.alloc(8 if name == "rows_needed" else n * w) for name, w in tab_w.items()}
    b = {name: ctx.alloc(n * w) for name, w in BC_WIDTHS.items()}
    entries = count * 8

    # the upload of the columns the row op replaces, as the host route pays it: pageable numpy arrays to the device
    ctx.sync()
    t0 = time.perf_counter()
    ups = [ctx.to_device(host[name]) for name in ch.ROW_COLUMNS]
    ctx.sync()
    res["upload_rows_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
    for u in ups:
        u.free()

    rows_call = lambda outs: ctx.code_hash_rows(d_bytes, total, d_offs, d_lens, 4, count, n, d_out, **{name: d[name] for name in outs})
    res["rows_every_output"] = summary(timed(ctx, lambda: rows_call(tuple(row_w)), warmup, repeat), entries + total + n * (32 + sum(row_w.values())))
    res["rows_field_input_only"] = summary(timed(ctx, lambda: rows_call(()), warmup, repeat), entries + total + n * 32)
    rows_call(tuple(row_w))
    ctx.sync()
    equal = {name: bool(np.array_equal(d[name].download(n * w, np.uint8), host[name])) for name, w in row_w.items()}
    equal["field_input"] = bool(np.array_equal(d_out.download(32 * n, np.uint8), host["field_input"]))

    table_call = lambda: ctx.code_hash_table(d_bytes, total, d_offs, d_lens, 4, count, n, d_out, **t)
    res["table_every_output"] = summary(timed(ctx, table_call, warmup, repeat), entries + total + n * (32 + sum(w for name, w in tab_w.items() if name != "rows_needed")) + 8)
    table_call()
    ctx.sync()
    equal.update({"table_" + name: bool(np.array_equal(t[name].download(n * w, np.uint8), host_table[name])) for name, w in tab_w.items() if name != "rows_needed"})
    equal["table_input0"] = bool(np.array_equal(d_out.download(32 * n, np.uint8), host_table["input0"]))
    equal["table_rows_needed"] = int(t["rows_needed"].download(1, np.uint64)[0]) == needed

    if case == "single":                                                # one code that owns every table row
        rng = np.random.default_rng(33)
        long_code = rng.integers(0, 256, 62 * n, dtype=np.uint8)
        d_long, d_one_off, d_one_len = ctx.to_device(long_code), ctx.to_device(np.array([0], dtype=np.uint32)), ctx.to_device(np.array([62 * n], dtype=np.uint32))
        filled = lambda: ctx.code_hash_table(d_long, 62 * n, d_one_off, d_one_len, 4, 1, n, d_out, **t)
        res["table_filled_every_output"] = summary(timed(ctx, filled, warmup, repeat), 8 + 62 * n + n * (32 + sum(w for name, w in tab_w.items() if name != "rows_needed")) + 8)
        for buf_ in (d_long, d_one_off, d_one_len):
            buf_.free()

    d_hashes = ctx.to_device(np.random.default_rng(1).integers(0, 2**62, (count, 4), dtype=np.uint64))
    empty = np.arange(1, 5, dtype=np.uint64)
    sibling = lambda: ctx.bytecode_rows(d_bytes, total, d_offs, d_lens, 4, count, n, d_out, empty, hashes=d_hashes, **b)
    res["bytecode_rows_every_output"] = summary(timed(ctx, sibling, warmup, repeat), count * (8 + 32) + total + n * (32 + sum(BC_WIDTHS.values())))

    res["columns_equal_host"] = all(equal.values())
    res["unequal"] = sorted(name for name, ok in equal.items() if not ok)
    res["rows_over_sibling"] = round(res["rows_every_output"]["ms_median"] / res["bytecode_rows_every_output"]["ms_median"], 2)
    res["host_over_device"] = round((res["host_rows_ms"] + res["upload_rows_ms"]) / res["rows_every_output"]["ms_median"], 1)
    print(json.dumps(res), flush=True)
    for buf_ in (d_bytes, d_offs, d_lens, d_hashes, d_out, *d.values(), *t.values(), *b.values()):
        buf_.free()
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

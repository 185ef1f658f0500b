"""ZK_OP_SHA256 on one device, beside the only route there was before it: hashlib.sha256 per message on one host thread, then the
upload of the n x 32 B result (zk_h2d).  hashlib may use the CPU's SHA instructions; the library has no host SHA-256 of its own.

Cases: `blocks`, 2^17 messages of 64 bytes (two compressions each: the block and the padding block); `kib`, 2^14 messages of 1 KiB;
`mix`, 2^14 messages of 64 bytes with ONE message of 16 KiB among them (what lane-per-message divergence costs: its wave takes 257
compressions, the others two).  Every case times the op without and with d_input_rlc and, next to them, the host route on the same
messages: the wall clock of the loop over hashlib.sha256 (on consecutive slices of one bytes object) plus the upload of the
digests.  The host route makes no RLC at all, so the ratio flatters it.  The bytes are random, laid end to end from an odd
address; one process per case, nothing else on the device.  A call is timed with the context's HIP-event timer, the stream drained
before (zk_ctx_sync); --warmup untimed calls, then --repeat timed ones; the median, minimum and maximum are printed.  The device's
digests are compared with hashlib's, all of them.

Without --case this is the driver: it runs every case as a child process of its own under `timeout -k 10 SECONDS`, one after the
other, and stops at the first that fails -- nothing follows a failed step.  Prints one JSON line per case.

usage: python tools/sha256_time.py [--repeat 10] [--warmup 2] [--case blocks|kib|mix] [--step-timeout 240]"""
import argparse
import hashlib
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = ("blocks", "kib", "mix")
BLOCK = 64


def lengths_of(case):
    if case == "blocks":
        return np.full(1 << 17, 64, dtype=np.uint64)
    if case == "kib":
        return np.full(1 << 14, 1024, dtype=np.uint64)
    lens = np.full(1 << 14, 64, dtype=np.uint64)
    lens[5000] = 16 * 1024
    return lens


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


def run_case(case, warmup, repeat):
    import zkevm_circuits_amd as z
    from oracle import cref
    ctx = z.Context(0)
    device = ctx.device_info()[0].strip()
    lens = lengths_of(case)
    n = len(lens)
    offs = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.uint64)
    total = int(lens.sum())
    rng = np.random.default_rng(26)
    image = rng.integers(0, 256, size=total + 1, dtype=np.uint8)       # the messages start at byte 1: an odd device address
    compressions = int(((lens + 8) // BLOCK + 1).sum())                 # the pad byte and the 8-byte length behind the message
    longest = int(((int(lens.max()) + 8) // BLOCK) + 1)

    # ---- the host route: one thread, then the upload of n x 32 B
    message_bytes = image[1:].tobytes()
    pairs = list(zip((int(o) for o in offs), (int(ln) for ln in lens)))
    sha = hashlib.sha256
    t0 = time.perf_counter()
    joined = b"".join(sha(message_bytes[off:off + ln]).digest() for off, ln in pairs)
    t1 = time.perf_counter()
    digests = np.frombuffer(joined, dtype=np.uint8).reshape(n, 32)
    host_out = ctx.alloc(n * 32)
    t2 = time.perf_counter()
    host_out.upload(digests)
    ctx.sync()
    t3 = time.perf_counter()
    host_ms, upload_ms = (t1 - t0) * 1e3, (t3 - t2) * 1e3

    # ---- the op
    d_bytes = ctx.to_device(image)
    d_offs, d_lens = ctx.to_device(offs), ctx.to_device(lens)
    d_out, d_digest, d_in = ctx.alloc(n * 32), ctx.alloc(n * 32), ctx.alloc(n * 32)
    r_out, r_in = cref.to_mont([0x1234567890ABCDEF ** 3, 0xFEDCBA0987654321 ** 3])
    res = {"device": device, "case": case, "n": n, "message_bytes": total, "longest_message": int(lens.max()), "compressions": compressions, "compressions_of_the_longest": longest,
           "timed_calls": repeat, "warmup_calls": warmup, "host_hashlib_ms": round(host_ms, 2), "host_upload_ms": round(upload_ms, 3),
           "host_us_per_compression": round(host_ms * 1e3 / compressions, 4)}
    for name, with_rlc in (("plain", False), ("input_rlc", True)):
        call = lambda: ctx.sha256(d_bytes.ptr + 1, total, d_offs, d_lens, 8, n, d_out, r_out, r_in=r_in, digest=d_digest, input_rlc=d_in if with_rlc else None)
        ms = timed(ctx, call, warmup, repeat)
        med = statistics.median(ms)
        res[name] = dict(summary(ms), ns_per_compression=round(med * 1e6 / compressions, 3), us_per_compression_of_the_longest=round(med * 1e3 / longest, 3),
                         messages_per_s=round(n / med * 1e3), booked_bytes=n * (16 + 64 + (32 if with_rlc else 0)) + total, host_route_over_op=round((host_ms + upload_ms) / med, 1))
        res[name]["digests_equal_hashlib"] = bool(np.array_equal(d_digest.download((n, 32), np.uint8), digests))
    print(json.dumps(res), flush=True)
    for buf in (host_out, d_bytes, d_offs, d_lens, d_out, d_digest, d_in):
        buf.free()
    ctx.close()
    return 0 if res["plain"]["digests_equal_hashlib"] and res["input_rlc"]["digests_equal_hashlib"] else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--case", choices=CASES)
    ap.add_argument("--step-timeout", type=int, default=240)
    args = ap.parse_args()
    if args.case:
        return run_case(args.case, args.warmup, args.repeat)
    for case in CASES:                                                  # every GPU step under its own time limit; nothing follows a failed one
        cmd = ["timeout", "-k", "10", str(args.step_timeout), sys.executable, os.path.abspath(__file__), "--case", case, "--repeat", str(args.repeat), "--warmup", str(args.warmup)]
        rc = subprocess.run(cmd).returncode
        if rc != 0:
            print(json.dumps({"case": case, "failed_with_status": rc, "stopped": True}), flush=True)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())

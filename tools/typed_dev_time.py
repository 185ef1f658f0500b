"""Packed witness cells resident in HBM: what it costs to get them into a proving session, by the two routes a caller has.

  route A   zk_fr_from_uint once per column into n x 32 B buffers of the caller's, then zk_proof_advice_phase_dev with flags = 0
  route B   zk_proof_advice_phase_typed_dev on the packed cells

Workload: bench_proof.build_shape (the "small" distribution; at --k 20 --shape 1000,150,150,100,9 that is 666 columns of 4-byte
cells, 333 of 8-byte cells and one of bytes), SHPLONK.  The packed witness is put on the device once, one buffer per column.  Each
route runs in a child process of its own, one after the other, against the same library: `--repeat` timed proofs (the first is
the process's warm-up: report proofs 2..), then one untimed proof with zk_prof_enable(1) and a thread that samples
hipMemGetInfo, for the expansion kernels' device time and the peak of device memory in use.  The parent compares the two
routes' proofs byte for byte and prints one JSON line per route and one for the comparison.

--kernels: the two expansion kernels alone instead, nothing else on the device: 64 columns of 2^k cells per width through 64
zk_fr_from_uint calls and through one zk_fr_from_uint_batch call (HIP events around either; minimum of five after a warm-up).

usage: python tools/typed_dev_time.py [--k 20] [--shape 1000,150,150,100,9] [--repeat 5] [--kernels]"""
import argparse
import ctypes
import hashlib
import json
import os
import subprocess
import sys
import tempfile
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


class MemoryPeak:
    """peak of (total - free) device memory while running, sampled from a thread"""

    def __init__(self, lib, interval_s=0.002):
        self.hip = lib                                    # the HIP runtime's symbols resolve through the library that links it
        self.interval, self.peak, self.stop = interval_s, 0, threading.Event()

    def used(self):
        free, total = ctypes.c_size_t(), ctypes.c_size_t()
        if self.hip.hipMemGetInfo(ctypes.byref(free), ctypes.byref(total)) != 0:
            raise RuntimeError("hipMemGetInfo failed")
        return total.value - free.value

    def __enter__(self):
        self.peak = self.used()

        def loop():
            while not self.stop.is_set():
                self.peak = max(self.peak, self.used())
                time.sleep(self.interval)
        self.thread = threading.Thread(target=loop, daemon=True)
        self.thread.start()
        return self

    def __exit__(self, *exc):
        self.stop.set()
        self.thread.join()
        self.peak = max(self.peak, self.used())


def run_route(args):
    import bench_proof as bp
    import zkevm_circuits_amd as z
    from zkevm_circuits_amd import plonk
    ctx = z.Context(0)
    mem = MemoryPeak(z.lib())
    sa, sf, sp, sl, sd = (int(v) for v in args.shape.split(","))
    circ, blob, adv_m, inst_m, inst = bp.build_shape(ctx, args.k, sa, sf, sp, sl, sd)
    del adv_m                                             # the witness lives on the device as the integers it was made from
    n, u = circ.n, circ.u
    npub = [int(np.flatnonzero(np.asarray(a).reshape(-1, 4).any(axis=1))[-1]) + 1 if np.asarray(a).any() else 0 for a in inst_m]
    inst_m = [np.ascontiguousarray(a[:m]) for a, m in zip(inst_m, npub)]
    srs = ctx.srs_setup_with_s(args.k, np.frombuffer(plonk.fr_mont_bytes(0x5EC2E7), dtype=np.uint64).copy())
    pk = ctx.pk_create(srs, blob)
    ctx.sync()
    used_before = mem.used()
    narrow = {}
    for v in circ.advice_ints:
        assert v is not None, "a column of this shape is not held as integers"
        if v.ctypes.data not in narrow:                   # the shape's columns alias a few distinct arrays on the host
            narrow[v.ctypes.data] = np.ascontiguousarray(bp.narrowest_cells(v)[:u])
    cells = [narrow[v.ctypes.data] for v in circ.advice_ints]
    widths = [c.dtype.itemsize for c in cells]
    packed = [ctx.to_device(c) for c in cells]            # one buffer per column, as a witness kernel would leave them
    expanded = [ctx.alloc(n * 32) for _ in cells] if args.route == "a" else []
    if expanded:                                          # rows from usable_rows on are the session's; the caller's hold nothing
        zero = np.zeros((n - u, 4), dtype=np.uint64)
        for buf in expanded:
            ctx._ck(z.lib().zk_h2d(ctx.h, ctypes.c_void_p(buf.ptr + u * 32), zero.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(zero.nbytes)))
    ctx.sync()
    used_witness = mem.used()

    def prove():
        sess = ctx.proof_session(pk, inst_m, bytes(16), instance_slices=True)
        sess.set_multiopen(1)
        if args.route == "a":
            for src, w, dst in zip(packed, widths, expanded):
                ctx.fr_from_uint(src, w, u, dst)
            sess.advice_phase_dev(dict(enumerate(expanded)), in_place=False)
        else:
            sess.advice_phase_typed_dev({i: (b_, w) for i, (b_, w) in enumerate(zip(packed, widths))})
        return sess.finish()

    times, proof = [], b""
    for _ in range(args.repeat):
        ctx.sync()
        t0 = time.perf_counter()
        proof = prove()
        times.append(time.perf_counter() - t0)
    ctx.prof_reset()
    ctx.prof_enable(True)
    with mem:
        profiled = prove()
        ctx.sync()
    ctx.prof_enable(False)
    name = "fr_from_uint" if args.route == "a" else "fr_from_uint_batch"
    ms, launches = ctx.prof_get(name)
    assert profiled == proof
    with open(args.proof_out, "wb") as f:
        f.write(proof)
    later = times[1:] or times
    print(json.dumps({
        "route": args.route, "k": args.k, "shape": args.shape, "multiopen": "shplonk", "usable_rows": u,
        "columns_by_cell_bytes": {str(w): widths.count(w) for w in sorted(set(widths))},
        "create_proof_s": [round(t, 4) for t in times], "proof_s_min": round(min(later), 4), "proof_s_max": round(max(later), 4),
        "expansion_kernel": name, "expansion_device_ms": round(ms, 3), "expansion_launches": launches,
        "expansion_algorithmic_bytes": ctx.prof_get_bytes(name),
        "device_bytes_before_witness": used_before, "device_bytes_callers_witness": used_witness - used_before,
        "device_bytes_peak": mem.peak, "device_bytes_peak_caller_plus_session": mem.peak - used_before,
        "proof_bytes": len(proof), "proof_sha256": hashlib.sha256(proof).hexdigest()}), flush=True)
    for b_ in packed + expanded:
        b_.free()
    pk.destroy()
    srs.destroy()
    ctx.close()


def run_kernels(args):
    import zkevm_circuits_amd as z
    ctx = z.Context(0)
    n, count, res = 1 << args.k, 64, {"k": args.k, "columns": 64}
    for w in (1, 2, 4, 8, 16):
        src = [ctx.to_device(np.random.default_rng(c).integers(0, 255, size=n * w, dtype=np.uint8)) for c in range(count)]
        out = [ctx.alloc(n * 32) for _ in range(count)]
        for name in ("single", "batch"):
            ms = []
            for _ in range(6):
                ctx.sync()
                ctx.timer_start()
                if name == "single":
                    for s_, o_ in zip(src, out):
                        ctx.fr_from_uint(s_, w, n, o_)
                else:
                    ctx.fr_from_uint_batch(src, [w] * count, n, out)
                ms.append(ctx.timer_stop_ms())
            res[f"width{w}_{name}_ms"] = round(min(ms[1:]), 4)
            res[f"width{w}_{name}_TB_per_s"] = round(count * n * (w + 32) / min(ms[1:]) / 1e9, 3)
        for b_ in src + out:
            b_.free()
    print(json.dumps(res))
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, default=20)
    ap.add_argument("--shape", default="1000,150,150,100,9")
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--route", choices=["a", "b"], help="run one route in this process (what the parent starts)")
    ap.add_argument("--proof-out", help="with --route: where the proof bytes go")
    ap.add_argument("--kernels", action="store_true", help="time the two expansion kernels alone instead of the proofs")
    args = ap.parse_args()
    if args.kernels:
        return run_kernels(args)
    if args.route:
        return run_route(args)
    results, proofs = {}, {}
    with tempfile.TemporaryDirectory() as tmp:
        for route in ("a", "b"):                          # fresh processes, one after the other: nothing parked by one route is counted for the other
            path = os.path.join(tmp, f"proof_{route}.bin")
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--k", str(args.k), "--shape", args.shape, "--repeat", str(args.repeat),
                                  "--route", route, "--proof-out", path], stdout=subprocess.PIPE, text=True, check=True).stdout
            line = [ln for ln in out.splitlines() if ln.startswith("{")][-1]
            print(line, flush=True)
            results[route] = json.loads(line)
            proofs[route] = open(path, "rb").read()
    a, b_ = results["a"], results["b"]
    spread = lambda r: (r["proof_s_max"] - r["proof_s_min"]) / r["proof_s_min"]
    print(json.dumps({
        "proofs_equal_byte_for_byte": proofs["a"] == proofs["b"] and len(proofs["a"]) > 0,
        "proof_s_min_a": a["proof_s_min"], "proof_s_min_b": b_["proof_s_min"], "b_over_a": round(b_["proof_s_min"] / a["proof_s_min"], 4),
        "spread_a": round(spread(a), 4), "spread_b": round(spread(b_), 4),
        "expansion_device_ms_a": a["expansion_device_ms"], "expansion_device_ms_b": b_["expansion_device_ms"],
        "peak_bytes_a": a["device_bytes_peak_caller_plus_session"], "peak_bytes_b": b_["device_bytes_peak_caller_plus_session"],
        "peak_bytes_saved": a["device_bytes_peak_caller_plus_session"] - b_["device_bytes_peak_caller_plus_session"],
        "witness_bytes_as_fr": sum(a["columns_by_cell_bytes"].values()) * (1 << args.k) * 32}))
    if proofs["a"] != proofs["b"]:
        sys.exit("the two routes' proofs differ")


if __name__ == "__main__":
    main()

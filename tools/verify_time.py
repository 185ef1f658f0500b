"""Times zk_verify_proofs (the library's halo2 verify_proof) against the oracle verifier on the same proofs.

  python tools/verify_time.py [--batches 1,8,32] [--k 6] [--k20]

* a batch of B proofs of one small key (the three-phase SuperCircuit stand-in of tests/test_gpu_verify.py, SHPLONK, Poseidon),
  split into the steps zk_verify_proofs reports under ZK_VERIFY_TRACE=1: setup (gather), decode (device), replay (host, up to 16
  threads), msm (device), pairing (host); then oracle/plonk_verifier.verify on the same proofs, one after the other;
* --k20: a single verify of the EVM-style k = 20 proof (bench_proof.build_shape as tests/test_gpu_evm_shape.py builds it; needs
  about 64 GiB of host memory and a few minutes to prove).
One JSON line per measurement."""
import argparse
import json
import os
import re
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
os.environ["ZK_VERIFY_TRACE"] = "1"

import zkevm_circuits_amd as z  # noqa: E402
from oracle import cref, pairing as pr, params_file, plonk_verifier as pv  # noqa: E402
from zkevm_circuits_amd import plonk  # noqa: E402

S_SECRET = 0x5EC2E7
G2 = params_file.g2_raw_bytes(pr.G2_GEN)


class StderrSteps:
    """captures what the library writes to fd 2 and sums the [zk verify] marks per step"""

    def __enter__(self):
        sys.stderr.flush()
        self.f = tempfile.TemporaryFile(mode="w+b")
        self.saved = os.dup(2)
        os.dup2(self.f.fileno(), 2)
        return self

    def __exit__(self, *a):
        sys.stderr.flush()
        os.dup2(self.saved, 2)
        os.close(self.saved)
        self.f.seek(0)
        self.steps = {}
        for name, ms in re.findall(rb"\[zk verify\] (\w+)\s+([0-9.]+) ms", self.f.read()):
            self.steps[name.decode()] = self.steps.get(name.decode(), 0.0) + float(ms)
        self.f.close()


def timed_verify(ctx, vk, proofs, insts, kind, mo, s_g2, reps):
    ctx.verify_proofs(vk, proofs, insts, kind, mo, G2, s_g2)          # warm-up: pairing constants, MSM scratch
    best, steps = None, None
    for _ in range(reps):
        with StderrSteps() as cap:
            t0 = time.perf_counter()
            ok = ctx.verify_proofs(vk, proofs, insts, kind, mo, G2, s_g2)
            dt = (time.perf_counter() - t0) * 1e3
        assert ok
        if best is None or dt < best:
            best, steps = dt, cap.steps
    return best, steps


def small_batches(ctx, batches, k, reps):
    from test_gpu_verify import three_phase, _prove
    circ, _, _ = three_phase(k, 1)
    srs = ctx.srs_setup_with_s(k, cref.fr_const(S_SECRET))
    pk = ctx.pk_create(srs, circ.blob())
    proofs, insts = [], []
    try:
        com, rep = pk.vk(circ.F + len(circ.perm_cols))
        for s_ in range(max(batches)):
            c2, synth, inst = three_phase(k, s_ + 1)
            proofs.append(_prove(ctx, cref, pk, c2, synth, inst, bytes([s_ & 0xFF] * 16), "shplonk", "poseidon", "one"))
            insts.append(inst)
    finally:
        pk.destroy()
        srs.destroy()
    vk = z.VerifyingKey(circ.cs_blob(), com, rep)
    s_g2_pt = pr.ec_mul(pr.G2_GEN, S_SECRET)
    s_g2 = params_file.g2_raw_bytes(s_g2_pt)
    vk_points, vk_repr = cref.affine_from_mont(com), cref.from_mont(rep.reshape(1, 4))[0]
    for B in batches:
        mont = [[plonk.column_to_mont(c) for c in i] for i in insts[:B]]
        ms, steps = timed_verify(ctx, vk, proofs[:B], mont, z.TRANSCRIPT_POSEIDON, 1, s_g2, reps)
        t0 = time.perf_counter()
        for p_, i in zip(proofs[:B], insts[:B]):
            assert pv.verify(circ, vk_points, vk_repr, i, p_, s_g2_pt, multiopen="shplonk", transcript="poseidon")
        oracle_ms = (time.perf_counter() - t0) * 1e3
        print(json.dumps({"what": "batch", "k": k, "proofs": B, "proof_bytes": len(proofs[0]), "native_ms": round(ms, 3),
                          "steps_ms": {k_: round(v, 3) for k_, v in steps.items()}, "oracle_ms": round(oracle_ms, 1)}), flush=True)
    vk.destroy()


def k20(ctx, reps):
    import numpy as np
    import bench_proof as bp
    shape = (20, 1000, 150, 150, 100, 9)
    circ, blob, adv_m, inst_m, inst, rlc = bp.build_shape(ctx, *shape, dist="survey", phases=True, evm=dict(bp.EVM_DEFAULT))
    npub = [int(np.flatnonzero(np.asarray(a).reshape(-1, 4).any(axis=1))[-1]) + 1 if np.asarray(a).any() else 0 for a in inst_m]
    inst = [list(col[:m]) for col, m in zip(inst, npub)]
    inst_m = [np.ascontiguousarray(a[:m]) for a, m in zip(inst_m, npub)]
    srs = ctx.srs_setup_with_s(circ.k, cref.fr_const(S_SECRET))
    pk = ctx.pk_create(srs, blob)
    del blob
    adv_dev = [ctx.to_device(a) for a in adv_m]
    driver = bp.PhaseDriver(ctx, circ, adv_dev, rlc)
    try:
        com, rep = pk.vk(circ.F + len(circ.perm_cols))
        sess = ctx.proof_session(pk, inst_m, bytes(16), instance_slices=True)
        sess.set_multiopen(1)
        driver.run(sess)
        proof = sess.finish()
    finally:
        driver.free()
        for b_ in adv_dev:
            b_.free()
        pk.destroy()
        srs.destroy()
    vk = z.VerifyingKey(circ.cs_blob(), com, rep)
    s_g2_pt = pr.ec_mul(pr.G2_GEN, S_SECRET)
    ms, steps = timed_verify(ctx, vk, [proof], [inst_m], z.TRANSCRIPT_BLAKE2B, 1, params_file.g2_raw_bytes(s_g2_pt), reps)
    t0 = time.perf_counter()
    assert pv.verify(circ, cref.affine_from_mont(com), cref.from_mont(rep.reshape(1, 4))[0], inst, proof, s_g2_pt, multiopen="shplonk")
    oracle_ms = (time.perf_counter() - t0) * 1e3
    print(json.dumps({"what": "evm_k20_single", "proof_bytes": len(proof), "native_ms": round(ms, 3), "steps_ms": {k_: round(v, 3) for k_, v in steps.items()},
                      "oracle_ms": round(oracle_ms, 1)}), flush=True)
    vk.destroy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,8,32")
    ap.add_argument("--k", type=int, default=6)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--k20", action="store_true")
    a = ap.parse_args()
    cref.lib()
    ctx = z.Context(0)
    try:
        small_batches(ctx, [int(x) for x in a.batches.split(",")], a.k, a.reps)
        if a.k20:
            k20(ctx, a.reps)
    finally:
        ctx.close()


if __name__ == "__main__":
    main()

"""Times zk_verify_accumulators on 45 child snarks of the fixture-shaped circuit (the reference ChunkProof's constraint system at
k = 8, Poseidon, SHPLONK: what an aggregation layer hands to extract_accumulators_and_proof), split into the steps it reports
under ZK_VERIFY_TRACE=1, and next to it
  * the route there was before zk_msm_g1_segments: the same 90 coefficient vectors through 90 zk_msm_g1 calls after the same decode
    and replay (ZK_ACC_MSM_LOOP=1);
  * zk_verify_proofs on the same batch (one DualMSM and one pairing for all).

  python tools/acc_time.py [--proofs 45] [--reps 12]

Medians over --reps runs after one warm-up each; one JSON line per route."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
os.environ["ZK_VERIFY_TRACE"] = "1"

import zkevm_circuits_amd as z  # noqa: E402
from oracle import cref  # noqa: E402
from verify_time import StderrSteps  # noqa: E402


def measure(what, call, reps):
    call()
    walls, steps = [], {}
    for _ in range(reps):
        with StderrSteps() as cap:
            t0 = time.perf_counter()
            call()
            walls.append((time.perf_counter() - t0) * 1e3)
        for k_, v in cap.steps.items():
            steps.setdefault(k_, []).append(v)
    print(json.dumps({"what": what, "reps": reps, "median_ms": round(statistics.median(walls), 3), "min_ms": round(min(walls), 3), "max_ms": round(max(walls), 3),
                      "steps_median_ms": {k_: round(statistics.median(v), 3) for k_, v in steps.items()}}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--proofs", type=int, default=45)
    ap.add_argument("--reps", type=int, default=12)
    a = ap.parse_args()
    from test_gpu_accumulators import G2, S_G2, S_SECRET, _mont_cols, _prove, build_reference_cs
    cref.lib()
    ctx = z.Context(0)
    circ, adv, inst = build_reference_cs(8, 1)
    srs = ctx.srs_setup_with_s(8, cref.fr_const(S_SECRET))
    pk = ctx.pk_create(srs, circ.blob())
    try:
        com, rep = pk.vk(circ.F + len(circ.perm_cols))
        proofs = [_prove(ctx, pk, adv, inst, bytes([s_ + 1] * 16), "shplonk", "poseidon", slices=True) for s_ in range(a.proofs)]
    finally:
        pk.destroy()
        srs.destroy()
    vk = z.VerifyingKey(circ.cs_blob(), com, rep)
    insts = [_mont_cols(inst)] * a.proofs
    results = {}

    def accumulators(tag):
        def call():
            lhs, rhs, ok = ctx.verify_accumulators(vk, proofs, insts, z.TRANSCRIPT_POSEIDON, 1)
            assert all(ok)
            results[tag] = (lhs.copy(), rhs.copy())
        return call
    try:
        for _round in range(2):               # both routes twice, interleaved: drift of the machine shows as a difference between the rounds
            os.environ.pop("ZK_ACC_MSM_LOOP", None)
            measure("verify_accumulators, one segmented MSM", accumulators("seg"), a.reps)
            os.environ["ZK_ACC_MSM_LOOP"] = "1"
            measure("verify_accumulators, one zk_msm_g1 call per vector", accumulators("loop"), a.reps)
        os.environ.pop("ZK_ACC_MSM_LOOP", None)
        assert (results["seg"][0] == results["loop"][0]).all() and (results["seg"][1] == results["loop"][1]).all()
        measure("verify_proofs", lambda: ctx.verify_proofs(vk, proofs, insts, z.TRANSCRIPT_POSEIDON, 1, G2, S_G2), a.reps)
    finally:
        vk.destroy()
        ctx.close()


if __name__ == "__main__":
    main()

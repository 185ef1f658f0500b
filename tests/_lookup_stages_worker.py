"""Worker of tests/test_gpu_lookup_stages.py: one rank of a sharded proving session over a circuit with several lookup
arguments (tests/_sharded_proof_worker.py's set-up).  Every rank proves twice, with the fused lookup stages and under
ZK_LOOKUP_FUSED=0, and writes <out_dir>/proof_<rank>_<fused>.bin and the profiling scopes that were recorded to
<out_dir>/scopes_<rank>_<fused>.json; rank 0 adds the proof of an unsharded session."""
import datetime
import json
import os
import sys

import numpy as np
import torch.distributed as dist

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import zkevm_circuits_amd as z  # noqa: E402
from zkevm_circuits_amd import plonk, sharding  # noqa: E402
from plonk_fixtures import build_multi_lookup_circuit  # noqa: E402


def main():
    out_dir, k = sys.argv[1], int(sys.argv[2])
    dist.init_process_group(backend=os.environ.get("ZK_TEST_BACKEND", "gloo"), timeout=datetime.timedelta(seconds=150))
    rank = dist.get_rank()
    ctx = z.Context(0)
    circ, adv, inst = build_multi_lookup_circuit(k, seed=5, n_inputs=7, gate_degree=3)
    srs = ctx.srs_setup_with_s(k, np.frombuffer(plonk.fr_mont_bytes(0x5EC2E7), dtype=np.uint64).copy())
    pk = ctx.pk_create(srs, circ.blob())
    adv_m = [plonk.column_to_mont(c) for c in adv]
    inst_m = [plonk.column_to_mont(c) for c in inst]

    def prove(sharded: bool) -> bytes:
        sess = ctx.proof_session(pk, inst_m, bytes(range(16)))
        sess.set_multiopen(1)
        keep = sharding.shard_session(sess) if sharded else None
        sess.advice_phase({i: c for i, c in enumerate(adv_m)})
        proof = sess.finish()
        del keep
        return proof

    ctx.prof_enable(True)
    for fused in ("1", "0"):
        os.environ["ZK_LOOKUP_FUSED"] = fused
        ctx.prof_reset()
        proof = prove(True)
        open(os.path.join(out_dir, f"proof_{rank}_{fused}.bin"), "wb").write(proof)
        json.dump(ctx.prof_names(), open(os.path.join(out_dir, f"scopes_{rank}_{fused}.json"), "w"))
    os.environ.pop("ZK_LOOKUP_FUSED")
    if rank == 0:
        open(os.path.join(out_dir, "proof_single.bin"), "wb").write(prove(False))
    dist.barrier()
    pk.destroy()
    srs.destroy()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()

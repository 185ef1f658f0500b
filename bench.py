#!/usr/bin/env python
"""bench.py -- BASELINE.json's metric: "SuperCircuit proof-gen wall-clock (s) at k; MSM Mscalar/s + NTT Gfield-op/s vs HBM roofline".

A "step" is ONE FULL PROOF of the SuperCircuit-shape circuit at k = 20 (BASELINE configs[3] -- it fits one MI355X: ~185 of
288 GB -- stand-in circuit of SURVEY 8d config 4: 1000 advice / 150 fixed / 150 permutation columns, 100 lookups, degree 9;
the reference's own witness needs its Rust + Go toolchain, so every number here is "synthetic-shape"):
  * witness cells distributed as SURVEY 8d prescribes -- ~60 % zero / ~30 % below 2^16 / 10 % uniform field elements PER CELL;
  * THREE advice phases with the SuperCircuit's challenges (evm_word, keccak_input after the first, lookup_input after the
    second [REF zkevm-circuits/src/util.rs:120-133]); the two challenge-dependent columns are computed between the phases;
  * SHPLONK + Blake2b as at [REF circuit-benchmarks/src/super_circuit.rs:117-132];
  * the witness columns are RESIDENT IN HBM when the timed region starts (zk_proof_advice_phase_dev).  The same proof from
    page-locked host memory (what a Rust caller hands over) is timed beside it: `pcie_inclusive_s`.
`value` = seconds per proof over the K timed steps (lower is better); `ms_per_step` = the same in milliseconds.

A plain run (`python bench.py --gpus 1 --steps K --warmup W`) does only what that figure needs: it builds the circuit, key and
resident witness, runs W warm-up proofs and the K timed ones, and prints one short line (metric, value, unit, ms_per_step,
dtype, config, the last proof's size and SHA-256).  `--dump-outputs DIR` writes what the last timed proof handed its caller:
DIR/proof.npy (the proof's bytes) and DIR/challenges.npy (the three challenges the advice phases returned, 32 little-endian
bytes each), both float32; the inputs are seeded, so two builds can be compared output for output.

`--full` adds everything else, as before: the proof checked by the oracle verifier (outside the timed region), HIP events on
the kernel classes over the timed region, and the side measurements.  The full line carries
  * `roofline`   -- the dominant kernel class of the proof, the size-2^20 NTT (k_ntt_pass + k_ntt_last), HIP events over the
                    timed region; `rooflines` -- MSM bucket accumulation and the quotient evaluator beside it;
  * `proof_roofline` -- sum of the algorithmic bytes of the proof's stages (SURVEY 8d, K1-K10 counts) / wall-clock / 8 TB/s;
  * `msm_ntt`    -- BASELINE configs[1]: MSM 2^20 Mscalar/s and NTT 2^20 Gfield-op/s over rotating columns (what rounds 1-3 headlined);
  * `cpu_baseline` -- halo2's create_proof restated on the host cores, Keccak shape at k = 18 (BASELINE configs[2]), with the GPU
                    time of the same circuit / witness / seed (same bytes required);
  * `proof`      -- the other shapes and witness distributions, one prover process each.

`python bench.py --gpus N` launches itself as N ranks (torch.distributed.run, 127.0.0.1) when not started under a launcher.
N > 1: the SAME workload -- one proof of the same three-phase circuit, witness resident and handed over in place --
sharded over the ranks: a rank holds the columns it owns, commits them and all-gathers them device to device over the library's RCCL
communicator; quotient by (degree class, coset); strong scaling, value = seconds per proof, same `roofline` record from rank 0.
"""
import argparse
import json
import os
import socket
import subprocess
import sys
import time

os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

K = 20
N = 1 << K
NCOL = 32                  # msm_ntt section: 32 x 32 MiB committed + 32 x 32 MiB transformed (2 GiB, eight times the Infinity Cache)
# ZK_BENCH_K: test switch (tests/test_gpu_bench_sharded.py) -- the SAME code path over the same column counts at a small k, so that
# `bench.py --gpus 2` can run end to end with two ranks sharing the test box's one GPU.  The driver never sets it.
HEADLINE_K = int(os.environ.get("ZK_BENCH_K", "20"))
SC_SHAPE = (HEADLINE_K, 1000, 150, 150, 100, 9)      # k, advice, fixed, permutation columns, lookups, degree
HBM_PEAK_GBS = 8000.0      # MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec
MULPEAK_G = 169.0          # measured 9x29-bit Montgomery products/s (G) of the library's own product routine (tools/ubench.hip)
MAD_PEAK_T = 30.4          # measured v_mad_u64_u32 lane-ops/s (T), tools/ubench.hip: the hardware-side bound
MADS_PER_PRODUCT = 162     # v_mad_u64_u32 per 9 x 29-bit Montgomery product (81 operand + 81 reduction, counted in the ISA)
MADS_PER_MIXED_ADD = 1476  # per XYZZ mixed addition (csrc/ec29.hip.hpp madd29)
R_MOD = 0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001
DTYPE = "u32x8 limbs (254-bit modular integer, Montgomery)"
METRIC = f"SuperCircuit-shape proof-gen wall-clock (s) at k = {HEADLINE_K}"
# Two stand-ins of the same outer shape (1000 advice / 150 fixed / 150 permutation columns, 100 lookups, degree 9):
#   "evm"   (the headline since round 6) -- 160 of the advice columns are the step columns of an EVM-style execution-state machine:
#           >= 5 000 constraints  q_usable * q_step * state_selector_s * (constraint * condition)  of degree 5 .. 9 reading them at
#           rotations 0 / 1 / 2 [REF zkevm-circuits/src/evm_circuit/execution.rs:832-851, util/constraint_builder.rs:33-34,322-341,
#           param.rs:10], lookups with 4- / 6- / 8-column tuples; the other 840 columns keep the triple gates;
#   "plain" (rounds 1-5's headline) -- 333 column triples under q (a b - c) and q (a + b - c(w X)), ONE degree-9 gate on three
#           columns, two-column lookups: the friendliest degree structure that still says "degree 9" (round-5 review).
# The slower, and the one closer to the reference's constraint system, is `value`; the other is `proof.supercircuit_shape_k20_plain`.
HEADLINE_SHAPE = os.environ.get("ZK_BENCH_SHAPE", "evm")
SHAPE_NOTE = {"evm": "EVM-style: 160 step columns under >= 5 000 constraints q_usable * q_step * state_selector * (constraint * condition) of degree 5..9 at rotations 0/1/2, "
                     "840 columns under degree-2/3 triple gates, lookups of 4/6/8-column tuples",
              "plain": "rounds 1-5's shape: 333 column triples under degree-2/3 gates, one degree-9 gate on three columns, two-column lookups"}


def workload_text(shape):
    return (f"BASELINE configs[3] stand-in: SuperCircuit shape k = {HEADLINE_K} (1000 advice / 150 fixed / 150 permutation columns, 100 lookups, degree 9; {SHAPE_NOTE[shape]}), "
            "three advice phases, witness 60/30/10 per cell on the non-step columns (SURVEY 8d), SHPLONK, Blake2b; one full proof per step")


WORKLOAD = workload_text(HEADLINE_SHAPE)


class _NoTorch:
    """stands in for torch where it is not loaded (`--proof-worker`, a plain single-GPU run): the library's own sync is the fence"""
    class cuda:
        @staticmethod
        def synchronize():
            pass


def relaunch_under_launcher(args) -> int:
    """`--gpus N` without a launcher: start N ranks of this script (one per GPU) and relay their output."""
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}", "--master-addr", "127.0.0.1", "--master-port", str(port),
           os.path.abspath(__file__), "--gpus", str(args.gpus), "--steps", str(args.steps), "--warmup", str(args.warmup), "--batch", str(args.batch)]
    for flag in ("full", "no_cpu_baseline", "no_proof", "no_verify", "no_msm_ntt"):
        if getattr(args, flag, False):
            cmd.append("--" + flag.replace("_", "-"))
    if getattr(args, "dump_outputs", None):
        cmd += ["--dump-outputs", os.path.abspath(args.dump_outputs)]
    return subprocess.call(cmd)


def dump_outputs(out_dir, proof, challenges):
    """what the timed path handed its caller in the last timed step, as float32 arrays (exact: every value is a byte)"""
    import numpy as np

    os.makedirs(out_dir, exist_ok=True)
    np.save(os.path.join(out_dir, "proof.npy"), np.frombuffer(proof, dtype=np.uint8).astype(np.float32))
    ch = np.ascontiguousarray(np.asarray(challenges, dtype=np.uint64).reshape(-1, 4))
    np.save(os.path.join(out_dir, "challenges.npy"), ch.view(np.uint8).reshape(-1, 32).astype(np.float32))


def fr_mont(v: int):
    import numpy as np
    x = (v << 256) % R_MOD
    return np.array([(x >> (64 * i)) & ((1 << 64) - 1) for i in range(4)], dtype=np.uint64)


def hbm_roof(kernel, alg_bytes, ms, note, products=None, launches=None):
    """roofline record of one kernel class: algorithmic bytes / measured time against the HBM peak (the metric's roof) plus, where
    given, the integer-ALU roof that binds"""
    if not ms:
        return None
    ach = alg_bytes / (ms * 1e-3) / 1e9
    rec = {"kernel": kernel, "bound": "hbm", "achieved": round(ach, 2), "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": round(ach / HBM_PEAK_GBS, 5),
           "avg_launch_ms": round(ms, 4), "algorithmic_bytes_per_launch": int(alg_bytes), "note": note, "traffic": None}
    if launches is not None:
        rec["launches_timed"] = launches
    if products:
        gps = products / (ms * 1e-3) / 1e9
        rec["alu"] = {"unit": "G Montgomery-product equivalents/s (162 multiply-adds each)", "achieved": round(gps, 1), "peak_own_routine": MULPEAK_G, "frac_own_routine": round(gps / MULPEAK_G, 3),
                      "peak_v_mad_u64_u32": round(MAD_PEAK_T * 1e3 / MADS_PER_PRODUCT, 1), "frac_v_mad_u64_u32": round(gps / (MAD_PEAK_T * 1e3 / MADS_PER_PRODUCT), 3)}
    return rec


def committed_traffic(key):
    """PMC traffic (FETCH_SIZE + WRITE_SIZE per launch) from the newest committed rocprofv3 --pmc passes under profiles/"""
    for tname in ("traffic_r06.json", "traffic_r05.json", "traffic_r04.json", "traffic_r03.json", "traffic_r02.json"):
        tpath = os.path.join(ROOT, "profiles", tname)
        if os.path.exists(tpath):
            try:
                v = json.load(open(tpath)).get(key)
            except Exception:
                v = None
            if v:
                return v, tname
    return None, None


def proof_algorithmic_bytes(circ, shplonk=True, uniform_random_poly=False):
    """SURVEY 8d "ALGORITHMIC bytes per unit of work", summed over one create_proof with the K1-K10 counts of this circuit:
    what a prover that touched every operand exactly once per stage would move.  n = 2^k rows of 32 B."""
    n = circ.n
    d, A, F, I, P, L = circ.degree(), circ.A, circ.F, circ.I, len(circ.perm_cols), len(circ.lookups)
    C = (P + d - 3) // (d - 2) if P else 0
    cosets = 1 << (circ.extended_k() - circ.k)
    inputs = sum(len(lk.inputs) for lk in circ.lookups)
    committed_lagrange = A + 2 * L + C                               # advice, m and phi per lookup, Z per chunk
    msm = committed_lagrange + (d - 1) + (2 if shplonk else 0) + (1 if uniform_random_poly else 0)
    opened = A + F + P + C + 2 * L + 2                               # polynomials the multi-open touches (h and the random polynomial included)
    b = {
        "msm (K1): 96 B x n per commitment": 96 * n * msm,
        "lagrange_to_coeff (K2): 64 B x n per polynomial": 64 * n * (committed_lagrange + I),
        "coset transforms (K3): 64 B x n per polynomial per coset": 64 * n * (A + I + C + 2 * L) * cosets,
        "quotient evaluation (K4/K5): 32 B x n x (columns + 1) per coset": 32 * n * (A + F + I + P + C + 2 * L + 3 + 1) * cosets,
        "extended_to_coeff of h (K6): 64 B x n per coset": 64 * n * cosets,
        "permutation products (K7): ratio programs + inversion + scan": (32 * n * (2 * P + 2) + 64 * n * 2) * 1 if not C else (32 * n * (2 * P + 2 * C) + 2 * 64 * n * C),
        "lookups (K8): compression, multiplicities, inversion, scan": 32 * n * (3 * inputs + 3 * L) + 3 * 64 * n * L,
        "evaluations (K9): 32 B x n per opened polynomial": 32 * n * opened,
        "multi-open (K10/K11): two linear combinations over the opened polynomials": 2 * 32 * n * (opened + 1),
    }
    return b


def class_program_operands(circ):
    """memory operands (column reads + parked values read back) and parked values written per row of every degree class's compiled
    program, out of zk_host_quotient_plan on the circuit's constraint system (the plan zk_proof_finish follows under the knobs in force)"""
    import ctypes

    import numpy as np

    from zkevm_circuits_amd import binding
    lib = binding.lib()
    blob = circ.cs_blob()
    E = circ.extended_k() - circ.k
    out = []
    for e in range(E + 1):
        summ = np.zeros(8 + 8 * (E + 1), dtype=np.uint32)
        cnt = ctypes.c_uint32()
        ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)
        if lib.zk_host_quotient_plan(blob, ctypes.c_size_t(len(blob)), ptr(summ), ctypes.c_size_t(summ.size), ctypes.c_uint32(e), None, ctypes.c_size_t(0), ctypes.byref(cnt)) != 0:
            return None
        words = np.zeros(max(3 * cnt.value, 3), dtype=np.uint32)
        lib.zk_host_quotient_plan(blob, ctypes.c_size_t(len(blob)), ptr(summ), ctypes.c_size_t(summ.size), ctypes.c_uint32(e), ptr(words), ctypes.c_size_t(words.size), ctypes.byref(cnt))
        ops = words[:3 * cnt.value:3]
        out.append({"reads": int(((ops == 1) | (ops == 13)).sum()), "parks": int((ops == 12).sum()), "products": int(summ[8 + 8 * e + 2]), "used": int(summ[8 + 8 * e])})
    return out


def device_sync(ctx, torch):
    # the library's streams belong to the HIP runtime it links (/opt/rocm), torch's to the one torch bundles:
    # torch.cuda.synchronize() alone would not wait for what the library left in flight
    ctx.sync()
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------ the headline, N = 1 and N > 1 alike
def headline(args, torch, rank=0, world=1, dist=None, local_rank=0, shared_gpu=False, shape=None, side=True, project=None, full=True):
    """One full proof per step, the same circuit / witness / phases / hand-over for every N.  full=False (a plain run): the timed
    proofs and the short line only -- no HIP events, no verification, no side measurements.  N > 1: ONE proof sharded
    over the ranks -- a rank keeps only the witness columns it OWNS resident (position j of a phase's columns, j % N == rank), commits
    them and sends them to the others device to device; the 64-byte commitments are all-gathered per transcript round; the quotient is
    split by (degree class, coset).  Exchanges: the library's own RCCL communicator (csrc/comm.hip; its 128-byte id travels over the
    launcher's process group, which otherwise carries only the barriers), or torch.distributed gloo callbacks when the ranks share one
    GPU (test boxes: RCCL ranks cannot share a device).  Timing: W warm-up proofs, then K proofs between barrier + synchronize on both
    sides, MAX over the ranks."""
    import numpy as np

    import bench_proof as bp
    import zkevm_circuits_amd as z

    ctx = z.Context(local_rank)
    shard = None
    if world > 1:
        from zkevm_circuits_amd import sharding as shard
        if not shared_gpu:
            if os.environ.get("MASTER_ADDR", "127.0.0.1") in ("127.0.0.1", "localhost", "::1"):
                os.environ.setdefault("NCCL_SOCKET_IFNAME", "lo")       # one node, rendezvous over loopback: RCCL's bootstrap must not go looking for another interface
            shard.comm_init_from_torch(ctx)
    shape = shape or HEADLINE_SHAPE
    t0 = time.perf_counter()
    evm = None
    if shape == "evm":
        evm = dict(bp.EVM_DEFAULT)
        if HEADLINE_K < 14:          # the test switch (ZK_BENCH_K): the same code path with a block that fits the rows
            evm.update(states=8, per_state=16, input_cols=8, cond_cols=2)
    circ, blob, adv_m, inst_m, inst, rlc = bp.build_shape(ctx, *SC_SHAPE, dist="survey", phases=True, evm=evm)
    t_build = time.perf_counter() - t0
    dist_cells = bp.cell_distribution(adv_m[:SC_SHAPE[1] - 2])
    npub = [int(np.flatnonzero(np.asarray(a).reshape(-1, 4).any(axis=1))[-1]) + 1 if np.asarray(a).any() else 0 for a in inst_m]
    inst = [list(col[:m]) for col, m in zip(inst, npub)]
    inst_m = [np.ascontiguousarray(a[:m]) for a, m in zip(inst_m, npub)]
    S = 0x5EC2E7
    srs = ctx.srs_setup_with_s(circ.k, fr_mont(S))
    t0 = time.perf_counter()
    pk = ctx.pk_create(srs, blob)
    ctx.sync()
    t_keygen = time.perf_counter() - t0
    del blob
    plan = pk.quotient_plan()
    # the witness, resident in HBM: one device buffer per advice column this rank owns (aliased host arrays become distinct device
    # columns); a rank that does not own a_0 / b_0 keeps private copies of them for the two challenge-dependent columns
    t0 = time.perf_counter()
    owned = bp.owned_columns(circ, rank, world)
    adv_dev = {c: ctx.to_device(adv_m[c]) for c in sorted(owned | {0, 1, rlc["w"], rlc["t"]})}
    ctx.sync()
    t_upload = time.perf_counter() - t0
    driver = bp.PhaseDriver(ctx, circ, adv_dev, rlc, owned=owned if world > 1 else None)
    state = {}

    def step():
        sess = ctx.proof_session(pk, inst_m, bytes(16), instance_slices=True)
        sess.set_multiopen(1)
        keep = None
        if world > 1:
            keep = shard.shard_session_device(sess) if shared_gpu else sess.set_sharding_comm()
        state["challenges"] = driver.run(sess)
        state["proof"] = sess.finish()
        del keep

    def fence():
        if dist is not None:
            dist.barrier()
        device_sync(ctx, torch)

    # the same proof from page-locked HOST memory (what a Rust caller of create_proof holds): zk_proof_advice_phase, 33.5 GB over PCIe inside the proof
    host = {}

    def host_setup():
        if host:
            return
        pinned = {}
        for a in adv_m[:SC_SHAPE[1] - 2]:
            if id(a) not in pinned:
                pinned[id(a)] = ctx.host_alloc(a.shape)
                pinned[id(a)][:] = a
        host["pinned"] = pinned
        host["cols"] = [pinned[id(a)] for a in adv_m[:SC_SHAPE[1] - 2]]
        host["w"], host["t"] = ctx.host_alloc((circ.n, 4)), ctx.host_alloc((circ.n, 4))

    def host_teardown():
        if not host:
            return
        for a in list(host["pinned"].values()) + [host["w"], host["t"]]:
            ctx.host_free(a)
        host.clear()

    def step_host():
        host_cols, w_h, t_h = host["cols"], host["w"], host["t"]
        sess = ctx.proof_session(pk, inst_m, bytes(16), instance_slices=True)
        sess.set_multiopen(1)
        ph = circ.advice_phase
        ch0 = sess.advice_phase({i: host_cols[i] for i in range(circ.A - 2) if ph[i] == 0})
        driver._rlc(0, ch0[0], rlc["w"])
        w_h[:] = adv_dev[rlc["w"]].download((circ.n, 4))          # a host caller synthesises the RLC column on the host; here it comes back from the device
        ch1 = sess.advice_phase({**{i: host_cols[i] for i in range(circ.A - 2) if ph[i] == 1}, rlc["w"]: w_h})
        driver._rlc(rlc["w"], ch1[0], rlc["t"])
        t_h[:] = adv_dev[rlc["t"]].download((circ.n, 4))
        sess.advice_phase({**{i: host_cols[i] for i in range(circ.A - 2) if ph[i] == 2}, rlc["t"]: t_h})
        state["challenges"] = list(ch0) + list(ch1)
        state["proof"] = sess.finish()

    # record runs (tools/gpu_r6_record.sh): ZK_BENCH_KIND=host makes the TIMED proofs the host-memory kind, so that a kernel trace holds one kind only
    timed_step = step
    if os.environ.get("ZK_BENCH_KIND") == "host" and world == 1:
        host_setup()
        timed_step = step_host

    def teardown():
        host_teardown()
        driver.free()
        for b_ in adv_dev.values():
            b_.free()
        pk.destroy()
        srs.destroy()
        if world > 1 and not shared_gpu:
            ctx.comm_destroy()
        ctx.close()

    for _ in range(args.warmup):
        timed_step()
    fence()
    if full:
        ctx.prof_reset()
        ctx.prof_enable(2)       # HIP events around the kernel classes of the proof (MSM classes, NTT passes, quotient evaluator)
    t0 = time.perf_counter()
    for _ in range(args.steps):
        timed_step()
    fence()
    elapsed = time.perf_counter() - t0
    if full:
        ctx.prof_enable(False)
    if dist is not None:         # the slowest rank's clock
        box = [None] * world
        dist.all_gather_object(box, elapsed)
        elapsed = max(box)
    per_proof = elapsed / args.steps
    if getattr(args, "dump_outputs", None) and rank == 0:
        dump_outputs(args.dump_outputs, state["proof"], state.get("challenges", []))
    config = {"workload": workload_text(shape), "k": circ.k, "advice": circ.A, "fixed": circ.F, "permutation_columns": len(circ.perm_cols), "lookups": len(circ.lookups),
              "degree": circ.degree(), "extended_k": circ.extended_k(), "advice_phases": circ.num_phases(), "advice_columns_per_phase": [circ.advice_phase.count(p) for p in range(circ.num_phases())],
              "challenges": len(circ.challenge_phase), "advice_queries": len(circ.advice_queries), "fixed_queries": len(circ.fixed_queries),
              "witness_cell_distribution": dist_cells,
              "rows_with_an_active_lookup": round(float(np.asarray(rlc["q_lk"]).reshape(-1, 4).any(axis=1).mean()), 4),
              "rows_with_a_copy_constraint_per_column": round(len(set(r for pair in circ.copies for (_, _, r) in pair)) / circ.n, 5),
              "witness_residency": "HBM (device buffers handed to zk_proof_advice_phase_dev, in place: the session writes its blinding rows into them)"
                                   + ("; every rank holds the columns it owns, the others reach it device to device" if world > 1 else ""),
              "multiopen": "shplonk", "transcript": "blake2b",
              "vanishing_random_polynomial": "constant 1 (as the reference's own proofs)",
              "parallelism": "single GPU" if world == 1 else
                             f"one proof sharded x{world}: commitments by column, quotient by (degree class, coset), 64-byte commitments and witness columns all-gathered "
                             + ("over torch.distributed gloo callbacks (the ranks share one GPU: test box)" if shared_gpu else "over the library's RCCL communicator (xGMI)")}
    head = {"metric": METRIC, "value": round(per_proof, 4), "unit": "s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(per_proof * 1e3, 2),
            "higher_is_better": False, "scaling": "strong", "vs_baseline": None, "dtype": DTYPE, "data": "synthetic-shape", "config": config}
    if not full:
        out = dict(head, extra={"proof_bytes": len(state["proof"]), "proof_sha256": __import__("hashlib").sha256(state["proof"]).hexdigest(), "shape": shape,
                                "keygen_pk_s": round(t_keygen, 3), "witness_upload_s_outside_timing": round(t_upload, 2), "host_circuit_build_s": round(t_build, 2)})
        teardown()
        return out
    prof = {name: ctx.prof_get(name) for name in ctx.prof_names()}
    prof_bytes = {name: ctx.prof_get_bytes(name) for name in prof}

    # ---- outside the timed region: the same proof with the two commitment paths that read structure out of the data turned off
    # (permutation products by their run ends, lookup sums through their first differences: csrc/runs.hip) -- what a circuit
    # with a copy constraint on most rows and every lookup switched on everywhere would pay
    quick = os.environ.get("ZK_BENCH_QUICK") == "1" or not side          # A/B runs (tools/gpu_ab.sh): the timed proofs only, no side measurements
    proof_timed = state["proof"]

    def under(knobs, note):
        """the same proof under measurement knobs (outside the timed region): second of two runs, bytes compared"""
        if os.environ.get("ZK_BENCH_QUICK") == "1":
            return {"error": "skipped (ZK_BENCH_QUICK)"}
        try:
            os.environ.update(knobs)
            tb = []
            for _ in range(2):
                fence()
                t1 = time.perf_counter()
                step()
                fence()
                tb.append(time.perf_counter() - t1)
            rec = {"value": round(tb[-1], 4), "unit": "s", "same_proof_bytes": state["proof"] == proof_timed, "note": note}
            if "ZK_QUOTIENT_SPLIT" in knobs:
                rec["plan"] = pk.quotient_plan()
            return rec
        except Exception as e:
            return {"error": repr(e)}
        finally:
            for k_ in knobs:
                os.environ.pop(k_, None)
    blind = under({"ZK_MSM_RUNS": "0", "ZK_MSM_DIFF": "0"}, "ZK_MSM_RUNS=0 ZK_MSM_DIFF=0: every permutation product and lookup sum committed as a dense column")
    # ... and with the degree classes off: every constraint evaluated on all 2^(extended_k - k) cosets, every column transformed to all
    # of them -- what halo2's evaluate_h does, and what a circuit whose every column is read by a degree-9 constraint pays anyway
    degree_blind = under({"ZK_QUOTIENT_SPLIT": "0", "ZK_QUOTIENT_ADDSPLIT": "0"},
                         "ZK_QUOTIENT_SPLIT=0 ZK_QUOTIENT_ADDSPLIT=0: one degree class -- every constraint and every column on all 8 cosets (halo2's evaluate_h); the class-program compiler stays on")
    state["proof"] = proof_timed
    # ---- the proof is checked (rank 0), the same proof is made from page-locked host memory (N = 1)
    verified = None
    if not args.no_verify and rank == 0:
        from oracle import cref, pairing as pr, plonk_verifier as pv
        com, rep = pk.vk(circ.F + len(circ.perm_cols))
        verified = bool(pv.verify(circ, cref.affine_from_mont(com), cref.from_mont(rep.reshape(1, 4))[0], inst, state["proof"], pr.ec_mul(pr.G2_GEN, S), multiopen="shplonk"))
    pcie = None
    if world == 1 and not quick:
        try:
            host_setup()
            times = []
            for _ in range(2):
                t1 = time.perf_counter()
                step_host()
                times.append(time.perf_counter() - t1)
            pcie = {"value": round(min(times), 4), "unit": "s", "same_proof_bytes": state["proof"] == proof_timed,
                    "note": "the same proof with the witness in page-locked HOST memory (zk_proof_advice_phase): 33.5 GB cross PCIe inside the proof; what a Rust caller of "
                            "create_proof pays today.  Never `value` (inputs resident in HBM)."}
            state["proof"] = proof_timed
        except Exception as e:       # the headline must survive this side measurement
            pcie = {"error": repr(e)}
        finally:
            host_teardown()

    # ---- what ONE rank of an N-GPU run of this proof computes, measured here: rank 0 of N = 2 / 4 / 8 emulated on this GPU
    # (zkevm-circuits_amd/sharding.EmulatedRank: own commitments, every column's transforms, the (degree class, coset) pairs the rank
    # is dealt, everything the session replicates; the exchanges served locally, so NO communication time is in it).  A projection
    # of the compute side of the scaling curve, not a measurement of N GPUs -- the driver's SCALE run is that.
    projected = None
    if world == 1 and (not quick if project is None else project):
        projected = {"note": "wall-clock of the SLOWEST rank's share (every rank emulated in turn: `by_rank_s`) of the SAME proof sharded over N ranks, emulated on one GPU (peers' columns served from the resident witness, their commitments and "
                             "quotient pairs and lookup columns replaced by stand-ins: the emulated proof is not valid); excludes every byte that would cross xGMI -- `exchange_gb_in` says how many would arrive at the rank",
                     "rank_device_s": {}, "exchange_gb_in": {}}
        try:
            from zkevm_circuits_amd import sharding as shard_mod
            projected["by_rank_s"] = {}
            for nn in (2, 4, 8):
                # EVERY rank of the N is emulated in turn (the (class, coset) pairs are dealt by cost: which rank is the busiest depends on the deal); `rank_device_s` is the slowest
                per_rank = []
                for rr in range(nn):
                    owned_n = bp.owned_columns(circ, rr, nn)
                    emu = shard_mod.EmulatedRank(ctx, circ, adv_dev, rr, nn)
                    drv = bp.PhaseDriver(ctx, circ, adv_dev, rlc, owned=owned_n)
                    tt = []
                    for _ in range(2 if rr == 0 else 1):                     # the first run of an N also fills what the key caches per sharded layout
                        fence()
                        t1 = time.perf_counter()
                        sess = ctx.proof_session(pk, inst_m, bytes(16), instance_slices=True)
                        sess.set_multiopen(1)
                        emu.attach(sess)
                        drv.run(sess, before_phase=emu.begin_phase)
                        sess.finish()
                        fence()
                        tt.append(time.perf_counter() - t1)
                    drv.free()
                    per_rank.append(round(min(tt), 4))
                projected["by_rank_s"][str(nn)] = per_rank
                projected["rank_device_s"][str(nn)] = max(per_rank)
                owned_n = bp.owned_columns(circ, 0, nn)
                pairs = sum((1 << e_) for e_, c_ in enumerate(plan["classes"]) if c_["used"])
                lk_cols = 2 * len(circ.lookups) * (nn - 1) / nn if len(circ.lookups) >= nn else 0       # m and phi of the other ranks' lookup arguments (round 6: arguments split over the ranks)
                projected["exchange_gb_in"][str(nn)] = round(((circ.A - len(owned_n)) + pairs * (nn - 1) / nn + lk_cols) * circ.n * 32 / 1e9, 2)
        except Exception as e:
            projected["error"] = repr(e)

    # ---- rooflines of the proof's kernel classes, from this rank's events of the timed region
    n = circ.n
    ntt_ms = prof.get("ntt_pass", (0.0, 0))[0] + prof.get("ntt_last", (0.0, 0))[0]
    ntt_bytes = prof_bytes.get("ntt_pass", 0) + prof_bytes.get("ntt_last", 0)
    transforms = ntt_bytes / (64.0 * n) if ntt_bytes else 0
    traffic_ntt, tsrc_ntt = committed_traffic("ntt_bytes_per_transform") if circ.k == 20 else (None, None)
    roof_ntt = None
    if transforms:
        roof_ntt = hbm_roof(f"k_ntt_pass + k_ntt_last (one size-2^{circ.k} transform: lagrange_to_coeff / coset forms)", 64.0 * n, ntt_ms / transforms,
                            f"dominant kernel class of the proof by device time; algorithmic bytes = 64 B x 2^{circ.k} per transform (read once, write once; SURVEY 8d); `avg_launch_ms` is per TRANSFORM "
                            "(both launches; the columns of a launch share it).  VALU-issue bound: k/2 x 2^k Montgomery products per transform; `alu.frac_own_routine` here is the IN-PROOF fraction of the "
                            "product peak (transforms share the device with the commitments running on the other stream) -- the same kernels alone reach the fraction in `msm_ntt.rooflines[1]`",
                            products=n * circ.k / 2.0, launches=prof.get("ntt_pass", (0, 0))[1] + prof.get("ntt_last", (0, 0))[1])
        roof_ntt["transforms_per_proof"] = round(transforms / args.steps, 1)
        roof_ntt["device_ms_per_proof"] = round(ntt_ms / args.steps, 2)
        roof_ntt["traffic"] = traffic_ntt
        roof_ntt["traffic_source"] = f"profiles/{tsrc_ntt}" if traffic_ntt else None
        if world > 1:
            roof_ntt["rank"] = 0
    bk = prof.get("msm_buckets", (0.0, 0))
    traffic_msm, tsrc_msm = committed_traffic("msm_buckets_bytes_per_launch")
    roof_msm = hbm_roof("k_msm_buckets (merged-window launches of the proof: dense and mixed columns)", 96.0 * n, bk[0] / bk[1] if bk[1] else 0,
                        f"algorithmic bytes = 96 B (32 B scalar + 64 B affine base) x 2^{circ.k} per commitment (SURVEY 8d)", launches=bk[1])
    if roof_msm:
        roof_msm["device_ms_per_proof"] = round(bk[0] / args.steps, 2)
        roof_msm["traffic_dense_column"] = traffic_msm if circ.k == 20 else None
    q = prof.get("quotient_coset", (0.0, 0))
    roof_q = None
    qb = prof_bytes.get("quotient_coset", 0)
    if q[1]:
        roof_q = {"kernel": "k_quotient_eval (degree-class launches)", "bound": "hbm", "achieved": round(qb / (q[0] * 1e-3) / 1e9, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                  "frac": round(qb / (q[0] * 1e-3) / 1e9 / HBM_PEAK_GBS, 4), "device_ms_per_proof": round(q[0] / args.steps, 2), "launches_timed": q[1],
                  "avg_launch_ms": round(q[0] / q[1], 4), "algorithmic_bytes_per_launch": int(qb / q[1]),
                  "algorithmic_bytes_per_proof": int(qb / args.steps), "traffic": None,
                  "note": "`achieved` counts ALGORITHMIC bytes: 32 B x rows x (distinct (column, rotation) operands + parked intermediates + 1 result) per launch, as the library books them -- "
                          "every operand once.  `executed` counts what the interpreter actually loads: every memory operand of every instruction (a cell read by twenty constraints is loaded "
                          "twenty times, hundreds of instructions apart), and the field products it performs.  Since the second half of round 6 the large class programs run in slices that share "
                          "their rows' operands through the caches: `traffic` (counters, per launch) is a quarter of the executed loads"}
        ops = class_program_operands(circ) if world == 1 else None
        if ops:
            ex_bytes = sum((1 << e_) * (c_["reads"] + c_["parks"] + 1) * 32 * n for e_, c_ in enumerate(ops) if c_["used"])
            ex_prod = sum((1 << e_) * c_["products"] * n for e_, c_ in enumerate(ops) if c_["used"])
            roof_q["executed"] = {"operand_bytes_per_proof": int(ex_bytes), "achieved_gb_s": round(ex_bytes / (q[0] / args.steps * 1e-3) / 1e9, 1),
                                  "frac_of_hbm_peak": round(ex_bytes / (q[0] / args.steps * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
                                  "products_per_proof": int(ex_prod), "g_products_per_s": round(ex_prod / (q[0] / args.steps * 1e-3) / 1e9, 1),
                                  "frac_of_product_peak": round(ex_prod / (q[0] / args.steps * 1e-3) / 1e9 / MULPEAK_G, 3)}
            roof_q["alu"] = {"unit": "G Montgomery products/s", "achieved": roof_q["executed"]["g_products_per_s"], "peak_own_routine": MULPEAK_G,
                             "frac_own_routine": roof_q["executed"]["frac_of_product_peak"]}
        tq, tsrc_q = committed_traffic("quotient_bytes_per_launch") if circ.k == 20 and shape == "evm" else (None, None)
        roof_q["traffic"] = tq
        roof_q["traffic_source"] = f"profiles/{tsrc_q}" if tq else None
    alg = proof_algorithmic_bytes(circ)
    alg_total = sum(alg.values())
    # the same sum with the two stages the degree classes shrink replaced by what this implementation executes: the transforms the
    # library launched (64 B x n each: one per committed column, one per (column, coset) a class reads) and the bytes its class
    # programs stream -- halo2's algorithm books every column on all 2^(extended_k - k) cosets
    executed = dict(alg)
    k_l2c, k_cos, k_q = (next(k_ for k_ in alg if k_.startswith(p_)) for p_ in ("lagrange_to_coeff", "coset transforms", "quotient evaluation"))
    if transforms and world == 1:
        executed[k_l2c], executed[k_cos] = 0, int(64 * n * transforms / args.steps)
        executed[k_q] = int(qb / args.steps)
    executed_total = sum(executed.values()) if transforms and world == 1 else None
    proof_traffic, tsrc_proof = committed_traffic("proof_traffic_bytes") if circ.k == 20 and world == 1 else (None, None)
    out = {
        **head,
        # the dominant kernel class of THIS proof by device time: the evaluator on the EVM-style shape, the NTT passes on the plain one
        "roofline": max((r for r in (roof_ntt, roof_q) if r), key=lambda r: r.get("device_ms_per_proof", 0), default=None),
        "rooflines": [r for r in (roof_ntt, roof_msm, roof_q) if r],
        "proof_roofline": {"algorithmic_bytes": int(alg_total), "achieved": round(alg_total / per_proof / 1e9, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                           "frac": round(alg_total / per_proof / 1e9 / HBM_PEAK_GBS, 4), "by_stage_bytes": {k_: int(v) for k_, v in alg.items()},
                           "executed_algorithmic_bytes": executed_total,
                           "executed_frac": round(executed_total / per_proof / 1e9 / HBM_PEAK_GBS, 4) if executed_total else None,
                           "traffic": proof_traffic, "traffic_source": f"profiles/{tsrc_proof}" if proof_traffic else None,
                           "note": "`algorithmic_bytes` = sum over the stages of one create_proof of SURVEY 8d's algorithmic bytes as HALO2'S algorithm incurs them (every committed column "
                                   "transformed to all 2^(extended_k - k) cosets, every operand once per stage) / wall-clock / 8 TB/s: a work-equivalent throughput, NOT bytes this "
                                   "implementation moves -- its degree classes transform a column to 2 / 4 / 8 cosets only; `executed_algorithmic_bytes` counts the transforms and class "
                                   "programs actually launched; `traffic` = what the PMC counters saw per proof (FETCH_SIZE raw, x 2 as the guide corrects 64-byte requests, WRITE_SIZE)"},
        "extra": {"proof_bytes": len(state["proof"]), "proof_sha256": __import__("hashlib").sha256(state["proof"]).hexdigest(), "verified_by_oracle": verified,
                  "create_proof_s_mean": round(per_proof, 4), "keygen_pk_s": round(t_keygen, 3),
                  "witness_upload_s_outside_timing": round(t_upload, 2), "host_circuit_build_s": round(t_build, 2),
                  "msm_count": circ.A + 2 * len(circ.lookups) + (len(circ.perm_cols) + circ.degree() - 3) // (circ.degree() - 2) + (circ.degree() - 1) + 2,
                  "kernel_class_device_ms_per_proof": {k_: round(v[0] / args.steps, 2) for k_, v in prof.items() if v[1]},
                  "pcie_inclusive": pcie, "structure_blind": blind, "degree_blind": degree_blind, "projected_rank_device_s": projected,
                  "shape": shape, "gate_polynomials": len(circ.gates), "gate_degrees": {str(d_): sum(1 for g_ in circ.gates if g_.degree() == d_) for d_ in sorted({g_.degree() for g_ in circ.gates})},
                  "lookup_tuple_widths": sorted({len(lk.table) for lk in circ.lookups}),
                  "evaluator": {"plan": plan, "class_launches_per_proof": round(q[1] / args.steps, 1), "device_ms_per_proof": round(q[0] / args.steps, 2),
                                "transforms_per_proof": round(transforms / args.steps, 1) if transforms else None,
                                "note": "plan = zk_pk_quotient_plan: per degree class the compiled program's instructions / field products per row / columns read / values parked / parking slots alive "
                                        "at once (csrc/class_compile.hpp); a class of index e runs on 2^e cosets"}},
    }
    teardown()
    return out


# ------------------------------------------------------------------------------------ BASELINE configs[1]: MSM 2^20 + NTT 2^20
def msm_ntt_section(args, torch):
    """Standalone BN254 G1 MSM 2^20 + Fr NTT 2^20 (BASELINE configs[1]): a batch of commitments (pipelined on the device) then the
    batch of transforms, over rotating sets of 32 + 32 distinct columns (2 GiB, eight times the Infinity Cache), inputs resident in HBM."""
    import numpy as np

    import zkevm_circuits_amd as z

    steps, warmup = 32, 16
    ctx = z.Context(0)
    srs = ctx.srs_setup_with_s(K, fr_mont(0xC0FFEE))

    def synth_column(seed: int) -> np.ndarray:
        rng = np.random.default_rng(seed)
        a = rng.integers(0, 1 << 63, size=(N, 4), dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=(N, 4), dtype=np.uint64)
        a[:, 3] &= np.uint64((1 << 60) - 1)
        return a
    first_column = synth_column(1000)
    d_cols = [ctx.to_device(first_column if i == 0 else synth_column(1000 + i)) for i in range(NCOL)]
    d_work = [ctx.to_device(synth_column(5000 + i)) for i in range(NCOL)]
    cursor = [0]

    def run_steps(count):
        done = 0
        while done < count:
            b = min(args.batch, count - done)
            ids = [(cursor[0] + j) % NCOL for j in range(b)]
            cursor[0] += b
            ctx.commit_batch(srs, [d_cols[i].ptr for i in ids], N, lagrange=True, narrow=[0] * b)
            ctx.ntt_batch([d_work[i] for i in ids], K, inverse=True)
            done += b
    run_steps(warmup)
    device_sync(ctx, torch)
    ctx.prof_reset()
    ctx.prof_enable(2)
    t0 = time.perf_counter()
    run_steps(steps)
    device_sync(ctx, torch)
    elapsed = time.perf_counter() - t0
    ctx.prof_enable(False)
    prof = {name: ctx.prof_get(name) for name in ctx.prof_names()}
    lone = []
    for i in range(6):
        t1 = time.perf_counter()
        ctx.commit(srs, d_cols[i % NCOL], N, lagrange=True)
        lone.append(time.perf_counter() - t1)
    plan = ctx.msm_plan(srs, N)
    bucket = prof.get("msm_buckets", (0.0, 0))
    bucket_ms = bucket[0] / bucket[1] if bucket[1] else 0
    ntt_ms = (prof.get("ntt_pass", (0, 0))[0] + prof.get("ntt_last", (0, 0))[0]) / steps
    traffic, tsrc = committed_traffic("msm_buckets_bytes_per_launch")
    roof = hbm_roof("k_msm_buckets", 96.0 * N, bucket_ms,
                    f"algorithmic bytes = 96 B x 2^20 (SURVEY 8d); integer-ALU bound: one mixed XYZZ addition ({MADS_PER_MIXED_ADD} multiply-adds) per (scalar, window), {plan['windows']} windows",
                    products=MADS_PER_MIXED_ADD / MADS_PER_PRODUCT * N * plan["windows"], launches=bucket[1])
    if roof:
        roof["traffic"] = traffic
        roof["traffic_source"] = f"profiles/{tsrc}" if traffic else None
    rec = {
        "workload": "BASELINE configs[1]: BN254 G1 MSM 2^20 + Fr NTT 2^20 per step, uniform scalars, batches of 32 columns",
        "msm_mscalar_per_s": round(N * steps / elapsed / 1e6, 2), "ms_per_step": round(elapsed / steps * 1e3, 4), "steps": steps, "warmup": warmup,
        "msm_lone_ms": round(sorted(lone)[len(lone) // 2] * 1e3, 4),
        "ntt_only_ms": round(ntt_ms, 4), "ntt_gfieldop_per_s": round(1.5 * N * K / (ntt_ms * 1e-3) / 1e9, 2) if ntt_ms else None,
        "msm_window_bits": plan.get("c"), "msm_windows": plan["windows"],
        "rooflines": [r for r in (roof, hbm_roof("k_ntt_pass + k_ntt_last (one 2^20 transform)", 64.0 * N, ntt_ms,
                                                 "algorithmic bytes = 64 B x 2^20; VALU-issue bound: 10.5 M Montgomery products per transform", products=N * K / 2.0)) if r],
    }
    if not args.no_cpu_baseline:
        rec["cpu_baseline"] = cpu_baseline_msm_ntt(srs, first_column)
    for b_ in d_cols + d_work:
        b_.free()
    srs.destroy()
    ctx.close()
    return rec


def cpu_baseline_msm_ntt(srs, column):
    """Oracle (C restatement of halo2's best_multiexp + best_fft, OpenMP) on the host cores: one 2^20 MSM + one 2^20 NTT."""
    from oracle import bn254, cref

    bases = srs.download_g_lagrange()
    threads = cref.num_threads()
    t0 = time.perf_counter()
    cref.best_multiexp(column, bases, threads)
    t1 = time.perf_counter()
    cref.best_fft(column, bn254.omega_for_k(K), K)
    t2 = time.perf_counter()
    return {"value": round(N / (t2 - t0) / 1e6, 4), "unit": "Mscalar/s", "cores": threads, "kind": "port",
            "sample": f"one MSM 2^20 ({t1 - t0:.2f} s) + one NTT 2^20 ({t2 - t1:.2f} s), C oracle (halo2 best_multiexp / best_fft restated), OpenMP {threads} threads"}


# ------------------------------------------------------------------------------------ other shapes: one prover process each
OTHER_SHAPE = "plain" if HEADLINE_SHAPE == "evm" else "evm"
PROOF_SHAPES = (f"supercircuit_shape_k20_{OTHER_SHAPE}", "keccak_shape_k18", "bundle_shape_k21", "supercircuit_shape_k20_dense", "supercircuit_shape_k20_small", "evm_shape_k14_mock")
MOCK_SHAPES = {"evm_shape_k14_mock": ("build_large", (14, 53)),                           # BASELINE configs[0] stand-in: k = 14, 159 advice columns
               "supercircuit_shape_k20_mock": ("build_shape", SC_SHAPE)}                   # only with ZK_BENCH_PROOFS=supercircuit_shape_k20_mock


def proof_section(timeout=600):
    """The other shapes and witness distributions, each in a prover process of its own (`bench.py --proof-worker <shape>`: the
    library and nothing else -- no torch, as in a Rust / C prover), each proof checked by the oracle verifier."""
    out = {}
    only = os.environ.get("ZK_BENCH_PROOFS", "")          # measurement knob: comma-separated subset of the shapes
    for name in PROOF_SHAPES:
        if only and name not in only.split(","):
            continue
        try:
            res = subprocess.run([sys.executable, os.path.abspath(__file__), "--proof-worker", name], capture_output=True, text=True, timeout=timeout)
            lines = [ln for ln in res.stdout.splitlines() if ln.startswith("{")]
            if res.returncode != 0 or not lines:
                out[name] = {"error": f"worker exited with {res.returncode}: {res.stderr[-400:]}"}
            else:
                out[name] = json.loads(lines[-1])
            if os.environ.get("ZK_PROVER_TRACE"):
                sys.stderr.write(res.stderr)
        except Exception as e:           # the headline must survive a failure here
            out[name] = {"error": repr(e)}
    return out


def cpu_baseline_proof(k=18):
    """The proof-level CPU baseline, MEASURED (SURVEY 8d last row; the reference's `[Proof generation]` timer
    [REF circuit-benchmarks/src/super_circuit.rs:115-134] needs Rust): halo2's create_proof restated over arrays with the oracle's C
    primitives and OpenMP (oracle/cpu_prover.py: whole-extended-domain evaluate_h, as upstream's CPU prover), on the Keccak shape at
    k = 18 (BASELINE configs[2]) -- the SuperCircuit shape at k = 20 (1300 MSMs of 2^20) would take the host a quarter of an hour --
    beside the GPU session on the SAME circuit, witness, seed and vk.transcript_repr: the two proofs must be the same bytes.  Key
    generation and the SRS are outside both timings.  Runs in a process of its own (`--proof-worker keccak_shape_cpu_vs_gpu`)."""
    try:
        res = subprocess.run([sys.executable, os.path.abspath(__file__), "--proof-worker", f"keccak_shape_cpu_vs_gpu:{k}"], capture_output=True, text=True, timeout=900)
        lines = [ln for ln in res.stdout.splitlines() if ln.startswith("{")]
        if res.returncode != 0 or not lines:
            return {"error": f"worker exited with {res.returncode}: {res.stderr[-400:]}"}
        return json.loads(lines[-1])
    except Exception as e:
        return {"error": repr(e)}


def cpu_vs_gpu_worker(k=18):
    import numpy as np

    import bench_proof as bp
    import zkevm_circuits_amd as z
    from oracle import cpu_prover as cp, cref

    S = 0x5EC2E7
    ctx = z.Context(0)
    circ, blob, adv_m, inst_m, inst = bp.build_keccak_shape(ctx, k)
    npub = [int(np.flatnonzero(np.asarray(a).reshape(-1, 4).any(axis=1))[-1]) + 1 if np.asarray(a).any() else 0 for a in inst_m]
    inst_m = [np.ascontiguousarray(a[:m]) for a, m in zip(inst_m, npub)]
    srs = ctx.srs_setup_with_s(k, cref.fr_const(S))
    pk = ctx.pk_create(srs, blob)
    _, rep = pk.vk(circ.F + len(circ.perm_cols))
    repr_int = cref.from_mont(rep.reshape(1, 4))[0]
    adv_dev = [ctx.to_device(a) for a in adv_m]
    gpu_times, gpu_proof = [], b""
    for _ in range(4):
        t0 = time.perf_counter()
        sess = ctx.proof_session(pk, inst_m, bytes(16), instance_slices=True)
        sess.set_multiopen(1)
        sess.advice_phase_dev({i: c for i, c in enumerate(adv_dev)}, in_place=True)
        gpu_proof = sess.finish()
        gpu_times.append(time.perf_counter() - t0)
    for b_ in adv_dev:
        b_.free()
    pk.destroy()
    srs.destroy()
    ctx.close()
    circ_h, adv_h, inst_h = bp.build_keccak_shape(None, k)          # same seed: the same circuit and witness, host side only
    key = cp.keygen(circ_h)
    srs_h = cp.Srs(k, S)
    stages = {}
    t0 = time.perf_counter()
    cpu_proof = cp.create_proof(circ_h, srs_h, adv_h, inst_h, repr_int, bytes(16), "shplonk", timings=stages, key=key)
    cpu_s = time.perf_counter() - t0
    threads = cref.num_threads()
    return {"value": round(cpu_s, 3), "unit": "s", "cores": threads, "kind": "port",
            "sample": f"ONE full proof of the Keccak shape at k = {k} (BASELINE configs[2] stand-in: {circ.A} advice, {circ.F} fixed, {len(circ.perm_cols)} permutation columns, {len(circ.lookups)} lookups, "
                      f"degree {circ.degree()}, {circ.bf} blinding factors): halo2 create_proof restated over arrays (oracle/cpu_prover.py), C primitives, OpenMP {threads} threads; keygen and SRS "
                      "outside the timing; not the reference's Rust prover (no toolchain here), and not the headline circuit (1300 commitments of 2^20 would take the host a quarter of an hour)",
            "stages_s": {name: round(v, 3) for name, v in stages.items()},
            "gpu_same_sample_s": round(min(gpu_times), 4), "gpu_create_proof_s": [round(t, 4) for t in gpu_times],
            "speedup_vs_restated_cpu": round(cpu_s / min(gpu_times), 1), "same_proof_bytes": cpu_proof == gpu_proof, "proof_bytes": len(gpu_proof)}


def mock_worker(name):
    """BASELINE configs[0] (the reference's own CPU-runnable case): MockProver over the EVM sub-circuit at k = 14
    [REF circuit-benchmarks/src/evm_circuit.rs:44-60] -- here zk_mock_verify (dev::MockProver::verify_par restated for the
    device) over the same-size stand-in: the satisfied witness, then one cell changed (the path that lists failures)."""
    import numpy as np

    import bench_proof as bp
    import zkevm_circuits_amd as z
    from zkevm_circuits_amd import plonk

    ctx = z.Context(0)
    builder, args = MOCK_SHAPES[name]
    circ, blob, adv_m, inst_m, inst = getattr(bp, builder)(ctx, *args)
    srs = ctx.srs_setup_with_s(circ.k, np.frombuffer(plonk.fr_mont_bytes(0x5EC2E7), dtype=np.uint64).copy())
    pk = ctx.pk_create(srs, blob)
    times = []
    for _ in range(3):
        t0 = time.perf_counter()
        got, total = ctx.mock_verify(pk, adv_m, inst_m)
        times.append(time.perf_counter() - t0)
        assert total == 0, got[:4]
    bad = [np.array(c, copy=True) for c in adv_m]
    row = int(np.flatnonzero(np.asarray(bad[2]).any(axis=1))[0])            # a cell a gate reads: first non-zero cell of advice column 2
    bad[2][row, 0] ^= np.uint64(1)
    t0 = time.perf_counter()
    got, total = ctx.mock_verify(pk, bad, inst_m)
    t_bad = time.perf_counter() - t0
    assert total >= 1
    rec = {"metric": "MockProver-style witness check wall-clock (s), zk_mock_verify on 1 x MI355X, witness columns uploaded from host memory inside the timed call", "value": round(min(times), 4),
           "unit": "s", "higher_is_better": False, "k": circ.k, "advice_columns": circ.A, "gate_polynomials": len(circ.gates), "lookups": len(circ.lookups),
           "permutation_columns": len(circ.perm_cols), "runs_s": [round(t, 4) for t in times],
           "one_cell_changed": {"wall_s": round(t_bad, 4), "failures": total, "first": list(got[0]) if got else None},
           "data": "synthetic circuit of the configuration's size class (the EVM circuit itself needs the Rust exporter)"}
    pk.destroy()
    srs.destroy()
    ctx.close()
    return rec


def proof_worker(name):
    """One proof shape, measured in this (fresh) process; witness resident in HBM."""
    import bench_proof as bp
    import zkevm_circuits_amd as z

    if name.startswith("keccak_shape_cpu_vs_gpu"):
        return cpu_vs_gpu_worker(int(name.split(":")[1]) if ":" in name else 18)
    if name in MOCK_SHAPES:
        return mock_worker(name)
    if name in ("supercircuit_shape_k20_plain", "supercircuit_shape_k20_evm"):
        # the OTHER stand-in of the headline's outer shape, measured exactly as the headline is (three phases, witness resident and handed
        # over in place, W warm-up + K timed proofs, HIP events on the roofline kernels, degree_blind / structure_blind beside it)
        import argparse as _ap
        a = _ap.Namespace(steps=int(os.environ.get("ZK_BENCH_STEPS", "3")), warmup=1, no_verify=False)
        rec = headline(a, _NoTorch, shape=name.rsplit("_", 1)[1], side=False, project=True)       # the emulated rank of N = 2 / 4 / 8 for this shape too (the round-5 review's target was stated on it)
        keep = {k_: rec[k_] for k_ in ("metric", "value", "unit", "steps", "warmup", "higher_is_better", "data", "roofline")}
        keep["config"] = {k_: rec["config"][k_] for k_ in ("workload", "advice_queries", "fixed_queries", "witness_cell_distribution")}
        keep["extra"] = {k_: rec["extra"][k_] for k_ in ("proof_bytes", "verified_by_oracle", "keygen_pk_s", "kernel_class_device_ms_per_proof", "structure_blind", "degree_blind", "shape",
                                                         "gate_polynomials", "gate_degrees", "lookup_tuple_widths", "evaluator", "projected_rank_device_s")}
        keep["rooflines"] = rec["rooflines"]
        return keep

    ctx = z.Context(0)
    repeat_env = int(os.environ.get("ZK_BENCH_STEPS", "0"))
    # (builder, proofs per key, transcript).  bundle_shape_k21: the recursion / bundle layer (BASELINE configs[4] stand-in) -- halo2-base
    # layout sized by [REF aggregator/configs/bundle_circuit.config] (degree 21, 5 + 1 advice, 1 fixed), FOUR sequential warm proofs (after one that fills the key's caches) sharing
    # one proving key, Poseidon transcript as gen_snark_shplonk uses [REF prover/src/common/prover/recursion.rs:60-77]
    build, repeat, tkind = {"keccak_shape_k18": (lambda: bp.build_keccak_shape(ctx, 18), 3, None),
                            "bundle_shape_k21": (lambda: bp.build_halo2_base_shape(ctx, 21, 5, 1, 20), 5, 1),
                            "supercircuit_shape_k20": (lambda: bp.build_shape(ctx, *SC_SHAPE, dist="survey"), 3, None),
                            "supercircuit_shape_k20_dense": (lambda: bp.build_shape(ctx, *SC_SHAPE, dist="dense"), 3, None),
                            "supercircuit_shape_k20_small": (lambda: bp.build_shape(ctx, *SC_SHAPE, dist="small"), 3, None)}[name]
    if repeat_env:
        repeat = repeat_env
    t0 = time.perf_counter()
    circ, blob, adv_m, inst_m, inst = build()
    t_build = time.perf_counter() - t0
    rec = bp.proof_bench(ctx, circ.k, circ, blob, adv_m, inst_m, inst, shplonk=True, repeat=repeat, verify=True, resident=True, t_build=t_build, transcript_kind=tkind)
    if rec is not None and tkind == 1:
        rec["transcript"] = "poseidon"
        rec["chain_of_4_proofs_s"] = round(sum(rec["create_proof_s"][-4:]), 4)          # four WARM proofs sharing one key (the first proof of a key also fills its coset cache: left out)
    ctx.close()
    return rec


# ------------------------------------------------------------------------------------ N > 1: can this box hold it?
def sharded_preflight(torch, dist, rank, world, shared_gpu):
    """None when the sharded headline can run here, else the reason (the same on every rank)"""
    def host_bytes_free():
        free = None
        try:
            import psutil
            free = psutil.virtual_memory().available
        except Exception:
            pass
        try:
            lim = open("/sys/fs/cgroup/memory.max").read().strip()
            if lim != "max":
                cur = int(open("/sys/fs/cgroup/memory.current").read())
                free = min(free, int(lim) - cur) if free is not None else int(lim) - cur
        except Exception:
            pass
        return free

    need = (24 << 30) >> max(0, 2 * (20 - HEADLINE_K))             # host bytes per rank at k = 20 (blob + witness + builder temporaries)
    verdict = [None]
    if rank == 0:
        free = host_bytes_free()
        if shared_gpu and HEADLINE_K > 14:
            verdict[0] = (f"{world} ranks on {torch.cuda.device_count()} GPU(s): the sharded proof at k = {HEADLINE_K} needs one GPU per rank (RCCL ranks cannot share a device; "
                          "150 GB of session state each); ranks may share a device only under the test switch ZK_BENCH_K <= 14")
        elif free is not None and free < world * need:
            verdict[0] = f"host memory: {free >> 30} GiB free, {world} ranks x {need >> 30} GiB needed"
    dist.broadcast_object_list(verdict, src=0)
    return verdict[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=3, help="timed proofs")
    ap.add_argument("--warmup", type=int, default=1, help="untimed proofs in front of them")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None, help="write what the last timed proof returned to DIR/*.npy (float32)")
    ap.add_argument("--full", action="store_true", help="also verify the proof, time the kernel classes and run every side measurement (the --no-* flags thin it out)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-proof", action="store_true", help="skip the other shapes / distributions (N = 1 only)")
    ap.add_argument("--no-verify", action="store_true", help="skip the oracle verifier's check of the last timed proof")
    ap.add_argument("--no-msm-ntt", action="store_true", help="skip the BASELINE configs[1] section")
    ap.add_argument("--only-msm-ntt", action="store_true", help="run the BASELINE configs[1] section alone and print its record (profiling passes)")
    ap.add_argument("--proof-worker", default="", help=argparse.SUPPRESS)      # internal: run ONE proof shape in this process and print its record
    ap.add_argument("--batch", type=int, default=32, help="msm_ntt section: columns submitted per commit_batch call")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be at least 1 and --warmup at least 0")

    if args.proof_worker:
        print(json.dumps(proof_worker(args.proof_worker)), flush=True)
        return
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        raise SystemExit(relaunch_under_launcher(args))
    if max(args.gpus, 1) == 1 and os.environ.get("WORLD_SIZE", "1") == "1" and not (args.full or args.only_msm_ntt):
        # a plain single-GPU run: the headline alone, torch not loaded (the library's own sync is the fence, as in the proof workers)
        print(json.dumps(headline(args, _NoTorch, full=False)), flush=True)
        return

    import torch  # device plumbing + torch.distributed only

    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != max(args.gpus, 1):
        raise SystemExit(f"bench.py: --gpus {args.gpus} but the launcher started {world} ranks")
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X: the hot path has no CPU fallback")
    ndev = torch.cuda.device_count()
    shared_gpu = world > ndev           # fewer GPUs than ranks (single-GPU test box): ranks share devices, exchange over gloo
    local_rank %= max(ndev, 1)
    torch.cuda.set_device(local_rank)

    if world == 1 and args.only_msm_ntt:
        print(json.dumps(msm_ntt_section(args, torch)), flush=True)
        return
    if world == 1:
        out = headline(args, torch, full=args.full)
        if args.full:
            if not args.no_cpu_baseline:
                out["cpu_baseline"] = cpu_baseline_proof(18)
            else:
                out["cpu_baseline"] = None
            if not args.no_msm_ntt:
                try:
                    out["msm_ntt"] = msm_ntt_section(args, torch)
                except Exception as e:
                    out["msm_ntt"] = {"error": repr(e)}
            if not args.no_proof:
                out["proof"] = proof_section()
        print(json.dumps(out), flush=True)
        return

    import datetime

    import torch.distributed as dist

    # the launcher's process group carries the barriers, the library communicator's 128-byte id and the per-rank clocks; the proof's
    # data moves over the library's own RCCL communicator (gloo callbacks when the ranks share a GPU)
    dist.init_process_group("gloo", timeout=datetime.timedelta(minutes=20))
    why_not = sharded_preflight(torch, dist, rank, world, shared_gpu)
    if why_not:
        if rank == 0:
            print(json.dumps({"metric": METRIC, "value": None, "unit": "s", "n_gpus": world, "steps": 0, "warmup": 0, "ms_per_step": None, "higher_is_better": False, "scaling": "strong",
                              "vs_baseline": None, "dtype": DTYPE, "data": "synthetic-shape", "config": {"workload": WORKLOAD}, "roofline": None, "cpu_baseline": None, "error": why_not}), flush=True)
        dist.barrier()
        dist.destroy_process_group()
        return
    out = headline(args, torch, rank, world, dist, local_rank, shared_gpu, full=args.full)
    if rank == 0:
        if args.full:
            out["cpu_baseline"] = None      # timed on rank 0 at N = 1 only (the N = 1 line carries it)
        print(json.dumps(out), flush=True)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()

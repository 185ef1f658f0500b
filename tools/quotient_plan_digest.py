"""Digests of the quotient plans zk_host_quotient_plan makes (no GPU): for a fixed set of constraint systems and every setting of
the planner's knobs, SHA-256 of the full summary (room for 8 + 14 (E + 1) words) and of every degree class's program words.  Two
builds of the library plan alike exactly when their outputs are the same text; tests/golden/quotient_plans.json is one such
output and tests/test_quotient_plan_golden.py recomputes it.

    python tools/quotient_plan_digest.py                  # every knob setting in a process of its own, JSON on stdout
    python tools/quotient_plan_digest.py --dump DIR       # also writes every constraint-system blob to DIR/<circuit>.bin
                                                          # (the input of tools/quotient_plan_check.cpp)

Circuits: every builder of tests/plonk_fixtures.py, the EVM-style system of tests/test_quotient_compile.py (>= 5 000 constraints)
and the constraint system bench.py plans for (SuperCircuit shape with the EVM-style block).  The last one is built at k = 10 with
the device-side witness conversion stubbed out and its header word set to the bench's k = 20: the plan reads the shape only."""
import argparse
import ctypes
import hashlib
import json
import os
import struct
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

KNOBS = [("default", {})] + [(f"{name[3:]}={v}", {name: v}) for name, v in (
    ("ZK_QUOTIENT_SPLIT", "0"), ("ZK_QUOTIENT_ADDSPLIT", "0"), ("ZK_QUOTIENT_GROUP", "0"), ("ZK_QUOTIENT_DAG", "0"), ("ZK_QUOTIENT_COSTGATE", "0"),
    ("ZK_QUOTIENT_MAC", "0"), ("ZK_QUOTIENT_MAC", "1"), ("ZK_QUOTIENT_CHUNK", "0"), ("ZK_QUOTIENT_CHUNK", "1"), ("ZK_LOOKUP_PLAIN", "1"))] + [
    ("QUOTIENT_DAG=0,QUOTIENT_GROUP=0", {"ZK_QUOTIENT_DAG": "0", "ZK_QUOTIENT_GROUP": "0"})]
KNOB_NAMES = sorted({name for _, kv in KNOBS for name in kv})


def bench_constraint_system():
    """cs blob of bench.py's headline circuit (SC_SHAPE with the EVM-style block, three phases)"""
    import bench_proof as bp
    real = bp.to_mont_gpu, bp.assemble_blob
    bp.to_mont_gpu, bp.assemble_blob = (lambda ctx, canon: canon), (lambda *a: None)       # witness and key columns: not needed for the plan
    try:
        circ = bp.build_shape(None, 10, 1000, 150, 150, 100, 9, dist="survey", phases=True, evm=dict(bp.EVM_DEFAULT))[0]
    finally:
        bp.to_mont_gpu, bp.assemble_blob = real
    blob = bytearray(circ.cs_blob())
    struct.pack_into("<I", blob, 8, 20)          # header: magic, version, k
    return bytes(blob)


def circuits():
    """name -> constraint-system blob"""
    import bench_proof as bp
    import plonk_fixtures as fx
    from zkevm_circuits_amd import plonk
    out = {
        "fixture_k6": fx.build_circuit(6)[0],
        "fixture_wide_k6": fx.build_circuit(6, wide=True)[0],
        "rotation_k7": fx.build_rotation_circuit(7)[0],
        "multi_lookup_k6": fx.build_multi_lookup_circuit(6)[0],
        "multi_lookup_deg2_k6": fx.build_multi_lookup_circuit(6, n_inputs=4, input_degree=2, gate_degree=5)[0],
        "evm_k6": fx.build_evm_circuit(6, seed=2)[0],
        "evm_k8": fx.build_evm_circuit(8, seed=8, states=12, per_state=24)[0],
    }
    out = {name: c.cs_blob() for name, c in out.items()}
    p = dict(bp.EVM_DEFAULT)
    c = plonk.Circuit(10, num_fixed=1, num_advice=bp.evm_step_columns(p), num_instance=0, blinding_factors=5)
    bp.evm_block(c, 0, c.fixed_col(0), p)
    out["evm_style_5000"] = c.cs_blob()
    out["bench_headline"] = bench_constraint_system()
    return out


def plan_digest(blob: bytes) -> dict:
    """the plan of one constraint system under the knobs in force: {"summary": sha256, "classes": [sha256 per class]}"""
    from zkevm_circuits_amd import binding
    lib = binding.lib()
    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    d = struct.unpack_from("<I", blob, 16)[0]              # header: magic, version, k, blinding factors, degree
    E = (d - 2).bit_length()                               # the extended domain has 2^E cosets, 2^E >= d - 1
    summ = np.zeros(8 + 14 * (E + 1), dtype=np.uint32)
    words = np.zeros(3 << 20, dtype=np.uint32)
    classes = []
    for e in range(E + 1):
        summ[:] = 0
        cnt = ctypes.c_uint32()
        rc = lib.zk_host_quotient_plan(blob, ctypes.c_size_t(len(blob)), ptr(summ), ctypes.c_size_t(summ.size), ctypes.c_uint32(e), ptr(words), ctypes.c_size_t(words.size), ctypes.byref(cnt))
        assert rc == 0 and summ[0] == E, (rc, int(summ[0]), E)
        classes.append(hashlib.sha256(words[:3 * cnt.value].tobytes()).hexdigest())
    return {"summary": hashlib.sha256(summ.tobytes()).hexdigest(), "classes": classes}


def digests(blobs: dict, label: str) -> dict:
    return {f"{label}|{name}": plan_digest(blob) for name, blob in blobs.items()}


def render(entries: dict) -> str:
    """one line per (knob setting, circuit)"""
    return "{\n" + ",\n".join(f"{json.dumps(k)}: {json.dumps(v)}" for k, v in entries.items()) + "\n}\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dump", metavar="DIR", help="write the constraint-system blobs to DIR/<circuit>.bin")
    ap.add_argument("--child", nargs=2, metavar=("DIR", "LABEL"), help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:          # one knob setting (already in the environment) over the blobs the parent wrote
        src, label = args.child
        blobs = {f[:-4]: open(os.path.join(src, f), "rb").read() for f in json.load(open(os.path.join(src, "order.json")))}
        json.dump(digests(blobs, label), sys.stdout)
        return
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        dst = args.dump or tmp
        os.makedirs(dst, exist_ok=True)
        blobs = circuits()
        for name, blob in blobs.items():
            with open(os.path.join(dst, name + ".bin"), "wb") as f:
                f.write(blob)
        with open(os.path.join(dst, "order.json"), "w") as f:
            json.dump([name + ".bin" for name in blobs], f)
        entries = {}
        for label, kv in KNOBS:      # a process per setting: the result cannot depend on what an earlier setting left behind
            env = {k: v for k, v in os.environ.items() if k not in KNOB_NAMES}
            env.update(kv)
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", dst, label], env=env, check=True, stdout=subprocess.PIPE).stdout
            entries.update(json.loads(out))
    sys.stdout.write(render(entries))


if __name__ == "__main__":
    main()

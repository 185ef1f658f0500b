"""GPU: sums of two column products and stack products under one reduction (PUSH_COL32 / MAC2_COL / MAC_STK, csrc/quotient.hip).
ZK_QUOTIENT_MAC: 0 = no fused steps, 1 = K_MAC_COL alone, unset / 2 = everything.
  * the device's new in-place products (mul2add29_ub_ipb, mul3add29_ub_ipa) equal their C forms in every limb (zk_selftest_products bits 256 / 512);
  * zk_quotient_eval gives the same bytes under the three knob values on programs rich in the new shapes and on edge operands, in one piece and
    sliced, and those bytes are the big-int oracle's;
  * an EVM-style proof is byte-equal across the three knob values, equal to the oracle prover's and accepted by the oracle verifier (k = 8), and the
    benched configuration at k = 20 proves to the same bytes under the three."""
import ctypes
import os
import random
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import bn254 as b  # noqa: E402
from test_gpu_quotient_mac import env, oracle_rows  # noqa: E402

pytestmark = pytest.mark.gpu
R = b.R_MOD
KNOBS = ("0", "1", None)


@pytest.mark.parametrize("field", [0, 1])
def test_the_new_products_equal_their_c_forms(zk, ctx, field):
    out = (ctypes.c_uint32 * 3)()
    for seed in (11, 0x51ED2702):
        ctx._ck(zk.lib().zk_selftest_products(ctx.h, ctypes.c_int(field), ctypes.c_uint32(1 << 20), ctypes.c_uint32(seed), out))
        assert (out[0], out[1]) == (0, 0), f"{out[0]} lanes differ, routines mask {out[1]:#x}"
        assert out[2] == 1 << 20


def pair_program(zk, rng, ncols, nconsts, terms):
    """a top-level sum of Horner sums whose terms are sums of two column products (bare, under sums, over computed factors), products of two
    computed values, and the shapes of test_gpu_quotient_mac; every other statement sits under a factor (one stack entry deeper)"""
    M32 = 1 << 32
    col = lambda: (zk.Q_PUSH_COL, rng.randrange(ncols), rng.choice([0, 0, 1, (-1) % M32]))
    mul, add, sub = (zk.Q_MUL, 0, 0), (zk.Q_ADD, 0, 0), (zk.Q_SUB, 0, 0)
    prog = []
    for t in range(terms):
        under_factor = t % 2 == 1
        if under_factor:
            prog += [col(), col(), sub]
        prog += [col(), col(), mul]
        for _ in range(rng.randrange(2, 9)):
            prog += [(zk.Q_MUL_CONST, rng.randrange(nconsts), 0)]
            shape = rng.randrange(7)
            if shape == 0:      # a * m1 + (k - n) * m2 - z
                prog += [col(), col(), mul, (zk.Q_PUSH_CONST, rng.randrange(nconsts), 0), col(), sub, col(), mul, add, col(), sub]
            elif shape == 1:    # k * m1 + (k * m2 + c)
                prog += [(zk.Q_PUSH_CONST, rng.randrange(nconsts), 0), col(), mul, (zk.Q_PUSH_CONST, rng.randrange(nconsts), 0), col(), mul, col(), add, add]
            elif shape == 2:    # (a - b - c) * m1 + (d + e + f) * m2: wide first factors
                prog += [col(), col(), sub, col(), sub, col(), mul, col(), col(), add, col(), add, col(), mul, add]
            elif shape == 3:    # (a + b) * (c - d): a stack product
                prog += [col(), col(), add, col(), col(), sub, mul, col(), sub]
            elif shape == 4:    # (a - b - c) * (d * e): a stack product with an unsettled first factor
                prog += [col(), col(), sub, col(), sub, col(), col(), mul, mul]
            elif shape == 5:    # a * m + (b - c): one product and a sum
                prog += [col(), col(), mul, col(), col(), sub, add]
            else:
                prog += [col(), col(), mul, col(), sub]
            prog += [add]
        if under_factor:
            prog += [mul]
        prog += [(zk.Q_FOLD, rng.randrange(nconsts), 0)]
    return prog


def lowered_ops(zk, prog, ncols, fuse):
    words = np.array(prog, dtype=np.uint32).reshape(-1)
    n_out, depth = ctypes.c_uint32(), ctypes.c_int()
    out = np.zeros(3 * (2 * len(prog) + 8), dtype=np.uint32)
    assert zk.lib().zk_host_quotient_lower(words.ctypes.data_as(ctypes.c_void_p), ctypes.c_uint32(len(prog)), ctypes.c_uint32(ncols), ctypes.c_int(fuse),
                                           out.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(out.size), ctypes.byref(n_out), ctypes.byref(depth)) == 0
    return [int(w) & 0xff for w in out[:3 * n_out.value:3]]


@pytest.mark.parametrize("k,ext_k,divide,slices,kind", [(11, 11, False, 0, "random"), (11, 12, True, 0, "random"), (11, 12, True, 3, "random"), (12, 12, False, 5, "random"),
                                                        (11, 11, False, 0, "max"), (11, 12, True, 2, "zero"), (11, 11, False, 0, "one")])
def test_the_three_streams_are_byte_equal_and_the_oracles(zk, ctx, cref, k, ext_k, divide, slices, kind, monkeypatch):
    rng = random.Random(37 * k + ext_k + slices + len(kind))
    ne, ncols, nconsts = 1 << ext_k, 8, 5
    fill = {"max": R - 1, "zero": 0, "one": 1}.get(kind)
    cols = [[rng.randrange(R) if fill is None else fill for _ in range(ne)] for _ in range(ncols)]
    for c in cols[:2]:
        for i in range(0, ne, 7):
            c[i] = R - 1                                   # operands at the top of the range
    consts = [rng.randrange(R) for _ in range(nconsts - 1)] + [R - 1]
    prog = pair_program(zk, rng, ncols, nconsts, 24)
    ops = lowered_ops(zk, prog, ncols, 7)
    assert ops.count(24) >= 10 and ops.count(25) >= 10 and ops.count(23) == ops.count(24), "the program must exercise MAC2_COL and MAC_STK"
    monkeypatch.setenv("ZK_QUOTIENT_SLICES", str(slices))
    dcols = [ctx.to_device(cref.to_mont(c)) for c in cols]
    outs = []
    for mac in KNOBS:
        if mac is None:
            monkeypatch.delenv("ZK_QUOTIENT_MAC", raising=False)
        else:
            monkeypatch.setenv("ZK_QUOTIENT_MAC", mac)
        out = ctx.alloc(ne * 32)
        ctx.quotient_eval(np.array(prog, dtype=np.uint32), [d.ptr for d in dcols], cref.to_mont(consts), k, ext_k, out, divide)
        outs.append(out.download((ne, 4)))
    assert np.array_equal(outs[0], outs[1]) and np.array_equal(outs[0], outs[2])
    sample = list(range(0, ne, max(1, ne // 32)))
    got = cref.from_mont(outs[2])
    assert [got[i] for i in sample] == oracle_rows_c(prog, cols, consts, k, ext_k, divide, sample)


def oracle_rows_c(prog, cols, consts, k, ext_k, divide, rows):
    """test_gpu_quotient_mac's big-int evaluation, PUSH_CONST added (rewritten as a column of that constant)"""
    ne = 1 << ext_k
    cols = list(cols)
    prog2 = []
    for op, a, bb in prog:
        if op == 2:
            cols.append([consts[a]] * ne)
            prog2.append((1, len(cols) - 1, 0))
        else:
            prog2.append((op, a, bb))
    return oracle_rows(prog2, cols, consts, k, ext_k, divide, rows)


def test_small_evm_shape_proof_is_the_same_under_the_three_knob_values(ctx, cref):
    from oracle import pairing as pr
    from oracle import plonk_prover as pp
    from oracle import plonk_verifier as pv
    from plonk_fixtures import build_evm_circuit
    from zkevm_circuits_amd import plonk
    k, S = 8, 0x5EC2E7
    circ, adv, inst = build_evm_circuit(k, seed=k, states=12, per_state=24)
    srs = ctx.srs_setup_with_s(k, cref.fr_const(S))
    pk = ctx.pk_create(srs, circ.blob())
    seed = bytes(range(3, 19))
    try:
        com, rep = pk.vk(circ.F + len(circ.perm_cols))
        vk_points, vk_repr = cref.affine_from_mont(com), cref.from_mont(rep.reshape(1, 4))[0]

        def prove():
            sess = ctx.proof_session(pk, [plonk.column_to_mont(c) for c in inst], seed)
            sess.set_multiopen(1)
            sess.advice_phase({i: plonk.column_to_mont(c) for i, c in enumerate(adv)})
            return sess.finish()
        proof = prove()
        assert proof == pp.create_proof(circ, pp.Srs(k, S), adv, inst, vk_repr, seed, "shplonk")
        assert pv.verify(circ, vk_points, vk_repr, inst, proof, pr.ec_mul(pr.G2_GEN, S), multiopen="shplonk")
        for mac in ("0", "1", "2"):
            with env({"ZK_QUOTIENT_MAC": mac}):
                assert prove() == proof, mac
    finally:
        pk.destroy()
        srs.destroy()


def test_the_benched_evm_configuration_at_k20_proves_the_same_bytes_under_the_three_knob_values(ctx, cref):
    from test_gpu_headline_config import require_host_memory
    require_host_memory(64)
    import bench_proof as bp
    shape = (20, 1000, 150, 150, 100, 9)
    circ, blob, adv_m, inst_m, inst, rlc = bp.build_shape(ctx, *shape, dist="survey", phases=True, evm=dict(bp.EVM_DEFAULT))
    npub = [int(np.flatnonzero(np.asarray(a).reshape(-1, 4).any(axis=1))[-1]) + 1 if np.asarray(a).any() else 0 for a in inst_m]
    inst_m = [np.ascontiguousarray(a[:m]) for a, m in zip(inst_m, npub)]
    srs = ctx.srs_setup_with_s(circ.k, cref.fr_const(0x5EC2E7))
    pk = ctx.pk_create(srs, blob)
    del blob
    adv_dev = [ctx.to_device(a) for a in adv_m]
    driver = bp.PhaseDriver(ctx, circ, adv_dev, rlc)
    try:
        def resident():
            sess = ctx.proof_session(pk, inst_m, bytes(16), instance_slices=True)
            sess.set_multiopen(1)
            driver.run(sess)
            return sess.finish()
        proof = resident()
        for mac in ("0", "1"):
            with env({"ZK_QUOTIENT_MAC": mac}):
                assert resident() == proof, mac
    finally:
        driver.free()
        for b_ in adv_dev:
            b_.free()
        pk.destroy()
        srs.destroy()

"""GPU: the evaluator's fused Horner steps (K_MAC_COL, csrc/quotient.hip; ZK_QUOTIENT_MAC=0 turns them off).
  * the device's in-place products (mul29_ipa / mul29_ipb / mul29_ub_ipa and the fused mul2add29_ub_ipa) equal the C forms in every limb;
  * zk_quotient_eval gives the same bytes with the fused stream and without it, on Horner-shaped programs in one piece and sliced;
  * the benched EVM-style configuration at k = 20 proves to the same bytes either way."""
import os
import random
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import bn254 as b  # noqa: E402

pytestmark = pytest.mark.gpu
R = b.R_MOD


class env:
    def __init__(self, kv): self.kv = kv
    def __enter__(self): os.environ.update(self.kv)
    def __exit__(self, *a):
        for k_ in self.kv:
            os.environ.pop(k_, None)


@pytest.mark.parametrize("field", [0, 1])
def test_in_place_and_fused_products_equal_the_c_forms(zk, ctx, field):
    """zk_selftest_products bits 16 / 32 / 64 / 128: the in-place forms the evaluator runs, at the lazy-reduction limb bounds, with a
    workgroup-uniform scalar factor for the _ub forms"""
    import ctypes
    out = (ctypes.c_uint32 * 3)()
    for seed in (7, 0x51ED2701):
        ctx._ck(zk.lib().zk_selftest_products(ctx.h, ctypes.c_int(field), ctypes.c_uint32(1 << 20), ctypes.c_uint32(seed), out))
        assert (out[0], out[1]) == (0, 0), f"{out[0]} lanes differ, routines mask {out[1]:#x}"
        assert out[2] == 1 << 20


def horner_program(zk, rng, ncols, nconsts, terms):
    """a top-level sum of Horner sums as the class compiler emits them: S y^g + sel * (a * b - c), S y^g + a * b + c, ..."""
    M32 = 1 << 32
    col = lambda: (zk.Q_PUSH_COL, rng.randrange(ncols), rng.choice([0, 0, 1, (-1) % M32]))
    prog = []
    for t in range(terms):
        prog += [col(), col(), (zk.Q_MUL, 0, 0)]
        for _ in range(rng.randrange(2, 9)):
            prog += [(zk.Q_MUL_CONST, rng.randrange(nconsts), 0)]
            shape = rng.randrange(4)
            if shape == 0:
                prog += [col(), col(), (zk.Q_MUL, 0, 0), col(), (zk.Q_SUB, 0, 0), col(), (zk.Q_MUL, 0, 0)]
            elif shape == 1:
                prog += [col(), col(), col(), (zk.Q_MUL, 0, 0), (zk.Q_MUL, 0, 0), col(), (zk.Q_SUB, 0, 0), col(), (zk.Q_ADD, 0, 0)]
            elif shape == 2:
                prog += [col(), col(), (zk.Q_MUL, 0, 0), (zk.Q_ADD_CONST, rng.randrange(nconsts), 0)]
            else:
                prog += [col(), col(), (zk.Q_SUB, 0, 0)]
            prog += [(zk.Q_ADD, 0, 0)]
        prog += [(zk.Q_FOLD, rng.randrange(nconsts), 0)]
    return prog


@pytest.mark.parametrize("k,ext_k,divide,slices", [(11, 11, False, 0), (11, 12, True, 0), (11, 12, True, 3), (12, 12, False, 5)])
def test_fused_stream_is_byte_equal_to_the_plain_one(zk, ctx, cref, k, ext_k, divide, slices, monkeypatch):
    rng = random.Random(31 * k + ext_k + slices)
    ne, ncols, nconsts = 1 << ext_k, 8, 5
    cols = [[rng.randrange(R) for _ in range(ne)] for _ in range(ncols)]
    for c in cols[:2]:
        for i in range(0, ne, 7):
            c[i] = R - 1                                   # operands at the top of the range
    consts = [rng.randrange(R) for _ in range(nconsts - 1)] + [R - 1]
    prog = horner_program(zk, rng, ncols, nconsts, 24)
    monkeypatch.setenv("ZK_QUOTIENT_SLICES", str(slices))
    dcols = [ctx.to_device(cref.to_mont(c)) for c in cols]
    outs = []
    for mac in ("1", "0"):
        monkeypatch.setenv("ZK_QUOTIENT_MAC", mac)
        out = ctx.alloc(ne * 32)
        ctx.quotient_eval(np.array(prog, dtype=np.uint32), [d.ptr for d in dcols], cref.to_mont(consts), k, ext_k, out, divide)
        outs.append(out.download((ne, 4)))
    assert np.array_equal(outs[0], outs[1])
    sample = list(range(0, ne, max(1, ne // 32)))
    got = cref.from_mont(outs[0])
    assert [got[i] for i in sample] == oracle_rows(prog, cols, consts, k, ext_k, divide, sample)


def oracle_rows(prog, cols, consts, k, ext_k, divide, rows):
    """big-int evaluation of the program on some rows (the ops these programs use)"""
    ne, scale = 1 << ext_k, 1 << (ext_k - k)
    tev = None
    if divide:
        zn, step = pow(b.FR_ZETA, 1 << k, R), pow(b.omega_for_k(ext_k), 1 << k, R)
        tev = [b.fr_inv((zn * pow(step, j, R) - 1) % R) for j in range(scale)]
    out = []
    for i in rows:
        st, acc = [], 0
        for op, a, bb in prog:
            if op == 1:
                rot = bb if bb < (1 << 31) else bb - (1 << 32)
                st.append(cols[a][(i + rot * scale) % ne])
            elif op == 3: y = st.pop(); st[-1] = (st[-1] + y) % R
            elif op == 4: y = st.pop(); st[-1] = (st[-1] - y) % R
            elif op == 5: y = st.pop(); st[-1] = st[-1] * y % R
            elif op == 9: acc = (acc * consts[a] + st.pop()) % R
            elif op == 10: st[-1] = st[-1] * consts[a] % R
            elif op == 11: st[-1] = (st[-1] + consts[a]) % R
            else: raise AssertionError(op)
        out.append(acc * tev[i % scale] % R if divide else acc)
    return out


def test_the_benched_evm_configuration_at_k20_proves_the_same_bytes_fused_or_not(ctx, cref):
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
        with env({"ZK_QUOTIENT_MAC": "0"}):
            assert resident() == proof
    finally:
        driver.free()
        for b_ in adv_dev:
            b_.free()
        pk.destroy()
        srs.destroy()

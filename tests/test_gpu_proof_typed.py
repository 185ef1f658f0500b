"""GPU: zk_proof_advice_phase_typed -- witness columns handed over as the integers they are (1, 2, 4, 8, 16 bytes per cell, or
Montgomery Fr) -- yields the challenges and the proof bytes of zk_proof_advice_phase on the same values, for both multi-open
schemes, on the EVM-style fixture (a lookup and a permutation over advice columns; one phase) and on the three-phase circuit of
test_gpu_proof; the caller's blinding rows are ignored; zk_proof_mock_verify sees ordinary columns; refused calls leave the
session usable."""
import os
import random
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from oracle import bn254 as b  # noqa: E402
from oracle import pairing as pr  # noqa: E402
from oracle import plonk_verifier as pv  # noqa: E402
from plonk_fixtures import build_evm_circuit  # noqa: E402
from test_gpu_proof import _three_phase_circuit  # noqa: E402
from zkevm_circuits_amd import plonk, sharding  # noqa: E402

pytestmark = pytest.mark.gpu
S_SECRET = 0x5EC2E7
R = b.R_MOD
SEED = bytes(range(5, 21))
SCHEMES = {"gwc": 0, "shplonk": 1}


def typed_column(values, u: int) -> np.ndarray:
    """the narrowest typed form of a column, judged by its usable rows (the others are the session's)"""
    vals = [v if i < u else 0 for i, v in enumerate(values)]
    top = max(vals)
    for bits, dt in ((8, np.uint8), (16, np.uint16), (32, np.uint32), (64, np.uint64)):
        if top < 1 << bits:
            return np.array(vals, dtype=dt)
    if top < 1 << 128:
        return np.array([[v & (2 ** 64 - 1), v >> 64] for v in vals], dtype=np.uint64)
    return plonk.column_to_mont(vals)


class Case:
    """a circuit, its key, and the witness of every phase as a function of the challenges squeezed so far"""

    def __init__(self, ctx, cref, circ, synth, inst):
        self.ctx, self.circ, self.synth, self.inst = ctx, circ, synth, inst
        self.srs = ctx.srs_setup_with_s(circ.k, cref.fr_const(S_SECRET))
        self.pk = ctx.pk_create(self.srs, circ.blob())
        com, rep = self.pk.vk(circ.F + len(circ.perm_cols))
        self.vk_points, self.vk_repr = cref.affine_from_mont(com), cref.from_mont(rep.reshape(1, 4))[0]
        self.cref = cref
        self.reference = {}

    def session(self, scheme="shplonk"):
        sess = self.ctx.proof_session(self.pk, [plonk.column_to_mont(c) for c in self.inst], SEED)
        sess.set_multiopen(SCHEMES[scheme])
        return sess

    def run(self, sess, form, widths_seen=None):
        """all phases of `sess`; form(column values) -> what is handed over (typed array, or None for the Montgomery call).
        Returns the challenges of every phase."""
        ch, per_phase = [], []
        for phase in range(self.circ.num_phases()):
            cols = self.synth(phase, ch)
            typed = {i: form(i, v) for i, v in cols.items()}
            if any(t is None for t in typed.values()):
                got = sess.advice_phase({i: plonk.column_to_mont(v) for i, v in cols.items()})
            else:
                if widths_seen is not None:
                    widths_seen.update(binding_width(t) for t in typed.values())
                got = sess.advice_phase_typed(typed)
            per_phase.append(got.copy())
            ch += self.cref.from_mont(got) if len(got) else []
        return per_phase

    def fr_proof(self, scheme):
        """the proof and the per-phase challenges of the Montgomery call: the reference of every comparison, made once"""
        if scheme not in self.reference:
            sess = self.session(scheme)
            ch = self.run(sess, lambda i, v: None)
            self.reference[scheme] = (sess.finish(), ch)
        return self.reference[scheme]

    def close(self):
        self.pk.destroy()
        self.srs.destroy()


def binding_width(a):
    from zkevm_circuits_amd import binding
    return binding.typed_cell_width(a)


@pytest.fixture(scope="module")
def evm_case(ctx, cref):
    """build_evm_circuit at its smallest size: step columns of bits, bytes and counters, products of bytes, field-sized a, b, c.
    The second triple (a', b', c'; no copy constraint touches it) is re-drawn on its product rows as 64-bit x 64-bit = 128-bit, so
    that every width occurs by construction."""
    circ, adv, inst = build_evm_circuit(6, seed=2)
    S = circ.A - 6
    rng = random.Random(9)
    for row in range(circ.u):
        if circ.fixed[1][row]:
            x, y = rng.randrange(1 << 63, 1 << 64), rng.randrange(1 << 63, 1 << 64)
            adv[S + 3][row], adv[S + 4][row], adv[S + 5][row] = x, y, x * y
    assert pv.check_witness(circ, adv, inst) is None
    case = Case(ctx, cref, circ, lambda phase, ch: dict(enumerate(adv)), inst)
    case.adv = adv
    yield case
    case.close()


@pytest.fixture(scope="module")
def phase_case(ctx, cref):
    """three phases, two rounds of challenges: a holds bytes and b 16-bit values; what depends on a challenge is field-sized"""
    circ, picks = _three_phase_circuit(6)
    n, u = circ.n, circ.u
    rng = random.Random(5)
    av = [rng.randrange(1, 256) if i < u - 1 else 0 for i in range(n)]
    bv = [rng.randrange(1, 1 << 16) if i < u - 1 else 0 for i in range(n)]

    def synth(phase, ch):
        if phase == 0:
            return {0: av, 1: bv}
        wv = [(av[i] + ch[0] * bv[i]) % R if i < u else 0 for i in range(n)]
        kv = [(bv[i] + ch[1] * av[i]) % R if i < u else 0 for i in range(n)]
        if phase == 1:
            return {2: wv, 3: kv}
        tv = [(wv[i] + ch[2] * kv[i]) % R if i < u else 0 for i in range(n)]
        sv, lv = [0] * n, [0] * n
        for row in range(u):
            if circ.fixed[1][row]:
                sv[row + 1] = tv[row] * tv[row] % R * ch[2] % R * b.fr_inv(wv[row]) % R
        for row, src in picks:
            lv[row] = wv[src]
        return {4: tv, 5: sv, 6: lv}
    case = Case(ctx, cref, circ, synth, [[av[0]] + [0] * (n - 1)])
    yield case
    case.close()


@pytest.mark.parametrize("scheme", sorted(SCHEMES))
@pytest.mark.parametrize("which", ["evm", "three_phase"])
def test_typed_columns_give_the_bytes_of_the_montgomery_call(request, which, scheme):
    case = request.getfixturevalue("evm_case" if which == "evm" else "phase_case")
    u = case.circ.u
    want, want_ch = case.fr_proof(scheme)
    widths = set()
    sess = case.session(scheme)
    got_ch = case.run(sess, lambda i, v: typed_column(v, u), widths)
    proof = sess.finish()
    assert len(got_ch) == len(want_ch) and all(np.array_equal(x, y) for x, y in zip(got_ch, want_ch))
    assert proof == want
    assert pv.verify(case.circ, case.vk_points, case.vk_repr, case.inst, proof, pr.ec_mul(pr.G2_GEN, S_SECRET), multiopen=scheme)
    if which == "evm":
        assert widths == {1, 2, 4, 8, 16, 32}, widths
    else:
        assert {1, 2, 32} <= widths and sum(len(c) for c in want_ch) == 3


def test_callers_blinding_rows_are_ignored(evm_case):
    circ = evm_case.circ
    rng = np.random.default_rng(3)

    def form(i, v):
        t = typed_column(v, circ.u).copy()
        t[circ.u:] = rng.integers(1, 255, size=t[circ.u:].shape, dtype=np.uint64).astype(t.dtype)
        return t
    sess = evm_case.session()
    evm_case.run(sess, form)
    assert sess.finish() == evm_case.fr_proof("shplonk")[0]


def test_all_columns_of_width_32(evm_case):
    widths = set()
    sess = evm_case.session()
    evm_case.run(sess, lambda i, v: plonk.column_to_mont(v), widths)
    assert widths == {32} and sess.finish() == evm_case.fr_proof("shplonk")[0]


def test_mock_verify_sees_ordinary_columns(evm_case):
    circ, adv = evm_case.circ, evm_case.adv
    sess = evm_case.session()
    evm_case.run(sess, lambda i, v: typed_column(v, circ.u))
    assert sess.mock_verify() == ([], 0)
    sess.abort()
    byte_cols = [i for i in range(circ.A) if typed_column(adv[i], circ.u).dtype == np.uint8]
    for col, row in ((c_, r_) for c_ in reversed(byte_cols) for r_ in range(2, circ.u, 7)):      # the first wrong byte that a constraint notices
        bad = [list(c) for c in adv]
        bad[col][row] ^= 0x80                               # still a byte
        if pv.mock_failures(circ, bad, evm_case.inst):
            break
    else:
        pytest.fail("no byte cell of the fixture is constrained")
    reports = []
    for typed in (False, True):
        sess = evm_case.session()
        if typed:
            sess.advice_phase_typed({i: typed_column(c, circ.u) for i, c in enumerate(bad)})
        else:
            sess.advice_phase({i: plonk.column_to_mont(c) for i, c in enumerate(bad)})
        reports.append(sess.mock_verify())
        sess.abort()
    assert reports[1] == reports[0] and reports[0][1] > 0
    assert reports[0][0] == pv.mock_failures(circ, bad, evm_case.inst)


def test_a_bad_width_leaves_the_session_usable(zk, evm_case):
    import ctypes
    circ = evm_case.circ
    lib = zk.lib()
    cols = [typed_column(c, circ.u) for c in evm_case.adv]
    idx = (ctypes.c_uint32 * circ.A)(*range(circ.A))
    ptrs = (ctypes.c_void_p * circ.A)(*[c.ctypes.data for c in cols])
    good = [binding_width(c) for c in cols]
    sess = evm_case.session()
    for wrong in (0, 3, 5, 24, 64):
        widths = (ctypes.c_uint8 * circ.A)(*(good[:2] + [wrong] + good[3:]))
        assert lib.zk_proof_advice_phase_typed(evm_case.ctx.h, sess.h, idx, ptrs, widths, ctypes.c_uint32(circ.A), None, None) == -1      # ZK_ERR_INVALID_ARG
    assert lib.zk_proof_advice_phase_typed(evm_case.ctx.h, sess.h, idx, ptrs, None, ctypes.c_uint32(circ.A), None, None) == -1             # null widths
    sess.advice_phase_typed(dict(enumerate(cols)))
    assert sess.finish() == evm_case.fr_proof("shplonk")[0]


def test_a_sharded_session_refuses_typed_columns(zk, evm_case):
    circ = evm_case.circ
    calls = []

    def gather(user, send, nbytes, recv):
        calls.append(nbytes)
        return 1
    cb = sharding.ALLGATHER_FN(gather)
    sess = evm_case.session()
    sess.set_sharding(0, 2, cb)
    try:
        with pytest.raises(zk.ZkError, match="status -5"):                  # ZK_ERR_UNSUPPORTED
            sess.advice_phase_typed({i: typed_column(c, circ.u) for i, c in enumerate(evm_case.adv)})
        assert calls == []
    finally:
        sess.abort()

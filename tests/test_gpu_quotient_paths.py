"""GPU: the quotient evaluator (csrc/quotient.hip) bit for bit against the big-int reference, on every device path.

The corpus of tests/quotient_programs.py -- nested folds, Horner sums (K_MAC_COL), parked values read right behind their TEE, a few
hundred parking slots, stacks 16 deep, rotations far outside the domain -- at ext_k 0, 1, 3, 7, 8, 10, 11, 12 with ext_k - k = 0 .. 3,
dividing by the vanishing polynomial and not, columns of stored words in segments of p - 1, 0, R, p - 2 and random values.  It runs
under each knob the host reads per call: the default (k_quotient_eval2, fused Horner steps), ZK_QUOTIENT_MAC=0, ZK_QUOTIENT_FUSE=0 (the
caller's own instruction sequence), ZK_QUOTIENT_RELAXED=0 (round 5's settle rule) and ZK_QUOTIENT_KERNEL=1 (k_quotient_eval), and its
sliceable sums under ZK_QUOTIENT_SLICES = 0, 2, 3, 64.  Which of the eight <FULL, ACC_MEM> instantiations of the two kernels and the
sliced launch each run takes is computed with the host's own predicate (quotient_programs.variant); every one is reached several
times, and every lowered opcode and settle flag occurs (test_the_corpus_reaches_every_path)."""
import numpy as np
import pytest

import quotient_programs as qp

pytestmark = pytest.mark.gpu


def _set(monkeypatch, env):
    for k in qp.KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


class _Data:
    """columns (device), constants and reference values of the corpus, made once"""
    def __init__(self, ctx):
        self.ctx = ctx
        self.cases = {}

    def get(self, case):
        key = id(case)           # the entry keeps the case alive: its id is not reused
        if key not in self.cases:
            import random
            rng = random.Random(len(case.prog) * 131 + case.ext_k * 7 + case.k)
            ne = 1 << case.ext_k
            cols = [qp.column(rng, ne) for _ in range(case.ncols)]
            consts = qp.constants(rng, case.nconsts)
            rows = qp.sample_rows(case.ext_k)
            want = qp.reference(case.prog, cols, consts, case.k, case.ext_k, case.divide, rows)
            bufs = [self.ctx.to_device(qp.to_words(c)) for c in cols]
            self.cases[key] = (case, bufs, qp.to_words(consts), rows, want)
        return self.cases[key][1:]

    def run(self, case):
        bufs, consts, rows, want = self.get(case)
        ne = 1 << case.ext_k
        out = self.ctx.alloc(ne * 32)
        try:
            self.ctx.quotient_eval(np.array(case.prog, dtype=np.uint32), [b.ptr for b in bufs], consts, case.k, case.ext_k, out, case.divide)
            got = qp.from_words(out.download((ne, 4)))
        finally:
            out.free()
        return got, rows, want


_CORPUS = qp.corpus()
_SLICEABLE = qp.sliceable_corpus()


@pytest.fixture(scope="module")
def data(ctx):
    d = _Data(ctx)
    yield d
    for _, bufs, _, _, _ in d.cases.values():
        for b in bufs:
            b.free()


@pytest.mark.parametrize("setting", list(qp.SETTINGS))
def test_corpus_matches_the_reference(data, setting, monkeypatch):
    env = qp.SETTINGS[setting]
    _set(monkeypatch, env)
    for case in _CORPUS:
        got, rows, want = data.run(case)
        if rows is not None:
            got = [got[i] for i in rows]
        bad = next((j for j, (x, y) in enumerate(zip(got, want)) if x != y), None)
        assert bad is None, f"{case} under {setting} ({qp.variant(case.prog, case.ncols, case.ext_k, env)}): row {bad if rows is None else rows[bad]} differs"


@pytest.mark.parametrize("slices", qp.SLICE_SETTINGS)
def test_sliced_sums_match_the_reference_and_the_unsliced_run(data, slices, monkeypatch):
    nested_after_the_first = 0          # slice 0 starts from acc = 0: its constant multiplies nothing
    for case in _SLICEABLE:
        _set(monkeypatch, {"ZK_QUOTIENT_SLICES": "0"})
        whole, rows, want = data.run(case)
        _set(monkeypatch, {"ZK_QUOTIENT_SLICES": slices})
        cuts = qp.slice_cuts(case.prog, case.ext_k)
        assert (len(cuts) > 2) == (slices != "0"), (case, cuts)
        nested_after_the_first += sum(qp.nested_folds(case.prog[x:y]) for x, y in zip(cuts[1:], cuts[2:]))
        got, _, _ = data.run(case)
        assert [got[i] for i in rows] == want, f"{case}: sliced {len(cuts) - 1} ways"
        bad = next((i for i, (x, y) in enumerate(zip(got, whole)) if x != y), None)
        assert bad is None, f"{case}: sliced {len(cuts) - 1} ways, row {bad} differs from the unsliced run"
    assert slices == "0" or nested_after_the_first > 0, "no slice but the first holds a nested fold"


@pytest.mark.parametrize("ext_k", [8, 3])
def test_stack_depth_limit(zk, data, ext_k, monkeypatch):
    """caller depth 16 (LDS for 15 entries of nine limbs x 256 lanes: 138 KiB per workgroup) runs under every setting; 17 is refused"""
    case = qp.deep_case(16, ext_k, ext_k)
    assert qp.stack_depth(case.prog) == qp.MAX_STACK
    for setting, env in qp.SETTINGS.items():
        _set(monkeypatch, env)
        got, rows, want = data.run(case)
        assert got == want, setting
    _set(monkeypatch, {})
    deeper = qp.deep_case(17, ext_k, ext_k)
    with pytest.raises(zk.ZkError, match="status -5"):
        data.run(deeper)


def test_the_corpus_reaches_every_path():
    """every kernel instantiation and the sliced launch (with its combine pass) several times, every lowered opcode, both settle widths and the
    carry propagation -- a generator change must not silently stop testing one of them"""
    hits, ops, flags = qp.coverage()
    assert all(hits[v] >= 3 for v in qp.VARIANTS), hits
    assert set(qp.K_OPS) <= set(ops), ops
    assert all(flags[f] > 0 for f in ("settle", "settle8", "norm")), flags

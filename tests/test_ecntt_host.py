"""CPU: the butterfly of the group FFT behind g_to_lagrange (csrc/ec29.hip.hpp: ecntt_butterfly29, mul_scalar29, neg29pt over
add29pt / dbl29pt) compiled for the host as a stand-alone program (tests/host_ecntt_harness.hip) and run on the cases of
tests/ecntt_cases.py, where butterflies meet identities, the same point twice and opposite points in different lazily reduced
representations -- the branches of add29pt that no generic SRS reaches.  Mode `fft` runs the kernels' schedule and must give the
model's basis and the model's per-stage counts of doublings, cancellations and identity operands, with the stored invariant
kept after every butterfly; mode `add` gives add29pt two lazily reduced operands (independent z, y also as the neg29pt image
8p - y) in every pair shape and inside chains.  The program is built twice, plain and with the address and undefined-behaviour
sanitizers, and run directly; nothing here is loaded into Python.  The affine conversion of the outputs is done here in big
integers (inv29 is device code); k_ecntt_finish's own conversion is checked by tests/test_gpu_g_to_lagrange.py."""
import os
import random
import shutil
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import ecntt_cases as ec  # noqa: E402
from oracle import bn254 as o  # noqa: E402
from oracle import cref  # noqa: E402
from test_host_arith import P, check_stored_invariant, from_xyzz, limbs, points, same, val, xyzz_limbs  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = o.R_MOD


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def exe(request, tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    d = tmp_path_factory.mktemp("ecntt_" + request.param)
    path = str(d / "host_ecntt")
    flags = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all", "-g"] if request.param == "sanitized" else []
    subprocess.run([hipcc, "--cuda-host-only", "-O2", "-std=c++17", *flags, os.path.join(ROOT, "tests", "host_ecntt_harness.hip"), "-o", path], check=True, timeout=600)
    return path, str(d)


def run(exe, mode, text, tag="in"):
    path, d = exe
    name = os.path.join(d, f"{mode}_{''.join(ch if ch.isalnum() else '_' for ch in tag)}.txt")
    with open(name, "w") as f:
        f.write(text)
    r = subprocess.run([path, mode, name], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-600:], r.stderr[-2000:])
    assert r.stderr == "", r.stderr
    return r.stdout.splitlines()


def fft(exe, case):
    """-> (affine outputs as big-int points, per-stage counts)"""
    n = 1 << case.k
    mont = lambda v: int.from_bytes(o.mont_bytes(v, R), "little")
    rows = cref.limbs_to_ints(case.g.reshape(-1, 4))
    text = f"{case.k}\n{mont(ec.omega_inv(case.k)):x} {mont(o.fr_inv(n)):x}\n" + "".join(f"{rows[2 * i]:x} {rows[2 * i + 1]:x}\n" for i in range(n))
    lines = run(exe, "fft", text, f"{case.k}_{case.name}")
    assert len(lines) == case.k + n, lines[:case.k + 1]
    counts = []
    for s, ln in enumerate(lines[:case.k]):
        w = ln.split()
        assert w[0] == "stage" and int(w[1]) == s
        counts.append(tuple(int(v) for v in w[2:]))
    out = []
    for ln in lines[case.k:]:
        l = [int(v, 16) for v in ln.split()]
        assert len(l) == 36
        out.append(from_xyzz(l))
    return out, counts


def check(exe, case):
    out, counts = fft(exe, case)
    assert out == cref.affine_from_mont(case.expect), case.name
    if case.counts is not None:
        assert counts == case.counts, (case.name, counts)
    return counts


@pytest.mark.parametrize("k", ec.KS)
def test_every_family_matches_the_model(exe, k):
    """outputs bit for bit on the affine image, and the branch counts of every stage: the doubling and the cancellation are
    taken exactly where the model says two operands are equal or opposite"""
    cases = ec.families(k)
    assert [c.name for c in cases] == ec.case_ids(k)
    for case in cases:
        counts = check(exe, case)
        if case.name.startswith("root_of_unity") and k >= 2:
            assert all(c[0] > 0 and c[1] > 0 for c in counts[1:])
        if case.a is None:                                         # hash-to-curve points: nothing exceptional
            assert case.name == "unknown_dlog" and all(c == (0, 0, 0) for c in counts)


def test_random_at_k_8(exe):
    check(exe, ec.random_case(8, random.Random(0xECF8)))


def test_the_model_agrees_with_the_big_int_group_law():
    """the expected rows (C oracle: scalar multiplication, inverse FFT) against the pure-Python curve and a naive inverse DFT"""
    for case in ec.families(2):
        if case.a is None:
            continue
        n, wi, ninv = 4, ec.omega_inv(2), o.fr_inv(4)
        want = [sum(case.a[j] * pow(wi, i * j, R) for j in range(n)) * ninv % R for i in range(n)]
        assert cref.affine_from_mont(case.expect) == [o.g1_mul(o.G1_GEN, v) if v else None for v in want]
        assert cref.affine_from_mont(case.g) == [o.g1_mul(o.G1_GEN, v) if v else None for v in case.a]
    wide = ec.wide_families()
    assert [c.name for c in wide] == list(ec.WIDE_FAMILIES) and all(c.k == ec.K_WIDE for c in wide)


# ---- add29pt with two lazily reduced operands ------------------------------------------------------------------------

def lazy_operand(pt, rng):
    """a stored representation of pt: random z, x and y anywhere below 8p, zz and zzz below 2p; half of the time the image that
    neg29pt makes of a representation of -pt, y = 8p - y' (up to 8p - 1)"""
    if pt is None or rng.random() < 0.5:
        return xyzz_limbs(pt, rng, lazy=True)
    l = xyzz_limbs(o.g1_neg(pt), rng, lazy=True)
    y = 8 * P - val(l[9:18])
    assert 0 < y < 8 * P
    return l[:9] + limbs(y) + l[18:]


def add_lines(pairs):
    return "".join(" ".join(f"{v:x}" for v in a + b) + "\n" for a, b in pairs)


def test_add29pt_with_two_lazy_operands(exe):
    """every pair shape, 200 random representations each, against the oracle's group law"""
    rng = random.Random(0xADD29)
    pts = points(rng, 8)
    shapes = {"P+Q": lambda: (rng.choice(pts[:4]), rng.choice(pts[4:])), "P+P": lambda: (lambda p: (p, p))(rng.choice(pts)),
              "P-P": lambda: (lambda p: (p, o.g1_neg(p)))(rng.choice(pts)), "O+Q": lambda: (None, rng.choice(pts)),
              "P+O": lambda: (rng.choice(pts), None), "O+O": lambda: (None, None)}
    todo = []
    for name, make in shapes.items():
        for _ in range(200):
            a, b = make()
            todo.append((name, a, b, lazy_operand(a, rng), lazy_operand(b, rng)))
    lines = run(exe, "add", add_lines([(t[3], t[4]) for t in todo]), "shapes")
    assert len(lines) == len(todo) == 1200
    for (name, a, b, la, lb), ln in zip(todo, lines):
        got = [int(v, 16) for v in ln.split()]
        want = o.g1_add(a, b)
        assert same(from_xyzz(got), want), name
        assert (want is None) == (name in ("P-P", "O+O"))
        if a is not None and b is not None and want is not None:
            check_stored_invariant(got)
        elif want is not None:
            assert got == (lb if a is None else la)               # an identity operand hands the other one through as it is


def test_add29pt_exceptional_cases_inside_a_chain(exe):
    """the chain of test_host_arith.test_exceptional_cases_inside_a_chain through add29pt: 60 steps, the second operand the
    accumulated point (10 %), its inverse (10 %) or another point, always a fresh lazy representation; the accumulator goes on
    as add29pt left it or, half of the time, as a fresh lazy representation of the same point"""
    text, wants = "", []
    for seed in range(6):
        rng = random.Random(700 + seed)
        pts = points(rng, 4)
        acc, fresh = None, xyzz_limbs(None, rng)
        for i in range(60):
            r = rng.random()
            q = acc if (acc is not None and r < 0.1) else o.g1_neg(acc) if (acc is not None and r < 0.2) else pts[rng.randrange(len(pts))]
            lq = lazy_operand(q, rng)
            text += (" ".join(f"{v:x}" for v in fresh + lq) if fresh is not None else "acc " + " ".join(f"{v:x}" for v in lq)) + "\n"
            acc = o.g1_add(acc, q)
            wants.append((seed, i, acc))
            fresh = lazy_operand(acc, rng) if (acc is not None and rng.random() < 0.5) else None
    assert sum(1 for w in wants if w[2] is None) >= 6               # cancellations did happen
    lines = run(exe, "add", text, "chain")
    assert len(lines) == len(wants) == 360
    for (seed, i, want), ln in zip(wants, lines):
        got = [int(v, 16) for v in ln.split()]
        assert same(from_xyzz(got), want), (seed, i)
        if want is not None:
            check_stored_invariant(got)


def test_the_kernels_use_the_header_the_harness_compiles():
    csrc = os.path.join(ROOT, "zkevm-circuits_amd", "csrc")
    unit, header = open(os.path.join(csrc, "ecntt.hip")).read(), open(os.path.join(csrc, "ec29.hip.hpp")).read()
    assert '#include "ec29.hip.hpp"' in unit and "ecntt_butterfly29(u, v, w, j != 0, &lo, &hi);" in unit
    for name in ("mul_scalar29(const", "neg29pt(const", "add29pt(const"):
        assert name not in unit                                    # defined in the header only; the stage kernel holds no group law of its own
    assert "add29pt(" not in unit.split("k_ecntt_stage(")[1].split("k_ecntt_finish(")[0]
    for sig in ("__host__ __device__ inline G1Xyzz29 mul_scalar29(", "__host__ __device__ __forceinline__ G1Xyzz29 neg29pt(",
                "__host__ __device__ __forceinline__ void ecntt_butterfly29(", "__host__ __device__ __forceinline__ G1Xyzz29 add29pt("):
        assert sig in header
    assert "csrc/ec29.hip.hpp" in open(os.path.join(ROOT, "zkevm-circuits_amd", "Makefile")).read().split("HDR :=")[1]
    assert '#include "../zkevm-circuits_amd/csrc/ec29.hip.hpp"' in open(os.path.join(ROOT, "tests", "host_ecntt_harness.hip")).read()

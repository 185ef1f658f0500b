"""CPU: the lane-free code of ZK_OP_KEY_SORT and ZK_OP_KEY_ORDER (csrc/keyorder.hip.hpp) compiled for the host as a stand-alone
program (tests/host_key_order_harness.hip) and compared with the model of tests/key_order_cases.py: first differing limb and signed
difference for a difference in each of the 32 limbs (both signs, the limbs behind it different too) and for equal records; the
difference as a canonical Montgomery element for +-1, +-65535 and 0; the inverse entry; the gathers at every legal (offset, width);
and the sort's index arithmetic driven serially over whole small sorts -- n around one and several tiles, all records equal, 4
distinct records, masks -- where every scatter destination must be below n and the result the model's permutation.  The program is
built twice, plain and with the address and undefined-behaviour sanitizers, and run directly."""
import os
import shutil
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import key_order_cases as kc  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P, R256, TILE = kc.P, kc.R256, kc.TILE
DIFFS = [0, 1, -1, 65535, -65535, 2, -300, 256, -32768]


def make_pairs():
    """[(name, cur, prev)]"""
    rng = kc.rng(0x0DDE)
    pairs = []
    for j in range(32):
        for sign in (1, -1):
            prev = bytearray(rng.randbytes(64))
            cur = bytearray(prev)
            lo, hi = sorted(rng.sample(range(1 << 16), 2))
            a, b = (hi, lo) if sign > 0 else (lo, hi)
            cur[2 * j:2 * j + 2], prev[2 * j:2 * j + 2] = a.to_bytes(2, "big"), b.to_bytes(2, "big")
            cur[2 * j + 2:] = rng.randbytes(64 - 2 * j - 2)                # everything behind the limb differs too
            pairs.append((f"limb {j}, sign {sign}", bytes(cur), bytes(prev)))
        # only the low byte, only the high byte of the limb
        for byte in (0, 1):
            prev = bytearray(rng.randbytes(64))
            cur = bytearray(prev)
            cur[2 * j + byte] ^= 1 << rng.randrange(8)
            pairs.append((f"limb {j}, byte {byte}", bytes(cur), bytes(prev)))
    same = rng.randbytes(64)
    pairs += [("equal", same, same), ("zeros", bytes(64), bytes(64)), ("largest difference", b"\xff" * 64, bytes(64)), ("smallest difference", bytes(64), b"\xff" * 64)]
    return pairs


def make_sorts():
    """[(name, keys, mask)]"""
    rng = kc.rng(0x5027)
    four = kc.random_keys(rng, 4)
    sorts = []
    for n in (0, 1, 2, 63, 64, 65, 255, 256, 257, TILE - 1, TILE, TILE + 1, 3 * TILE + 5):
        sorts.append((f"random bytes 60..63, n = {n}", [bytes(60) + rng.randbytes(4) for _ in range(n)], kc.FULL_MASK))
    sorts.append(("random records, 700", kc.random_keys(rng, 700), kc.FULL_MASK))
    sorts.append(("all equal, two tiles and a bit", [four[0]] * (2 * TILE + 77), kc.FULL_MASK))
    sorts.append(("4 distinct records, 3 tiles + 5", [rng.choice(four) for _ in range(3 * TILE + 5)], kc.FULL_MASK))
    sorts.append(("4 distinct records, one byte kept", [rng.choice(four) for _ in range(TILE + 9)], bytes(17) + b"\x01" + bytes(46)))
    rows = kc.realistic_rows(rng, TILE + 300)
    sorts.append(("realistic rows, full mask", rows, kc.FULL_MASK))
    sorts.append(("realistic rows, no counter", rows, kc.NO_COUNTER_MASK))
    sorts.append(("mask of zeros", kc.random_keys(rng, 300), bytes(64)))
    sorts.append(("reversed", sorted(kc.random_keys(rng, 600), reverse=True), kc.FULL_MASK))
    return sorts


PAIRS, SORTS = make_pairs(), make_sorts()
GATHER = kc.rng(3).randbytes(64)
LEGAL = [(off, width) for off in range(64) for width in (1, 2, 4) if off + width <= 64]


def case_file(path):
    with open(path, "w") as f:
        for _, cur, prev in PAIRS:
            f.write(f"pair {cur.hex()} {prev.hex()}\n")
        for d in DIFFS:
            f.write(f"diff {d}\n")
        f.write(f"gather {GATHER.hex()}\ngather {(bytes(range(1, 65))).hex()}\n")
        for _, keys, mask in SORTS:
            f.write(f"sort {len(keys)} {bytes(mask).hex()}\n" + "".join(k.hex() + "\n" for k in keys))


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def outputs(request, tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    d = tmp_path_factory.mktemp("key_order_" + request.param)
    exe, cases = str(d / "host_key_order"), str(d / "cases.txt")
    flags = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all", "-g"] if request.param == "sanitized" else []
    subprocess.run([hipcc, "--cuda-host-only", "-O2", "-std=c++17", *flags, os.path.join(ROOT, "tests", "host_key_order_harness.hip"), "-o", exe], check=True, timeout=300)
    case_file(cases)
    run = subprocess.run([exe, cases], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, (run.stdout[-500:], run.stderr)
    assert run.stderr == "", run.stderr
    lines = [ln.split() for ln in run.stdout.splitlines()]
    assert [ln[0] for ln in lines] == ["pair"] * len(PAIRS) + ["diff"] * len(DIFFS) + ["gather"] * 2 + ["sort"] * len(SORTS)
    return {"pair": lines[:len(PAIRS)], "diff": lines[len(PAIRS):len(PAIRS) + len(DIFFS)], "gather": lines[len(PAIRS) + len(DIFFS):len(PAIRS) + len(DIFFS) + 2],
            "sort": lines[len(PAIRS) + len(DIFFS) + 2:]}


def test_first_differing_limb_difference_and_inverse(outputs):
    seen = set()
    for (name, cur, prev), out in zip(PAIRS, outputs["pair"]):
        cols = kc.order_columns([prev, cur])
        j, d = int(out[1]), int(out[2])
        assert j == cols["index"][1] and d % P == cols["diff"][1] and -65535 <= d <= 65535, name
        assert int(out[3], 16) == cols["diff"][1] * R256 % P and int(out[4], 16) == cols["inv"][1] * R256 % P, name
        seen.add((j, d > 0))
    assert seen >= {(j, s) for j in range(32) for s in (True, False)}
    by_name = {name: out for (name, _, _), out in zip(PAIRS, outputs["pair"])}
    assert by_name["equal"][1:3] == ["31", "0"] and by_name["zeros"][1:3] == ["31", "0"] and int(by_name["equal"][3], 16) == 0 == int(by_name["equal"][4], 16)
    assert by_name["largest difference"][1:3] == ["0", "65535"] and by_name["smallest difference"][1:3] == ["0", "-65535"]


def test_the_difference_as_a_canonical_element(outputs):
    assert {0, 1, -1, 65535, -65535} <= set(DIFFS)
    for d, out in zip(DIFFS, outputs["diff"]):
        got = int(out[1], 16)
        assert got < P and got == d % P * R256 % P, d


def test_gathers_at_every_legal_offset_and_width(outputs):
    assert len(LEGAL) == 64 + 63 + 61
    for rec, out in zip((GATHER, bytes(range(1, 65))), outputs["gather"]):
        got = [int(x, 16) for x in out[1:]]
        assert got == [int.from_bytes(rec[off:off + width], "big") for off, width in LEGAL]
        assert got == [col[0] for col in kc.gather([rec], LEGAL)]


def test_whole_sorts_give_the_models_permutation_and_stay_below_n(outputs):
    for (name, keys, mask), out in zip(SORTS, outputs["sort"]):
        n = len(keys)
        passes, top, perm = int(out[1]), int(out[2]), [int(x) for x in out[3:]]
        assert perm == kc.sort_perm(keys, mask), name
        assert top == (n if passes else 0), name                           # the largest destination of a live pass is n - 1: a permutation
        varying = sum(1 for j in range(64) if mask[j] and len({k[j] for k in keys}) > 1)
        assert passes == varying, name                                     # exactly the kept bytes at which the records differ
    by_name = {name: out for (name, _, _), out in zip(SORTS, outputs["sort"])}
    assert int(by_name["all equal, two tiles and a bit"][1]) == 0 and int(by_name["mask of zeros"][1]) == 0
    assert by_name["realistic rows, full mask"][3:] == by_name["realistic rows, no counter"][3:]

"""CPU: the framing of the reference's Poseidon code hash (eth-types/src/utils/codehash.rs) that ZK_OP_POSEIDON is tested against: the
helper's sponge over oracle.hashes.poseidon_spec(3, 8, 57) reproduces the reference's five known answers (codes of 0, 1, 2, 32 and
5 036 bytes, the last being 82 blocks), and so does the same sponge driven through the library's zk_host_poseidon_permute_width3."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import poseidon_cases as pc  # noqa: E402

VECTORS = pc.golden_vectors()


def test_the_fixture_holds_the_five_vectors_with_their_source_lines():
    assert [len(code) for code, _ in VECTORS] == [0, 1, 2, 32, 5036]
    assert VECTORS[3][0] == bytes([1] * 32)
    assert len(pc.padded_bytes(VECTORS[4][0])) // 62 == 82
    import json
    raw = json.load(open(pc.GOLDEN))
    assert all(v["ref"].startswith("eth-types/src/utils/codehash.rs:") for v in raw["vectors"])


@pytest.mark.parametrize("index", range(5))
def test_helper_reproduces_the_reference(index):
    code, want = VECTORS[index]
    assert pc.code_hash(code) == want


def test_empty_code_is_one_permutation_of_zeros():
    assert pc.code_hash(b"") == pc.SPEC.permute([0, 0, 0])[0] == VECTORS[0][1]


def test_rows_and_final_column_of_the_model_give_the_same_hashes():
    codes = [code for code, _ in VECTORS]
    data, kinds, lens = pc.code_rows(codes)
    n = len(kinds)
    assert n == 1 + 1 + 1 + 1 + 82
    in0, in1 = pc.rows_of_bytes(data, n)
    out, w0, w1 = pc.expected(in0, in1, lens, kinds, pc.CAP_SCALE_CODE, final=True)
    at = 0
    for code, want in VECTORS:
        rows = len(pc.padded_bytes(code)) // 62
        assert out[at:at + rows] == [want] * rows
        at += rows
    running, _, _ = pc.expected(in0, in1, lens, kinds, pc.CAP_SCALE_CODE)
    assert running[-1] == VECTORS[4][1] and len(set(running[4:])) == 82


@pytest.mark.parametrize("index", range(5))
def test_library_host_permutation_reproduces_the_reference(zk, cref, index):
    def permute(state):
        return [int(v) for v in cref.from_mont(zk.binding.host_poseidon_permute_width3(cref.to_mont(state)))]
    code, want = VECTORS[index]
    assert pc.code_hash(code, permute) == want

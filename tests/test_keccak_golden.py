"""CPU: what ZK_OP_KECCAK is tested against.  The model of tests/keccak_cases.py reproduces keccak256("") as the reference holds it
(eth-types/src/lib.rs:274, tests/golden/reference_vectors.json) and the published keccak256("abc"); its output_rlc has the byte order
of the table (zkevm-circuits/src/table.rs:1493-1498: the digest as a big-endian word, its little-endian bytes under rlc::value, so
digest[0] carries the highest power); and the library's zk_host_keccak256, the function the device op states it computes, agrees
with the model on every length of the shared list."""
import os
import random
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import keccak_cases as kc  # noqa: E402


def test_the_model_reproduces_the_reference_held_empty_digest():
    want = kc.empty_digest()
    assert want.hex().startswith("c5d2") and want.hex().endswith("a470") and len(want) == 32
    assert kc.expected([b""], 1, 1)[0] == [want]


def test_the_model_reproduces_the_published_vector():
    vectors = kc.published_vectors()
    assert [m for m, _ in vectors] == [b"abc"]
    for message, digest in vectors:
        assert kc.expected([message], 1, 1)[0] == [digest]
        assert digest.hex() == "4e03657aea45a94fc7d47ba826c8d667c0d1e6e33a64a036ec44f58fa12d6c45"


def test_output_rlc_at_256_is_the_big_endian_digest():
    """r = 256 makes the RLC the integer whose base-256 digits are the bytes in RLC order: digest[0] is the top digit"""
    _, out, inp = kc.expected([b""], 256, 256)
    assert out == [int.from_bytes(kc.empty_digest(), "big") % kc.P]
    assert inp == [0]
    _, _, inp = kc.expected([b"abc"], 5, 256)
    assert inp == [0x616263]


def test_the_length_list_is_the_one_the_issue_states():
    assert kc.LENGTHS == [0, 1, 7, 8, 9, 63, 64, 127, 128, 129, 134, 135, 136, 137, 143, 144, 271, 272, 273, 408, 1000, 2049]


def test_library_host_keccak_agrees_with_the_model_on_the_length_list(zk):
    rng = random.Random(0xCECCA)
    messages = [bytes(rng.randrange(256) for _ in range(n)) for n in kc.LENGTHS] + [b"\xff" * n for n in (135, 136, 137)]
    digests, _, _ = kc.expected(messages, 1, 1)
    for message, want in zip(messages, digests):
        assert zk.binding.host_keccak256(message) == want, len(message)

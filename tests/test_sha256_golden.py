"""CPU: what ZK_OP_SHA256 is tested against.  The model of tests/sha256_cases.py (hashlib.sha256 and Python integers) reproduces the
five message/digest pairs the reference holds (zkevm-circuits/src/sha256_circuit/circuit.rs:1198-1227,
tests/golden/sha256_reference.json); its output_rlc has the byte order of the table (zkevm-circuits/src/table.rs:1660-1662: the
digest as a big-endian word, its little-endian bytes under rlc::value, so digest[0] carries the highest power -- the circuit's
"the first byte is multiplied with R^31"); input_rlc runs the same way over the message."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import sha256_cases as sc  # noqa: E402


def test_the_model_reproduces_the_five_reference_held_digests():
    vectors = sc.reference_vectors()
    assert {name: m for name, (m, _) in vectors.items()} == {"abc": b"abc", "abd": b"abd", "a x 64": b"a" * 64, "a x 65": b"a" * 65, "empty": b""}
    for name, (message, digest) in vectors.items():
        assert len(digest) == 32
        assert sc.expected([message], 1, 1)[0] == [digest], name
    starts = {name: d.hex()[:8] for name, (_, d) in vectors.items()}
    assert starts == {"abc": "ba7816bf", "abd": "a52d159f", "a x 64": "ffe054fe", "a x 65": "635361c4", "empty": "e3b0c442"}
    assert sc.empty_digest().hex() == "e3b0c44298fc1c149afbf4c8996fb92427ae41e4649b934ca495991b7852b855"


def test_output_rlc_at_256_is_the_big_endian_digest():
    """r = 256 makes the RLC the integer whose base-256 digits are the bytes in RLC order: digest[0] is the top digit"""
    _, out, inp = sc.expected([b""], 256, 256)
    assert out == [int.from_bytes(sc.empty_digest(), "big") % sc.P]
    assert inp == [0]


def test_input_rlc_of_abc_at_256():
    _, _, inp = sc.expected([b"abc"], 5, 256)
    assert inp == [0x616263]
    assert sc.horner(b"abc", 7) == 0x61 * 49 + 0x62 * 7 + 0x63 and sc.mont([1]) == [sc.R256]


def test_the_length_list_is_the_one_the_issue_states():
    assert sc.LENGTHS == [0, 1, 3, 4, 5, 7, 8, 9, 31, 32, 54, 55, 56, 57, 59, 60, 61, 63, 64, 65, 119, 120, 121, 127, 128, 129, 183, 184, 191, 192, 1000, 2049]

"""Helper (not collected): the model of ZK_OP_SHA256 in Python integers over hashlib.sha256 -- the digests and the two
challenge-phase columns of the reference's SHA256Table (zkevm-circuits/src/table.rs:1600-1719) -- and the shared list of lengths
at which loading or padding can go wrong (64-byte blocks of big-endian 32-bit words: around one word, the 55/56 boundary behind
which the length no longer fits the block, one, two and three blocks, and the second-block case behind each)."""
import hashlib
import json
import os

from oracle import bn254 as o

P = o.R_MOD
R256 = (1 << 256) % P
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sha256_reference.json")
LENGTHS = [0, 1, 3, 4, 5, 7, 8, 9, 31, 32, 54, 55, 56, 57, 59, 60, 61, 63, 64, 65, 119, 120, 121, 127, 128, 129, 183, 184, 191, 192, 1000, 2049]


def reference_vectors():
    """{name: (message bytes, digest bytes)} as the reference holds them (sha256_circuit/circuit.rs:1198-1227)"""
    return {v["name"]: (bytes.fromhex(v["message"]), bytes.fromhex(v["digest"])) for v in json.load(open(GOLDEN))["vectors"]}


def empty_digest():
    return reference_vectors()["empty"][1]


def horner(data, r):
    """sum_k data[k] r^(len-1-k): rlc::value over the bytes reversed"""
    acc = 0
    for b in data:
        acc = (acc * r + b) % P
    return acc


def expected(messages, r_out, r_in):
    """(digests as bytes, output_rlc, input_rlc) -- the RLCs as integers (not Montgomery).  output_rlc = sum_k digest[k] r_out^(31-k) =
    rlc::value(Word::from_big_endian(output).to_le_bytes(), challenge); input_rlc = rlc::value(input.iter().rev(), challenge)."""
    digests = [hashlib.sha256(bytes(m)).digest() for m in messages]
    return digests, [horner(d, r_out) for d in digests], [horner(m, r_in) for m in messages]


def mont(values):
    return [v * R256 % P for v in values]

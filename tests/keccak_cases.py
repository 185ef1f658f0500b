"""Helper (not collected): the model of ZK_OP_KECCAK in Python integers over oracle.hashes.keccak256 -- the digests and the two
challenge-phase columns of the reference's KeccakTable (zkevm-circuits/src/table.rs:1433-1506) -- and the shared list of lengths
at which absorbing or padding can go wrong (rate 136: around one word, one block, two and three blocks, the 0x81 case at 135)."""
import json
import os

from oracle import bn254 as o
from oracle import hashes

P = o.R_MOD
R256 = (1 << 256) % P
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "keccak_published.json")
REFERENCE_VECTORS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_vectors.json")
LENGTHS = [0, 1, 7, 8, 9, 63, 64, 127, 128, 129, 134, 135, 136, 137, 143, 144, 271, 272, 273, 408, 1000, 2049]


def published_vectors():
    """[(message bytes, digest bytes)]"""
    return [(bytes.fromhex(v["message"]), bytes.fromhex(v["digest"])) for v in json.load(open(GOLDEN))["vectors"]]


def empty_digest():
    """keccak256("") as the reference holds it (eth-types/src/lib.rs:274)"""
    return bytes.fromhex(json.load(open(REFERENCE_VECTORS))["keccak256_empty"]["value"])


def horner(data, r):
    """sum_k data[k] r^(len-1-k): rlc::value over the bytes reversed"""
    acc = 0
    for b in data:
        acc = (acc * r + b) % P
    return acc


def expected(messages, r_out, r_in):
    """(digests as bytes, output_rlc, input_rlc) -- the RLCs as integers (not Montgomery).  output_rlc = sum_k digest[k] r_out^(31-k) =
    rlc::value(Word::from_big_endian(digest).to_le_bytes(), evm_word); input_rlc = rlc::value(input.iter().rev(), keccak_input)."""
    digests = [hashes.keccak256(bytes(m)) for m in messages]
    return digests, [horner(d, r_out) for d in digests], [horner(m, r_in) for m in messages]


def mont(values):
    return [v * R256 % P for v in values]

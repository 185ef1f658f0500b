"""Helper (not collected): the model of ZK_OP_POSEIDON in Python integers over oracle.hashes.poseidon_spec(3, 8, 57) -- the Poseidon
code hash as the reference frames it, the padded-bytes and row builders of the 31-byte layout, and the row-by-row expected out, word0
and word1 columns for any kinds column."""
import json
import os

from oracle import bn254 as o
from oracle import hashes

P = o.R_MOD
R256 = (1 << 256) % P
SPEC = hashes.poseidon_spec(3, 8, 57)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "poseidon_code_hash.json")
HEAD, CONT, OFF = 0, 1, 2
CAP_SCALE_CODE = 1 << 64


def golden_vectors():
    """[(code bytes, hash as an integer)] -- the reference's five known answers"""
    return [(bytes.fromhex(v["code"]), int(v["hash"], 16)) for v in json.load(open(GOLDEN))["vectors"]]


def words31(code):
    """the 31-byte big-endian words of a bytecode, the last one zero-padded on the right, an odd count completed with a zero word"""
    padded = padded_bytes(code)
    return [int.from_bytes(padded[i:i + 31], "big") for i in range(0, len(padded), 31)]


def padded_bytes(code):
    """the bytecode zero-padded to a multiple of 62 bytes (empty code: one block of zeros)"""
    blocks = max(1, -(-len(code) // 62))
    return bytes(code) + bytes(62 * blocks - len(code))


def code_hash(code, permute=SPEC.permute):
    """state (len 2^64, 0, 0); per block state[1] += w0, state[2] += w1, permute; the hash is state[0].  Empty code: permute(0, 0, 0)[0]."""
    w = words31(code)
    s = [len(code) * CAP_SCALE_CODE % P, 0, 0]
    for i in range(0, len(w), 2):
        s = permute([s[0], (s[1] + w[i]) % P, (s[2] + w[i + 1]) % P])
    return s[0]


def code_rows(codes):
    """the table rows of bytecodes laid end to end: (all padded bytes, kinds, capacity column = the byte length on every row of a code)"""
    data, kinds, lens = b"", [], []
    for code in codes:
        pb = padded_bytes(code)
        rows = len(pb) // 62
        data += pb
        kinds += [HEAD] + [CONT] * (rows - 1)
        lens += [len(code)] * rows
    return data, kinds, lens


def rows_of_bytes(data, n):
    """in0, in1 of the 31-byte layout: cell i of in0 at 62 i, of in1 at 62 i + 31"""
    return ([int.from_bytes(data[62 * i:62 * i + 31], "big") for i in range(n)], [int.from_bytes(data[62 * i + 31:62 * i + 62], "big") for i in range(n)])


def expected(in0, in1, cap=None, kinds=None, cap_scale=1, final=False):
    """(out, word0, word1) as integers (not Montgomery) for value columns in0, in1, cap"""
    n = len(in0)
    out, w0, w1 = [0] * n, [0] * n, [0] * n
    state, start = [0, 0, 0], None
    spans = []
    for i in range(n):
        kind = HEAD if kinds is None else kinds[i] & 3
        if kind >= OFF:
            if start is not None:
                spans.append((start, i))
            state, start = [0, 0, 0], None
            continue
        if kind == HEAD:
            if start is not None:
                spans.append((start, i))
            state, start = [(cap_scale * cap[i]) % P if cap is not None else 0, 0, 0], i
        elif start is None:
            start = i
        state = SPEC.permute([state[0], (state[1] + in0[i]) % P, (state[2] + in1[i]) % P])
        out[i], w0[i], w1[i] = state[0], in0[i] % P, in1[i] % P
    if start is not None:
        spans.append((start, n))
    if final:
        for a, b_ in spans:
            for i in range(a, b_):
                out[i] = out[b_ - 1]
    return out, w0, w1


def mont(values):
    return [v * R256 % P for v in values]

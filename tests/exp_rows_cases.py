"""The exponentiation circuit's rows twice over, and the scenarios the tests of ZK_OP_EXP_ROWS share.

assign(events, n)   the reference's serial loop restated block by block (file:line of zkevm-circuits at each block): exp_by_squaring,
                    assign_exp_events with its padding loop and unusable rows, ExpTable::assignments, MulAddChip::assign with its
                    wrapping U256 arithmetic, the range chip's to_repr chunks.
closed(events, n)   what the op computes: the closed forms of include/zkmi355.h, no walk over an event.

Both return {column: [int] * n} over COLUMNS, the 36 advice columns.  An event is a pair (base, exponent) of integers below 2^256.
Where the events do not fit into n rows the reference asserts; the op writes whole steps only and zeros behind the first step that
does not fit (assign(..., cut=True) stops its walk there, which is the op's rule, not the reference's)."""
import hashlib

import numpy as np

M256, M128, M64 = (1 << 256) - 1, (1 << 128) - 1, (1 << 64) - 1
OFFSET_INCREMENT, UNUSABLE_EXP_ROWS = 8, 10               # exp_circuit/param.rs:3, :11
T = 1024                                                  # the implementation's row tile

TABLE_COLUMNS = ("is_last", "base_limb", "exponent_lo_hi", "exponentiation_lo_hi")
CHIP_COLUMNS = tuple(f"cols.{c}" for c in range(4)) + tuple(f"u16_64.{c}" for c in range(4)) + tuple(f"u16_128.{c}" for c in range(8))
COLUMNS = TABLE_COLUMNS + tuple(f"mul_{c}" for c in CHIP_COLUMNS) + tuple(f"parity_{c}" for c in CHIP_COLUMNS)
assert len(COLUMNS) == 36
# the op's outputs: (name, cell bytes, planes); exponentiation_lo_hi is d_out
OUTPUTS = (("exponentiation_lo_hi", 16, 1), ("is_last", 1, 1), ("base_limb", 8, 1), ("exponent_lo_hi", 16, 1), ("mul_cols", 16, 4), ("mul_u16_64", 2, 4), ("mul_u16_128", 2, 8),
           ("parity_cols", 16, 4), ("parity_u16_64", 2, 4), ("parity_u16_128", 2, 8))
U16_OUTPUTS = ("mul_u16_64", "mul_u16_128", "parity_u16_64", "parity_u16_128")


def limbs64(v):
    return [v >> 64 * i & M64 for i in range(4)]


def lo_hi(v):
    return v & M128, v >> 128


# ---- the reference, block by block ----------------------------------------------------------------------------------------------------------
def exp_by_squaring(base, exponent, steps):
    """bus-mapping/src/evm/opcodes/exp.rs:12-34"""
    if exponent == 0:
        return 1
    if exponent == 1:
        return base
    exponent_div2, odd = divmod(exponent, 2)
    exp1 = exp_by_squaring(base, exponent_div2, steps)
    exp2 = exp1 * exp1 & M256                                           # overflowing_mul
    steps.append((exp1, exp1, exp2))
    if odd == 0:
        return exp2
    exp = base * exp2 & M256
    steps.append((exp2, base, exp))
    return exp


def mul_add_assign(cols, prefix, offset, words):
    """gadgets/src/mul_add.rs:261-415 MulAddChip::assign, and gadgets/src/range.rs:108-136 for the two range chips"""
    a, b, c, d = words
    a_limbs, b_limbs = limbs64(a), limbs64(b)
    (c_lo, c_hi), (d_lo, d_hi) = lo_hi(c), lo_hi(d)
    t0 = a_limbs[0] * b_limbs[0]
    t1 = a_limbs[0] * b_limbs[1] + a_limbs[1] * b_limbs[0]
    t2 = a_limbs[0] * b_limbs[2] + a_limbs[1] * b_limbs[1] + a_limbs[2] * b_limbs[0]
    t3 = a_limbs[0] * b_limbs[3] + a_limbs[1] * b_limbs[2] + a_limbs[2] * b_limbs[1] + a_limbs[3] * b_limbs[0]
    c_lo_minus_d_lo = (c_lo - d_lo) & M256                              # overflowing_sub
    temp = t0 + (t1 << 64)
    assert temp <= M256
    carry_lo = ((temp + c_lo_minus_d_lo) & M256) >> 128                 # overflowing_add
    carry_lo_minus_d_hi = (carry_lo - d_hi) & M256
    temp = t2 + (t3 << 64) + c_hi
    assert temp <= M256
    carry_hi = ((temp + carry_lo_minus_d_hi) & M256) >> 128
    col = [cols[f"{prefix}_cols.{i}"] for i in range(4)]
    for i in range(4):                                                  # mul_add.rs:291-328 a limbs, b limbs
        col[i][offset] = a_limbs[i]
        col[i][offset + 1] = b_limbs[i]
    for i, v in enumerate((c_lo, c_hi, d_lo, d_hi)):                    # mul_add.rs:341-365
        col[i][offset + 2] = v
    for row, carry in ((3, carry_lo), (5, carry_hi)):                   # mul_add.rs:377-412: the first five of to_le_u16_array
        digits = [carry >> 16 * i & 0xFFFF for i in range(16)]
        for (cc, rr), v in zip([(0, row), (1, row), (2, row), (3, row), (0, row + 1)], digits):
            col[cc][offset + rr] = v
    # range.rs:117-133: value.to_repr() in chunks of two bytes, the first N_2BYTE of them
    for row_idx, value in enumerate(a_limbs + b_limbs):                 # mul_add.rs:329-339 range_check_64
        repr_ = value.to_bytes(32, "little")
        for col_idx in range(4):
            cols[f"{prefix}_u16_64.{col_idx}"][offset + row_idx] = repr_[2 * col_idx] | repr_[2 * col_idx + 1] << 8
    for row_idx, value in enumerate((c_lo, c_hi, d_lo, d_hi)):          # mul_add.rs:366-375 range_check_128
        repr_ = value.to_bytes(32, "little")
        for col_idx in range(8):
            cols[f"{prefix}_u16_128.{col_idx}"][offset + row_idx] = repr_[2 * col_idx] | repr_[2 * col_idx + 1] << 8


def exp_table_assignments(base, exponent, steps):
    """zkevm-circuits/src/table.rs:2207-2271 ExpTable::assignments: rows of [is_last, base_limb, exponent_lo_hi, exponentiation_lo_hi]"""
    assignments = []
    base_limbs = limbs64(base)
    for step_idx, (_, _, d) in enumerate(reversed(steps)):
        is_last = int(step_idx == len(steps) - 1)
        exp_lo, exp_hi = lo_hi(d)
        exponent_lo, exponent_hi = lo_hi(exponent)
        assignments.append([is_last, base_limbs[0], exponent_lo, exp_lo])
        assignments.append([0, base_limbs[1], exponent_hi, exp_hi])
        assignments.append([0, base_limbs[2], 0, 0])
        assignments.append([0, base_limbs[3], 0, 0])
        for _ in range(4, OFFSET_INCREMENT):
            assignments.append([0, 0, 0, 0])
        exponent_div2, remainder = divmod(exponent, 2)
        exponent = exponent_div2 if remainder == 0 else exponent - 1
    return assignments


def assign(events, n, cut=False):
    cols = {name: [0] * n for name in COLUMNS}
    events = [(b, x, _steps(b, x)) for b, x in events]
    min_num_rows = sum(len(s) * OFFSET_INCREMENT for _, _, s in events) + UNUSABLE_EXP_ROWS   # exp_circuit.rs:516-522
    assert cut or min_num_rows <= n, "insufficient rows to populate the exponentiation trace"   # exp_circuit.rs:332-335
    state = {"offset": 0, "full": False}

    def assign_exp_event(base, exponent0, steps):
        """exp_circuit.rs:390-448, with assign_step :450-482"""
        exponent = exponent0
        table = exp_table_assignments(base, exponent0, steps)
        for k, (a, b, d) in enumerate(reversed(steps)):
            offset = state["offset"]
            if cut and (state["full"] or offset + OFFSET_INCREMENT + UNUSABLE_EXP_ROWS > n):
                state["full"] = True
                return
            exponent_div2, remainder = divmod(exponent, 2)
            mul_add_assign(cols, "mul", offset, (a, b, 0, d))                                  # :470
            mul_add_assign(cols, "parity", offset, (2, exponent_div2, remainder, exponent))    # :471
            exponent = exponent_div2 if remainder == 0 else exponent - 1                       # :474-480
            for i, row in enumerate(table[k * OFFSET_INCREMENT:(k + 1) * OFFSET_INCREMENT]):   # :415-427
                for name, v in zip(TABLE_COLUMNS, row):
                    cols[name][offset + i] = v
            state["offset"] += OFFSET_INCREMENT                                                # :445

    for base, exponent, steps in events:                                                       # :349-357
        assign_exp_event(base, exponent, steps)
    pad = (2, 2, _steps(2, 2))                                                                 # ExpEvent::default(): base 2, exponent 2
    while not state["full"] and n >= UNUSABLE_EXP_ROWS and state["offset"] + OFFSET_INCREMENT <= n - UNUSABLE_EXP_ROWS:   # :362
        assign_exp_event(*pad)
    # :384 assign_unused_rows: UNUSABLE_EXP_ROWS rows of zeros, which is what every row behind the offset holds already
    return cols


def _steps(base, exponent):
    steps = []
    exp_by_squaring(base, exponent, steps)
    return steps


# ---- the op's closed forms --------------------------------------------------------------------------------------------------------------------
def steps_of(x):
    return 0 if x < 2 else (x.bit_length() - 1) + (bin(x).count("1") - 1)


def rows_needed(events):
    return 8 * sum(steps_of(x) for _, x in events) + 10


def step_exponent(x, j):
    P = lambda i: i + bin(x & ((1 << i) - 1)).count("1")   # noqa: E731
    lo, hi = 0, x.bit_length() - 1
    while lo < hi:
        mid = (lo + hi + 1) // 2
        if P(mid) <= j:
            lo = mid
        else:
            hi = mid - 1
    xj = x >> lo
    return xj & ~1 if j - P(lo) == 1 else xj


def muladd_witness(a, b, c, d):
    """{(row, col): 16-byte cell}, {(row, col): u16 of range_check_64}, {(row, col): u16 of range_check_128} of one chip"""
    al, bl = limbs64(a), limbs64(b)
    t = [sum(al[i] * bl[k - i] for i in range(k + 1)) for k in range(4)]
    (c_lo, c_hi), (d_lo, d_hi) = lo_hi(c), lo_hi(d)
    carry_lo = ((t[0] + (t[1] << 64) + c_lo - d_lo) & M256) >> 128
    carry_hi = ((t[2] + (t[3] << 64) + c_hi + carry_lo - d_hi) & M256) >> 128
    cells = {}
    for i in range(4):
        cells[0, i], cells[1, i], cells[2, i] = al[i], bl[i], (c_lo, c_hi, d_lo, d_hi)[i]
        cells[3, i], cells[5, i] = carry_lo >> 16 * i & 0xFFFF, carry_hi >> 16 * i & 0xFFFF
    cells[4, 0], cells[6, 0] = carry_lo >> 64 & 0xFFFF, carry_hi >> 64 & 0xFFFF
    u64 = {(r, c): v >> 16 * c & 0xFFFF for r, v in enumerate(al + bl) for c in range(4)}
    u128 = {(r, c): v >> 16 * c & 0xFFFF for r, v in enumerate((c_lo, c_hi, d_lo, d_hi)) for c in range(8)}
    return cells, u64, u128


def closed(events, n):
    cols = {name: [0] * n for name in COLUMNS}

    def put_step(o, base, is_last, x, a, b, d):
        cols["is_last"][o] = is_last
        for r in range(4):
            cols["base_limb"][o + r] = base >> 64 * r & M64
        cols["exponent_lo_hi"][o], cols["exponent_lo_hi"][o + 1] = lo_hi(x)
        cols["exponentiation_lo_hi"][o], cols["exponentiation_lo_hi"][o + 1] = lo_hi(d)
        for prefix, words in (("mul", (a, b, 0, d)), ("parity", (2, x >> 1, x & 1, x))):
            cells, u64, u128 = muladd_witness(*words)
            for (r, c), v in cells.items():
                cols[f"{prefix}_cols.{c}"][o + r] = v
            for (r, c), v in u64.items():
                cols[f"{prefix}_u16_64.{c}"][o + r] = v
            for (r, c), v in u128.items():
                cols[f"{prefix}_u16_128.{c}"][o + r] = v

    live = lambda o: o + 8 + 10 <= n   # noqa: E731
    start = 0
    for base, x in events:
        S = steps_of(x)
        for j in range(S):
            o = start + 8 * j
            if not live(o):
                return cols                                             # nothing behind a step that does not fit
            xj = step_exponent(x, j)
            d = pow(base, xj, 1 << 256)
            a = pow(base, xj - 1, 1 << 256) if xj & 1 else pow(base, xj // 2, 1 << 256)
            put_step(o, base, int(j == S - 1), xj, a, base if xj & 1 else a, d)
        start += 8 * S
    while live(start):
        put_step(start, 2, 1, 2, 2, 2, 4)
        start += 8
    return cols


# ---- bytes as the op lays them out --------------------------------------------------------------------------------------------------------------
def pack_events(events):
    """count x 64 B: base, then exponent, little-endian"""
    return np.frombuffer(b"".join(b.to_bytes(32, "little") + x.to_bytes(32, "little") for b, x in events), dtype=np.uint8).copy()


def output_bytes(cols, n, name):
    """the n rows of output `name` of OUTPUTS as the device holds them: planes one behind the other"""
    width, planes = next((w, p) for o, w, p in OUTPUTS if o == name)
    if planes == 1:
        return b"".join(v.to_bytes(width, "little") for v in cols[name])
    prefix, kind = name.split("_", 1)
    return b"".join(v.to_bytes(width, "little") for c in range(planes) for v in cols[f"{prefix}_{kind}.{c}"])


def column_digest(values):
    return hashlib.sha256(b"".join(v.to_bytes(16, "little") for v in values)).hexdigest()


# ---- scenarios: name -> (events, n) ---------------------------------------------------------------------------------------------------------------
RANDOM_WORD = 0xB5C0FBCFEC4D3B2F9A1E07D6A8C4E1F3D2B6A5948372615F0E1D2C3B4A596877
EXPONENTS = (0, 1, 2, 3, 4, 1 << 64, 1 << 128, (1 << 128) + 1, 1 << 255, M256)
BASES = (0, 1, 2, M64, M256, RANDOM_WORD)


def fit(events, extra=0):
    return events, rows_needed(events) + extra


def scenarios():
    rng = np.random.default_rng(0xE4B)
    word = lambda bits: int.from_bytes(rng.bytes(32), "little") >> (256 - bits)   # noqa: E731
    s = {}
    # every exponent with every base; the long ones (2^255: 255 steps, 2^256 - 1: 510) once per base class to stay small
    short = [x for x in EXPONENTS if steps_of(x) <= 130]
    s["every_short_exponent_with_every_base"] = fit([(b, x) for x in short for b in BASES], extra=8 * 3 + 5)
    s["exponent_2_255_with_every_base"] = fit([(b, 1 << 255) for b in BASES])
    s["exponent_all_ones_with_extreme_bases"] = fit([(M256, M256), (RANDOM_WORD, M256)], extra=3)
    s["empty_events_front_middle_back"] = fit([(5, 0), (7, 1), (3, 13), (9, 1), (11, 0), (RANDOM_WORD, 6), (2, 1), (4, 0)], extra=16)
    s["only_empty_events"] = ([(3, 0), (3, 1)], 40)
    s["no_events"] = ([], T + 8 + 5)
    s["one_510_step_event_across_four_tiles"] = fit([(RANDOM_WORD | 1, M256)], extra=8 * 2 + 1)
    # an event boundary at rows 1016, 1024, 1032: a first event of 127, 128, 129 steps
    x127 = 1 << 127                                                     # 127 steps, one more with every further bit
    assert steps_of(x127) == 127 and steps_of(x127 | 1) == 128 and steps_of(x127 | 3) == 129
    for rows, x in ((1016, x127), (1024, x127 | 1), (1032, x127 | 3)):
        s[f"event_boundary_at_row_{rows}"] = fit([(RANDOM_WORD, x), (M64, 0xDEADBEEF), (3, 2)], extra=8)
    s["2049_one_step_events"] = fit([(word(256), 2) for _ in range(2049)], extra=8)
    s["4097_one_step_events_cut_at_2_15_rows"] = ([(word(64), 2) for _ in range(4097)], 1 << 15)
    mixed = [(word(int(rng.integers(1, 257))), word(int(rng.integers(1, 130)))) for _ in range(12)]
    s["mixed_random_events"] = fit(mixed, extra=8 * 4 + 7)
    few = [(3, 13), (RANDOM_WORD, 6), (7, 1), (M256, 37)]
    for n in (0, 1, 9, 10, 17, 18, 26):
        s[f"n_{n}"] = (few, n)
        s[f"n_{n}_no_events"] = ([], n)
    need = rows_needed(few)
    s["n_exactly_needed"] = (few, need)
    s["n_one_step_more"] = (few, need + 8)
    s["n_seven_more_is_no_pad_step"] = (few, need + 7)
    s["n_cuts_an_event_midway"] = (few, need - 8 * 3)
    s["n_cuts_at_one_row_short"] = (few, need - 1)
    s["n_cuts_inside_the_first_event"] = (few, 8 * 2 + 10 + 3)
    s["n_cuts_a_long_event_behind_a_tile_edge"] = ([(RANDOM_WORD, M256)], 2 * T + 8 * 5 + 10 + 4)
    return s


def fits(events, n):
    return rows_needed(events) <= n

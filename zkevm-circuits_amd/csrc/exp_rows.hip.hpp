// Lane-free code of ZK_OP_EXP_ROWS (csrc/exp_rows.hip holds the kernels and the host side): a 256-bit integer word and its truncated
// multiply, the steps of an exponentiation event as closed forms of (exponent, step), the MulAdd witness of a * b + c == d mod 2^256
// and what one row of the exponentiation circuit holds.  Nothing here names a thread, a wave or LDS, so the host compiles it as it
// stands: tests/host_exp_rows_harness.hip drives whole small inputs serially through exactly these functions.  The arithmetic is on
// integers, not on field elements; later integer gadgets can take ExWord, ex_mul and ex_muladd_witness from here.
//
// Steps.  An event (base, x) with x >= 2 has S = (bitlen(x) - 1) + (popcount(x) - 1) steps of 8 rows (exp_circuit OFFSET_INCREMENT),
// in the reference's reversed order: step 0 holds d = base^x.  With P(i) = i + popcount(x mod 2^i) and i the largest index with
// P(i) <= j, step j holds the intermediate exponent x_j = x >> i, bit 0 cleared when j - P(i) == 1, and d_j = base^(x_j) mod 2^256;
// x_j odd: a_j = base^(x_j - 1), b_j = base; x_j even: a_j = b_j = base^(x_j / 2).  a_j is d_(j + 1), and base on the last step,
// where x_j == 2.  So the only serial part of an event is the chain d_(S - 1) .. d_0: square and multiply from the top bit down
// (ex_chain_next).  x < 2 gives no steps.
//
// Rows.  Event e owns the 8 S_e rows from start_e = sum_(c<e) 8 S_c (exclusive scan under bc_sat_add, saturating at n).  A step slot
// at row o (a multiple of 8) is live where its 8 rows lie below the n - 10 rows in use (exp_circuit UNUSABLE_EXP_ROWS): o + 18 <= n.
// A live slot below start_count holds a step of an event, a live slot behind it the padding step (base 2, exponent 2); every other
// row is zero.
#pragma once
#include "bytecode_rows.hip.hpp"

namespace zk {

constexpr uint32_t EX_STEP_ROWS = 8, EX_UNUSABLE = 10, EX_EVENT_BYTES = 64, EX_EVENT_WORDS = 8;
constexpr uint32_t EX_TILE = 1024, EX_TILE_STEPS = EX_TILE / EX_STEP_ROWS;

// ---- 256-bit words ------------------------------------------------------------------------------------------------------------------------
struct ExWord { uint64_t w[4]; };                                     // little-endian 64-bit limbs

ZK_BC_HD ExWord ex_word(uint64_t v) { return ExWord{{v, 0, 0, 0}}; }
// which ? a : b, limb by limb: a choice between two words in memory would keep both there
ZK_BC_HD ExWord ex_select(bool which, const ExWord& a, const ExWord& b) {
    return ExWord{{which ? a.w[0] : b.w[0], which ? a.w[1] : b.w[1], which ? a.w[2] : b.w[2], which ? a.w[3] : b.w[3]}};
}
ZK_BC_HD bool ex_lt2(const ExWord& x) { return x.w[0] < 2 && !(x.w[1] | x.w[2] | x.w[3]); }
ZK_BC_HD uint32_t ex_popc64(uint64_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
    return (uint32_t)__popcll(v);
#else
    return (uint32_t)__builtin_popcountll(v);
#endif
}
ZK_BC_HD uint32_t ex_clz64(uint64_t v) {                              // v != 0
#if defined(__HIP_DEVICE_COMPILE__)
    return (uint32_t)__clzll((long long)v);
#else
    return (uint32_t)__builtin_clzll(v);
#endif
}
// a * b as (lo, hi)
ZK_BC_HD void ex_mul64(uint64_t a, uint64_t b, uint64_t& lo, uint64_t& hi) {
#if defined(__HIP_DEVICE_COMPILE__)
    lo = a * b, hi = __umul64hi(a, b);
#else
    const unsigned __int128 p = (unsigned __int128)a * b;
    lo = (uint64_t)p, hi = (uint64_t)(p >> 64);
#endif
}
// (c0, c1, c2) += a * b: a sum of up to four such products fits in 130 bits
ZK_BC_HD void ex_mac(uint64_t a, uint64_t b, uint64_t& c0, uint64_t& c1, uint64_t& c2) {
    uint64_t lo, hi;
    ex_mul64(a, b, lo, hi);
    c0 += lo;
    hi += c0 < lo;                                                      // hi <= 2^64 - 2: does not wrap
    c1 += hi;
    c2 += c1 < hi;
}
ZK_BC_HD uint32_t ex_bitlen(const ExWord& x) {
    uint32_t len = 0;
#pragma unroll
    for (uint32_t k = 0; k < 4; ++k) len = x.w[k] ? 64u * k + 64u - ex_clz64(x.w[k]) : len;
    return len;
}
ZK_BC_HD uint32_t ex_popcount(const ExWord& x) { return ex_popc64(x.w[0]) + ex_popc64(x.w[1]) + ex_popc64(x.w[2]) + ex_popc64(x.w[3]); }
ZK_BC_HD uint32_t ex_bit(const ExWord& x, uint32_t i) {              // i < 256; no variable index: the word stays in registers
    uint64_t v = 0;
#pragma unroll
    for (uint32_t k = 0; k < 4; ++k) v = k == i >> 6 ? x.w[k] : v;
    return (uint32_t)(v >> (i & 63u)) & 1u;
}
// popcount(x mod 2^i), i <= 256
ZK_BC_HD uint32_t ex_popcount_below(const ExWord& x, uint32_t i) {
    uint32_t s = 0;
#pragma unroll
    for (uint32_t k = 0; k < 4; ++k) {
        const uint32_t lo = 64u * k;
        const uint64_t m = i >= lo + 64u ? ~0ull : i > lo ? (1ull << (i - lo)) - 1 : 0ull;
        s += ex_popc64(x.w[k] & m);
    }
    return s;
}
// x >> i, i < 256
ZK_BC_HD ExWord ex_shr(const ExWord& x, uint32_t i) {
    const uint32_t q = i >> 6, s = i & 63u;
    ExWord r;
#pragma unroll
    for (uint32_t k = 0; k < 4; ++k) {
        uint64_t lo = 0, hi = 0;
#pragma unroll
        for (uint32_t m = 0; m < 4; ++m) {                              // x.w[k + q] and x.w[k + q + 1] without a variable index
            lo = m == k + q ? x.w[m] : lo;
            hi = m == k + q + 1 ? x.w[m] : hi;
        }
        r.w[k] = s ? lo >> s | hi << (64u - s) : lo;
    }
    return r;
}
// a + b and a - b mod 2^256 (the reference's overflowing_add and overflowing_sub)
ZK_BC_HD ExWord ex_add(const ExWord& a, const ExWord& b) {
    ExWord r;
    uint64_t c = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const uint64_t s = a.w[k] + b.w[k], t = s + c;
        c = (uint64_t)(s < a.w[k]) | (uint64_t)(t < s);
        r.w[k] = t;
    }
    return r;
}
ZK_BC_HD ExWord ex_sub(const ExWord& a, const ExWord& b) {
    ExWord r;
    uint64_t c = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const uint64_t s = a.w[k] - b.w[k], t = s - c;
        c = (uint64_t)(a.w[k] < b.w[k]) | (uint64_t)(s < c);
        r.w[k] = t;
    }
    return r;
}
// a * b mod 2^256 (overflowing_mul): the ten limb products of the low half, column by column
ZK_BC_HD ExWord ex_mul(const ExWord& a, const ExWord& b) {
    ExWord r;
    uint64_t c0 = 0, c1 = 0, c2 = 0;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
#pragma unroll
        for (int i = 0; i <= k; ++i) ex_mac(a.w[i], b.w[k - i], c0, c1, c2);
        r.w[k] = c0, c0 = c1, c1 = c2, c2 = 0;
    }
#pragma unroll
    for (int i = 0; i <= 3; ++i) c0 += a.w[i] * b.w[3 - i];
    r.w[3] = c0;
    return r;
}

// ---- the steps of an event ----------------------------------------------------------------------------------------------------------------
ZK_BC_HD uint32_t ex_steps(const ExWord& x) { return ex_lt2(x) ? 0u : ex_bitlen(x) + ex_popcount(x) - 2u; }
// the rows of an event, saturating at cap = n
ZK_BC_HD uint32_t ex_rows_of(uint32_t steps, uint32_t cap) { return EX_STEP_ROWS * steps < cap ? EX_STEP_ROWS * steps : cap; }
ZK_BC_HD uint32_t ex_P(const ExWord& x, uint32_t i) { return i + ex_popcount_below(x, i); }
// the intermediate exponent of step j < S
ZK_BC_HD ExWord ex_step_exponent(const ExWord& x, uint32_t j) {
    uint32_t lo = 0, hi = ex_bitlen(x) - 1u;
    while (lo < hi) {
        const uint32_t mid = (lo + hi + 1u) >> 1;
        if (ex_P(x, mid) <= j) lo = mid;
        else hi = mid - 1u;
    }
    ExWord xj = ex_shr(x, lo);
    if (j != ex_P(x, lo)) xj.w[0] &= ~1ull;                             // j - P(i) == 1: the squaring behind the multiply by base
    return xj;
}
// a step slot at row o holds a step: its 8 rows lie below the n - 10 rows in use
ZK_BC_HD bool ex_live(uint64_t o, uint64_t n) { return o + EX_STEP_ROWS + EX_UNUSABLE <= n; }
// the chain keeps d_j where step j or step j - 1, which takes it as its a, is live
ZK_BC_HD bool ex_kept(uint64_t o, uint64_t n) { return o + EX_UNUSABLE <= n; }
// The chain d_(S - 1) .. d_0 of an event with S >= 1 steps: acc starts as base, bit as bitlen(x) - 1, j as S.  Each call makes the
// next multiply -- a squaring where the bit below has not been squared in yet, else the multiply by base for a set bit -- and
// names the step j < S whose d it is.
struct ExChain { ExWord acc; uint32_t bit, j; bool squared; };
ZK_BC_HD ExChain ex_chain_begin(const ExWord& base, const ExWord& x) { return ExChain{base, ex_bitlen(x) - 1u, ex_steps(x), false}; }
ZK_BC_HD void ex_chain_next(ExChain& c, const ExWord& base, const ExWord& x) {
    // one multiply whichever it is, its second operand chosen limb by limb: lanes of a wave that differ in kind stay in step
    const bool square = !c.squared;
    c.bit -= square ? 1u : 0u;
    c.acc = ex_mul(c.acc, ex_select(square, c.acc, base));
    c.squared = square && ex_bit(x, c.bit) != 0;                        // a set bit: the multiply by base comes next
    c.j -= 1u;
}

// ---- MulAddChip::assign(offset, [a, b, c, d]) ---------------------------------------------------------------------------------------------
struct ExMulAdd {
    ExWord a, b, c, d;
    uint16_t carry_lo[5], carry_hi[5];
};
ZK_BC_HD ExMulAdd ex_muladd_witness(const ExWord& a, const ExWord& b, const ExWord& c, const ExWord& d) {
    ExMulAdd m;
    m.a = a, m.b = b, m.c = c, m.d = d;
    // t_k = sum_(i<=k) a_i b_(k-i), at most 130 bits each
    uint64_t t[4][3];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        t[k][0] = t[k][1] = t[k][2] = 0;
#pragma unroll
        for (int i = 0; i <= k; ++i) ex_mac(a.w[i], b.w[k - i], t[k][0], t[k][1], t[k][2]);
    }
    // carry_lo = (t0 + (t1 << 64) + (c_lo - d_lo)) >> 128, carry_hi = (t2 + (t3 << 64) + c_hi + (carry_lo - d_hi)) >> 128, every
    // sum and difference mod 2^256 as the reference takes them
    const ExWord c_lo{{c.w[0], c.w[1], 0, 0}}, c_hi{{c.w[2], c.w[3], 0, 0}}, d_lo{{d.w[0], d.w[1], 0, 0}}, d_hi{{d.w[2], d.w[3], 0, 0}};
    const ExWord t0{{t[0][0], t[0][1], t[0][2], 0}}, t1s{{0, t[1][0], t[1][1], t[1][2]}};
    const ExWord t2{{t[2][0], t[2][1], t[2][2], 0}}, t3s{{0, t[3][0], t[3][1], t[3][2]}};
    const ExWord lo = ex_add(ex_add(t0, t1s), ex_sub(c_lo, d_lo));
    const ExWord carry_lo{{lo.w[2], lo.w[3], 0, 0}};
    const ExWord hi = ex_add(ex_add(ex_add(t2, t3s), c_hi), ex_sub(carry_lo, d_hi));
#pragma unroll
    for (int k = 0; k < 5; ++k) {                                       // the first five of to_le_u16_array
        m.carry_lo[k] = (uint16_t)(k < 4 ? lo.w[2] >> (16 * k) : lo.w[3]);
        m.carry_hi[k] = (uint16_t)(k < 4 ? hi.w[2] >> (16 * k) : hi.w[3]);
    }
    return m;
}
struct ExCell { uint64_t lo, hi; };                                   // a 16-byte cell
// the cell of chip column col (0..3) on row r (0..7) of the step
ZK_BC_HD ExCell ex_muladd_cell(const ExMulAdd& m, uint32_t r, uint32_t col) {
    uint64_t a = 0, b = 0, l = 0, h = 0;
#pragma unroll
    for (uint32_t k = 0; k < 4; ++k) {
        a = k == col ? m.a.w[k] : a;
        b = k == col ? m.b.w[k] : b;
        l = k == col ? m.carry_lo[k] : l;
        h = k == col ? m.carry_hi[k] : h;
    }
    switch (r) {
        case 0: return ExCell{a, 0};
        case 1: return ExCell{b, 0};
        case 2:                                                         // c_lo, c_hi, d_lo, d_hi
            return col == 0 ? ExCell{m.c.w[0], m.c.w[1]} : col == 1 ? ExCell{m.c.w[2], m.c.w[3]} : col == 2 ? ExCell{m.d.w[0], m.d.w[1]} : ExCell{m.d.w[2], m.d.w[3]};
        case 3: return ExCell{l, 0};
        case 4: return ExCell{col ? 0u : m.carry_lo[4], 0};
        case 5: return ExCell{h, 0};
        case 6: return ExCell{col ? 0u : m.carry_hi[4], 0};
        default: return ExCell{0, 0};
    }
}
// range_check_64: digit col (0..3) of a_0 .. a_3, b_0 .. b_3 on rows 0 .. 7
ZK_BC_HD uint32_t ex_u16_64(const ExMulAdd& m, uint32_t r, uint32_t col) {
    uint64_t v = 0;
#pragma unroll
    for (uint32_t k = 0; k < 4; ++k) v = k == (r & 3u) ? (r < 4 ? m.a.w[k] : m.b.w[k]) : v;
    return (uint32_t)(v >> (16 * col)) & 0xffffu;
}
// range_check_128: digit col (0..7) of c_lo, c_hi, d_lo, d_hi on rows 0 .. 3, zero below
ZK_BC_HD uint32_t ex_u16_128(const ExMulAdd& m, uint32_t r, uint32_t col) {
    if (r >= 4) return 0;
    const uint32_t k = 2 * (r & 1u) + (col >> 2);                       // the limb of c (rows 0, 1) or d (rows 2, 3)
    uint64_t v = 0;
#pragma unroll
    for (uint32_t q = 0; q < 4; ++q) v = q == k ? (r < 2 ? m.c.w[q] : m.d.w[q]) : v;
    return (uint32_t)(v >> (16 * (col & 3u))) & 0xffffu;
}

// ---- one step -------------------------------------------------------------------------------------------------------------------------------
// what the rows of a step are made from: a zero step (live == false) gives the zero rows
struct ExStep {
    bool live, is_last;
    ExWord base, x, a, b, d;
};
ZK_BC_HD ExStep ex_zero_step() { return ExStep{false, false, ex_word(0), ex_word(0), ex_word(0), ex_word(0), ex_word(0)}; }
// the default event of the padding loop: base 2, exponent 2, one step
ZK_BC_HD ExStep ex_pad_step() { return ExStep{true, true, ex_word(2), ex_word(2), ex_word(2), ex_word(2), ex_word(4)}; }
// step j < S of an event with d = d_j and next = d_(j + 1) (not looked at on the last step)
ZK_BC_HD ExStep ex_event_step(const ExWord& base, const ExWord& x, uint32_t j, const ExWord& d, const ExWord& next) {
    ExStep s;
    s.live = true;
    s.is_last = j + 1u == ex_steps(x);
    s.base = base;
    s.x = ex_step_exponent(x, j);
    s.a = ex_select(s.is_last, base, next);
    s.b = ex_select(s.x.w[0] & 1u, base, s.a);
    s.d = d;
    return s;
}
// the two chips of a step: [a, b, 0, d] and [2, x >> 1, x & 1, x]
ZK_BC_HD ExMulAdd ex_mul_chip(const ExStep& s) { return ex_muladd_witness(s.a, s.b, ex_word(0), s.d); }
ZK_BC_HD ExMulAdd ex_parity_chip(const ExStep& s) {
    if (!s.live) return ex_muladd_witness(ex_word(0), ex_word(0), ex_word(0), ex_word(0));
    return ex_muladd_witness(ex_word(2), ex_shr(s.x, 1), ex_word(s.x.w[0] & 1u), s.x);
}
// ExTable::assignments on row r (0..7) of the step
ZK_BC_HD uint32_t ex_is_last(const ExStep& s, uint32_t r) { return s.is_last && r == 0; }
ZK_BC_HD uint64_t ex_base_limb(const ExStep& s, uint32_t r) {
    uint64_t v = 0;
#pragma unroll
    for (uint32_t k = 0; k < 4; ++k) v = k == r ? s.base.w[k] : v;
    return v;
}
ZK_BC_HD ExCell ex_lo_hi(const ExWord& v, uint32_t r) { return r == 0 ? ExCell{v.w[0], v.w[1]} : r == 1 ? ExCell{v.w[2], v.w[3]} : ExCell{0, 0}; }

// every output cell of one row
struct ExRow {
    uint8_t is_last;
    uint64_t base_limb;
    ExCell exponent_lo_hi, exponentiation_lo_hi, mul_cols[4], parity_cols[4];
    uint16_t mul_u16_64[4], mul_u16_128[8], parity_u16_64[4], parity_u16_128[8];
};
// row r (0..7) of a step and its two chips
ZK_BC_HD ExRow exp_row(const ExStep& s, const ExMulAdd& mul, const ExMulAdd& par, uint32_t r) {
    ExRow o;
    o.is_last = (uint8_t)ex_is_last(s, r);
    o.base_limb = ex_base_limb(s, r);
    o.exponent_lo_hi = ex_lo_hi(s.x, r);
    o.exponentiation_lo_hi = ex_lo_hi(s.d, r);
    for (uint32_t c = 0; c < 4; ++c) {
        o.mul_cols[c] = ex_muladd_cell(mul, r, c);
        o.parity_cols[c] = ex_muladd_cell(par, r, c);
        o.mul_u16_64[c] = (uint16_t)ex_u16_64(mul, r, c);
        o.parity_u16_64[c] = (uint16_t)ex_u16_64(par, r, c);
    }
    for (uint32_t c = 0; c < 8; ++c) {
        o.mul_u16_128[c] = (uint16_t)ex_u16_128(mul, r, c);
        o.parity_u16_128[c] = (uint16_t)ex_u16_128(par, r, c);
    }
    return o;
}

}  // namespace zk

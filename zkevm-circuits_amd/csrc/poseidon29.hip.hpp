// The per-lane arithmetic of ZK_OP_POSEIDON (csrc/poseidon.hip): the width-3 Poseidon permutation of host::PoseidonWidth3
// (csrc/host_hash.hpp: x^5, R_F = 8, R_P = 57, the plain round schedule) on 9 x 29-bit limbs.  __host__ __device__, so that
// tests/host_poseidon_harness.hip runs it on the CPU against Python integers.
//
// Forms.  mul29 is Montgomery by R' = 2^261: write [x]_e for the residue x 2^e, then mul29([x]_e, [y]_f) = [x y]_(e + f - 261).  The
// state lives in R' form, [s]_261, from the input conversion to the output conversion, so every product of two state words and
// every product of a state word by an MDS entry [M]_261 is in R' form again.
//
// The table (PSD_RECORDS = 204 records of nine limbs, canonical, each limb below 2^29; built once per context from
// PoseidonWidth3::get()):
//   records 0 .. 2          the round constants of round 0 as [c]_261: added to the entering state, limb by limb;
//   records 3 r .. 3 r + 2  (r = 1 .. 64) the round constants of round r as [c]_522: they START the column sums of the MDS rows of
//                           round r - 1, so the reduction of those rows leaves M s + c -- the addition of the next round's constants
//                           costs no instruction and no carry pass (the same values modulo p as adding them afterwards);
//   records 195 + 3 i + j   the MDS entry M[i][j] as [M]_261.
// The walk over the rounds is wave-uniform, so a lane's reads of the table are wave-uniform too.
//
// Bounds.  Every operand of sqr29 / mul29 / psd_mds_row is normalised (limbs below 2^29) and below 3p:
//   * a converted input and the result of every product or MDS row are below 2p (mul29's result bound; an MDS row is
//     T = sum_j s_j M_ij + c < 3 (3p) p + p, far below 2^261 p = 169 p^2, and T / 2^261 + p < 2p);
//   * psd_enter adds the inputs of a continue row to the state the row before left (below 2p + 2p), REDUCES the sum below
//     (1 + 2^-20) p (reduce_lazy29_limbs) and only then adds the constants of round 0: below 2p + p, normalised by one carry pass;
//   * squares and products of such values are below 9 p^2 < 2^261 p.
// A column of psd_mds_row holds 27 state-by-entry products, one limb of the constant and the nine products of the reduction:
// 36 2^58 + 2^29 < 2^64.
// Per permutation: 4 + 4 full rounds of 3 S-boxes and 57 partial rounds of one, 81 S-boxes of two squarings and a product, and
// 65 x 3 MDS rows of three products each: 243 + 585 = 828 products under 243 + 195 = 438 reductions.
#pragma once
#include "ff29.hip.hpp"

namespace zk {

constexpr int PSD_FULL_HALF = 4, PSD_PARTIAL = 57, PSD_ROUNDS = 2 * PSD_FULL_HALF + PSD_PARTIAL;
constexpr int PSD_MDS_AT = 3 * PSD_ROUNDS;             // first MDS record
constexpr int PSD_RECORDS = PSD_MDS_AT + 9;            // 204 records, 7 344 B
constexpr int PSD_TAB_WORDS = PSD_RECORDS * 9;

// x^5: two squarings and one product, [x]_261 -> [x^5]_261
template <class P>
__host__ __device__ __forceinline__ F29<P> psd_pow5(const F29<P>& x) { return mul29(sqr29(sqr29(x)), x); }

// (s0 m0 + s1 m1 + s2 m2 + c) 2^-261 mod p under ONE reduction: m0, m1, m2, c wave-uniform records.  The column sums of mul29_c with
// three products and one limb of c in each; the columns are a compile-time recursion, not a loop, so that every dot product has a
// constant length when the function is first simplified (a loop over the columns is too large to be unrolled as written).
template <int K, class P>
__host__ __device__ __forceinline__ void psd_mds_col(uint64_t& acc, uint32_t (&m)[9], F29<P>& t, const F29<P>& s0, const F29<P>& s1, const F29<P>& s2, const F29<P>& m0, const F29<P>& m1,
                                                     const F29<P>& m2, const F29<P>& c) {
    constexpr int lo = K < 9 ? 0 : K - 8, hi = K < 9 ? K : 8, nm = K < 9 ? K : 17 - K;
    uint32_t k0[9], k1[9], k2[9], ks[9];
#pragma unroll
    for (int i = lo; i <= hi; ++i) { k0[i - lo] = m0.l[K - i]; k1[i - lo] = m1.l[K - i]; k2[i - lo] = m2.l[K - i]; ks[i - lo] = P::M(K - i); }
    if constexpr (K < 9) acc += c.l[K];
    acc = dotk(s0.l + lo, k0, hi - lo + 1, acc);
    acc = dotk(s1.l + lo, k1, hi - lo + 1, acc);
    acc = dotk(s2.l + lo, k2, hi - lo + 1, acc);
    acc = dotk(m + lo, ks, nm, acc);
    if constexpr (K < 9) {
        m[K] = ((uint32_t)acc * P::INV) & MASK29;
        acc += (uint64_t)m[K] * P::M(0);
    } else {
        t.l[K - 9] = (uint32_t)acc & MASK29;
    }
    acc >>= 29;
    if constexpr (K < 16) psd_mds_col<K + 1>(acc, m, t, s0, s1, s2, m0, m1, m2, c);
}
template <class P>
__host__ __device__ __forceinline__ F29<P> psd_mds_row(const F29<P>& s0, const F29<P>& s1, const F29<P>& s2, const F29<P>& m0, const F29<P>& m1, const F29<P>& m2, const F29<P>& c) {
    uint32_t m[9];
    F29<P> t;
    uint64_t acc = 0;
    psd_mds_col<0>(acc, m, t, s0, s1, s2, m0, m1, m2, c);
    t.l[8] = (uint32_t)acc;
    return t;
}

// The state a row permutes: what the row before left (zero for a head row; s[0] of a head row is the capacity word) plus the row's
// two inputs [in0]_261, [in1]_261, reduced, plus the constants of round 0.
template <class P>
__host__ __device__ __forceinline__ void psd_enter(F29<P> (&s)[3], const F29<P>& in0, const F29<P>& in1, const uint32_t* tab) {
    s[1] = add29(s[1], in0);
    s[2] = add29(s[2], in1);
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        normalize29(s[i]);
        s[i] = reduce_lazy29_limbs(s[i]);
#pragma unroll
        for (int j = 0; j < 9; ++j) s[i].l[j] += tab[9 * i + j];
        normalize29(s[i]);
    }
}

// PoseidonPerm<3, 8, 57>::permute on a state that psd_enter prepared; leaves [s']_261, normalised, below 2p
template <class P>
__host__ __device__ inline void psd_rounds(F29<P> (&s)[3], const uint32_t* tab) {
    const uint32_t* mds = tab + 9 * PSD_MDS_AT;
#pragma unroll 1
    for (int r = 0; r < PSD_ROUNDS; ++r) {
        s[0] = psd_pow5(s[0]);
        if (r < PSD_FULL_HALF || r >= PSD_FULL_HALF + PSD_PARTIAL) {
            s[1] = psd_pow5(s[1]);
            s[2] = psd_pow5(s[2]);
        }
        const bool last = r == PSD_ROUNDS - 1;
        const uint32_t keep = last ? 0u : ~0u;
        const uint32_t* cn = tab + 27 * (last ? r : r + 1);           // the constants of the NEXT round; none behind the last
        F29<P> M[9], c[3];
#pragma unroll
        for (int i = 0; i < 9; ++i)
#pragma unroll
            for (int j = 0; j < 9; ++j) M[i].l[j] = mds[9 * i + j];
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 9; ++j) c[i].l[j] = cn[9 * i + j] & keep;
        const F29<P> n0 = psd_mds_row(s[0], s[1], s[2], M[0], M[1], M[2], c[0]);
        const F29<P> n1 = psd_mds_row(s[0], s[1], s[2], M[3], M[4], M[5], c[1]);
        const F29<P> n2 = psd_mds_row(s[0], s[1], s[2], M[6], M[7], M[8], c[2]);
        s[0] = n0;
        s[1] = n1;
        s[2] = n2;
    }
}

// a cell as a 256-bit integer x and the plain constant K of its width (2^522 for an unsigned cell, 2^266 for a Montgomery Fr; the
// capacity's K carries cap_scale as well) -> [x]_261, normalised, below 2p.  K is wave-uniform.
template <class P>
__host__ __device__ __forceinline__ F29<P> psd_in(const Fp<typename P::P32>& x, const F29<P>& K) { return mul29_ub(unpack29<P>(x), K); }
// [x]_261 -> the canonical Montgomery image [x]_256: one product by the integer 2^256 mod p
template <class P>
__host__ __device__ __forceinline__ Fp<typename P::P32> psd_out(const F29<P>& x) {
    return pack29_lt2p(mul29_ub(x, unpack29<P>(Fp<typename P::P32>::one())));
}

// Cell i of a typed column as a 256-bit integer.  The width is wave-uniform.  1 .. 16: packed little-endian at stride = width,
// aligned to the width; 32: four 8-byte words; 31: the bytes ptr + 62 i .. + 30, BIG-endian, any alignment, byte loads only --
// nothing outside the cell is read in any case.
__host__ __device__ __forceinline__ Fr psd_load(const uint8_t* __restrict__ p, uint32_t width, uint64_t i) {
    Fr v = Fr::zero();
    switch (width) {
        case 1: v.l[0] = p[i]; break;
        case 2: v.l[0] = reinterpret_cast<const uint16_t*>(p)[i]; break;
        case 4: v.l[0] = reinterpret_cast<const uint32_t*>(p)[i]; break;
        case 8: { const uint2 w = reinterpret_cast<const uint2*>(p)[i]; v.l[0] = w.x; v.l[1] = w.y; break; }
        case 16: { const uint4 w = reinterpret_cast<const uint4*>(p)[i]; v.l[0] = w.x; v.l[1] = w.y; v.l[2] = w.z; v.l[3] = w.w; break; }
        case 32: {
            const uint2* q = reinterpret_cast<const uint2*>(p) + 4 * i;
#pragma unroll
            for (int j = 0; j < 4; ++j) { const uint2 w = q[j]; v.l[2 * j] = w.x; v.l[2 * j + 1] = w.y; }
            break;
        }
        default: {                      // 31
            const uint8_t* q = p + 62 * i;
#pragma unroll
            for (int k = 0; k < 31; ++k) v.l[k >> 2] |= (uint32_t)q[30 - k] << (8 * (k & 3));
            break;
        }
    }
    return v;
}

}  // namespace zk

// Unsaturated-limb BN254 field arithmetic for the ALU-bound inner loops (NTT butterflies, EC
// additions): 9 limbs x 29 bits, Montgomery radix R' = 2^261.
//
// Why (measured on MI355X, tools/ubench.hip): v_mad_u64_u32 issues at ~30 G lane-op/s x 1000 --
// the same rate as v_add_co/v_addc (carry-producing adds are half rate) -- so with saturated
// 32-bit limbs every 32x32 product needs a carry fix-up that costs as much as the multiply.
// With 29-bit limbs a 64-bit column accumulator absorbs all 18 products of a column without any
// carry handling: 162 pure v_mad_u64_u32 per Montgomery product and plain (carry-less) v_add_u32
// for field additions.
//
// Domain conventions:
//   * limbs are "normalised" when each is < 2^29 (top limb may carry the excess);
//   * values are kept lazily reduced (0 <= v < a few p); only pack() produces the canonical
//     representative;
//   * mul29(a, b) = a*b*2^-261 mod p, result normalised and < 2p provided a*b < 2^261 * p
//     (e.g. a < 2^258, b < 2^256).  Limb bounds: a[i] < 2^30, b[i] < 2^29 + small is safe
//     (column sum < 9*2^59 + 9*2^58 < 2^63).
//   * boundary data stays in halo2curves' R = 2^256 Montgomery form: mul29(X*2^256, W*2^261)
//     = X*W*2^256, so constants that multiply data (twiddles, SRS bases held by us) are stored
//     in R' form and data needs no conversion.
#pragma once
#include "ff.hip.hpp"

namespace zk {

constexpr uint32_t MASK29 = (1u << 29) - 1;

struct Fq29P {
    static constexpr uint32_t INV = 0x4866389u;
    __host__ __device__ static constexpr uint32_t M(int i) {
        constexpr uint32_t m[9] = {0x187cfd47u, 0x10460b6u, 0x1c72a34fu, 0x2d522d0u, 0x1585d978u, 0x2db40c0u, 0xa6e141u, 0xe5c2634u, 0x30644eu};
        return m[i];
    }
    using P32 = FqP;
};
struct Fr29P {
    static constexpr uint32_t INV = 0xfffffffu;
    __host__ __device__ static constexpr uint32_t M(int i) {
        constexpr uint32_t m[9] = {0x10000001u, 0x1f0fac9fu, 0xe5c2450u, 0x7d090f3u, 0x1585d283u, 0x2db40c0u, 0xa6e141u, 0xe5c2634u, 0x30644eu};
        return m[i];
    }
    using P32 = FrP;
};

template <class P>
struct F29 {
    uint32_t l[9];
};

// 8 x 32 -> 9 x 29 (any 256-bit value)
template <class P>
__host__ __device__ __forceinline__ F29<P> unpack29(const Fp<typename P::P32>& a) {
    F29<P> r;
#pragma unroll
    for (int i = 0; i < 9; ++i) {
        const int bit = 29 * i, w = bit >> 5, s = bit & 31;
        uint32_t v = a.l[w] >> s;
        if (s > 3 && w + 1 < 8) v |= a.l[w + 1] << (32 - s);
        r.l[i] = i == 8 ? v : (v & MASK29);
    }
    return r;
}
// carry-propagate so that limbs 0..7 < 2^29
template <class P>
__host__ __device__ __forceinline__ void normalize29(F29<P>& a) {
#pragma unroll
    for (int i = 0; i < 8; ++i) { a.l[i + 1] += a.l[i] >> 29; a.l[i] &= MASK29; }
}
// normalised 9 x 29 (value < 2^256) -> 8 x 32, no modular reduction
template <class P>
__host__ __device__ __forceinline__ Fp<typename P::P32> pack29_raw(const F29<P>& a) {
    Fp<typename P::P32> r;
#pragma unroll
    for (int w = 0; w < 8; ++w) {
        const int bit = 32 * w, i = bit / 29, s = bit - 29 * i;   // word w starts inside limb i at offset s
        uint32_t v = a.l[i] >> s;
        v |= a.l[i + 1] << (29 - s);
        if (29 - s + 29 < 32 && i + 2 < 9) v |= a.l[i + 2] << (58 - s);
        r.l[w] = v;
    }
    return r;
}
// full reduction to the canonical representative of a normalised value < 4p
template <class P>
__host__ __device__ __forceinline__ Fp<typename P::P32> pack29(const F29<P>& a) {
    Fp<typename P::P32> r = pack29_raw(a);
    cond_sub<typename P::P32>(r.l);   // value < 4p: subtract 2p? -> two conditional subtractions of p
    cond_sub<typename P::P32>(r.l);
    cond_sub<typename P::P32>(r.l);
    return r;
}

template <class P>
__host__ __device__ __forceinline__ F29<P> add29(const F29<P>& a, const F29<P>& b) {
    F29<P> r;
#pragma unroll
    for (int i = 0; i < 9; ++i) r.l[i] = a.l[i] + b.l[i];
    return r;
}
// limb i of K*p in "balanced" form: normalised limbs n[i] of K*p with 2^29 borrowed from the next
// limb (c[i] = n[i] + 2^29 - [i > 0], c[8] = n[8] - 1), so c[i] >= 2^29 - 1 >= any normalised limb.
template <class P>
__host__ __device__ constexpr uint32_t kp_balanced(int K, int idx) {
    uint64_t carry = 0;
    uint32_t out = 0;
    for (int i = 0; i <= idx; ++i) {
        const uint64_t v = (uint64_t)K * P::M(i) + carry;
        out = i < 8 ? (uint32_t)(v & MASK29) : (uint32_t)v;
        carry = v >> 29;
    }
    if (idx < 8) out += 1u << 29;
    if (idx > 0) out -= 1u;
    return out;
}
// a - b + K*p, limb-wise non-negative for normalised b < K*p; result limbs < a.l[i] + 2^30.
// K*p must stay below the 2^261 capacity together with a (K <= 64 in practice).
template <int K, class P>
__host__ __device__ __forceinline__ F29<P> sub29k(const F29<P>& a, const F29<P>& b) {
    F29<P> r;
#pragma unroll
    for (int i = 0; i < 9; ++i) r.l[i] = a.l[i] + kp_balanced<P>(K, i) - b.l[i];
    return r;
}
// The same for a subtrahend whose limbs are plain sums of S normalised limbs (b.l[i] <= S * (2^29 - 1), b < K*p - S * 2^232):
// S borrows of 2^29 per limb instead of one.  Result limbs < a.l[i] + (S + 1) * 2^29.
template <int K, int S, class P>
__host__ __device__ __forceinline__ F29<P> sub29kw(const F29<P>& a, const F29<P>& b) {
    F29<P> r;
#pragma unroll
    for (int i = 0; i < 9; ++i) {
        uint32_t c = kp_balanced<P>(K, i);
        if (i < 8) c += (uint32_t)(S - 1) << 29;
        if (i > 0) c -= (uint32_t)(S - 1);
        r.l[i] = a.l[i] + c - b.l[i];
    }
    return r;
}
// canonical representative of a normalised value < 2p
template <class P>
__host__ __device__ __forceinline__ Fp<typename P::P32> pack29_lt2p(const F29<P>& a) {
    Fp<typename P::P32> r = pack29_raw(a);
    cond_sub<typename P::P32>(r.l);
    return r;
}

// Column sums of the products below: acc + sum_j x[j]*y[j] (dotv: both factors in registers) and acc + sum_j x[j]*k[j]
// (dotk: k[] compile-time constants, held in scalar registers).  Left to itself the compiler starts every column sum from
// zero (so that the multiplications do not wait for the carry out of the previous column) and joins the carry with a 64-bit
// add of its own: 16 instructions per product, bought for latency that four resident waves hide anyway.  ZK_MAD_CHAIN makes
// the multiply-adds opaque so that the sums run as written, carry first: 1 = one asm statement per multiply-add, 2 = one
// per column part (the hazard recogniser puts an s_nop behind every asm statement).  0 = plain C, the association is the
// compiler's; host compilation always takes this form.  Measured (tools/gpu_arith_ab.sh, one MI355X): mode 2 against mode 0
// k_msm_buckets 0.998 -> 0.983 ms, the weighted bucket sum chain 2.01 -> 1.77 ms, NTT 2^20 124 -> 120 us, evaluator 3.43 ->
// 3.34 ms; it also needs fewer registers (the evaluator 95 -> 77, the NTT passes lose their scratch spills).
#ifndef ZK_MAD_CHAIN
#define ZK_MAD_CHAIN 2
#endif
#if ZK_MAD_CHAIN && defined(__HIP_DEVICE_COMPILE__)
__device__ __forceinline__ uint64_t dotv_asm(const uint32_t* x, const uint32_t* y, int n, uint64_t acc) {
    switch (n) {
        case 1:
            asm("v_mad_u64_u32 %0, vcc, %1, %2, %0\n\t"
                : "+v"(acc) : "v"(x[0]), "v"(y[0]) : "vcc");
            break;
        case 2:
            asm("v_mad_u64_u32 %0, vcc, %1, %3, %0\n\t"
                "v_mad_u64_u32 %0, vcc, %2, %4, %0\n\t"
                : "+v"(acc) : "v"(x[0]), "v"(x[1]), "v"(y[0]), "v"(y[1]) : "vcc");
            break;
        case 3:
            asm("v_mad_u64_u32 %0, vcc, %1, %4, %0\n\t"
                "v_mad_u64_u32 %0, vcc, %2, %5, %0\n\t"
                "v_mad_u64_u32 %0, vcc, %3, %6, %0\n\t"
                : "+v"(acc) : "v"(x[0]), "v"(x[1]), "v"(x[2]), "v"(y[0]), "v"(y[1]), "v"(y[2]) : "vcc");
            break;
        case 4:
            asm("v_mad_u64_u32 %0, vcc, %1, %5, %0\n\t"
                "v_mad_u64_u32 %0, vcc, %2, %6, %0\n\t"
                "v_mad_u64_u32 %0, vcc, %3, %7, %0\n\t"
                "v_mad_u64_u32 %0, vcc, %4, %8, %0\n\t"
                : "+v"(acc) : "v"(x[0]), "v"(x[1]), "v"(x[2]), "v"(x[3]), "v"(y[0]), "v"(y[1]), "v"(y[2]), "v"(y[3]) : "vcc");
            break;
        case 5:
            asm("v_mad_u64_u32 %0, vcc, %1, %6, %0\n\t"
                "v_mad_u64_u32 %0, vcc, %2, %7, %0\n\t"
                "v_mad_u64_u32 %0, vcc, %3, %8, %0\n\t"
                "v_mad_u64_u32 %0, vcc, %4, %9, %0\n\t"
                "v_mad_u64_u32 %0, vcc, %5, %10, %0\n\t"
                : "+v"(acc) : "v"(x[0]), "v"(x[1]), "v"(x[2]), "v"(x[3]), "v"(x[4]), "v"(y[0]), "v"(y[1]), "v"(y[2]), "v"(y[3]), "v"(y[4]) : "vcc");
            break;
        case 6:
            asm("v_mad_u64_u32 %0, vcc, %1, %7, %0\n\t"
                "v_mad_u64_u32 %0, vcc, %2, %8, %0\n\t"
                "v_mad_u64_u32 %0, vcc, %3, %9, %0\n\t"
                "v_mad_u64_u32 %0, vcc, %4, %10, %0\n\t"
                "v_mad_u64_u32 %0, vcc, %5, %11, %0\n\t"
                "v_mad_u64_u32 %0, vcc, %6, %12, %0\n\t"
                : "+v"(acc) : "v"(x[0]), "v"(x[1]), "v"(x[2]), "v"(x[3]), "v"(x[4]), "v"(x[5]), "v"(y[0]), "v"(y[1]), "v"(y[2]), "v"(y[3]), "v"(y[4]), "v"(y[5]) : "vcc");
            break;
        case 7:
            asm("v_mad_u64_u32 %0, vcc, %1, %8, %0\n\t"
                "v_mad_u64_u32 %0, vcc, %2, %9, %0\n\t"
                "v_mad_u64_u32 %0, vcc, %3, %10, %0\n\t"
                "v_mad_u64_u32 %0, vcc, %4, %11, %0\n\t"
                "v_mad_u64_u32 %0, vcc, %5, %12, %0\n\t"
                "v_mad_u64_u32 %0, vcc, %6, %13, %0\n\t"
                "v_mad_u64_u32 %0, vcc, %7, %14, %0\n\t"
                : "+v"(acc) : "v"(x[0]), "v"(x[1]), "v"(x[2]), "v"(x[3]), "v"(x[4]), "v"(x[5]), "v"(x[6]), "v"(y[0]), "v"(y[1]), "v"(y[2]), "v"(y[3]), "v"(y[4]), "v"(y[5]), "v"(y[6]) : "vcc");
            break;
        case 8:
            asm("v_mad_u64_u32 %0, vcc, %1, %9, %0\n\t"
                "v_mad_u64_u32 %0, vcc, %2, %10, %0\n\t"
                "v_mad_u64_u32 %0, vcc, %3, %11, %0\n\t"
                "v_mad_u64_u32 %0, vcc, %4, %12, %0\n\t"
                "v_mad_u64_u32 %0, vcc, %5, %13, %0\n\t"
                "v_mad_u64_u32 %0, vcc, %6, %14, %0\n\t"
                "v_mad_u64_u32 %0, vcc, %7, %15, %0\n\t"
                "v_mad_u64_u32 %0, vcc, %8, %16, %0\n\t"
                : "+v"(acc) : "v"(x[0]), "v"(x[1]), "v"(x[2]), "v"(x[3]), "v"(x[4]), "v"(x[5]), "v"(x[6]), "v"(x[7]), "v"(y[0]), "v"(y[1]), "v"(y[2]), "v"(y[3]), "v"(y[4]), "v"(y[5]), "v"(y[6]), "v"(y[7]) : "vcc");
            break;
        case 9:
            asm("v_mad_u64_u32 %0, vcc, %1, %10, %0\n\t"
                "v_mad_u64_u32 %0, vcc, %2, %11, %0\n\t"
                "v_mad_u64_u32 %0, vcc, %3, %12, %0\n\t"
                "v_mad_u64_u32 %0, vcc, %4, %13, %0\n\t"
                "v_mad_u64_u32 %0, vcc, %5, %14, %0\n\t"
                "v_mad_u64_u32 %0, vcc, %6, %15, %0\n\t"
                "v_mad_u64_u32 %0, vcc, %7, %16, %0\n\t"
                "v_mad_u64_u32 %0, vcc, %8, %17, %0\n\t"
                "v_mad_u64_u32 %0, vcc, %9, %18, %0\n\t"
                : "+v"(acc) : "v"(x[0]), "v"(x[1]), "v"(x[2]), "v"(x[3]), "v"(x[4]), "v"(x[5]), "v"(x[6]), "v"(x[7]), "v"(x[8]), "v"(y[0]), "v"(y[1]), "v"(y[2]), "v"(y[3]), "v"(y[4]), "v"(y[5]), "v"(y[6]), "v"(y[7]), "v"(y[8]) : "vcc");
            break;
        default: break;
    }
    return acc;
}
__device__ __forceinline__ uint64_t dotk_asm(const uint32_t* x, const uint32_t* y, int n, uint64_t acc) {
    switch (n) {
        case 1:
            asm("v_mad_u64_u32 %0, vcc, %1, %2, %0\n\t"
                : "+v"(acc) : "v"(x[0]), "s"(y[0]) : "vcc");
            break;
        case 2:
            asm("v_mad_u64_u32 %0, vcc, %1, %3, %0\n\t"
                "v_mad_u64_u32 %0, vcc, %2, %4, %0\n\t"
                : "+v"(acc) : "v"(x[0]), "v"(x[1]), "s"(y[0]), "s"(y[1]) : "vcc");
            break;
        case 3:
            asm("v_mad_u64_u32 %0, vcc, %1, %4, %0\n\t"
                "v_mad_u64_u32 %0, vcc, %2, %5, %0\n\t"
                "v_mad_u64_u32 %0, vcc, %3, %6, %0\n\t"
                : "+v"(acc) : "v"(x[0]), "v"(x[1]), "v"(x[2]), "s"(y[0]), "s"(y[1]), "s"(y[2]) : "vcc");
            break;
        case 4:
            asm("v_mad_u64_u32 %0, vcc, %1, %5, %0\n\t"
                "v_mad_u64_u32 %0, vcc, %2, %6, %0\n\t"
                "v_mad_u64_u32 %0, vcc, %3, %7, %0\n\t"
                "v_mad_u64_u32 %0, vcc, %4, %8, %0\n\t"
                : "+v"(acc) : "v"(x[0]), "v"(x[1]), "v"(x[2]), "v"(x[3]), "s"(y[0]), "s"(y[1]), "s"(y[2]), "s"(y[3]) : "vcc");
            break;
        case 5:
            asm("v_mad_u64_u32 %0, vcc, %1, %6, %0\n\t"
                "v_mad_u64_u32 %0, vcc, %2, %7, %0\n\t"
                "v_mad_u64_u32 %0, vcc, %3, %8, %0\n\t"
                "v_mad_u64_u32 %0, vcc, %4, %9, %0\n\t"
                "v_mad_u64_u32 %0, vcc, %5, %10, %0\n\t"
                : "+v"(acc) : "v"(x[0]), "v"(x[1]), "v"(x[2]), "v"(x[3]), "v"(x[4]), "s"(y[0]), "s"(y[1]), "s"(y[2]), "s"(y[3]), "s"(y[4]) : "vcc");
            break;
        case 6:
            asm("v_mad_u64_u32 %0, vcc, %1, %7, %0\n\t"
                "v_mad_u64_u32 %0, vcc, %2, %8, %0\n\t"
                "v_mad_u64_u32 %0, vcc, %3, %9, %0\n\t"
                "v_mad_u64_u32 %0, vcc, %4, %10, %0\n\t"
                "v_mad_u64_u32 %0, vcc, %5, %11, %0\n\t"
                "v_mad_u64_u32 %0, vcc, %6, %12, %0\n\t"
                : "+v"(acc) : "v"(x[0]), "v"(x[1]), "v"(x[2]), "v"(x[3]), "v"(x[4]), "v"(x[5]), "s"(y[0]), "s"(y[1]), "s"(y[2]), "s"(y[3]), "s"(y[4]), "s"(y[5]) : "vcc");
            break;
        case 7:
            asm("v_mad_u64_u32 %0, vcc, %1, %8, %0\n\t"
                "v_mad_u64_u32 %0, vcc, %2, %9, %0\n\t"
                "v_mad_u64_u32 %0, vcc, %3, %10, %0\n\t"
                "v_mad_u64_u32 %0, vcc, %4, %11, %0\n\t"
                "v_mad_u64_u32 %0, vcc, %5, %12, %0\n\t"
                "v_mad_u64_u32 %0, vcc, %6, %13, %0\n\t"
                "v_mad_u64_u32 %0, vcc, %7, %14, %0\n\t"
                : "+v"(acc) : "v"(x[0]), "v"(x[1]), "v"(x[2]), "v"(x[3]), "v"(x[4]), "v"(x[5]), "v"(x[6]), "s"(y[0]), "s"(y[1]), "s"(y[2]), "s"(y[3]), "s"(y[4]), "s"(y[5]), "s"(y[6]) : "vcc");
            break;
        case 8:
            asm("v_mad_u64_u32 %0, vcc, %1, %9, %0\n\t"
                "v_mad_u64_u32 %0, vcc, %2, %10, %0\n\t"
                "v_mad_u64_u32 %0, vcc, %3, %11, %0\n\t"
                "v_mad_u64_u32 %0, vcc, %4, %12, %0\n\t"
                "v_mad_u64_u32 %0, vcc, %5, %13, %0\n\t"
                "v_mad_u64_u32 %0, vcc, %6, %14, %0\n\t"
                "v_mad_u64_u32 %0, vcc, %7, %15, %0\n\t"
                "v_mad_u64_u32 %0, vcc, %8, %16, %0\n\t"
                : "+v"(acc) : "v"(x[0]), "v"(x[1]), "v"(x[2]), "v"(x[3]), "v"(x[4]), "v"(x[5]), "v"(x[6]), "v"(x[7]), "s"(y[0]), "s"(y[1]), "s"(y[2]), "s"(y[3]), "s"(y[4]), "s"(y[5]), "s"(y[6]), "s"(y[7]) : "vcc");
            break;
        case 9:
            asm("v_mad_u64_u32 %0, vcc, %1, %10, %0\n\t"
                "v_mad_u64_u32 %0, vcc, %2, %11, %0\n\t"
                "v_mad_u64_u32 %0, vcc, %3, %12, %0\n\t"
                "v_mad_u64_u32 %0, vcc, %4, %13, %0\n\t"
                "v_mad_u64_u32 %0, vcc, %5, %14, %0\n\t"
                "v_mad_u64_u32 %0, vcc, %6, %15, %0\n\t"
                "v_mad_u64_u32 %0, vcc, %7, %16, %0\n\t"
                "v_mad_u64_u32 %0, vcc, %8, %17, %0\n\t"
                "v_mad_u64_u32 %0, vcc, %9, %18, %0\n\t"
                : "+v"(acc) : "v"(x[0]), "v"(x[1]), "v"(x[2]), "v"(x[3]), "v"(x[4]), "v"(x[5]), "v"(x[6]), "v"(x[7]), "v"(x[8]), "s"(y[0]), "s"(y[1]), "s"(y[2]), "s"(y[3]), "s"(y[4]), "s"(y[5]), "s"(y[6]), "s"(y[7]), "s"(y[8]) : "vcc");
            break;
        default: break;
    }
    return acc;
}
#endif
__host__ __device__ __forceinline__ uint64_t dotv(const uint32_t* x, const uint32_t* y, int n, uint64_t acc) {
#if ZK_MAD_CHAIN == 2 && defined(__HIP_DEVICE_COMPILE__)
    return dotv_asm(x, y, n, acc);
#elif ZK_MAD_CHAIN == 1 && defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
    for (int j = 0; j < n; ++j) acc = dotv_asm(x + j, y + j, 1, acc);
    return acc;
#else
#pragma unroll
    for (int j = 0; j < n; ++j) acc += (uint64_t)x[j] * y[j];
    return acc;
#endif
}
__host__ __device__ __forceinline__ uint64_t dotk(const uint32_t* x, const uint32_t* k, int n, uint64_t acc) {
#if ZK_MAD_CHAIN == 2 && defined(__HIP_DEVICE_COMPILE__)
    return dotk_asm(x, k, n, acc);
#elif ZK_MAD_CHAIN == 1 && defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
    for (int j = 0; j < n; ++j) acc = dotk_asm(x + j, k + j, 1, acc);
    return acc;
#else
#pragma unroll
    for (int j = 0; j < n; ++j) acc += (uint64_t)x[j] * k[j];
    return acc;
#endif
}

// Montgomery product, product-scanning (FIPS) form, 64-bit column accumulator, no carries.
template <class P>
__host__ __device__ __forceinline__ F29<P> mul29_c(const F29<P>& a, const F29<P>& b) {
    uint32_t m[9];
    F29<P> t;
    uint64_t acc = 0;
#pragma unroll
    for (int k = 0; k < 17; ++k) {
        // column k: a[i] * b[k - i] and m[i] * M[k - i] over lo <= i <= hi (the m[k] * M[0] term of k < 9 comes once m[k] is known)
        const int lo = k < 9 ? 0 : k - 8, hi = k < 9 ? k : 8, nm = k < 9 ? k : 17 - k;
        uint32_t ys[9], ks[9];
#pragma unroll
        for (int i = lo; i <= hi; ++i) { ys[i - lo] = b.l[k - i]; ks[i - lo] = P::M(k - i); }
        acc = dotv(a.l + lo, ys, hi - lo + 1, acc);
        acc = dotk(m + lo, ks, nm, acc);
        if (k < 9) {
            m[k] = ((uint32_t)acc * P::INV) & MASK29;
            acc += (uint64_t)m[k] * P::M(0);
        } else {
            t.l[k - 9] = (uint32_t)acc & MASK29;
        }
        acc >>= 29;
    }
    t.l[8] = (uint32_t)acc;
    return t;
}

// The same product with a wave-uniform second factor (a constant of a program, a challenge): its limbs stay in scalar
// registers and enter the multiply-adds as the scalar operand, like the modulus -- no vector copies of b.
template <class P>
__host__ __device__ __forceinline__ F29<P> mul29_ub_c(const F29<P>& a, const F29<P>& b) {
    uint32_t m[9];
    F29<P> t;
    uint64_t acc = 0;
#pragma unroll
    for (int k = 0; k < 17; ++k) {
        const int lo = k < 9 ? 0 : k - 8, hi = k < 9 ? k : 8, nm = k < 9 ? k : 17 - k;
        uint32_t ys[9], ks[9];
#pragma unroll
        for (int i = lo; i <= hi; ++i) { ys[i - lo] = b.l[k - i]; ks[i - lo] = P::M(k - i); }
        acc = dotk(a.l + lo, ys, hi - lo + 1, acc);
        acc = dotk(m + lo, ks, nm, acc);
        if (k < 9) {
            m[k] = ((uint32_t)acc * P::INV) & MASK29;
            acc += (uint64_t)m[k] * P::M(0);
        } else {
            t.l[k - 9] = (uint32_t)acc & MASK29;
        }
        acc >>= 29;
    }
    t.l[8] = (uint32_t)acc;
    return t;
}

// (a*b + c*d) * 2^-261 mod p in one pass: the second product joins the column sums of the first, one reduction serves both
// (243 v_mad_u64_u32 instead of 324 + the subtraction or addition that would have combined two reduced products).
// a, b, c normalised (limbs < 2^29), d with limbs < 2^30 (e.g. K*p - x taken limb-wise, see neg29k), a*b + c*d < 2^261 * p:
// a column holds at most 9*2^58 + 9*2^59 + 9*2^58 < 2^64.  Result normalised, < (a*b + c*d) / 2^261 + p.
template <class P>
__host__ __device__ __forceinline__ F29<P> mul2add29_c(const F29<P>& a, const F29<P>& b, const F29<P>& c, const F29<P>& d) {
    uint32_t m[9];
    F29<P> t;
    uint64_t acc = 0;
#pragma unroll
    for (int k = 0; k < 17; ++k) {
        const int lo = k < 9 ? 0 : k - 8, hi = k < 9 ? k : 8, nm = k < 9 ? k : 17 - k;
        uint32_t ys[9], ds[9], ks[9];
#pragma unroll
        for (int i = lo; i <= hi; ++i) { ys[i - lo] = b.l[k - i]; ds[i - lo] = d.l[k - i]; ks[i - lo] = P::M(k - i); }
        acc = dotv(a.l + lo, ys, hi - lo + 1, acc);
        acc = dotv(c.l + lo, ds, hi - lo + 1, acc);
        acc = dotk(m + lo, ks, nm, acc);
        if (k < 9) {
            m[k] = ((uint32_t)acc * P::INV) & MASK29;
            acc += (uint64_t)m[k] * P::M(0);
        } else {
            t.l[k - 9] = (uint32_t)acc & MASK29;
        }
        acc >>= 29;
    }
    t.l[8] = (uint32_t)acc;
    return t;
}
// (a*b + c*d + e*f) * 2^-261 mod p in one pass: three products in the same column sums, one reduction (the evaluator's Horner step over a
// sum of two column products, csrc/quotient.hip K_MAC2_COL).  b, d, f normalised; limbs of a, c, e below L_a 2^29, L_c 2^29, L_e 2^29 with
// L_a + L_c + L_e <= 6: a column holds below 9 (L_a + L_c + L_e + 1) 2^58 + 2^35 < 2^64.  a*b + c*d + e*f < 2^261 p.  Result normalised, below 2p.
template <class P>
__host__ __device__ __forceinline__ F29<P> mul3add29_c(const F29<P>& a, const F29<P>& b, const F29<P>& c, const F29<P>& d, const F29<P>& e, const F29<P>& f) {
    uint32_t m[9];
    F29<P> t;
    uint64_t acc = 0;
#pragma unroll
    for (int k = 0; k < 17; ++k) {
        const int lo = k < 9 ? 0 : k - 8, hi = k < 9 ? k : 8, nm = k < 9 ? k : 17 - k;
        uint32_t ys[9], ds[9], fs[9], ks[9];
#pragma unroll
        for (int i = lo; i <= hi; ++i) { ys[i - lo] = b.l[k - i]; ds[i - lo] = d.l[k - i]; fs[i - lo] = f.l[k - i]; ks[i - lo] = P::M(k - i); }
        acc = dotv(a.l + lo, ys, hi - lo + 1, acc);
        acc = dotv(c.l + lo, ds, hi - lo + 1, acc);
        acc = dotv(e.l + lo, fs, hi - lo + 1, acc);
        acc = dotk(m + lo, ks, nm, acc);
        if (k < 9) {
            m[k] = ((uint32_t)acc * P::INV) & MASK29;
            acc += (uint64_t)m[k] * P::M(0);
        } else {
            t.l[k - 9] = (uint32_t)acc & MASK29;
        }
        acc >>= 29;
    }
    t.l[8] = (uint32_t)acc;
    return t;
}
// K*p - b taken limb by limb (b normalised, top limb of b below the top limb of K*p, i.e. b < K*p - 2^232): the value is
// K*p - b, limbs are non-negative and below 2^30, not normalised -- what mul2add29 takes as its last operand.
template <int K, class P>
__host__ __device__ __forceinline__ F29<P> neg29k(const F29<P>& b) {
    F29<P> r;
#pragma unroll
    for (int i = 0; i < 9; ++i) r.l[i] = kp_balanced<P>(K, i) - b.l[i];
    return r;
}

// canonical representative of a normalised lazy value < 64 m (sums of a few dozen reduced terms): quotient estimate from the bits
// above 2^232 -- t = x >> 232 is the top limb, q = floor(t C / 2^52) with C = floor(2^92 / ((m >> 192) + 1)) <= 2^284 / m (31 bits; both
// BN254 moduli share their top 128 bits) -- never exceeds x / m and misses it by less than 1 + 2^-20, so x - q m lies in
// [0, (1 + 2^-20) m): one multiple of m subtracted with signed carries, then ONE conditional subtraction (round 5; the estimate from
// six bits that this replaces missed by up to 2 and paid three conditional subtractions -- 50 instructions per output of the NTT's
// last pass).  ~half the work of multiplying by one just to reduce.
template <class P>
__host__ __device__ __forceinline__ F29<P> reduce_lazy29_limbs(const F29<P>& x) {       // the step before the conditional subtraction: normalised, < (1 + 2^-20) m
    constexpr uint64_t mhi = ((uint64_t)P::P32::M(7) << 32) | P::P32::M(6);
    constexpr uint32_t C = (uint32_t)((((unsigned __int128)1) << 92) / ((unsigned __int128)mhi + 1));
    const uint32_t q = (uint32_t)(((uint64_t)x.l[8] * C) >> 52);
    F29<P> r;
    int64_t c = 0;
#pragma unroll
    for (int i = 0; i < 9; ++i) {
        const int64_t s_ = (int64_t)x.l[i] - (int64_t)((uint64_t)q * P::M(i)) + c;
        r.l[i] = i < 8 ? (uint32_t)(s_ & MASK29) : (uint32_t)s_;
        c = s_ >> 29;
    }
    return r;
}
template <class P>
__host__ __device__ __forceinline__ Fp<typename P::P32> reduce_lazy29(const F29<P>& x) { return pack29_lt2p(reduce_lazy29_limbs(x)); }

// ---- coset records: a field element as the nine limbs the 9 x 29 products compute on ----------------------------------------
// The quotient evaluator reads every coset operand ~70 times per row; kept as packed 8 x 32 words each read pays 16-17 vector
// instructions to get the limbs back.  A coset buffer of n rows is therefore written ONCE as records (split layout, 36 n bytes):
//   bytes [0, 32 n):      row i = limbs 0 .. 7 of the canonical value (each below 2^29), 32-byte aligned like a packed element
//   bytes [32 n, 36 n):   the plane of top limbs, one u32 per row
// so a row is two 16-byte accesses at the address a packed element would have, plus one 4-byte access in the plane.
// ZK_REC29_AOS=1 (A/B builds: make VARIANT=aos EXTRA=-DZK_REC29_AOS=1) lays the same 36 n bytes out as an array of 36-byte rows,
// limbs 0 .. 8 in order: two 16-byte accesses and a 4-byte one at 4-byte alignment.  profiles/r19_coset_records.md has both measured.
#ifndef ZK_REC29_AOS
#define ZK_REC29_AOS 0
#endif
constexpr size_t REC29_BYTES = 36;
// canonical limbs of a normalised value < 2p
template <class P>
__host__ __device__ __forceinline__ F29<P> canon29_lt2p(const F29<P>& a) {
    F29<P> d;
    int32_t c = 0;
#pragma unroll
    for (int i = 0; i < 9; ++i) {
        const int32_t s_ = (int32_t)a.l[i] - (int32_t)P::M(i) + c;
        d.l[i] = i < 8 ? ((uint32_t)s_ & MASK29) : (uint32_t)s_;
        c = s_ >> 29;
    }
    const bool neg_ = (int32_t)d.l[8] < 0;
    F29<P> r;
#pragma unroll
    for (int i = 0; i < 9; ++i) r.l[i] = neg_ ? a.l[i] : d.l[i];
    return r;
}
#if defined(__HIPCC__)
// row `idx` of the record buffer `base` of n rows <- v (canonical limbs)
template <class P>
__device__ __forceinline__ void rec29_store(Fp<typename P::P32>* base, uint64_t n, uint64_t idx, const F29<P>& v) {
#if ZK_REC29_AOS
    typedef uint32_t U4A __attribute__((ext_vector_type(4), aligned(4)));
    char* p = reinterpret_cast<char*>(base) + idx * REC29_BYTES;
    *reinterpret_cast<U4A*>(p) = U4A{v.l[0], v.l[1], v.l[2], v.l[3]};
    *reinterpret_cast<U4A*>(p + 16) = U4A{v.l[4], v.l[5], v.l[6], v.l[7]};
    *reinterpret_cast<uint32_t*>(p + 32) = v.l[8];
#else
    uint4* q = reinterpret_cast<uint4*>(base + idx);
    q[0] = make_uint4(v.l[0], v.l[1], v.l[2], v.l[3]);
    q[1] = make_uint4(v.l[4], v.l[5], v.l[6], v.l[7]);
    reinterpret_cast<uint32_t*>(base + n)[idx] = v.l[8];
#endif
}
#endif

// Montgomery square: the cross products a_i a_j (i < j) are taken once against the doubled limb,
// 45 products instead of 81 in the operand part (the reduction part is unchanged): 126 vs 162.
// Same operand and result bounds as mul29(a, a).
template <class P>
__host__ __device__ __forceinline__ F29<P> sqr29_c(const F29<P>& a) {
    uint32_t m[9], a2[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) a2[i] = a.l[i] << 1;
    F29<P> t;
    uint64_t acc = 0;
#pragma unroll
    for (int k = 0; k < 17; ++k) {
        const int lo = k < 9 ? 0 : k - 8, hi = k < 9 ? k : 8, nm = k < 9 ? k : 17 - k;
        // cross terms lo <= i < k - i, then the square of the middle limb of an even column
        uint32_t xs[9], ys[9], ks[9];
        int n = 0;
#pragma unroll
        for (int i = lo; 2 * i < k; ++i) { xs[n] = a2[i]; ys[n] = a.l[k - i]; ++n; }
        if (!(k & 1)) { xs[n] = a.l[k / 2]; ys[n] = a.l[k / 2]; ++n; }
#pragma unroll
        for (int i = lo; i <= hi; ++i) ks[i - lo] = P::M(k - i);
        acc = dotv(xs, ys, n, acc);
        acc = dotk(m + lo, ks, nm, acc);
        if (k < 9) {
            m[k] = ((uint32_t)acc * P::INV) & MASK29;
            acc += (uint64_t)m[k] * P::M(0);
        } else {
            t.l[k - 9] = (uint32_t)acc & MASK29;
        }
        acc >>= 29;
    }
    t.l[8] = (uint32_t)acc;
    return t;
}


// The products as the rest of the library calls them.  On the device (ZK_MUL_ASM, default 1) each is ONE asm statement generated by
// tools/gen_mul29_asm.py (csrc/mul29_asm.hip.hpp) -- the same column sums in the same order as the C forms above, which stay the
// definition (host compilation, tests/test_host_arith.py) and what the device forms are compared with on the GPU (tools/ubench.hip:
// 4 M operand sets at the documented bounds, bit-identical).  With one statement per column part (ZK_MAD_CHAIN = 2, the C forms) a
// product carries its 162 multiply-adds in ~260 instructions; written out whole it is 162 + 9 v_mul_lo + 26 v_and + 17 v_lshrrev_b64 + 1.
// The bare product chain does not gain from that (179 vs 176 G/s: its other instructions hide behind the multiply-adds), the kernels
// do: NTT class of the headline proof 718 -> 700 ms, proof 1.033 -> 1.014 s on one box (alternating A/B, profiles/r05_experiments.md).
// `make VARIANT=c EXTRA=-DZK_MUL_ASM=0` builds the C forms for A/B runs.
#ifndef ZK_MUL_ASM
#define ZK_MUL_ASM 1
#endif
#if ZK_MUL_ASM && defined(__HIP_DEVICE_COMPILE__)
#include "mul29_asm.hip.hpp"
#define ZK_MUL29_DISPATCH(NAME, ...) return NAME##_asm<P>(__VA_ARGS__)
#else
#define ZK_MUL29_DISPATCH(NAME, ...) return NAME##_c<P>(__VA_ARGS__)
#endif
template <class P>
__host__ __device__ __forceinline__ F29<P> mul29(const F29<P>& a, const F29<P>& b) { ZK_MUL29_DISPATCH(mul29, a, b); }
template <class P>
__host__ __device__ __forceinline__ F29<P> mul29_ub(const F29<P>& a, const F29<P>& b) { ZK_MUL29_DISPATCH(mul29_ub, a, b); }
template <class P>
__host__ __device__ __forceinline__ F29<P> mul2add29(const F29<P>& a, const F29<P>& b, const F29<P>& c, const F29<P>& d) { ZK_MUL29_DISPATCH(mul2add29, a, b, c, d); }
template <class P>
__host__ __device__ __forceinline__ F29<P> sqr29(const F29<P>& a) { ZK_MUL29_DISPATCH(sqr29, a); }
#undef ZK_MUL29_DISPATCH
// In-place forms (round 6; the evaluator's interpreter keeps its top of stack in fixed registers): on the device the result is
// written over the named factor's registers by the asm statement itself -- no copy, no phi at the join of an interpreter's switch.
//   mul29_ipa(x, y): x <- mul29(x, y)      mul29_ipb(x, y): x <- mul29(y, x)      mul29_ub_ipa(x, y): x <- mul29_ub(x, y)
template <class P>
__host__ __device__ __forceinline__ void mul29_ipa(F29<P>& x, const F29<P>& y) {
#if ZK_MUL_ASM && defined(__HIP_DEVICE_COMPILE__)
    mul29_ipa_asm<P>(x, y);
#else
    x = mul29_c<P>(x, y);
#endif
}
template <class P>
__host__ __device__ __forceinline__ void mul29_ipb(F29<P>& x, const F29<P>& y) {
#if ZK_MUL_ASM && defined(__HIP_DEVICE_COMPILE__)
    mul29_ipb_asm<P>(x, y);
#else
    x = mul29_c<P>(y, x);
#endif
}
template <class P>
__host__ __device__ __forceinline__ void mul29_ub_ipa(F29<P>& x, const F29<P>& y) {
#if ZK_MUL_ASM && defined(__HIP_DEVICE_COMPILE__)
    mul29_ub_ipa_asm<P>(x, y);
#else
    x = mul29_ub_c<P>(x, y);
#endif
}
// x <- mul2add29(x, y, s, c) = (x y + s c) / 2^261 mod p, c wave-uniform (scalar registers): the evaluator's fused Horner step t0 B + S y^gap.
// Operand bounds as the caller keeps them (csrc/quotient_lower.hpp, lower_bounds): y, c normalised, limbs of x below L_x 2^29 and of s below
// L_s 2^29 with L_x + L_s <= 6 (a column then holds below 9 (L_x + L_s + 1) 2^58 + 2^35 < 2^64), x y + s c < 2^261 p.
template <class P>
__host__ __device__ __forceinline__ void mul2add29_ub_ipa(F29<P>& x, const F29<P>& y, const F29<P>& s, const F29<P>& c) {
#if ZK_MUL_ASM && defined(__HIP_DEVICE_COMPILE__)
    mul2add29_ub_ipa_asm<P>(x, y, s, c);
#else
    x = mul2add29_c<P>(x, y, s, c);
#endif
}
// x <- mul2add29(y, x, s, c): x is the SECOND factor of the first product (normalised; a stack product's top entry, shifted), y its first
// (limbs below L_y 2^29, L_y + L_s <= 6): the Horner step over a product of two computed values, K_MAC_STK.
template <class P>
__host__ __device__ __forceinline__ void mul2add29_ub_ipb(F29<P>& x, const F29<P>& y, const F29<P>& s, const F29<P>& c) {
#if ZK_MUL_ASM && defined(__HIP_DEVICE_COMPILE__)
    mul2add29_ub_ipb_asm<P>(x, y, s, c);
#else
    x = mul2add29_c<P>(y, x, s, c);
#endif
}
// x <- mul3add29(x, y, a, b, s, c) = (x y + a b + s c) / 2^261 mod p, c wave-uniform: K_MAC2_COL's  t0 * 32 m2 + X * 32 m1 + S y^gap.
// y, b, c normalised; limbs of x, a, s below L 2^29 each with L_x + L_a + L_s <= 6 (mul3add29_c).
template <class P>
__host__ __device__ __forceinline__ void mul3add29_ub_ipa(F29<P>& x, const F29<P>& y, const F29<P>& a, const F29<P>& b, const F29<P>& s, const F29<P>& c) {
#if ZK_MUL_ASM && defined(__HIP_DEVICE_COMPILE__)
    mul3add29_ub_ipa_asm<P>(x, y, a, b, s, c);
#else
    x = mul3add29_c<P>(x, y, a, b, s, c);
#endif
}

// a^(m-2) for a canonical 8 x 32 element in R = 2^256 Montgomery form; result in the same form.
// The 254-step exponentiation runs on 29-bit limbs (R' domain): its dependent chain is what a
// batch inversion waits for, and sqr29 / mul29 make it about half as long as the 32-bit CIOS one.
template <class P29>
__host__ __device__ inline Fp<typename P29::P32> inv_via29(const Fp<typename P29::P32>& a) {
    using F = Fp<typename P29::P32>;
    F t = a, one_rp = F::one();
#pragma unroll
    for (int i = 0; i < 5; ++i) { t = dbl(t); one_rp = dbl(one_rp); }     // x 32: R -> R'
    F29<P29> b = unpack29<P29>(t), r = unpack29<P29>(one_rp);
#pragma unroll 1
    for (int i = 0; i < 254; ++i) {
        const uint32_t limb = P29::P32::M(i >> 5) - (i < 32 ? 2u : 0u);     // bits of m - 2 (low limb >= 2: no borrow)
        if ((limb >> (i & 31)) & 1) r = mul29(r, b);
        b = sqr29(b);
    }
    return pack29_lt2p(mul29(r, unpack29<P29>(F::one())));                 // x 2^256 / 2^261: R' -> R
}

// ---- sum of short products under ONE reduction: T = sum_j x_j K_j, then T 2^-261 mod p (the row RLC of csrc/typed_rows.hip) ---------
// x_j is an integer of L_j <= 9 limbs and K_j a plain normalised constant below p; both have limbs below 2^29, so every product
// is below 2^58.  The sum is kept as 18 integer column sums c[k] of weight 2^(29 k) (x_i K_j goes to column i + j <= 16, column 17
// only ever takes carries), in 64-bit words, and nothing is reduced until rlc29_reduce.  Plain C on the host and on the device
// (a term is L_j x 9 multiply-adds whose second factor sits in scalar registers when K_j is wave-uniform); two bounds hold it up:
//   (1) columns.  The reduction adds to a column its nine products m_i M_(k-i) and a carry below 2^36, so a column may hold at most
//       RLC29_MAX_LOAD = 54 products when it starts: (54 + 9) 2^58 + 2^36 < 2^64.  `load` counts, for the fullest column, the
//       products taken since the last carry pass (a term of L limbs adds at most L to any column); rlc29_mac runs rlc29_carry
//       BEFORE a term that would pass the limit.  A carry pass leaves every column below 2^29 (counted as one product) and moves
//       less than 2^35 into the next one.  Bytes (L = 1) get 53 terms between passes, 16-byte cells 10, full elements 5.
//   (2) the sum.  rlc29_reduce needs T < 2^261 p, like mul29; its result is then normalised and below 2p.  A narrow term (x below
//       2^128) is below 2^128 p, so their number does not matter; a full-size one (x < p) is below p^2 and 2^261 / p = 169.2 of
//       those fit in Fr (147.6 in Fq).  The caller counts them: csrc/typed_rows.hip puts at most RR_BATCH = 64 terms under one reduction.
// rlc29_room(t, need) makes room for `need` products ahead of a run of terms whose limb counts add up to `need`: the tests that
// rlc29_mac still makes for every term of the run then cannot fire.  `load` is a runtime value; where the run is unrolled with a
// constant `need`, the compiler's range propagation (load <= MAX - need after the call) can remove those tests and their copies
// of the carry pass (k_fr_row_rlc: 18.3 k -> 11.3 k lines of ISA), but nothing depends on that: the bound is kept by the tests.
constexpr uint32_t RLC29_MAX_LOAD = 54;
template <class P>
struct Rlc29 {
    uint64_t c[18];
    uint32_t load;
};
// T = the plain normalised value k (one product per column at most: the constant term, taken with the cell 1), or 0
template <class P>
__host__ __device__ __forceinline__ void rlc29_init(Rlc29<P>& t, const uint32_t* k) {
#pragma unroll
    for (int i = 0; i < 18; ++i) t.c[i] = i < 9 ? k[i] : 0;
    t.load = 1;
}
template <class P>
__host__ __device__ __forceinline__ void rlc29_carry(Rlc29<P>& t) {
#pragma unroll
    for (int i = 0; i < 17; ++i) { t.c[i + 1] += t.c[i] >> 29; t.c[i] &= MASK29; }
    t.load = 1;
}
template <class P>
__host__ __device__ __forceinline__ void rlc29_room(Rlc29<P>& t, uint32_t need) {       // need < RLC29_MAX_LOAD
    if (t.load > RLC29_MAX_LOAD - need) rlc29_carry(t);
}
// T += x K for x of L limbs and K of nine, all below 2^29
template <int L, class P>
__host__ __device__ __forceinline__ void rlc29_mac(Rlc29<P>& t, const uint32_t* x, const uint32_t* k) {
    static_assert(L >= 1 && L <= 9 && L + 1 <= RLC29_MAX_LOAD, "a term is one to nine limbs");
    rlc29_room(t, L);
    t.load += L;
#pragma unroll
    for (int i = 0; i < L; ++i)
#pragma unroll
        for (int j = 0; j < 9; ++j) t.c[i + j] += (uint64_t)x[i] * k[j];
}
// T 2^-261 mod p for T < 2^261 p: normalised, below 2p.  The column sums stand where mul29_c has its a[i] b[k - i] products.
template <class P>
__host__ __device__ __forceinline__ F29<P> rlc29_reduce(const Rlc29<P>& t) {
    uint32_t m[9];
    F29<P> r;
    uint64_t acc = 0;
#pragma unroll
    for (int k = 0; k < 17; ++k) {
        const int lo = k < 9 ? 0 : k - 8, nm = k < 9 ? k : 17 - k;
        uint32_t ks[9];
#pragma unroll
        for (int i = 0; i < nm; ++i) ks[i] = P::M(k - lo - i);
        acc += t.c[k];
        acc = dotk(m + lo, ks, nm, acc);
        if (k < 9) {
            m[k] = ((uint32_t)acc * P::INV) & MASK29;
            acc += (uint64_t)m[k] * P::M(0);
        } else {
            r.l[k - 9] = (uint32_t)acc & MASK29;
        }
        acc >>= 29;
    }
    r.l[8] = (uint32_t)(acc + t.c[17]);
    return r;
}

// ---- one row of a running RLC: z <- (z M + x K) 2^-261 mod p (the typed scan of csrc/vec.hip, ZK_OP_SCAN_RLC) ---------------------
// z is the state, normalised and below 2p (a Montgomery image: the integer Z 2^256), x the row's cell as an integer of L limbs, M and
// K the plain normalised constants of the row's kind: M = m 2^261 and K = w 2^517 (K = w 2^261 where x is itself a Montgomery image)
// give the image of m Z + w X.  Two terms under one reduction: T < 2p p + 2^128 p < 2^261 p (x < p instead of 2^128: T < 3 p^2), and
// the fullest column holds 1 + 9 + L <= 19 products, far below RLC29_MAX_LOAD -- rlc29_mac never runs a carry pass here.
template <int L, class P>
__host__ __device__ __forceinline__ F29<P> scan_rlc29_step(const F29<P>& z, const uint32_t* x, const uint32_t* M, const uint32_t* K) {
    Rlc29<P> t;
    const uint32_t zero[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    rlc29_init(t, zero);
    rlc29_mac<9>(t, z.l, M);
    rlc29_mac<L>(t, x, K);
    return rlc29_reduce(t);
}
// The same row as a map z -> A z + B composed onto the rows before it (A, B Montgomery images, normalised, below 2p; the identity
// is A = 2^256 mod p, B = 0): A <- A M 2^-261, B <- (B M + x K) 2^-261.  A chunk of rows folds into one map by calling this in scan
// order; applying that map to the entering state equals walking the rows with scan_rlc29_step.
template <int L, class P>
__host__ __device__ __forceinline__ void scan_rlc29_fold(F29<P>& A, F29<P>& B, const uint32_t* x, const uint32_t* M, const uint32_t* K) {
    Rlc29<P> t;
    const uint32_t zero[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    rlc29_init(t, zero);
    rlc29_mac<9>(t, A.l, M);
    A = rlc29_reduce(t);
    B = scan_rlc29_step<L>(B, x, M, K);
}

// ---- inverse-or-zero of a row sum: out = num * inv0(D), inv0(0) = 0 (the per-lane steps of k_fr_row_inv0, csrc/typed_rows.hip, ZK_OP_ROW_INV0) --
// Forms.  mul29 is Montgomery by R' = 2^261, the columns are R = 2^256.  Write [x]_e for the residue x 2^e; mul29([x]_e, [y]_f) =
// [x y]_(e + f - 261), so a factor in R' form ([y]_261) leaves the form of the other factor as it is.
//   * the denominator: the host hands the inverting launch its constants with a further 2^5 (w 2^522 narrow, w 2^266 for a 32-byte
//     column, c 2^522), so rlc29_reduce leaves [D]_261 directly -- k_batch_invert's five doublings per element are not paid;
//   * prefix products, the products over the wave and the back-substitution multiply R' forms only; the ONE inverse of a wave is put
//     into the form e that the numerator wants by the constant of inv29_rp (2^(e + 522) instead of 2^783), once per wave on lane
//     63, and every quotient [1/D]_e = iv * pre below inherits it:
//       no numerator            e = 256: the quotient IS the result, no product by one_r          (constant 2^778)
//       32-byte numerator [N]_256  e = 261: mul29([1/D]_261, [N]_256) = [N/D]_256, in one_r's place  (constant 2^783)
//       narrow numerator N = [N]_0  e = 517: mul29([1/D]_517, N) = [N/D]_256                         (constant 2^1039)
// Bounds.  Every mul29 operand here is normalised (limbs below 2^29) and below 2p: a result of rlc29_reduce / canon29_lt2p / mul29, a
// canonical constant, a canonical 32-byte numerator (below p) or a narrow integer (below 2^128); every product is below 4 p^2 <
// 2^261 p, as mul29 assumes, and its result is normalised and below 2p again.
// Zero.  rlc29_reduce is only below 2p: a denominator that cancels modulo p may arrive as the integer p, so the test is made on the
// canonical limbs (canon29_lt2p) -- an untested p would enter the wave's product as a zero factor.  `live` has bit s set for a row
// that takes part: inside n and non-zero.  The others enter the products as one and come out as 0.
enum { INV0_NUM_ONE = 0, INV0_NUM_UINT = 1, INV0_NUM_FR = 2 };
// the reduced sum as canonical limbs ([D]_261 with the inverting launch's constants); false: D = 0 mod p
template <class P>
__host__ __device__ __forceinline__ bool inv0_29_den(const Rlc29<P>& t, F29<P>& d) {
    d = canon29_lt2p(rlc29_reduce(t));
    uint32_t any = 0;
#pragma unroll
    for (int i = 0; i < 9; ++i) any |= d.l[i];
    return any != 0;
}
// pre[k] = the product of the live d[j], j < k, starting from one_rp = [1]_261; returns the product of all of them
template <int K, class P>
__host__ __device__ __forceinline__ F29<P> inv0_29_prefix(const F29<P> (&d)[K], uint32_t live, const F29<P>& one_rp, F29<P> (&pre)[K]) {
    F29<P> acc = one_rp;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        pre[k] = acc;
        if (live >> k & 1u) acc = mul29(acc, d[k]);
    }
    return acc;
}
// iv = [1 / (the product inv0_29_prefix returned)]_e  ->  q[k] = [1 / D_k]_e for every live k (the others are left alone)
template <int K, class P>
__host__ __device__ __forceinline__ void inv0_29_back(F29<P> iv, const F29<P> (&d)[K], const F29<P> (&pre)[K], uint32_t live, F29<P> (&q)[K]) {
#pragma unroll
    for (int k = K; k-- > 0;) {
        if (!(live >> k & 1u)) continue;
        q[k] = mul29(iv, pre[k]);
        if (k) iv = mul29(iv, d[k]);
    }
}
// the row's result from its quotient (in the form of its NUM, above) and its numerator: canonical, R = 2^256 form
template <int NUM, class P>
__host__ __device__ __forceinline__ Fp<typename P::P32> inv0_29_out(const F29<P>& q, const F29<P>& num) {
    if constexpr (NUM == INV0_NUM_ONE) return pack29_lt2p(q);
    else return pack29_lt2p(mul29(q, num));
}

using Fq29 = F29<Fq29P>;
using Fr29 = F29<Fr29P>;

// 1 / b for b in R' = 2^261 form, times c 2^-522: the residue as a plain integer X = B 2^261 has X^-1 = B^-1 2^-261 (binary extended
// Euclid, ff.hip.hpp), and one product by the plain constant c brings it to B^-1 c 2^-522 -- c783 = 2^783 gives R' form again.  A
// lone lane runs this while its wave waits: the Fermat ladder (381 products, ~95 000 instructions) took 250 us there, this takes a
// quarter of the instructions.
__host__ __device__ inline Fr29 inv29_rp(const Fr29& b, const Fr29& c783) {
    const Fr x = pack29_lt2p(b);
    Fr y;
    inv_xgcd<FrP>(y.l, x.l);
    return mul29(unpack29<Fr29P>(y), c783);
}

// a limb record from another lane of the wave
__device__ __forceinline__ Fr29 shfl_up29(const Fr29& v, int off) {
    Fr29 r;
#pragma unroll
    for (int k = 0; k < 9; ++k) r.l[k] = __shfl_up(v.l[k], off);
    return r;
}
__device__ __forceinline__ Fr29 shfl_down29(const Fr29& v, int off) {
    Fr29 r;
#pragma unroll
    for (int k = 0; k < 9; ++k) r.l[k] = __shfl_down(v.l[k], off);
    return r;
}
__device__ __forceinline__ Fr29 shfl29(const Fr29& v, int src) {
    Fr29 r;
#pragma unroll
    for (int k = 0; k < 9; ++k) r.l[k] = __shfl(v.l[k], src);
    return r;
}

}  // namespace zk

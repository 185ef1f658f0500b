// The affine maps z -> A z + B of the scan ops and their block-level composition, shared by csrc/vec.hip (ZK_OP_SCAN_AFFINE,
// ZK_OP_SCAN_RLC) and csrc/copy_rows.hip (ZK_OP_COPY_RLC).  "First p, then q" is (q.A p.A, q.A p.B + q.B): associative, NOT
// commutative, so every combine names the earlier map first.  k_affine_b itself stays in vec.hip; affine_b_launch enqueues it.
#pragma once
#include "ctx.hpp"

namespace zk {

constexpr int SCAN_THREADS = 256;
constexpr int SCAN_PER = 8;

struct Aff { Fr A, B; };
__device__ __forceinline__ Aff aff_id() { return Aff{Fr::one(), Fr::zero()}; }
__device__ __forceinline__ Aff aff_then(const Aff& p, const Aff& q) { return Aff{q.A * p.A, q.A * p.B + q.B}; }   // first p, then q
__device__ __forceinline__ Fr aff_apply(const Aff& p, const Fr& z) { return p.A * z + p.B; }

// composite of the block's SCAN_THREADS maps in thread order (valid in thread 0): neighbours pair up, the earlier one first
__device__ __forceinline__ Aff aff_block_total(const Aff& v, Aff* sh) {
    const int t = threadIdx.x;
    sh[t] = v;
    __syncthreads();
    for (int m = SCAN_THREADS / 2; m > 0; m >>= 1) {
        Aff x;
        if (t < m) x = aff_then(sh[2 * t], sh[2 * t + 1]);
        __syncthreads();
        if (t < m) sh[t] = x;
        __syncthreads();
    }
    return sh[0];
}
// block_exclusive_scan over maps: returns the composite of the threads before this one; *total = the whole block's
__device__ __forceinline__ Aff aff_block_exclusive_scan(const Aff& v, Aff* sh, Aff* total) {
    const int t = threadIdx.x;
    sh[t] = v;
    __syncthreads();
    for (int off = 1; off < SCAN_THREADS; off <<= 1) {
        Aff x = sh[t];
        if (t >= off) x = aff_then(sh[t - off], x);
        __syncthreads();
        sh[t] = x;
        __syncthreads();
    }
    *total = sh[SCAN_THREADS - 1];
    Aff ex = t ? sh[t - 1] : aff_id();
    __syncthreads();
    return ex;
}

// entering[i] = the recurrence's value after the maps before map i (0 for map 0), from cnt block maps: k_affine_b of vec.hip on the
// context's stream
void affine_b_launch(zk_ctx* ctx, const Aff* maps, Fr* entering, uint32_t cnt);

}  // namespace zk

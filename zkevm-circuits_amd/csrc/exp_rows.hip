// ZK_OP_EXP_ROWS of zk_field_vec_op: the rows of the exponentiation circuit and of the exponentiation table (exp_circuit.rs
// assign_exp_events, table.rs ExpTable::assignments, gadgets mul_add.rs MulAddChip::assign and range.rs UIntRangeCheckChip::assign) from
// one 64-byte (base, exponent) record per event on the device.  The row logic and the 256-bit integer arithmetic are
// csrc/exp_rows.hip.hpp, which the host compiles too.
//
//   k_exp_widths    w[e] = min(8 S_e, n), w[count] = 0; with d_rows_needed the sum of S over each block of 256 events
//   bc_scan         the exclusive scan of bytecode_rows.hip, saturating at n, in place -> start[0 .. count], start[count] = the rows in use
//   k_exp_total     (only with d_rows_needed) one workgroup adds the block sums: 8 sum S + 10, exact, one 8-byte store from one lane
//   k_exp_chain     the serial part and nothing else: one lane per event squares and multiplies from the exponent's top bit down and
//                   stores d_j at step slot start_e / 8 + j of the scratch, (n / 8 + 1) x 32 B, where step j or step j - 1 is live.
//                   Lanes of a wave differ in trip count (at most 510 multiplies); that is accepted
//   k_exp_rows      in row space: a workgroup takes EX_TILE = 1024 rows, lane l the step slot of rows 8 l .. 8 l + 7: one search of
//                   start per tile for its first and last row, one per lane inside that window, the closed forms of ex_event_step with
//                   d_j and d_(j + 1) from the slots, the 8- and 16-byte cells stored straight, the 1- and 2-byte columns packed in LDS
//                   and stored as aligned dwords with head and tail bytes; the padding steps and the zero rows too
// No atomics, no host wait; no byte outside d_events is read whatever the records hold, and only slots that k_exp_chain wrote are read.
#include "ctx.hpp"
#include "exp_rows.hip.hpp"
#include "op_check.hpp"

namespace zk {

static_assert(sizeof(zk_exp_event) == EX_EVENT_BYTES && offsetof(zk_exp_event, exponent) == 32, "zk_exp_event is 64 packed bytes");

struct alignas(16) ExCell16 { uint64_t lo, hi; };

struct ExArgs {
    const uint64_t* events;             // count records of eight words: base, then exponent
    const uint32_t* starts;             // count + 1 entries
    ExCell16* slots;                    // two per step slot: d_j
    uint32_t count, n;
    uint8_t* is_last;
    uint64_t* base_limb;
    ExCell16 *exponent, *out, *mul_cols, *parity_cols;
    uint8_t *mul_u16_64, *mul_u16_128, *parity_u16_64, *parity_u16_128;
};

// word 0 (base) or 1 (exponent) of event e
__device__ __forceinline__ ExWord ex_load_word(const ExArgs& g, uint32_t e, uint32_t which) {
    ExWord v;
#pragma unroll
    for (uint32_t k = 0; k < 4; ++k) v.w[k] = g.events[(uint64_t)e * EX_EVENT_WORDS + 4 * which + k];
    return v;
}
__device__ __forceinline__ ExWord ex_load_slot(const ExArgs& g, uint64_t slot) {
    const ExCell16 lo = g.slots[2 * slot], hi = g.slots[2 * slot + 1];
    return ExWord{{lo.lo, lo.hi, hi.lo, hi.hi}};
}

__global__ void __launch_bounds__(256) k_exp_widths(const ExArgs g, uint32_t* w, uint32_t* block_steps) {
    __shared__ uint32_t sh[256];
    const uint64_t e = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    const uint32_t steps = e < g.count ? ex_steps(ex_load_word(g, (uint32_t)e, 1)) : 0u;
    if (e <= g.count) w[e] = ex_rows_of(steps, g.n);
    if (!block_steps) return;
    sh[threadIdx.x] = steps;
    __syncthreads();
    for (uint32_t d = 128; d; d >>= 1) {
        if (threadIdx.x < d) sh[threadIdx.x] += sh[threadIdx.x + d];   // at most 256 x 510
        __syncthreads();
    }
    if (threadIdx.x == 0) block_steps[blockIdx.x] = sh[0];
}
__global__ void __launch_bounds__(256) k_exp_total(const uint32_t* block_steps, uint32_t blocks, uint64_t* rows_needed) {
    __shared__ uint64_t sh[256];
    uint64_t s = 0;
    for (uint32_t i = threadIdx.x; i < blocks; i += 256) s += block_steps[i];
    sh[threadIdx.x] = s;
    __syncthreads();
    for (uint32_t d = 128; d; d >>= 1) {
        if (threadIdx.x < d) sh[threadIdx.x] += sh[threadIdx.x + d];
        __syncthreads();
    }
    if (threadIdx.x == 0) *rows_needed = EX_STEP_ROWS * sh[0] + EX_UNUSABLE;
}

__global__ void __launch_bounds__(256) k_exp_chain(const ExArgs g) {
    const uint64_t e64 = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (e64 >= g.count) return;
    const uint32_t e = (uint32_t)e64;
    const uint64_t start = g.starts[e];
    if (!ex_kept(start, g.n)) return;                                   // not even d_0 has a slot
    const ExWord x = ex_load_word(g, e, 1);
    if (ex_lt2(x)) return;
    const ExWord base = ex_load_word(g, e, 0);
    ExChain c = ex_chain_begin(base, x);
#pragma unroll 1
    while (c.j) {
        ex_chain_next(c, base, x);
        const uint64_t o = start + (uint64_t)EX_STEP_ROWS * c.j;
        if (ex_kept(o, g.n)) {                                          // slot o / 8 <= (n - 10) / 8
            g.slots[2 * (o / EX_STEP_ROWS)] = ExCell16{c.acc.w[0], c.acc.w[1]};
            g.slots[2 * (o / EX_STEP_ROWS) + 1] = ExCell16{c.acc.w[2], c.acc.w[3]};
        }
    }
}

// `bytes` bytes of a 1- or 2-byte column from the tile's packed bytes in LDS (st: one word more than the tile holds), as k_cp_rows
// stores them: bytes up to the first address that is a multiple of 4, dwords, bytes again
__device__ __forceinline__ void ex_store_small(uint8_t* p, const uint32_t* st, uint32_t bytes) {
    const uint8_t* sb = (const uint8_t*)st;
    uint32_t head = (uint32_t)(-(uintptr_t)p & 3);
    head = head < bytes ? head : bytes;
    if (threadIdx.x < head) p[threadIdx.x] = sb[threadIdx.x];
    const uint32_t body = (bytes - head) >> 2;
    for (uint32_t i = threadIdx.x; i < body; i += EX_TILE_STEPS) {
        const uint32_t o = head + 4 * i, sh = (o & 3) * 8;
        const uint32_t lo = st[o >> 2], hi = st[(o >> 2) + 1];
        ((uint32_t*)(p + head))[i] = sh ? lo >> sh | hi << (32 - sh) : lo;
    }
    const uint32_t done = head + 4 * body;
    if (threadIdx.x < bytes - done) p[done + threadIdx.x] = sb[done + threadIdx.x];
}

constexpr uint32_t EX_STAGE_WORDS = EX_TILE * 2 / 4 + 1;                // a 2-byte plane of one tile and the word behind it

// the outputs of one chip for the lane's step slot at row o (o < n may fail: then nothing is stored straight, and zeros are staged)
template <bool U16>
__device__ __forceinline__ void ex_store_chip(const ExArgs& g, const ExMulAdd& m, ExCell16* cols, uint8_t* u16_64, uint8_t* u16_128, uint32_t (*stage)[EX_STAGE_WORDS], uint64_t o, uint32_t r0,
                                              uint32_t rows) {
    const uint64_t n = g.n;
    if (cols) {
#pragma unroll
        for (uint32_t c = 0; c < 4; ++c) {
#pragma unroll
            for (uint32_t r = 0; r < EX_STEP_ROWS; ++r) {
                const ExCell v = ex_muladd_cell(m, r, c);
                if (o + r < n) cols[c * n + o + r] = ExCell16{v.lo, v.hi};
            }
        }
    }
    if (!U16) return;
    if (u16_64) {                                                       // uniform: the barriers are met by every lane
#pragma unroll
        for (uint32_t c = 0; c < 4; ++c) {
#pragma unroll
            for (uint32_t k = 0; k < 4; ++k) stage[c][4 * threadIdx.x + k] = ex_u16_64(m, 2 * k, c) | ex_u16_64(m, 2 * k + 1, c) << 16;
        }
        __syncthreads();
        for (uint32_t c = 0; c < 4; ++c) ex_store_small(u16_64 + (c * n + r0) * 2, stage[c], rows * 2);
        __syncthreads();
    }
    if (u16_128) {
#pragma unroll
        for (uint32_t c = 0; c < 8; ++c) {
#pragma unroll
            for (uint32_t k = 0; k < 4; ++k) stage[c][4 * threadIdx.x + k] = ex_u16_128(m, 2 * k, c) | ex_u16_128(m, 2 * k + 1, c) << 16;
        }
        __syncthreads();
        for (uint32_t c = 0; c < 8; ++c) ex_store_small(u16_128 + (c * n + r0) * 2, stage[c], rows * 2);
        __syncthreads();
    }
}

// U16: a u16 plane is asked for
template <bool U16>
__global__ void __launch_bounds__(EX_TILE_STEPS) k_exp_rows(const ExArgs g) {
    __shared__ uint32_t stage[U16 ? 8 : 1][EX_STAGE_WORDS];
    const uint32_t r0 = blockIdx.x * EX_TILE;
    const uint32_t rows = g.n - r0 < EX_TILE ? g.n - r0 : EX_TILE;
    const uint64_t n = g.n, o = (uint64_t)r0 + EX_STEP_ROWS * threadIdx.x;
    if (threadIdx.x < (U16 ? 8 : 1)) stage[threadIdx.x][EX_STAGE_WORDS - 1] = 0;

    ExStep s = ex_zero_step();
    if (ex_live(o, n)) {
        const uint32_t lo = bc_find(g.starts, 0, g.count, r0);
        const uint32_t hi = bc_find(g.starts, lo, g.count, r0 + rows - 1);
        const uint32_t e = bc_find(g.starts, lo, hi, (uint32_t)o);
        if (e < g.count) {                                              // start_e <= o < start_(e + 1): both exact, o - start_e < 8 S_e
            const ExWord x = ex_load_word(g, e, 1);
            const uint32_t j = ((uint32_t)o - g.starts[e]) / EX_STEP_ROWS;
            const ExWord d = ex_load_slot(g, o / EX_STEP_ROWS);
            const ExWord next = j + 1u < ex_steps(x) ? ex_load_slot(g, o / EX_STEP_ROWS + 1) : ex_word(0);   // kept: o + 8 + 10 <= n
            s = ex_event_step(ex_load_word(g, e, 0), x, j, d, next);
        } else {
            s = ex_pad_step();
        }
    }

    // the table
#pragma unroll
    for (uint32_t r = 0; r < EX_STEP_ROWS; ++r) {
        if (o + r >= n) continue;
        const ExCell d = ex_lo_hi(s.d, r), x = ex_lo_hi(s.x, r);
        g.out[o + r] = ExCell16{d.lo, d.hi};
        if (g.exponent) g.exponent[o + r] = ExCell16{x.lo, x.hi};
        if (g.base_limb) g.base_limb[o + r] = ex_base_limb(s, r);
    }
    if (g.is_last) {
        stage[0][2 * threadIdx.x] = s.is_last;
        stage[0][2 * threadIdx.x + 1] = 0;
        __syncthreads();
        ex_store_small(g.is_last + r0, stage[0], rows);
        __syncthreads();
    }
    // the chips, one behind the other
    if (g.mul_cols || (U16 && (g.mul_u16_64 || g.mul_u16_128))) {
        const ExMulAdd m = ex_mul_chip(s);
        ex_store_chip<U16>(g, m, g.mul_cols, g.mul_u16_64, g.mul_u16_128, stage, o, r0, rows);
    }
    if (g.parity_cols || (U16 && (g.parity_u16_64 || g.parity_u16_128))) {
        const ExMulAdd m = ex_parity_chip(s);
        ex_store_chip<U16>(g, m, g.parity_cols, g.parity_u16_64, g.parity_u16_128, stage, o, r0, rows);
    }
}

// ---- host side --------------------------------------------------------------------------------------------------------------------------------
// Everything is validated before n is looked at and before the first launch.
int exp_rows_run(zk_ctx* ctx, const zk_exp_rows* desc, const void* h_b, void* d_out, uint64_t n) {
    if (desc->flags) return ctx->fail(ZK_ERR_INVALID_ARG, "exp rows: flags 0x%x: must be 0", desc->flags);
    if (desc->count && !desc->d_events) return ctx->fail(ZK_ERR_INVALID_ARG, "exp rows: NULL d_events with %u events", desc->count);
    if (desc->count && (uintptr_t)desc->d_events % 8) return ctx->fail(ZK_ERR_INVALID_ARG, "exp rows: d_events at an address that is no multiple of 8");
    if (n >> 32) return ctx->fail(ZK_ERR_INVALID_ARG, "exp rows: %llu rows: 2^32 or more", (unsigned long long)n);
    if (h_b) return ctx->fail(ZK_ERR_INVALID_ARG, "exp rows: the op takes no second operand");
    if ((uintptr_t)d_out % 16 || (uintptr_t)desc->d_exponent_lo_hi % 16 || (uintptr_t)desc->d_mul_cols % 16 || (uintptr_t)desc->d_parity_cols % 16)
        return ctx->fail(ZK_ERR_INVALID_ARG, "exp rows: d_out, d_exponent_lo_hi, d_mul_cols or d_parity_cols at an address that is no multiple of 16");
    if ((uintptr_t)desc->d_base_limb % 8 || (uintptr_t)desc->d_rows_needed % 8)
        return ctx->fail(ZK_ERR_INVALID_ARG, "exp rows: d_base_limb or d_rows_needed at an address that is no multiple of 8");
    if ((uintptr_t)desc->d_mul_u16_64 % 2 || (uintptr_t)desc->d_mul_u16_128 % 2 || (uintptr_t)desc->d_parity_u16_64 % 2 || (uintptr_t)desc->d_parity_u16_128 % 2)
        return ctx->fail(ZK_ERR_INVALID_ARG, "exp rows: a u16 plane at an address that is no multiple of 2");
    SpanList<12> spans;
    spans.add(d_out, n * 16, "d_out", true);
    spans.add(desc->d_is_last, n, "d_is_last", true);
    spans.add(desc->d_base_limb, n * 8, "d_base_limb", true);
    spans.add(desc->d_exponent_lo_hi, n * 16, "d_exponent_lo_hi", true);
    spans.add(desc->d_mul_cols, n * 64, "d_mul_cols", true);
    spans.add(desc->d_mul_u16_64, n * 8, "d_mul_u16_64", true);
    spans.add(desc->d_mul_u16_128, n * 16, "d_mul_u16_128", true);
    spans.add(desc->d_parity_cols, n * 64, "d_parity_cols", true);
    spans.add(desc->d_parity_u16_64, n * 8, "d_parity_u16_64", true);
    spans.add(desc->d_parity_u16_128, n * 16, "d_parity_u16_128", true);
    spans.add(desc->d_rows_needed, 8, "d_rows_needed", true);
    spans.add(desc->d_events, (uint64_t)desc->count * EX_EVENT_BYTES, "d_events", false);
    const char *what, *other;
    if (spans.overlap(&what, &other)) return ctx->fail(ZK_ERR_INVALID_ARG, "exp rows: %s overlaps %s", what, other);
    if (!n) return ZK_OK;

    ExArgs g;
    memset(&g, 0, sizeof g);
    g.events = (const uint64_t*)desc->d_events;
    g.count = desc->count, g.n = (uint32_t)n;
    g.out = (ExCell16*)d_out, g.is_last = (uint8_t*)desc->d_is_last, g.base_limb = (uint64_t*)desc->d_base_limb, g.exponent = (ExCell16*)desc->d_exponent_lo_hi;
    g.mul_cols = (ExCell16*)desc->d_mul_cols, g.mul_u16_64 = (uint8_t*)desc->d_mul_u16_64, g.mul_u16_128 = (uint8_t*)desc->d_mul_u16_128;
    g.parity_cols = (ExCell16*)desc->d_parity_cols, g.parity_u16_64 = (uint8_t*)desc->d_parity_u16_64, g.parity_u16_128 = (uint8_t*)desc->d_parity_u16_128;
    const bool u16 = g.mul_u16_64 || g.mul_u16_128 || g.parity_u16_64 || g.parity_u16_128;

    uint64_t widths = 16;
    widths += (desc->d_is_last ? 1 : 0) + (desc->d_base_limb ? 8 : 0) + (desc->d_exponent_lo_hi ? 16 : 0);
    widths += (desc->d_mul_cols ? 64 : 0) + (desc->d_mul_u16_64 ? 8 : 0) + (desc->d_mul_u16_128 ? 16 : 0);
    widths += (desc->d_parity_cols ? 64 : 0) + (desc->d_parity_u16_64 ? 8 : 0) + (desc->d_parity_u16_128 ? 16 : 0);
    ZkProfScope prof(ctx, "exp_rows");
    prof.bytes = (uint64_t)desc->count * EX_EVENT_BYTES + n * widths;

    // scratch: start[0 .. count] | the sums of the scan's levels | the step sums of k_exp_widths' blocks | the step slots
    const auto pad = [](uint64_t b) { return (b + 255) & ~(uint64_t)255; };
    const uint64_t entries = (uint64_t)g.count + 1, blocks = (entries + 255) / 256;
    const uint64_t starts_bytes = pad(entries * 4);
    uint64_t sums_bytes = 0;
    for (uint64_t c = entries; c > BC_SCAN_TILE;) { c = (c + BC_SCAN_TILE - 1) / BC_SCAN_TILE; sums_bytes += ((c + 63) & ~(uint64_t)63) * 4; }
    sums_bytes = pad(sums_bytes);
    const uint64_t blocks_bytes = pad(blocks * 4), slots_bytes = (n / EX_STEP_ROWS + 1) * 32;
    uint8_t* s = (uint8_t*)ctx->get_scratch(SC_EXP, starts_bytes + sums_bytes + blocks_bytes + slots_bytes);
    if (!s) return ZK_ERR_OOM;
    g.starts = (const uint32_t*)s;
    g.slots = (ExCell16*)(s + starts_bytes + sums_bytes + blocks_bytes);
    uint32_t* block_steps = desc->d_rows_needed ? (uint32_t*)(s + starts_bytes + sums_bytes) : nullptr;
    hipLaunchKernelGGL(k_exp_widths, dim3((unsigned)blocks), dim3(256), 0, ctx->stream, g, (uint32_t*)s, block_steps);
    if (block_steps) hipLaunchKernelGGL(k_exp_total, dim3(1), dim3(256), 0, ctx->stream, (const uint32_t*)block_steps, (uint32_t)blocks, (uint64_t*)desc->d_rows_needed);
    bc_scan(ctx, (uint32_t*)s, entries, (uint32_t*)(s + starts_bytes), g.n);
    if (g.count) {
        ZkProfScope chain(ctx, "exp_rows_chain");                       // the two kernels on their own, inside "exp_rows", no bytes booked
        hipLaunchKernelGGL(k_exp_chain, dim3((unsigned)(((uint64_t)g.count + 255) / 256)), dim3(256), 0, ctx->stream, g);
    }
    const unsigned tiles = (unsigned)((n + EX_TILE - 1) / EX_TILE);
    {
        ZkProfScope rows(ctx, "exp_rows_tiles");
        if (u16) hipLaunchKernelGGL(k_exp_rows<true>, dim3(tiles), dim3(EX_TILE_STEPS), 0, ctx->stream, g);
        else hipLaunchKernelGGL(k_exp_rows<false>, dim3(tiles), dim3(EX_TILE_STEPS), 0, ctx->stream, g);
    }
    ZK_CHECK_LAUNCH(ctx);
    return ZK_OK;
}

}  // namespace zk

// The typed-cell row code: packed little-endian cells of 1, 2, 4, 8 or 16 bytes (and 32-byte Montgomery elements) read where they lie.
//   zk_fr_from_uint(_batch)             out[i] = the Montgomery image of cell[i], one column or sixteen per launch
//   row RLC z = c + sum w_j cell_j      rlc::value / RwRow::rlc across typed columns, one reduction per row       (ZK_OP_ROW_RLC)
//   row inverse z = num * inv0(row RLC) IsZeroChip::value_inv, Assigned::Rational(num, den).evaluate() (K12)      (ZK_OP_ROW_INV0)
// The loader (fu_*) is shared by all three; the typed scan RLC, which walks ALONG a column, lives in csrc/vec.hip beside the affine scan.
#include <algorithm>

#include "ctx.hpp"
#include "ff29.hip.hpp"
#include "op_check.hpp"

namespace zk {

// ---- typed narrow cells: out[i] = Montgomery Fr of the W-byte little-endian unsigned integer in[i] ------------------------------
// One mul29 per cell: the integer (at most five non-zero limbs) times the plain constant 2^517 = 2^256 * 2^261 leaves x * 2^256.
// Memory shape: a wave owns FU_CELLS * 64 consecutive cells and writes them in FU_CELLS sweeps, lane L the cell sweep * 64 + L, so
// every sweep stores 64 consecutive elements (the two 16-byte transactions per lane of the rest of this file).  The loads of all
// sweeps are issued before the first product.  W >= 4: a lane loads its own cell (4 / 8 / 16 B per lane, consecutive lanes on
// consecutive cells).  W < 4: a byte or a halfword per lane would spend a whole load instruction on 64 or 128 bytes, so lane L loads
// the FU_CELLS consecutive cells FU_CELLS * L .. as ONE dword (W = 1) or dwordx2 (W = 2) and the sweeps fetch their cell from the
// owning lane with a shuffle.  That load needs 4 / 8-byte alignment while the caller guarantees W: the launch passes the pointer
// rounded down and `head`, the number of cells of the first packed word that lie in front of the data.  Cells are addressed by their
// virtual index v = i + head; a packed word that is not wholly inside [head, head + n) -- only the first and the last can be --
// is put together from loads of its valid cells alone, so nothing outside the caller's n * W bytes is read.
constexpr int FU_CELLS = 4;
// The packed word (W < 4: FU_CELLS cells, cell t in bits [8 W t, 8 W (t + 1))) at virtual cell q, a multiple of FU_CELLS: one load
// when it lies wholly inside [head, end), else put together from its valid cells alone (none: 0).
template <int W>
__device__ __forceinline__ uint2 fu_packed_word(const uint8_t* __restrict__ src, uint64_t q, uint32_t head, uint64_t end) {
    static_assert(FU_CELLS == 4, "a packed word holds four cells");
    uint32_t lo = 0, hi = 0;
    if (q >= head && q + FU_CELLS <= end) {
        if constexpr (W == 1) lo = *reinterpret_cast<const uint32_t*>(src + q);
        else { const uint2 p = *reinterpret_cast<const uint2*>(src + q * 2); lo = p.x; hi = p.y; }
    } else {
#pragma unroll
        for (int t = 0; t < FU_CELLS; ++t) {
            if (q + t < head || q + t >= end) continue;
            if constexpr (W == 1) lo |= (uint32_t)src[q + t] << (8 * t);
            else {
                const uint32_t c = *reinterpret_cast<const uint16_t*>(src + (q + t) * 2);
                if (t < 2) lo |= c << (16 * t); else hi |= c << (16 * (t - 2));
            }
        }
    }
    return make_uint2(lo, hi);
}
// The loader of both typed-cell kernels, in two halves so that a caller may put the loads of several columns in flight before it
// touches the first cell.  Together: x[j] = the cell at virtual index wave * FU_CELLS * 64 + j * 64 + lane + shift as up to four 32-bit
// words, 0 where that index is outside [head, head + n).  shift is wave-uniform and below FU_CELLS.  k_fr_from_uint* address their
// lanes by virtual index and pass 0; the row RLC, whose lanes own ROWS (the same row in every column, whatever the column's head),
// passes shift = head: the packed words are still loaded at their aligned places, each lane then takes the upper cells of its own
// word and the lower ones of its neighbour's (a shuffle; lane 63 loads the wave's 65th word) -- a funnel shift by `shift` cells -- and
// the sweeps fetch their cells as before.  W >= 4 has head = 0 and takes no shift.
//   fu_load_raw: the loads and nothing else.  W < 4: raw[0] = {this lane's packed word (two halves), lane 63's extra word when shift};
//                W >= 4: raw[j] = the lane's cell of sweep j.
//   fu_cells:    raw -> x (W < 4: the funnel shift and the fetch from the owning lane; W >= 4: a copy)
template <int W>
__device__ __forceinline__ void fu_load_raw(const uint8_t* __restrict__ src, uint32_t head, uint64_t n, uint64_t wave, uint32_t shift, uint32_t (&raw)[FU_CELLS][4]) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t v0 = wave * (FU_CELLS * 64), end = head + n;         // virtual cells [v0, v0 + 256) of this wave; valid: head <= v < end
#pragma unroll
    for (int j = 0; j < FU_CELLS; ++j) raw[j][0] = raw[j][1] = raw[j][2] = raw[j][3] = 0;
    if constexpr (W < 4) {
        const uint64_t q = v0 + (uint64_t)FU_CELLS * lane;              // first virtual cell of this lane's packed word
        const uint2 w = fu_packed_word<W>(src, q, head, end);           // cell t of the word: bits [8 W t, 8 W (t + 1)) of y:x
        raw[0][0] = w.x; raw[0][1] = w.y;
        if (shift && lane == 63u) { const uint2 nx = fu_packed_word<W>(src, q + FU_CELLS, head, end); raw[0][2] = nx.x; raw[0][3] = nx.y; }
    } else {
#pragma unroll
        for (int j = 0; j < FU_CELLS; ++j) {
            const uint64_t v = v0 + (uint64_t)j * 64 + lane;
            if (v >= end) continue;                                     // head == 0 here
            if constexpr (W == 4) raw[j][0] = *reinterpret_cast<const uint32_t*>(src + v * 4);
            else if constexpr (W == 8) { const uint2 p = *reinterpret_cast<const uint2*>(src + v * 8); raw[j][0] = p.x; raw[j][1] = p.y; }
            else { const uint4 p = *reinterpret_cast<const uint4*>(src + v * 16); raw[j][0] = p.x; raw[j][1] = p.y; raw[j][2] = p.z; raw[j][3] = p.w; }
        }
    }
}
template <int W>
__device__ __forceinline__ void fu_cells(const uint32_t (&raw)[FU_CELLS][4], uint32_t shift, uint32_t (&x)[FU_CELLS][4]) {
    const uint32_t lane = threadIdx.x & 63u;
#pragma unroll
    for (int j = 0; j < FU_CELLS; ++j) { x[j][0] = raw[j][0]; x[j][1] = raw[j][1]; x[j][2] = raw[j][2]; x[j][3] = raw[j][3]; }
    if constexpr (W < 4) {
        uint32_t lo = raw[0][0], hi = raw[0][1];
        if (shift) {
            uint2 nx = make_uint2(__shfl_down(lo, 1), __shfl_down(hi, 1));
            if (lane == 63u) nx = make_uint2(raw[0][2], raw[0][3]);
            const uint64_t cur = lo | (uint64_t)hi << 32, nxt = nx.x | (uint64_t)nx.y << 32;
            if constexpr (W == 1) lo = (uint32_t)((lo | nxt << 32) >> (8 * shift));
            else { const uint64_t f = cur >> (16 * shift) | nxt << (64 - 16 * shift); lo = (uint32_t)f; hi = (uint32_t)(f >> 32); }
        }
#pragma unroll
        for (int j = 0; j < FU_CELLS; ++j) {                            // cell j * 64 + lane of the wave sits in lane (j * 64 + lane) / 4, position lane % 4
            const int owner = j * (64 / FU_CELLS) + (int)(lane >> 2);
            const uint32_t t = lane & 3u;
            x[j][1] = x[j][2] = x[j][3] = 0;
            if constexpr (W == 1) x[j][0] = (__shfl(lo, owner) >> (8 * t)) & 0xffu;
            else {
                const uint32_t a = __shfl(lo, owner), b = __shfl(hi, owner);
                x[j][0] = ((t & 2u ? b : a) >> (16 * (t & 1u))) & 0xffffu;
            }
        }
    }
}
template <int W>
__device__ __forceinline__ void fu_load_wave(const uint8_t* __restrict__ src, uint32_t head, uint64_t n, uint64_t wave, uint32_t shift, uint32_t (&x)[FU_CELLS][4]) {
    uint32_t raw[FU_CELLS][4];
    fu_load_raw<W>(src, head, n, wave, shift, raw);
    fu_cells<W>(raw, shift, x);
}
template <int W>
__device__ __forceinline__ void fr_from_uint_wave(const uint8_t* __restrict__ src, uint32_t head, uint64_t n, Fr* __restrict__ out, const Fr& c517_plain, uint64_t wave) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t v0 = wave * (FU_CELLS * 64), end = head + n;
    uint32_t x[FU_CELLS][4];
    fu_load_wave<W>(src, head, n, wave, 0, x);
    const Fr29 c517 = unpack29<Fr29P>(c517_plain);
#pragma unroll
    for (int j = 0; j < FU_CELLS; ++j) {
        const uint64_t v = v0 + (uint64_t)j * 64 + lane;
        if (v < head || v >= end) continue;
        const Fr cell{{x[j][0], x[j][1], x[j][2], x[j][3], 0, 0, 0, 0}};
        stg(out + (v - head), pack29_lt2p(mul29(unpack29<Fr29P>(cell), c517)));
    }
}
template <int W>
__global__ void __launch_bounds__(256) k_fr_from_uint(const uint8_t* __restrict__ src, uint32_t head, uint64_t n, Fr* __restrict__ out, Fr c517_plain) {
    fr_from_uint_wave<W>(src, head, n, out, c517_plain, ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6);
}
// The same for up to FU_BATCH columns of n cells each in ONE launch: blockIdx.y is the column, so a workgroup never straddles two
// columns and its cell width is uniform -- it selects the code path without divergence.  The table travels as a kernel argument (no
// upload, no host synchronisation).  Every column has its own `head` (its pointer is aligned to its cell width only), taken from the
// address here; the grid is sized for the longest column and a wave past its column's end does nothing.
constexpr int FU_BATCH = 16;
struct FuColumn { const void* src; Fr* dst; uint32_t width; };
struct FuBatch { FuColumn col[FU_BATCH]; };
__global__ void __launch_bounds__(256) k_fr_from_uint_batch(FuBatch b, uint64_t n, Fr c517_plain) {
    const FuColumn col = b.col[blockIdx.y];
    const uint32_t load_bytes = col.width < 4 ? col.width * FU_CELLS : col.width;
    const uint32_t head = (uint32_t)((uintptr_t)col.src % load_bytes) / col.width;
    const uint8_t* base = (const uint8_t*)col.src - (size_t)head * col.width;
    const uint64_t wave = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    if (wave * (FU_CELLS * 64) >= head + n) return;                     // whole waves only: the shuffles stay inside a wave
    switch (col.width) {
        case 1: fr_from_uint_wave<1>(base, head, n, col.dst, c517_plain, wave); break;
        case 2: fr_from_uint_wave<2>(base, head, n, col.dst, c517_plain, wave); break;
        case 4: fr_from_uint_wave<4>(base, head, n, col.dst, c517_plain, wave); break;
        case 8: fr_from_uint_wave<8>(base, head, n, col.dst, c517_plain, wave); break;
        default: fr_from_uint_wave<16>(base, head, n, col.dst, c517_plain, wave); break;
    }
}
static const Fr& fr_c517() {
    static const Fr c517 = fr_pow2(517);
    return c517;
}
int fr_from_uint_run(zk_ctx* ctx, hipStream_t stream, const void* d_packed, uint32_t width, uint64_t n, Fr* d_out) {
    if (!typed_cell_width_ok(width, false)) return ctx->fail(ZK_ERR_INVALID_ARG, "cell width %u: must be 1, 2, 4, 8 or 16 bytes", width);
    if ((uintptr_t)d_packed % typed_cell_align(width)) return ctx->fail(ZK_ERR_INVALID_ARG, "packed cells of %u bytes at an address that is no multiple of %u", width, width);
    if (!n) return ZK_OK;
    const Fr& c517 = fr_c517();
    const uint32_t load_bytes = width < 4 ? width * FU_CELLS : width;
    const uint32_t head = (uint32_t)((uintptr_t)d_packed % load_bytes) / width;
    const uint8_t* base = (const uint8_t*)d_packed - (size_t)head * width;
    const uint64_t per_block = (uint64_t)FU_CELLS * 256, blocks = (head + n + per_block - 1) / per_block;
    if (blocks > 0x7fffffffull) return ctx->fail(ZK_ERR_INVALID_ARG, "too many cells for one launch");
    ZkProfScope prof(ctx, "fr_from_uint", stream);
    prof.bytes = n * (width + 32ull);
    const dim3 g((unsigned)blocks), t(256);
    switch (width) {
        case 1: hipLaunchKernelGGL(k_fr_from_uint<1>, g, t, 0, stream, base, head, n, d_out, c517); break;
        case 2: hipLaunchKernelGGL(k_fr_from_uint<2>, g, t, 0, stream, base, head, n, d_out, c517); break;
        case 4: hipLaunchKernelGGL(k_fr_from_uint<4>, g, t, 0, stream, base, head, n, d_out, c517); break;
        case 8: hipLaunchKernelGGL(k_fr_from_uint<8>, g, t, 0, stream, base, head, n, d_out, c517); break;
        default: hipLaunchKernelGGL(k_fr_from_uint<16>, g, t, 0, stream, base, head, n, d_out, c517); break;
    }
    ZK_CHECK_LAUNCH(ctx);
    return ZK_OK;
}
// count columns, FU_BATCH per launch; everything is validated before the first launch, so a refused call has written nothing
int fr_from_uint_batch_run(zk_ctx* ctx, hipStream_t stream, const void* const* d_packed, const uint8_t* widths, size_t count, uint64_t n, Fr* const* d_out) {
    for (size_t c = 0; c < count; ++c) {
        const uint32_t width = widths[c];
        if (!typed_cell_width_ok(width, false)) return ctx->fail(ZK_ERR_INVALID_ARG, "column %zu: cell width %u: must be 1, 2, 4, 8 or 16 bytes", c, width);
        if ((uintptr_t)d_packed[c] % typed_cell_align(width)) return ctx->fail(ZK_ERR_INVALID_ARG, "column %zu: packed cells of %u bytes at an address that is no multiple of %u", c, width, width);
    }
    if (!n || !count) return ZK_OK;
    const uint64_t per_block = (uint64_t)FU_CELLS * 256, blocks = (FU_CELLS - 1 + n + per_block - 1) / per_block;      // a column's head is below FU_CELLS cells
    if (blocks > 0x7fffffffull) return ctx->fail(ZK_ERR_INVALID_ARG, "too many cells for one launch");
    for (size_t c0 = 0; c0 < count; c0 += FU_BATCH) {
        const size_t cnt = std::min<size_t>(FU_BATCH, count - c0);
        FuBatch b;
        ZkProfScope prof(ctx, "fr_from_uint_batch", stream);
        for (size_t c = 0; c < FU_BATCH; ++c) {
            if (c < cnt) { b.col[c] = {d_packed[c0 + c], d_out[c0 + c], widths[c0 + c]}; prof.bytes += n * (widths[c0 + c] + 32ull); }
            else b.col[c] = {nullptr, nullptr, 0};
        }
        hipLaunchKernelGGL(k_fr_from_uint_batch, dim3((unsigned)blocks, (unsigned)cnt), dim3(256), 0, stream, b, n, fr_c517());
    }
    ZK_CHECK_LAUNCH(ctx);
    return ZK_OK;
}

// ---- row RLC of typed cells: out[i] = c + sum_j w_j * cell_j[i] (ZK_OP_ROW_RLC) ----------------------------------------------------
// The RLC ACROSS the columns of a row (rlc::value over the bytes of a word, RwRow::rlc over mixed-width fields), from the packed cells
// themselves: nothing is expanded to 32 bytes and no term is reduced.  A lane owns one row per sweep in the wave, sweep and store shape
// of fr_from_uint_wave (a wave covers FU_CELLS * 64 consecutive rows, fu_load_raw / fu_cells fetch every column's cells of those rows), keeps one
// Rlc29 (csrc/ff29.hip.hpp: 18 integer column sums) per sweep and walks the columns in a wave-uniform loop: cell limbs (1, 1, 2, 3, 5
// for 1, 2, 4, 8, 16 bytes; 9 for a 32-byte Montgomery element) times the nine limbs of the column's constant K_j, which sit in scalar
// registers.  The host prepares K_j as plain normalised limbs: w_j 2^517 for a narrow column (x K_j / 2^261 = w_j x 2^256, the Montgomery
// image, as in k_fr_from_uint), w_j 2^261 for a 32-byte column (whose cells carry their 2^256 already), c 2^517 for the constant, which
// starts the sums.  ONE reduction by 2^261 and one conditional subtraction per row.  Bounds (kept by rlc29_mac and by RR_BATCH, see
// ff29.hip.hpp): a carry pass before a column sum could overflow, and at most RR_BATCH <= 64 terms below p^2 under one reduction, far
// inside the 169 that T < 2^261 p admits.  The table (pointer, width, K limbs: 48 B a column) travels as a kernel argument: no upload,
// no host synchronisation.  More than RR_BATCH columns: the next launch takes d_out as its first column, 32 bytes wide with weight one
// -- a lane reads all its rows before it writes them, so that column may be the output itself.  The same holds for a caller's column
// that is d_out, but only inside one launch: fr_row_rlc_run gives every such column to the FIRST launch (merged into one term).
constexpr int RR_BATCH = 64;
struct RrColumn { const void* src; uint32_t width; uint32_t k[9]; };
struct RrBatch { RrColumn col[RR_BATCH]; uint32_t k0[9]; uint32_t count; };
static_assert(RR_BATCH <= 64 && sizeof(RrBatch) < 4096 - 64, "terms under one reduction (T < 2^261 p), kernel argument size");
// The terms of a run of up to G columns of one width, from column j on; returns how many it took.  The host has sorted the table by
// width (the order of a sum is free), so runs are long; all loads of a run are issued before its first product -- a byte column is
// ONE 4-byte load per lane, and a wave that waited for each of them by itself would spend its time on memory latency.
template <int W>
__device__ __forceinline__ uint32_t row_rlc_terms(const RrBatch& b, uint32_t j, uint64_t n, uint64_t wave, Rlc29<Fr29P> (&acc)[FU_CELLS]) {
    constexpr int L = W <= 2 ? 1 : W == 4 ? 2 : W == 8 ? 3 : W == 16 ? 5 : 9;
    constexpr int G = W <= 2 ? 8 : W == 4 ? 4 : W <= 16 ? 2 : 1;
    if constexpr (W == 32) {
        const RrColumn& col = b.col[j];
        const uint32_t lane = threadIdx.x & 63u;
        const uint2* src = (const uint2*)col.src;                       // 8-byte aligned
        uint2 v[FU_CELLS][4];
#pragma unroll
        for (int s = 0; s < FU_CELLS; ++s) {
            const uint64_t row = wave * (FU_CELLS * 64) + (uint64_t)s * 64 + lane;
#pragma unroll
            for (int q = 0; q < 4; ++q) v[s][q] = row < n ? src[row * 4 + q] : make_uint2(0, 0);
        }
#pragma unroll
        for (int s = 0; s < FU_CELLS; ++s) {
            const Fr cell{{v[s][0].x, v[s][0].y, v[s][1].x, v[s][1].y, v[s][2].x, v[s][2].y, v[s][3].x, v[s][3].y}};
            const Fr29 x = unpack29<Fr29P>(cell);
            rlc29_mac<9>(acc[s], x.l, col.k);
        }
        return 1;
    } else {
        constexpr uint32_t load_bytes = W < 4 ? W * FU_CELLS : W;
        uint32_t g = 1;
        while (g < (uint32_t)G && j + g < b.count && b.col[j + g].width == (uint32_t)W) ++g;
        static_assert(G * L < (int)RLC29_MAX_LOAD, "a run fits between two carry passes");
#pragma unroll
        for (int s = 0; s < FU_CELLS; ++s) rlc29_room(acc[s], G * L);   // one test and one place for the carry pass per run and sweep
        uint32_t raw[G][FU_CELLS][4];
#pragma unroll
        for (int c = 0; c < G; ++c) {
            if ((uint32_t)c >= g) break;                                // wave-uniform
            const uint8_t* src = (const uint8_t*)b.col[j + c].src;
            const uint32_t head = (uint32_t)((uintptr_t)src % load_bytes) / W;
            fu_load_raw<W>(src - (size_t)head * W, head, n, wave, head, raw[c]);
        }
#pragma unroll
        for (int c = 0; c < G; ++c) {
            if ((uint32_t)c >= g) break;
            const RrColumn& col = b.col[j + c];
            const uint32_t head = (uint32_t)((uintptr_t)col.src % load_bytes) / W;
            uint32_t x[FU_CELLS][4];
            fu_cells<W>(raw[c], head, x);
#pragma unroll
            for (int s = 0; s < FU_CELLS; ++s) {                        // rows at or past n read as 0 and are not stored
                const Fr cell{{x[s][0], x[s][1], x[s][2], x[s][3], 0, 0, 0, 0}};
                const Fr29 xl = unpack29<Fr29P>(cell);
                rlc29_mac<L>(acc[s], xl.l, col.k);
            }
        }
        return g;
    }
}
// the sums of a wave's rows over the whole table, unreduced: acc[s] is the row wave * FU_CELLS * 64 + s * 64 + lane.  A macro, not a
// function: with the accumulators handed on by reference the compiler spills them (k_fr_row_rlc: 414 registers and no scratch as
// written here, 512 and 196 B of scratch per lane through a function).
#define ZK_ROW_RLC_SUMS(b, n, wave, acc)                                                                                   \
    _Pragma("unroll") for (int s = 0; s < FU_CELLS; ++s) rlc29_init(acc[s], b.k0);                                         \
    for (uint32_t j = 0; j < b.count;) {                                /* wave-uniform, and so is the width */            \
        switch (b.col[j].width) {                                                                                          \
            case 1: j += row_rlc_terms<1>(b, j, n, wave, acc); break;                                                      \
            case 2: j += row_rlc_terms<2>(b, j, n, wave, acc); break;                                                      \
            case 4: j += row_rlc_terms<4>(b, j, n, wave, acc); break;                                                      \
            case 8: j += row_rlc_terms<8>(b, j, n, wave, acc); break;                                                      \
            case 16: j += row_rlc_terms<16>(b, j, n, wave, acc); break;                                                    \
            default: j += row_rlc_terms<32>(b, j, n, wave, acc); break;                                                    \
        }                                                                                                                  \
    }
__global__ void __launch_bounds__(256) k_fr_row_rlc(RrBatch b, uint64_t n, Fr* out) {
    const uint64_t wave = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    if (wave * (FU_CELLS * 64) >= n) return;                            // whole waves only: the shuffles stay inside a wave
    const uint32_t lane = threadIdx.x & 63u;
    Rlc29<Fr29P> acc[FU_CELLS];
    ZK_ROW_RLC_SUMS(b, n, wave, acc)
#pragma unroll
    for (int s = 0; s < FU_CELLS; ++s) {
        const uint64_t row = wave * (FU_CELLS * 64) + (uint64_t)s * 64 + lane;
        if (row < n) stg(out + row, pack29_lt2p(rlc29_reduce(acc[s])));
    }
}
// ---- inverse-or-zero of a row RLC: out[i] = num[i] * inv0(c + sum_j w_j * cell_j[i]) (ZK_OP_ROW_INV0) ----------------------------------
// IsZeroChip's value_inv, IsEqual's inverse of a difference, halo2's Assigned::Rational(num, den).evaluate() with a denominator that is
// linear in typed cells, in ONE launch that writes only d_out.  A wave takes RI_TILES consecutive tiles of FU_CELLS * 64 rows, each in
// the wave, sweep and store shape of k_fr_row_rlc and by its column walk (ZK_ROW_RLC_SUMS over row_rlc_terms); a tile's FU_CELLS Rlc29
// records are dead once its denominators are reduced, and the lane's RI_ROWS = RI_TILES * FU_CELLS denominators then go the way of
// k_batch_invert's BI_K values: zeros skipped, prefix products in the lane, products over the wave from both ends by shuffles, ONE
// inv29_rp per wave on lane 63, back-substitution -- one inversion per RI_TILES * 256 rows.  The arithmetic of a lane, the forms and
// the operand bounds are inv0_29_* in csrc/ff29.hip.hpp (a host harness runs exactly that code).  Rows at or past n and zero rows
// enter the products as one (`live`); a wave whose rows are all zero inverts the constant one; whole waves past n have left before
// any shuffle, and a tile past n is skipped by the whole wave.  A lane reads all its rows of every column, the numerator included,
// before its first store, and the shuffles move values between lanes, never rows: d_out may be a 32-byte column of this launch,
// denominator or numerator.
// Rows per inversion.  inv_xgcd runs on one lane while its wave waits, and at one wave per SIMD (the column walk needs 414
// registers) nothing else runs on that SIMD meanwhile: the kernel's time is (waves / wave slots) rounds of one inversion each, about
// 130 us a round on an MI355X, so the rows of a wave are what counts.  Measured at 2^20 rows (profiles/r23_row_inv0.md): 256 rows
// 0.59 ms, 512 rows 0.34 ms, 1024 rows 0.20 ms (one round on 1024 wave slots; the composition of three calls it replaces: 0.195 ms).
// RI_TILES = 4 it is.  A tile's denominators wait in LDS (144 KB of the CU's 160 KB for the one resident workgroup), not in registers,
// because the tiles have to be a loop; see there.  ZK_ROW_INV0_TILES = 1, 2 build the other forms (A/B builds: make VARIANT=...
// EXTRA=-DZK_ROW_INV0_TILES=...).
// NUM: how a numerator is read -- INV0_NUM_ONE none, INV0_NUM_UINT packed cells of num_width bytes (loaded like a column of the
// table), INV0_NUM_FR canonical Montgomery elements; cinv is the plain constant of inv29_rp that puts the wave's inverse into the form
// that NUM wants (fr_row_inv0_run), one_rp the integer 2^261 mod r.
#ifndef ZK_ROW_INV0_TILES
#define ZK_ROW_INV0_TILES 4
#endif
constexpr int RI_TILES = ZK_ROW_INV0_TILES, RI_ROWS = RI_TILES * FU_CELLS;
static_assert(RI_TILES == 1 || RI_TILES == 2 || RI_TILES == 4, "256, 512 or 1024 rows per inversion");
struct RiArgs { const void* num; uint32_t num_width; uint32_t one_rp[9]; uint32_t cinv[9]; };
static_assert(sizeof(RrBatch) + sizeof(RiArgs) < 4096 - 64, "kernel argument size");
template <int W>
__device__ __forceinline__ void row_inv0_num(const void* num, uint64_t n, uint64_t tile, Fr29* x29) {
    constexpr uint32_t load_bytes = W < 4 ? W * FU_CELLS : W;
    const uint8_t* src = (const uint8_t*)num;
    const uint32_t head = (uint32_t)((uintptr_t)src % load_bytes) / W;
    uint32_t x[FU_CELLS][4];
    fu_load_wave<W>(src - (size_t)head * W, head, n, tile, head, x);
#pragma unroll
    for (int s = 0; s < FU_CELLS; ++s) x29[s] = unpack29<Fr29P>(Fr{{x[s][0], x[s][1], x[s][2], x[s][3], 0, 0, 0, 0}});
}
template <int NUM>
__global__ void __launch_bounds__(256) k_fr_row_inv0(RrBatch b, RiArgs a, uint64_t n, Fr* out) {
    const uint64_t tile0 = (((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6) * RI_TILES;     // this wave's first tile of 256 rows
    if (tile0 * (FU_CELLS * 64) >= n) return;                           // whole waves only: the shuffles stay inside a wave
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t row0 = tile0 * (FU_CELLS * 64) + lane;               // this lane's rows: row0 + 64 k, k < RI_ROWS
    Fr29 d[RI_ROWS], num[RI_ROWS];
    uint32_t live = 0;
    if constexpr (RI_TILES == 1) {
        Rlc29<Fr29P> acc[FU_CELLS];
        ZK_ROW_RLC_SUMS(b, n, tile0, acc)
#pragma unroll
        for (int s = 0; s < FU_CELLS; ++s)
            if (inv0_29_den(acc[s], d[s]) && row0 + 64u * s < n) live |= 1u << s;
    } else {
        // ONE copy of the column walk in a loop that is not unrolled (two copies in line spill 3 KB per lane), so a tile's
        // denominators cannot go to registers named by the loop variable: they are parked in LDS, limb k of row r of thread T at
        // [r][k][T] (no bank conflicts, no barrier: a lane reads back what it wrote), and fetched once all tiles are done
        __shared__ uint32_t park[RI_ROWS][9][256];
#pragma unroll 1
        for (int t = 0; t < RI_TILES; ++t) {
            if ((tile0 + t) * (FU_CELLS * 64) >= n) break;              // wave-uniform
            Rlc29<Fr29P> acc[FU_CELLS];
            ZK_ROW_RLC_SUMS(b, n, (tile0 + t), acc)
#pragma unroll
            for (int s = 0; s < FU_CELLS; ++s) {
                Fr29 ds;
                if (inv0_29_den(acc[s], ds) && row0 + 64u * (t * FU_CELLS + s) < n) live |= 1u << (t * FU_CELLS + s);
#pragma unroll
                for (int k = 0; k < 9; ++k) park[t * FU_CELLS + s][k][threadIdx.x] = ds.l[k];
            }
        }
#pragma unroll
        for (int r = 0; r < RI_ROWS; ++r)                               // rows of a skipped tile are not live: whatever is there is not used
#pragma unroll
            for (int k = 0; k < 9; ++k) d[r].l[k] = park[r][k][threadIdx.x];
    }
    if constexpr (NUM == INV0_NUM_FR) {
        const uint2* src = (const uint2*)a.num;                         // 8-byte aligned
        uint2 v[RI_ROWS][4];
#pragma unroll
        for (int k = 0; k < RI_ROWS; ++k)
#pragma unroll
            for (int q = 0; q < 4; ++q) v[k][q] = row0 + 64u * k < n ? src[(row0 + 64u * k) * 4 + q] : make_uint2(0, 0);
#pragma unroll
        for (int k = 0; k < RI_ROWS; ++k) num[k] = unpack29<Fr29P>(Fr{{v[k][0].x, v[k][0].y, v[k][1].x, v[k][1].y, v[k][2].x, v[k][2].y, v[k][3].x, v[k][3].y}});
    } else if constexpr (NUM == INV0_NUM_UINT) {
#define ZK_ROW_INV0_NUM(t)                                                                                                 \
    if ((tile0 + t) * (FU_CELLS * 64) < n) {                            /* wave-uniform, and so is the width */            \
        switch (a.num_width) {                                                                                             \
            case 1: row_inv0_num<1>(a.num, n, tile0 + t, num + t * FU_CELLS); break;                                       \
            case 2: row_inv0_num<2>(a.num, n, tile0 + t, num + t * FU_CELLS); break;                                       \
            case 4: row_inv0_num<4>(a.num, n, tile0 + t, num + t * FU_CELLS); break;                                       \
            case 8: row_inv0_num<8>(a.num, n, tile0 + t, num + t * FU_CELLS); break;                                       \
            default: row_inv0_num<16>(a.num, n, tile0 + t, num + t * FU_CELLS); break;                                     \
        }                                                                                                                  \
    }
        ZK_ROW_INV0_NUM(0)
        if constexpr (RI_TILES > 1) { ZK_ROW_INV0_NUM(1) }
        if constexpr (RI_TILES > 2) { ZK_ROW_INV0_NUM(2) ZK_ROW_INV0_NUM(3) }
#undef ZK_ROW_INV0_NUM
    }
    Fr29 one_rp, cinv, pre[RI_ROWS];
#pragma unroll
    for (int k = 0; k < 9; ++k) { one_rp.l[k] = a.one_rp[k]; cinv.l[k] = a.cinv[k]; }
    const Fr29 mine = inv0_29_prefix(d, live, one_rp, pre);
    // inclusive products over the lanes from both ends
    Fr29 up = mine, down = mine;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const Fr29 u = shfl_up29(up, off), dn = shfl_down29(down, off);
        if (lane >= (uint32_t)off) up = mul29(up, u);
        if (lane + off < 64u) down = mul29(down, dn);
    }
    // one inversion per wave: of the product of all its lanes, into the form the numerator wants
    Fr29 inv_total = one_rp;
    if (lane == 63u) inv_total = inv29_rp(up, cinv);
    inv_total = shfl29(inv_total, 63);
    // 1 / (this lane's product) = 1 / total x (product of the lanes below) x (product of the lanes above)
    const Fr29 below = shfl_up29(up, 1), above = shfl_down29(down, 1);
    Fr29 iv = inv_total;
    if (lane > 0u) iv = mul29(iv, below);
    if (lane < 63u) iv = mul29(iv, above);
    Fr29 q[RI_ROWS];
    inv0_29_back(iv, d, pre, live, q);
#pragma unroll
    for (int k = 0; k < RI_ROWS; ++k) {
        if (row0 + 64u * k >= n) continue;
        stg(out + row0 + 64u * k, live >> k & 1u ? inv0_29_out<NUM>(q[k], num[k]) : Fr::zero());
    }
}

// ---- the host side of both row ops --------------------------------------------------------------------------------------------------
// One typed column (of the table, or the numerator of ZK_OP_ROW_INV0) against the op's output: width, pointer, alignment, and the
// overlap rule -- a lane reads its rows of every column before it writes them: the output may BE a 32-byte column, and nothing else.
static int rr_check_column(zk_ctx* ctx, const char* op, const char* what, size_t c, const void* col, uint32_t width, const Fr* d_out, uint64_t n) {
    const uintptr_t o = (uintptr_t)d_out, o_end = o + n * sizeof(Fr), p = (uintptr_t)col, p_end = p + n * width;
    if (!typed_cell_width_ok(width, true)) return ctx->fail(ZK_ERR_INVALID_ARG, "%s %s %zu: cell width %u: must be 1, 2, 4, 8, 16 or 32 bytes", op, what, c, width);
    if (!p) return ctx->fail(ZK_ERR_INVALID_ARG, "%s %s %zu: NULL pointer", op, what, c);
    if (p % typed_cell_align(width)) return ctx->fail(ZK_ERR_INVALID_ARG, "%s %s %zu: cells of %u bytes at a misaligned address", op, what, c, width);
    if (n && !(width == 32 && p == o) && p < o_end && o < p_end) return ctx->fail(ZK_ERR_INVALID_ARG, "%s %s %zu overlaps the output", op, what, c);
    return ZK_OK;
}
// the column table of a row op: everything is validated before the first launch, so a refused call has written nothing
static int rr_validate(zk_ctx* ctx, const char* op, size_t count, const void* const* d_cols, const uint8_t* widths, const Fr* d_out, uint64_t n) {
    if (count && (!d_cols || !widths)) return ctx->fail(ZK_ERR_INVALID_ARG, "%s: NULL column or width table", op);
    for (size_t c = 0; c < count; ++c)
        if (int e = rr_check_column(ctx, op, "column", c, d_cols[c], widths[c], d_out, n)) return e;
    return ZK_OK;
}
static void rr_limbs(uint32_t* k, const Fr& mont, const Fr& by) {       // plain normalised limbs of (value of mont) * by: canonical, below 2^29 each
    const Fr29 l = unpack29<Fr29P>(mont * by);
    for (int i = 0; i < 9; ++i) k[i] = l.l[i];
}
// The terms in launch order.  "A lane reads its rows before it writes them" holds inside ONE launch only: the first launch
// overwrites d_out, so every column that IS d_out must be read by it.  All of them (there may be several) become one term with
// the sum of their weights, at the head of the list; the others follow in table order.
struct RrTerm { const void* src; uint32_t width; Fr w; uint32_t booked; };
static std::vector<RrTerm> rr_terms(size_t count, const void* const* d_cols, const uint8_t* widths, const uint8_t* hk, const Fr* d_out) {
    std::vector<RrTerm> terms;
    terms.reserve(count + 1);
    Fr alias_w = Fr::zero();
    uint32_t alias_bytes = 0;
    for (size_t c = 0; c < count; ++c) {
        Fr w;
        memcpy(&w, hk + (1 + c) * sizeof(Fr), sizeof w);
        if (widths[c] == 32 && d_cols[c] == (const void*)d_out) { alias_w = alias_w + w; alias_bytes += 32; continue; }
        terms.push_back({d_cols[c], widths[c], w, widths[c]});
    }
    if (alias_bytes) terms.insert(terms.begin(), {d_out, 32, alias_w, alias_bytes});   // booked as the table states it: 32 B per aliased column
    return terms;
}
// The next launch's table: the constant (first launch) or the sum so far as a 32-byte column of weight one (k0 stays 0), then the
// terms from c0 on, RR_BATCH in all.  K = w 2^(517 + up) for a narrow column and the constant, w 2^(261 + up) for a 32-byte one: up = 0
// leaves the Montgomery image of the sum, up = 5 its R' = 2^261 form (the inverting launch).  Returns the launch's booked widths.
static uint64_t rr_fill(RrBatch& b, const std::vector<RrTerm>& terms, size_t& c0, const uint8_t* hk, const Fr* d_out, bool up) {
    static const Fr by[2][2] = {{fr_pow2(517), fr_pow2(261)}, {fr_pow2(522), fr_pow2(266)}};      // [up][32-byte]
    memset(&b, 0, sizeof b);
    uint64_t width_sum = 0;
    uint32_t cnt = 0;
    if (c0 == 0) {
        Fr c;
        memcpy(&c, hk, sizeof c);
        rr_limbs(b.k0, c, by[up][0]);
    } else {
        b.col[cnt] = {d_out, 32, {}};
        rr_limbs(b.col[cnt].k, Fr::one(), by[up][1]);
        width_sum += 32;
        ++cnt;
    }
    for (; cnt < RR_BATCH && c0 < terms.size(); ++cnt, ++c0) {
        b.col[cnt] = {terms[c0].src, terms[c0].width, {}};
        rr_limbs(b.col[cnt].k, terms[c0].w, by[up][terms[c0].width == 32]);
        width_sum += terms[c0].booked;
    }
    b.count = cnt;
    std::stable_sort(b.col, b.col + cnt, [](const RrColumn& x, const RrColumn& y) { return x.width < y.width; });   // runs of one width for the kernel
    return width_sum;
}
// desc->count columns, RR_BATCH per launch.  h_k: the constant and the count weights, Montgomery Fr in host memory.
int fr_row_rlc_run(zk_ctx* ctx, const zk_row_rlc* desc, const void* h_k, Fr* d_out, uint64_t n) {
    if (int e = rr_validate(ctx, "row RLC", desc->count, desc->d_cols, desc->widths, d_out, n)) return e;
    if (!n) return ZK_OK;
    const uint64_t per_block = (uint64_t)FU_CELLS * 256, blocks = (n + per_block - 1) / per_block;
    if (blocks > 0x7fffffffull) return ctx->fail(ZK_ERR_INVALID_ARG, "too many rows for one launch");
    const uint8_t* hk = (const uint8_t*)h_k;
    const std::vector<RrTerm> terms = rr_terms(desc->count, desc->d_cols, desc->widths, hk, d_out);
    size_t c0 = 0;
    do {
        RrBatch b;
        ZkProfScope prof(ctx, "fr_row_rlc");
        prof.bytes = n * (rr_fill(b, terms, c0, hk, d_out, false) + 32ull);
        hipLaunchKernelGGL(k_fr_row_rlc, dim3((unsigned)blocks), dim3(256), 0, ctx->stream, b, n, d_out);
    } while (c0 < terms.size());
    ZK_CHECK_LAUNCH(ctx);
    return ZK_OK;
}
// The same table under an inversion.  More than RR_BATCH terms: the earlier launches are k_fr_row_rlc itself into d_out (the sum so
// far) and only the last one inverts; d_out then holds that sum, so it cannot also be the numerator -- refused, like any overlap.
int fr_row_inv0_run(zk_ctx* ctx, const zk_row_inv0* desc, const void* h_k, Fr* d_out, uint64_t n) {
    if (int e = rr_validate(ctx, "row inverse", desc->count, desc->d_cols, desc->widths, d_out, n)) return e;
    if (desc->d_num)
        if (int e = rr_check_column(ctx, "row inverse", "numerator", 0, desc->d_num, desc->num_width, d_out, n)) return e;
    if (!n) return ZK_OK;
    const uint64_t per_block = (uint64_t)FU_CELLS * 256, blocks = (n + per_block - 1) / per_block;                   // k_fr_row_rlc's
    const uint64_t inv_blocks = (n + per_block * RI_TILES - 1) / (per_block * RI_TILES);                              // a wave takes RI_TILES tiles
    if (blocks > 0x7fffffffull) return ctx->fail(ZK_ERR_INVALID_ARG, "too many rows for one launch");
    const uint8_t* hk = (const uint8_t*)h_k;
    const std::vector<RrTerm> terms = rr_terms(desc->count, desc->d_cols, desc->widths, hk, d_out);
    if (terms.size() > RR_BATCH && desc->d_num == (const void*)d_out) return ctx->fail(ZK_ERR_INVALID_ARG, "row inverse: the output holds the sum so far of more than %d columns and cannot be the numerator", RR_BATCH);
    // the constant of inv29_rp by numerator: the quotients come out as [1/D]_256 (they are the result), [1/D]_261 (times [N]_256) or
    // [1/D]_517 (times the integer N) -- csrc/ff29.hip.hpp
    static const Fr c261 = fr_pow2(261), cinv[3] = {fr_pow2(778), fr_pow2(1039), fr_pow2(783)};
    const int num = !desc->d_num ? INV0_NUM_ONE : desc->num_width == 32 ? INV0_NUM_FR : INV0_NUM_UINT;
    RiArgs a;
    memset(&a, 0, sizeof a);
    a.num = desc->d_num;
    a.num_width = desc->d_num ? desc->num_width : 0;
    const Fr29 one_l = unpack29<Fr29P>(c261), cinv_l = unpack29<Fr29P>(cinv[num]);
    for (int i = 0; i < 9; ++i) { a.one_rp[i] = one_l.l[i]; a.cinv[i] = cinv_l.l[i]; }
    size_t c0 = 0;
    do {
        RrBatch b;
        ZkProfScope prof(ctx, "fr_row_inv0");
        const bool last = terms.size() - c0 <= (size_t)RR_BATCH - (c0 ? 1 : 0);
        const uint64_t width_sum = rr_fill(b, terms, c0, hk, d_out, last);
        const dim3 g((unsigned)blocks), t(256);
        if (!last) {
            prof.bytes = n * (width_sum + 32ull);
            hipLaunchKernelGGL(k_fr_row_rlc, g, t, 0, ctx->stream, b, n, d_out);
            continue;
        }
        prof.bytes = n * (width_sum + a.num_width + 32ull);
        const dim3 gi((unsigned)inv_blocks);
        switch (num) {
            case INV0_NUM_ONE: hipLaunchKernelGGL(k_fr_row_inv0<INV0_NUM_ONE>, gi, t, 0, ctx->stream, b, a, n, d_out); break;
            case INV0_NUM_UINT: hipLaunchKernelGGL(k_fr_row_inv0<INV0_NUM_UINT>, gi, t, 0, ctx->stream, b, a, n, d_out); break;
            default: hipLaunchKernelGGL(k_fr_row_inv0<INV0_NUM_FR>, gi, t, 0, ctx->stream, b, a, n, d_out); break;
        }
    } while (c0 < terms.size());
    ZK_CHECK_LAUNCH(ctx);
    return ZK_OK;
}
}  // namespace zk

using namespace zk;

extern "C" {

int zk_fr_from_uint(zk_ctx* ctx, const void* d_packed, uint32_t width_bytes, size_t n, void* d_out) {
    if (!ctx) return ZK_ERR_INVALID_ARG;
    ZK_REQUIRE(ctx, (d_packed && d_out) || !n, "null pointer");
    const uintptr_t a = (uintptr_t)d_packed, o = (uintptr_t)d_out;
    ZK_REQUIRE(ctx, width_bytes > 16 || a + n * width_bytes <= o || o + n * sizeof(Fr) <= a, "the output overlaps the packed cells");
    return fr_from_uint_run(ctx, ctx->stream, d_packed, width_bytes, n, (Fr*)d_out);
}

int zk_fr_from_uint_batch(zk_ctx* ctx, const void* const* d_packed, const uint8_t* widths, size_t count, size_t n, void* const* d_out) {
    if (!ctx) return ZK_ERR_INVALID_ARG;
    if (!count) return ZK_OK;
    ZK_REQUIRE(ctx, d_packed && widths && d_out, "null pointer");
    // an output may touch neither another output nor any input (inputs may coincide): one sweep over the buffers in address order
    std::vector<Span> spans;
    for (size_t c = 0; c < count; ++c) {
        ZK_REQUIRE(ctx, (d_packed[c] && d_out[c]) || !n, "null column pointer");
        if (widths[c] > 16) continue;                                   // refused below, with the other widths
        spans.push_back({(uintptr_t)d_packed[c], (uintptr_t)d_packed[c] + n * widths[c], "packed cells", false});
        spans.push_back({(uintptr_t)d_out[c], (uintptr_t)d_out[c] + n * sizeof(Fr), "an output", true});
    }
    std::sort(spans.begin(), spans.end(), [](const Span& x, const Span& y) { return x.lo < y.lo; });
    uintptr_t end_any = 0, end_out = 0;
    for (const Span& s : spans) {
        ZK_REQUIRE(ctx, s.lo >= (s.out ? end_any : end_out) || !n, "an output overlaps another output or packed cells");
        end_any = std::max(end_any, s.hi);
        if (s.out) end_out = std::max(end_out, s.hi);
    }
    return fr_from_uint_batch_run(ctx, ctx->stream, d_packed, widths, count, n, (Fr* const*)d_out);
}
}  // extern "C"

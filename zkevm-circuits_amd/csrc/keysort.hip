// ZK_OP_KEY_SORT and ZK_OP_KEY_ORDER of zk_field_vec_op: the row order of the state circuit and its ordering witness, from key records
// that live on the device.  A record is 64 bytes, compared as a big-endian 512-bit integer; rw_to_be_limbs of the reference packs an
// RW row into one (include/zkmi355.h has the layout).  The per-lane code and every index of the sort are csrc/keyorder.hip.hpp, which
// the host compiles too; this file holds the kernels and the host side.
//
// The sort is a least-significant-digit radix sort of the PERMUTATION: the records stay where they are, a pass moves 4-byte indices
// between two scratch buffers and reads one byte of the record each index names.  One digit is one key byte; the passes run from byte
// 63 up to byte 0 over the bytes the host's mask keeps.  Launches per call:
//   k_ks_init     buffer 0 = identity; OR of (record ^ record 0) over all records -> the bytes at which the records differ at all.
//                 The OR goes through atomicOr, whose result does not depend on the order of arrival.
//   per kept byte k_ks_count   a workgroup's 256-bin histogram of its tile (LDS adds; a count has no order) -> counts[bin][tile]
//                 k_ks_scan    one workgroup per bin: exclusive scan along its row of counts, the row's total -> bin_total[bin]
//                 k_ks_scatter a workgroup scans the 256 bin totals, ranks the places of its tile and stores every index at
//                              bin base + tile base + wave base + rank
//   k_ks_finish   d_out = the buffer the last live pass wrote; d_sorted = the records in that order
// A pass whose byte no record differs in is dead: its three launches return at once, and as only live passes change buffers, every
// workgroup works the buffer it reads out of the mask of live bytes (ks_source).  That is the pruning, decided on the device; the host
// never waits.  Ranks inside a tile: a wave takes KS_ITEMS rounds of 64 consecutive places; in a round the lanes that hold the same
// digit find each other by eight __ballot's (ks_peers), the lowest of them reads and advances the wave's counter of that digit in LDS
// -- one lane per digit and wave, no atomics, rounds in program order -- and a lane's rank is the counter before the round plus the
// peers below it.  The waves' counters are then summed in wave order on top of the scanned base.  Every place goes to the number of
// places that precede it in the stable order, which is below n; the sum is still compared with n before the store (ks_dest).
// k_ks_scatter: 256 lanes, KS_ITEMS index registers and as many (digit, rank) words per lane, 5 KB of LDS.
//
// The order kernel: one lane, one row.  Two 64-byte loads as eight 8-byte words each, first differing limb by byte-swapped xor and
// count-leading-zeros, the difference a signed integer in +-65535.  The inverse is a LOOKUP: the context caches the inverses of
// 0..65535 (2 MB, made on the device at the first call by 65536 lanes of Fermat inversion, no host data and no wait), the entry of |d|
// is negated for a negative difference.  The per-wave batch inversion of ZK_OP_ROW_INV0 would put one inv_xgcd per 64 rows on lane
// 63 while its wave waits (130 us a round, csrc/typed_rows.hip) and carry 9-limb prefix products through twelve shuffled multiplications;
// the table costs one 32-byte load per row from a table that stays in L2, and no multiplication.  The gathered columns run in the
// same launch, out of the record the lane already holds: word selects (ko_word), no second pass over the records.
#include "ctx.hpp"
#include "keyorder.hip.hpp"
#include "op_check.hpp"

namespace zk {

struct KsState { unsigned long long vary; };                           // scratch: the bytes at which some record differs from record 0
constexpr size_t KS_STATE_BYTES = 256;

struct KsArgs {
    const uint8_t* keys;
    uint64_t n, tiles;
    uint32_t* buf[2];                   // the permutation, alternately
    uint32_t* counts;                   // [256][tiles]
    uint32_t* bin_total;                // [256]
    const KsState* state;
    uint64_t keep;                      // the host's mask, bit j = key byte j
};

__device__ __forceinline__ uint64_t ks_shfl_xor64(uint64_t v, int m) {
    return (uint64_t)(uint32_t)__shfl_xor((int)(uint32_t)v, m) | (uint64_t)(uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), m) << 32;
}

__global__ void __launch_bounds__(256) k_ks_init(const uint8_t* keys, uint64_t n, uint32_t* buf0, KsState* state) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    uint64_t m = 0;
    if (i < n) {
        buf0[i] = (uint32_t)i;
        const uint2* first = (const uint2*)keys;
        const uint2* mine = (const uint2*)(keys + 64 * i);
        uint64_t x[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const uint2 a = mine[k], b = first[k];
            x[k] = (uint64_t)(a.x ^ b.x) | (uint64_t)(a.y ^ b.y) << 32;
        }
        m = ks_vary_bits(x);
    }
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) m |= ks_shfl_xor64(m, off);
    if ((threadIdx.x & 63u) == 0 && m) atomicOr(&state->vary, (unsigned long long)m);
}

__device__ __forceinline__ uint32_t ks_digit(const KsArgs& g, uint32_t idx, uint32_t byte) {
    return idx < g.n ? g.keys[64 * (uint64_t)idx + byte] : 0u;          // an index is below n by construction; nothing else is ever read
}

__global__ void __launch_bounds__(256) k_ks_count(const KsArgs g, uint32_t byte) {
    const uint64_t live = ks_live(g.state->vary, g.keep);
    if (!ks_pass_live(live, byte)) return;
    const uint32_t* src = g.buf[ks_source(live, byte)];
    __shared__ uint32_t hist[KS_BINS];
    hist[threadIdx.x] = 0;
    __syncthreads();
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
#pragma unroll
    for (uint32_t r = 0; r < KS_ITEMS; ++r) {
        const uint64_t pos = ks_pos(blockIdx.x, wave, r, lane);
        if (pos < g.n) atomicAdd(&hist[ks_digit(g, src[pos], byte)], 1u);
    }
    __syncthreads();
    g.counts[ks_count_at(threadIdx.x, blockIdx.x, g.tiles)] = hist[threadIdx.x];
}

// exclusive scan of one value per lane over the 256 lanes of the workgroup; total: the sum of all.  wsum: KS_WAVES words of LDS, free
// again after the call's last barrier.
__device__ __forceinline__ uint32_t ks_block_scan(uint32_t v, uint32_t* wsum, uint32_t& total) {
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    uint32_t inc = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t up = (uint32_t)__shfl_up((int)inc, off);
        if (lane >= (uint32_t)off) inc += up;
    }
    if (lane == 63u) wsum[wave] = inc;
    __syncthreads();
    uint32_t before = 0;
    total = 0;
#pragma unroll
    for (uint32_t w = 0; w < KS_WAVES; ++w) {
        const uint32_t s = wsum[w];
        before += w < wave ? s : 0u;
        total += s;
    }
    __syncthreads();
    return before + inc - v;
}

__global__ void __launch_bounds__(256) k_ks_scan(const KsArgs g, uint32_t byte) {
    const uint64_t live = ks_live(g.state->vary, g.keep);
    if (!ks_pass_live(live, byte)) return;
    __shared__ uint32_t wsum[KS_WAVES];
    const uint32_t bin = blockIdx.x;
    uint32_t carry = 0;
    for (uint64_t t0 = 0; t0 < g.tiles; t0 += 256) {                    // the same trips for every lane
        const uint64_t tile = t0 + threadIdx.x;
        const bool in = tile < g.tiles;
        const uint32_t v = in ? g.counts[ks_count_at(bin, tile, g.tiles)] : 0u;
        uint32_t total;
        const uint32_t excl = ks_block_scan(v, wsum, total);
        if (in) g.counts[ks_count_at(bin, tile, g.tiles)] = carry + excl;
        carry += total;
    }
    if (threadIdx.x == 0) g.bin_total[bin] = carry;
}

__global__ void __launch_bounds__(256) k_ks_scatter(const KsArgs g, uint32_t byte) {
    const uint64_t live = ks_live(g.state->vary, g.keep);
    if (!ks_pass_live(live, byte)) return;
    const uint32_t from = ks_source(live, byte);
    const uint32_t* src = g.buf[from];
    uint32_t* dst = g.buf[from ^ 1u];
    __shared__ uint32_t wsum[KS_WAVES];
    __shared__ uint32_t wcnt[KS_WAVES][KS_BINS];
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    // lane = bin: records with a smaller digit anywhere, and with this digit in earlier tiles
    uint32_t all;
    const uint32_t bin_base = ks_block_scan(g.bin_total[threadIdx.x], wsum, all);
    const uint32_t tile_base = g.counts[ks_count_at(threadIdx.x, blockIdx.x, g.tiles)];
#pragma unroll
    for (uint32_t w = 0; w < KS_WAVES; ++w) wcnt[w][threadIdx.x] = 0;
    __syncthreads();
    uint32_t idx[KS_ITEMS], key[KS_ITEMS];                              // key: digit | rank inside the wave << 8
#pragma unroll
    for (uint32_t r = 0; r < KS_ITEMS; ++r) {
        const uint64_t pos = ks_pos(blockIdx.x, wave, r, lane);
        const bool valid = pos < g.n;
        idx[r] = valid ? src[pos] : 0u;
        const uint32_t digit = valid ? ks_digit(g, idx[r], byte) : 0u;
        uint64_t ballot[8];
#pragma unroll
        for (int b = 0; b < 8; ++b) ballot[b] = __ballot(valid && (digit >> b & 1));
        const uint64_t peers = ks_peers(ballot, __ballot(valid), digit);
        const uint32_t leader = ks_leader(peers);
        uint32_t prior = 0;
        if (valid && lane == leader) {                                  // one lane per digit of the wave
            prior = wcnt[wave][digit];
            wcnt[wave][digit] = prior + ks_popc64(peers);
        }
        prior = (uint32_t)__shfl((int)prior, (int)leader);
        key[r] = digit | (prior + ks_rank_below(peers, lane)) << 8;
        __builtin_amdgcn_wave_barrier();                                // the next round's reads of wcnt stay behind this round's writes
    }
    __syncthreads();
    {   // lane = bin: the waves' counts become their bases, in wave order
        uint32_t run = 0;
#pragma unroll
        for (uint32_t w = 0; w < KS_WAVES; ++w) {
            const uint32_t c = wcnt[w][threadIdx.x];
            wcnt[w][threadIdx.x] = run;
            run += c;
        }
    }
    __shared__ uint32_t base[2][KS_BINS];
    base[0][threadIdx.x] = bin_base;
    base[1][threadIdx.x] = tile_base;
    __syncthreads();
#pragma unroll
    for (uint32_t r = 0; r < KS_ITEMS; ++r) {
        const uint64_t pos = ks_pos(blockIdx.x, wave, r, lane);
        const uint32_t digit = key[r] & 0xffu;
        const uint64_t dest = ks_dest(base[0][digit], base[1][digit], wcnt[wave][digit], key[r] >> 8);
        if (pos < g.n && dest < g.n) dst[dest] = idx[r];
    }
}

__global__ void __launch_bounds__(256) k_ks_finish(const KsArgs g, uint32_t* out, uint8_t* sorted) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= g.n) return;
    const uint32_t idx = g.buf[ks_result(ks_live(g.state->vary, g.keep))][i];
    out[i] = idx;
    if (sorted && idx < g.n) {
        const uint2* from = (const uint2*)(g.keys + 64 * (uint64_t)idx);
        uint2* to = (uint2*)(sorted + 64 * i);
        uint2 v[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = from[k];
#pragma unroll
        for (int k = 0; k < 8; ++k) to[k] = v[k];
    }
}

// h_mask: NULL or 64 bytes in host memory.  Everything is validated before n is looked at and before the first launch.
int key_sort_run(zk_ctx* ctx, const zk_key_sort* desc, const void* h_mask, void* d_out, uint64_t n) {
    if (desc->flags) return ctx->fail(ZK_ERR_INVALID_ARG, "key sort: flags 0x%x: must be 0", desc->flags);
    if (!desc->d_keys || !d_out) return ctx->fail(ZK_ERR_INVALID_ARG, "key sort: NULL d_keys or d_out");
    if ((uintptr_t)desc->d_keys % 8 || (uintptr_t)desc->d_sorted % 8) return ctx->fail(ZK_ERR_INVALID_ARG, "key sort: records at an address that is no multiple of 8");
    if ((uintptr_t)d_out % 4) return ctx->fail(ZK_ERR_INVALID_ARG, "key sort: d_out at an address that is no multiple of 4");
    if (n >> 32) return ctx->fail(ZK_ERR_INVALID_ARG, "key sort: %llu records: 2^32 or more", (unsigned long long)n);
    if (desc->d_sorted == desc->d_keys) return ctx->fail(ZK_ERR_INVALID_ARG, "key sort: d_sorted is d_keys");
    SpanList<3> spans;
    spans.add(d_out, n * 4, "d_out", true);
    spans.add(desc->d_sorted, n * 64, "d_sorted", true);
    spans.add(desc->d_keys, n * 64, "d_keys", false);
    const char *what, *other;
    if (spans.overlap(&what, &other)) return ctx->fail(ZK_ERR_INVALID_ARG, "key sort: %s overlaps %s", what, other);
    if (!n) return ZK_OK;

    uint64_t keep = 0;
    for (int j = 0; j < 64; ++j) keep |= (uint64_t)(!h_mask || ((const uint8_t*)h_mask)[j] != 0) << j;
    KsArgs g;
    memset(&g, 0, sizeof g);
    g.keys = (const uint8_t*)desc->d_keys;
    g.n = n;
    g.tiles = ks_tiles(n);
    g.keep = keep;
    // scratch: state | bin totals | counts [256][tiles] | two permutation buffers
    const size_t totals_at = KS_STATE_BYTES, counts_at = totals_at + KS_BINS * 4, buf_at = (counts_at + (size_t)KS_BINS * g.tiles * 4 + 255) & ~(size_t)255;
    const size_t buf_bytes = ((size_t)n * 4 + 255) & ~(size_t)255;
    uint8_t* s = (uint8_t*)ctx->get_scratch(SC_KEYSORT, buf_at + 2 * buf_bytes);
    if (!s) return ZK_ERR_OOM;
    g.state = (const KsState*)s;
    g.bin_total = (uint32_t*)(s + totals_at);
    g.counts = (uint32_t*)(s + counts_at);
    g.buf[0] = (uint32_t*)(s + buf_at);
    g.buf[1] = (uint32_t*)(s + buf_at + buf_bytes);

    uint32_t passes = 0;
    for (int j = 0; j < 64; ++j) passes += (uint32_t)(keep >> j & 1);
    ZkProfScope prof(ctx, "key_sort");
    // init 64 + 4, every kept byte's pass (count 4 + 1, scatter 4 + 1 + 4; the host cannot know which are dead), finish 4 + 4 (+ 64 + 64)
    prof.bytes = n * (68 + 14ull * passes + 8 + (desc->d_sorted ? 128 : 0));
    const dim3 rows((unsigned)((n + 255) / 256)), tiles((unsigned)g.tiles), t(256);
    ZK_HIP(ctx, hipMemsetAsync(s, 0, KS_STATE_BYTES, ctx->stream));
    hipLaunchKernelGGL(k_ks_init, rows, t, 0, ctx->stream, g.keys, n, g.buf[0], (KsState*)s);
    for (int byte = 63; byte >= 0; --byte) {
        if (!(keep >> byte & 1)) continue;
        hipLaunchKernelGGL(k_ks_count, tiles, t, 0, ctx->stream, g, (uint32_t)byte);
        hipLaunchKernelGGL(k_ks_scan, dim3(KS_BINS), t, 0, ctx->stream, g, (uint32_t)byte);
        hipLaunchKernelGGL(k_ks_scatter, tiles, t, 0, ctx->stream, g, (uint32_t)byte);
    }
    hipLaunchKernelGGL(k_ks_finish, rows, t, 0, ctx->stream, g, (uint32_t*)d_out, (uint8_t*)desc->d_sorted);
    ZK_CHECK_LAUNCH(ctx);
    return ZK_OK;
}

// ---- ZK_OP_KEY_ORDER ----------------------------------------------------------------------------------------------------------------------
constexpr uint32_t KO_MAX_COLS = 64, KO_TABLE = 65536;

struct KoArgs {
    const uint8_t* keys;
    const uint32_t* perm;               // NULL: row i is record i
    Fr* inv;                            // d_out
    Fr* diff;
    uint8_t* index;
    uint8_t* bits;
    uint8_t* not_first;
    const Fr* table;                    // 1 / a for a < 65536, 0 for a = 0
    uint64_t n;
    uint32_t group_limbs, count;
    void* col[KO_MAX_COLS];
    uint32_t cell[KO_MAX_COLS];         // offset | width << 8: whole words, which a scalar load can index
};
static_assert(sizeof(KoArgs) < 4096 - 64, "kernel argument size");

__global__ void __launch_bounds__(256) k_key_inv_table(Fr* table) {
    const uint32_t a = blockIdx.x * 256 + threadIdx.x;
    if (a < KO_TABLE) stg(table + a, key_inv_entry(a));
}

__device__ __forceinline__ void ko_load(const uint8_t* keys, uint64_t idx, bool ok, uint32_t (&r)[16]) {
    const uint2* p = (const uint2*)(keys + 64 * idx);
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const uint2 v = ok ? p[k] : make_uint2(0, 0);
        r[2 * k] = v.x;
        r[2 * k + 1] = v.y;
    }
}

__global__ void __launch_bounds__(256) k_key_order(const KoArgs g) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= g.n) return;
    const uint64_t own = g.perm ? g.perm[i] : i, before = i ? (g.perm ? g.perm[i - 1] : i - 1) : 0;
    const bool own_ok = own < g.n, pair = i && own_ok && before < g.n;
    uint32_t cur[16], prev[16];
    ko_load(g.keys, own, own_ok, cur);
    ko_load(g.keys, before, pair, prev);
    uint64_t c8[8], p8[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        c8[k] = (uint64_t)cur[2 * k] | (uint64_t)cur[2 * k + 1] << 32;
        p8[k] = (uint64_t)prev[2 * k] | (uint64_t)prev[2 * k + 1] << 32;
    }
    int32_t d;
    uint32_t j = key_first_diff(c8, p8, d);
    if (!pair) { j = 0; d = 0; }                                        // row 0, and a row without a record or a predecessor: zeros
    const uint32_t a = d < 0 ? (uint32_t)(-d) : (uint32_t)d;            // at most 65535
    stg(g.inv + i, key_inv_signed(ldg(g.table + a), d));
    if (g.diff) stg(g.diff + i, key_diff_fr(d));
    if (g.index) g.index[i] = (uint8_t)j;
    if (g.bits) {
#pragma unroll
        for (uint32_t b = 0; b < 5; ++b) g.bits[b * g.n + i] = (uint8_t)(j >> (4 - b) & 1);
    }
    if (g.not_first) g.not_first[i] = (uint8_t)(pair && j >= g.group_limbs);
    for (uint32_t c = 0; c < g.count; ++c) {                            // uniform: the table is a kernel argument
        const uint32_t width = g.cell[c] >> 8;
        const uint32_t v = key_gather(cur, g.cell[c] & 0xffu, width);   // a row without a record holds zeros
        if (width == 1) ((uint8_t*)g.col[c])[i] = (uint8_t)v;
        else if (width == 2) ((uint16_t*)g.col[c])[i] = (uint16_t)v;
        else ((uint32_t*)g.col[c])[i] = v;
    }
}

static int key_inv_table(zk_ctx* ctx, const Fr** out) {
    if (!ctx->key_inv_tab) {
        void* d = nullptr;
        ZK_HIP(ctx, hipMalloc(&d, sizeof(Fr) * KO_TABLE));
        hipLaunchKernelGGL(k_key_inv_table, dim3(KO_TABLE / 256), dim3(256), 0, ctx->stream, (Fr*)d);
        if (hipGetLastError() != hipSuccess) { (void)hipFree(d); return ctx->fail(ZK_ERR_HIP, "key order: the table of inverses could not be launched"); }
        ctx->key_inv_tab = d;                                           // every later user is ordered behind the launch on ctx->stream
    }
    *out = (const Fr*)ctx->key_inv_tab;
    return ZK_OK;
}

int key_order_run(zk_ctx* ctx, const zk_key_order* desc, void* d_out, uint64_t n) {
    if (desc->flags) return ctx->fail(ZK_ERR_INVALID_ARG, "key order: flags 0x%x: must be 0", desc->flags);
    if (!desc->d_keys || !d_out) return ctx->fail(ZK_ERR_INVALID_ARG, "key order: NULL d_keys or d_out");
    if ((uintptr_t)desc->d_keys % 8) return ctx->fail(ZK_ERR_INVALID_ARG, "key order: records at an address that is no multiple of 8");
    if ((uintptr_t)desc->d_perm % 4) return ctx->fail(ZK_ERR_INVALID_ARG, "key order: d_perm at an address that is no multiple of 4");
    if ((uintptr_t)d_out % 16 || (uintptr_t)desc->d_diff % 16) return ctx->fail(ZK_ERR_INVALID_ARG, "key order: an Fr output at an address that is no multiple of 16");
    if (n >> 32) return ctx->fail(ZK_ERR_INVALID_ARG, "key order: %llu rows: 2^32 or more", (unsigned long long)n);
    if (desc->group_limbs > 32) return ctx->fail(ZK_ERR_INVALID_ARG, "key order: group_limbs %u: at most 32", desc->group_limbs);
    if (desc->count > KO_MAX_COLS) return ctx->fail(ZK_ERR_INVALID_ARG, "key order: %u gathered columns: at most 64", desc->count);
    if (desc->count && (!desc->cols || !desc->d_cols)) return ctx->fail(ZK_ERR_INVALID_ARG, "key order: NULL cols or d_cols with %u columns", desc->count);
    SpanList<7 + KO_MAX_COLS> spans;
    spans.add(d_out, n * sizeof(Fr), "d_out", true);
    spans.add(desc->d_diff, n * sizeof(Fr), "d_diff", true);
    spans.add(desc->d_index, n, "d_index", true);
    spans.add(desc->d_bits, 5 * n, "d_bits", true);
    spans.add(desc->d_not_first, n, "d_not_first", true);
    uint64_t col_bytes = 0;
    for (uint32_t c = 0; c < desc->count; ++c) {
        const uint32_t offset = desc->cols[c].offset, width = desc->cols[c].width;
        if (!key_col_ok(offset, width)) return ctx->fail(ZK_ERR_INVALID_ARG, "key order: column %u: key bytes [%u, %u + %u): width 1, 2 or 4 inside the 64 bytes", c, offset, offset, width);
        if (!desc->d_cols[c]) return ctx->fail(ZK_ERR_INVALID_ARG, "key order: column %u: NULL", c);
        if ((uintptr_t)desc->d_cols[c] % typed_cell_align(width)) return ctx->fail(ZK_ERR_INVALID_ARG, "key order: column %u: cells of %u bytes at a misaligned address", c, width);
        spans.add(desc->d_cols[c], n * width, "a gathered column", true);
        col_bytes += width;
    }
    spans.add(desc->d_keys, n * 64, "d_keys", false);
    spans.add(desc->d_perm, n * 4, "d_perm", false);
    const char *what, *other;
    if (spans.overlap(&what, &other)) return ctx->fail(ZK_ERR_INVALID_ARG, "key order: %s overlaps %s", what, other);
    if (!n) return ZK_OK;

    KoArgs g;
    memset(&g, 0, sizeof g);
    if (int e = key_inv_table(ctx, &g.table)) return e;
    g.keys = (const uint8_t*)desc->d_keys;
    g.perm = (const uint32_t*)desc->d_perm;
    g.inv = (Fr*)d_out;
    g.diff = (Fr*)desc->d_diff;
    g.index = (uint8_t*)desc->d_index;
    g.bits = (uint8_t*)desc->d_bits;
    g.not_first = (uint8_t*)desc->d_not_first;
    g.n = n;
    g.group_limbs = desc->group_limbs;
    g.count = desc->count;
    for (uint32_t c = 0; c < desc->count; ++c) {
        g.col[c] = desc->d_cols[c];
        g.cell[c] = desc->cols[c].offset | (uint32_t)desc->cols[c].width << 8;
    }
    ZkProfScope prof(ctx, "key_order");
    // two records, the table entry and the inverse; the permutation twice; the optional outputs; the gathered cells
    prof.bytes = n * (128 + 32 + 32 + (g.perm ? 8 : 0) + (g.diff ? 32 : 0) + (g.index ? 1 : 0) + (g.bits ? 5 : 0) + (g.not_first ? 1 : 0) + col_bytes);
    hipLaunchKernelGGL(k_key_order, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, g);
    ZK_CHECK_LAUNCH(ctx);
    return ZK_OK;
}

}  // namespace zk

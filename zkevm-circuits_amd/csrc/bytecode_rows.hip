// ZK_OP_BYTECODE_ROWS of zk_field_vec_op: the rows of the bytecode circuit (bytecode_circuit/bytecode_unroller.rs, circuit.rs
// assign_bytecode) from code bytes that live on the device -- tag, index, value, length, is_code, push_data_left, push_data_size, the
// code hash on every row, and the two kind columns from which ZK_OP_SCAN_RLC and ZK_OP_SCAN_RLC_REV make push_acc and push_rlc.  The
// row logic and the parallel form of push_data_left are csrc/bytecode_rows.hip.hpp, which the host compiles too.
//
// The work is laid out in ROW space, which the host knows (n), not in bytecode space, which it does not: no lane walks a bytecode.
//   k_bc_widths     w[b] = min(L_b + 1, n) for the first m = min(count, n) entries, w[m] = 0
//   scan            exclusive, saturating at n, in place: per 2048 entries a reduce, the sums scanned the same way (recursion on the
//                   host, three levels at 2^32 entries), then a down pass -> start[0 .. m], start[m] = the rows in use
//   k_bc_tile_map   (only with a state output) a workgroup takes BC_TILE = 1024 rows, lane l the rows 4 l .. 4 l + 3: one search of
//                   start per tile for its first and last row, a search per lane inside that window, the bytes as dwords, next
//                   landing rows into LDS, ten rounds of pointer doubling, the 33-byte exit map of the tile
//   k_bc_compose    one wave per node of a level: lane s < 33 carries state s through its 64 children in order (the children's maps
//                   in LDS: 64 dependent LDS reads, the only serial part, independent of the lengths) and stores per child the map
//                   "state entering the node -> state entering the child", and the node's own map.  Levels until one node is left.
//   k_bc_rows       the same tile again: its entry state by one lookup per level from the root, the landing rows marked from the
//                   first one along the doubled pointers, the data rows filled from their opcode row, every output written: 1-byte
//                   columns packed in LDS and stored as aligned dwords with head and tail bytes, 4-byte cells and the code hash
//                   straight.  <false, ..>: no state output, no LDS marking; <.., false>: no output reads d_bytes.
// No atomics decide a value (one LDS atomicMin finds the first reset row of a tile: a minimum has no order), no host wait.
#include "bytecode_rows.hip.hpp"
#include "ctx.hpp"
#include "op_check.hpp"

namespace zk {

struct BcArgs {
    const uint8_t* bytes;
    uint64_t total;
    const void* offs;
    const void* lens;
    const uint8_t* hashes;              // 8-byte aligned
    uint8_t *tag, *is_code, *left, *size, *acc, *rlc;
    uint32_t *index, *value, *length;
    Fr* out;
    const uint32_t* starts;             // m + 1 entries
    uint8_t* maps;                      // level 0: the tiles' exit maps
    const uint8_t* prefix[BC_MAX_LEVELS];   // per level, per node: state entering its parent -> state entering the node
    uint32_t m, n, index_width, levels;
    Fr empty;
};

__device__ __forceinline__ void bc_entry(const BcArgs& g, uint32_t b, uint64_t& off, uint64_t& len) {
    if (g.index_width == 4) { off = ((const uint32_t*)g.offs)[b]; len = ((const uint32_t*)g.lens)[b]; }
    else { off = ((const uint64_t*)g.offs)[b]; len = ((const uint64_t*)g.lens)[b]; }
    if (!bc_entry_ok(off, len, g.total)) off = 0, len = 0;
}

__global__ void __launch_bounds__(256) k_bc_widths(const BcArgs g, uint32_t* w) {
    const uint64_t b = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (b > g.m) return;
    uint32_t rows = 0;
    if (b < g.m) {
        uint64_t off, len;
        bc_entry(g, (uint32_t)b, off, len);
        rows = bc_rows_of(len, g.n);
    }
    w[b] = rows;
}

// inclusive scan over the 256 lanes under the saturating sum; excl: the sum of the lanes below; returns the sum of all.  wsum: four
// words of LDS, free again after the call's last barrier.
__device__ __forceinline__ uint32_t bc_block_scan(uint32_t v, uint32_t cap, uint32_t* wsum, uint32_t& excl) {
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    uint32_t inc = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t up = (uint32_t)__shfl_up((int)inc, off);
        if (lane >= (uint32_t)off) inc = bc_sat_add(up, inc, cap);
    }
    const uint32_t below = (uint32_t)__shfl_up((int)inc, 1);
    if (lane == 63u) wsum[wave] = inc;
    __syncthreads();
    uint32_t before = 0, total = 0;
#pragma unroll
    for (uint32_t k = 0; k < BC_LANES / 64; ++k) {
        const uint32_t s = wsum[k];
        before = k < wave ? bc_sat_add(before, s, cap) : before;
        total = bc_sat_add(total, s, cap);
    }
    __syncthreads();
    excl = lane ? bc_sat_add(before, below, cap) : before;
    return total;
}

__global__ void __launch_bounds__(256) k_bc_scan_reduce(const uint32_t* w, uint64_t count, uint32_t* sums, uint32_t cap) {
    __shared__ uint32_t wsum[BC_LANES / 64];
    const uint64_t at = (uint64_t)blockIdx.x * BC_SCAN_TILE + threadIdx.x * BC_SCAN_ITEMS;
    uint32_t s = 0;
#pragma unroll
    for (uint32_t k = 0; k < BC_SCAN_ITEMS; ++k) s = bc_sat_add(s, at + k < count ? w[at + k] : 0u, cap);
    uint32_t excl;
    const uint32_t total = bc_block_scan(s, cap, wsum, excl);
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

// sums: the exclusive sums of the tiles, or NULL where one tile is all there is
__global__ void __launch_bounds__(256) k_bc_scan_down(uint32_t* w, uint64_t count, const uint32_t* sums, uint32_t cap) {
    __shared__ uint32_t wsum[BC_LANES / 64];
    const uint64_t at = (uint64_t)blockIdx.x * BC_SCAN_TILE + threadIdx.x * BC_SCAN_ITEMS;
    uint32_t v[BC_SCAN_ITEMS], s = 0;
#pragma unroll
    for (uint32_t k = 0; k < BC_SCAN_ITEMS; ++k) {
        v[k] = at + k < count ? w[at + k] : 0u;
        s = bc_sat_add(s, v[k], cap);
    }
    uint32_t excl;
    (void)bc_block_scan(s, cap, wsum, excl);
    uint32_t run = bc_sat_add(sums ? sums[blockIdx.x] : 0u, excl, cap);
#pragma unroll
    for (uint32_t k = 0; k < BC_SCAN_ITEMS; ++k) {
        if (at + k < count) w[at + k] = run;
        run = bc_sat_add(run, v[k], cap);
    }
}

// ---- a tile ---------------------------------------------------------------------------------------------------------------------------------
// what a lane knows of its four rows
struct BcLane {
    uint32_t kind[BC_PER_LANE], b[BC_PER_LANE], v[BC_PER_LANE];
    uint64_t p[BC_PER_LANE], len[BC_PER_LANE];
};

// the four bytes at d_bytes + at .. + 3 of which the first `want` (1..4) are wanted and lie inside the buffer: aligned dwords where
// they lie inside the buffer too, single bytes otherwise
__device__ __forceinline__ uint32_t bc_load4(const BcArgs& g, uint64_t at, uint32_t want) {
    const uintptr_t base = (uintptr_t)g.bytes, a = base + at, lo = a & ~(uintptr_t)3, sh = (uint32_t)(a & 3) * 8;
    const uintptr_t last = (a + want - 1) & ~(uintptr_t)3;              // the dword of the last wanted byte
    if (lo >= base && last + 4 <= base + g.total) {
        const uint32_t x = *(const uint32_t*)lo;
        const uint32_t y = last != lo ? *(const uint32_t*)last : 0u;
        return sh ? x >> sh | y << (32 - sh) : x;
    }
    uint32_t r = 0;
#pragma unroll
    for (uint32_t k = 0; k < 4; ++k)
        if (k < want) r |= (uint32_t)g.bytes[at + k] << (8 * k);
    return r;
}

// BYTES: the byte values are loaded
template <bool BYTES>
__device__ __forceinline__ void bc_load_lane(const BcArgs& g, uint32_t r0, BcLane& t) {
    // one search per tile for its first and its last row, the lane's search inside that window
    const uint32_t tile_last = g.n - r0 > BC_TILE ? r0 + BC_TILE - 1 : g.n - 1;
    const uint32_t b_lo = bc_find(g.starts, 0, g.m, r0), b_hi = bc_find(g.starts, b_lo, g.m, tile_last);
    const uint32_t row0 = r0 + threadIdx.x * BC_PER_LANE;
    uint32_t b = 0, start = 0;
    uint64_t off = 0, len = 0;
    bool have = false;
#pragma unroll
    for (uint32_t k = 0; k < BC_PER_LANE; ++k) {
        const uint32_t row = row0 + k;
        t.kind[k] = BC_PAD, t.b[k] = g.m, t.v[k] = 0, t.p[k] = 0, t.len[k] = 0;
        if (row >= g.n) continue;                                       // a row that is not written: padding, which resets
        if (!have) { b = bc_find(g.starts, b_lo, b_hi, row); have = true; start = g.starts[b]; if (b < g.m) bc_entry(g, b, off, len); }
        else if (b < g.m && row >= g.starts[b + 1]) { ++b; start = g.starts[b]; if (b < g.m) bc_entry(g, b, off, len); }
        if (b >= g.m) continue;
        t.b[k] = b;
        t.len[k] = len;
        t.kind[k] = row == start ? BC_HEADER : BC_BYTE;
        t.p[k] = row == start ? 0 : (uint64_t)(row - start) - 1;
    }
    if (!BYTES) return;
    // the byte rows of one bytecode that follow each other in this lane share a load
#pragma unroll
    for (uint32_t k = 0; k < BC_PER_LANE; ++k) {
        if (t.kind[k] != BC_BYTE) continue;
        if (k && t.kind[k - 1] == BC_BYTE && t.b[k - 1] == t.b[k]) continue;   // loaded with the row before
        uint32_t want = 1;
#pragma unroll
        for (uint32_t j = k + 1; j < BC_PER_LANE; ++j) want += (uint32_t)(j == k + want && t.kind[j] == BC_BYTE && t.b[j] == t.b[k]);
        uint64_t o, l;
        bc_entry(g, t.b[k], o, l);
        const uint32_t word = bc_load4(g, o + t.p[k], want);
#pragma unroll
        for (uint32_t j = 0; j < BC_PER_LANE; ++j)
            if (j >= k && j < k + want) t.v[j] = word >> (8 * (j - k)) & 0xffu;
    }
}

// next landing rows of the lane's rows into jump, the first reset row of the tile into *h0 (set to BC_TILE before)
__device__ __forceinline__ void bc_put_next(const BcLane& t, uint16_t* jump, uint32_t* h0) {
#pragma unroll
    for (uint32_t k = 0; k < BC_PER_LANE; ++k) {
        const uint32_t i = threadIdx.x * BC_PER_LANE + k;
        jump[i] = (uint16_t)bc_next(i, t.kind[k], t.v[k], t.len[k] - t.p[k]);
        if (t.kind[k] != BC_BYTE) atomicMin(h0, i);
    }
}

__global__ void __launch_bounds__(256) k_bc_tile_map(const BcArgs g) {
    __shared__ uint16_t jump[2][BC_TILE];
    __shared__ uint32_t h0;
    const uint32_t r0 = blockIdx.x * BC_TILE;
    if (threadIdx.x == 0) h0 = BC_TILE;
    __syncthreads();
    BcLane t;
    bc_load_lane<true>(g, r0, t);
    bc_put_next(t, jump[0], &h0);
    __syncthreads();
    uint32_t cur = 0;
    for (uint32_t round = 0; round < BC_TILE_LOG2; ++round) {
#pragma unroll
        for (uint32_t k = 0; k < BC_PER_LANE; ++k) {
            const uint32_t i = threadIdx.x * BC_PER_LANE + k;
            jump[cur ^ 1][i] = (uint16_t)bc_jump_twice(jump[cur], i);
        }
        __syncthreads();
        cur ^= 1;
    }
    if (threadIdx.x < BC_STATES)
        g.maps[(uint64_t)blockIdx.x * BC_MAP_STRIDE + threadIdx.x] = (uint8_t)bc_exit_state(jump[cur][bc_first_landing(threadIdx.x, h0)]);
}

// one wave per node: children [BC_FAN node, BC_FAN node + BC_FAN) of `count` maps below
__global__ void __launch_bounds__(64) k_bc_compose(const uint8_t* child, uint64_t count, uint8_t* prefix, uint8_t* parent) {
    __shared__ uint32_t maps[BC_FAN * BC_MAP_STRIDE / 4];
    const uint64_t first = (uint64_t)blockIdx.x * BC_FAN;
    const uint32_t have = count - first < BC_FAN ? (uint32_t)(count - first) : BC_FAN;
    const uint32_t* src = (const uint32_t*)(child + first * BC_MAP_STRIDE);
    for (uint32_t i = threadIdx.x; i < have * (BC_MAP_STRIDE / 4); i += 64) maps[i] = src[i];
    __syncthreads();
    if (threadIdx.x >= BC_STATES) return;
    uint32_t s = threadIdx.x;
    for (uint32_t c = 0; c < have; ++c) {
        prefix[(first + c) * BC_MAP_STRIDE + threadIdx.x] = (uint8_t)s;
        s = bc_apply((const uint8_t*)maps + c * BC_MAP_STRIDE, s);
    }
    parent[(uint64_t)blockIdx.x * BC_MAP_STRIDE + threadIdx.x] = (uint8_t)s;
}

// rows [r0, r0 + rows) of a 1-byte column from the tile's packed bytes in LDS (st: BC_TILE / 4 + 1 words): bytes up to the first
// address that is a multiple of 4, dwords, bytes again
__device__ __forceinline__ void bc_store_col(uint8_t* col, const uint32_t* st, uint32_t r0, uint32_t rows) {
    if (!col) return;
    uint8_t* p = col + r0;
    const uint8_t* sb = (const uint8_t*)st;
    uint32_t head = (uint32_t)(-(uintptr_t)p & 3);
    head = head < rows ? head : rows;
    if (threadIdx.x < head) p[threadIdx.x] = sb[threadIdx.x];
    const uint32_t body = (rows - head) >> 2;
    if (threadIdx.x < body) {                                           // body <= BC_LANES
        const uint32_t o = head + 4 * threadIdx.x, sh = (o & 3) * 8;
        const uint32_t lo = st[o >> 2], hi = st[(o >> 2) + 1];
        ((uint32_t*)(p + head))[threadIdx.x] = sh ? lo >> sh | hi << (32 - sh) : lo;
    }
    const uint32_t done = head + 4 * body;
    if (threadIdx.x < rows - done) p[done + threadIdx.x] = sb[done + threadIdx.x];
}

template <bool STATE, bool BYTES>
__global__ void __launch_bounds__(256) k_bc_rows(const BcArgs g) {
    constexpr uint32_t COLS = 6, ST = BC_TILE / 4 + 1;
    __shared__ uint32_t stage[COLS][ST];
    __shared__ uint32_t rowb[BC_TILE];
    __shared__ uint16_t jump[STATE ? 2 : 1][STATE ? BC_TILE : 1];
    __shared__ uint32_t mark[STATE ? BC_TILE / 4 : 1], left[STATE ? BC_TILE / 4 : 1];
    __shared__ uint32_t h0;
    const uint32_t r0 = blockIdx.x * BC_TILE;
    const uint32_t rows = g.n - r0 < BC_TILE ? g.n - r0 : BC_TILE;
    if (threadIdx.x == 0) h0 = BC_TILE;
    if (threadIdx.x < COLS) stage[threadIdx.x][ST - 1] = 0;
    __syncthreads();
    BcLane t;
    bc_load_lane<BYTES>(g, r0, t);
    uint32_t s4 = 0;                                                    // push_data_left of the lane's rows, a byte each
    if (STATE) {
        // the state that enters the tile: the root is entered with 0, one lookup per level down
        uint32_t entry = 0;
        for (uint32_t l = g.levels; l-- > 0;) entry = bc_apply(g.prefix[l] + bc_node(blockIdx.x, l) * BC_MAP_STRIDE, entry);
        bc_put_next(t, jump[0], &h0);
        __syncthreads();
        const uint32_t c0 = bc_first_landing(entry, h0);
        uint32_t m4 = 0, l4 = 0;
#pragma unroll
        for (uint32_t k = 0; k < BC_PER_LANE; ++k) {
            const uint32_t i = threadIdx.x * BC_PER_LANE + k;
            m4 |= (uint32_t)(i == c0) << (8 * k);
            l4 |= (i < c0 ? entry - i : 0u) << (8 * k);                 // the data rows of an instruction that began in an earlier tile
        }
        mark[threadIdx.x] = m4;
        left[threadIdx.x] = l4;
        __syncthreads();
        uint8_t* mk = (uint8_t*)mark;
        uint32_t cur = 0;
        for (uint32_t round = 0; round < BC_TILE_LOG2; ++round) {
            const uint32_t mine = mark[threadIdx.x];
            uint32_t to[BC_PER_LANE], twice[BC_PER_LANE];
#pragma unroll
            for (uint32_t k = 0; k < BC_PER_LANE; ++k) {
                const uint32_t i = threadIdx.x * BC_PER_LANE + k;
                to[k] = jump[cur][i];
                twice[k] = bc_jump_twice(jump[cur], i);
            }
            __syncthreads();
#pragma unroll
            for (uint32_t k = 0; k < BC_PER_LANE; ++k) {
                const uint32_t i = threadIdx.x * BC_PER_LANE + k;
                if ((mine >> (8 * k) & 0xffu) && to[k] < BC_TILE) mk[to[k]] = 1;
                jump[cur ^ 1][i] = (uint16_t)twice[k];
            }
            __syncthreads();
            cur ^= 1;
        }
        // a landing row with a push fills in the rows of its data, up to the next reset row and the end of the tile
        const uint32_t mine = mark[threadIdx.x];
        uint8_t* lf = (uint8_t*)left;
#pragma unroll
        for (uint32_t k = 0; k < BC_PER_LANE; ++k) {
            const uint32_t i = threadIdx.x * BC_PER_LANE + k;
            if (!(mine >> (8 * k) & 0xffu) || t.kind[k] != BC_BYTE) continue;
            const uint32_t size = bc_push_size(t.v[k]);
            const uint64_t room = t.len[k] - t.p[k] - 1;               // byte rows of this bytecode behind this one
            const uint32_t fill = size < room ? size : (uint32_t)room;
            for (uint32_t d = 1; d <= fill && i + d < BC_TILE; ++d) lf[i + d] = (uint8_t)(size - d + 1);
        }
        __syncthreads();
        s4 = left[threadIdx.x];
    }
    // the rows
    uint32_t pk[COLS] = {0, 0, 0, 0, 0, 0}, idx[BC_PER_LANE], val[BC_PER_LANE], len[BC_PER_LANE];
#pragma unroll
    for (uint32_t k = 0; k < BC_PER_LANE; ++k) {
        const BcRow r = bc_row(t.kind[k], t.p[k], t.len[k], t.v[k], s4 >> (8 * k) & 0xffu);
        pk[0] |= (uint32_t)r.tag << (8 * k);
        pk[1] |= (uint32_t)r.is_code << (8 * k);
        pk[2] |= (uint32_t)r.push_data_left << (8 * k);
        pk[3] |= (uint32_t)r.push_data_size << (8 * k);
        pk[4] |= (uint32_t)r.acc_kind << (8 * k);
        pk[5] |= (uint32_t)r.rlc_kind << (8 * k);
        idx[k] = r.index, val[k] = r.value, len[k] = r.length;
        rowb[threadIdx.x * BC_PER_LANE + k] = t.b[k];
    }
#pragma unroll
    for (uint32_t c = 0; c < COLS; ++c) stage[c][threadIdx.x] = pk[c];
    __syncthreads();
    bc_store_col(g.tag, stage[0], r0, rows);
    bc_store_col(g.is_code, stage[1], r0, rows);
    bc_store_col(g.left, stage[2], r0, rows);
    bc_store_col(g.size, stage[3], r0, rows);
    bc_store_col(g.acc, stage[4], r0, rows);
    bc_store_col(g.rlc, stage[5], r0, rows);
#pragma unroll
    for (uint32_t k = 0; k < BC_PER_LANE; ++k) {
        const uint32_t i = threadIdx.x * BC_PER_LANE + k;
        if (i >= rows) continue;
        if (g.index) g.index[r0 + i] = idx[k];
        if (g.value) g.value[r0 + i] = val[k];
        if (g.length) g.length[r0 + i] = len[k];
    }
    // the code hash: consecutive lanes on consecutive rows
#pragma unroll
    for (uint32_t k = 0; k < BC_PER_LANE; ++k) {
        const uint32_t i = k * BC_LANES + threadIdx.x;
        if (i >= rows) continue;
        const uint32_t b = rowb[i];
        Fr h = g.empty;
        if (b < g.m) {
            h = Fr::zero();
            if (g.hashes) {
                const uint2* q = (const uint2*)(g.hashes + 32 * (uint64_t)b);
#pragma unroll
                for (int j = 0; j < 4; ++j) { const uint2 w = q[j]; h.l[2 * j] = w.x; h.l[2 * j + 1] = w.y; }
            }
        }
        stg(g.out + r0 + i, h);
    }
}

// exclusive saturating scan of w[0 .. count) in place; tmp: room for the sums of every level (copy_rows.hip scans its row starts with it too)
void bc_scan(zk_ctx* ctx, uint32_t* w, uint64_t count, uint32_t* tmp, uint32_t cap) {
    const uint64_t tiles = (count + BC_SCAN_TILE - 1) / BC_SCAN_TILE;
    if (tiles <= 1) {
        hipLaunchKernelGGL(k_bc_scan_down, dim3(1), dim3(256), 0, ctx->stream, w, count, (const uint32_t*)nullptr, cap);
        return;
    }
    hipLaunchKernelGGL(k_bc_scan_reduce, dim3((unsigned)tiles), dim3(256), 0, ctx->stream, (const uint32_t*)w, count, tmp, cap);
    bc_scan(ctx, tmp, tiles, tmp + ((tiles + 63) & ~(uint64_t)63), cap);
    hipLaunchKernelGGL(k_bc_scan_down, dim3((unsigned)tiles), dim3(256), 0, ctx->stream, w, count, (const uint32_t*)tmp, cap);
}

// h_empty: one Montgomery Fr in host memory.  Everything is validated before n is looked at and before the first launch.
int bytecode_rows_run(zk_ctx* ctx, const zk_bytecode_rows* desc, const void* h_empty, void* d_out, uint64_t n) {
    const uint32_t iw = desc->index_width;
    if (desc->flags) return ctx->fail(ZK_ERR_INVALID_ARG, "bytecode rows: flags 0x%x: must be 0", desc->flags);
    if (iw != 4 && iw != 8) return ctx->fail(ZK_ERR_INVALID_ARG, "bytecode rows: index width %u: must be 4 or 8 bytes", iw);
    if (desc->count && (!desc->d_offsets || !desc->d_lens)) return ctx->fail(ZK_ERR_INVALID_ARG, "bytecode rows: NULL offsets or lengths with %u bytecodes", desc->count);
    if (desc->count && ((uintptr_t)desc->d_offsets % iw || (uintptr_t)desc->d_lens % iw))
        return ctx->fail(ZK_ERR_INVALID_ARG, "bytecode rows: offsets or lengths of %u bytes at a misaligned address", iw);
    if (!desc->d_bytes && desc->total_bytes) return ctx->fail(ZK_ERR_INVALID_ARG, "bytecode rows: NULL d_bytes with %llu bytes", (unsigned long long)desc->total_bytes);
    if (desc->total_bytes >> 61) return ctx->fail(ZK_ERR_INVALID_ARG, "bytecode rows: %llu bytes: 2^61 or more", (unsigned long long)desc->total_bytes);
    if ((uintptr_t)desc->d_hashes % 8) return ctx->fail(ZK_ERR_INVALID_ARG, "bytecode rows: d_hashes at an address that is no multiple of 8");
    if ((uintptr_t)d_out % 16) return ctx->fail(ZK_ERR_INVALID_ARG, "bytecode rows: d_out at an address that is no multiple of 16");
    if ((uintptr_t)desc->d_index % 4 || (uintptr_t)desc->d_value % 4 || (uintptr_t)desc->d_length % 4)
        return ctx->fail(ZK_ERR_INVALID_ARG, "bytecode rows: d_index, d_value or d_length at an address that is no multiple of 4");
    if (n >> 32) return ctx->fail(ZK_ERR_INVALID_ARG, "bytecode rows: %llu rows: 2^32 or more", (unsigned long long)n);
    SpanList<15> spans;
    spans.add(d_out, n * sizeof(Fr), "d_out", true);
    spans.add(desc->d_tag, n, "d_tag", true);
    spans.add(desc->d_index, n * 4, "d_index", true);
    spans.add(desc->d_value, n * 4, "d_value", true);
    spans.add(desc->d_is_code, n, "d_is_code", true);
    spans.add(desc->d_push_data_left, n, "d_push_data_left", true);
    spans.add(desc->d_push_data_size, n, "d_push_data_size", true);
    spans.add(desc->d_length, n * 4, "d_length", true);
    spans.add(desc->d_acc_kinds, n, "d_acc_kinds", true);
    spans.add(desc->d_rlc_kinds, n, "d_rlc_kinds", true);
    spans.add(desc->d_bytes, desc->total_bytes, "d_bytes", false);
    spans.add(desc->d_offsets, (uint64_t)desc->count * iw, "d_offsets", false);
    spans.add(desc->d_lens, (uint64_t)desc->count * iw, "d_lens", false);
    spans.add(desc->d_hashes, (uint64_t)desc->count * 32, "d_hashes", false);
    const char *what, *other;
    if (spans.overlap(&what, &other)) return ctx->fail(ZK_ERR_INVALID_ARG, "bytecode rows: %s overlaps %s", what, other);
    if (!n) return ZK_OK;

    BcArgs g;
    memset(&g, 0, sizeof g);
    g.bytes = (const uint8_t*)desc->d_bytes;
    g.total = desc->total_bytes;
    g.offs = desc->d_offsets;
    g.lens = desc->d_lens;
    g.hashes = (const uint8_t*)desc->d_hashes;
    g.tag = (uint8_t*)desc->d_tag;
    g.is_code = (uint8_t*)desc->d_is_code;
    g.left = (uint8_t*)desc->d_push_data_left;
    g.size = (uint8_t*)desc->d_push_data_size;
    g.acc = (uint8_t*)desc->d_acc_kinds;
    g.rlc = (uint8_t*)desc->d_rlc_kinds;
    g.index = (uint32_t*)desc->d_index;
    g.value = (uint32_t*)desc->d_value;
    g.length = (uint32_t*)desc->d_length;
    g.out = (Fr*)d_out;
    g.n = (uint32_t)n;
    g.m = desc->count < n ? desc->count : (uint32_t)n;               // a bytecode has at least its header row
    g.index_width = iw;
    memcpy(&g.empty, h_empty, sizeof(Fr));
    const bool state = g.is_code || g.left || g.acc || g.rlc;
    const bool bytes = g.m && (state || g.value || g.size);

    // scratch: start[0 .. m] | the sums of the scan's levels | per level of the hierarchy the nodes' maps and their prefix maps
    const uint64_t tiles = (n + BC_TILE - 1) / BC_TILE;
    const auto pad = [](uint64_t b) { return (b + 255) & ~(uint64_t)255; };
    const uint64_t starts_bytes = pad(((uint64_t)g.m + 1) * 4);
    uint64_t sums_bytes = 0;
    for (uint64_t c = (uint64_t)g.m + 1; c > BC_SCAN_TILE;) { c = (c + BC_SCAN_TILE - 1) / BC_SCAN_TILE; sums_bytes += ((c + 63) & ~(uint64_t)63) * 4; }
    sums_bytes = pad(sums_bytes);
    uint64_t map_at[BC_MAX_LEVELS + 1], prefix_at[BC_MAX_LEVELS], at = starts_bytes + sums_bytes;
    uint32_t levels = 0;
    if (state) {
        for (uint64_t c = tiles;; c = (c + BC_FAN - 1) / BC_FAN) {
            map_at[levels] = at, at += pad(c * BC_MAP_STRIDE);
            if (c == 1) break;
            prefix_at[levels] = at, at += pad(c * BC_MAP_STRIDE);
            ++levels;
        }
    }
    uint8_t* s = (uint8_t*)ctx->get_scratch(SC_BYTECODE, at);
    if (!s) return ZK_ERR_OOM;
    uint32_t* starts = (uint32_t*)s;
    g.starts = starts;
    g.levels = levels;
    g.maps = s + starts_bytes + sums_bytes;
    for (uint32_t l = 0; l < levels; ++l) g.prefix[l] = s + prefix_at[l];

    uint64_t widths = 32 + (g.tag ? 1 : 0) + (g.is_code ? 1 : 0) + (g.left ? 1 : 0) + (g.size ? 1 : 0) + (g.acc ? 1 : 0) + (g.rlc ? 1 : 0);
    widths += (g.index ? 4 : 0) + (g.value ? 4 : 0) + (g.length ? 4 : 0);
    ZkProfScope prof(ctx, "bytecode_rows");
    prof.bytes = (uint64_t)desc->count * (2ull * iw + (g.hashes ? 32 : 0)) + (bytes ? desc->total_bytes : 0) + n * widths;
    const dim3 t(256);
    hipLaunchKernelGGL(k_bc_widths, dim3((unsigned)(((uint64_t)g.m + 1 + 255) / 256)), t, 0, ctx->stream, g, starts);
    bc_scan(ctx, starts, (uint64_t)g.m + 1, (uint32_t*)(s + starts_bytes), g.n);
    if (state && levels) {                                              // one tile is entered with 0 and needs no map
        hipLaunchKernelGGL(k_bc_tile_map, dim3((unsigned)tiles), t, 0, ctx->stream, g);
        uint64_t c = tiles;
        for (uint32_t l = 0; l < levels; ++l, c = (c + BC_FAN - 1) / BC_FAN)
            hipLaunchKernelGGL(k_bc_compose, dim3((unsigned)((c + BC_FAN - 1) / BC_FAN)), dim3(64), 0, ctx->stream, (const uint8_t*)(s + map_at[l]), c, s + prefix_at[l], s + map_at[l + 1]);
    }
    if (state) hipLaunchKernelGGL((k_bc_rows<true, true>), dim3((unsigned)tiles), t, 0, ctx->stream, g);
    else if (bytes) hipLaunchKernelGGL((k_bc_rows<false, true>), dim3((unsigned)tiles), t, 0, ctx->stream, g);
    else hipLaunchKernelGGL((k_bc_rows<false, false>), dim3((unsigned)tiles), t, 0, ctx->stream, g);
    ZK_CHECK_LAUNCH(ctx);
    return ZK_OK;
}

}  // namespace zk

// ZK_OP_CODE_HASH_ROWS and ZK_OP_CODE_HASH_TABLE of zk_field_vec_op: the eight advice columns the Poseidon-hash extension adds to the
// bytecode circuit (bytecode_circuit/circuit/to_poseidon_hash.rs assign_extended_row, set_header_row) and the code-hash rows of the
// PoseidonTable (table.rs PoseidonTable::dev_load) in the shape ZK_OP_POSEIDON reads, both from the code bytes ZK_OP_KECCAK and
// ZK_OP_BYTECODE_ROWS read.  Every row rule is csrc/code_hash_rows.hip.hpp, which the host compiles too.
//
// Both ops work in ROW space, the circuit's rows (L_b + 1 per bytecode) or the table's (ceil(L_b / 62) per bytecode): no lane walks a
// bytecode, and a row is a closed form of its position, so nothing is carried from tile to tile.
//   k_ch_widths     w[b] = the rows of entry b, saturating at n, w[m] = 0; for the table, with d_rows_needed, the unsaturated sum of each
//                   block of 256 entries
//   bc_scan         the exclusive scan of bytecode_rows.hip, saturating at n, in place -> start[0 .. m], start[m] = the rows in use
//   k_ch_total      (only with d_rows_needed) one workgroup adds the block sums: one 8-byte store from one lane
//   k_ch_rows / k_ch_table   a workgroup takes BC_TILE = 1024 rows.  First lane l takes the rows 4 l .. 4 l + 3: one search of start per
//                   tile for its first and last row, one search per lane inside that window, the owner and the position of each row
//                   into LDS, the 1-byte planes packed in LDS and stored as aligned dwords with head and tail bytes.  Then lane l takes
//                   the rows l, l + 256, ..: consecutive lanes on consecutive rows for the wide cells.  A field's bytes come as up to
//                   nine aligned dwords per lane, single bytes at the two ends of a bytecode: nothing outside [off, off + len) is read.
// No atomics, no scratch memory, no host wait.
#include "code_hash_rows.hip.hpp"
#include "ctx.hpp"
#include "op_check.hpp"

namespace zk {

struct alignas(16) ChCell16 { uint64_t lo, hi; };

// the inputs of both ops and the row starts
struct ChIn {
    const uint8_t* bytes;
    uint64_t total;
    const void* offs;
    const void* lens;
    const uint32_t* starts;             // m + 1 entries
    uint32_t m, n, index_width;
};
struct ChRowsArgs {
    ChIn in;
    Fr *field_input, *inv, *shift;
    uint32_t* control;
    uint8_t *index, *border, *field_index, *field_index_inv;
};
struct ChTableArgs {
    ChIn in;
    Fr *in0, *in1;
    ChCell16* control;
    uint64_t* cap;
    uint8_t *mark, *kinds;
};

__device__ __forceinline__ void ch_entry(const ChIn& g, uint32_t b, uint64_t& off, uint64_t& len) {
    if (g.index_width == 4) { off = ((const uint32_t*)g.offs)[b]; len = ((const uint32_t*)g.lens)[b]; }
    else { off = ((const uint64_t*)g.offs)[b]; len = ((const uint64_t*)g.lens)[b]; }
    if (!bc_entry_ok(off, len, g.total)) off = 0, len = 0;
}

// TABLE: the rows of the table, and per block of 256 entries their unsaturated sum (block_rows may be NULL)
template <bool TABLE>
__global__ void __launch_bounds__(256) k_ch_widths(const ChIn g, uint32_t* w, uint64_t* block_rows) {
    __shared__ uint64_t sh[256];
    const uint64_t b = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    uint64_t off = 0, len = 0;
    if (b < g.m) ch_entry(g, (uint32_t)b, off, len);
    if (b <= g.m) w[b] = b < g.m ? (TABLE ? ch_table_rows_of(len, g.n) : bc_rows_of(len, g.n)) : 0u;
    if (!TABLE || !block_rows) return;
    sh[threadIdx.x] = b < g.m ? ch_blocks_of(len) : 0u;                 // at most 2^32 entries of less than 2^61 / 62 blocks
    __syncthreads();
    for (uint32_t d = 128; d; d >>= 1) {
        if (threadIdx.x < d) sh[threadIdx.x] += sh[threadIdx.x + d];
        __syncthreads();
    }
    if (threadIdx.x == 0) block_rows[blockIdx.x] = sh[0];
}
__global__ void __launch_bounds__(256) k_ch_total(const uint64_t* block_rows, uint32_t blocks, uint64_t* rows_needed) {
    __shared__ uint64_t sh[256];
    uint64_t s = 0;
    for (uint32_t i = threadIdx.x; i < blocks; i += 256) s += block_rows[i];
    sh[threadIdx.x] = s;
    __syncthreads();
    for (uint32_t d = 128; d; d >>= 1) {
        if (threadIdx.x < d) sh[threadIdx.x] += sh[threadIdx.x + d];
        __syncthreads();
    }
    if (threadIdx.x == 0) *rows_needed = sh[0];
}

// The owner (g.m: none) and the offset from the owner's first row of the lane's four rows 4 l .. 4 l + 3 of the tile at r0, into
// LDS and into b[], d[]: one search per tile for its first and its last row, the lane's search inside that window.  A row at or
// after n has no owner.
__device__ __forceinline__ void ch_find_lane(const ChIn& g, uint32_t r0, uint32_t* rowb, uint32_t* rowd, uint32_t (&b4)[BC_PER_LANE], uint32_t (&d4)[BC_PER_LANE]) {
    const uint32_t tile_last = g.n - r0 > BC_TILE ? r0 + BC_TILE - 1 : g.n - 1;
    const uint32_t b_lo = bc_find(g.starts, 0, g.m, r0), b_hi = bc_find(g.starts, b_lo, g.m, tile_last);
    const uint32_t row0 = r0 + threadIdx.x * BC_PER_LANE;
    uint32_t b = 0, start = 0;
    bool have = false;
#pragma unroll
    for (uint32_t k = 0; k < BC_PER_LANE; ++k) {
        const uint32_t row = row0 + k;
        b4[k] = g.m, d4[k] = 0;
        if (row < g.n) {
            // the largest b whose rows begin at or before this one: an entry without rows shares its start with the next one
            if (!have) { b = bc_find(g.starts, b_lo, b_hi, row); have = true; start = g.starts[b]; }
            else if (b < b_hi && g.starts[b + 1] <= row) { b = bc_find(g.starts, b + 1, b_hi, row); start = g.starts[b]; }
            if (b < g.m) b4[k] = b, d4[k] = row - start;
        }
        rowb[threadIdx.x * BC_PER_LANE + k] = b4[k];
        rowd[threadIdx.x * BC_PER_LANE + k] = d4[k];
    }
}

// rows [r0, r0 + rows) of a 1-byte column from the tile's packed bytes in LDS (st: BC_TILE / 4 + 1 words): bytes up to the first
// address that is a multiple of 4, dwords, bytes again
__device__ __forceinline__ void ch_store_col(uint8_t* col, const uint32_t* st, uint32_t r0, uint32_t rows) {
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

__global__ void __launch_bounds__(256) k_ch_rows(const ChRowsArgs g) {
    constexpr uint32_t COLS = 4, ST = BC_TILE / 4 + 1;
    __shared__ uint32_t stage[COLS][ST];
    __shared__ uint32_t rowb[BC_TILE], rowd[BC_TILE];
    const uint32_t r0 = blockIdx.x * BC_TILE;
    const uint32_t rows = g.in.n - r0 < BC_TILE ? g.in.n - r0 : BC_TILE;
    if (threadIdx.x < COLS) stage[threadIdx.x][ST - 1] = 0;
    uint32_t b4[BC_PER_LANE], d4[BC_PER_LANE];
    ch_find_lane(g.in, r0, rowb, rowd, b4, d4);
    if (g.index || g.border || g.field_index || g.field_index_inv) {
        uint32_t pk[COLS] = {0, 0, 0, 0};
        uint32_t have = g.in.m;
        uint64_t off = 0, len = 0;
#pragma unroll
        for (uint32_t k = 0; k < BC_PER_LANE; ++k) {
            if (b4[k] < g.in.m && b4[k] != have) { have = b4[k]; ch_entry(g.in, have, off, len); }
            const uint32_t kind = b4[k] >= g.in.m ? BC_PAD : d4[k] ? BC_BYTE : BC_HEADER;
            const ChRow r = ch_row(kind, kind == BC_BYTE ? (uint64_t)d4[k] - 1 : 0, len);
            pk[0] |= (uint32_t)r.bytes_in_field_index << (8 * k);
            pk[1] |= (uint32_t)r.is_field_border << (8 * k);
            pk[2] |= (uint32_t)r.field_index << (8 * k);
            pk[3] |= (uint32_t)r.field_index_inv << (8 * k);
        }
#pragma unroll
        for (uint32_t c = 0; c < COLS; ++c) stage[c][threadIdx.x] = pk[c];
    }
    __syncthreads();
    ch_store_col(g.index, stage[0], r0, rows);
    ch_store_col(g.border, stage[1], r0, rows);
    ch_store_col(g.field_index, stage[2], r0, rows);
    ch_store_col(g.field_index_inv, stage[3], r0, rows);
    // the wide cells: consecutive lanes on consecutive rows
#pragma unroll 1
    for (uint32_t k = 0; k < BC_PER_LANE; ++k) {
        const uint32_t i = k * BC_LANES + threadIdx.x;
        if (i >= rows) continue;
        const uint32_t b = rowb[i], d = rowd[i];
        uint64_t off = 0, len = 0;
        if (b < g.in.m) ch_entry(g.in, b, off, len);
        const uint32_t kind = b >= g.in.m ? BC_PAD : d ? BC_BYTE : BC_HEADER;
        const uint64_t p = kind == BC_BYTE ? (uint64_t)d - 1 : 0;
        const ChRow r = ch_row(kind, p, len);
        if (g.control) g.control[r0 + i] = r.control_length;
        if (g.inv) stg(g.inv + r0 + i, ch_inv_small(r.inv_of));
        if (g.shift) stg(g.shift + r0 + i, ch_pow256(r.shift));
        stg(g.field_input + r0 + i, kind == BC_BYTE ? ch_field_input(g.in.bytes, off, len, p, r.m) : Fr::zero());
    }
}

__global__ void __launch_bounds__(256) k_ch_table(const ChTableArgs g) {
    constexpr uint32_t COLS = 2, ST = BC_TILE / 4 + 1;
    __shared__ uint32_t stage[COLS][ST];
    __shared__ uint32_t rowb[BC_TILE], rowd[BC_TILE];
    const uint32_t r0 = blockIdx.x * BC_TILE;
    const uint32_t rows = g.in.n - r0 < BC_TILE ? g.in.n - r0 : BC_TILE;
    if (threadIdx.x < COLS) stage[threadIdx.x][ST - 1] = 0;
    uint32_t b4[BC_PER_LANE], d4[BC_PER_LANE];
    ch_find_lane(g.in, r0, rowb, rowd, b4, d4);
    uint32_t pk[COLS] = {0, 0};
#pragma unroll
    for (uint32_t k = 0; k < BC_PER_LANE; ++k) {
        const ChTableRow r = ch_table_row(b4[k] < g.in.m, d4[k], 0);   // the two planes do not depend on the length
        pk[0] |= (uint32_t)r.heading_mark << (8 * k);
        pk[1] |= (uint32_t)r.kind << (8 * k);
    }
    stage[0][threadIdx.x] = pk[0];
    stage[1][threadIdx.x] = pk[1];
    __syncthreads();
    ch_store_col(g.mark, stage[0], r0, rows);
    ch_store_col(g.kinds, stage[1], r0, rows);
#pragma unroll 1
    for (uint32_t k = 0; k < BC_PER_LANE; ++k) {
        const uint32_t i = k * BC_LANES + threadIdx.x;
        if (i >= rows) continue;
        const uint32_t b = rowb[i], j = rowd[i];
        const bool owned = b < g.in.m;
        uint64_t off = 0, len = 0;
        if (owned) ch_entry(g.in, b, off, len);
        const ChTableRow r = ch_table_row(owned, j, len);
        if (g.control) g.control[r0 + i] = ChCell16{0, r.control_hi};
        if (g.cap) g.cap[r0 + i] = r.cap;
        stg(g.in0 + r0 + i, owned ? ch_table_input(g.in.bytes, off, len, j, 0) : Fr::zero());
        if (g.in1) stg(g.in1 + r0 + i, owned ? ch_table_input(g.in.bytes, off, len, j, 1) : Fr::zero());
    }
}

// the checks both ops share with the bytecode op, in its order and its words; `op` names the op in the message
static int ch_check_inputs(zk_ctx* ctx, const char* op, const void* d_bytes, uint64_t total_bytes, const void* d_offsets, const void* d_lens, uint32_t count, uint32_t iw, uint32_t flags) {
    if (flags) return ctx->fail(ZK_ERR_INVALID_ARG, "%s: flags 0x%x: must be 0", op, flags);
    if (iw != 4 && iw != 8) return ctx->fail(ZK_ERR_INVALID_ARG, "%s: index width %u: must be 4 or 8 bytes", op, iw);
    if (count && (!d_offsets || !d_lens)) return ctx->fail(ZK_ERR_INVALID_ARG, "%s: NULL offsets or lengths with %u bytecodes", op, count);
    if (count && ((uintptr_t)d_offsets % iw || (uintptr_t)d_lens % iw)) return ctx->fail(ZK_ERR_INVALID_ARG, "%s: offsets or lengths of %u bytes at a misaligned address", op, iw);
    if (!d_bytes && total_bytes) return ctx->fail(ZK_ERR_INVALID_ARG, "%s: NULL d_bytes with %llu bytes", op, (unsigned long long)total_bytes);
    if (total_bytes >> 61) return ctx->fail(ZK_ERR_INVALID_ARG, "%s: %llu bytes: 2^61 or more", op, (unsigned long long)total_bytes);
    return ZK_OK;
}

// scratch of both ops: start[0 .. m] | the sums of the scan's levels | (table, with d_rows_needed) the block sums
struct ChScratch { uint64_t starts_bytes, sums_bytes, blocks, blocks_bytes; };
static ChScratch ch_scratch(uint32_t m, bool block_sums) {
    const auto pad = [](uint64_t b) { return (b + 255) & ~(uint64_t)255; };
    ChScratch s;
    s.starts_bytes = pad(((uint64_t)m + 1) * 4);
    s.sums_bytes = 0;
    for (uint64_t c = (uint64_t)m + 1; c > BC_SCAN_TILE;) { c = (c + BC_SCAN_TILE - 1) / BC_SCAN_TILE; s.sums_bytes += ((c + 63) & ~(uint64_t)63) * 4; }
    s.sums_bytes = pad(s.sums_bytes);
    s.blocks = ((uint64_t)m + 1 + 255) / 256;
    s.blocks_bytes = block_sums ? pad(s.blocks * 8) : 0;
    return s;
}

// Everything is validated before n is looked at and before the first launch.
int code_hash_rows_run(zk_ctx* ctx, const zk_code_hash_rows* desc, const void* h_b, void* d_out, uint64_t n) {
    const uint32_t iw = desc->index_width;
    if (h_b) return ctx->fail(ZK_ERR_INVALID_ARG, "code hash rows: d_b must be NULL");
    if (int e = ch_check_inputs(ctx, "code hash rows", desc->d_bytes, desc->total_bytes, desc->d_offsets, desc->d_lens, desc->count, iw, desc->flags)) return e;
    if ((uintptr_t)d_out % 16 || (uintptr_t)desc->d_bytes_in_field_inv % 16 || (uintptr_t)desc->d_padding_shift % 16)
        return ctx->fail(ZK_ERR_INVALID_ARG, "code hash rows: d_out, d_bytes_in_field_inv or d_padding_shift at an address that is no multiple of 16");
    if ((uintptr_t)desc->d_control_length % 4) return ctx->fail(ZK_ERR_INVALID_ARG, "code hash rows: d_control_length at an address that is no multiple of 4");
    if (n >> 32) return ctx->fail(ZK_ERR_INVALID_ARG, "code hash rows: %llu rows: 2^32 or more", (unsigned long long)n);
    SpanList<11> spans;
    spans.add(d_out, n * sizeof(Fr), "d_out", true);
    spans.add(desc->d_control_length, n * 4, "d_control_length", true);
    spans.add(desc->d_bytes_in_field_index, n, "d_bytes_in_field_index", true);
    spans.add(desc->d_bytes_in_field_inv, n * sizeof(Fr), "d_bytes_in_field_inv", true);
    spans.add(desc->d_is_field_border, n, "d_is_field_border", true);
    spans.add(desc->d_padding_shift, n * sizeof(Fr), "d_padding_shift", true);
    spans.add(desc->d_field_index, n, "d_field_index", true);
    spans.add(desc->d_field_index_inv, n, "d_field_index_inv", true);
    spans.add(desc->d_bytes, desc->total_bytes, "d_bytes", false);
    spans.add(desc->d_offsets, (uint64_t)desc->count * iw, "d_offsets", false);
    spans.add(desc->d_lens, (uint64_t)desc->count * iw, "d_lens", false);
    const char *what, *other;
    if (spans.overlap(&what, &other)) return ctx->fail(ZK_ERR_INVALID_ARG, "code hash rows: %s overlaps %s", what, other);
    if (!n) return ZK_OK;

    ChRowsArgs g;
    memset(&g, 0, sizeof g);
    g.in.bytes = (const uint8_t*)desc->d_bytes;
    g.in.total = desc->total_bytes;
    g.in.offs = desc->d_offsets;
    g.in.lens = desc->d_lens;
    g.in.n = (uint32_t)n;
    g.in.m = desc->count < n ? desc->count : (uint32_t)n;            // a bytecode has at least its header row
    g.in.index_width = iw;
    g.field_input = (Fr*)d_out;
    g.inv = (Fr*)desc->d_bytes_in_field_inv;
    g.shift = (Fr*)desc->d_padding_shift;
    g.control = (uint32_t*)desc->d_control_length;
    g.index = (uint8_t*)desc->d_bytes_in_field_index;
    g.border = (uint8_t*)desc->d_is_field_border;
    g.field_index = (uint8_t*)desc->d_field_index;
    g.field_index_inv = (uint8_t*)desc->d_field_index_inv;

    const ChScratch sc = ch_scratch(g.in.m, false);
    uint8_t* s = (uint8_t*)ctx->get_scratch(SC_CODE_HASH, sc.starts_bytes + sc.sums_bytes);
    if (!s) return ZK_ERR_OOM;
    uint32_t* starts = (uint32_t*)s;
    g.in.starts = starts;

    const uint64_t widths = 32 + (g.inv ? 32 : 0) + (g.shift ? 32 : 0) + (g.control ? 4 : 0) + (g.index ? 1 : 0) + (g.border ? 1 : 0) + (g.field_index ? 1 : 0) + (g.field_index_inv ? 1 : 0);
    ZkProfScope prof(ctx, "code_hash_rows");
    prof.bytes = (uint64_t)desc->count * 2ull * iw + (g.in.m ? desc->total_bytes : 0) + n * widths;
    const uint64_t tiles = (n + BC_TILE - 1) / BC_TILE;
    hipLaunchKernelGGL(k_ch_widths<false>, dim3((unsigned)sc.blocks), dim3(256), 0, ctx->stream, g.in, starts, (uint64_t*)nullptr);
    bc_scan(ctx, starts, (uint64_t)g.in.m + 1, (uint32_t*)(s + sc.starts_bytes), g.in.n);
    hipLaunchKernelGGL(k_ch_rows, dim3((unsigned)tiles), dim3(256), 0, ctx->stream, g);
    ZK_CHECK_LAUNCH(ctx);
    return ZK_OK;
}

int code_hash_table_run(zk_ctx* ctx, const zk_code_hash_table* desc, const void* h_b, void* d_out, uint64_t n) {
    const uint32_t iw = desc->index_width;
    if (h_b) return ctx->fail(ZK_ERR_INVALID_ARG, "code hash table: d_b must be NULL");
    if (int e = ch_check_inputs(ctx, "code hash table", desc->d_bytes, desc->total_bytes, desc->d_offsets, desc->d_lens, desc->count, iw, desc->flags)) return e;
    if ((uintptr_t)d_out % 16 || (uintptr_t)desc->d_input1 % 16 || (uintptr_t)desc->d_control % 16)
        return ctx->fail(ZK_ERR_INVALID_ARG, "code hash table: d_out, d_input1 or d_control at an address that is no multiple of 16");
    if ((uintptr_t)desc->d_cap % 8 || (uintptr_t)desc->d_rows_needed % 8) return ctx->fail(ZK_ERR_INVALID_ARG, "code hash table: d_cap or d_rows_needed at an address that is no multiple of 8");
    if (n >> 32) return ctx->fail(ZK_ERR_INVALID_ARG, "code hash table: %llu rows: 2^32 or more", (unsigned long long)n);
    SpanList<10> spans;
    spans.add(d_out, n * sizeof(Fr), "d_out", true);
    spans.add(desc->d_input1, n * sizeof(Fr), "d_input1", true);
    spans.add(desc->d_control, n * 16, "d_control", true);
    spans.add(desc->d_heading_mark, n, "d_heading_mark", true);
    spans.add(desc->d_kinds, n, "d_kinds", true);
    spans.add(desc->d_cap, n * 8, "d_cap", true);
    spans.add(desc->d_rows_needed, 8, "d_rows_needed", true);
    spans.add(desc->d_bytes, desc->total_bytes, "d_bytes", false);
    spans.add(desc->d_offsets, (uint64_t)desc->count * iw, "d_offsets", false);
    spans.add(desc->d_lens, (uint64_t)desc->count * iw, "d_lens", false);
    const char *what, *other;
    if (spans.overlap(&what, &other)) return ctx->fail(ZK_ERR_INVALID_ARG, "code hash table: %s overlaps %s", what, other);
    if (!n) return ZK_OK;

    ChTableArgs g;
    memset(&g, 0, sizeof g);
    g.in.bytes = (const uint8_t*)desc->d_bytes;
    g.in.total = desc->total_bytes;
    g.in.offs = desc->d_offsets;
    g.in.lens = desc->d_lens;
    g.in.n = (uint32_t)n;
    g.in.m = desc->count;                                               // an empty bytecode owns no row: every entry takes part
    g.in.index_width = iw;
    g.in0 = (Fr*)d_out;
    g.in1 = (Fr*)desc->d_input1;
    g.control = (ChCell16*)desc->d_control;
    g.cap = (uint64_t*)desc->d_cap;
    g.mark = (uint8_t*)desc->d_heading_mark;
    g.kinds = (uint8_t*)desc->d_kinds;

    const ChScratch sc = ch_scratch(g.in.m, desc->d_rows_needed != nullptr);
    uint8_t* s = (uint8_t*)ctx->get_scratch(SC_CODE_HASH, sc.starts_bytes + sc.sums_bytes + sc.blocks_bytes);
    if (!s) return ZK_ERR_OOM;
    uint32_t* starts = (uint32_t*)s;
    uint64_t* block_rows = desc->d_rows_needed ? (uint64_t*)(s + sc.starts_bytes + sc.sums_bytes) : nullptr;
    g.in.starts = starts;

    const uint64_t widths = 32 + (g.in1 ? 32 : 0) + (g.control ? 16 : 0) + (g.cap ? 8 : 0) + (g.mark ? 1 : 0) + (g.kinds ? 1 : 0);
    ZkProfScope prof(ctx, "code_hash_table");
    prof.bytes = (uint64_t)desc->count * 2ull * iw + (g.in.m ? desc->total_bytes : 0) + n * widths + (block_rows ? 8 : 0);
    const uint64_t tiles = (n + BC_TILE - 1) / BC_TILE;
    hipLaunchKernelGGL(k_ch_widths<true>, dim3((unsigned)sc.blocks), dim3(256), 0, ctx->stream, g.in, starts, block_rows);
    if (block_rows) hipLaunchKernelGGL(k_ch_total, dim3(1), dim3(256), 0, ctx->stream, (const uint64_t*)block_rows, (uint32_t)sc.blocks, (uint64_t*)desc->d_rows_needed);
    bc_scan(ctx, starts, (uint64_t)g.in.m + 1, (uint32_t*)(s + sc.starts_bytes), g.in.n);
    hipLaunchKernelGGL(k_ch_table, dim3((unsigned)tiles), dim3(256), 0, ctx->stream, g);
    ZK_CHECK_LAUNCH(ctx);
    return ZK_OK;
}

}  // namespace zk

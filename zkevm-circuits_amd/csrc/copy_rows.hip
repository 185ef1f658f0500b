// ZK_OP_COPY_ROWS and ZK_OP_COPY_RLC of zk_field_vec_op: the rows of the copy circuit and of the copy table (table.rs
// CopyTable::assignments, copy_circuit.rs assign_copy_event and assign_padding_row) from one 88-byte record per copy event and the byte
// heap, both on the device.  The row logic is csrc/copy_rows.hip.hpp, which the host compiles too.
//
// The work is laid out in ROW space, which the host knows (n), not in event space, which it does not: no lane walks an event.
//   k_cp_widths     w[e] = min(2 L_e, n) (0 for an event that does not count), w[count] = 0
//   bc_scan         the exclusive scan of bytecode_rows.hip, saturating at n, in place -> start[0 .. count], start[count] = the rows in use
// ZK_OP_COPY_ROWS
//   k_cp_rows       a workgroup takes CP_TILE = 1024 rows, lane l the rows 4 l .. 4 l + 3 (two steps, both threads): one search of start
//                   per tile for its first and last row, a search per lane inside that window, the closed forms of cp_row, the 1-byte
//                   columns packed in LDS and stored as aligned dwords with head and tail bytes, the 8-byte cells straight
// ZK_OP_COPY_RLC    in STEP space (step g holds rows 2 g and 2 g + 1), blockIdx.y the thread, a lane SCAN_PER consecutive steps:
//   k_cp_acc_a      the composite map of every block of SCAN_THREADS x SCAN_PER steps
//   k_affine_b      (vec.hip, unchanged) the value that enters each block
//   k_cp_acc_c      the lane's exclusive map inside the block, then its steps again: value_acc, stored as it goes
//   k_cp_cols       (only with one of its outputs) the word RLCs, carried along the lane's steps and restarted from the word's first
//                   byte, at most 31 steps back, and the gathers: rlc_acc from value_acc at the event's last writer row, the ids
// No atomics, no host wait; every byte that is read lies inside a run that cp_event_ok has checked against total_bytes.
#include "affine.hip.hpp"
#include "copy_rows.hip.hpp"
#include "ctx.hpp"
#include "op_check.hpp"

namespace zk {

static_assert(offsetof(zk_copy_rows, d_events) == offsetof(zk_copy_rlc, d_events) && offsetof(zk_copy_rows, count) == offsetof(zk_copy_rlc, count) &&
              offsetof(zk_copy_rows, d_bytes) == offsetof(zk_copy_rlc, d_bytes) && offsetof(zk_copy_rows, total_bytes) == offsetof(zk_copy_rlc, total_bytes) &&
              offsetof(zk_copy_rows, flags) == offsetof(zk_copy_rlc, flags) && offsetof(zk_copy_rows, d_is_first) == offsetof(zk_copy_rlc, d_ids),
              "zk_copy_rows and zk_copy_rlc share their first five members");
static_assert(sizeof(zk_copy_event) == CP_EVENT_BYTES && offsetof(zk_copy_event, length) == 64 && offsetof(zk_copy_event, src_tag) == 84, "zk_copy_event is 88 packed bytes");

struct CpArgs {
    const uint64_t* events;             // count records of eleven words
    const uint8_t* bytes;
    uint64_t total;
    const uint32_t* starts;             // count + 1 entries
    uint32_t count, n;
    // ZK_OP_COPY_ROWS
    uint8_t *is_first, *is_last, *tag, *tag_bits, *value, *value_prev, *mask, *front_mask, *word_index, *is_pad, *non_pad_non_mask, *types, *src_end_rows;
    uint64_t *addr, *src_addr_end, *real_bytes_left, *rw_counter, *rwc_inc_left;
    // ZK_OP_COPY_RLC
    const Fr* ids;
    Fr *acc, *id, *id_other, *rlc_acc, *word, *word_prev;
    Fr r_word, r_in;
};

// event e as the op takes it: one that does not count has no steps
__device__ __forceinline__ CpEvent cp_load_event(const CpArgs& g, uint32_t e) {
    uint64_t w[CP_EVENT_WORDS];
#pragma unroll
    for (uint32_t k = 0; k < CP_EVENT_WORDS; ++k) w[k] = g.events[(uint64_t)e * CP_EVENT_WORDS + k];
    CpEvent ev = cp_event(w);
    if (!cp_event_ok(ev, g.total)) ev.len = 0;
    return ev;
}

__global__ void __launch_bounds__(256) k_cp_widths(const CpArgs g, uint32_t* w) {
    const uint64_t e = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (e > g.count) return;
    w[e] = e < g.count ? cp_rows_of(cp_load_event(g, (uint32_t)e).len, g.n) : 0u;
}

// The event of a row, kept while consecutive rows are asked for: [start, end) are the rows of event e, e == count behind the last event.
struct CpCursor {
    uint32_t e, start, end, lo, hi;     // [lo, hi]: the window of events the rows of this lane can belong to
    bool have;
    CpEvent ev;
};
__device__ __forceinline__ void cp_seek(const CpArgs& g, CpCursor& c, uint32_t row) {
    if (c.have && row < c.end) return;
    // the event behind this one where it holds the row, a search otherwise (empty events share their start with the next one)
    uint32_t e;
    if (c.have && c.e + 2 <= g.count && g.starts[c.e + 2] > row) e = c.e + 1;
    else e = bc_find(g.starts, c.have ? c.e : c.lo, c.hi, row);
    c.e = e, c.have = true;
    c.start = g.starts[e];
    c.end = e < g.count ? g.starts[e + 1] : g.n;
    if (e < g.count) c.ev = cp_load_event(g, e);
}

// rows [r0, r0 + rows) of a 1-byte column from the tile's packed bytes in LDS (st: CP_TILE / 4 + 1 words), as bc_store_col stores them:
// bytes up to the first address that is a multiple of 4, dwords, bytes again
__device__ __forceinline__ void cp_store_col(uint8_t* col, const uint32_t* st, uint32_t r0, uint32_t rows) {
    if (!col) return;
    uint8_t* p = col + r0;
    const uint8_t* sb = (const uint8_t*)st;
    uint32_t head = (uint32_t)(-(uintptr_t)p & 3);
    head = head < rows ? head : rows;
    if (threadIdx.x < head) p[threadIdx.x] = sb[threadIdx.x];
    const uint32_t body = (rows - head) >> 2;
    if (threadIdx.x < body) {                                           // body <= CP_LANES
        const uint32_t o = head + 4 * threadIdx.x, sh = (o & 3) * 8;
        const uint32_t lo = st[o >> 2], hi = st[(o >> 2) + 1];
        ((uint32_t*)(p + head))[threadIdx.x] = sh ? lo >> sh | hi << (32 - sh) : lo;
    }
    const uint32_t done = head + 4 * body;
    if (threadIdx.x < rows - done) p[done + threadIdx.x] = sb[done + threadIdx.x];
}

constexpr uint32_t CP_BYTE_COLS = 19;
// BYTES: an output holds byte values
template <bool BYTES>
__global__ void __launch_bounds__(256) k_cp_rows(const CpArgs g) {
    constexpr uint32_t ST = CP_TILE / 4 + 1;
    __shared__ uint32_t stage[CP_BYTE_COLS][ST];
    const uint32_t r0 = blockIdx.x * CP_TILE;
    const uint32_t rows = g.n - r0 < CP_TILE ? g.n - r0 : CP_TILE;
    if (threadIdx.x < CP_BYTE_COLS) stage[threadIdx.x][ST - 1] = 0;
    CpCursor c;
    c.have = false;
    c.lo = bc_find(g.starts, 0, g.count, r0);
    c.hi = bc_find(g.starts, c.lo, g.count, r0 + rows - 1);
    uint32_t pk[CP_BYTE_COLS];
#pragma unroll
    for (uint32_t q = 0; q < CP_BYTE_COLS; ++q) pk[q] = 0;
    CpRow row[CP_PER_LANE];
#pragma unroll
    for (uint32_t k = 0; k < CP_PER_LANE; ++k) {
        const uint32_t i = r0 + threadIdx.x * CP_PER_LANE + k;
        row[k] = cp_padding_row(i);
        if (i < g.n) {
            cp_seek(g, c, i);
            if (c.e < g.count) {
                const uint32_t j = i - c.start, s = j >> 1;
                uint32_t v = 0, vp = 0;
                if (BYTES) {
                    v = g.bytes[(j & 1u ? c.ev.dst_off : c.ev.src_off) + s];
                    vp = j & 1u ? g.bytes[c.ev.prev_off + s] : v;
                }
                row[k] = cp_row(c.ev, j, v, vp);
            }
        }
        const CpRow& r = row[k];
        const uint32_t tag = r.tag, sh = 8 * k;
        pk[0] |= (uint32_t)r.is_first << sh;
        pk[1] |= (uint32_t)r.is_last << sh;
        pk[2] |= tag << sh;
        pk[3] |= (tag >> 2 & 1u) << sh;
        pk[4] |= (tag >> 1 & 1u) << sh;
        pk[5] |= (tag & 1u) << sh;
        pk[6] |= (uint32_t)r.value << sh;
        pk[7] |= (uint32_t)r.value_prev << sh;
        pk[8] |= (uint32_t)r.mask << sh;
        pk[9] |= (uint32_t)r.front_mask << sh;
        pk[10] |= (uint32_t)r.word_index << sh;
        pk[11] |= (uint32_t)r.is_pad << sh;
        pk[12] |= (uint32_t)r.non_pad_non_mask << sh;
        pk[13] |= (uint32_t)(tag == 1u) << sh;
        pk[14] |= (uint32_t)(tag == 2u) << sh;
        pk[15] |= (uint32_t)(tag == 3u) << sh;
        pk[16] |= (uint32_t)(tag == 4u) << sh;
        pk[17] |= (uint32_t)r.memory_copy << sh;
        pk[18] |= (uint32_t)r.src_end_row << sh;
    }
#pragma unroll
    for (uint32_t q = 0; q < CP_BYTE_COLS; ++q) stage[q][threadIdx.x] = pk[q];
    __syncthreads();
    const uint64_t n = g.n;
    cp_store_col(g.is_first, stage[0], r0, rows);
    cp_store_col(g.is_last, stage[1], r0, rows);
    cp_store_col(g.tag, stage[2], r0, rows);
    if (g.tag_bits) {
#pragma unroll
        for (uint32_t b = 0; b < 3; ++b) cp_store_col(g.tag_bits + b * n, stage[3 + b], r0, rows);
    }
    cp_store_col(g.value, stage[6], r0, rows);
    cp_store_col(g.value_prev, stage[7], r0, rows);
    cp_store_col(g.mask, stage[8], r0, rows);
    cp_store_col(g.front_mask, stage[9], r0, rows);
    cp_store_col(g.word_index, stage[10], r0, rows);
    cp_store_col(g.is_pad, stage[11], r0, rows);
    cp_store_col(g.non_pad_non_mask, stage[12], r0, rows);
    if (g.types) {
#pragma unroll
        for (uint32_t b = 0; b < 5; ++b) cp_store_col(g.types + b * n, stage[13 + b], r0, rows);
    }
    cp_store_col(g.src_end_rows, stage[18], r0, rows);
#pragma unroll
    for (uint32_t k = 0; k < CP_PER_LANE; ++k) {
        const uint32_t i = threadIdx.x * CP_PER_LANE + k;
        if (i >= rows) continue;
        g.addr[r0 + i] = row[k].addr;
        if (g.src_addr_end) g.src_addr_end[r0 + i] = row[k].src_addr_end;
        if (g.real_bytes_left) g.real_bytes_left[r0 + i] = row[k].real_bytes_left;
        if (g.rw_counter) g.rw_counter[r0 + i] = row[k].rw_counter;
        if (g.rwc_inc_left) g.rwc_inc_left[r0 + i] = row[k].rwc_inc_left;
    }
}

// ---- ZK_OP_COPY_RLC ---------------------------------------------------------------------------------------------------------------------
// the Montgomery forms of 0 .. 255 into LDS, one per lane of the 256
__device__ __forceinline__ void cp_byte_table(Fr* tab) {
    Fr x = Fr::zero();
    x.l[0] = threadIdx.x;
    tab[threadIdx.x] = to_mont(x);
    __syncthreads();
}
// the window of events of the block's steps [g0, g0 + count) of thread t; false: the block has no row
__device__ __forceinline__ bool cp_step_window(const CpArgs& g, CpCursor& c, uint64_t g0, uint32_t t) {
    c.have = false;
    const uint64_t first = 2 * g0 + t, last_step = g0 + SCAN_THREADS * SCAN_PER - 1;
    if (first >= g.n) return false;
    const uint64_t last = 2 * last_step + t < g.n ? 2 * last_step + t : g.n - 1;
    c.lo = bc_find(g.starts, 0, g.count, (uint32_t)first);
    c.hi = bc_find(g.starts, c.lo, g.count, (uint32_t)last);
    return true;
}
// the map of the step at `row` of thread t as (kind, x): padding steps are the constant 0
__device__ __forceinline__ uint32_t cp_step_at(const CpArgs& g, CpCursor& c, uint32_t row, uint32_t t, uint32_t& x) {
    cp_seek(g, c, row);
    x = 0;
    if (c.e >= g.count) return CP_CONST;
    const uint32_t s = (row - c.start) >> 1;
    // the byte is read only where it is added
    uint32_t kind = cp_acc_step(c.ev, s, t, 1u, x);
    if (x) x = g.bytes[(t ? c.ev.dst_off : c.ev.src_off) + s];
    return kind;
}
__device__ __forceinline__ Aff cp_chunk(const CpArgs& g, const Fr* tab, CpCursor& c, uint64_t g0, uint32_t t) {
    Aff acc = aff_id();
#pragma unroll 1
    for (int k = 0; k < SCAN_PER; ++k) {
        const uint64_t row = 2 * (g0 + k) + t;
        if (row >= g.n) break;
        uint32_t x;
        const uint32_t kind = cp_step_at(g, c, (uint32_t)row, t, x);
        if (kind == CP_CONST) acc.A = Fr::zero(), acc.B = tab[x];
        else if (kind == CP_STEP) acc.A = g.r_in * acc.A, acc.B = g.r_in * acc.B + tab[x];
    }
    return acc;
}
__global__ void __launch_bounds__(SCAN_THREADS) k_cp_acc_a(const CpArgs g, Aff* __restrict__ maps) {
    __shared__ Aff sh[SCAN_THREADS];
    __shared__ Fr tab[256];
    cp_byte_table(tab);
    const uint32_t t = blockIdx.y;
    const uint64_t b0 = (uint64_t)blockIdx.x * (SCAN_THREADS * SCAN_PER);
    CpCursor c;
    Aff v = aff_id();
    if (cp_step_window(g, c, b0, t)) v = cp_chunk(g, tab, c, b0 + (uint64_t)threadIdx.x * SCAN_PER, t);
    const Aff total = aff_block_total(v, sh);
    Aff* out = maps + (uint64_t)t * gridDim.x + blockIdx.x;
    if (threadIdx.x == 0) { stg(&out->A, total.A); stg(&out->B, total.B); }
}
// entering == nullptr: a single block per thread, 0 enters it
__global__ void __launch_bounds__(SCAN_THREADS) k_cp_acc_c(const CpArgs g, const Fr* __restrict__ entering) {
    __shared__ Aff sh[SCAN_THREADS];
    __shared__ Fr tab[256];
    cp_byte_table(tab);
    const uint32_t t = blockIdx.y;
    const uint64_t b0 = (uint64_t)blockIdx.x * (SCAN_THREADS * SCAN_PER), g0 = b0 + (uint64_t)threadIdx.x * SCAN_PER;
    CpCursor c;
    Aff v = aff_id();
    const bool any = cp_step_window(g, c, b0, t);
    if (any) v = cp_chunk(g, tab, c, g0, t);
    Aff total;
    const Aff ex = aff_block_exclusive_scan(v, sh, &total);
    if (!any) return;
    Fr z = entering ? aff_apply(ex, ldg(entering + (uint64_t)t * gridDim.x + blockIdx.x)) : ex.B;
    c.have = false;
#pragma unroll 1
    for (int k = 0; k < SCAN_PER; ++k) {
        const uint64_t row = 2 * (g0 + k) + t;
        if (row >= g.n) break;
        uint32_t x;
        const uint32_t kind = cp_step_at(g, c, (uint32_t)row, t, x);
        if (kind == CP_CONST) z = tab[x];
        else if (kind == CP_STEP) z = g.r_in * z + tab[x];
        stg(g.acc + row, z);
    }
}
// an Fr at an address that is a multiple of 8
__device__ __forceinline__ Fr cp_ld8(const Fr* p) {
    const uint2* q = (const uint2*)p;
    Fr h;
#pragma unroll
    for (int j = 0; j < 4; ++j) { const uint2 w = q[j]; h.l[2 * j] = w.x; h.l[2 * j + 1] = w.y; }
    return h;
}
// the word RLCs and the gathers, after value_acc has been written
__global__ void __launch_bounds__(SCAN_THREADS) k_cp_cols(const CpArgs g) {
    __shared__ Fr tab[256];
    cp_byte_table(tab);
    const uint32_t t = blockIdx.y;
    const uint64_t b0 = (uint64_t)blockIdx.x * (SCAN_THREADS * SCAN_PER), g0 = b0 + (uint64_t)threadIdx.x * SCAN_PER;
    CpCursor c;
    if (!cp_step_window(g, c, b0, t)) return;
    const bool words = g.word || g.word_prev;
    Fr w = Fr::zero(), wp = Fr::zero();
    bool fresh = true;                                                  // nothing is carried into the next step yet
#pragma unroll 1
    for (int k = 0; k < SCAN_PER; ++k) {
        const uint64_t row64 = 2 * (g0 + k) + t;
        if (row64 >= g.n) break;
        const uint32_t row = (uint32_t)row64;
        const uint32_t before = c.have ? c.e : 0xffffffffu;
        cp_seek(g, c, row);
        if (c.e != before) fresh = true;
        if (c.e >= g.count) {                                           // padding
            if (g.word) stg(g.word + row, Fr::zero());
            if (g.word_prev) stg(g.word_prev + row, Fr::zero());
            if (g.rlc_acc) stg(g.rlc_acc + row, Fr::zero());
            if (g.id) stg(g.id + row, Fr::zero());
            if (g.id_other) stg(g.id_other + row, Fr::one());
            continue;
        }
        const uint32_t s = (row - c.start) >> 1;
        if (words) {
            const uint64_t off = t ? c.ev.dst_off : c.ev.src_off;
            // a word starts at every s mod 32 == 0; a lane that enters a word in its middle runs through the bytes before
            const uint32_t from = cp_word_from(s, fresh);
            if (from != s || (s & 31u) == 0) { w = Fr::zero(); wp = Fr::zero(); }
            for (uint32_t u = from; u <= s; ++u) {
                w = w * g.r_word + tab[g.bytes[off + u]];
                if (t && g.word_prev) wp = wp * g.r_word + tab[g.bytes[c.ev.prev_off + u]];
            }
            fresh = false;
            if (g.word) stg(g.word + row, w);
            if (g.word_prev) stg(g.word_prev + row, t ? wp : w);
        }
        if (g.rlc_acc) {
            const uint64_t last = (uint64_t)c.start + 2ull * c.ev.len - 1;      // the event's last writer row
            stg(g.rlc_acc + row, cp_has_rlc(c.ev) && last < g.n ? ldg(g.acc + last) : Fr::zero());
        }
        if (g.id) stg(g.id + row, g.ids ? cp_ld8(g.ids + 2ull * c.e + t) : Fr::zero());
        if (g.id_other) stg(g.id_other + row, g.ids ? cp_ld8(g.ids + 2ull * c.e + 1 - t) : Fr::zero());
    }
}

// ---- host side --------------------------------------------------------------------------------------------------------------------------------
// the checks of the members the two descriptors share; `op`: the name in the message
static int cp_check_shared(zk_ctx* ctx, const char* op, const zk_copy_rows* d, uint64_t n) {
    if (d->flags) return ctx->fail(ZK_ERR_INVALID_ARG, "%s: flags 0x%x: must be 0", op, d->flags);
    if (d->count && !d->d_events) return ctx->fail(ZK_ERR_INVALID_ARG, "%s: NULL d_events with %u events", op, d->count);
    if (d->count && (uintptr_t)d->d_events % 8) return ctx->fail(ZK_ERR_INVALID_ARG, "%s: d_events at an address that is no multiple of 8", op);
    if (!d->d_bytes && d->total_bytes) return ctx->fail(ZK_ERR_INVALID_ARG, "%s: NULL d_bytes with %llu bytes", op, (unsigned long long)d->total_bytes);
    if (d->total_bytes >> 61) return ctx->fail(ZK_ERR_INVALID_ARG, "%s: %llu bytes: 2^61 or more", op, (unsigned long long)d->total_bytes);
    if (n >> 32) return ctx->fail(ZK_ERR_INVALID_ARG, "%s: %llu rows: 2^32 or more", op, (unsigned long long)n);
    return ZK_OK;
}
// scratch of the row starts: start[0 .. count] | the sums of the scan's levels; *extra more bytes behind them, 256-aligned
static uint8_t* cp_starts(zk_ctx* ctx, CpArgs& g, uint64_t extra, uint64_t* extra_at) {
    const auto pad = [](uint64_t b) { return (b + 255) & ~(uint64_t)255; };
    const uint64_t starts_bytes = pad(((uint64_t)g.count + 1) * 4);
    uint64_t sums_bytes = 0;
    for (uint64_t c = (uint64_t)g.count + 1; c > BC_SCAN_TILE;) { c = (c + BC_SCAN_TILE - 1) / BC_SCAN_TILE; sums_bytes += ((c + 63) & ~(uint64_t)63) * 4; }
    sums_bytes = pad(sums_bytes);
    uint8_t* s = (uint8_t*)ctx->get_scratch(SC_COPY, starts_bytes + sums_bytes + extra);
    if (!s) return nullptr;
    *extra_at = starts_bytes + sums_bytes;
    g.starts = (const uint32_t*)s;
    hipLaunchKernelGGL(k_cp_widths, dim3((unsigned)(((uint64_t)g.count + 1 + 255) / 256)), dim3(256), 0, ctx->stream, g, (uint32_t*)s);
    bc_scan(ctx, (uint32_t*)s, (uint64_t)g.count + 1, (uint32_t*)(s + starts_bytes), g.n);
    return s;
}

// Everything is validated before n is looked at and before the first launch.
int copy_rows_run(zk_ctx* ctx, const zk_copy_rows* desc, const void* h_b, void* d_out, uint64_t n) {
    if (const int rc = cp_check_shared(ctx, "copy rows", desc, n)) return rc;
    if (h_b) return ctx->fail(ZK_ERR_INVALID_ARG, "copy rows: the op takes no second operand");
    if ((uintptr_t)d_out % 8 || (uintptr_t)desc->d_src_addr_end % 8 || (uintptr_t)desc->d_real_bytes_left % 8 || (uintptr_t)desc->d_rw_counter % 8 || (uintptr_t)desc->d_rwc_inc_left % 8)
        return ctx->fail(ZK_ERR_INVALID_ARG, "copy rows: d_out, d_src_addr_end, d_real_bytes_left, d_rw_counter or d_rwc_inc_left at an address that is no multiple of 8");
    SpanList<20> spans;
    spans.add(d_out, n * 8, "d_out", true);
    spans.add(desc->d_is_first, n, "d_is_first", true);
    spans.add(desc->d_is_last, n, "d_is_last", true);
    spans.add(desc->d_tag, n, "d_tag", true);
    spans.add(desc->d_tag_bits, n * 3, "d_tag_bits", true);
    spans.add(desc->d_value, n, "d_value", true);
    spans.add(desc->d_value_prev, n, "d_value_prev", true);
    spans.add(desc->d_mask, n, "d_mask", true);
    spans.add(desc->d_front_mask, n, "d_front_mask", true);
    spans.add(desc->d_word_index, n, "d_word_index", true);
    spans.add(desc->d_src_addr_end, n * 8, "d_src_addr_end", true);
    spans.add(desc->d_is_pad, n, "d_is_pad", true);
    spans.add(desc->d_non_pad_non_mask, n, "d_non_pad_non_mask", true);
    spans.add(desc->d_real_bytes_left, n * 8, "d_real_bytes_left", true);
    spans.add(desc->d_rw_counter, n * 8, "d_rw_counter", true);
    spans.add(desc->d_rwc_inc_left, n * 8, "d_rwc_inc_left", true);
    spans.add(desc->d_types, n * 5, "d_types", true);
    spans.add(desc->d_src_end_rows, n, "d_src_end_rows", true);
    spans.add(desc->d_events, (uint64_t)desc->count * CP_EVENT_BYTES, "d_events", false);
    spans.add(desc->d_bytes, desc->total_bytes, "d_bytes", false);
    const char *what, *other;
    if (spans.overlap(&what, &other)) return ctx->fail(ZK_ERR_INVALID_ARG, "copy rows: %s overlaps %s", what, other);
    if (!n) return ZK_OK;

    CpArgs g;
    memset(&g, 0, sizeof g);
    g.events = (const uint64_t*)desc->d_events;
    g.bytes = (const uint8_t*)desc->d_bytes;
    g.total = desc->total_bytes;
    g.count = desc->count, g.n = (uint32_t)n;
    g.is_first = (uint8_t*)desc->d_is_first, g.is_last = (uint8_t*)desc->d_is_last, g.tag = (uint8_t*)desc->d_tag, g.tag_bits = (uint8_t*)desc->d_tag_bits;
    g.value = (uint8_t*)desc->d_value, g.value_prev = (uint8_t*)desc->d_value_prev, g.mask = (uint8_t*)desc->d_mask, g.front_mask = (uint8_t*)desc->d_front_mask;
    g.word_index = (uint8_t*)desc->d_word_index, g.is_pad = (uint8_t*)desc->d_is_pad, g.non_pad_non_mask = (uint8_t*)desc->d_non_pad_non_mask;
    g.types = (uint8_t*)desc->d_types, g.src_end_rows = (uint8_t*)desc->d_src_end_rows;
    g.addr = (uint64_t*)d_out, g.src_addr_end = (uint64_t*)desc->d_src_addr_end, g.real_bytes_left = (uint64_t*)desc->d_real_bytes_left;
    g.rw_counter = (uint64_t*)desc->d_rw_counter, g.rwc_inc_left = (uint64_t*)desc->d_rwc_inc_left;
    const bool bytes = g.count && (g.value || g.value_prev);

    uint64_t widths = 8, at;
    for (const void* p : {desc->d_is_first, desc->d_is_last, desc->d_tag, desc->d_value, desc->d_value_prev, desc->d_mask, desc->d_front_mask, desc->d_word_index, desc->d_is_pad,
                          desc->d_non_pad_non_mask, desc->d_src_end_rows})
        widths += p ? 1 : 0;
    for (const void* p : {desc->d_src_addr_end, desc->d_real_bytes_left, desc->d_rw_counter, desc->d_rwc_inc_left}) widths += p ? 8 : 0;
    widths += (desc->d_tag_bits ? 3 : 0) + (desc->d_types ? 5 : 0);
    ZkProfScope prof(ctx, "copy_rows");
    prof.bytes = (uint64_t)desc->count * CP_EVENT_BYTES + (bytes ? desc->total_bytes : 0) + n * widths;
    if (!cp_starts(ctx, g, 0, &at)) return ZK_ERR_OOM;
    const unsigned tiles = (unsigned)((n + CP_TILE - 1) / CP_TILE);
    if (bytes) hipLaunchKernelGGL(k_cp_rows<true>, dim3(tiles), dim3(256), 0, ctx->stream, g);
    else hipLaunchKernelGGL(k_cp_rows<false>, dim3(tiles), dim3(256), 0, ctx->stream, g);
    ZK_CHECK_LAUNCH(ctx);
    return ZK_OK;
}

// h_challenges: r_word, then r_in, Montgomery Fr in host memory
int copy_rlc_run(zk_ctx* ctx, const zk_copy_rlc* desc, const void* h_challenges, void* d_out, uint64_t n) {
    if (const int rc = cp_check_shared(ctx, "copy RLC", (const zk_copy_rows*)desc, n)) return rc;
    if ((uintptr_t)desc->d_ids % 8) return ctx->fail(ZK_ERR_INVALID_ARG, "copy RLC: d_ids at an address that is no multiple of 8");
    if ((uintptr_t)d_out % 16 || (uintptr_t)desc->d_id % 16 || (uintptr_t)desc->d_id_other % 16 || (uintptr_t)desc->d_rlc_acc % 16 || (uintptr_t)desc->d_word_rlc % 16 || (uintptr_t)desc->d_word_rlc_prev % 16)
        return ctx->fail(ZK_ERR_INVALID_ARG, "copy RLC: an output at an address that is no multiple of 16");
    SpanList<9> spans;
    spans.add(d_out, n * sizeof(Fr), "d_out", true);
    spans.add(desc->d_id, n * sizeof(Fr), "d_id", true);
    spans.add(desc->d_id_other, n * sizeof(Fr), "d_id_other", true);
    spans.add(desc->d_rlc_acc, n * sizeof(Fr), "d_rlc_acc", true);
    spans.add(desc->d_word_rlc, n * sizeof(Fr), "d_word_rlc", true);
    spans.add(desc->d_word_rlc_prev, n * sizeof(Fr), "d_word_rlc_prev", true);
    spans.add(desc->d_events, (uint64_t)desc->count * CP_EVENT_BYTES, "d_events", false);
    spans.add(desc->d_bytes, desc->total_bytes, "d_bytes", false);
    spans.add(desc->d_ids, (uint64_t)desc->count * 2 * sizeof(Fr), "d_ids", false);
    const char *what, *other;
    if (spans.overlap(&what, &other)) return ctx->fail(ZK_ERR_INVALID_ARG, "copy RLC: %s overlaps %s", what, other);
    Fr ch[2];
    memcpy(ch, h_challenges, sizeof ch);
    if (!n) return ZK_OK;

    CpArgs g;
    memset(&g, 0, sizeof g);
    g.events = (const uint64_t*)desc->d_events;
    g.bytes = (const uint8_t*)desc->d_bytes;
    g.total = desc->total_bytes;
    g.count = desc->count, g.n = (uint32_t)n;
    g.ids = (const Fr*)desc->d_ids;
    g.acc = (Fr*)d_out, g.id = (Fr*)desc->d_id, g.id_other = (Fr*)desc->d_id_other, g.rlc_acc = (Fr*)desc->d_rlc_acc;
    g.word = (Fr*)desc->d_word_rlc, g.word_prev = (Fr*)desc->d_word_rlc_prev;
    g.r_word = ch[0] * Fr::one(), g.r_in = ch[1] * Fr::one();            // times Montgomery one: the value itself, canonical
    const bool cols = g.id || g.id_other || g.rlc_acc || g.word || g.word_prev;

    const uint64_t steps = (n + 1) / 2, blocks = (steps + SCAN_THREADS * SCAN_PER - 1) / (SCAN_THREADS * SCAN_PER);
    uint64_t at;
    uint64_t outs = 1;
    for (const void* p : {desc->d_id, desc->d_id_other, desc->d_rlc_acc, desc->d_word_rlc, desc->d_word_rlc_prev}) outs += p ? 1 : 0;
    ZkProfScope prof(ctx, "copy_rlc");
    prof.bytes = (uint64_t)desc->count * (CP_EVENT_BYTES + (g.ids ? 64 : 0)) + desc->total_bytes + n * outs * sizeof(Fr);
    uint8_t* s = cp_starts(ctx, g, blocks > 1 ? 2 * blocks * (sizeof(Aff) + sizeof(Fr)) : 0, &at);
    if (!s) return ZK_ERR_OOM;
    Aff* maps = (Aff*)(s + at);
    Fr* entering = nullptr;
    const dim3 grid((unsigned)blocks, 2);
    if (blocks > 1) {
        entering = (Fr*)(maps + 2 * blocks);
        hipLaunchKernelGGL(k_cp_acc_a, grid, dim3(SCAN_THREADS), 0, ctx->stream, g, maps);
        affine_b_launch(ctx, maps, entering, (uint32_t)blocks);
        affine_b_launch(ctx, maps + blocks, entering + blocks, (uint32_t)blocks);
    }
    hipLaunchKernelGGL(k_cp_acc_c, grid, dim3(SCAN_THREADS), 0, ctx->stream, g, (const Fr*)entering);
    if (cols) hipLaunchKernelGGL(k_cp_cols, grid, dim3(SCAN_THREADS), 0, ctx->stream, g);
    ZK_CHECK_LAUNCH(ctx);
    return ZK_OK;
}

}  // namespace zk

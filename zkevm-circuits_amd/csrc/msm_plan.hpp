// Host-only planning of the MSM batches of msm.hip: the layout constants the kernels share with the host, the window plans,
// the measurement knobs, the two carvers (sort workspace, bucket buffer) and plan_batch -- everything a batch of commitments
// over an SRS decides before its first allocation, as a pure function of the batch's shape and the knobs.  No HIP, no context:
// a stand-alone program compiles this header without the kernels (tools/msm_batch_plan_check.cpp), and zk_host_msm_batch_plan
// shows the same records to the CPU tests (tests/test_msm_batch_plan.py).
#pragma once
#include <algorithm>
#include <climits>
#include <cstddef>
#include <cstdint>
#include <cstdlib>
#include <vector>

namespace zk {

// ---- layout constants shared with the kernels (msm.hip says what each kernel does with them) -------------------------
constexpr int MSM_MAX_C = 16;
constexpr int MSM_RANGE_MAX_BITS = 11;   // <= 2048 buckets per workgroup
constexpr int MSM_SLICES = 4;        // == SCAN_ITEMS: a scan thread sees the slices of one bucket
constexpr int MSM_M_MIN_C = 8, MSM_M_MAX_C = 22;
constexpr uint32_t MSM_M_MAX_BINS = 1u << (MSM_M_MAX_C - 1 - MSM_RANGE_MAX_BITS);     // 1024 partitions of 2048 buckets
constexpr uint32_t MSM_M_CHUNK = 2048;                                                   // scalars per workgroup of the partition passes
constexpr int GM_MAX_COLS = 16;
constexpr uint32_t MSM_M_SCHUNK = 1024;                 // scalars per workgroup of the staged scatter (and of its histogram pass)
static size_t scatter_staged_lds(int W) { return (size_t)(2 * MSM_M_MAX_BINS + 16) * 4 + (size_t)MSM_M_SCHUNK * W * 10; }
constexpr uint32_t MSM_M_STAGE = 15u * 1024u;      // 60 KiB of indices + 8 KiB of counters: two workgroups per CU
constexpr int SCAN_T = 1024, SCAN_ITEMS = 4;
constexpr uint32_t SIZE_BINS = 256;
constexpr uint32_t MSM_WFLAGS = 256;           // window flags of one sort (behind nmulti + 4): up to eight small-valued columns of 16 windows share a launch sequence
constexpr uint32_t TASK_DONE_MAX = 1u << 17;   // done-counters (behind nmulti + 4 + MSM_WFLAGS) of the split buckets that straddle a wave boundary inside k_msm_buckets: positions below this
constexpr uint32_t TASK_CAP = 48;       // points per task, see "skew-proof work split" in msm.hip
constexpr uint32_t TASK_MIN = 8, TASK_TARGET = 1u << 18;
constexpr int RED_G_WIDE = 8, RED_G_FOLDED = 2, RED_G_MERGED = 16;
constexpr int RED_THREADS = 256;
constexpr size_t MSM_AFFINE_BYTES = 64;        // sizeof(G1Affine): a window table entry
constexpr uint32_t FR_MODULUS[8] = {0xf0000001u, 0x43e1f593u, 0x79b97091u, 0x2833e848u, 0x8181585du, 0xb85045b6u, 0xe131a029u, 0x30644e72u};   // == FrP::M (msm.hip asserts it)

struct MsmPlan {
    int c;          // window bits
    int W;          // windows
    uint32_t B;     // buckets per window = 2^(c-1)
    int top_shift = 0;   // merged-window path: the top window's digit is scaled by 2^top_shift (its table entry is 2^(c (W-1) - top_shift) P)
};

static MsmPlan make_plan(size_t n) {
    int lg = 0;
    while ((1ull << (lg + 1)) <= n) ++lg;
    int c = lg - 4;
    if (c < 4) c = 4;
    if (c > MSM_MAX_C) c = MSM_MAX_C;
    MsmPlan p;
    p.c = c;
    p.W = (256 + c - 1) / c;
    p.B = 1u << (c - 1);
    return p;
}

// Measurement knobs.  read_knobs() is called at the top of every call that applies one and its result is never kept: a
// process may change the environment between two calls.  A field is the variable's atoi, KNOB_UNSET when it is not
// set; the range of a knob is checked where it is applied.
constexpr int KNOB_UNSET = INT_MIN;
struct MsmKnobs {
    int c, top_shift;                                       // ZK_MSM_C, ZK_MSM_TOP_SHIFT: the merged plan (make_plan_merged)
    int binsort, staged, chunk;                             // ZK_MSM_BINSORT, ZK_MSM_STAGED, ZK_MSM_CHUNK: the merged sort
    int pipes, graph;                                       // ZK_MSM_PIPES, ZK_MSM_GRAPH: pipelines of a small batch
    int narrow, narrow_group, narrow_gm, gm_sets;           // ZK_MSM_NARROW, ZK_MSM_NARROW_GROUP, ZK_MSM_NARROW_GM, ZK_MSM_GM_SETS: small-valued columns
    double table_gb;                                        // ZK_MSM_TABLE_GB: largest window table per basis (default 32 GiB)
    bool trace;                                             // ZK_MSM_TRACE (set at all): host enqueue / device drain times of every batch on stderr
};
static MsmKnobs read_knobs() {
    auto num = [](const char* name) { const char* e = getenv(name); return e ? atoi(e) : KNOB_UNSET; };
    MsmKnobs k;
    k.c = num("ZK_MSM_C");
    k.top_shift = num("ZK_MSM_TOP_SHIFT");
    k.binsort = num("ZK_MSM_BINSORT");
    k.staged = num("ZK_MSM_STAGED");
    k.chunk = num("ZK_MSM_CHUNK");
    k.pipes = num("ZK_MSM_PIPES");
    k.graph = num("ZK_MSM_GRAPH");
    k.narrow = num("ZK_MSM_NARROW");
    k.narrow_group = num("ZK_MSM_NARROW_GROUP");
    k.narrow_gm = num("ZK_MSM_NARROW_GM");
    k.gm_sets = num("ZK_MSM_GM_SETS");
    const char* gb = getenv("ZK_MSM_TABLE_GB");
    k.table_gb = gb ? atof(gb) : 32.0;
    k.trace = getenv("ZK_MSM_TRACE") != nullptr;
    return k;
}

// ---- merged-window MSM over an SRS window table ----------------------------------------------------
static MsmPlan make_plan_merged(uint32_t k_srs, const MsmKnobs& kn) {
    int c = (int)k_srs;
    if (c < MSM_M_MIN_C) c = MSM_M_MIN_C;
    if (c > MSM_M_MAX_C) c = MSM_M_MAX_C;
    if (kn.c >= MSM_M_MIN_C && kn.c <= MSM_M_MAX_C) c = kn.c;   // measurement knob
    MsmPlan p;
    p.c = c;
    p.W = (256 + c - 1) / c;
    p.B = 1u << (c - 1);
    // largest shift that keeps the top digit (leading bits of a canonical scalar, plus the carry of the window below)
    // at or below 2^(c-1)
    const int low = c * (p.W - 1);
    uint64_t top_max = 1;
    if (low < 254) {
        uint64_t v = 0;      // (modulus - 1) >> low, from the 8 x 32-bit limbs (the modulus is odd: -1 only clears bit 0)
        for (int b = 0; b < 40 && low + b < 256; ++b) {
            const int bit = low + b;
            const uint32_t limb = bit < 32 ? FR_MODULUS[0] - 1u : FR_MODULUS[bit >> 5];
            v |= (uint64_t)((limb >> (bit & 31)) & 1u) << b;
        }
        top_max = v + 1;
    }
    p.top_shift = 0;
    while (p.top_shift + 1 <= c - 1 && (top_max << (p.top_shift + 1)) <= (1ull << (c - 1))) ++p.top_shift;
    if (kn.top_shift >= 0 && kn.top_shift <= p.top_shift) p.top_shift = kn.top_shift;   // measurement knob
    return p;
}
// Commitments of n points over an SRS of 2^k take the merged-window table of plan `m`: not for a tiny MSM, not when the table
// would be larger than ZK_MSM_TABLE_GB, and table indices carry the sign in bit 31.  srs_window_table builds the table under
// this condition and zk_msm_plan reports the plan under it.
static bool merged_table_wanted(uint32_t k_srs, size_t n, const MsmPlan& m, const MsmKnobs& kn) {
    const uint64_t ns = 1ull << k_srs;
    return n >= 64 && (double)(MSM_AFFINE_BYTES * ns * m.W) <= kn.table_gb * (double)(1ull << 30) && (uint64_t)m.W * ns < (1ull << 31);
}

// ---- the two carvers ---------------------------------------------------------------------------------
// A bump allocator over elements of T describes a layout once: over a null base it only counts -- the size to ask for --,
// over the buffer it hands out the pointers, so the two cannot disagree.  log (nullable) receives every region taken.
struct CarvedRegion { int id; size_t at, len; };
template <class T>
struct Carver {
    T* base;
    size_t at = 0;
    std::vector<CarvedRegion>* log = nullptr;
    T* take(size_t count, size_t align = 1, int id = -1) {
        at = (at + align - 1) / align * align;
        T* p = base ? base + at : nullptr;
        if (log) log->push_back({id, at, count});
        at += count;
        return p;
    }
};
using WsCarver = Carver<uint32_t>;      // the sort workspace, in u32 words

static inline uint32_t scan_blocks_of(uint32_t cnt) { return (cnt + SCAN_T * SCAN_ITEMS - 1) / (SCAN_T * SCAN_ITEMS); }
// size_hist[SIZE_BINS] | nmulti[4] | window flags[MSM_WFLAGS] | done-counters[TASK_DONE_MAX]: the kernels find the flags
// and the counters behind nmulti, and every sort starts by clearing the four with ONE memset -- they are one region
constexpr uint32_t MSM_CLEARED_WORDS = SIZE_BINS + 4 + MSM_WFLAGS + TASK_DONE_MAX;
// The three layouts by their dimensions:
//   per-window "N" (msm_batch_tab, small-valued columns):  slices, idx[n * windows], digit matrix
//   merged "M":                                            slices (the sliced sort), partition histogram, idx and entries[n * W]
//   grouped "GM":                                          partition histogram, idx and entries[n * W * columns]
struct SortDims {
    uint32_t nb;            // buckets
    bool slices;            // [bucket][slice] counters and offsets of a sort by MSM_SLICES workgroups per bucket range
    uint32_t hist_cnt;      // partition histogram: partitions x workgroups (0: no partition pass)
    uint64_t idx_cnt;       // sorted indices, worst case
    size_t dig_words;       // u16 digit matrix, in words (0: none)
    bool entries;           // u64 (bucket, table index) entries, idx_cnt of them
};
struct SortWs {
    uint32_t *slice_counts, *slice_off, *block_tot_s;       // slices (both 16-B aligned: k_scan_u32_c reads the MSM_SLICES words of a bucket as one uint4)
    uint32_t *counts, *offsets, *order, *ntasks, *toff, *block_tot;
    uint32_t *cleared, *size_hist, *nmulti, *wflag;         // the cleared region and its named parts
    uint32_t *hist, *hist_off, *block_tot_h;                // partition pass
    uint32_t* idx;
    uint16_t* dig;                                          // 16-B aligned
    uint64_t* entries;                                      // 8-B aligned
    size_t words;                                           // of the whole layout
};
enum SortRegion : int { SR_SLICE_COUNTS, SR_SLICE_OFF, SR_COUNTS, SR_CLEARED, SR_OFFSETS, SR_ORDER, SR_NTASKS, SR_TOFF, SR_BLOCK_TOT_S, SR_BLOCK_TOT, SR_BLOCK_TOT_H, SR_HIST, SR_HIST_OFF,
                        SR_IDX, SR_DIG, SR_ENTRIES };
static SortWs carve_sort_ws(const SortDims& d, uint32_t* base, std::vector<CarvedRegion>* log = nullptr) {
    WsCarver c{base, 0, log};
    SortWs w{};
    if (d.slices) {
        w.slice_counts = c.take((size_t)d.nb * MSM_SLICES, 4, SR_SLICE_COUNTS);
        w.slice_off = c.take((size_t)d.nb * MSM_SLICES + 4, 4, SR_SLICE_OFF);
    }
    w.counts = c.take(d.nb, 1, SR_COUNTS);
    w.cleared = c.take(MSM_CLEARED_WORDS, 1, SR_CLEARED);
    w.size_hist = w.cleared;
    w.nmulti = w.size_hist + SIZE_BINS;
    w.wflag = w.nmulti + 4;
    w.offsets = c.take((size_t)d.nb + 1, 1, SR_OFFSETS);
    w.order = c.take(d.nb, 1, SR_ORDER);
    w.ntasks = c.take(d.nb, 1, SR_NTASKS);
    w.toff = c.take((size_t)d.nb + 1, 1, SR_TOFF);
    if (d.slices) w.block_tot_s = c.take(scan_blocks_of(d.nb * MSM_SLICES), 1, SR_BLOCK_TOT_S);
    w.block_tot = c.take(scan_blocks_of(d.nb), 1, SR_BLOCK_TOT);
    if (d.hist_cnt) {
        w.block_tot_h = c.take(scan_blocks_of(d.hist_cnt), 1, SR_BLOCK_TOT_H);
        w.hist = c.take(d.hist_cnt, 1, SR_HIST);
        w.hist_off = c.take((size_t)d.hist_cnt + 1, 1, SR_HIST_OFF);
    }
    w.idx = c.take(d.idx_cnt, 1, SR_IDX);
    if (d.dig_words) w.dig = reinterpret_cast<uint16_t*>(c.take(d.dig_words, 4, SR_DIG));
    if (d.entries) w.entries = reinterpret_cast<uint64_t*>(c.take(2 * (size_t)d.idx_cnt, 2, SR_ENTRIES));
    w.words = c.at;
    return w;
}

// Bucket buffer of one MSM (or one group of columns), in points of type Pt:
//   buckets | partials of the weighted reduction | task partials | (per-window sorts) the folded windows
// nb and tasks are what the step at hand uses of the first and the third region (the grids and bounds of its launches).
enum BucketRegion : int { BR_BUCKETS, BR_PARTIAL, BR_TASK_PARTIAL, BR_FOLDED };
template <class Pt>
struct BucketRegions {
    Pt *buckets, *partial, *task_partial, *folded;          // folded: nullptr where nothing is folded
    uint32_t nb;
    size_t tasks;
    size_t points;                                          // of the whole layout
};
template <class Pt>
static BucketRegions<Pt> carve_bucket_regions(size_t buckets, size_t partial, size_t task_partial, size_t folded, Pt* base, std::vector<CarvedRegion>* log = nullptr) {
    Carver<Pt> c{base, 0, log};
    BucketRegions<Pt> r{};
    r.buckets = c.take(buckets, 1, BR_BUCKETS);
    r.partial = c.take(partial, 1, BR_PARTIAL);
    r.task_partial = c.take(task_partial, 1, BR_TASK_PARTIAL);
    if (folded) r.folded = c.take(folded, 1, BR_FOLDED);
    r.points = c.at;
    return r;
}

// ---- the plan of a batch over an SRS with its merged-window table (msm_batch_merged) ----------------------------------
struct MsmBatchShape {
    size_t n, count, tab_stride;
    MsmPlan pl;                     // merged plan, the one the table was built for
    const MsmPlan* pl_n;            // per-window plan of the small-valued columns; nullptr: there is no per-window table
    const uint8_t* hints;           // per column (nullable): 1 small-valued, 2 run-structured (sliced sort), anything else dense
    uint32_t blinded_tail;          // zk_ctx::msm_blinded_tail
    bool prof_on, graph_broken;     // zk_ctx::prof_on, zk_ctx::msm_graph_broken
    uint32_t group_cap;             // != 0: upper bound on the columns of a group (the retry of msm_batch_merged)
};
// STEP_WINDOW: per-window digit-matrix sort over the per-window table; STEP_DENSE / STEP_DENSE_SLICED: one merged column, sorted
// by the one-launch partition sort / the sliced sort; STEP_GM: a group of small-valued columns through the partition sort.
enum MsmStepKind : uint8_t { STEP_WINDOW = 0, STEP_DENSE = 1, STEP_DENSE_SLICED = 2, STEP_GM = 3 };
struct MsmStep { uint32_t first, cols; MsmStepKind kind; };
enum MsmPlanStatus : int { MSM_PLAN_OK = 0, MSM_PLAN_ENTRY_SPACE = 1 };     // 1: the batch exceeds the 32-bit entry space (no steps)
constexpr int MSM_GRAPH_PIPES = 4;       // pipelines of the graph mode: the context's stream and the three side streams
struct MsmBatchPlan {
    MsmPlanStatus status;
    size_t n, count, tab_stride;
    MsmPlan pl, pn;                 // merged plan; per-window plan (a placeholder when no column is small-valued)
    bool any_narrow;                // some column takes the per-window table (after the 32-bit give-up)
    uint32_t tail_rows;             // blinded tail rows committed apart by k_msm_tails
    uint64_t n_narrow, n_pad;       // rows of a small-valued column in front of its tail; digit-matrix row stride
    uint32_t NG;                    // columns per group
    bool gm;                        // groups go through the GM sort
    uint32_t SG;                    // bucket sets per column of a GM group
    int range_bits_G;
    uint32_t bpcG, perm_G, nwgG;    // GM: partitions per column, bucket numbering, partition workgroups per column
    SortDims dims_N, dims_G, dims_M;
    size_t words_N, words_G, words_M, words;    // of the three layouts; per copy (the largest in use, 256-B aligned)
    int copies;                     // sort workspace copies: one per pipeline
    bool binsort;
    int range_bits;
    uint32_t chunk;
    bool staged_scatter;
    uint32_t nwg;
    int npipe;
    bool graph;
    uint32_t nb, nbN, red_blocks_N, red_pts;    // bucket layout dimensions
    size_t max_tasks, max_tasks_N;
    size_t npts29;                  // points per bucket buffer
    uint32_t smaller_cap;           // the group_cap to try next when the sort workspace cannot be had (0: none)
    std::vector<MsmStep> steps;
};

// the sort layout of a step of `kind`
static const SortDims& sort_dims_of(const MsmBatchPlan& bp, MsmStepKind kind) { return kind == STEP_GM ? bp.dims_G : kind == STEP_WINDOW ? bp.dims_N : bp.dims_M; }
// Bucket regions of a step of `kind` over `cols` columns.  A group's regions are those of a full group of NG columns whatever
// `cols` is -- a shorter last group uses the front of each -- so every buffer of the rotation has ONE layout per kind.
template <class Pt>
static BucketRegions<Pt> carve_buckets(const MsmBatchPlan& bp, MsmStepKind kind, uint32_t cols, Pt* base, std::vector<CarvedRegion>* log = nullptr) {
    if (kind == STEP_DENSE || kind == STEP_DENSE_SLICED) {
        // partial: scratch of the weighted bucket sum (group sums of every level of wsum_enqueue, partials), which also holds the
        // <= nb / 2048 + 1 partials of the one-launch reduction
        BucketRegions<Pt> r = carve_bucket_regions(bp.nb, bp.red_pts, bp.max_tasks, 0, base, log);
        r.nb = bp.nb;
        r.tasks = bp.max_tasks;
        return r;
    }
    const bool gmk = kind == STEP_GM;
    // x 4: the GM path reduces up to four bucket sets per column; it folds nothing (the accumulation already sums the windows)
    BucketRegions<Pt> r = carve_bucket_regions(bp.nbN, (size_t)bp.red_blocks_N * bp.NG * (gmk ? 4 : 1), bp.max_tasks_N, gmk ? 0 : (size_t)bp.pn.B * bp.NG, base, log);
    r.nb = gmk ? cols * bp.SG * bp.pn.B : cols * (uint32_t)bp.pn.W * bp.pn.B;
    r.tasks = (size_t)r.nb + std::max(((size_t)bp.n * cols * bp.pn.W) / TASK_CAP, (size_t)TASK_TARGET) + 1;
    return r;
}

static MsmBatchPlan plan_batch(const MsmBatchShape& sh, const MsmKnobs& kn) {
    MsmBatchPlan bp{};
    const size_t n = sh.n, count = sh.count;
    const MsmPlan& pl = sh.pl;
    bp.n = n; bp.count = count; bp.tab_stride = sh.tab_stride; bp.pl = pl;
    bool any_narrow = false;
    if (sh.pl_n && sh.hints) for (size_t i = 0; i < count; ++i) any_narrow |= sh.hints[i] == 1;
    // the per-window path indexes n * W entries with 32 bits; decided BEFORE the blinded tails are split off: a column that
    // takes the merged path over all n rows must not have its tail committed a second time by k_msm_tails
    if (any_narrow && (uint64_t)n * sh.pl_n->W >= (1ull << 32)) any_narrow = false;
    bp.any_narrow = any_narrow;
    // blinded tails of the hint-1 columns (zk_ctx::msm_blinded_tail): committed by k_msm_tails, the main MSM stops in front of them
    bp.tail_rows = (any_narrow && sh.blinded_tail && (size_t)sh.blinded_tail + 1024 <= n && sh.blinded_tail <= 256) ? sh.blinded_tail : 0u;
    bp.n_narrow = (uint64_t)n - bp.tail_rows;
    // ---- per-window ("narrow") path: sizes and workspace, as in msm_batch_tab with a window table
    const MsmPlan pn = any_narrow ? *sh.pl_n : MsmPlan{4, 64, 8};
    bp.pn = pn;
    // Consecutive small-valued columns share ONE launch sequence: column j of a group owns windows [j W, (j + 1) W) of a
    // (group x W)-window MSM over the same per-window table -- digits, LDS sweeps, scans, task split, accumulation and
    // combination run once per group, the fold / reduction with the column on blockIdx.y.  Such a column is a chain of sixteen
    // small, latency-bound launches (a few hundred thousand entries); a group amortises every launch over up to eight columns
    // (MSM_WFLAGS window flags).  ZK_MSM_NARROW_GROUP=1 turns it off, 2 / 4 / 8 set the group size (measurement knob; 2^20 rows,
    // 30-bit values: 0.68 / 0.51 / 0.43 / 0.38 ms per column, tools/gpu_r3u.sh).
    uint32_t NG = 1;
    if (any_narrow) {
        NG = std::min<uint32_t>((uint32_t)GM_MAX_COLS, MSM_WFLAGS / (uint32_t)pn.W);       // sixteen at c = 16: a group's dozen short launches (scans, size bins, task split) cost the same for eight
                                                                                            // columns or sixteen -- 60/30/10 columns 0.265 -> 0.255 ms each in a batch, the sort 0.81 ms per eight -> 1.45 per sixteen
        if (kn.narrow_group >= 1 && kn.narrow_group <= GM_MAX_COLS) NG = std::min<uint32_t>((uint32_t)kn.narrow_group, MSM_WFLAGS / (uint32_t)pn.W);
        if (sh.group_cap && NG > sh.group_cap) NG = sh.group_cap;
        while (NG > 1 && (uint64_t)n * pn.W * NG >= (1ull << 32)) --NG;
        if (NG < 1) NG = 1;
    }
    bp.NG = NG;
    const uint32_t Wg = (uint32_t)pn.W * NG;
    const uint32_t nbN = Wg * pn.B;
    bp.nbN = nbN;
    const uint64_t n_pad = ((uint64_t)n + 16 * MSM_SLICES - 1) & ~(uint64_t)(16 * MSM_SLICES - 1);
    bp.n_pad = n_pad;
    bp.dims_N = SortDims{nbN, true, 0, (uint64_t)n * Wg, (size_t)(n_pad * Wg + 1) / 2 + 4, false};
    // Groups of small-valued columns, sorted like the merged path ("GM"; ZK_MSM_NARROW_GM=0 keeps the digit matrix + LDS sweeps):
    // the digit matrix of a group is 16 x n codes per column of which a witness-like column fills a tenth, and every row of it
    // was streamed by sixteen range workgroups, twice -- 0.22 ms of sort per column for 0.12 ms of accumulation.  Here the non-zero
    // digits become entries keyed by (column, bucket) -- the per-window table gives every window's bucket b the same weight, so a
    // column needs ONE set of 2^(c-1) buckets, not one per window -- and go through the merged path's partition / one-launch
    // counting sort: column j of the group owns partitions [j * bpc, (j + 1) * bpc) and buckets [j B, (j + 1) B); the fold of the
    // windows disappears (the accumulation already sums them), reduction and window sum run per column as before.
    const bool gm = any_narrow && pn.c >= MSM_M_MIN_C && pn.c <= 16 && NG <= (uint32_t)GM_MAX_COLS && kn.narrow_gm != 0;
    bp.gm = gm;
    // A column's windows are dealt over SG bucket sets (window w -> set w mod SG): a witness-like column (10 % field-sized cells) puts
    // ~2 M entries into its buckets -- 61 per bucket with one set of 2^15, every bucket split into two unequal tasks and put together
    // again afterwards (accumulation + combination 2.2 ms per group of eight against the 1.0 ms the additions cost); with two sets
    // the buckets hold 26-35 entries, one task each.  ZK_MSM_GM_SETS = 1 / 2 / 4 (measurement knob).
    uint32_t SG = 2;
    if (kn.gm_sets == 1 || kn.gm_sets == 2 || kn.gm_sets == 4) SG = (uint32_t)kn.gm_sets;
    bp.SG = SG;
    int range_bits_G = pn.c - 1 - 7;                                  // 128 * SG partitions per column of 2^(c-8) buckets each
    if (range_bits_G < 0) range_bits_G = 0;
    bp.range_bits_G = range_bits_G;
    bp.bpcG = (SG * pn.B) >> range_bits_G;                // partitions per column
    bp.perm_G = ((uint32_t)range_bits_G << 8) | (uint32_t)(pn.c - 1 - range_bits_G);      // the GM sort numbers buckets low bits first (perm_true)
    bp.nwgG = (uint32_t)((bp.n_narrow + MSM_M_CHUNK - 1) / MSM_M_CHUNK);      // partition workgroups per column
    bp.dims_G = SortDims{NG * SG * pn.B, false, NG * bp.bpcG * bp.nwgG, (uint64_t)n * pn.W * NG, 0, true};      // entries, worst case: every digit of every column non-zero
    bp.words_N = any_narrow ? carve_sort_ws(bp.dims_N, nullptr).words : 0;
    bp.words_G = gm ? carve_sort_ws(bp.dims_G, nullptr).words : 0;
    const size_t words_N = std::max(bp.words_N, bp.words_G);
    bp.red_blocks_N = ((pn.B + RED_G_WIDE - 1) / RED_G_WIDE + RED_THREADS - 1) / RED_THREADS;
    bp.max_tasks_N = (size_t)nbN + std::max(((size_t)n * Wg) / TASK_CAP, (size_t)TASK_TARGET) + 1;
    const uint32_t nb = pl.B;
    bp.nb = nb;
    const uint64_t max_entries = (uint64_t)n * pl.W;
    // table indices carry the sign in bit 31, cursors are 32-bit
    if ((uint64_t)pl.W * sh.tab_stride >= (1ull << 31) || max_entries >= (1ull << 32)) { bp.status = MSM_PLAN_ENTRY_SPACE; return bp; }
    int range_bits = pl.c - 1;
    if (range_bits > MSM_RANGE_MAX_BITS) range_bits = MSM_RANGE_MAX_BITS;
    // one-launch partition sort (k_msm_m_binsort) when 1024 partitions are small enough for its LDS staging buffer;
    // ZK_MSM_BINSORT=0 keeps the sliced count / scan / scatter sequence (measurement knob)
    bool binsort = kn.binsort != 0;
    if (binsort) {
        int rb = pl.c - 1 - 10;
        if (rb < 0) rb = 0;
        const uint64_t per_partition = max_entries / (nb >> rb);
        if (per_partition + per_partition / 8 <= MSM_M_STAGE) range_bits = rb;
        else binsort = false;
    }
    bp.binsort = binsort;
    bp.range_bits = range_bits;
    uint32_t chunk = MSM_M_CHUNK;
    if (kn.chunk >= 256 && kn.chunk <= 65536) chunk = (uint32_t)kn.chunk;   // measurement knob
    // scatter with LDS-staged runs (k_msm_m_scatter_staged): window sizes whose 1024 x W entries fit the LDS, and only next to the
    // one-launch partition sort (same 1024-partition layout); ZK_MSM_STAGED=0 keeps the direct scatter (measurement knob)
    bp.staged_scatter = binsort && pl.c >= 19 && scatter_staged_lds(pl.W) <= (size_t)150 * 1024 && kn.staged != 0;
    if (bp.staged_scatter) chunk = MSM_M_SCHUNK;
    bp.chunk = chunk;
    bp.nwg = (uint32_t)((n + chunk - 1) / chunk);
    bp.dims_M = SortDims{nb, true, (nb >> range_bits) * bp.nwg, max_entries, 0, true};
    bp.words_M = carve_sort_ws(bp.dims_M, nullptr).words;
    bp.words = (std::max(bp.words_M, words_N) + 63) & ~(size_t)63;      // per copy: every copy starts 256-B aligned
    // Below 2^20 points an MSM does not fill the device: its sort / accumulation / combination is a chain of some twenty
    // short launches.  Two such chains then run side by side -- even columns on the context's stream, odd columns on the
    // third side stream, each with its own sort workspace -- and hide each other's latency.  ZK_MSM_PIPES overrides.
    bp.npipe = (n <= ((size_t)1 << 19) && count >= 2) ? 2 : 1;
    if (kn.pipes == 1 || (kn.pipes == 2 && count >= 2)) bp.npipe = kn.pipes;
    // Graph mode: the launch sequence of a column is captured once per pipeline and replayed -- at these sizes the
    // host's launch rate, ~30 API calls per column, is what bounds a batch.  ZK_MSM_GRAPH=0 disables it.
    bp.graph = n <= ((size_t)1 << 19) && n >= 1024 && count >= 4 && !sh.prof_on && !sh.graph_broken && kn.graph != 0 && !(any_narrow && NG > 1);
    bp.copies = bp.graph ? MSM_GRAPH_PIPES : bp.npipe;      // one copy per pipeline
    // the sort workspace of the groups is what may not fit: groups of half the size are the next to try
    bp.smaller_cap = (any_narrow && NG > 1 && words_N > bp.words_M) ? NG / 2 : 0;
    bp.red_pts = nb / 4 + 1024;       // scratch of the weighted bucket sum (group sums of every level, partials)
    bp.max_tasks = (size_t)nb + std::max((size_t)(max_entries / TASK_CAP), (size_t)TASK_TARGET) + 1;
    // the steps: up to NG consecutive small-valued columns, or one column alone.  Graph mode has no groups (NG == 1) and sends a
    // small-valued column through the per-window sort; hint 2: long runs of equal scalars (running products) put whole runs into
    // one partition; four slice-workgroups per partition stream them faster than one
    auto is_narrow = [&](size_t it) { return any_narrow && sh.hints[it] == 1; };
    for (size_t it = 0; it < count;) {
        MsmStep s{(uint32_t)it, 1, STEP_DENSE};
        if (is_narrow(it)) {
            while (s.cols < NG && it + s.cols < count && is_narrow(it + s.cols)) ++s.cols;
            s.kind = gm && !bp.graph ? STEP_GM : STEP_WINDOW;
        } else if (!binsort || (sh.hints && sh.hints[it] == 2)) s.kind = STEP_DENSE_SLICED;
        bp.steps.push_back(s);
        it += s.cols;
    }
    // a bucket buffer fits every kind of step the batch has
    for (const MsmStep& s : bp.steps) bp.npts29 = std::max(bp.npts29, carve_buckets<char>(bp, s.kind, NG, nullptr).points);
    return bp;
}

// The plan's part of a graph key (msm_batch_merged adds the step kind, the pipeline and the addresses): every plan value that
// reaches a kernel argument or a grid of a captured step.  The two window sizes fix W, B, the sweep's range bits and -- with
// n and n_narrow -- n_pad, the task bounds and every sort dimension; top_shift, the merged sort's range_bits, nwg and the
// staged scatter are knobs of their own (ZK_MSM_TOP_SHIFT and ZK_MSM_CHUNK change two of them without moving any address);
// tab_stride is the table's; words places the pipeline's workspace copy.  Graph mode has no groups: NG = 1, no GM value.
static std::vector<uint64_t> graph_key_part(const MsmBatchPlan& bp) {
    return {(uint64_t)bp.n, (uint64_t)bp.pl.c, (uint64_t)bp.pn.c, (uint64_t)bp.pl.top_shift, (uint64_t)bp.tab_stride, (uint64_t)bp.words, (uint64_t)bp.staged_scatter, (uint64_t)bp.range_bits,
            bp.n_narrow, (uint64_t)bp.nwg};
}

// ---- the record of zk_host_msm_batch_plan (include/zkmi355.h gives the layout) --------------------------------------------
static std::vector<uint64_t> plan_record(const MsmBatchPlan& bp) {
    std::vector<uint64_t> r = {(uint64_t)bp.status, bp.any_narrow, bp.tail_rows, bp.n_narrow, bp.n_pad, bp.NG, bp.gm, bp.SG, (uint64_t)bp.range_bits_G, bp.bpcG, bp.perm_G, bp.nwgG,
                               bp.words_N, bp.words_G, bp.words_M, bp.words, (uint64_t)bp.copies, bp.binsort, (uint64_t)bp.range_bits, bp.chunk, bp.staged_scatter, bp.nwg,
                               (uint64_t)bp.npipe, bp.graph, bp.npts29, bp.smaller_cap, (uint64_t)bp.pl.c, (uint64_t)bp.pl.W, (uint64_t)bp.pl.top_shift, (uint64_t)bp.pn.c, (uint64_t)bp.pn.W,
                               bp.red_blocks_N};
    if (bp.status != MSM_PLAN_OK) return r;
    std::vector<CarvedRegion> log;
    auto put_log = [&](uint64_t total) {
        r.push_back(total);
        r.push_back(log.size());
        for (const CarvedRegion& g : log) { r.push_back((uint64_t)g.id); r.push_back(g.at); r.push_back(g.len); }
        log.clear();
    };
    const SortDims* dims[3] = {&bp.dims_N, &bp.dims_G, &bp.dims_M};
    const bool used[3] = {bp.any_narrow, bp.gm, true};
    for (int i = 0; i < 3; ++i) {
        const size_t words = used[i] ? carve_sort_ws(*dims[i], nullptr, &log).words : 0;
        put_log(words);
    }
    for (int kind = 0; kind < 4; ++kind) {
        bool present = false;
        for (const MsmStep& s : bp.steps) present |= s.kind == kind;
        BucketRegions<char> b{};
        if (present) b = carve_buckets<char>(bp, (MsmStepKind)kind, bp.NG, nullptr, &log);
        r.push_back(present ? b.nb : 0);
        r.push_back(present ? b.tasks : 0);
        put_log(b.points);
    }
    r.push_back(bp.steps.size());
    for (const MsmStep& s : bp.steps) { r.push_back(s.first); r.push_back(s.cols); r.push_back(s.kind); }
    const std::vector<uint64_t> key = graph_key_part(bp);
    r.push_back(key.size());
    r.insert(r.end(), key.begin(), key.end());
    return r;
}
// the plan zk_host_msm_batch_plan reports: an SRS of 2^k points with its merged table, with or without the per-window one
static MsmBatchPlan plan_batch_of_srs(uint32_t k, size_t n, size_t count, const uint8_t* hints, uint32_t blinded_tail, bool window_table, uint32_t group_cap, bool prof_on, bool graph_broken,
                                      const MsmKnobs& kn) {
    const MsmPlan pln = make_plan((size_t)1 << k);
    std::vector<uint8_t> forced;
    if (kn.narrow != KNOB_UNSET) { forced.assign(count, (uint8_t)(kn.narrow != 0)); hints = forced.data(); }     // as msm_batch_srs applies ZK_MSM_NARROW
    return plan_batch(MsmBatchShape{n, count, (size_t)1 << k, make_plan_merged(k, kn), window_table ? &pln : nullptr, hints, blinded_tail, prof_on, graph_broken, group_cap}, kn);
}

}  // namespace zk

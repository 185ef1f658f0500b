// Context object behind the C ABI (include/zkmi355.h): device, stream, cached NTT domains,
// a growable scratch arena, and the error string.  One host thread per context.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "../../include/zkmi355.h"
#include "ec.hip.hpp"
#include "ff.hip.hpp"

namespace zk {

struct NttDomain;   // ntt.hip

struct Scratch {
    void* ptr = nullptr;
    size_t cap = 0;
};

}  // namespace zk

struct zk_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    std::string err;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    hipDeviceProp_t prop{};
    // scratch arenas, grown on demand (never shrunk): index = purpose
    zk::Scratch scratch[24];
    // side stream + events for pipelining consecutive MSMs (msm.hip): created on first use
    hipStream_t stream2 = nullptr, stream2b = nullptr, stream2c = nullptr;
    std::vector<hipStream_t> owned_streams;      // every stream zk_ctx_create made (roles may share one; 'd' entries of the layout have no role at all)
    hipEvent_t ev_p1[3] = {nullptr, nullptr, nullptr}, ev_p2[3] = {nullptr, nullptr, nullptr};
    std::map<uint64_t, std::vector<uint64_t>> msm_graph_keys;   // the full key behind every hash in msm_graphs (compared on a hit)
    std::map<uint64_t, void*> msm_graphs;   // hipGraphExec_t per (column kind, pipeline, sizes, buffer addresses): msm_batch_merged's graph mode
    uint32_t msm_blinded_tail = 0;          // set by the prover around a commit batch: this many rows at the end of the hint-1 (small-valued) columns
                                            // hold field-sized blinding values; they are committed apart (k_msm_tails) so that the main MSM sees small values only
    bool msm_graph_broken = false;          // a capture or replay failed once: the plain launch path from then on
    hipEvent_t ev_pipe = nullptr;        // joins the second MSM pipeline of small batches (msm_batch_merged)
    // copy stream: host -> device staging of the next column under the current MSM (api.hip)
    hipStream_t stream_copy = nullptr;
    hipEvent_t ev_copy = nullptr;
    // auxiliary compute stream: transforms of freshly uploaded columns run beside the commitment pipeline
    hipStream_t stream_aux = nullptr;
    hipEvent_t ev_aux = nullptr;
    // The auxiliary stream (transforms of freshly uploaded columns beside the commitment pipeline).  ZK_AUX_PRIORITY=1 creates it
    // with the highest stream priority -- a measurement knob, OFF by default: it did not help the sort-ahead experiment
    // (profiles/r03_sort_ahead.md) and it slows the witness uploads of the advice phase from 0.64 to 0.94 ms per 32 MiB column
    // (643 -> 940 ms for the SuperCircuit shape, tools/gpu_r3i.sh): a priority stream takes a hardware queue of its own, and which
    // streams share queues decides the upload rate (DESIGN "stream topology").
    bool ensure_aux() {
        // stream and event are a pair: whoever created the stream (zk_ctx_debug_delay can), the event exists when this returns true
        if (stream_aux) return ev_aux || hipEventCreateWithFlags(&ev_aux, hipEventDisableTiming) == hipSuccess;
        int least = 0, greatest = 0;
        const char* e = getenv("ZK_AUX_PRIORITY");
        const bool prio = e && atoi(e) == 1 && hipDeviceGetStreamPriorityRange(&least, &greatest) == hipSuccess && greatest != least;
        hipError_t rc = prio ? hipStreamCreateWithPriority(&stream_aux, hipStreamNonBlocking, greatest) : hipStreamCreateWithFlags(&stream_aux, hipStreamNonBlocking);
        if (rc != hipSuccess) { (void)hipGetLastError(); rc = hipStreamCreateWithFlags(&stream_aux, hipStreamNonBlocking); }
        if (rc != hipSuccess) { stream_aux = nullptr; return false; }
        if (!ev_aux && hipEventCreateWithFlags(&ev_aux, hipEventDisableTiming) != hipSuccess) return false;
        return true;
    }
    // RCCL communicator of this rank (comm.hip; opaque here so that rccl.h stays out of the other translation units)
    void* comm = nullptr;
    uint32_t comm_rank = 0, comm_world = 1;
    std::map<uint64_t, std::shared_ptr<zk::NttDomain>> domains;   // key: log_n | kind << 8
    std::map<uint64_t, void*> pow_tables;                         // cached two-level power tables of the coset generators
    void* poseidon_tab = nullptr;                                 // the width-3 Poseidon constants as limb records (poseidon.hip), built on first use
    void* key_inv_tab = nullptr;                                  // the inverses of 0..65535 as Montgomery Fr (keysort.hip: ZK_OP_KEY_ORDER), made on the device at first use
    std::map<const void*, void*> loop_records;                    // measurement only (ZK_QUOTIENT_LOOP_RECORDS, quotient.hip): column buffer -> its image as a coset record buffer
    std::vector<void*> pinned;   // small pinned host staging buffers
    // Device block pool for the prover's column buffers: a proof allocates and frees hundreds of
    // n x 32 B / 2^ext_k x 32 B blocks, and hipFree is a device-wide synchronisation.  Blocks are
    // recycled by exact size; every user is ordered on `stream`, so reuse needs no extra fence.
    std::map<size_t, std::vector<void*>> pool;
    size_t pool_bytes = 0, pool_cap = (size_t)96 << 30;
    size_t coset_cache_bytes = 0;        // device memory held by the coset caches of every proving key alive on this context (prover.hip)
    void* pool_get(size_t bytes) {
        bytes = (bytes + 255) & ~(size_t)255;
        if (!bytes) bytes = 256;
        auto it = pool.find(bytes);
        if (it != pool.end() && !it->second.empty()) { void* p = it->second.back(); it->second.pop_back(); pool_bytes -= bytes; return p; }
        void* p = nullptr;
        if (hipMalloc(&p, bytes) == hipSuccess) return p;
        (void)hipGetLastError();
        pool_trim();                                   // give cached blocks back and retry once
        if (hipMalloc(&p, bytes) == hipSuccess) return p;
        (void)hipGetLastError();
        return nullptr;
    }
    void pool_put(void* p, size_t bytes) {
        if (!p) return;
        bytes = (bytes + 255) & ~(size_t)255;
        if (!bytes) bytes = 256;
        if (pool_bytes + bytes > pool_cap) { (void)hipStreamSynchronize(stream); (void)hipFree(p); return; }
        pool[bytes].push_back(p);
        pool_bytes += bytes;
    }
    void pool_trim() {
        (void)hipStreamSynchronize(stream);
        for (auto& kv : pool) for (void* p : kv.second) (void)hipFree(p);
        pool.clear();
        pool_bytes = 0;
    }
    // per-kernel HIP-event profiling (zk_prof_*): off by default
    uint32_t msm_attr_set = 0;            // bit C: k_msm_m_scatter_staged<C> has its dynamic-LDS attribute on this device
    bool quotient_attr_set = false;       // hipFuncSetAttribute (large dynamic LDS) is per device: remembered per context, not per process
    std::map<const void*, bool> ntt_fixed_attr;   // the same for every NTT pass kernel, generic or compile-time instance (ntt.hip, pass_kernel_ready): kernel -> the device took the LDS size (false: that kernel stays unused)
    bool prof_on = false;
    bool prof_main_only = false;         // zk_prof_enable(ctx, 2): only the scopes of the roofline kernels (accumulation, transforms, evaluator) record events
    const char* prof_tag = nullptr;      // when set, zk_quotient_eval books its launch under this name (the prover tags the big coset programs)
    struct ProfEntry { double ms = 0; uint64_t count = 0; uint64_t bytes = 0; };   // bytes: algorithmic HBM bytes of the booked launches, where the scope states them
    std::map<std::string, ProfEntry> prof;
    struct ProfPending { const char* name; hipEvent_t a, b; uint64_t bytes; };
    std::vector<ProfPending> prof_pending;
    std::vector<hipEvent_t> prof_pool;
    hipEvent_t prof_event() {
        if (!prof_pool.empty()) { hipEvent_t e = prof_pool.back(); prof_pool.pop_back(); return e; }
        hipEvent_t e = nullptr;
        (void)hipEventCreate(&e);
        return e;
    }
    void prof_resolve() {
        for (auto& p : prof_pending) {
            float ms = 0;
            if (hipEventSynchronize(p.b) == hipSuccess && hipEventElapsedTime(&ms, p.a, p.b) == hipSuccess) {
                auto& e = prof[p.name];
                e.ms += ms;
                e.count += 1;
                e.bytes += p.bytes;
            }
            prof_pool.push_back(p.a);
            prof_pool.push_back(p.b);
        }
        prof_pending.clear();
    }

    int fail(int code, const char* fmt, ...) {
        char buf[512];
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(buf, sizeof buf, fmt, ap);
        va_end(ap);
        err = buf;
        return code;
    }
    // returns nullptr on failure (err set)
    void* get_scratch(int slot, size_t bytes) {
        zk::Scratch& s = scratch[slot];
        if (s.cap >= bytes) return s.ptr;
        if (s.ptr) { (void)hipStreamSynchronize(stream); (void)hipFree(s.ptr); s.ptr = nullptr; s.cap = 0; }
        size_t want = bytes + bytes / 4;
        hipError_t e = hipMalloc(&s.ptr, want);
        if (e != hipSuccess) { (void)hipGetLastError(); e = hipMalloc(&s.ptr, bytes); want = bytes; }
        if (e != hipSuccess) { s.ptr = nullptr; fail(ZK_ERR_OOM, "scratch alloc of %zu bytes failed: %s", bytes, hipGetErrorString(e)); return nullptr; }
        s.cap = want;
        return s.ptr;
    }
};

// RAII scope: records a HIP event pair around the enclosed launches on ctx->stream
struct ZkProfScope {
    // level 2 (what bench.py's timed region runs under): every MSM class (merged and grouped bucket launches, sorts, reductions), the NTT passes, the evaluator
    static bool is_main(const char* n) { return !strncmp(n, "msm_", 4) || !strncmp(n, "ntt_", 4) || !strncmp(n, "quotient", 8); }
    zk_ctx* c; const char* name; hipEvent_t a = nullptr; hipStream_t s; uint64_t bytes = 0;
    ZkProfScope(zk_ctx* ctx, const char* n, hipStream_t on = nullptr) : c(ctx), name(n), s(on ? on : ctx->stream) {
        if (c->prof_on && (!c->prof_main_only || is_main(n))) { a = c->prof_event(); (void)hipEventRecord(a, s); }
    }
    ~ZkProfScope() {
        if (a) { hipEvent_t b = c->prof_event(); (void)hipEventRecord(b, s); c->prof_pending.push_back({name, a, b, bytes}); }
    }
};

struct zk_srs {
    uint32_t k = 0;
    zk::G1Affine* g = nullptr;
    zk::G1Affine* g_lagrange = nullptr;
    // lazily built copies in R' = 2^261 Montgomery form (the MSM kernels' native base format)
    zk::G1Affine* g_rp = nullptr;
    zk::G1Affine* g_lagrange_rp = nullptr;
    // lazily built fixed-base window tables [W][2^k] (R' form) and the window size they were built for
    // basis index 2 = the prefix sums of the Lagrange basis (pfx[1]) used as a basis of its own: columns committed through
    // their first differences (runs.hip)
    zk::G1Affine* tab[3] = {nullptr, nullptr, nullptr};
    zk::G1Affine* tabn[3] = {nullptr, nullptr, nullptr};   // per-window tables (c <= 16) for the columns that fill few windows
    zk::G1Affine* pfx[2] = {nullptr, nullptr};    // prefix sums of a basis (R' form), for run-structured columns (runs.hip)
    int tab_c[3] = {0, 0, 0};
    int tab_shift[3] = {0, 0, 0};   // and the top-window shift baked into its top window (MsmPlan::top_shift)
    zk::G1Affine* pfx_negtot[2] = {nullptr, nullptr};   // one point on the device: -(sum of pfx[b][j], j <= 2^k - 2), R' form
    zk::G1Affine* pfx_negtot_tab[2] = {nullptr, nullptr};   // its fixed-base table: [32 byte windows][256 digits] = digit * 2^(8 w) * point, R' form (runs.hip: k_fixed_mul)
};

#define ZK_HIP(ctx, call)                                                                          \
    do {                                                                                           \
        hipError_t e__ = (call);                                                                   \
        if (e__ != hipSuccess) return (ctx)->fail(ZK_ERR_HIP, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e__), __FILE__, __LINE__); \
    } while (0)

#define ZK_CHECK_LAUNCH(ctx)                                                                       \
    do {                                                                                           \
        hipError_t e__ = hipGetLastError();                                                        \
        if (e__ != hipSuccess) return (ctx)->fail(ZK_ERR_HIP, "kernel launch failed: %s (%s:%d)", hipGetErrorString(e__), __FILE__, __LINE__); \
    } while (0)

#define ZK_REQUIRE(ctx, cond, msg)                                                                 \
    do {                                                                                           \
        if (!(cond)) return (ctx)->fail(ZK_ERR_INVALID_ARG, "invalid argument: %s (%s:%d)", msg, __FILE__, __LINE__); \
    } while (0)

namespace zk {
enum ScratchSlot { SC_NTT = 0, SC_MSM_KEYS = 1, SC_MSM_BUCKETS = 2, SC_MSM_MISC = 3, SC_POLY = 4, SC_POLY2 = 5, SC_TMP = 6, SC_TMP2 = 7, SC_MSM_BUCKETS2 = 8, SC_MSM_RESULTS = 9, SC_QTMP = 10, SC_COMM = 11, SC_MSM_BUCKETS3 = 12, SC_MSM_BUCKETS4 = 13, SC_MSM_DESC = 14, SC_MSM_TAILS = 15, SC_NTT_AUX = 16, SC_QACC = 17, SC_QSLICE = 18, SC_KEYSORT = 19, SC_BYTECODE = 20, SC_COPY = 21, SC_EXP = 22, SC_CODE_HASH = 23 };

// host-side field helpers (slow path, used for constants / tables only)
Fr fr_from_u64(uint64_t v);
Fr fr_pow(Fr base, uint64_t e);
Fr fr_inv_host(const Fr& a);
Fr fr_root_of_unity(uint32_t log_n);   // ROOT_OF_UNITY^(2^(28-log_n))
Fr fr_zeta();

// internal entry points shared between translation units
int ntt_run(zk_ctx* ctx, Fr* d_data, uint32_t log_n, const Fr& omega, const Fr* scale /*nullable*/, const Fr* coset_pre /*nullable: a[i] *= g^i before*/, const Fr* coset_post /*nullable: out[i] *= g^i after*/,
            const Fr* d_src = nullptr /*nullable: read the input from here, d_data receives the result*/,
            bool fuse_pre = false /*coset_pre from a cached full power table inside the first pass (no separate sweep)*/);
// `count` transforms over one domain, NTT_BATCH columns per launch (d_srcs nullable: in place)
int ntt_run_many(zk_ctx* ctx, Fr* const* d_datas, const Fr* const* d_srcs, size_t count, uint32_t log_n, const Fr& omega, const Fr* scale, const Fr* coset_pre, const Fr* coset_post, bool fuse_pre);
// the same with the output format chosen: records = the last pass writes coset records (ff29.hip.hpp REC29_BYTES per row, out of place only)
int ntt_run_many_fmt(zk_ctx* ctx, Fr* const* d_datas, const Fr* const* d_srcs, size_t count, uint32_t log_n, const Fr& omega, const Fr* scale, const Fr* coset_pre, const Fr* coset_post, bool fuse_pre,
                     bool records);
// Coset operands of the quotient's class programs, packed (what the exported functions of these names do) or as records of 32 x the
// value (R' = 2^261 form, canonical limbs): zk_coeff_to_coset_batch, zk_fr_powers and zk_quotient_eval with the format chosen.
// quotient_eval_fmt with records: EVERY column is a record buffer of 2^ext_k rows, the result is packed and holds 32 x the value.
int coeff_to_coset_batch_fmt(zk_ctx* ctx, const void* const* d_coeffs, uint32_t k, const Fr& g, void* const* d_outs, size_t count, bool records);
int fr_powers_fmt(zk_ctx* ctx, const Fr& base, const Fr& mul, void* d_out, size_t n, bool records);
int quotient_eval_fmt(zk_ctx* ctx, const uint32_t* h_program, uint32_t num_instr, const void* const* h_col_ptrs, uint32_t num_cols, const void* h_consts, uint32_t num_consts, uint32_t k, uint32_t ext_k,
                      int divide_by_vanishing, void* d_out, bool records);
int fr_scale_run(zk_ctx* ctx, Fr* d_a, const Fr& s, uint64_t n);
int fr_row_rlc_run(zk_ctx* ctx, const zk_row_rlc* desc, const void* h_k, Fr* d_out, uint64_t n);       // typed_rows.hip: ZK_OP_ROW_RLC of zk_field_vec_op
int fr_row_inv0_run(zk_ctx* ctx, const zk_row_inv0* desc, const void* h_k, Fr* d_out, uint64_t n);     // typed_rows.hip: ZK_OP_ROW_INV0 of zk_field_vec_op
int fr_poseidon_run(zk_ctx* ctx, const zk_poseidon* desc, const void* h_scale, Fr* d_out, uint64_t n);   // poseidon.hip: ZK_OP_POSEIDON of zk_field_vec_op
int fr_keccak_run(zk_ctx* ctx, const zk_keccak* desc, const void* h_challenges, Fr* d_out, uint64_t n);   // keccak.hip: ZK_OP_KECCAK of zk_field_vec_op
int fr_sha256_run(zk_ctx* ctx, const zk_sha256* desc, const void* h_challenges, Fr* d_out, uint64_t n);   // sha256.hip: ZK_OP_SHA256 of zk_field_vec_op
int key_sort_run(zk_ctx* ctx, const zk_key_sort* desc, const void* h_mask, void* d_out, uint64_t n);   // keysort.hip: ZK_OP_KEY_SORT of zk_field_vec_op
int key_order_run(zk_ctx* ctx, const zk_key_order* desc, void* d_out, uint64_t n);                     // keysort.hip: ZK_OP_KEY_ORDER of zk_field_vec_op
int bytecode_rows_run(zk_ctx* ctx, const zk_bytecode_rows* desc, const void* h_empty, void* d_out, uint64_t n);   // bytecode_rows.hip: ZK_OP_BYTECODE_ROWS of zk_field_vec_op
void bc_scan(zk_ctx* ctx, uint32_t* w, uint64_t count, uint32_t* tmp, uint32_t cap);   // bytecode_rows.hip: exclusive scan in place under the sum that saturates at cap
int copy_rows_run(zk_ctx* ctx, const zk_copy_rows* desc, const void* h_b, void* d_out, uint64_t n);   // copy_rows.hip: ZK_OP_COPY_ROWS of zk_field_vec_op
int copy_rlc_run(zk_ctx* ctx, const zk_copy_rlc* desc, const void* h_challenges, void* d_out, uint64_t n);   // copy_rows.hip: ZK_OP_COPY_RLC of zk_field_vec_op
int exp_rows_run(zk_ctx* ctx, const zk_exp_rows* desc, const void* h_b, void* d_out, uint64_t n);   // exp_rows.hip: ZK_OP_EXP_ROWS of zk_field_vec_op
int code_hash_rows_run(zk_ctx* ctx, const zk_code_hash_rows* desc, const void* h_b, void* d_out, uint64_t n);     // code_hash_rows.hip: ZK_OP_CODE_HASH_ROWS of zk_field_vec_op
int code_hash_table_run(zk_ctx* ctx, const zk_code_hash_table* desc, const void* h_b, void* d_out, uint64_t n);   // code_hash_rows.hip: ZK_OP_CODE_HASH_TABLE of zk_field_vec_op
// G1 encodings read on the device (params.hip k_g1_decode): 32 B compressed, 64 B Montgomery limbs, 64 B big-endian x || y (EVM)
enum G1Enc : int { G1_ENC_COMPRESSED = 0, G1_ENC_RAW = 1, G1_ENC_BE_XY = 2 };
int g1_decode_run(zk_ctx* ctx, const void* d_in, int enc, G1Affine* d_out, uint64_t n, uint32_t* d_bad, uint8_t* d_bad_at);
int msm_run(zk_ctx* ctx, const Fr* d_scalars, const G1Affine* d_bases, size_t n, G1Affine* h_out);
int msm_run_rp(zk_ctx* ctx, const Fr* d_scalars, const G1Affine* d_bases, const G1Affine* d_bases_rp, size_t n, G1Affine* h_out);
int msm_batch_rp(zk_ctx* ctx, const Fr* const* d_scalar_ptrs, size_t count, const G1Affine* d_bases, const G1Affine* d_bases_rp, size_t n, G1Affine* h_out);
// out[s] = sum over [h_off[s], h_off[s + 1]) of scalars[i] * bases[i], arbitrary bases, one pass and one download for all segments
int msm_segments_run(zk_ctx* ctx, const Fr* d_scalars, const G1Affine* d_bases, const uint32_t* h_off, size_t num_segments, G1Affine* h_out);
int srs_bases_rp(zk_ctx* ctx, const zk_srs* srs, int basis, const G1Affine** out);
int srs_window_table(zk_ctx* ctx, const zk_srs* srs, int basis, size_t n, const G1Affine** out, size_t* stride);
// stage(user, it) makes the scalars of MSM `it` available (ordered before the main stream's next
// launches); it is called with 0 before the first MSM and with it + 1 once MSM `it` is enqueued,
// so an upload on the copy stream runs under the previous MSM.
typedef int (*MsmStageFn)(void* user, size_t it);
int msm_batch_tab(zk_ctx* ctx, const Fr* const* d_scalar_ptrs, size_t count, const G1Affine* d_bases, const G1Affine* d_bases_rp, const G1Affine* d_table, size_t tab_stride,
                  size_t n, G1Affine* h_out, MsmStageFn stage = nullptr, void* stage_user = nullptr);
int msm_batch_srs(zk_ctx* ctx, const zk_srs* srs, int basis, const Fr* const* d_scalar_ptrs, size_t count, size_t n, G1Affine* h_out, MsmStageFn stage = nullptr, void* stage_user = nullptr,
                  const uint8_t* narrow = nullptr /*per column: scalars fill few windows*/);
// runs.hip: commits the columns hinted as run-structured that do have few runs (done[i] = 1), leaves the others to the caller
int msm_runs_try(zk_ctx* ctx, const zk_srs* srs, int basis, const Fr* const* d_scalar_ptrs, size_t count, size_t n, const uint8_t* narrow, G1Affine* h_out, uint8_t* done);
int msm_diff_try(zk_ctx* ctx, const zk_srs* srs, int basis, const Fr* const* d_scalar_ptrs, size_t count, size_t n, const uint8_t* narrow, G1Affine* h_out, uint8_t* done);
int commit_batch_staged(zk_ctx* ctx, const zk_srs* srs, int basis, const void* const* d_scalar_ptrs, size_t count, size_t n, void* h_out_affine, MsmStageFn stage, void* stage_user, const uint8_t* narrow = nullptr);
void sample_narrow(const void* const* h_cols, size_t count, size_t n, uint8_t* narrow);   // host sampling of Montgomery-form columns: 1 = at most a quarter of the sampled values are >= 2^64
int sample_narrow_dev(zk_ctx* ctx, const void* const* d_cols, size_t count, size_t n, uint8_t* narrow);   // the same for columns resident on the device
int sample_narrow_dev_typed(zk_ctx* ctx, const void* const* d_cols, const uint8_t* widths, size_t count, size_t n, size_t rows, uint8_t* narrow);   // typed columns on the device: <= 8 bytes small by construction, 16 judged over `rows` packed cells, 32 as sample_narrow_dev
int lookup_multiplicities_enqueue(zk_ctx* ctx, const Fr* const* d_inputs, size_t num_inputs, const Fr* d_table, size_t usable_rows, Fr* d_m, size_t n, uint32_t* d_status, bool reuse_hash = false,
                                  bool one_launch = false);   // lookup.hip, no sync
// One theta-compressed tuple of a lookup argument (lookup.hip k_lk_compress_many): `width` elements, most significant power of theta first.
// Element i is col[i] read at rotation rot[i] (LK_ELEM_CONST: col[i] points at ONE value on the device), times fac[i] at frot[i] where fac[i]
// is set; common: every element carries fac[0] / frot[0], applied once to the sum.
constexpr uint32_t LK_TUPLE_MAX = 16, LK_ELEM_CONST = 1;
struct LkTuple {
    const Fr* col[LK_TUPLE_MAX];
    const Fr* fac[LK_TUPLE_MAX];
    int32_t rot[LK_TUPLE_MAX], frot[LK_TUPLE_MAX];
    uint32_t flags[LK_TUPLE_MAX];
    Fr* dst;
    uint32_t width, common;
};
int lookup_compress_many_enqueue(zk_ctx* ctx, const LkTuple* d_descs, size_t count, const void* h_theta, size_t n);   // lookup.hip, no sync
// The logUp running sums of a batch of arguments (vec.hip).  Argument a: phi[0] = 0, phi[i + 1] = phi[i] + sum_j inv_f[j n + i] - m[i] inv_t[i],
// with inv_f its N inverted input columns, one behind the other.
struct LkSum { const Fr* m; const Fr* inv_t; const Fr* inv_f; Fr* phi; uint64_t N; };
int fr_batch_invert_from(zk_ctx* ctx, const Fr* const* d_src, const void* h_beta, uint32_t log_n, Fr* d_inv, size_t slots);   // d_inv[s n + i] = 1 / (d_src[s][i] + beta), zero where that is zero; d_src on the device
int lookup_sums_enqueue(zk_ctx* ctx, const LkSum* d_args, size_t count, size_t n);   // d_args on the device; enqueued, no sync
// row checks of zk_mock_verify (lookup.hip; enqueued on the context's stream, no sync)
struct MockFail { uint32_t kind, index, sub, row; };          // == zk_mock_failure
int mock_hash_build(zk_ctx* ctx, const Fr* d_table, size_t rows, int scratch_slot, const uint32_t** slots_out, uint32_t* mask_out);
int mock_nonzero_enqueue(zk_ctx* ctx, const Fr* d_vals, const uint32_t* d_row_ids, uint32_t count, uint32_t kind, uint32_t index, uint32_t sub, MockFail* d_out, uint32_t cap, uint32_t* d_counter);
int mock_probe_enqueue(zk_ctx* ctx, const Fr* d_inputs, const Fr* d_table, const uint32_t* d_slots, uint32_t mask, const uint32_t* d_row_ids, uint32_t count,
                       uint32_t kind, uint32_t index, uint32_t sub, MockFail* d_out, uint32_t cap, uint32_t* d_counter);
int mock_perm_enqueue(zk_ctx* ctx, const Fr* const* d_sigma, const Fr* const* d_cols, const Fr* d_ids, const uint32_t* d_slots, uint32_t mask, uint32_t num_cols, uint32_t k,
                      uint32_t kind, MockFail* d_out, uint32_t cap, uint32_t* d_counter);
int fr_add_const_many(zk_ctx* ctx, const void* const* d_src, void* const* d_dst, size_t count, const void* h_k, size_t n);   // vec.hip: dst[c] = src[c] + k, any number of columns, no upload / sync
int fr_from_uint_run(zk_ctx* ctx, hipStream_t stream, const void* d_packed, uint32_t width, uint64_t n, Fr* d_out);   // typed_rows.hip: zk_fr_from_uint on any stream of the context (validates width and alignment)
int fr_from_uint_batch_run(zk_ctx* ctx, hipStream_t stream, const void* const* d_packed, const uint8_t* widths, size_t count, uint64_t n, Fr* const* d_out);   // typed_rows.hip: count columns of n cells each, sixteen per launch (validates every width and alignment before the first launch)
int sigma_from_mapping_run(zk_ctx* ctx, hipStream_t stream, const void* const* d_map, size_t count, uint64_t n, uint32_t P, const Fr* d_omega, const Fr* d_delta, uint32_t* d_bad, Fr* const* d_out);   // vec.hip: count sigma columns of n cells from halo2's permutation mapping, (u32 j', u32 i') per cell, sixteen per launch; a pair outside [0, P) x [0, n) stores zero and sets *d_bad
int g_to_lagrange(zk_ctx* ctx, const G1Affine* d_g, uint32_t k, G1Affine* d_out);   // ecntt.hip: inverse FFT over G1
bool comm_ready(const zk_ctx* ctx);                                                              // comm.hip: in-library RCCL collectives
int comm_allgather_dev(zk_ctx* ctx, const void* d_send, size_t bytes, void* d_recv);             // stream-ordered, no host sync
int comm_allgather_host(zk_ctx* ctx, const void* h_send, size_t bytes, void* h_recv);           // small host buffers, returns complete
int comm_alltoall_dev(zk_ctx* ctx, const void* d_send, size_t bytes_per_peer, void* d_recv);
void comm_release(zk_ctx* ctx);
int copy_stream_open(zk_ctx* ctx);      // copy stream starts after everything enqueued on the main stream so far
int copy_stream_fence(zk_ctx* ctx);     // main stream continues after everything enqueued on the copy stream so far
}  // namespace zk

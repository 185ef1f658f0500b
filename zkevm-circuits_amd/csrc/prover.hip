// Host orchestration of a full PLONKish/KZG proof on top of the device kernels: the surface of
// halo2_proofs::plonk::{keygen_pk, create_proof} with the GWC (poly::kzg::multiopen::ProverGWC,
// what BASELINE.json's north_star names) or SHPLONK (ProverSHPLONK, what the reference's call
// sites instantiate) multi-open.  External crate;
// reference call sites [REF circuit-benchmarks/src/super_circuit.rs:109-132],
// [REF prover/src/common/prover/utils.rs:31,55].
//
// What runs where:
//   device : every commitment (MSM), every NTT / coset NTT, expression evaluation over Lagrange
//            rows and over the cosets of the extended domain (quotient.hip), lookup multiplicities
//            (lookup.hip), batch inversion, grand product / grand sum scans, the blinding
//            polynomial (ChaCha20 counter mode), polynomial evaluation, Kate division, linear
//            combinations
//   host   : transcript (built-in Blake2b or the caller's object through a callback table), the
//            blinding-row RNG (XorShift), program assembly, a handful of scalar field operations
//            per challenge; for multi-GPU sessions the all-gather callbacks
// The key blob's constraint system is parsed by cs.hip; the quotient's plan (degree classes, class programs) is made by
// quotient_plan.hip from the constraint system and the knobs alone, and kept here per key (zk_pk::qplan).
//
// Protocol (mv-lookup/logUp lookups as in the Scroll halo2 fork, SURVEY note L):
//   vk_repr, instances | per phase: advice commitments, the phase's challenges | theta |
//   m commitments | beta, gamma | permutation Z commitments | lookup phi commitments |
//   random poly | y | h pieces | x | evaluations | GWC: v, witnesses  or  SHPLONK: y, v, h, u, pi.
// The matching verifier is oracle/plonk_verifier.py; oracle/plonk_prover.py restates this file over
// Python integers and the tests require both to produce the same proof bytes.
//
// The circuit arrives as a flat "pk blob" (zkevm-circuits_amd/plonk.py serialises it, the Rust shim
// fills it from halo2's ConstraintSystem; layout in INTEGRATION.md, SURVEY 8f-1 export format):
// header, phases, the advice / fixed / instance query lists in halo2's registration order (the order
// of the evaluations in the proof), permutation columns, constants, gate programs, lookup arguments
// (one table tuple and one or more input tuples each, as chunk_lookups() leaves them), fixed columns
// and sigma columns in Lagrange form.
#include <algorithm>
#include <array>
#include <unordered_map>
#include <unordered_set>
#include <memory>
#include <string>

#include <chrono>
#include <cstdlib>
#include <random>
#include <tuple>
#include <functional>
#include "ctx.hpp"
#include "ff29.hip.hpp"
#include "host_hash.hpp"
#include "cs.hpp"
#include "quotient_plan.hpp"
#include "quotient_lower.hpp"

using namespace zk;
using zk::host::F4;
using namespace zk::cs;
using namespace zk::qplan;

extern "C" int zk_quotient_eval(zk_ctx*, const uint32_t*, uint32_t, const void* const*, uint32_t, const void*, uint32_t, uint32_t, uint32_t, int, void*);
extern "C" int zk_fr_powers(zk_ctx*, const void*, const void*, void*, size_t);
extern "C" int zk_ntt(zk_ctx*, void*, uint32_t, int);
extern "C" int zk_fr_batch_invert(zk_ctx*, void*, size_t);
extern "C" int zk_fr_random(zk_ctx*, const uint8_t*, uint64_t, uint64_t, void*, size_t);
extern "C" int zk_lookup_multiplicities(zk_ctx*, const void*, const void*, size_t, void*, size_t, uint64_t*);
extern "C" int zk_coeff_to_coset(zk_ctx*, const void*, uint32_t, const void*, void*);
extern "C" int zk_coeff_to_coset_batch(zk_ctx*, const void* const*, uint32_t, const void*, void* const*, size_t);
extern "C" int zk_fr_scatter_scaled(zk_ctx*, const void*, size_t, const void*, void*, size_t, size_t);
extern "C" int zk_msm_g1(zk_ctx*, const void*, const void*, size_t, void*);
extern "C" int zk_g1_sum_host(const void*, size_t, void*);
extern "C" int zk_poly_eval_batch(zk_ctx*, const void* const*, size_t, size_t, const void*, void*);
extern "C" int zk_poly_eval_pairs(zk_ctx*, const void* const*, const uint32_t*, size_t, const void*, size_t, size_t, void*);

namespace {

// Inside a PoolScope (the proof-session entry points) DevBuf blocks come from and return to the
// context's block pool; outside (key generation: buffers that live as long as the key) they are
// plain hipMalloc / hipFree.  A session must not outlive its context.
static thread_local zk_ctx* tl_pool_ctx = nullptr;
struct PoolScope {
    zk_ctx* prev;
    explicit PoolScope(zk_ctx* c) : prev(tl_pool_ctx) { tl_pool_ctx = c; }
    ~PoolScope() { tl_pool_ctx = prev; }
};

struct DevBuf {
    void* p = nullptr;
    size_t bytes = 0;
    zk_ctx* owner = nullptr;
    bool borrowed = false;
    DevBuf() {}
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    DevBuf(DevBuf&& o) noexcept : p(o.p), bytes(o.bytes), owner(o.owner), borrowed(o.borrowed) { o.p = nullptr; o.borrowed = false; }
    DevBuf& operator=(DevBuf&& o) noexcept { if (this != &o) { release(); p = o.p; bytes = o.bytes; owner = o.owner; borrowed = o.borrowed; o.p = nullptr; o.borrowed = false; } return *this; }
    ~DevBuf() { release(); }
    void release() {
        if (!p) return;
        if (borrowed) { p = nullptr; borrowed = false; return; }
        if (owner) owner->pool_put(p, bytes); else (void)hipFree(p);
        p = nullptr;
    }
    // a view of somebody else's block (never released through this object)
    void borrow(void* q) { release(); p = q; borrowed = true; }
    bool alloc(size_t n) {
        release();
        bytes = n;
        owner = tl_pool_ctx;
        if (owner) { p = owner->pool_get(n); return p != nullptr; }
        return hipMalloc(&p, n ? n : 1) == hipSuccess;
    }
    // plain hipMalloc / hipFree even inside a PoolScope (buffers that outlive the session, e.g. the key's coset cache)
    bool alloc_unpooled(size_t n) {
        release();
        bytes = n;
        owner = nullptr;
        return hipMalloc(&p, n ? n : 1) == hipSuccess;
    }
    Fr* fr() const { return (Fr*)p; }
};

// page-locked host staging (blinding rows): an asynchronous copy from pageable memory blocks the
// host until the stream reaches it, which would serialise the upload pipeline with the enqueueing thread
struct PinnedBuf {
    void* p = nullptr;
    ~PinnedBuf() { if (p) (void)hipHostFree(p); }
    bool alloc(size_t bytes) { return hipHostMalloc(&p, bytes ? bytes : 1, hipHostMallocDefault) == hipSuccess; }
};


// ZK_PROVER_TRACE=1: wall-clock per prover stage on stderr (device drained at every mark)
struct StageTrace {
    zk_ctx* ctx; bool on; std::chrono::steady_clock::time_point t0;
    explicit StageTrace(zk_ctx* c) : ctx(c), on(getenv("ZK_PROVER_TRACE") != nullptr), t0(std::chrono::steady_clock::now()) {}
    void mark(const char* what) {
        if (!on) return;
        (void)hipStreamSynchronize(ctx->stream);
        const auto t1 = std::chrono::steady_clock::now();
        fprintf(stderr, "[zk prover] %-28s %8.2f ms\n", what, std::chrono::duration<double, std::milli>(t1 - t0).count());
        t0 = t1;
    }
};

}  // namespace

struct zk_pk : zk::cs::ConstraintSystem {   // the constraint system (cs.hpp) and what keygen derives from it
    // device-resident key material
    std::vector<DevBuf> fixed_lag, fixed_coeff, sigma_lag, sigma_coeff;
    DevBuf omega_lag, l0_lag, llast_lag, lactive_lag, l0_coeff, llast_coeff, lactive_coeff;
    // cosets of the key's own columns (fixed, sigma, l0 / l_last / l_active, X), filled by the first
    // proof and reused by later ones when they fit the budget (ZK_PK_COSET_CACHE_GB, default 96):
    // part_cache[r][column reference].  Plain device allocations owned by the key (a slot appears
    // only once it is filled).  A key serves one proving thread at a time, as its context does.
    mutable std::vector<std::unordered_map<uint32_t, DevBuf>> part_cache;
    mutable int part_cache_state = -1;       // -1 undecided, 0 off, 1 on, 2 frozen (slots that exist are used, no new ones: an allocation failed)
    mutable size_t part_cache_bytes = 0;     // what this key's slots hold of the context's shared budget (zk_ctx::coset_cache_bytes)
    mutable bool part_cache_records = false; // the slots hold coset records (quotient_records below); a session of the other format empties the cache and fills it again
    std::vector<G1Affine> fixed_com, sigma_com;
    F4 vk_repr;                              // vk.transcript_repr: the default, or what zk_pk_set_transcript_repr installed
    const zk_srs* srs = nullptr;
    mutable std::shared_ptr<const QuotientPlan> qplan;      // the quotient's plan (degree classes, class programs), made on first use
};

struct zk_proof {
    const zk_pk* pk;
    host::XorShiftRng rng;
    host::Transcript tr;
    std::vector<DevBuf> inst_lag, inst_coeff, adv_lag, adv_coeff;
    // Cosets of advice columns computed AHEAD, during the advice phases (the uploads are PCIe-bound and leave the device idle for
    // part of every column; which coset reads which column is a property of the key, advice_coset_plan): adv_coset[r][column],
    // empty where nothing was precomputed.  pre_mask[column] = cosets to precompute (bit r), chosen once per session.
    std::vector<std::vector<DevBuf>> adv_coset;
    std::vector<uint32_t> pre_mask;
    bool pre_planned = false;
    int coset_fmt = -1;                       // what adv_coset holds: -1 nothing yet, 0 packed elements, 1 coset records (session_records)
    uint32_t phase = 0;
    int multiopen = ZK_MULTIOPEN_GWC;
    int vanishing_random = ZK_VANISHING_ONE;
    bool advice_on_device = false;            // the witness came as device buffers (zk_proof_advice_phase_dev)
    bool advice_in_place = false;             // the Lagrange forms of the advice columns are the caller's device buffers (zk_proof_advice_phase_dev, IN_PLACE)
    bool lag_partial = false;                 // sharded session: some advice columns of other ranks arrived in coefficient form only (nothing on this side of the boundary reads their Lagrange form)
    // multi-GPU sharding (one process per GPU, every rank runs the same session on the same inputs):
    // commitments and quotient cosets are split over the ranks, results exchanged through `gather`
    std::vector<F4> absorbed;                // what zk_proof_begin fed the transcript (replayed into an external one)
    zk_transcript_vtable ext_vt{};           // copy of the caller's vtable when an external transcript is set
    uint32_t rank = 0, world = 1;
    zk_allgather_fn gather = nullptr;
    void* gather_user = nullptr;
    bool use_comm = false;                   // exchanges go through the context's RCCL communicator (zk_proof_set_sharding_comm)
    zk_allgather_fn gather_dev = nullptr;    // optional: all-gather of DEVICE buffers (RCCL over xGMI) for the advice columns
    void* gather_dev_user = nullptr;
    std::vector<F4> challenges;
    zk_proof(const zk_pk* k, const uint8_t* seed) : pk(k), rng(seed), inst_lag(k->I), inst_coeff(k->I), adv_lag(k->A), adv_coeff(k->A), challenges(k->chal_phase.size(), host::fr_zero()) {}
};

namespace {

#define PK_TRY(expr) do { int rc__ = (expr); if (rc__) return rc__; } while (0)
#define PK_ALLOC(ctx, buf, nbytes) do { if (!(buf).alloc(nbytes)) return (ctx)->fail(ZK_ERR_OOM, "prover: alloc failed"); } while (0)

// puts the context's stream back, on every way out, in a scope that redirects it to the auxiliary stream
struct StreamRestore {
    zk_ctx* c; hipStream_t s;
    explicit StreamRestore(zk_ctx* ctx) : c(ctx), s(ctx->stream) {}
    ~StreamRestore() { c->stream = s; }
};

// Free device memory right now (the session pool's parked blocks are not in it: callers add zk_ctx::pool_bytes).  When the
// runtime cannot tell: 0, and *ok = false for a caller that reacts to that in another way than by counting on nothing.
size_t device_free_bytes(bool* ok = nullptr) {
    size_t free_b = 0, total_b = 0;
    const bool got = hipMemGetInfo(&free_b, &total_b) == hipSuccess;
    if (!got) { (void)hipGetLastError(); free_b = 0; }
    if (ok) *ok = got;
    return free_b;
}

// The cosets of the columns are read by the quotient's class programs and by nothing else, so they are written as what those programs
// compute on: coset records of 32 x the value (ff29.hip.hpp; the last pass of the transform writes them, k_quotient_eval2's record mode
// reads them without unpacking).  ZK_QUOTIENT_RECORDS=0 keeps packed elements, and so does the older kernel (ZK_QUOTIENT_KERNEL=1), which
// has no record mode.  Read where a session first makes a coset and again where its quotient starts: the tests flip both knobs in one process.
bool quotient_records(uint32_t k) {
    const char* r = getenv("ZK_QUOTIENT_RECORDS");
    return !(r && atoi(r) == 0) && records_supported(QuotientEvalKnobs::read(), k);        // a coset has 2^k rows
}
size_t coset_row_bytes(bool records) { return records ? REC29_BYTES : sizeof(Fr); }
bool session_records(zk_proof* pr) {
    if (pr->coset_fmt < 0) pr->coset_fmt = quotient_records(pr->pk->k) ? 1 : 0;
    return pr->coset_fmt == 1;
}

// Degree class e is evaluated on the cosets class_on_coset(E, e, r) names (quotient_plan.hpp) and, in a sharded session, by the rank
// the (class, coset) pair was dealt to: a table filled once, when the deal is made
struct PairOwners {
    uint32_t E = 0, rank = 0;
    bool sharded = false;
    std::vector<uint32_t> owner;              // [e << E | r]
    size_t at(uint32_t e, uint32_t r) const { return ((size_t)e << E) | r; }
    bool mine(uint32_t e, uint32_t r) const { return class_on_coset(E, e, r) && (!sharded || owner[at(e, r)] == rank); }
};

// (columns served, coset) of every coset r < R that serves a column, most columns first, then by index: the order in which
// cosets of the advice columns are taken to be computed ahead (plan_advice_cosets, stage_late_advice_cosets)
template <class Count>
std::vector<std::pair<uint32_t, uint32_t>> cosets_by_columns_served(uint32_t R, Count served) {
    std::vector<std::pair<uint32_t, uint32_t>> by_count;
    for (uint32_t r = 0; r < R; ++r) {
        const uint32_t cnt = served(r);
        if (cnt) by_count.push_back({cnt, r});
    }
    std::sort(by_count.begin(), by_count.end(), [](const auto& a, const auto& b) { return a.first != b.first ? a.first > b.first : a.second < b.second; });
    return by_count;
}

// sum_j ch^j * polys[j] over 2^k rows on the device: Horner from the last polynomial down (FOLD multiplies the accumulator by ch)
int lincomb(zk_ctx* ctx, uint32_t k, const std::vector<const void*>& polys, const F4& ch, void* d_out) {
    std::vector<uint32_t> words;
    std::vector<const void*> cols;
    for (size_t j = polys.size(); j-- > 0;) { words.insert(words.end(), {Q_PUSH_COL, (uint32_t)cols.size(), 0u, Q_FOLD, 0u, 0u}); cols.push_back(polys[j]); }
    return zk_quotient_eval(ctx, words.data(), (uint32_t)(words.size() / 3), cols.data(), (uint32_t)cols.size(), &ch, 1, k, k, 0, d_out);
}

int commit_lagrange(zk_ctx* ctx, const zk_srs* srs, const Fr* d_vals, size_t n, G1Affine* out) { return zk_commit(ctx, srs, 1, d_vals, n, out); }
int commit_coeff(zk_ctx* ctx, const zk_srs* srs, const Fr* d_vals, size_t n, G1Affine* out) { return zk_commit(ctx, srs, 0, d_vals, n, out); }

// Lagrange values -> coefficients (EvaluationDomain::lagrange_to_coeff)
int to_coeff(zk_ctx* ctx, const zk_pk* pk, const DevBuf& lag, DevBuf* coeff) {
    const size_t n = (size_t)1 << pk->k;
    PK_ALLOC(ctx, *coeff, n * 32);
    const Fr omega_inv = fr_inv_host(fr_root_of_unity(pk->k)), ninv = fr_inv_host(fr_from_u64(1ull << pk->k));
    return ntt_run(ctx, coeff->fr(), pk->k, omega_inv, &ninv, nullptr, nullptr, lag.fr());
}

// to_coeff on the auxiliary stream (the caller orders that stream after the column's upload and the
// main stream after it again): the advice phase keeps its main stream for the commitment pipeline
int to_coeff_aux(zk_ctx* ctx, const zk_pk* pk, const DevBuf& lag, DevBuf* coeff) {
    hipStream_t main_stream = ctx->stream;
    ctx->stream = ctx->stream_aux;
    const int rc = to_coeff(ctx, pk, lag, coeff);
    ctx->stream = main_stream;
    return rc;
}

// ------------------------------------------------------------------------------------------------
// Program concretisation: abstract column references -> indices into a flat pointer table,
// abstract constants -> indices into a flat constant table.
struct Concrete {
    std::vector<uint32_t> words;
    std::vector<const void*> cols;
    std::vector<F4> consts;
    std::unordered_map<uint32_t, uint32_t> col_index, const_index;
};

struct Env {   // where an abstract column lives in the form being read (Lagrange values or coefficients)
    const zk_pk* pk;
    const std::unordered_map<uint32_t, const void*>* part;   // non-null: one coset of the extended domain, by column reference
    const std::vector<DevBuf>* advice;
    const std::vector<DevBuf>* instance;
    const std::vector<DevBuf>* perm_z;
    const std::vector<DevBuf>* lk_m;
    const std::vector<DevBuf>* lk_phi;
    F4 theta, beta, gamma, y;
    std::vector<F4> beta_delta;   // beta * delta^j
    std::vector<F4> challenges;   // user challenges (halo2 `Challenge`), by index
    std::vector<F4> ypow;         // y^g, g < size (optional: the weights of a grouped class program, assemble_grouped)
};

const void* resolve_col(const Env& e, uint32_t ref) {
    const uint32_t type = ref >> 24, idx = ref & 0xFFFFFF;
    const zk_pk* pk = e.pk;
    if (e.part) { auto it = e.part->find(ref); return it == e.part->end() ? nullptr : it->second; }
    switch (type) {
        case CT_FIXED: return idx < pk->F ? pk->fixed_lag[idx].p : nullptr;
        case CT_ADVICE: return e.advice && idx < e.advice->size() ? (*e.advice)[idx].p : nullptr;
        case CT_INSTANCE: return e.instance && idx < e.instance->size() ? (*e.instance)[idx].p : nullptr;
        case CT_SPECIAL:
            if (idx == SP_X) return pk->omega_lag.p;
            if (idx == SP_L0) return pk->l0_lag.p;
            if (idx == SP_LLAST) return pk->llast_lag.p;
            if (idx == SP_LACTIVE) return pk->lactive_lag.p;
            return nullptr;
        case CT_PERM_Z: return e.perm_z && idx < e.perm_z->size() ? (*e.perm_z)[idx].p : nullptr;
        case CT_SIGMA: return idx < pk->P ? pk->sigma_lag[idx].p : nullptr;
        case CT_LK_M: return e.lk_m && idx < e.lk_m->size() ? (*e.lk_m)[idx].p : nullptr;
        case CT_LK_PHI: return e.lk_phi && idx < e.lk_phi->size() ? (*e.lk_phi)[idx].p : nullptr;
        default: return nullptr;
    }
}
bool resolve_const(const Env& e, uint32_t ref, F4* out) {
    if (ref < e.pk->consts.size()) { *out = e.pk->consts[ref]; return true; }
    switch (ref) {
        case C_THETA: *out = e.theta; return true;
        case C_BETA: *out = e.beta; return true;
        case C_GAMMA: *out = e.gamma; return true;
        case C_Y: *out = e.y; return true;
        case C_ONE: *out = host::fr_one(); return true;
        case C_ZERO: *out = host::fr_zero(); return true;
        default: break;
    }
    if (ref >= C_DELTA0 && ref - C_DELTA0 < e.beta_delta.size()) { *out = e.beta_delta[ref - C_DELTA0]; return true; }
    if (ref >= C_CHAL0 && ref - C_CHAL0 < e.challenges.size()) { *out = e.challenges[ref - C_CHAL0]; return true; }
    if (ref >= C_YPOW0 && ref < C_CHAL0) { *out = ref - C_YPOW0 < e.ypow.size() ? e.ypow[ref - C_YPOW0] : host::fr_pow(e.y, ref - C_YPOW0); return true; }
    return false;
}
int concretise(zk_ctx* ctx, const Env& e, const Prog& g, Concrete* c) {
    for (const Instr& in : g) {
        uint32_t a = in.a;
        if (in.op == Q_PUSH_COL) {
            auto it = c->col_index.find(in.a);
            if (it == c->col_index.end()) {
                const void* p = resolve_col(e, in.a);
                if (!p) return ctx->fail(ZK_ERR_INVALID_ARG, "prover: unresolved column reference 0x%08x", in.a);
                a = (uint32_t)c->cols.size();
                c->cols.push_back(p);
                c->col_index[in.a] = a;
            } else a = it->second;
        } else if (in.op == Q_PUSH_CONST || in.op == Q_FOLD || in.op == Q_MUL_CONST || in.op == Q_ADD_CONST) {
            auto it = c->const_index.find(in.a);
            if (it == c->const_index.end()) {
                F4 v;
                if (!resolve_const(e, in.a, &v)) return ctx->fail(ZK_ERR_INVALID_ARG, "prover: unresolved constant reference 0x%08x", in.a);
                a = (uint32_t)c->consts.size();
                c->consts.push_back(v);
                c->const_index[in.a] = a;
            } else a = it->second;
        }
        c->words.push_back(in.op); c->words.push_back(a); c->words.push_back(in.b);
    }
    return ZK_OK;
}
// Every form the prover evaluates over has n = 2^k rows (Lagrange values, or one coset of the
// extended domain), so a rotation is a plain index shift modulo n.
// records: the columns of `e` are coset records (a class program on one coset); d_out then holds 32 x the values
int run_program(zk_ctx* ctx, const Env& e, const Prog& g, void* d_out, bool records = false) {
    Concrete c;
    PK_TRY(concretise(ctx, e, g, &c));
    {   // measurement knob (results are WRONG): every operand read from ONE column -- the same instruction stream with its loads served by the caches
        static const int alias = getenv("ZK_QUOTIENT_ALIAS") ? atoi(getenv("ZK_QUOTIENT_ALIAS")) : 0;      // N: the class programs read N distinct columns in all
        if (alias > 0 && ctx->prof_tag && !strcmp(ctx->prof_tag, "quotient_coset")) for (size_t i = 0; i < c.cols.size(); ++i) c.cols[i] = c.cols[i % (size_t)alias];
    }
    return quotient_eval_fmt(ctx, c.words.data(), (uint32_t)(c.words.size() / 3), c.cols.data(), (uint32_t)c.cols.size(),
                             c.consts.empty() ? nullptr : c.consts.data(), (uint32_t)c.consts.size(), e.pk->k, e.pk->k, 0, d_out, records);
}
// coefficient form of an abstract column (nullptr for X, which has no stored polynomial)
const Fr* coeff_of(const zk_pk* pk, uint32_t ref, const std::vector<DevBuf>& adv, const std::vector<DevBuf>& inst, const std::vector<DevBuf>& pz,
                   const std::vector<DevBuf>& lkm, const std::vector<DevBuf>& lkphi) {
    const uint32_t type = ref >> 24, idx = ref & 0xFFFFFF;
    auto at = [&](const std::vector<DevBuf>& v) -> const Fr* { return idx < v.size() ? v[idx].fr() : nullptr; };
    switch (type) {
        case CT_FIXED: return at(pk->fixed_coeff);
        case CT_ADVICE: return at(adv);
        case CT_INSTANCE: return at(inst);
        case CT_SPECIAL: return idx == SP_L0 ? pk->l0_coeff.fr() : idx == SP_LLAST ? pk->llast_coeff.fr() : idx == SP_LACTIVE ? pk->lactive_coeff.fr() : nullptr;
        case CT_PERM_Z: return at(pz);
        case CT_SIGMA: return at(pk->sigma_coeff);
        case CT_LK_M: return at(lkm);
        case CT_LK_PHI: return at(lkphi);
        default: return nullptr;
    }
}

// Results of `count` items that a sharded session deals round-robin (item i to rank i % world), `elem` bytes each.  `local`
// holds this rank's results in its own order, share_size() of them with the unused tail zeroed; they are all-gathered, and
// `out` receives all `count` in item order -- on every rank the same, so the transcripts stay identical.
size_t share_size(const zk_proof* pr, size_t count) { return (count + pr->world - 1) / pr->world; }
int share_gather(zk_ctx* ctx, const zk_proof* pr, const void* local, size_t count, size_t elem, void* out) {
    const size_t per = share_size(pr, count);
    std::vector<uint8_t> all(per * pr->world * elem);
    if (per && pr->gather(pr->gather_user, local, per * elem, all.data())) return ctx->fail(ZK_ERR_INVALID_ARG, "sharded session: all-gather callback failed");
    for (size_t i = 0; i < count; ++i) memcpy((uint8_t*)out + i * elem, all.data() + ((i % pr->world) * per + i / pr->world) * elem, elem);
    return ZK_OK;
}

// usable-row masks in Lagrange form
// `count` commitments over one basis, split over the ranks of a sharded session: rank r commits
// columns i = r, r + world, ... (pipelined batch) and the 64-byte points are all-gathered, so every
// rank ends up with all of them in order and the transcripts stay identical.
int sharded_commit(zk_ctx* ctx, const zk_proof* pr, const zk_srs* srs, int basis, const void* const* ptrs, size_t count, size_t n, G1Affine* out, uint8_t kind = 0 /* zk_commit_batch_hint: 0 dense, 1 small values, 2 runs of equal values, 3 sums with mostly equal increments */) {
    const std::vector<uint8_t> hint(count, kind);
    if (pr->world <= 1 || !pr->gather) return commit_batch_staged(ctx, srs, basis, ptrs, count, n, out, nullptr, nullptr, hint.data());
    if (count < pr->world && n >= ((size_t)pr->world << 10)) {
        // Fewer columns than ranks (aggregation layers: ~10 columns at k = 22..25, h pieces, the closing
        // commitments): shard every MSM by POINTS instead -- rank r takes the r-th slice of the bases of
        // each column, the 64-byte partial results are all-gathered (RCCL has no elliptic-curve reduction)
        // and summed on the host.
        const size_t base = n / pr->world, rem = n % pr->world;
        const size_t lo = pr->rank * base + std::min<size_t>(pr->rank, rem), len = base + (pr->rank < rem ? 1 : 0);
        const G1Affine* bases = basis ? srs->g_lagrange : srs->g;
        std::vector<G1Affine> local(count), all(count * pr->world);
        for (size_t i = 0; i < count; ++i)
            PK_TRY(zk_msm_g1(ctx, (const Fr*)ptrs[i] + lo, bases + lo, len, &local[i]));
        if (pr->gather(pr->gather_user, local.data(), count * sizeof(G1Affine), all.data())) return ctx->fail(ZK_ERR_INVALID_ARG, "sharded session: all-gather callback failed");
        std::vector<G1Affine> parts(pr->world);
        for (size_t i = 0; i < count; ++i) {
            for (uint32_t q_ = 0; q_ < pr->world; ++q_) parts[q_] = all[(size_t)q_ * count + i];
            if (zk_g1_sum_host(parts.data(), pr->world, &out[i])) return ctx->fail(ZK_ERR_INVALID_ARG, "sharded session: partial sums could not be added");
        }
        return ZK_OK;
    }
    std::vector<const void*> mine;
    for (size_t i = pr->rank; i < count; i += pr->world) mine.push_back(ptrs[i]);
    std::vector<G1Affine> local(share_size(pr, count));
    memset((void*)local.data(), 0, sizeof(G1Affine) * local.size());
    PK_TRY(commit_batch_staged(ctx, srs, basis, mine.data(), mine.size(), n, local.data(), nullptr, nullptr, hint.data()));
    return share_gather(ctx, pr, local.data(), count, sizeof(G1Affine), out);
}

int upload(zk_ctx* ctx, DevBuf* b, const void* h, size_t bytes) {
    if (!b->alloc(bytes)) return ctx->fail(ZK_ERR_OOM, "prover: alloc of %zu bytes failed", bytes);
    return zk_h2d(ctx, b->p, h, bytes);
}


// One all-gather of `bytes` per rank out of the device buffer d_send, by the first transport the session has:
//   use_comm (a caller that may): the context's RCCL communicator, device to device into d_recv, stream-ordered -- no host
//               copy, no synchronisation;
//   the caller's device all-gather (zk_proof_set_device_gather), into d_recv: the stream is drained first, the callback
//               completes on return;
//   the host callback: d_send is downloaded into host.send (stage_send false: host.send goes out as it stands) and the
//               ranks' blocks arrive in host.recv -- bringing them to the device is the caller's step.
// *on_device says where the result lies.
struct HostStaging { std::vector<uint8_t> send, recv; };
int allgather_rows(zk_ctx* ctx, const zk_proof* pr, bool use_comm, const void* d_send, bool stage_send, size_t bytes, void* d_recv, HostStaging& host, bool* on_device) {
    *on_device = use_comm || pr->gather_dev;
    if (use_comm) return comm_allgather_dev(ctx, d_send, bytes, d_recv);
    if (pr->gather_dev) {
        PK_TRY(zk_ctx_sync(ctx));
        if (pr->gather_dev(pr->gather_dev_user, d_send, bytes, d_recv)) return ctx->fail(ZK_ERR_INVALID_ARG, "sharded session: device all-gather callback failed");
        return ZK_OK;
    }
    host.send.resize(bytes); host.recv.resize((size_t)pr->world * bytes);
    if (stage_send) PK_TRY(zk_d2h(ctx, host.send.data(), d_send, bytes));
    if (pr->gather(pr->gather_user, host.send.data(), bytes, host.recv.data())) return ctx->fail(ZK_ERR_INVALID_ARG, "sharded session: all-gather callback failed");
    return ZK_OK;
}

struct Open { const Fr* poly; int32_t rot; F4 eval; };      // one opening: a polynomial (coefficients on the device), the rotation of x, the value there

// ---- SHPLONK's host mathematics
// construct_intermediate_sets: polynomials in order of first appearance with their point sets;
// rotation sets in order of first appearance, each listing its polynomials; `super`: every point that is opened somewhere
struct PolyQ { const Fr* poly; std::vector<int32_t> rots; std::vector<F4> evals; };
struct RotSet { std::vector<int32_t> rots; std::vector<size_t> members; };
void shplonk_intermediate_sets(const std::vector<Open>& queries, std::vector<PolyQ>& polys, std::vector<RotSet>& sets, std::vector<int32_t>& super) {
    for (const Open& o : queries) {
        auto it = std::find_if(polys.begin(), polys.end(), [&](const PolyQ& p) { return p.poly == o.poly; });
        if (it == polys.end()) { polys.push_back({o.poly, {}, {}}); it = polys.end() - 1; }
        if (std::find(it->rots.begin(), it->rots.end(), o.rot) == it->rots.end()) { it->rots.push_back(o.rot); it->evals.push_back(o.eval); }
    }
    for (size_t pi = 0; pi < polys.size(); ++pi) {
        std::vector<int32_t> key = polys[pi].rots;
        std::sort(key.begin(), key.end());
        auto it = std::find_if(sets.begin(), sets.end(), [&](const RotSet& s_) { return s_.rots == key; });
        if (it == sets.end()) { sets.push_back({key, {}}); it = sets.end() - 1; }
        it->members.push_back(pi);
        for (int32_t r_ : key) if (std::find(super.begin(), super.end(), r_) == super.end()) super.push_back(r_);
    }
}
// r_ij(X): interpolation of polynomial j's evaluations over its set's points (degree < |S|), host side.  The Lagrange basis
// of a set -- L_a(X) = prod_{b != a} (X - x_b) / (x_a - x_b), |S|^3 products -- is built ONCE per set; a member then costs
// |S|^2.  (Per member it was 3.9 ms of the Keccak-shape proof: 48 columns opened at the same 14 points.)
std::vector<std::vector<F4>> lagrange_basis(const std::vector<F4>& xs) {
    const size_t m = xs.size();
    std::vector<std::vector<F4>> basis(m);
    for (size_t a = 0; a < m; ++a) {
        std::vector<F4> num{host::fr_one()};       // prod_{b != a} (X - x_b)
        F4 den = host::fr_one();
        for (size_t b2 = 0; b2 < m; ++b2) {
            if (b2 == a) continue;
            std::vector<F4> nx(num.size() + 1, host::fr_zero());
            for (size_t t = 0; t < num.size(); ++t) { nx[t + 1] = host::fr_add(nx[t + 1], num[t]); nx[t] = host::fr_sub(nx[t], host::fr_mul(num[t], xs[b2])); }
            num.swap(nx);
            den = host::fr_mul(den, host::fr_sub(xs[a], xs[b2]));
        }
        const F4 dinv = host::fr_inv(den);
        for (F4& c : num) c = host::fr_mul(c, dinv);
        basis[a] = std::move(num);
    }
    return basis;
}
std::vector<F4> interpolate(const std::vector<std::vector<F4>>& basis, const std::vector<F4>& ys) {
    const size_t m = basis.size();
    std::vector<F4> out(m, host::fr_zero());
    for (size_t a = 0; a < m; ++a)
        for (size_t t = 0; t < m; ++t) out[t] = host::fr_add(out[t], host::fr_mul(basis[a][t], ys[a]));
    return out;
}
F4 eval_small(const std::vector<F4>& c, const F4& at) { F4 acc = host::fr_zero(); for (size_t t = c.size(); t-- > 0;) acc = host::fr_add(host::fr_mul(acc, at), c[t]); return acc; }

// The column data of a version 4 key blob: F cell widths, the F fixed payloads (1-16-byte unsigned integers or
// Montgomery elements), the permutation mapping.  Sixteen columns at a time cross the link on the copy stream into one staging
// buffer and are expanded there, right behind their upload, into the key's Lagrange buffers -- fr_from_uint_batch_run for the
// narrow fixed columns, k_sigma_from_mapping for the sigma columns (Montgomery fixed columns go straight to their buffer) --
// while the commitments of the previous columns run: the staging callback of commit_batch_staged fences each group.  `tables`
// receives the delta^j table and, behind it, the kernel's flag word; the caller reads the flag once the device is drained.
constexpr size_t V4_GROUP = 16;                    // columns per expansion launch (FU_BATCH of typed_rows.hip, SM_BATCH of vec.hip)
int load_columns_v4(zk_ctx* ctx, zk_pk* pk, Reader& r, DevBuf* tables) {
    const size_t n = (size_t)1 << pk->k, F = pk->F, P = pk->P;
    struct Stage {
        zk_ctx* ctx; size_t n, F, P;
        std::vector<const uint8_t*> src; std::vector<uint8_t> width; std::vector<void*> dst;      // F fixed then P sigma columns
        char* staging = nullptr; const Fr* omega = nullptr; const Fr* delta = nullptr; uint32_t* bad = nullptr;
        size_t done = 0;                          // columns [0, done) are enqueued on the copy stream
    } st{ctx, n, F, P, {}, {}, {}};
    for (size_t i = 0; i < F; ++i) {
        const uint32_t w = r.u32();
        if (!r.ok) return ctx->fail(ZK_ERR_INVALID_ARG, "pk blob: truncated table of fixed cell widths");
        if (w != 1 && w != 2 && w != 4 && w != 8 && w != 16 && w != 32) return ctx->fail(ZK_ERR_INVALID_ARG, "pk blob: fixed column %zu has cell width %u (must be 1, 2, 4, 8, 16 or 32 bytes)", i, w);
        st.width.push_back((uint8_t)w);
    }
    for (size_t i = 0; i < F; ++i) {
        const uint8_t* b = r.bytes(n * st.width[i]);
        if (!b) return ctx->fail(ZK_ERR_INVALID_ARG, "pk blob: truncated fixed column %zu (%zu cells of %u bytes)", i, n, (unsigned)st.width[i]);
        st.src.push_back(b);
    }
    for (size_t j = 0; j < P; ++j) {
        const uint8_t* b = r.bytes(n * 8);
        if (!b) return ctx->fail(ZK_ERR_INVALID_ARG, "pk blob: truncated permutation mapping (column %zu of %zu)", j, P);
        st.src.push_back(b);
        st.width.push_back(8);
    }
    for (size_t i = 0; i < F + P; ++i) {
        DevBuf& lag = i < F ? pk->fixed_lag[i] : pk->sigma_lag[i - F];
        if (!lag.alloc(n * 32)) return ctx->fail(ZK_ERR_OOM, "prover: alloc of %zu bytes failed", n * 32);
        st.dst.push_back(lag.p);
    }
    if (F + P == 0) return ZK_OK;
    // the staging buffer holds the packed cells or the mapping slices of one group (payload offsets in the blob have no alignment: the
    // uploads are byte copies, and every column starts on a 16-byte boundary here)
    auto slot = [n](uint8_t w) { return (n * w + 15) / 16 * 16; };
    size_t staging_bytes = 0;
    for (size_t g0 = 0; g0 < F + P; g0 = g0 < F ? std::min(g0 + V4_GROUP, F) : g0 + V4_GROUP) {
        size_t bytes = 0;
        for (size_t g = g0; g < std::min(g0 + V4_GROUP, g0 < F ? F : F + P); ++g) if (g >= F || st.width[g] < 32) bytes += slot(st.width[g]);
        staging_bytes = std::max(staging_bytes, bytes);
    }
    DevBuf staging;
    if (staging_bytes) PK_ALLOC(ctx, staging, staging_bytes);
    st.staging = (char*)staging.p;
    if (P) {
        PK_ALLOC(ctx, *tables, P * 32 + 32);
        std::vector<F4> dp;
        const F4 delta = host::fr_pow(host::fr_from_u64(7), 1ull << 28);          // as the permutation argument forms beta * delta^j
        F4 cur = host::fr_one();
        for (size_t j = 0; j < P; ++j) { dp.push_back(cur); cur = host::fr_mul(cur, delta); }
        ZK_HIP(ctx, hipMemcpyAsync(tables->p, dp.data(), P * 32, hipMemcpyHostToDevice, ctx->stream));
        ZK_HIP(ctx, hipMemsetAsync((char*)tables->p + P * 32, 0, 32, ctx->stream));
        ZK_HIP(ctx, hipStreamSynchronize(ctx->stream));                            // `dp` goes out of scope
        st.delta = (const Fr*)tables->p;
        st.bad = (uint32_t*)((char*)tables->p + P * 32);
        st.omega = pk->omega_lag.fr();
    }
    // hints for the MSM (speed only): cells of 8 bytes or fewer are below 2^64 by construction, wider ones are sampled on the host
    // as the v3 path samples its columns (through an aligned copy of the samples); sigma columns are field-sized
    std::vector<uint8_t> narrow(F + P, 0);
    {
        const size_t samples = std::min<size_t>(n, 1024), step = n / samples;
        std::vector<std::vector<F4>> picked;
        std::vector<const void*> picked_ptr;
        std::vector<size_t> picked_at;
        for (size_t i = 0; i < F; ++i) {
            if (st.width[i] <= 8) narrow[i] = 1;
            else if (st.width[i] == 16) {
                size_t large = 0;
                for (size_t s_ = 0; s_ < samples; ++s_) { uint64_t hi; memcpy(&hi, st.src[i] + (s_ * step) * 16 + 8, 8); large += hi != 0; }
                narrow[i] = large <= samples / 4;
            } else {
                picked.emplace_back(samples);
                for (size_t s_ = 0; s_ < samples; ++s_) memcpy(picked.back()[s_].l, st.src[i] + (s_ * step) * 32, 32);
                picked_at.push_back(i);
            }
        }
        for (const auto& v : picked) picked_ptr.push_back(v.data());
        std::vector<uint8_t> picked_narrow(picked.size());
        sample_narrow(picked_ptr.data(), picked.size(), samples, picked_narrow.data());
        for (size_t t = 0; t < picked.size(); ++t) narrow[picked_at[t]] = picked_narrow[t];
    }
    PK_TRY(copy_stream_open(ctx));
    auto stage = [](void* user, size_t it) -> int {
        Stage* s_ = (Stage*)user;
        if (it >= s_->done) {                     // first column of a group: the whole group is enqueued now, the calls for the others only fence
            const size_t g0 = s_->done, g1 = std::min(g0 + V4_GROUP, g0 < s_->F ? s_->F : s_->F + s_->P);
            const void* gsrc[V4_GROUP]; Fr* gdst[V4_GROUP]; uint8_t gw[V4_GROUP];
            size_t cnt = 0, off = 0;
            for (size_t g = g0; g < g1; ++g) {
                if (g < s_->F && s_->width[g] == 32) { ZK_HIP(s_->ctx, hipMemcpyAsync(s_->dst[g], s_->src[g], s_->n * 32, hipMemcpyHostToDevice, s_->ctx->stream_copy)); continue; }
                const size_t bytes = s_->n * s_->width[g];
                ZK_HIP(s_->ctx, hipMemcpyAsync(s_->staging + off, s_->src[g], bytes, hipMemcpyHostToDevice, s_->ctx->stream_copy));
                gsrc[cnt] = s_->staging + off; gdst[cnt] = (Fr*)s_->dst[g]; gw[cnt] = s_->width[g]; ++cnt;
                off += (bytes + 15) / 16 * 16;
            }
            if (g0 < s_->F) PK_TRY(fr_from_uint_batch_run(s_->ctx, s_->ctx->stream_copy, gsrc, gw, cnt, s_->n, gdst));
            else PK_TRY(sigma_from_mapping_run(s_->ctx, s_->ctx->stream_copy, gsrc, cnt, s_->n, (uint32_t)s_->P, s_->omega, s_->delta, s_->bad, gdst));
            s_->done = g1;
        }
        return copy_stream_fence(s_->ctx);
    };
    std::vector<G1Affine> coms(F + P);
    PK_TRY(commit_batch_staged(ctx, pk->srs, 1, (const void* const*)st.dst.data(), F + P, n, coms.data(), stage, &st, narrow.data()));
    PK_TRY(zk_ctx_sync(ctx));                     // the staging buffer is released on return
    ZK_HIP(ctx, hipStreamSynchronize(ctx->stream_copy));
    for (size_t i = 0; i < F; ++i) { pk->fixed_com[i] = coms[i]; PK_TRY(to_coeff(ctx, pk, pk->fixed_lag[i], &pk->fixed_coeff[i])); }
    for (size_t i = 0; i < P; ++i) { pk->sigma_com[i] = coms[F + i]; PK_TRY(to_coeff(ctx, pk, pk->sigma_lag[i], &pk->sigma_coeff[i])); }
    return ZK_OK;
}

}  // namespace

extern "C" {

void zk_pk_destroy(zk_ctx* ctx, zk_pk* pk) {
    if (ctx) (void)zk_ctx_sync(ctx);
    if (ctx && pk) ctx->coset_cache_bytes -= std::min(ctx->coset_cache_bytes, pk->part_cache_bytes);     // its slots go back to the shared budget
    delete pk;
}

// keygen_pk: parse the blob, make the key material device resident, commit fixed / sigma columns.
int zk_pk_create(zk_ctx* ctx, const zk_srs* srs, const void* h_blob, size_t blob_len, zk_pk** out) {
    if (!ctx) return ZK_ERR_INVALID_ARG;
    ZK_REQUIRE(ctx, srs && h_blob && out, "null pointer");
    Reader r{(const uint8_t*)h_blob, blob_len};
    std::unique_ptr<zk_pk> pk(new zk_pk());
    pk->srs = srs;
    {
        std::string err;
        const int rc = parse_cs(r, pk.get(), blob_len, true, &err);
        if (rc) return ctx->fail(rc, "%s", err.c_str());
    }
    // commit_lagrange needs the Lagrange basis of exactly this domain (halo2: ParamsKZG::downsize)
    if (pk->k != srs->k) return ctx->fail(ZK_ERR_INVALID_ARG, "SRS is for k=%u but the circuit has k=%u: downsize the SRS first", srs->k, pk->k);
    if (!srs->g_lagrange) return ctx->fail(ZK_ERR_INVALID_ARG, "SRS has no Lagrange basis");
    const size_t n = (size_t)1 << pk->k;
    const size_t cs_len = blob_len - r.left;        // the constraint-system part: everything before the column data
    // fixed + sigma columns
    pk->fixed_lag.resize(pk->F); pk->fixed_coeff.resize(pk->F);
    pk->sigma_lag.resize(pk->P); pk->sigma_coeff.resize(pk->P);
    pk->fixed_com.resize(pk->F); pk->sigma_com.resize(pk->P);
    auto omega_column = [&]() -> int {              // omega^i, row by row
        const Fr w = fr_root_of_unity(pk->k), one = Fr::one();
        return zk_fr_powers(ctx, &w, &one, pk->omega_lag.p, n);
    };
    DevBuf v4_tables;                               // version 4: delta^j table and the flag word of k_sigma_from_mapping (read below, once the device is drained)
    if (pk->version == 4u) {                        // the omega^i column first: the sigma columns are products with its rows
        PK_ALLOC(ctx, pk->omega_lag, n * 32);
        PK_TRY(omega_column());
        PK_TRY(load_columns_v4(ctx, pk.get(), r, &v4_tables));
    } else {   // keygen's commit_lagrange over every fixed and sigma column as ONE pipelined batch: column i + 1
        // crosses PCIe on the copy stream while the MSM of column i runs; the coefficient forms follow
        std::vector<const void*> h_cols;
        std::vector<void*> d_cols;
        for (uint32_t i = 0; i < pk->F + pk->P; ++i) {
            const uint8_t* b = r.bytes(n * 32);
            if (!b) return ctx->fail(ZK_ERR_INVALID_ARG, "pk blob: truncated %s column", i < pk->F ? "fixed" : "sigma");
            DevBuf& lag = i < pk->F ? pk->fixed_lag[i] : pk->sigma_lag[i - pk->F];
            if (!lag.alloc(n * 32)) return ctx->fail(ZK_ERR_OOM, "prover: alloc of %zu bytes failed", n * 32);
            h_cols.push_back(b);
            d_cols.push_back(lag.p);
        }
        std::vector<G1Affine> coms(h_cols.size());
        PK_TRY(zk_commit_batch_h2d(ctx, srs, 1, h_cols.data(), d_cols.data(), h_cols.size(), n, coms.data()));
        for (uint32_t i = 0; i < pk->F; ++i) { pk->fixed_com[i] = coms[i]; PK_TRY(to_coeff(ctx, pk.get(), pk->fixed_lag[i], &pk->fixed_coeff[i])); }
        for (uint32_t i = 0; i < pk->P; ++i) { pk->sigma_com[i] = coms[pk->F + i]; PK_TRY(to_coeff(ctx, pk.get(), pk->sigma_lag[i], &pk->sigma_coeff[i])); }
    }
    // l0, l_last, l_active (built on the device: a delta at row 0, a delta at row u, ones below u) and the omega^i column
    {
        const Fr one = Fr::one();
        PK_ALLOC(ctx, pk->l0_lag, n * 32); PK_ALLOC(ctx, pk->llast_lag, n * 32); PK_ALLOC(ctx, pk->lactive_lag, n * 32);
        if (pk->version != 4u) PK_ALLOC(ctx, pk->omega_lag, n * 32);
        ZK_HIP(ctx, hipMemsetAsync(pk->l0_lag.p, 0, n * 32, ctx->stream));
        ZK_HIP(ctx, hipMemsetAsync(pk->llast_lag.p, 0, n * 32, ctx->stream));
        ZK_HIP(ctx, hipMemsetAsync(pk->lactive_lag.p, 0, n * 32, ctx->stream));
        PK_TRY(zk_h2d(ctx, pk->l0_lag.p, &one, 32));
        PK_TRY(zk_h2d(ctx, (char*)pk->llast_lag.p + (size_t)pk->u * 32, &one, 32));
        PK_TRY(zk_fr_powers(ctx, &one, &one, pk->lactive_lag.p, pk->u));          // 1 * 1^i: ones on the usable rows
        PK_TRY(to_coeff(ctx, pk.get(), pk->l0_lag, &pk->l0_coeff));
        PK_TRY(to_coeff(ctx, pk.get(), pk->llast_lag, &pk->llast_coeff));
        PK_TRY(to_coeff(ctx, pk.get(), pk->lactive_lag, &pk->lactive_coeff));
        if (pk->version != 4u) PK_TRY(omega_column());
        PK_TRY(zk_ctx_sync(ctx));
    }
    if (pk->version == 4u && pk->P) {               // the device is drained: did a mapping pair name a column or a row that does not exist?
        uint32_t bad = 0;
        ZK_HIP(ctx, hipMemcpy(&bad, (const char*)v4_tables.p + (size_t)pk->P * 32, 4, hipMemcpyDeviceToHost));
        if (bad) return ctx->fail(ZK_ERR_INVALID_ARG, "pk blob: a permutation mapping entry is out of range (column >= %u or row >= %zu)", pk->P, n);
    }
    // Default vk.transcript_repr: Blake2b-512 ("Halo2-Verify-Key") over the whole constraint-system
    // part of the blob and the compressed fixed / sigma commitments.  halo2's own value hashes the Debug
    // string of the pinned verifying key, which only the Rust side can produce: the shim installs it
    // with zk_pk_set_transcript_repr, and then proofs are made for exactly the reference's verifier.
    {
        host::Blake2b hsh;
        hsh.init("Halo2-Verify-Key");
        const uint32_t as_v3 = 3u;                   // the version word is read as 3: one circuit, one stand-in value, whichever layout carried its columns
        hsh.update(h_blob, 4);
        hsh.update(&as_v3, 4);
        hsh.update((const uint8_t*)h_blob + 8, cs_len - 8);
        for (const auto& c : pk->fixed_com) { uint8_t b[32]; host::g1_compress(c, b); hsh.update(b, 32); }
        for (const auto& c : pk->sigma_com) { uint8_t b[32]; host::g1_compress(c, b); hsh.update(b, 32); }
        uint8_t dg[64];
        hsh.finalize(dg);
        pk->vk_repr = host::fr_from_uniform(dg);
    }
    PK_TRY(zk_ctx_sync(ctx));
    *out = pk.release();
    return ZK_OK;
}

// halo2 absorbs `vk.transcript_repr()` first [REF zkevm-circuits/src/super_circuit/test.rs:70-85 pins its
// value for the SuperCircuit]; the caller that holds the real VerifyingKey passes that scalar here.
int zk_pk_set_transcript_repr(zk_ctx* ctx, zk_pk* pk, const void* h_repr) {
    if (!ctx) return ZK_ERR_INVALID_ARG;
    ZK_REQUIRE(ctx, pk && h_repr, "null pointer");
    memcpy(pk->vk_repr.l, h_repr, 32);
    return ZK_OK;
}

// Shape of a key, for callers that size buffers from it: out[0..15] = k, degree, extended k, F, A, I,
// P (permutation columns), C (permutation chunks), L (lookup arguments), phases, challenges,
// blinding factors, advice queries, fixed queries, commitments in a proof, evaluations in a proof.
int zk_pk_shape(zk_ctx* ctx, const zk_pk* pk, uint32_t* out16) {
    if (!ctx) return ZK_ERR_INVALID_ARG;
    ZK_REQUIRE(ctx, pk && out16, "null pointer");
    const uint32_t evals = (uint32_t)pk->adv_q.size() + (uint32_t)pk->fix_q.size() + 1 + pk->P + (pk->C ? 3 * pk->C - 1 : 0) + 3 * pk->L;
    const uint32_t v[16] = {pk->k, pk->d, pk->ext_k, pk->F, pk->A, pk->I, pk->P, pk->C, pk->L, pk->num_phases, (uint32_t)pk->chal_phase.size(), pk->bf,
                            (uint32_t)pk->adv_q.size(), (uint32_t)pk->fix_q.size(), pk->A + 2 * pk->L + pk->C + 1 + (pk->d - 1), evals};
    memcpy(out16, v, sizeof v);
    return ZK_OK;
}

// vk side of the key: commitments (F fixed then P sigma, 64-byte affine each) and vk_repr
int zk_pk_vk(zk_ctx* ctx, const zk_pk* pk, void* h_commitments, void* h_vk_repr) {
    if (!ctx) return ZK_ERR_INVALID_ARG;
    ZK_REQUIRE(ctx, pk, "null pointer");
    if (h_commitments) {
        G1Affine* o = (G1Affine*)h_commitments;
        for (uint32_t i = 0; i < pk->F; ++i) o[i] = pk->fixed_com[i];
        for (uint32_t i = 0; i < pk->P; ++i) o[pk->F + i] = pk->sigma_com[i];
    }
    if (h_vk_repr) memcpy(h_vk_repr, &pk->vk_repr, 32);
    return ZK_OK;
}

// ---- proving session: begin -> one call per advice phase -> finish ---------------------------------
// halo2's create_proof synthesises the circuit once per phase and squeezes that phase's challenges
// after committing its advice columns (the SuperCircuit has three phases
// [REF zkevm-circuits/src/util.rs:120-133]); witness synthesis stays on the host, so the phases
// are separate calls and each returns the challenges the next synthesis pass needs.
void zk_proof_abort(zk_ctx* ctx, zk_proof* pr) {
    if (ctx) (void)zk_ctx_sync(ctx);
    delete pr;
}

int zk_proof_set_multiopen(zk_ctx* ctx, zk_proof* pr, int kind) {
    if (!ctx) return ZK_ERR_INVALID_ARG;
    ZK_REQUIRE(ctx, pr && (kind == ZK_MULTIOPEN_GWC || kind == ZK_MULTIOPEN_SHPLONK), "unknown multi-open scheme");
    pr->multiopen = kind;
    return ZK_OK;
}

int zk_proof_set_vanishing_random(zk_ctx* ctx, zk_proof* pr, int kind) {
    if (!ctx) return ZK_ERR_INVALID_ARG;
    ZK_REQUIRE(ctx, pr && (kind == ZK_VANISHING_UNIFORM || kind == ZK_VANISHING_ONE), "unknown kind of vanishing-argument polynomial");
    pr->vanishing_random = kind;
    return ZK_OK;
}

int zk_proof_set_transcript(zk_ctx* ctx, zk_proof* pr, const zk_transcript_vtable* vt, void* user) {
    if (!ctx) return ZK_ERR_INVALID_ARG;
    ZK_REQUIRE(ctx, pr && vt && vt->common_point && vt->common_scalar && vt->write_point && vt->write_scalar && vt->squeeze_challenge, "incomplete transcript vtable");
    ZK_REQUIRE(ctx, pr->phase == 0 && !pr->tr.vt, "the transcript must be set once, before the first advice phase");
    pr->ext_vt = *vt;
    pr->tr.vt = &pr->ext_vt;
    pr->tr.user = user;
    for (const F4& s_ : pr->absorbed) pr->tr.common_scalar(s_);
    pr->absorbed.clear();
    pr->absorbed.shrink_to_fit();
    if (pr->tr.err) return ctx->fail(ZK_ERR_INVALID_ARG, "external transcript callback failed with status %d", pr->tr.err);
    return ZK_OK;
}

// Built-in transcripts: Blake2b (default), Poseidon (gen_snark_shplonk) or Keccak / EVM
// (gen_evm_proof_shplonk).  Same rule as zk_proof_set_transcript: right after zk_proof_begin; what
// begin absorbed is replayed into the chosen transcript.
int zk_proof_set_transcript_kind(zk_ctx* ctx, zk_proof* pr, int kind) {
    if (!ctx) return ZK_ERR_INVALID_ARG;
    ZK_REQUIRE(ctx, pr && (kind == ZK_TRANSCRIPT_BLAKE2B || kind == ZK_TRANSCRIPT_POSEIDON || kind == ZK_TRANSCRIPT_EVM), "unknown transcript kind");
    ZK_REQUIRE(ctx, pr->phase == 0 && !pr->tr.vt, "the transcript must be chosen once, before the first advice phase");
    pr->tr.reset(kind);
    for (const F4& s_ : pr->absorbed) pr->tr.common_scalar(s_);
    return ZK_OK;
}

int zk_proof_set_sharding(zk_ctx* ctx, zk_proof* pr, uint32_t rank, uint32_t world, zk_allgather_fn gather, void* user) {
    if (!ctx) return ZK_ERR_INVALID_ARG;
    ZK_REQUIRE(ctx, pr && world >= 1 && rank < world && (world == 1 || gather), "need rank < world and an all-gather callback");
    ZK_REQUIRE(ctx, pr->phase == 0, "sharding must be set before the first advice phase");
    pr->rank = rank; pr->world = world; pr->gather = gather; pr->gather_user = user;
    return ZK_OK;
}

// Sharded session over the context's own RCCL communicator (zk_comm_init): rank and world come from it,
// commitments are all-gathered through a device staging buffer, advice columns and finished quotient
// cosets device to device over xGMI -- no callback, no host-language collective needed.
static int comm_gather_host_thunk(void* user, const void* send, size_t bytes, void* recv) { return comm_allgather_host((zk_ctx*)user, send, bytes, recv); }
static int comm_gather_dev_thunk(void* user, const void* d_send, size_t bytes, void* d_recv) {
    zk_ctx* c = (zk_ctx*)user;
    const int rc = comm_allgather_dev(c, d_send, bytes, d_recv);
    return rc ? rc : (hipStreamSynchronize(c->stream) == hipSuccess ? 0 : ZK_ERR_HIP);     // the callback contract: complete on return
}
int zk_proof_set_sharding_comm(zk_ctx* ctx, zk_proof* pr) {
    if (!ctx) return ZK_ERR_INVALID_ARG;
    ZK_REQUIRE(ctx, pr, "null pointer");
    ZK_REQUIRE(ctx, comm_ready(ctx), "no communicator on this context: call zk_comm_init first");
    ZK_REQUIRE(ctx, pr->phase == 0, "sharding must be set before the first advice phase");
    pr->rank = ctx->comm_rank; pr->world = ctx->comm_world;
    pr->gather = comm_gather_host_thunk; pr->gather_user = ctx;
    pr->gather_dev = comm_gather_dev_thunk; pr->gather_dev_user = ctx;
    pr->use_comm = true;
    return ZK_OK;
}

int zk_proof_set_device_gather(zk_ctx* ctx, zk_proof* pr, zk_allgather_fn gather_dev, void* user) {
    if (!ctx) return ZK_ERR_INVALID_ARG;
    ZK_REQUIRE(ctx, pr && gather_dev, "null pointer");
    ZK_REQUIRE(ctx, pr->world > 1 && pr->gather, "set the sharding (zk_proof_set_sharding) first");
    ZK_REQUIRE(ctx, pr->phase == 0, "must be set before the first advice phase");
    pr->gather_dev = gather_dev;
    pr->gather_dev_user = user;
    return ZK_OK;
}

// create_proof's instance handling: every PROVIDED value is absorbed (KZG: instances are not
// committed), a column longer than the usable rows is Error::InstanceTooLarge, and the column is
// zero-padded to n.  h_len == NULL is the full-column form: the usable rows of an n-row image.
static int proof_begin(zk_ctx* ctx, const zk_pk* pk, const void* const* h_instance, const uint32_t* h_len, const uint8_t* seed16, zk_proof** out) {
    if (!ctx) return ZK_ERR_INVALID_ARG;
    PoolScope pool_scope(ctx);
    ZK_REQUIRE(ctx, pk && seed16 && out && (h_instance || !pk->I), "null pointer");
    const size_t n = (size_t)1 << pk->k;
    if (h_len)
        for (uint32_t i = 0; i < pk->I; ++i)
            if (h_len[i] > pk->u) return ctx->fail(ZK_ERR_INVALID_ARG, "instance column %u has %u values, the circuit has %zu usable rows (InstanceTooLarge)", i, h_len[i], pk->u);
    std::unique_ptr<zk_proof> pr(new zk_proof(pk, seed16));
    pr->tr.common_scalar(pk->vk_repr);
    pr->absorbed.push_back(pk->vk_repr);
    for (uint32_t i = 0; i < pk->I; ++i) {
        const F4* v = (const F4*)h_instance[i];
        const size_t len = h_len ? h_len[i] : pk->u;
        ZK_REQUIRE(ctx, v || !len, "null instance column");
        for (size_t row = 0; row < len; ++row) { pr->tr.common_scalar(v[row]); pr->absorbed.push_back(v[row]); }
        if (h_len) {
            if (!pr->inst_lag[i].alloc(n * 32)) return ctx->fail(ZK_ERR_OOM, "prover: alloc of %zu bytes failed", n * 32);
            ZK_HIP(ctx, hipMemsetAsync(pr->inst_lag[i].p, 0, n * 32, ctx->stream));
            if (len) PK_TRY(zk_h2d(ctx, pr->inst_lag[i].p, v, len * 32));
        } else {
            PK_TRY(upload(ctx, &pr->inst_lag[i], h_instance[i], n * 32));
        }
        PK_TRY(to_coeff(ctx, pk, pr->inst_lag[i], &pr->inst_coeff[i]));
    }
    *out = pr.release();
    return ZK_OK;
}
int zk_proof_begin(zk_ctx* ctx, const zk_pk* pk, const void* const* h_instance, const uint8_t* seed16, zk_proof** out) {
    return proof_begin(ctx, pk, h_instance, nullptr, seed16, out);
}
int zk_proof_begin_instances(zk_ctx* ctx, const zk_pk* pk, const void* const* h_instance, const uint32_t* h_instance_len, const uint8_t* seed16, zk_proof** out) {
    if (!ctx) return ZK_ERR_INVALID_ARG;
    ZK_REQUIRE(ctx, pk && (h_instance_len || !pk->I), "null pointer");
    static const uint32_t none = 0;
    return proof_begin(ctx, pk, h_instance, h_instance_len ? h_instance_len : &none, seed16, out);
}

// Commits the advice columns of the current phase (h_cols[j] is advice column col_index[j]; exactly
// the columns of this phase, each n x 32 B Lagrange values; rows >= n - bf are replaced by blinding
// values) and squeezes the challenges that become available after it into h_challenges (Fr each,
// in challenge-index order).  When h_challenges is given, *num_challenges holds its capacity (in
// challenges) on entry; on return it holds how many the phase produced.
static int plan_advice_cosets(zk_ctx* ctx, zk_proof* pr);
static int advice_lagrange_readers(zk_ctx* ctx, const zk_pk* pk, std::vector<uint8_t>* need);
static int advice_phase_impl(zk_ctx* ctx, zk_proof* pr, const uint32_t* col_index, const void* const* h_cols, uint32_t ncols, void* h_challenges, uint32_t* num_challenges, bool dev_src, bool in_place,
                             const uint8_t* widths = nullptr /* host columns as typed cells: bytes per cell of h_cols[j], 32 = Montgomery Fr */);
int zk_proof_advice_phase(zk_ctx* ctx, zk_proof* pr, const uint32_t* col_index, const void* const* h_cols, uint32_t ncols, void* h_challenges, uint32_t* num_challenges) {
    return advice_phase_impl(ctx, pr, col_index, h_cols, ncols, h_challenges, num_challenges, false, false);
}
// The same phase for host columns given as typed cells (widths[j] bytes per cell of h_cols[j]: 1, 2, 4, 8, 16 = unsigned little-endian
// integers, 32 = Montgomery Fr): a narrow column crosses PCIe as usable_rows x width bytes and becomes the Montgomery column on the
// device (k_fr_from_uint, on the copy stream right behind its upload).  Same transcript, same bytes.
int zk_proof_advice_phase_typed(zk_ctx* ctx, zk_proof* pr, const uint32_t* col_index, const void* const* h_cols, const uint8_t* widths, uint32_t ncols, void* h_challenges, uint32_t* num_challenges) {
    if (!ctx) return ZK_ERR_INVALID_ARG;
    ZK_REQUIRE(ctx, pr && widths, "null pointer");
    for (uint32_t j = 0; j < ncols; ++j) {
        const uint8_t w = widths[j];
        if (w != 1 && w != 2 && w != 4 && w != 8 && w != 16 && w != 32) return ctx->fail(ZK_ERR_INVALID_ARG, "column %u: cell width %u (must be 1, 2, 4, 8, 16 or 32 bytes)", j, (unsigned)w);
    }
    if (pr->world > 1) return ctx->fail(ZK_ERR_UNSUPPORTED, "typed witness columns in a sharded session (world %u) are not supported: pass Montgomery columns to zk_proof_advice_phase", pr->world);
    return advice_phase_impl(ctx, pr, col_index, h_cols, ncols, h_challenges, num_challenges, false, false, widths);
}
// The same phase for witness columns that are RESIDENT ON THE DEVICE (n x 32 B each, Montgomery, device pointers): a witness
// generated on the GPU, or one uploaded ahead of the proof.  Judged small / dense on the device.  Same transcript, same bytes as the
// host-column call.  flags:
//   0                        the columns are copied (device to device, on the copy stream) into the session's own buffers; the caller's
//                            stay untouched
//   ZK_ADVICE_DEV_IN_PLACE   the session works IN the caller's buffers: it overwrites their last blinding_factors + 1 rows (the rows
//                            halo2 fills with blinding values; a witness has nothing there) and reads them until zk_proof_finish /
//                            zk_proof_abort returns.  No copy, and n x 32 B per column less device memory -- which is what lets a
//                            1000-column session keep two cosets of every column computed ahead.
int zk_proof_advice_phase_dev(zk_ctx* ctx, zk_proof* pr, const uint32_t* col_index, const void* const* d_cols, uint32_t ncols, uint32_t flags, void* h_challenges, uint32_t* num_challenges) {
    if (!ctx) return ZK_ERR_INVALID_ARG;
    ZK_REQUIRE(ctx, (flags & ~(uint32_t)ZK_ADVICE_DEV_IN_PLACE) == 0, "unknown flag");
    return advice_phase_impl(ctx, pr, col_index, d_cols, ncols, h_challenges, num_challenges, true, (flags & ZK_ADVICE_DEV_IN_PLACE) != 0);
}
// The typed phase for cells RESIDENT ON THE DEVICE (d_cols[j]: at least usable_rows packed cells of widths[j] bytes, or an n x 32 B
// Montgomery column): a witness kernel's bytes, flags, counters and 128-bit halves become the session's Lagrange columns without a
// caller-side n x 32 B copy -- sixteen narrow columns per k_fr_from_uint_batch launch, written straight into the session's buffers on
// the copy stream.  The caller's buffers are only read, and not after the call returns.  Same transcript, same bytes.
int zk_proof_advice_phase_typed_dev(zk_ctx* ctx, zk_proof* pr, const uint32_t* col_index, const void* const* d_cols, const uint8_t* widths, uint32_t ncols, void* h_challenges, uint32_t* num_challenges) {
    if (!ctx) return ZK_ERR_INVALID_ARG;
    ZK_REQUIRE(ctx, pr && widths, "null pointer");
    for (uint32_t j = 0; j < ncols; ++j) {
        const uint8_t w = widths[j];
        if (w != 1 && w != 2 && w != 4 && w != 8 && w != 16 && w != 32) return ctx->fail(ZK_ERR_INVALID_ARG, "column %u: cell width %u (must be 1, 2, 4, 8, 16 or 32 bytes)", j, (unsigned)w);
        if (d_cols && (uintptr_t)d_cols[j] % (w < 32 ? w : 8)) return ctx->fail(ZK_ERR_INVALID_ARG, "column %u: cells of %u bytes at a misaligned address", j, (unsigned)w);
    }
    if (pr->world > 1) return ctx->fail(ZK_ERR_UNSUPPORTED, "typed witness columns in a sharded session (world %u) are not supported: pass Montgomery columns to zk_proof_advice_phase_dev", pr->world);
    return advice_phase_impl(ctx, pr, col_index, d_cols, ncols, h_challenges, num_challenges, true, false, widths);
}
static int advice_phase_impl(zk_ctx* ctx, zk_proof* pr, const uint32_t* col_index, const void* const* h_cols, uint32_t ncols, void* h_challenges, uint32_t* num_challenges, bool dev_src, bool in_place,
                             const uint8_t* widths) {
    if (!ctx) return ZK_ERR_INVALID_ARG;
    PoolScope pool_scope(ctx);
    ZK_REQUIRE(ctx, pr && (ncols == 0 || (col_index && h_cols)), "null pointer");
    const zk_pk* pk = pr->pk;
    if (pr->phase >= pk->num_phases) return ctx->fail(ZK_ERR_INVALID_ARG, "all %u advice phases are already committed", pk->num_phases);
    const size_t n = (size_t)1 << pk->k;
    uint32_t expected = 0, phase_challenges = 0;
    for (uint32_t i = 0; i < pk->A; ++i) expected += pk->adv_phase[i] == pr->phase;
    for (uint32_t cp : pk->chal_phase) phase_challenges += cp == pr->phase;
    if (h_challenges && (!num_challenges || *num_challenges < phase_challenges))
        return ctx->fail(ZK_ERR_INVALID_ARG, "phase %u yields %u challenges: pass a buffer for at least that many and its capacity in *num_challenges", pr->phase, phase_challenges);
    if (ncols != expected) return ctx->fail(ZK_ERR_INVALID_ARG, "phase %u has %u advice columns, %u were passed", pr->phase, expected, ncols);
    // Sharded session with a device all-gather and a device-resident witness: a rank holds only the columns it OWNS (position j of
    // the phase's columns in ascending column order, j % world == rank); the others arrive over the fabric and may be passed as NULL.
    const bool owner_only = dev_src && pr->world > 1 && pr->gather && pr->gather_dev;
    std::vector<const void*> by_col(pk->A, nullptr);
    std::vector<uint8_t> seen(pk->A, 0), width_of(pk->A, 32);
    for (uint32_t j = 0; j < ncols; ++j) {
        const uint32_t c = col_index[j];
        if (c >= pk->A || pk->adv_phase[c] != pr->phase || seen[c] || (!h_cols[j] && !owner_only)) return ctx->fail(ZK_ERR_INVALID_ARG, "advice column %u does not belong to phase %u (or is repeated)", c, pr->phase);
        by_col[c] = h_cols[j];
        seen[c] = 1;
        if (widths) width_of[c] = widths[j];
    }
    if (owner_only) {
        uint32_t pos = 0;
        for (uint32_t c = 0; c < pk->A; ++c) {
            if (!seen[c]) continue;
            if (pos % pr->world == pr->rank && !by_col[c]) return ctx->fail(ZK_ERR_INVALID_ARG, "advice column %u is owned by this rank (position %u of the phase, rank %u of %u) and was passed as NULL", c, pos, pr->rank, pr->world);
            ++pos;
        }
    }
    if (dev_src) pr->advice_on_device = true;
    if (in_place) {
        std::vector<const void*> sorted_ptrs;
        for (uint32_t j = 0; j < ncols; ++j) if (h_cols[j]) sorted_ptrs.push_back(h_cols[j]);
        std::sort(sorted_ptrs.begin(), sorted_ptrs.end());
        if (std::adjacent_find(sorted_ptrs.begin(), sorted_ptrs.end()) != sorted_ptrs.end()) return ctx->fail(ZK_ERR_INVALID_ARG, "in-place witness columns must be distinct buffers (each gets its own blinding rows)");
        pr->advice_in_place = true;
    }
    StageTrace trace(ctx);
    // Column c+1 is uploaded on the copy stream while the MSM of column c runs; the last bf + 1 rows
    // (u .. n - 1) of every column are blinding values (drawn up front, in column-index = transcript order).
    struct Stage {
        zk_ctx* ctx; size_t body, tail;
        std::vector<const void*> src; std::vector<void*> dst; std::vector<F4> blind_v; const F4* blind = nullptr;
        std::vector<uint8_t> width;                                      // bytes per cell of src[c]: below 32, the column is uploaded packed and expanded on the device
        void* packed = nullptr;                                          // staging of ONE packed column: upload and expansion share the in-order copy stream, so the next upload cannot overtake the expansion
        bool grouped = false; size_t expanded = 0;                       // typed cells resident on the device: columns [0, expanded) are on the copy stream, a group of FU_GROUP per staging call that runs out of them
        uint32_t world = 1;
        hipMemcpyKind kind = hipMemcpyHostToDevice;                       // device-resident witness: device to device
        std::vector<size_t> own;                                         // device-gather mode: only these columns are uploaded by this rank
        const zk_pk* pk = nullptr; std::vector<DevBuf*> lag, coeff;     // coefficient forms are produced as the columns arrive
        // plain (unsharded) sessions: coefficient forms AND the planned cosets of the columns, several columns per launch, on the
        // auxiliary stream behind their uploads
        zk_proof* pr = nullptr; std::vector<uint32_t> col; std::vector<size_t> pending; std::vector<Fr> g_of_r;
        int flush() {
            if (pending.empty()) return ZK_OK;
            StreamRestore back(ctx);
            ctx->stream = ctx->stream_aux;
            const size_t n_ = (size_t)1 << pk->k;
            std::vector<Fr*> dsts;
            std::vector<const Fr*> srcs;
            for (size_t c_ : pending) {
                PK_ALLOC(ctx, *coeff[c_], n_ * 32);
                dsts.push_back(coeff[c_]->fr());
                srcs.push_back(lag[c_]->fr());
            }
            const Fr omega_inv = fr_inv_host(fr_root_of_unity(pk->k)), ninv = fr_inv_host(fr_from_u64(1ull << pk->k));
            PK_TRY(ntt_run_many(ctx, dsts.data(), srcs.data(), dsts.size(), pk->k, omega_inv, &ninv, nullptr, nullptr, false));
            for (size_t r = 0; r < g_of_r.size(); ++r) {
                std::vector<const void*> csrc;
                std::vector<void*> cdst;
                for (size_t c_ : pending) {
                    const uint32_t gc = col[c_];
                    if (!(pr->pre_mask[gc] >> r & 1u)) continue;
                    DevBuf& slot = pr->adv_coset[r][gc];
                    if (!slot.alloc(n_ * coset_row_bytes(session_records(pr)))) {          // the estimate was too generous: stop computing ahead, the quotient transforms the rest itself
                        for (uint32_t& m_ : pr->pre_mask) m_ = 0;
                        break;
                    }
                    csrc.push_back(coeff[c_]->p);
                    cdst.push_back(slot.p);
                }
                if (!csrc.empty()) PK_TRY(coeff_to_coset_batch_fmt(ctx, csrc.data(), pk->k, g_of_r[r], cdst.data(), csrc.size(), session_records(pr)));
            }
            pending.clear();
            return ZK_OK;
        }
    } sg{ctx, (size_t)pk->u * 32, (size_t)(pk->bf + 1) * 32, {}, {}, {}};   // halo2: advice_values[n - (blinding_factors + 1)..] are random, row u included
    sg.pk = pk;
    sg.pr = pr;
    sg.kind = dev_src ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    sg.grouped = dev_src && widths;
    for (uint32_t c = 0; c < pk->A; ++c) {        // column-index order = transcript order
        if (!seen[c]) continue;
        if (in_place && by_col[c] && (!owner_only || sg.dst.size() % pr->world == pr->rank)) pr->adv_lag[c].borrow(const_cast<void*>(by_col[c]));
        else if (!pr->adv_lag[c].alloc(n * 32)) return ctx->fail(ZK_ERR_OOM, "prover: alloc of %zu bytes failed", n * 32);
        sg.src.push_back(by_col[c]);
        sg.width.push_back(width_of[c]);
        sg.dst.push_back(pr->adv_lag[c].p);
        sg.lag.push_back(&pr->adv_lag[c]);
        sg.coeff.push_back(&pr->adv_coeff[c]);
        sg.col.push_back(c);
        for (uint32_t r = 0; r <= pk->bf; ++r) sg.blind_v.push_back(pr->rng.next_fr());
    }
    DevBuf packed_buf;                            // back in the pool when the phase returns: by then the main stream has waited for the last expansion
    size_t widest_packed = 0;
    for (uint8_t w : sg.width) if (w < 32) widest_packed = std::max<size_t>(widest_packed, w);
    if (widest_packed && !sg.grouped) {        // cells already on the device are expanded from where they are
        PK_ALLOC(ctx, packed_buf, (size_t)pk->u * widest_packed);
        sg.packed = packed_buf.p;
    }
    PinnedBuf blind_pinned;
    if (!blind_pinned.alloc(sg.blind_v.size() * sizeof(F4))) return ctx->fail(ZK_ERR_OOM, "prover: pinned staging allocation failed");
    memcpy(blind_pinned.p, sg.blind_v.data(), sg.blind_v.size() * sizeof(F4));
    sg.blind = (const F4*)blind_pinned.p;
    trace.mark("  advice: blinding rows drawn and staged");
    PK_TRY(copy_stream_open(ctx));
    if (!ctx->ensure_aux()) return ctx->fail(ZK_ERR_HIP, "could not create the auxiliary stream");
    ZK_HIP(ctx, hipEventRecord(ctx->ev_aux, ctx->stream));                 // pooled blocks: everything enqueued so far comes first
    ZK_HIP(ctx, hipStreamWaitEvent(ctx->stream_aux, ctx->ev_aux, 0));
    // Sharded session: every rank uploads every column (each GPU has its own PCIe link; all of them
    // are needed for the quotient) but commits only columns rank, rank + world, ...: the upload of
    // `world` columns hides one MSM.
    sg.world = pr->world > 1 && pr->gather ? pr->world : 1;
    if (!pr->pre_planned) PK_TRY(plan_advice_cosets(ctx, pr));
    trace.mark("  advice: coset plan");
    if (sg.world == 1 && !pr->adv_coset.empty()) {
        const Fr w_ext = fr_root_of_unity(pk->ext_k);
        Fr g = fr_zeta();
        for (size_t r = 0; r < pr->adv_coset.size(); ++r) { sg.g_of_r.push_back(g); g = g * w_ext; }
    }
    auto stage = [](void* user, size_t it) -> int {
        Stage* s_ = (Stage*)user;
        if (!s_->own.empty()) {      // device-gather mode: one own column per call
            if (it > 0) PK_TRY(to_coeff_aux(s_->ctx, s_->pk, *s_->lag[s_->own[it - 1]], s_->coeff[s_->own[it - 1]]));
            const size_t c_ = s_->own[it];
            if (s_->dst[c_] != s_->src[c_]) ZK_HIP(s_->ctx, hipMemcpyAsync(s_->dst[c_], s_->src[c_], s_->body, s_->kind, s_->ctx->stream_copy));
            ZK_HIP(s_->ctx, hipMemcpyAsync((char*)s_->dst[c_] + s_->body, s_->blind + c_ * (s_->tail / 32), s_->tail, hipMemcpyHostToDevice, s_->ctx->stream_copy));
            PK_TRY(copy_stream_fence(s_->ctx));
            ZK_HIP(s_->ctx, hipStreamWaitEvent(s_->ctx->stream_aux, s_->ctx->ev_copy, 0));
            return ZK_OK;
        }
        // the group uploaded by the previous call is on the device (the main stream has waited for it):
        // its lagrange_to_coeff runs now, on a main stream that is otherwise waiting for PCIe
        if (it > 0 && s_->world == 1) {
            s_->pending.push_back(it - 1);
            static const size_t flush_at = [] { const char* e = getenv("ZK_ADVICE_NTT_GROUP"); const int v = e ? atoi(e) : 32; return (size_t)(v < 1 ? 1 : v > 64 ? 64 : v); }();      // measurement knob
            if (s_->pending.size() >= flush_at) PK_TRY(s_->flush());        // two launch pairs of sixteen columns (ntt_run_many's granularity at k = 20) per hand-over to the auxiliary stream: headline 0.9785 / 0.9882 s with 16, 0.9738 / 0.9851 with 32, 0.9812 with 64, 0.9788 with 8 (two alternating A/B runs)
        } else if (it > 0)
            for (size_t c_ = (it - 1) * s_->world; c_ < std::min(it * (size_t)s_->world, s_->dst.size()); ++c_)
                PK_TRY(to_coeff_aux(s_->ctx, s_->pk, *s_->lag[c_], s_->coeff[c_]));
        static const bool skip_upload = getenv("ZK_DEBUG_SKIP_UPLOAD") != nullptr;       // measurement only (the proof is garbage): is the phase bound by PCIe or by the device?
        for (size_t c_ = it * s_->world; c_ < std::min((it + 1) * (size_t)s_->world, s_->dst.size()); ++c_) {
            if (skip_upload) continue;
            if (s_->grouped) {
                // the narrow columns of sixteen consecutive columns in one launch, from the caller's cells into the session's buffers; the
                // Montgomery columns among them are copied, and every column gets its blinding rows.  The calls for the other fifteen only fence.
                if (c_ < s_->expanded) continue;
                constexpr size_t FU_GROUP = 16;
                const size_t g1 = std::min(c_ + FU_GROUP, s_->dst.size());
                const void* gsrc[FU_GROUP]; Fr* gdst[FU_GROUP]; uint8_t gw[FU_GROUP];
                size_t cnt = 0;
                for (size_t g = c_; g < g1; ++g) {
                    if (s_->width[g] < 32) { gsrc[cnt] = s_->src[g]; gdst[cnt] = (Fr*)s_->dst[g]; gw[cnt] = s_->width[g]; ++cnt; }
                    else ZK_HIP(s_->ctx, hipMemcpyAsync(s_->dst[g], s_->src[g], s_->body, s_->kind, s_->ctx->stream_copy));
                }
                PK_TRY(fr_from_uint_batch_run(s_->ctx, s_->ctx->stream_copy, gsrc, gw, cnt, s_->body / 32, gdst));
                for (size_t g = c_; g < g1; ++g)
                    ZK_HIP(s_->ctx, hipMemcpyAsync((char*)s_->dst[g] + s_->body, s_->blind + g * (s_->tail / 32), s_->tail, hipMemcpyHostToDevice, s_->ctx->stream_copy));
                s_->expanded = g1;
                continue;
            }
            if (s_->width[c_] < 32) {                                     // typed cells: body / 32 rows of width bytes, expanded behind the upload
                ZK_HIP(s_->ctx, hipMemcpyAsync(s_->packed, s_->src[c_], s_->body / 32 * s_->width[c_], hipMemcpyHostToDevice, s_->ctx->stream_copy));
                PK_TRY(fr_from_uint_run(s_->ctx, s_->ctx->stream_copy, s_->packed, s_->width[c_], s_->body / 32, (Fr*)s_->dst[c_]));
            } else if (s_->dst[c_] != s_->src[c_]) ZK_HIP(s_->ctx, hipMemcpyAsync(s_->dst[c_], s_->src[c_], s_->body, s_->kind, s_->ctx->stream_copy));      // in place: only the blinding rows move
            ZK_HIP(s_->ctx, hipMemcpyAsync((char*)s_->dst[c_] + s_->body, s_->blind + c_ * (s_->tail / 32), s_->tail, hipMemcpyHostToDevice, s_->ctx->stream_copy));
        }
        PK_TRY(copy_stream_fence(s_->ctx));
        ZK_HIP(s_->ctx, hipStreamWaitEvent(s_->ctx->stream_aux, s_->ctx->ev_copy, 0));      // the aux stream transforms what was just uploaded
        return ZK_OK;
    };
    std::vector<G1Affine> coms(sg.dst.size());
    std::vector<uint8_t> narrow(sg.src.size());
    if (owner_only) {                             // only this rank's own columns are on this device (and only they are committed here)
        std::vector<const void*> own_src;
        for (size_t c_ = pr->rank; c_ < sg.src.size(); c_ += pr->world) own_src.push_back(sg.src[c_]);
        std::vector<uint8_t> own_narrow(own_src.size());
        PK_TRY(sample_narrow_dev(ctx, own_src.data(), own_src.size(), n, own_narrow.data()));
        for (size_t j = 0; j < own_src.size(); ++j) narrow[pr->rank + j * pr->world] = own_narrow[j];
    } else if (dev_src && widths) PK_TRY(sample_narrow_dev_typed(ctx, sg.src.data(), sg.width.data(), sg.src.size(), n, pk->u, narrow.data()));
    else if (dev_src) PK_TRY(sample_narrow_dev(ctx, sg.src.data(), sg.src.size(), n, narrow.data()));
    else if (!widths) sample_narrow(sg.src.data(), sg.src.size(), n, narrow.data());       // witness columns of (mostly) small values take the per-window MSM path
    else {
        // typed cells: 8 bytes or fewer are below 2^64 by construction; 16-byte cells are sampled as the integers they are (same rule: at
        // most a quarter of the samples at 2^64 or above), Montgomery columns as ever
        std::vector<const void*> fr_only(sg.src.size(), nullptr);
        for (size_t c_ = 0; c_ < sg.src.size(); ++c_) if (sg.width[c_] == 32) fr_only[c_] = sg.src[c_];
        sample_narrow(fr_only.data(), fr_only.size(), n, narrow.data());
        const size_t samples = std::min<size_t>(pk->u, 1024), step = pk->u / (samples ? samples : 1);
        for (size_t c_ = 0; c_ < sg.src.size(); ++c_) {
            if (sg.width[c_] <= 8) narrow[c_] = 1;
            if (sg.width[c_] != 16) continue;
            size_t large = 0;
            for (size_t i = 0; i < samples; ++i) large += ((const uint64_t*)sg.src[c_])[2 * (i * step) + 1] != 0;
            narrow[c_] = large <= samples / 4;
        }
    }
    trace.mark("  advice: columns sampled");
    // ... and their blinding rows (the last blinding_factors + 1, field-sized) are committed apart, so that they do not occupy every window
    struct TailGuard { zk_ctx* c; ~TailGuard() { c->msm_blinded_tail = 0; } } tail_guard{ctx};
    ctx->msm_blinded_tail = pk->bf + 1;
    if (sg.world == 1) {
        PK_TRY(commit_batch_staged(ctx, pk->srs, 1, (const void* const*)sg.dst.data(), sg.dst.size(), n, coms.data(), stage, &sg, narrow.data()));
        if (!sg.dst.empty()) {                    // the last column (its upload was fenced into the auxiliary stream by the last staging call) and what is pending
            sg.pending.push_back(sg.dst.size() - 1);
            PK_TRY(sg.flush());
        }
    } else {
        const size_t total = sg.dst.size(), per = (total + sg.world - 1) / sg.world;
        std::vector<const void*> mine;
        std::vector<uint8_t> mine_narrow;
        for (size_t c_ = pr->rank; c_ < total; c_ += sg.world) { mine.push_back(sg.dst[c_]); mine_narrow.push_back(narrow[c_]); }
        std::vector<G1Affine> local(per), all(per * sg.world);
        memset((void*)local.data(), 0, sizeof(G1Affine) * per);
        if (pr->gather_dev) {
            // Device all-gather mode: this rank uploads only ITS columns (1/world of the PCIe traffic),
            // commits them, and the ranks then exchange the columns group by group over the fabric.
            for (size_t c_ = pr->rank; c_ < total; c_ += sg.world) sg.own.push_back(c_);
            PK_TRY(commit_batch_staged(ctx, pk->srs, 1, mine.data(), mine.size(), n, local.data(), stage, &sg, mine_narrow.data()));
            // The exchange goes SEVERAL groups of `world` columns at a time (ZK_SHARD_EXCHANGE_GROUPS, default 16): this rank's columns of the chunk are packed into one
            // send buffer and ONE all-gather moves world x 16 columns -- fewer, larger collectives (a collective per column group was 125 host-synchronised rounds of
            // 32 MB per rank at eight ranks; RCCL over point-to-point xGMI wants its messages large).
            static const size_t xg_knob = getenv("ZK_SHARD_EXCHANGE_GROUPS") ? (size_t)atol(getenv("ZK_SHARD_EXCHANGE_GROUPS")) : 16;
            const size_t groups_total = (total + sg.world - 1) / sg.world, XG = std::max<size_t>(1, std::min(xg_knob, groups_total));
            DevBuf gbuf, sbuf;
            PK_ALLOC(ctx, gbuf, (size_t)sg.world * XG * n * 32); PK_ALLOC(ctx, sbuf, XG * n * 32);
            // the last own column of the phase has not been transformed yet (the staging callback transforms column i - 1 when it uploads column i; the auxiliary
            // stream already waits for its upload): the exchange below may ship its coefficient form
            for (size_t c_ : sg.own) if (!sg.coeff[c_]->p) PK_TRY(to_coeff_aux(ctx, pk, *sg.lag[c_], sg.coeff[c_]));
            // the transforms of this rank's own columns still run on the auxiliary stream and share the NTT
            // scratch with the ones enqueued below on the main stream: finish them first
            ZK_HIP(ctx, hipStreamSynchronize(ctx->stream_aux));
            // WHAT travels (round 6): the owner has transformed its column already, and a column that no program over the Lagrange domain reads on this side of the
            // boundary -- no lookup tuple, not a permutation column, no remainder of the additive split: on the EVM-style shape 544 of 1000 -- is needed by its peers in
            // coefficient form only (cosets, evaluations, multi-open).  It is shipped in THAT form: same bytes, no inverse transform on the seven other ranks.
            // ZK_SHARD_COEFF=0 ships every column as Lagrange values (and every rank transforms every column), as before.
            std::vector<uint8_t> need_lag;
            PK_TRY(advice_lagrange_readers(ctx, pk, &need_lag));
            static const bool ship_coeff = !(getenv("ZK_SHARD_COEFF") && atoi(getenv("ZK_SHARD_COEFF")) == 0);
            auto as_coeff = [&](size_t c_) { return ship_coeff && !need_lag[sg.col[c_]]; };
            for (size_t grp0 = 0; grp0 < groups_total; grp0 += XG) {
                const size_t gcnt = std::min(XG, groups_total - grp0);
                for (size_t g = 0; g < gcnt; ++g) {
                    const size_t mine_c = (grp0 + g) * sg.world + pr->rank;
                    if (mine_c < total) {
                        const void* src_ = sg.dst[mine_c];
                        if (as_coeff(mine_c)) {
                            if (!sg.coeff[mine_c]->p) return ctx->fail(ZK_ERR_INVALID_ARG, "sharded session: the coefficient form of an own column is missing at the exchange");
                            src_ = sg.coeff[mine_c]->p;
                        }
                        ZK_HIP(ctx, hipMemcpyAsync((char*)sbuf.p + g * n * 32, src_, n * 32, hipMemcpyDeviceToDevice, ctx->stream));
                    } else ZK_HIP(ctx, hipMemsetAsync((char*)sbuf.p + g * n * 32, 0, n * 32, ctx->stream));
                }
                PK_TRY(zk_ctx_sync(ctx));                                  // own columns uploaded and packed, previous copies out of gbuf done
                if (pr->gather_dev(pr->gather_dev_user, sbuf.p, gcnt * n * 32, gbuf.p))
                    return ctx->fail(ZK_ERR_INVALID_ARG, "sharded session: device all-gather callback failed");
                for (size_t g = 0; g < gcnt; ++g)
                    for (uint32_t q_ = 0; q_ < sg.world; ++q_) {
                        const size_t c_ = (grp0 + g) * sg.world + q_;
                        if (q_ == pr->rank || c_ >= total) continue;
                        const char* got = (const char*)gbuf.p + ((size_t)q_ * gcnt + g) * n * 32;
                        if (as_coeff(c_)) {
                            PK_ALLOC(ctx, *sg.coeff[c_], n * 32);
                            ZK_HIP(ctx, hipMemcpyAsync(sg.coeff[c_]->p, got, n * 32, hipMemcpyDeviceToDevice, ctx->stream));
                            sg.lag[c_]->release();                   // nobody reads the Lagrange form of this column here
                            pr->lag_partial = true;
                        } else {
                            ZK_HIP(ctx, hipMemcpyAsync(sg.dst[c_], got, n * 32, hipMemcpyDeviceToDevice, ctx->stream));
                            PK_TRY(to_coeff(ctx, pk, *sg.lag[c_], sg.coeff[c_]));
                        }
                    }
            }
        } else {
            PK_TRY(commit_batch_staged(ctx, pk->srs, 1, mine.data(), mine.size(), n, local.data(), stage, &sg, mine_narrow.data()));   // MSM j reads group j of `world` columns
            for (size_t grp = mine.size(); grp * sg.world < total; ++grp) PK_TRY(stage(&sg, grp));                   // a last group without a column of this rank
        }
        PK_TRY(zk_ctx_sync(ctx));
        if (per && pr->gather(pr->gather_user, local.data(), per * sizeof(G1Affine), all.data())) return ctx->fail(ZK_ERR_INVALID_ARG, "sharded session: all-gather callback failed");
        for (size_t c_ = 0; c_ < total; ++c_) coms[c_] = all[(c_ % sg.world) * per + c_ / sg.world];
    }
    ZK_HIP(ctx, hipEventRecord(ctx->ev_aux, ctx->stream_aux));             // the main stream continues after the transforms
    ZK_HIP(ctx, hipStreamWaitEvent(ctx->stream, ctx->ev_aux, 0));
    trace.mark("advice upload + commits");
    for (const G1Affine& com : coms) pr->tr.write_point(com);
    uint32_t written = 0;
    for (uint32_t i = 0; i < pk->chal_phase.size(); ++i) {
        if (pk->chal_phase[i] != pr->phase) continue;
        pr->challenges[i] = pr->tr.squeeze();
        if (h_challenges) memcpy((uint8_t*)h_challenges + 32 * written, &pr->challenges[i], 32);
        ++written;
    }
    if (num_challenges) *num_challenges = written;
    if (pr->tr.err) return ctx->fail(ZK_ERR_INVALID_ARG, "external transcript callback failed with status %d", pr->tr.err);
    pr->absorbed.clear();
    pr->absorbed.shrink_to_fit();
    ++pr->phase;
    return ZK_OK;
}

// The quotient's plan of a key (quotient_plan.hpp): a pure function of the constraint system and of the knobs, so it is made once
// per key (zk_pk::qplan), again when a knob changed since, and shared by the advice phases (which cosets read which column) and
// zk_proof_finish.
static int quotient_plan(zk_ctx* ctx, const zk_pk* pk, std::shared_ptr<const QuotientPlan>* out) {
    const QuotientKnobs knobs = QuotientKnobs::read();
    if (!pk->qplan || pk->qplan->key != knobs.key()) {
        std::string err;
        const int rc = choose_quotient_plan(*pk, knobs, &pk->qplan, &err);
        if (rc) return ctx->fail(rc, "%s", err.c_str());
    }
    *out = pk->qplan;
    return ZK_OK;
}
// advice_coset_masks / advice_lagrange_readers (quotient_plan.hpp) of the key's plan
static int advice_coset_plan(zk_ctx* ctx, const zk_pk* pk, std::vector<uint32_t>& mask, size_t* key_slots = nullptr) {
    std::shared_ptr<const QuotientPlan> qp;
    PK_TRY(quotient_plan(ctx, pk, &qp));
    advice_coset_masks(*pk, *qp, mask, key_slots);
    return ZK_OK;
}
static int advice_lagrange_readers(zk_ctx* ctx, const zk_pk* pk, std::vector<uint8_t>* need) {
    std::shared_ptr<const QuotientPlan> qp;
    PK_TRY(quotient_plan(ctx, pk, &qp));
    advice_lagrange_readers(*pk, *qp, need);
    return ZK_OK;
}


// Which cosets of which advice columns this session computes ahead, during its advice phases (zk_proof::pre_mask, adv_coset).
// Cosets are taken in the order of how many advice columns they serve, as long as the buffers fit what the device can spare:
// free memory (the pool's parked blocks count as free) less everything the session still has to allocate -- Lagrange and
// coefficient forms of the advice columns, of m / phi / Z, one coset buffer per column the quotient reads, h -- less the
// key's own coset cache if it is still to be filled, capped by ZK_ADVICE_COSET_GB (default 64; 0 turns the feature off).
// Sharded sessions do not precompute (their quotient is split by coset over the ranks).
static int plan_advice_cosets(zk_ctx* ctx, zk_proof* pr) {
    pr->pre_planned = true;
    const zk_pk* pk = pr->pk;
    const bool sharded = pr->world > 1 && pr->gather;
    const char* env = getenv("ZK_ADVICE_COSET_GB");
    // A witness that is already on the device leaves no PCIe wait to fill: the phase is bound by the device's arithmetic, and cosets
    // computed ahead only compete with the commitments (measured on the SuperCircuit shape, 60/30/10 witness, resident columns: two
    // cosets ahead 1.54 s per proof, none 1.41 s).  Off for such sessions unless asked for.
    const double cap = (env ? atof(env) : (pr->advice_on_device ? 0.0 : 64.0)) * (double)(1ull << 30);
    if (sharded || cap <= 0 || pk->A == 0) return ZK_OK;
    std::vector<uint32_t> mask;
    size_t key_slots = 0;
    PK_TRY(advice_coset_plan(ctx, pk, mask, &key_slots));
    const uint32_t E = pk->ext_k - pk->k, R = 1u << E;
    if (E > 5) return ZK_OK;
    const double col_bytes = (double)((size_t)1 << pk->k) * 32.0;
    const double coset_bytes = (double)((size_t)1 << pk->k) * (double)coset_row_bytes(session_records(pr));       // a coset buffer, in the session's format
    bool mem_known = false;
    const size_t free_b = device_free_bytes(&mem_known);
    if (!mem_known) return ZK_OK;            // nothing is computed ahead on a guess
    // columns' worth of buffers still to come, the advice columns' own coset buffers aside (counted below, per choice of cosets):
    // Lagrange + coefficient forms of the advice columns, of m / phi / Z with their temporaries, their coset buffers, h, slack
    // (a witness handed over in place brings its Lagrange forms along)
    const double cols_ahead = (pr->advice_in_place ? 1.0 : 2.0) * pk->A + 3.0 * (2.0 * pk->L + pk->C) + 2.0 * R + 32.0, cosets_ahead = 2.0 * pk->L + pk->C + pk->I + 8.0;
    const double reserve = cols_ahead * col_bytes + cosets_ahead * coset_bytes;
    double avail = (double)free_b + (double)ctx->pool_bytes - reserve - 16.0 * (double)(1ull << 30);
    if (pk->part_cache_state < 0 || (pk->part_cache_state == 1 && pk->part_cache_bytes == 0)) {
        // the key's own cosets (fixed, sigma, l_0 ...) are still to be cached by this proof's quotient: reserved, counted from the
        // class programs (a fixed column read only by low-degree gates is cached on two cosets, not on all)
        const double key_need = (double)key_slots * coset_bytes;
        const char* kenv = getenv("ZK_PK_COSET_CACHE_GB");
        const double kcap = std::min((kenv ? atof(kenv) : 96.0) * (double)(1ull << 30), (double)ctx->prop.totalGlobalMem / 3.0);
        if (key_need <= kcap) avail -= std::max(0.0, key_need - (double)pk->part_cache_bytes);
    }
    const double budget = std::min(cap, avail);
    const auto by_count = cosets_by_columns_served(R, [&](uint32_t r) { uint32_t cnt = 0; for (uint32_t m_ : mask) cnt += m_ >> r & 1u; return cnt; });
    uint32_t chosen = 0;
    double used = 0;
    for (const auto& cr : by_count) {
        uint32_t rest = 0;                       // advice columns the quotient still has to transform itself (one coset buffer each)
        for (uint32_t m_ : mask) rest += (m_ & ~(chosen | 1u << cr.second)) != 0;
        if (used + cr.first * coset_bytes > cap || used + (cr.first + rest) * coset_bytes > avail) break;
        used += cr.first * coset_bytes;
        chosen |= 1u << cr.second;
    }
    if (getenv("ZK_PROVER_TRACE")) {
        fprintf(stderr, "[zk prover] advice coset plan: free %.1f + pooled %.1f GiB, reserve %.1f GiB, budget %.1f GiB, cosets by columns served:", free_b / 1073741824.0, ctx->pool_bytes / 1073741824.0,
                reserve / 1073741824.0 + 16.0, budget / 1073741824.0);
        for (const auto& cr : by_count) fprintf(stderr, " r%u:%u", cr.second, cr.first);
        fprintf(stderr, " -> chosen 0x%x\n", chosen);
    }
    if (!chosen) return ZK_OK;
    pr->pre_mask.assign(pk->A, 0u);
    for (uint32_t c = 0; c < pk->A; ++c) pr->pre_mask[c] = mask[c] & chosen;
    pr->adv_coset.resize(R);
    for (auto& v : pr->adv_coset) v.resize(pk->A);
    if (getenv("ZK_PROVER_TRACE")) fprintf(stderr, "[zk prover] advice cosets computed ahead: cosets 0x%x, %.1f GiB\n", chosen, used / (double)(1ull << 30));
    return ZK_OK;
}

// The plan of a key (what zk_proof_finish follows for it under the knobs in force): same summary as zk_host_quotient_plan.
int zk_pk_quotient_plan(zk_ctx* ctx, const zk_pk* pk, uint32_t* out_summary, size_t cap_summary) {
    if (!ctx) return ZK_ERR_INVALID_ARG;
    ZK_REQUIRE(ctx, pk && out_summary, "null pointer");
    std::shared_ptr<const QuotientPlan> qp;
    PK_TRY(quotient_plan(ctx, pk, &qp));
    if (write_plan_summary(*qp, out_summary, cap_summary, 0xFFFFFFFFu, nullptr, 0, nullptr)) return ctx->fail(ZK_ERR_INVALID_ARG, "zk_pk_quotient_plan: the summary needs %u words", 8 + 8 * (qp->E + 1));
    return ZK_OK;
}


// ================================================================================================
// The finishing pass: everything after the advice phases.  One function per stage of the protocol, called by zk_proof_finish
// (at the end of this part) in transcript order.  `Finish` carries what more than one stage reads; a buffer that only one stage
// uses is a local of that stage's function and goes back to the session pool where the function returns.
struct Finish {
    zk_ctx* ctx;
    zk_proof* pr;
    const zk_pk* pk;
    const zk_srs* srs;
    const uint32_t k, ext_k;
    const size_t n;
    Env lag;                                  // the Lagrange forms, and the challenges as they are squeezed
    StageTrace trace;
    const bool sharded;                       // one of several ranks
    // Sharded sessions (round 6): the lookup arguments are split over the ranks like their commitments -- rank r compresses the tuples, counts the multiplicities and forms the
    // running sum of arguments r, r + world, ... only; the Lagrange forms of m and phi (what the additive split's remainders, the coefficient forms and with them every later
    // stage read) are all-gathered device to device behind each of the two rounds.  The blinding rows are drawn for every argument on every rank (one RNG sequence).
    // ZK_SHARD_LOOKUPS=0: every rank works on every argument, as before.
    const bool shard_args;
    std::vector<uint32_t> act;                // the arguments this rank works on, in order
    std::vector<uint32_t> lk_order;           // `act` in the order the two lookup stages take them: arguments into one table side by side (stage_lookup_multiplicities)
    bool late_cosets = false;                 // the auxiliary stream holds coset transforms of this session's advice columns
    bool records = false;                     // the cosets of this session are coset records (finish_coset_format)
    // lookups: compressed inputs and tables (until the grand sums have read them), m and phi in Lagrange form
    std::vector<std::vector<DevBuf>> lk_f;
    std::vector<DevBuf> lk_t, lk_m, lk_phi;
    std::vector<uint8_t> same_table;          // lookup l reads the table of the lookup this rank worked on before it (lk_t lives at table_owner[l])
    std::vector<uint32_t> table_owner;
    std::vector<DevBuf> pz_lag;               // permutation products, Lagrange form
    // coefficient forms of what the quotient reads and the proof opens
    DevBuf random_coeff;
    std::vector<DevBuf> pz_coeff, m_coeff, phi_coeff, rem_coeff;      // rem_coeff: the remainders of the additive split (CT_SPLIT_R)
    DevBuf h;                                 // the quotient: d - 1 pieces of n coefficients
    // the evaluation point, and the evaluations in the order the proof lists them (marks: where each group starts)
    F4 x, w, w_inv;
    std::vector<Open> evals, queries;         // queries: the multi-open's order
    size_t e_fix = 0, e_random = 0, e_sigma = 0, e_lk = 0;
    std::vector<size_t> e_pz;
    DevBuf hcomb;                             // h(X) = sum_i x^(n i) h_i(X)
    F4 h_eval;

    Finish(zk_ctx* c, zk_proof* p)
        : ctx(c), pr(p), pk(p->pk), srs(p->pk->srs), k(p->pk->k), ext_k(p->pk->ext_k), n((size_t)1 << p->pk->k),
          lag{p->pk, nullptr, &p->adv_lag, &p->inst_lag, nullptr, nullptr, nullptr, host::fr_one(), host::fr_one(), host::fr_one(), host::fr_one(), {}, p->challenges},
          trace(c), sharded(p->world > 1 && p->gather),
          shard_args(sharded && pk->L >= p->world && !(getenv("ZK_SHARD_LOOKUPS") && atoi(getenv("ZK_SHARD_LOOKUPS")) == 0)),
          lk_f(pk->L), lk_t(pk->L), lk_m(pk->L), lk_phi(pk->L), same_table(pk->L, 0), table_owner(pk->L, 0), pz_lag(pk->C),
          pz_coeff(pk->C), m_coeff(pk->L), phi_coeff(pk->L), e_pz(pk->C) {
        for (uint32_t l = 0; l < pk->L; ++l) if (!shard_args || l % pr->world == pr->rank) act.push_back(l);
        const Fr t = fr_root_of_unity(k);
        memcpy(w.l, &t, 32);
        w_inv = host::fr_inv(w);
    }
    Finish(const Finish&) = delete;           // `lag` points into this object
    Finish& operator=(const Finish&) = delete;

    // rotations are points: x w^rot, rot mod n
    F4 rotate(int32_t rot) const { F4 p = x; const F4 b = rot >= 0 ? w : w_inv; for (int32_t i = 0; i < (rot >= 0 ? rot : -rot); ++i) p = host::fr_mul(p, b); return p; }
    int32_t norm_rot(int32_t rot) const { const int64_t nn = (int64_t)n; return (int32_t)((((int64_t)rot % nn) + nn) % nn); }
    F4 point_of(int32_t nrot) const { const int64_t nn = (int64_t)n; return rotate(nrot > nn / 2 ? (int32_t)(nrot - nn) : nrot); }
};

// whatever way zk_proof_finish is left, the auxiliary stream must be through with the session's buffers before they go back to the pool
struct AuxJoin { zk_ctx* c; const bool* on; ~AuxJoin() { if (*on && c->stream_aux) (void)hipStreamSynchronize(c->stream_aux); } };

// ---- more cosets of the advice columns, ahead of the quotient: what the advice phases could not fit (or afford) is
// computed NOW on the auxiliary stream, beside the lookup / permutation / grand-sum stages below -- hash joins, scans,
// batch inversions and chains of small-valued commitments that leave most of the device idle.  Same plan as in the advice
// phase (plan_advice_cosets), with the memory that is free at this point; the quotient waits for the stream before its
// first coset.  OFF by default (ZK_ADVICE_COSET_LATE_GB=<GiB> turns it on): measured on the SuperCircuit shape with 48 GiB
// (tools/gpu_r3v.sh) the quotient's transform stage drops from 237 to 149 ms and the lookup stage beside which the transforms
// run grows from 46 to 118 ms -- 1.437 -> 1.424 s for 25 GiB of device memory: these stages are not idle enough to hide them.
// The budget and the selection rule are NOT plan_advice_cosets': this one reserves 24 GiB and four columns per m / phi / Z
// (there: 16 GiB and three) and skips a coset that does not fit to try a smaller one (there: stops at the first).  Nobody
// recorded why they differ; each is kept as it was measured.
static int stage_late_advice_cosets(Finish& f) {
    zk_ctx* ctx = f.ctx; zk_proof* pr = f.pr; const zk_pk* pk = f.pk; const size_t n = f.n;
    const char* env = getenv("ZK_ADVICE_COSET_LATE_GB");
    const double cap = (env ? atof(env) : 0.0) * (double)(1ull << 30);
    const uint32_t E = f.ext_k - f.k, R = 1u << E;
    if (f.sharded || !(cap > 0) || !pk->A || E > 5 || !ctx->ensure_aux()) return ZK_OK;
    std::vector<uint32_t> mask;
    size_t key_slots = 0;
    PK_TRY(advice_coset_plan(ctx, pk, mask, &key_slots));
    if (pr->adv_coset.empty()) { pr->adv_coset.resize(R); for (auto& v : pr->adv_coset) v.resize(pk->A); }
    const double col_bytes = (double)n * (double)coset_row_bytes(f.records);        // everything counted below is, or is taken to be as large as, a coset buffer
    const size_t free_b = device_free_bytes();          // unknown counts as none
    // still to come: m / phi / Z in Lagrange and coefficient form with their temporaries, their coset buffers, h, slack;
    // the key's own cosets if its cache is still empty
    double avail = (double)free_b + (double)ctx->pool_bytes - (4.0 * (2.0 * pk->L + pk->C) + (2.0 * pk->L + pk->C + pk->I + 8.0) + 2.0 * R + 32.0) * col_bytes - 24.0 * (double)(1ull << 30);
    if (pk->part_cache_state < 0 || (pk->part_cache_state == 1 && pk->part_cache_bytes == 0)) avail -= (double)key_slots * col_bytes;
    auto todo = [&](uint32_t r, uint32_t c) { return (mask[c] >> r & 1u) && !pr->adv_coset[r][c].p && pr->adv_coeff[c].p; };      // still to transform
    const auto by_count = cosets_by_columns_served(R, [&](uint32_t r) { uint32_t cnt = 0; for (uint32_t c = 0; c < pk->A; ++c) cnt += todo(r, c); return cnt; });
    double used = 0;
    StreamRestore back(ctx);
    const hipStream_t main_stream = ctx->stream;
    const Fr w_ext = fr_root_of_unity(f.ext_k);
    for (const auto& cr : by_count) {
        if (used + cr.first * col_bytes > std::min(cap, avail)) continue;          // a smaller coset further down may still fit
        Fr g = fr_zeta();
        for (uint32_t i = 0; i < cr.second; ++i) g = g * w_ext;
        std::vector<const void*> csrc;
        std::vector<void*> cdst;
        bool ok = true;
        for (uint32_t c = 0; c < pk->A && ok; ++c) {
            if (!todo(cr.second, c)) continue;
            DevBuf& slot = pr->adv_coset[cr.second][c];
            if (!slot.alloc(n * coset_row_bytes(f.records))) { ok = false; break; }
            csrc.push_back(pr->adv_coeff[c].p);
            cdst.push_back(slot.p);
        }
        if (!f.late_cosets) {          // first batch: the stream starts behind everything the main stream has enqueued (pooled blocks)
            ZK_HIP(ctx, hipEventRecord(ctx->ev_aux, main_stream));
            ZK_HIP(ctx, hipStreamWaitEvent(ctx->stream_aux, ctx->ev_aux, 0));
        }
        ctx->stream = ctx->stream_aux;
        f.late_cosets = true;
        if (!csrc.empty()) PK_TRY(coeff_to_coset_batch_fmt(ctx, csrc.data(), f.k, g, cdst.data(), csrc.size(), f.records));
        ctx->stream = main_stream;
        used += csrc.size() * col_bytes;
        if (!ok) break;
    }
    if (f.late_cosets) {
        ZK_HIP(ctx, hipEventRecord(ctx->ev_aux, ctx->stream_aux));
        if (getenv("ZK_PROVER_TRACE")) fprintf(stderr, "[zk prover] advice cosets computed beside the lookup / permutation stages: %.1f GiB\n", used / (double)(1ull << 30));
    }
    return ZK_OK;
}

// all-gather of columns owned round-robin (column l by rank l % world): a rank's columns packed into one send buffer, several groups of `world` per exchange
static int exchange_owned(Finish& f, std::vector<DevBuf>& cols) {
    zk_ctx* ctx = f.ctx; const zk_proof* pr = f.pr; const size_t n = f.n;
    const size_t total = cols.size(), W = pr->world, groups_total = (total + W - 1) / W;
    static const size_t xg_knob = getenv("ZK_SHARD_EXCHANGE_GROUPS") ? (size_t)atol(getenv("ZK_SHARD_EXCHANGE_GROUPS")) : 16;
    const size_t XG = std::max<size_t>(1, std::min(xg_knob, groups_total));
    DevBuf gbuf, sbuf;
    PK_ALLOC(ctx, gbuf, W * XG * n * 32);
    PK_ALLOC(ctx, sbuf, XG * n * 32);
    HostStaging host;
    for (size_t grp0 = 0; grp0 < groups_total; grp0 += XG) {
        const size_t gcnt = std::min(XG, groups_total - grp0);
        for (size_t g = 0; g < gcnt; ++g) {
            const size_t mine_c = (grp0 + g) * W + pr->rank;
            if (mine_c < total) ZK_HIP(ctx, hipMemcpyAsync((char*)sbuf.p + g * n * 32, cols[mine_c].p, n * 32, hipMemcpyDeviceToDevice, ctx->stream));
            else ZK_HIP(ctx, hipMemsetAsync((char*)sbuf.p + g * n * 32, 0, n * 32, ctx->stream));
        }
        bool on_device = false;
        PK_TRY(allgather_rows(ctx, pr, false, sbuf.p, true, gcnt * n * 32, gbuf.p, host, &on_device));
        if (!on_device) PK_TRY(zk_h2d(ctx, gbuf.p, host.recv.data(), host.recv.size()));
        for (size_t g = 0; g < gcnt; ++g)
            for (uint32_t q_ = 0; q_ < W; ++q_) {
                const size_t c_ = (grp0 + g) * W + q_;
                if (q_ == pr->rank || c_ >= total) continue;
                ZK_HIP(ctx, hipMemcpyAsync(cols[c_].p, (char*)gbuf.p + ((size_t)q_ * gcnt + g) * n * 32, n * 32, hipMemcpyDeviceToDevice, ctx->stream));
            }
        PK_TRY(zk_ctx_sync(ctx));                      // gbuf / sbuf are reused by the next chunk (and freed at the end)
    }
    return ZK_OK;
}

// ZK_LOOKUP_FUSED (default on; =0: the path before it): the two lookup stages compress every tuple they recognise in one launch,
// count an argument's inputs in one launch, invert the denominators out of place and form the running sums of a batch of arguments
// in one launch chain (lookup.hip, vec.hip).  Read at the top of each stage: the tests flip it inside one process.
static bool lookup_fused() { const char* e = getenv("ZK_LOOKUP_FUSED"); return !(e && atoi(e) == 0); }

// The tuples k_lk_compress_many takes (what push_compressed would emit for them is the same polynomial): every element is a column
// read at any rotation, a constant, or F * column / column * F with F a single column read.  Of two column reads under a product the
// factor is the one all elements share (the first operands are tried before the second ones, as push_compressed does), else the
// first.  Constants are appended to `consts`; the element's pointer is set once they have an address (flags: LK_ELEM_CONST, rot =
// index into consts).  false: the tuple keeps run_program.
static bool recognise_tuple(const Env& e, const std::vector<Prog>& exprs, LkTuple* d, std::vector<F4>* consts) {
    if (exprs.empty() || exprs.size() > LK_TUPLE_MAX) return false;
    const size_t consts0 = consts->size();
    auto decline = [&] { consts->resize(consts0); return false; };
    const size_t w = exprs.size();
    bool all_products = true;
    for (const Prog& g : exprs) {
        const bool leaf = g.size() == 1 && (g[0].op == Q_PUSH_COL || g[0].op == Q_PUSH_CONST);
        const bool product = g.size() == 3 && g[0].op == Q_PUSH_COL && g[1].op == Q_PUSH_COL && g[2].op == Q_MUL;
        if (!leaf && !product) return false;
        all_products = all_products && product;
    }
    int common = -1;          // operand (0 / 1) that is the same column read in every element
    if (all_products && w >= 2)
        for (int side = 0; side < 2 && common < 0; ++side) {
            bool same = true;
            for (size_t i = 1; i < w && same; ++i) same = exprs[i][side].a == exprs[0][side].a && exprs[i][side].b == exprs[0][side].b;
            if (same) common = side;
        }
    memset((void*)d, 0, sizeof *d);
    d->width = (uint32_t)w;
    d->common = common >= 0;
    for (size_t i = 0; i < w; ++i) {
        const Prog& g = exprs[i];
        if (g.size() == 1 && g[0].op == Q_PUSH_CONST) {
            F4 v;
            if (!resolve_const(e, g[0].a, &v)) return decline();
            d->flags[i] = LK_ELEM_CONST;
            d->rot[i] = (int32_t)consts->size();
            consts->push_back(v);
            continue;
        }
        const int fside = g.size() == 3 ? (common >= 0 ? common : 0) : -1;
        const Instr& c = g.size() == 3 ? g[1 - fside] : g[0];
        d->col[i] = (const Fr*)resolve_col(e, c.a);
        d->rot[i] = (int32_t)c.b;
        if (!d->col[i]) return decline();
        if (fside >= 0) {
            d->fac[i] = (const Fr*)resolve_col(e, g[fside].a);
            d->frot[i] = (int32_t)g[fside].b;
            if (!d->fac[i]) return decline();
        }
    }
    return true;
}

// ---- lookups, round 1 (mv_lookup::prover::Argument::prepare): theta-compressed table and input tuples,
// multiplicities m over ALL input tuples of the argument.  Every lookup is enqueued back to back
// (compression programs, device hash join); one download of the status words, one pipelined batch
// of commits.  The unusable rows of m stay zero, as upstream leaves them.
static int stage_lookup_multiplicities(Finish& f) {
    zk_ctx* ctx = f.ctx; zk_proof* pr = f.pr; const zk_pk* pk = f.pk; const size_t n = f.n; host::Transcript& tr = pr->tr;
    if (pk->L) {
        Prog prev_table;
        DevBuf status;
        PK_ALLOC(ctx, status, (size_t)pk->L * 4);
        ZK_HIP(ctx, hipMemsetAsync(status.p, 0xFF, (size_t)pk->L * 4, ctx->stream));
        std::vector<const void*> mptrs(pk->L);
        for (uint32_t l = 0; l < pk->L; ++l) {            // every m exists on every rank (the ones of other ranks arrive below)
            PK_ALLOC(ctx, f.lk_m[l], n * 32);
            mptrs[l] = f.lk_m[l].p;
        }
        const bool fused = lookup_fused();
        uint32_t prev_l = 0;
        bool have_prev = false;
        // every tuple the stage compresses: the recognised ones become descriptor rows (one upload, one launch), the others programs
        std::vector<LkTuple> descs;
        std::vector<F4> dconsts;
        std::vector<Prog> table_prog(pk->L);
        std::vector<std::vector<uint8_t>> by_program(pk->L);      // [l][0]: the table, [l][1 + a]: input a -- still to be compressed by run_program
        for (const uint32_t l : f.act) { PB pt; push_compressed(pt, pk->lookups[l].tables); pt.fold(C_ONE); table_prog[l] = std::move(pt.g); }
        // An argument reads the compressed table, the hash and the inverted denominators of the one taken before it when both name the
        // same table.  The fused path takes the arguments table by table, so that holds for EVERY argument into a table, not only for
        // neighbours (100 lookups into 3 tables, interleaved: 3 tables compressed, hashed and inverted instead of 100).  Every argument's m and
        // phi depend on its own tuples alone, and commitments, blinding rows and checks go by argument index: the order is free.
        f.lk_order = f.act;
        if (fused) std::stable_sort(f.lk_order.begin(), f.lk_order.end(), [&](uint32_t x, uint32_t y) {
            auto key = [](const Instr& in) { return std::make_tuple(in.op, in.a, in.b); };
            return std::lexicographical_compare(table_prog[x].begin(), table_prog[x].end(), table_prog[y].begin(), table_prog[y].end(), [&](const Instr& p, const Instr& q) { return key(p) < key(q); });
        });
        for (const uint32_t l : f.lk_order) {
            const auto& lk = pk->lookups[l];
            const Prog& tg = table_prog[l];
            // consecutive arguments into the same table (chunk_lookups() splits a table's inputs over as many arguments as the
            // degree bound needs; the EVM circuit's 80-odd lookups go into a dozen tables): one compressed table, one hash
            static const bool share_tables = !(getenv("ZK_LOOKUP_SHARE") && atoi(getenv("ZK_LOOKUP_SHARE")) == 0);      // measurement knob
            f.same_table[l] = share_tables && have_prev && tg.size() == prev_table.size() && memcmp(tg.data(), prev_table.data(), tg.size() * sizeof(Instr)) == 0;
            f.table_owner[l] = f.same_table[l] ? f.table_owner[prev_l] : l;
            prev_table = tg;
            prev_l = l; have_prev = true;
            by_program[l].assign(1 + lk.inputs.size(), 1);
            LkTuple d;
            if (!f.same_table[l]) {
                PK_ALLOC(ctx, f.lk_t[l], n * 32);
                if (fused && recognise_tuple(f.lag, lk.tables, &d, &dconsts)) { d.dst = f.lk_t[l].fr(); descs.push_back(d); by_program[l][0] = 0; }
            }
            f.lk_f[l].resize(lk.inputs.size());
            for (size_t a = 0; a < lk.inputs.size(); ++a) {
                PK_ALLOC(ctx, f.lk_f[l][a], n * 32);
                if (fused && recognise_tuple(f.lag, lk.inputs[a], &d, &dconsts)) { d.dst = f.lk_f[l][a].fr(); descs.push_back(d); by_program[l][1 + a] = 0; }
            }
        }
        DevBuf dtab;
        if (!descs.empty()) {          // descriptors and the constants they name: one upload for the stage
            const size_t consts_at = descs.size() * sizeof(LkTuple);
            PK_ALLOC(ctx, dtab, consts_at + dconsts.size() * 32 + 32);
            const Fr* d_consts = (const Fr*)((const char*)dtab.p + consts_at);
            for (LkTuple& d : descs)
                for (uint32_t i = 0; i < d.width; ++i)
                    if (d.flags[i] & LK_ELEM_CONST) { d.col[i] = d_consts + d.rot[i]; d.rot[i] = 0; }
            std::vector<uint8_t> host(consts_at + dconsts.size() * 32);
            memcpy(host.data(), descs.data(), consts_at);
            if (!dconsts.empty()) memcpy(host.data() + consts_at, dconsts.data(), dconsts.size() * 32);
            PK_TRY(zk_h2d(ctx, dtab.p, host.data(), host.size()));
            PK_TRY(lookup_compress_many_enqueue(ctx, (const LkTuple*)dtab.p, descs.size(), &f.lag.theta, n));
        }
        for (const uint32_t l : f.lk_order) {
            const auto& lk = pk->lookups[l];
            if (!f.same_table[l] && by_program[l][0]) PK_TRY(run_program(ctx, f.lag, table_prog[l], f.lk_t[l].p));
            std::vector<const Fr*> fptrs;
            for (size_t a = 0; a < lk.inputs.size(); ++a) {
                if (by_program[l][1 + a]) {
                    PB pf;
                    push_compressed(pf, lk.inputs[a]); pf.fold(C_ONE);
                    PK_TRY(run_program(ctx, f.lag, pf.g, f.lk_f[l][a].p));
                }
                fptrs.push_back(f.lk_f[l][a].fr());
            }
            PK_TRY(lookup_multiplicities_enqueue(ctx, fptrs.data(), fptrs.size(), f.lk_t[f.table_owner[l]].fr(), pk->u, f.lk_m[l].fr(), n, (uint32_t*)status.p + l, f.same_table[l], fused));
        }
        std::vector<uint32_t> st(pk->L);
        PK_TRY(zk_d2h(ctx, st.data(), status.p, (size_t)pk->L * 4));
        for (uint32_t l = 0; l < pk->L; ++l)
            if (st[l] != 0xFFFFFFFFu) return ctx->fail(ZK_ERR_INVALID_ARG, "lookup %u: input at row %u is not in the table (witness does not satisfy the circuit)", l, st[l]);
        f.trace.mark("  lookup: m (all lookups)");
        std::vector<G1Affine> coms(pk->L);
        PK_TRY(sharded_commit(ctx, pr, f.srs, 1, mptrs.data(), pk->L, n, coms.data(), 1));      // multiplicities are small counts
        for (const G1Affine& com : coms) tr.write_point(com);
        if (f.shard_args) PK_TRY(exchange_owned(f, f.lk_m));
    }
    f.trace.mark("lookup m");
    f.lag.lk_m = &f.lk_m;
    return ZK_OK;
}

// ---- permutation grand products
// All chunks are enqueued back to back (ratios -> unscaled running products); the chunks are
// chained afterwards with one small download: Z_c = Z_c^raw * prod_{c' < c} Z_c'^raw(omega^u).
static int stage_permutation_products(Finish& f) {
    zk_ctx* ctx = f.ctx; zk_proof* pr = f.pr; const zk_pk* pk = f.pk; const size_t n = f.n; host::XorShiftRng& rng = pr->rng; host::Transcript& tr = pr->tr;
    const F4 one = host::fr_one();
    {   // beta * delta^j for the permutation numerators (here and on the quotient's cosets);  delta = 7^(2^28)
        F4 delta = host::fr_pow(host::fr_from_u64(7), 1ull << 28), cur = f.lag.beta;
        for (uint32_t j = 0; j < pk->P; ++j) { f.lag.beta_delta.push_back(cur); cur = host::fr_mul(cur, delta); }
    }
    DevBuf num, den, tails_d;
    PK_ALLOC(ctx, num, n * 32); PK_ALLOC(ctx, den, n * 32); PK_ALLOC(ctx, tails_d, (size_t)pk->C * 32 + 32);
    for (uint32_t c = 0; c < pk->C; ++c) {
        PB pn, pd;
        const uint32_t j0 = c * pk->chunk, j1 = std::min(pk->P, j0 + pk->chunk);
        for (uint32_t j = j0; j < j1; ++j) {
            pn.col(pk->perm_cols[j]).col(CT_SPECIAL, SP_X).mulc(C_DELTA0 + j).op(Q_ADD).addc(C_GAMMA);
            if (j > j0) pn.op(Q_MUL);
            pd.col(pk->perm_cols[j]).col(CT_SIGMA, j).mulc(C_BETA).op(Q_ADD).addc(C_GAMMA);
            if (j > j0) pd.op(Q_MUL);
        }
        pn.fold(C_ONE); pd.fold(C_ONE);
        PK_TRY(run_program(ctx, f.lag, pn.g, num.p));
        PK_TRY(run_program(ctx, f.lag, pd.g, den.p));
        PK_TRY(zk_fr_batch_invert(ctx, den.p, n));
        PK_TRY(zk_field_vec_op(ctx, ZK_FIELD_FR, ZK_OP_MUL, num.p, den.p, num.p, n));
        PK_ALLOC(ctx, f.pz_lag[c], n * 32);
        PK_TRY(zk_fr_prefix_product(ctx, num.p, f.pz_lag[c].p, n));      // z[0] = 1, z[i+1] = z[i] * ratio[i]
        ZK_HIP(ctx, hipMemcpyAsync((char*)tails_d.p + (size_t)c * 32, (char*)f.pz_lag[c].p + (size_t)pk->u * 32, 32, hipMemcpyDeviceToDevice, ctx->stream));
    }
    std::vector<F4> tails(pk->C);
    if (pk->C) PK_TRY(zk_d2h(ctx, tails.data(), tails_d.p, (size_t)pk->C * 32));
    f.trace.mark("  perm: running products");
    std::vector<F4> blind((size_t)pk->C * pk->bf);
    std::vector<const void*> zptrs(pk->C);
    F4 start = one;
    for (uint32_t c = 0; c < pk->C; ++c) {
        if (c) PK_TRY(zk_fr_scale(ctx, f.pz_lag[c].p, &start, n));       // Z_c(1) = Z_{c-1}(omega^u)
        start = host::fr_mul(start, tails[c]);
        for (uint32_t r_ = 0; r_ < pk->bf; ++r_) blind[(size_t)c * pk->bf + r_] = rng.next_fr();
        ZK_HIP(ctx, hipMemcpyAsync((char*)f.pz_lag[c].p + (n - pk->bf) * 32, blind.data() + (size_t)c * pk->bf, (size_t)pk->bf * 32, hipMemcpyHostToDevice, ctx->stream));
        zptrs[c] = f.pz_lag[c].p;
    }
    f.trace.mark("  perm: chain + blind");
    std::vector<G1Affine> coms(pk->C);
    PK_TRY(sharded_commit(ctx, pr, f.srs, 1, zptrs.data(), pk->C, n, coms.data(), 2));      // running products stay constant over every stretch of rows without copies
    f.trace.mark("  perm: commits");
    for (const G1Affine& com : coms) tr.write_point(com);
    if (pk->C && !host::fr_eq(start, one)) return ctx->fail(ZK_ERR_INVALID_ARG, "permutation argument does not close: copy constraints are not satisfied by the witness");
    f.trace.mark("permutation Z");
    return ZK_OK;
}

// ---- lookups, round 2 (Prepared::commit_grand_sum): phi[0] = 0, phi[i+1] = phi[i] + sum_a 1/(f_a[i]+beta) - m[i]/(t[i]+beta),
// the last bf rows random; enqueued back to back with one closing check and one commit batch
static int stage_lookup_grand_sums(Finish& f) {
    zk_ctx* ctx = f.ctx; zk_proof* pr = f.pr; const zk_pk* pk = f.pk; const size_t n = f.n; host::XorShiftRng& rng = pr->rng; host::Transcript& tr = pr->tr;
    if (pk->L) {
        // ONE batch inversion for all arguments of the proof: every (t + beta) and (f_a + beta) column is written into one buffer --
        // slot list below; an argument that reads the table of the one before it has no table slot of its own --, inverted by a
        // single call (a batch inversion is one field inversion per wave behind two passes of products: a hundred calls of
        // 2-3 M elements each were a hundred inversion latencies, 16 ms on the SuperCircuit shape), then every argument forms
        // g = sum_a 1 / (f_a + beta) - m / (t + beta) and its prefix sum.  When the buffer would exceed a quarter of the free device
        // memory the arguments are processed in several such batches.
        std::vector<size_t> slot0(pk->L), tslot(pk->L), nslots(pk->L);
        DevBuf g, closing_d;
        PK_ALLOC(ctx, closing_d, (size_t)pk->L * 32);
        std::vector<F4> blind((size_t)pk->L * pk->bf);
        for (size_t q = 0; q < blind.size(); ++q) blind[q] = rng.next_fr();            // argument by argument, row by row: the order they were always drawn in, on every rank
        std::vector<const void*> pptrs(pk->L);
        for (uint32_t l = 0; l < pk->L; ++l) {            // every phi exists on every rank (the ones of other ranks arrive below)
            PK_ALLOC(ctx, f.lk_phi[l], n * 32);
            pptrs[l] = f.lk_phi[l].p;
        }
        ZK_HIP(ctx, hipMemsetAsync(closing_d.p, 0, (size_t)pk->L * 32, ctx->stream));
        const size_t free_b = device_free_bytes();          // unknown counts as none: batches of four slots
        size_t max_slots = std::max<size_t>(4, (free_b + ctx->pool_bytes) / 4 / (n * 32));
        if (const char* e = getenv("ZK_LOOKUP_PHI_SLOTS")) { if (atol(e) > 0) max_slots = (size_t)atol(e); }      // test knob: several batches at small n
        const bool fused = lookup_fused();
        if (!fused) PK_ALLOC(ctx, g, n * 32);
        const std::vector<uint32_t>& ord = f.lk_order;          // the order the multiplicities stage settled who shares whose table in
        const size_t NA = ord.size();
        for (size_t j0 = 0; j0 < NA;) {
            // arguments act[j0 .. j1) share one inversion; an argument is never separated from the owner of its table
            size_t slots = 0;
            size_t j1 = j0;
            while (j1 < NA) {
                const uint32_t l1 = ord[j1];
                const size_t need = f.lk_f[l1].size() + (f.same_table[l1] && j1 > j0 ? 0 : 1);
                if (j1 > j0 && slots + need > max_slots && !f.same_table[l1]) break;
                slot0[l1] = slots;
                tslot[l1] = (f.same_table[l1] && j1 > j0) ? tslot[ord[j1 - 1]] : slots;
                nslots[l1] = need;
                slots += need;
                ++j1;
            }
            DevBuf inv;
            PK_ALLOC(ctx, inv, slots * n * 32);
            if (fused) {
                // the denominators are inverted out of place (beta added at the load: no copy of the compressed columns), then ONE launch
                // chain forms g and its running sum for every argument of the batch; both tables travel in one upload
                std::vector<const void*> asrc(slots);
                std::vector<LkSum> sums;
                for (size_t j = j0; j < j1; ++j) {
                    const uint32_t l = ord[j];
                    const size_t N = f.lk_f[l].size();
                    const bool own_t = tslot[l] == slot0[l];
                    if (own_t) asrc[tslot[l]] = f.lk_t[f.table_owner[l]].p;
                    for (size_t a = 0; a < N; ++a) asrc[slot0[l] + (own_t ? 1 : 0) + a] = f.lk_f[l][a].p;
                    sums.push_back(LkSum{f.lk_m[l].fr(), (const Fr*)inv.p + tslot[l] * n, (const Fr*)inv.p + (slot0[l] + (own_t ? 1 : 0)) * n, f.lk_phi[l].fr(), (uint64_t)N});
                }
                const size_t sums_at = (slots * sizeof(void*) + 15) & ~(size_t)15;
                std::vector<uint8_t> host(sums_at + sums.size() * sizeof(LkSum));
                memcpy(host.data(), asrc.data(), slots * sizeof(void*));
                memcpy(host.data() + sums_at, sums.data(), sums.size() * sizeof(LkSum));
                DevBuf dtab;
                PK_ALLOC(ctx, dtab, host.size());
                PK_TRY(zk_h2d(ctx, dtab.p, host.data(), host.size()));
                ZkProfScope prof(ctx, "lookup_phi_fused");
                PK_TRY(fr_batch_invert_from(ctx, (const Fr* const*)dtab.p, &f.lag.beta, f.k, (Fr*)inv.p, slots));
                PK_TRY(lookup_sums_enqueue(ctx, (const LkSum*)((const char*)dtab.p + sums_at), sums.size(), n));
            } else {
            {   // t + beta and every f_a + beta of the batch, into their slots: ONE kind of launch for all of them (fr_add_const_many; each used to be a program of its own)
                std::vector<const void*> asrc;
                std::vector<void*> adst;
                for (size_t j = j0; j < j1; ++j) {
                    const uint32_t l = ord[j];
                    const size_t N = f.lk_f[l].size();
                    const bool own_t = tslot[l] == slot0[l];
                    for (size_t a = own_t ? 0 : 1; a <= N; ++a) {
                        const size_t slot = a == 0 ? tslot[l] : slot0[l] + (own_t ? a : a - 1);
                        asrc.push_back(a == 0 ? f.lk_t[f.table_owner[l]].p : f.lk_f[l][a - 1].p);
                        adst.push_back((char*)inv.p + slot * n * 32);
                    }
                }
                PK_TRY(fr_add_const_many(ctx, asrc.data(), adst.data(), asrc.size(), &f.lag.beta, n));
            }
            PK_TRY(zk_fr_batch_invert(ctx, inv.p, slots * n));
            }
            for (size_t j = j0; j < j1; ++j) {
                const uint32_t l = ord[j];
                DevBuf& phi = f.lk_phi[l];
                const size_t N = f.lk_f[l].size();
                const bool own_t = tslot[l] == slot0[l];
                const char* inv_t = (const char*)inv.p + tslot[l] * n * 32;
                const char* inv_f = (const char*)inv.p + (slot0[l] + (own_t ? 1 : 0)) * n * 32;
                if (!fused) {
                    // g = sum_a inv_f_a - m * inv_t
                    PK_TRY(zk_field_vec_op(ctx, ZK_FIELD_FR, ZK_OP_MUL, f.lk_m[l].p, inv_t, g.p, n));
                    PK_TRY(zk_field_vec_op(ctx, ZK_FIELD_FR, ZK_OP_SUB, inv_f, g.p, g.p, n));
                    for (size_t a = 1; a < N; ++a) PK_TRY(zk_field_vec_op(ctx, ZK_FIELD_FR, ZK_OP_ADD, g.p, inv_f + a * n * 32, g.p, n));
                    PK_TRY(zk_fr_prefix_sum(ctx, g.p, phi.p, n));                       // phi[0] = 0, phi[i+1] = phi[i] + g[i]
                }
                ZK_HIP(ctx, hipMemcpyAsync((char*)closing_d.p + (size_t)l * 32, (char*)phi.p + (size_t)pk->u * 32, 32, hipMemcpyDeviceToDevice, ctx->stream));
                ZK_HIP(ctx, hipMemcpyAsync((char*)phi.p + (n - pk->bf) * 32, blind.data() + (size_t)l * pk->bf, (size_t)pk->bf * 32, hipMemcpyHostToDevice, ctx->stream));
                f.lk_f[l].clear();                                                    // f, t are not needed again (the quotient recomputes them on its cosets)
                if (j + 1 == NA || !f.same_table[ord[j + 1]]) f.lk_t[f.table_owner[l]].release();      // the table's last reader
            }
            j0 = j1;
        }
        std::vector<F4> closing(pk->L);
        PK_TRY(zk_d2h(ctx, closing.data(), closing_d.p, (size_t)pk->L * 32));
        for (uint32_t l = 0; l < pk->L; ++l)
            if (!host::fr_is_zero(closing[l])) return ctx->fail(ZK_ERR_INVALID_ARG, "lookup %u: grand sum does not close", l);
        f.trace.mark("  lookup: phi (all lookups)");
        std::vector<G1Affine> coms(pk->L);
        PK_TRY(sharded_commit(ctx, pr, f.srs, 1, pptrs.data(), pk->L, n, coms.data(), 3));      // running sums: mostly equal increments (runs.hip)
        for (const G1Affine& com : coms) tr.write_point(com);
        if (f.shard_args) PK_TRY(exchange_owned(f, f.lk_phi));
    }
    f.trace.mark("lookup phi");
    return ZK_OK;
}

// ---- vanishing argument: the "random" polynomial.  In the reference's own proof it is the CONSTANT 1: the commitment in
// [REF aggregator/data/batch-task.json: chunk_proofs[0]] is g[0] = (1, 2) and its evaluation is 1 (tests/test_reference_chunk_proof.py)
// -- Scroll's halo2 fork commits no blinding polynomial; upstream PSE halo2 draws n uniform coefficients.  The verifier accepts
// either (it only opens the commitment); ZK_VANISHING_ONE (default) does what the reference's prover did, ZK_VANISHING_UNIFORM
// what upstream does.
static int stage_vanishing_random(Finish& f) {
    zk_ctx* ctx = f.ctx; zk_proof* pr = f.pr; const size_t n = f.n; host::XorShiftRng& rng = pr->rng; host::Transcript& tr = pr->tr;
    const F4 one = host::fr_one();
    PK_ALLOC(ctx, f.random_coeff, n * 32);
    G1Affine com;
    if (pr->vanishing_random == ZK_VANISHING_ONE) {
        ZK_HIP(ctx, hipMemsetAsync(f.random_coeff.p, 0, n * 32, ctx->stream));
        ZK_HIP(ctx, hipMemcpyAsync(f.random_coeff.p, &one, 32, hipMemcpyHostToDevice, ctx->stream));
        PK_TRY(zk_d2h(ctx, &com, f.srs->g, sizeof com));                    // commit(1) = g[0]
    } else {
        // n uniform coefficients: ChaCha20 in counter mode on the device, keyed from the session RNG
        uint32_t key[8];
        for (uint32_t& w_ : key) w_ = rng.next_u32();
        PK_TRY(zk_fr_random(ctx, (const uint8_t*)key, 0, 0, f.random_coeff.p, n));
        PK_TRY(commit_coeff(ctx, f.srs, f.random_coeff.fr(), n, &com));
    }
    tr.write_point(com);
    f.trace.mark("random poly");
    return ZK_OK;
}

// ---- coefficient forms of everything the quotient reads and the proof opens
static int stage_coefficient_forms(Finish& f) {
    zk_ctx* ctx = f.ctx; zk_proof* pr = f.pr; const zk_pk* pk = f.pk; const size_t n = f.n;
    // one batch: several columns share a launch (ntt_run_many)
    std::vector<Fr*> dsts;
    std::vector<const Fr*> srcs;
    auto want = [&](const DevBuf& lagv, DevBuf* co) -> int {
        PK_ALLOC(ctx, *co, n * 32);
        dsts.push_back(co->fr());
        srcs.push_back(lagv.fr());
        return ZK_OK;
    };
    for (uint32_t i = 0; i < pk->A; ++i) if (!pr->adv_coeff[i].p) PK_TRY(want(pr->adv_lag[i], &pr->adv_coeff[i]));
    for (uint32_t c = 0; c < pk->C; ++c) PK_TRY(want(f.pz_lag[c], &f.pz_coeff[c]));
    for (uint32_t l = 0; l < pk->L; ++l) { PK_TRY(want(f.lk_m[l], &f.m_coeff[l])); PK_TRY(want(f.lk_phi[l], &f.phi_coeff[l])); }
    const Fr omega_inv = fr_inv_host(fr_root_of_unity(pk->k)), ninv = fr_inv_host(fr_from_u64(1ull << pk->k));
    PK_TRY(ntt_run_many(ctx, dsts.data(), srcs.data(), dsts.size(), pk->k, omega_inv, &ninv, nullptr, nullptr, false));
    f.trace.mark("coefficient forms");
    return ZK_OK;
}

// ---- the quotient.  Its constraints come in halo2's order: gates, permutation, lookups (folded with y).
// The extended domain is evaluated one coset at a time (g_r = zeta * omega_ext^r, r < 2^(ext_k-k)):
// every column the program reads is taken to that coset with a size-n transform of its
// coefficients, the program runs over n rows (rotations are index shifts inside a coset), and
// the result, divided by the vanishing polynomial -- a constant g_r^n - 1 on a coset of H --
// lands at stride 2^(ext_k-k) in the extended buffer.  Live memory is one n-row block per
// column instead of 2^(ext_k-k) of them: what lets 10^3-column circuits fit.
//
// Degree classes.  h = (sum_i y^(K-1-i) g_i) / (X^n - 1) is linear in the constraints, and a constraint of
// degree g only needs (g - 1) n evaluation points, i.e. the cosets r that are multiples of
// 2^(E - e), e = ceil(log2(g - 1)), E = ext_k - k: the extended domain of size 2^(k+e) is the union of
// exactly those cosets.  The constraints are therefore grouped by e; class e is evaluated on its 2^e
// cosets only, brought to coefficient form over its own (smaller) extended domain and added to h.  A
// column that occurs only in low-degree constraints needs 2^e coset transforms instead of 2^E, and the
// low-degree part of the program runs over 2^e n rows instead of 2^E n.  The polynomial h -- and with
// it every proof byte -- is the same as when everything is evaluated on the full extended domain
// (what halo2's evaluate_h does); how much is saved depends on the circuit's degree profile.
// The plan (which class evaluates what, each class's program) is a function of the key: made once, make_quotient_plan.
struct Quotient {
    std::shared_ptr<const QuotientPlan> plan;
    uint32_t E = 0, K = 0, nparts = 0;
    std::vector<DevBuf> h;                    // class e over its own extended domain, 2^(k+e) rows (the top class's is the quotient itself)
    const QPlanClass& cls(uint32_t e) const { return plan->cls[e]; }
    bool reads(uint32_t e, uint32_t ref) const { return std::find(cls(e).refs.begin(), cls(e).refs.end(), ref) != cls(e).refs.end(); }
};
// What lives as long as the pass over the cosets (and the exchange of its results) does.
// Sharded session: the unit of work is a (class, coset) pair -- class e on coset r costs the transforms of the columns
// that class reads plus its program -- and the pairs are dealt to the ranks longest first (every rank computes the same
// deal).  A rank keeps the finished, already divided n-row results of its pairs; afterwards they are all-gathered round
// by round (round t = every rank's t-th pair) and interleaved into the classes' buffers on every rank.
struct QPair { uint32_t e, r; double cost; };
struct CosetWork { uint32_t r = 0; Fr g; std::vector<uint32_t> active; std::unordered_map<uint32_t, const void*> part_of; };      // one coset: the classes this rank runs there, where each column's coset lies
struct CosetPass {
    bool cache_on = false;                    // the key's own columns are read from (and put into) the key's coset cache
    std::vector<DevBuf> part_buf;             // one coset buffer per column that is transformed here: allocated on first use
    DevBuf hpart;                             // one class program's values on one coset
    Env part;                                 // `lag` with the columns of the current coset
    std::vector<std::vector<QPair>> deal;     // per rank, in the order of evaluation (by coset, then class)
    PairOwners owners;
    std::vector<std::pair<uint32_t, Fr>> cosets;      // the cosets this rank works on, with g_r
    std::vector<DevBuf> mine;                 // this rank's finished pairs, in the order of its deal
    DevBuf rtmp, gbuf;                        // the exchange: one received block (host transport), world of them (device transports)
    HostStaging host;
};

// the plan, the powers of y, the remainders of the split constraints, one buffer per class
static int quotient_prepare(Finish& f, Quotient& q) {
    zk_ctx* ctx = f.ctx; const zk_pk* pk = f.pk; const size_t n = f.n;
    PK_TRY(quotient_plan(ctx, pk, &q.plan));
    q.E = f.ext_k - f.k; q.K = q.plan->K; q.nparts = 1u << q.E;
    const uint32_t E = q.E, K = q.K;
    q.h.resize(E + 1);
    f.rem_coeff.resize(q.plan->rems.size());
    f.lag.ypow.resize(K + 1);
    f.lag.ypow[0] = host::fr_one();
    for (uint32_t g_ = 1; g_ <= K; ++g_) f.lag.ypow[g_] = host::fr_mul(f.lag.ypow[g_ - 1], f.lag.y);
    if (!f.rem_coeff.empty()) {
        Env lag_r = f.lag;                     // the remainders read the Lagrange forms of Z, m and phi as well
        lag_r.perm_z = &f.pz_lag;
        lag_r.lk_m = &f.lk_m;
        lag_r.lk_phi = &f.lk_phi;
        std::vector<Fr*> dsts;
        for (size_t j = 0; j < f.rem_coeff.size(); ++j) {
            const QPlanRem& rp = q.plan->rems[j];
            PK_ALLOC(ctx, f.rem_coeff[j], n * 32);
            PK_TRY(run_program(ctx, lag_r, rp.prog, f.rem_coeff[j].p));                 // the parts on H, folded with y
            const F4 yp = host::fr_pow(f.lag.y, K - 1 - rp.last);                       // ... and weighted like the constraints they belong to
            PK_TRY(zk_fr_scale(ctx, f.rem_coeff[j].p, &yp, n));
            dsts.push_back(f.rem_coeff[j].fr());
        }
        const Fr omega_inv = fr_inv_host(fr_root_of_unity(pk->k)), ninv = fr_inv_host(fr_from_u64(1ull << pk->k));
        PK_TRY(ntt_run_many(ctx, dsts.data(), nullptr, dsts.size(), pk->k, omega_inv, &ninv, nullptr, nullptr, false));
        f.trace.mark("  quotient: remainders of the split constraints");
    }
    for (uint32_t e = 0; e <= E; ++e)
        if (q.cls(e).used || e == E) {
            PK_ALLOC(ctx, q.h[e], ((size_t)n << e) * 32);
            if (!q.cls(e).used) ZK_HIP(ctx, hipMemsetAsync(q.h[e].p, 0, ((size_t)n << e) * 32, ctx->stream));
        }
    return ZK_OK;
}

// decided once per key: do the key's own cosets fit the budget?
static void quotient_decide_key_cache(Finish& f, const Quotient& q) {
    zk_ctx* ctx = f.ctx; const zk_pk* pk = f.pk; const size_t n = f.n;
    const std::vector<uint32_t>& refs = q.plan->refs;
    size_t key_slots = 0;             // (column of the key, coset) pairs some class reads: what the cache will hold
    for (uint32_t ref : refs) {
        if (!key_column(ref)) continue;
        for (uint32_t r = 0; r < q.nparts; ++r) {
            bool read = false;
            for (uint32_t e = 0; e <= q.E && !read; ++e) read = q.cls(e).used && class_on_coset(q.E, e, r) && q.reads(e, ref);
            key_slots += read;
        }
    }
    // The budget is shared by every key alive on this context (a Prover keeps the chunk, compression and aggregation
    // keys resident together): the cap (ZK_PK_COSET_CACHE_GB, default 96) or a third of the device, whichever is
    // smaller, less what other keys already hold -- and it must fit what the device has free right now, counting
    // the session pool's parked blocks as free (pool_trim gives them back).
    const char* env = getenv("ZK_PK_COSET_CACHE_GB");
    double budget = (env ? atof(env) : 96.0) * (double)(1ull << 30);
    budget = std::min(budget, (double)ctx->prop.totalGlobalMem / 3.0) - (double)ctx->coset_cache_bytes;
    const size_t free_b = device_free_bytes();          // unknown counts as none
    const double row = (double)coset_row_bytes(f.records);
    const double need = (double)key_slots * n * row;
    const double session = (double)refs.size() * n * row + (double)((size_t)n << q.E) * 32.0 * 2.0;       // this proof's own coset buffers and h
    pk->part_cache_state = (need <= budget && need + session <= (double)free_b + (double)ctx->pool_bytes) ? 1 : 0;
    if (pk->part_cache_state) pk->part_cache.resize(q.nparts);
}

// the (class, coset) pairs dealt to the ranks, who owns which, and the cosets this rank works on
static int quotient_deal_pairs(Finish& f, const Quotient& q, CosetPass& cp) {
    zk_ctx* ctx = f.ctx; const zk_proof* pr = f.pr;
    const uint32_t E = q.E;
    cp.deal.resize(f.sharded ? pr->world : 1);
    cp.owners = PairOwners{E, pr->rank, f.sharded, std::vector<uint32_t>((size_t)(E + 1) << E, 0u)};
    if (f.sharded) {
        PK_ALLOC(ctx, cp.rtmp, f.n * 32);
        std::vector<QPair> all;
        for (uint32_t e = 0; e <= E; ++e)
            if (q.cls(e).used)
                for (uint32_t r = 0; r < q.nparts; r += 1u << (E - e)) all.push_back({e, r, (double)q.cls(e).refs.size() + (double)q.cls(e).prog.size() / 64.0});
        std::stable_sort(all.begin(), all.end(), [](const QPair& a, const QPair& b) { return a.cost > b.cost; });
        std::vector<double> load(pr->world, 0.0);
        for (const QPair& pp_ : all) {
            uint32_t best = 0;
            for (uint32_t q_ = 1; q_ < pr->world; ++q_) if (load[q_] < load[best]) best = q_;
            load[best] += pp_.cost;
            cp.deal[best].push_back(pp_);
            cp.owners.owner[cp.owners.at(pp_.e, pp_.r)] = best;
        }
        for (auto& d_ : cp.deal) std::sort(d_.begin(), d_.end(), [](const QPair& a, const QPair& b) { return a.r != b.r ? a.r < b.r : a.e < b.e; });
    }
    const Fr w_ext = fr_root_of_unity(f.ext_k);
    Fr g = fr_zeta();
    for (uint32_t r_ = 0; r_ < q.nparts; ++r_) {
        bool any = false;
        for (uint32_t e = 0; e <= E && !any; ++e) any = q.cls(e).used && cp.owners.mine(e, r_);
        if (any) cp.cosets.push_back({r_, g});
        g = g * w_ext;
    }
    return ZK_OK;
}

// the columns the active classes read on coset w.r: taken from where they already are (computed ahead, the key's cache) or
// transformed into the pass's coset buffers
static int quotient_transform(Finish& f, const Quotient& q, CosetPass& cp, CosetWork& w) {
    zk_ctx* ctx = f.ctx; zk_proof* pr = f.pr; const zk_pk* pk = f.pk; const size_t n = f.n;
    const std::vector<uint32_t>& refs = q.plan->refs;
    std::vector<DevBuf>& bufs = cp.part_buf;
    const bool cache_on = cp.cache_on;
    const uint32_t k = f.k;
    const size_t coset_bytes = n * coset_row_bytes(f.records);
    const Fr w_n = fr_root_of_unity(k);
    auto pre_coset = [&](uint32_t ref, uint32_t r) -> const void* {      // an advice column's coset r computed during the advice phases, if any
        if ((ref >> 24) != CT_ADVICE || r >= pr->adv_coset.size()) return nullptr;
        const uint32_t c_ = ref & 0xFFFFFFu;
        return c_ < pr->adv_coset[r].size() ? pr->adv_coset[r][c_].p : nullptr;
    };
    const uint32_t r_ = w.r;
    w.active.clear();
    for (uint32_t e = 0; e <= q.E; ++e)
        if (q.cls(e).used && cp.owners.mine(e, r_)) w.active.push_back(e);
    w.part_of.clear();
    std::vector<const void*> bat_src;                 // the coset transforms of this round go out as one batch
    std::vector<void*> bat_dst;
    std::vector<std::pair<uint32_t, DevBuf>> fresh_slots;      // cache slots being filled: published only once they hold their coset
    for (size_t i = 0; i < refs.size(); ++i) {
        bool needed = false;
        for (uint32_t e : w.active) needed |= q.reads(e, refs[i]);
        if (!needed) continue;
        if (const void* pre = pre_coset(refs[i], r_)) { w.part_of[refs[i]] = pre; continue; }
        if (!(cache_on && key_column(refs[i])) && !bufs[i].p) PK_ALLOC(ctx, bufs[i], coset_bytes);
        void* dst = bufs[i].p;
        DevBuf fresh;                             // a cache slot being filled: published only once it holds the coset
        const bool cached = cache_on && key_column(refs[i]);
        if (cached) {
            auto it = pk->part_cache[r_].find(refs[i]);
            if (it != pk->part_cache[r_].end()) { w.part_of[refs[i]] = it->second.p; continue; }   // computed by an earlier proof
            // a slot lives as long as the key, not the session's pool.  When the device has no room for it: give the
            // pool's parked blocks back and retry; if that fails too, freeze the cache (existing slots stay in use) and
            // compute this coset into a session buffer like any witness column's -- the proof goes on, uncached.
            const char* env_fail = getenv("ZK_PK_COSET_CACHE_FAIL_AFTER");        // test knob: the device "runs out" after this many slots
            const bool inject = env_fail && pk->part_cache_bytes / coset_bytes + fresh_slots.size() >= (size_t)atoll(env_fail);
            bool got = pk->part_cache_state == 1 && !inject && fresh.alloc_unpooled(coset_bytes);
            if (!got && pk->part_cache_state == 1) {
                (void)hipGetLastError();
                ctx->pool_trim();
                got = !inject && fresh.alloc_unpooled(coset_bytes);
                if (!got) { (void)hipGetLastError(); pk->part_cache_state = 2; }
            }
            if (got) dst = fresh.p;
            else {
                if (!bufs[i].p) PK_ALLOC(ctx, bufs[i], coset_bytes);
                dst = bufs[i].p;
            }
        }
        w.part_of[refs[i]] = dst;
        if (refs[i] == colref(CT_SPECIAL, SP_X)) PK_TRY(fr_powers_fmt(ctx, w_n, w.g, dst, n, f.records));   // X on the coset: g * omega^i
        else {
            const Fr* cf = (refs[i] >> 24) == CT_SPLIT_R ? ((refs[i] & 0xFFFFFFu) < f.rem_coeff.size() ? f.rem_coeff[refs[i] & 0xFFFFFFu].fr() : nullptr)
                                                         : coeff_of(pk, refs[i], pr->adv_coeff, pr->inst_coeff, f.pz_coeff, f.m_coeff, f.phi_coeff);
            if (!cf) return ctx->fail(ZK_ERR_INVALID_ARG, "prover: unresolved column reference 0x%08x", refs[i]);
            bat_src.push_back(cf);
            bat_dst.push_back(dst);
        }
        if (cached && fresh.p) fresh_slots.emplace_back(refs[i], std::move(fresh));
    }
    PK_TRY(coeff_to_coset_batch_fmt(ctx, bat_src.data(), k, w.g, bat_dst.data(), bat_src.size(), f.records));
    for (auto& fs : fresh_slots) {
        pk->part_cache_bytes += coset_bytes;
        ctx->coset_cache_bytes += coset_bytes;
        pk->part_cache[r_][fs.first] = std::move(fs.second);
    }
    return ZK_OK;
}

// the programs of the classes active on coset w.r, divided by the vanishing polynomial, into the classes' buffers
static int quotient_programs(Finish& f, Quotient& q, CosetPass& cp, CosetWork& w) {
    zk_ctx* ctx = f.ctx; const size_t n = f.n;
    const uint32_t k = f.k, E = q.E, K = q.K;
    const bool sharded = f.sharded;
    const Fr one_fr = Fr::one();
    DevBuf& hpart = cp.hpart;
    Env& part = cp.part;
    std::vector<DevBuf>& mine = cp.mine;
    const uint32_t r_ = w.r;
    part.part = &w.part_of;
    Fr gn = w.g;
    for (uint32_t i = 0; i < k; ++i) gn = sqr(gn);
    const Fr vinv = fr_inv_host(gn - Fr::one()), inv32 = fr_inv_host(fr_from_u64(32));
    for (uint32_t e : w.active) {
        ctx->prof_tag = "quotient_coset";
        const int rc_q = run_program(ctx, part, q.cls(e).prog, hpart.p, f.records);
        ctx->prof_tag = nullptr;
        PK_TRY(rc_q);
        // class e lags (K - 1 - last) positions behind the end of the constraint list: its sum still takes y^(K-1-last)
        const F4 yp = host::fr_pow(f.lag.y, K - 1 - q.cls(e).last);
        Fr scale;
        memcpy((void*)&scale, yp.l, 32);
        scale = scale * vinv;
        if (f.records) scale = scale * inv32;          // a class program over records leaves 32 x its values
        if (sharded) {                 // peers receive the finished values: keep them until the exchange
            PK_TRY(zk_fr_scale(ctx, hpart.p, &scale, n));
            DevBuf keep;
            PK_ALLOC(ctx, keep, n * 32);
            ZK_HIP(ctx, hipMemcpyAsync(keep.p, hpart.p, n * 32, hipMemcpyDeviceToDevice, ctx->stream));
            mine.push_back(std::move(keep));
        }
        PK_TRY(zk_fr_scatter_scaled(ctx, hpart.p, n, sharded ? &one_fr : &scale, q.h[e].p, (size_t)1 << e, r_ >> (E - e)));
    }
    return ZK_OK;
}

// sharded session: the finished pairs of every rank into the classes' buffers of every rank
static int quotient_exchange_pairs(Finish& f, Quotient& q, CosetPass& cp) {
    zk_ctx* ctx = f.ctx; const zk_proof* pr = f.pr; const size_t n = f.n;
    const Fr one_fr = Fr::one();
    if (cp.mine.size() != cp.deal[pr->rank].size()) return ctx->fail(ZK_ERR_INVALID_ARG, "sharded session: %zu pairs evaluated, %zu dealt", cp.mine.size(), cp.deal[pr->rank].size());
    size_t rounds = 0;
    for (const auto& d_ : cp.deal) rounds = std::max(rounds, d_.size());
    for (size_t t = 0; t < rounds; ++t) {
        const void* mine_t = t < cp.mine.size() ? cp.mine[t].p : cp.hpart.p;           // a rank without a t-th pair sends filler nobody reads
        // in-library RCCL: the finished pairs go device to device, stream-ordered (no host copy, no synchronisation); a caller-supplied
        // device all-gather (zk_proof_set_device_gather): device to device as well, the callback completes on return; else through the host
        if ((pr->use_comm || pr->gather_dev) && !cp.gbuf.p) PK_ALLOC(ctx, cp.gbuf, (size_t)pr->world * n * 32);
        bool on_device = false;
        PK_TRY(allgather_rows(ctx, pr, pr->use_comm, mine_t, t < cp.mine.size(), n * 32, cp.gbuf.p, cp.host, &on_device));
        for (uint32_t q_ = 0; q_ < pr->world; ++q_) {
            if (q_ == pr->rank || t >= cp.deal[q_].size()) continue;
            const QPair& pp_ = cp.deal[q_][t];
            const void* src = on_device ? (const void*)((const char*)cp.gbuf.p + (size_t)q_ * n * 32) : nullptr;
            if (!src) { PK_TRY(zk_h2d(ctx, cp.rtmp.p, cp.host.recv.data() + (size_t)q_ * n * 32, n * 32)); src = cp.rtmp.p; }
            PK_TRY(zk_fr_scatter_scaled(ctx, src, n, &one_fr, q.h[pp_.e].p, (size_t)1 << pp_.e, pp_.r >> (q.E - pp_.e)));
        }
    }
    return ZK_OK;
}

// every class back to coefficients over its own extended domain; the smaller ones are added into h
static int quotient_to_coeff(Finish& f, Quotient& q) {
    zk_ctx* ctx = f.ctx;
    const uint32_t E = q.E;
    DevBuf& h = q.h[E];
    for (uint32_t e = 0; e < E; ++e) {
        if (!q.cls(e).used) continue;
        PK_TRY(zk_extended_to_coeff(ctx, q.h[e].p, f.k + e));
    }
    PK_TRY(zk_extended_to_coeff(ctx, h.p, f.ext_k));
    for (uint32_t e = 0; e < E; ++e) {
        if (!q.cls(e).used) continue;
        PK_TRY(zk_field_vec_op(ctx, ZK_FIELD_FR, ZK_OP_ADD, h.p, q.h[e].p, h.p, f.n << e));
        q.h[e].release();
    }
    f.h = std::move(h);
    return ZK_OK;
}

// The key's coset cache outlives sessions: one that finds it in the other format (the knobs changed in between) gives the slots back
// and decides and fills it again like the key's first proof.
static int key_cache_format(Finish& f) {
    zk_ctx* ctx = f.ctx; const zk_pk* pk = f.pk;
    if (pk->part_cache_records == f.records) return ZK_OK;
    if (pk->part_cache_bytes || !pk->part_cache.empty()) {
        ZK_HIP(ctx, hipStreamSynchronize(ctx->stream));       // an earlier proof's programs may still be reading the slots
        pk->part_cache.clear();
        ctx->coset_cache_bytes -= std::min(ctx->coset_cache_bytes, pk->part_cache_bytes);
        pk->part_cache_bytes = 0;
    }
    pk->part_cache_state = -1;
    pk->part_cache_records = f.records;
    return ZK_OK;
}

static int stage_quotient(Finish& f) {
    zk_ctx* ctx = f.ctx;
    Quotient q;
    PK_TRY(quotient_prepare(f, q));
    {
        CosetPass cp;                         // its buffers go back to the pool before the classes are transformed back
        PK_TRY(key_cache_format(f));
        if (f.pk->part_cache_state < 0) quotient_decide_key_cache(f, q);
        cp.cache_on = f.pk->part_cache_state >= 1;
        cp.part_buf.resize(q.plan->refs.size());
        PK_ALLOC(ctx, cp.hpart, f.n * 32);
        if (f.late_cosets) ZK_HIP(ctx, hipStreamWaitEvent(ctx->stream, ctx->ev_aux, 0));          // the cosets computed beside the earlier stages are complete
        cp.part = f.lag;
        PK_TRY(quotient_deal_pairs(f, q, cp));
        CosetWork work;
        for (const auto& rg : cp.cosets) {
            work.r = rg.first; work.g = rg.second;
            PK_TRY(quotient_transform(f, q, cp, work));
            f.trace.mark("  quotient: cosets of the columns");
            PK_TRY(quotient_programs(f, q, cp, work));
            f.trace.mark("  quotient: program");
        }
        if (f.sharded) PK_TRY(quotient_exchange_pairs(f, q, cp));
    }
    PK_TRY(quotient_to_coeff(f, q));
    f.trace.mark("quotient eval + ifft");
    return ZK_OK;
}

static int stage_h_commits(Finish& f) {
    zk_ctx* ctx = f.ctx; const size_t n = f.n;
    const uint32_t pieces = f.pk->d - 1;
    std::vector<const void*> hptrs(pieces);
    for (uint32_t i = 0; i < pieces; ++i) hptrs[i] = f.h.fr() + (size_t)i * n;
    std::vector<G1Affine> coms(pieces);
    PK_TRY(sharded_commit(ctx, f.pr, f.srs, 0, hptrs.data(), pieces, n, coms.data()));
    for (const G1Affine& com : coms) f.pr->tr.write_point(com);
    f.trace.mark("h commits");
    return ZK_OK;
}

// ---- evaluations, written in halo2's order: advice queries, fixed queries, the random polynomial,
// the permutation's sigma polynomials, per permutation set Z(x), Z(wx) (and Z(w^last x) for all but
// the last set), per lookup phi(x), phi(wx), m(x)
static int stage_evaluations(Finish& f) {
    zk_ctx* ctx = f.ctx; zk_proof* pr = f.pr; const zk_pk* pk = f.pk; const size_t n = f.n;
    const int32_t rot_last = -(int32_t)(pk->bf + 1);
    std::vector<Open>& evals = f.evals;
    for (const Query& qy : pk->adv_q) evals.push_back({pr->adv_coeff[qy.idx].fr(), qy.rot, host::fr_zero()});
    f.e_fix = evals.size();
    for (const Query& qy : pk->fix_q) evals.push_back({pk->fixed_coeff[qy.idx].fr(), qy.rot, host::fr_zero()});
    f.e_random = evals.size();
    evals.push_back({f.random_coeff.fr(), 0, host::fr_zero()});
    f.e_sigma = evals.size();
    for (uint32_t j = 0; j < pk->P; ++j) evals.push_back({pk->sigma_coeff[j].fr(), 0, host::fr_zero()});
    for (uint32_t c = 0; c < pk->C; ++c) {
        f.e_pz[c] = evals.size();
        for (int32_t rot : {0, 1}) evals.push_back({f.pz_coeff[c].fr(), rot, host::fr_zero()});
        if (c + 1 < pk->C) evals.push_back({f.pz_coeff[c].fr(), rot_last, host::fr_zero()});
    }
    f.e_lk = evals.size();
    for (uint32_t l = 0; l < pk->L; ++l) {
        for (int32_t rot : {0, 1}) evals.push_back({f.phi_coeff[l].fr(), rot, host::fr_zero()});
        evals.push_back({f.m_coeff[l].fr(), 0, host::fr_zero()});
    }
    // every (polynomial, point) pair in one pass: one table per distinct point, one Horner launch, one download
    std::vector<int32_t> distinct;
    std::vector<F4> points;
    std::vector<uint32_t> pidx(evals.size());
    std::vector<const void*> ptrs(evals.size());
    for (size_t i = 0; i < evals.size(); ++i) {
        const int32_t nr = f.norm_rot(evals[i].rot);
        size_t at = std::find(distinct.begin(), distinct.end(), nr) - distinct.begin();
        if (at == distinct.size()) { distinct.push_back(nr); points.push_back(f.rotate(evals[i].rot)); }
        pidx[i] = (uint32_t)at;
        ptrs[i] = evals[i].poly;
    }
    std::vector<F4> vals(evals.size());
    if (f.sharded) {
        // sharded session: pair i is evaluated by rank i mod world; the 32-byte values are all-gathered (every rank holds every
        // coefficient form, so which rank evaluates what is free to choose)
        std::vector<const void*> my_ptrs;
        std::vector<uint32_t> my_pidx;
        for (size_t i = pr->rank; i < evals.size(); i += pr->world) { my_ptrs.push_back(ptrs[i]); my_pidx.push_back(pidx[i]); }
        std::vector<F4> local(share_size(pr, evals.size()), host::fr_zero());
        if (!my_ptrs.empty()) PK_TRY(zk_poly_eval_pairs(ctx, my_ptrs.data(), my_pidx.data(), my_ptrs.size(), points.data(), points.size(), n, local.data()));
        PK_TRY(share_gather(ctx, pr, local.data(), evals.size(), sizeof(F4), vals.data()));
    } else
        PK_TRY(zk_poly_eval_pairs(ctx, ptrs.data(), pidx.data(), evals.size(), points.data(), points.size(), n, vals.data()));
    for (size_t i = 0; i < evals.size(); ++i) evals[i].eval = vals[i];
    for (const Open& o : evals) pr->tr.write_scalar(o.eval);
    f.trace.mark("evaluations");
    return ZK_OK;
}

// h(X) = sum_i x^(n i) h_i(X): opened at x, the verifier derives its expected value itself
static int stage_h_recombination(Finish& f) {
    zk_ctx* ctx = f.ctx; const size_t n = f.n;
    PK_ALLOC(ctx, f.hcomb, n * 32);
    F4 xn = f.x;
    for (uint32_t i = 0; i < f.k; ++i) xn = host::fr_mul(xn, xn);
    std::vector<const void*> pieces(f.pk->d - 1);
    for (size_t i = 0; i < pieces.size(); ++i) pieces[i] = f.h.fr() + i * n;
    PK_TRY(lincomb(ctx, f.k, pieces, xn, f.hcomb.p));
    PK_TRY(zk_poly_eval(ctx, f.hcomb.fr(), n, &f.x, &f.h_eval));
    f.trace.mark("h recombination");
    return ZK_OK;
}

// ---- the multi-open's queries in halo2's order (plonk::prover::create_proof): advice, permutation
// products (x and wx per set, then w^last x for all but the last set in REVERSE set order), lookups,
// fixed, permutation sigma, then h and the random polynomial
static void stage_opening_queries(Finish& f) {
    const zk_pk* pk = f.pk;
    const std::vector<Open>& evals = f.evals;
    std::vector<Open>& queries = f.queries;
    const size_t e_fix = f.e_fix, e_random = f.e_random, e_sigma = f.e_sigma, e_lk = f.e_lk;
    for (size_t i = 0; i < e_fix; ++i) queries.push_back(evals[i]);
    for (uint32_t c = 0; c < pk->C; ++c) { queries.push_back(evals[f.e_pz[c]]); queries.push_back(evals[f.e_pz[c] + 1]); }
    for (uint32_t c = pk->C > 1 ? pk->C - 1 : 0; c-- > 0;) queries.push_back(evals[f.e_pz[c] + 2]);
    for (size_t i = e_lk; i < evals.size(); ++i) queries.push_back(evals[i]);
    for (size_t i = e_fix; i < e_random; ++i) queries.push_back(evals[i]);
    for (size_t i = e_sigma; i < e_sigma + pk->P; ++i) queries.push_back(evals[i]);
    queries.push_back({f.hcomb.fr(), 0, f.h_eval});
    queries.push_back(evals[e_random]);
    for (Open& o : queries) o.rot = f.norm_rot(o.rot);
}

// Division of N_i (degree < n, vanishing on S; coefficients in `num`) by Z_S(X) = prod (X - z), in place.  Few points: one
// synthetic division per point.  Many (a column opened at 14 rotations: 14 dependent scans, 1.7 ms of the Keccak-shape proof
// at k = 18): Q_i = N_i / Z_S is fixed by its values on a coset g H of the domain -- transform, divide point by point by
// Z_S(g w^j) (one batch inversion), transform back: the cost no longer depends on |S|.
struct CosetDivision { DevBuf x, ginv, den; };      // g w^j and g^-i (made once per proof, by the first set that needs them), Z_S(g w^j)
static int shplonk_divide_by_zs(Finish& f, CosetDivision& cd, const std::vector<F4>& zs, DevBuf& num, DevBuf& tmp) {
    zk_ctx* ctx = f.ctx; const size_t n = f.n; const uint32_t k = f.k;
    const F4 coset_g = host::fr_from_u64(7), one = host::fr_one();
    bool by_coset = zs.size() >= 4 && n >= 4 * zs.size();
    if (by_coset) {
        // no point of S may lie on the coset (z = x w^rot for a random x: z^n = g^n has probability n / r)
        F4 gn = coset_g;
        for (uint32_t i = 0; i < k; ++i) gn = host::fr_mul(gn, gn);
        for (const F4& z : zs) { F4 zn = z; for (uint32_t i = 0; i < k; ++i) zn = host::fr_mul(zn, zn); if (host::fr_eq(zn, gn)) by_coset = false; }
    }
    if (!by_coset) {
        size_t len = n;
        for (const F4& z : zs) {
            PK_TRY(zk_kate_division(ctx, num.p, len, &z, tmp.p));
            --len;
            PK_TRY(zk_d2d(ctx, num.p, tmp.p, len * 32));
            ZK_HIP(ctx, hipMemsetAsync((char*)num.p + len * 32, 0, (n - len) * 32, ctx->stream));
        }
        return ZK_OK;
    }
    if (!cd.x.p) {
        PK_ALLOC(ctx, cd.x, n * 32);
        PK_ALLOC(ctx, cd.ginv, n * 32);
        PK_ALLOC(ctx, cd.den, n * 32);
        const F4 ginv = host::fr_inv(coset_g);
        PK_TRY(zk_fr_powers(ctx, &f.w, &coset_g, cd.x.p, n));
        PK_TRY(zk_fr_powers(ctx, &ginv, &one, cd.ginv.p, n));
    }
    std::vector<uint32_t> words;
    std::vector<F4> cs;
    for (size_t t = 0; t < zs.size(); ++t) {
        words.insert(words.end(), {Q_PUSH_COL, 0u, 0u, Q_ADD_CONST, (uint32_t)t, 0u});
        if (t) words.insert(words.end(), {Q_MUL, 0u, 0u});
        cs.push_back(host::fr_sub(host::fr_zero(), zs[t]));
    }
    words.insert(words.end(), {Q_FOLD, (uint32_t)zs.size(), 0u});
    cs.push_back(host::fr_one());
    const void* xcol[1] = {cd.x.p};
    PK_TRY(zk_quotient_eval(ctx, words.data(), (uint32_t)(words.size() / 3), xcol, 1, cs.data(), (uint32_t)cs.size(), k, k, 0, cd.den.p));     // Z_S(g w^j)
    PK_TRY(zk_fr_batch_invert(ctx, cd.den.p, n));
    PK_TRY(zk_coeff_to_coset(ctx, num.p, k, &coset_g, tmp.p));                                                                            // N_i(g w^j)
    const uint32_t mulw[] = {Q_PUSH_COL, 0u, 0u, Q_PUSH_COL, 1u, 0u, Q_MUL, 0u, 0u, Q_FOLD, 0u, 0u};
    const void* c2[2] = {tmp.p, cd.den.p};
    PK_TRY(zk_quotient_eval(ctx, mulw, 4, c2, 2, &one, 1, k, k, 0, num.p));                                                                // Q_i(g w^j)
    PK_TRY(zk_ntt(ctx, num.p, k, 1));                                                                                                    // q_i g^i
    const void* c3[2] = {num.p, cd.ginv.p};
    PK_TRY(zk_quotient_eval(ctx, mulw, 4, c3, 2, &one, 1, k, k, 0, tmp.p));
    return zk_d2d(ctx, num.p, tmp.p, n * 32);
}

// ---- SHPLONK / BDFG21 (poly::kzg::multiopen::shplonk::ProverSHPLONK::create_proof): what
// the reference's call sites instantiate.  Two commitments whatever the number of polynomials and points.
static int multiopen_shplonk(Finish& f) {
    zk_ctx* ctx = f.ctx; const size_t n = f.n; const uint32_t k = f.k; host::Transcript& tr = f.pr->tr;
    DevBuf batch, wit;
    PK_ALLOC(ctx, batch, n * 32);
    PK_ALLOC(ctx, wit, n * 32);
    const F4 y = tr.squeeze();
    std::vector<PolyQ> polys;
    std::vector<RotSet> sets;
    std::vector<int32_t> super;                  // every point that is opened somewhere
    shplonk_intermediate_sets(f.queries, polys, sets, super);
    const F4 v = tr.squeeze();
    std::vector<DevBuf> qfull(sets.size()), hset(sets.size());
    CosetDivision coset_div;
    std::vector<std::vector<F4>> Rset(sets.size());       // R_i(X) = sum_j y^j r_ij(X)
    DevBuf tmp;
    PK_ALLOC(ctx, tmp, n * 32);
    for (size_t si = 0; si < sets.size(); ++si) {
        const RotSet& st = sets[si];
        std::vector<F4> zs;
        for (int32_t r_ : st.rots) zs.push_back(f.point_of(r_));
        // N_i(X) = sum_j y^j (P_ij(X) - r_ij(X)):  Qfull_i = sum_j y^j P_ij on the device, R_i on the host
        std::vector<const void*> members;
        const std::vector<std::vector<F4>> basis = lagrange_basis(zs);
        std::vector<F4> R(st.rots.size(), host::fr_zero());
        F4 ypow = host::fr_one();
        for (size_t pi : st.members) {
            members.push_back(polys[pi].poly);
            std::vector<F4> ys(st.rots.size());
            for (size_t a = 0; a < st.rots.size(); ++a) {
                const size_t where = std::find(polys[pi].rots.begin(), polys[pi].rots.end(), st.rots[a]) - polys[pi].rots.begin();
                ys[a] = polys[pi].evals[where];
            }
            const std::vector<F4> rj = interpolate(basis, ys);
            for (size_t t = 0; t < R.size(); ++t) R[t] = host::fr_add(R[t], host::fr_mul(ypow, rj[t]));
            ypow = host::fr_mul(ypow, y);
        }
        Rset[si] = R;
        PK_ALLOC(ctx, qfull[si], n * 32);
        PK_ALLOC(ctx, hset[si], n * 32);
        f.trace.mark("  shplonk: interpolation (host)");
        PK_TRY(lincomb(ctx, k, members, y, qfull[si].p));
        f.trace.mark("  shplonk: set combination");
        // Q_i = N_i / prod (X - z): subtract R_i from the low coefficients, divide point by point
        PK_TRY(zk_d2d(ctx, hset[si].p, qfull[si].p, n * 32));
        std::vector<F4> low(R.size());
        PK_TRY(zk_d2h(ctx, low.data(), hset[si].p, R.size() * 32));
        for (size_t t = 0; t < R.size(); ++t) low[t] = host::fr_sub(low[t], R[t]);
        PK_TRY(zk_h2d(ctx, hset[si].p, low.data(), R.size() * 32));
        PK_TRY(shplonk_divide_by_zs(f, coset_div, zs, hset[si], tmp));
        f.trace.mark("  shplonk: set division");
    }
    // h = sum_i v^i Q_i; commit
    {
        std::vector<const void*> qs;
        for (size_t si = 0; si < sets.size(); ++si) qs.push_back(hset[si].p);
        PK_TRY(lincomb(ctx, k, qs, v, batch.p));
        G1Affine com;
        PK_TRY(commit_coeff(ctx, f.srs, batch.fr(), n, &com));
        tr.write_point(com);
    }
    f.trace.mark("  shplonk: h");
    const F4 u = tr.squeeze();
    // L(X) = sum_i v^i Z_{T \ S_i}(u) (Qfull_i(X) - R_i(u)) - Z_T(u) h(X);  the proof's second point commits to
    // L(X) / (X - u), normalised by 1 / Z_{T \ S_0}(u) (the verifier scales the first set's term to one)
    std::vector<F4> coef(sets.size() + 1);
    F4 zT = host::fr_one(), constant = host::fr_zero(), vpow = host::fr_one(), z0_inv = host::fr_one();
    for (int32_t r_ : super) zT = host::fr_mul(zT, host::fr_sub(u, f.point_of(r_)));
    for (size_t si = 0; si < sets.size(); ++si) {
        F4 zdiff = host::fr_one();
        for (int32_t r_ : super) if (std::find(sets[si].rots.begin(), sets[si].rots.end(), r_) == sets[si].rots.end()) zdiff = host::fr_mul(zdiff, host::fr_sub(u, f.point_of(r_)));
        if (si == 0) z0_inv = host::fr_inv(zdiff);
        coef[si] = host::fr_mul(host::fr_mul(vpow, zdiff), z0_inv);
        constant = host::fr_add(constant, host::fr_mul(coef[si], eval_small(Rset[si], u)));
        vpow = host::fr_mul(vpow, v);
    }
    coef[sets.size()] = host::fr_mul(zT, z0_inv);
    {
        std::vector<uint32_t> words;
        std::vector<const void*> cols;
        for (size_t si = 0; si < sets.size(); ++si) {
            words.insert(words.end(), {Q_PUSH_COL, (uint32_t)cols.size(), 0u, Q_MUL_CONST, (uint32_t)si, 0u});
            if (si) words.insert(words.end(), {Q_ADD, 0u, 0u});
            cols.push_back(qfull[si].p);
        }
        words.insert(words.end(), {Q_PUSH_COL, (uint32_t)cols.size(), 0u, Q_MUL_CONST, (uint32_t)sets.size(), 0u, Q_SUB, 0u, 0u});
        cols.push_back(batch.p);
        coef.push_back(host::fr_one());
        words.insert(words.end(), {Q_FOLD, (uint32_t)sets.size() + 1, 0u});
        PK_TRY(zk_quotient_eval(ctx, words.data(), (uint32_t)(words.size() / 3), cols.data(), (uint32_t)cols.size(), coef.data(), (uint32_t)coef.size(), k, k, 0, tmp.p));
        F4 c0;
        PK_TRY(zk_d2h(ctx, &c0, tmp.p, 32));
        c0 = host::fr_sub(c0, constant);
        PK_TRY(zk_h2d(ctx, tmp.p, &c0, 32));
        PK_TRY(zk_kate_division(ctx, tmp.p, n, &u, wit.p));
        G1Affine com;
        PK_TRY(commit_coeff(ctx, f.srs, wit.fr(), n - 1, &com));
        tr.write_point(com);
    }
    PK_TRY(zk_ctx_sync(ctx));
    f.trace.mark("multiopen (shplonk)");
    return ZK_OK;
}

// ---- GWC multi-open (poly::kzg::multiopen::gwc::ProverGWC::create_proof): one witness per distinct
// point in order of first appearance, the point's polynomials combined with ascending powers of v
static int multiopen_gwc(Finish& f) {
    zk_ctx* ctx = f.ctx; const size_t n = f.n; host::Transcript& tr = f.pr->tr;
    const std::vector<Open>& queries = f.queries;
    DevBuf batch, wit;
    PK_ALLOC(ctx, batch, n * 32);
    PK_ALLOC(ctx, wit, n * 32);
    const F4 v = tr.squeeze();
    std::vector<int32_t> rots;
    for (const Open& o : queries) if (std::find(rots.begin(), rots.end(), o.rot) == rots.end()) rots.push_back(o.rot);
    for (int32_t rot : rots) {
        std::vector<const void*> members;
        for (const Open& o : queries) if (o.rot == rot) members.push_back(o.poly);
        PK_TRY(lincomb(ctx, f.k, members, v, batch.p));
        const F4 z = f.point_of(rot);
        PK_TRY(zk_kate_division(ctx, batch.p, n, &z, wit.p));
        G1Affine com;
        PK_TRY(commit_coeff(ctx, f.srs, wit.fr(), n - 1, &com));
        tr.write_point(com);
    }
    PK_TRY(zk_ctx_sync(ctx));
    f.trace.mark("multiopen");
    return ZK_OK;
}

// the finished transcript into the caller's buffer
static int write_proof_out(zk_ctx* ctx, const host::Transcript& tr, void* h_proof, size_t proof_cap, size_t* proof_len) {
    if (tr.err) return ctx->fail(ZK_ERR_INVALID_ARG, "transcript failed with status %d (external callback, or the identity point in a Poseidon / EVM transcript)", tr.err);
    *proof_len = tr.proof.size();
    if (tr.proof.size() > proof_cap) return ctx->fail(ZK_ERR_INVALID_ARG, "proof buffer too small: need %zu bytes", tr.proof.size());
    memcpy(h_proof, tr.proof.data(), tr.proof.size());
    return ZK_OK;
}

// The format of this session's cosets, as the knobs stand now.  Cosets computed ahead under other knobs (set between the advice phases
// and this call) are dropped: the quotient transforms those columns itself.
static int finish_coset_format(Finish& f) {
    zk_proof* pr = f.pr;
    f.records = quotient_records(f.k);
    if (pr->coset_fmt >= 0 && (pr->coset_fmt == 1) != f.records) {
        ZK_HIP(f.ctx, hipDeviceSynchronize());                // their transforms run on the auxiliary stream
        pr->adv_coset.clear();
        for (uint32_t& m_ : pr->pre_mask) m_ = 0;
    }
    pr->coset_fmt = f.records ? 1 : 0;
    return ZK_OK;
}

// Everything after the advice phases: lookups, permutation, quotient, evaluations, multi-open -- the stages above, with the
// transcript's challenges squeezed between them.  Consumes the session (it is freed whether or not the call succeeds).
int zk_proof_finish(zk_ctx* ctx, zk_proof* pr_raw, void* h_proof, size_t proof_cap, size_t* proof_len) {
    if (!ctx) return ZK_ERR_INVALID_ARG;
    PoolScope pool_scope(ctx);
    std::unique_ptr<zk_proof> pr(pr_raw);
    ZK_REQUIRE(ctx, pr && h_proof && proof_len, "null pointer");
    if (pr->phase != pr->pk->num_phases) return ctx->fail(ZK_ERR_INVALID_ARG, "only %u of %u advice phases were committed", pr->phase, pr->pk->num_phases);
    host::Transcript& tr = pr->tr;
    Finish f(ctx, pr.get());
    // Declared after `pr` and `f`, so destroyed first: the auxiliary stream is joined before any buffer of the session (the
    // stages' in `f`, the advice columns and their cosets in `pr`) goes back to the pool, on every return path.
    AuxJoin aux_join{ctx, &f.late_cosets};
    f.lag.theta = tr.squeeze();
    PK_TRY(finish_coset_format(f));
    PK_TRY(stage_late_advice_cosets(f));
    PK_TRY(stage_lookup_multiplicities(f));
    f.lag.beta = tr.squeeze();
    f.lag.gamma = tr.squeeze();
    PK_TRY(stage_permutation_products(f));
    PK_TRY(stage_lookup_grand_sums(f));
    PK_TRY(stage_vanishing_random(f));
    f.lag.y = tr.squeeze();
    PK_TRY(stage_coefficient_forms(f));
    PK_TRY(stage_quotient(f));
    PK_TRY(stage_h_commits(f));
    f.x = tr.squeeze();
    PK_TRY(stage_evaluations(f));
    PK_TRY(stage_h_recombination(f));
    stage_opening_queries(f);
    PK_TRY(pr->multiopen == ZK_MULTIOPEN_SHPLONK ? multiopen_shplonk(f) : multiopen_gwc(f));
    return write_proof_out(ctx, tr, h_proof, proof_cap, proof_len);
}

// ---- host-only transcript objects and hashes (no context, no device) -----------------------------
struct zk_transcript { host::Transcript tr; };
zk_transcript* zk_transcript_new(int kind) {
    if (kind != ZK_TRANSCRIPT_BLAKE2B && kind != ZK_TRANSCRIPT_POSEIDON && kind != ZK_TRANSCRIPT_EVM) return nullptr;
    zk_transcript* t = new (std::nothrow) zk_transcript();
    if (t) t->tr.reset(kind);
    return t;
}
void zk_transcript_free(zk_transcript* t) { delete t; }
static int transcript_status(zk_transcript* t) { const int e = t->tr.err; t->tr.err = 0; return e; }
int zk_transcript_common_point(zk_transcript* t, const void* affine64) {
    if (!t || !affine64) return ZK_ERR_INVALID_ARG;
    G1Affine p; memcpy((void*)&p, affine64, 64);
    t->tr.common_point(p);
    return transcript_status(t);
}
int zk_transcript_common_scalar(zk_transcript* t, const void* fr32) {
    if (!t || !fr32) return ZK_ERR_INVALID_ARG;
    F4 s_; memcpy(s_.l, fr32, 32);
    t->tr.common_scalar(s_);
    return transcript_status(t);
}
int zk_transcript_write_point(zk_transcript* t, const void* affine64) {
    if (!t || !affine64) return ZK_ERR_INVALID_ARG;
    G1Affine p; memcpy((void*)&p, affine64, 64);
    if (t->tr.kind != ZK_TRANSCRIPT_BLAKE2B && p.is_identity()) return ZK_ERR_INVALID_ARG;
    t->tr.write_point(p);
    return transcript_status(t);
}
int zk_transcript_write_scalar(zk_transcript* t, const void* fr32) {
    if (!t || !fr32) return ZK_ERR_INVALID_ARG;
    F4 s_; memcpy(s_.l, fr32, 32);
    t->tr.write_scalar(s_);
    return transcript_status(t);
}
int zk_transcript_squeeze(zk_transcript* t, void* fr32_out) {
    if (!t || !fr32_out) return ZK_ERR_INVALID_ARG;
    const F4 c = t->tr.squeeze();
    memcpy(fr32_out, c.l, 32);
    return transcript_status(t);
}
size_t zk_transcript_proof(const zk_transcript* t, const void** data) {
    if (!t) return 0;
    if (data) *data = t->tr.proof.data();
    return t->tr.proof.size();
}
int zk_host_keccak256(const void* data, size_t len, void* out32) {
    if ((!data && len) || !out32) return ZK_ERR_INVALID_ARG;
    host::keccak256((const uint8_t*)data, len, (uint8_t*)out32);
    return ZK_OK;
}
int zk_host_poseidon_permute(void* state5_fr32) {
    if (!state5_fr32) return ZK_ERR_INVALID_ARG;
    F4 st[host::PoseidonSpec::T];
    memcpy(st, state5_fr32, sizeof st);
    host::PoseidonSpec::get().permute(st);
    memcpy(state5_fr32, st, sizeof st);
    return ZK_OK;
}
int zk_host_poseidon_permute_width3(void* state3_fr32) {
    if (!state3_fr32) return ZK_ERR_INVALID_ARG;
    F4 st[host::PoseidonWidth3::T];
    memcpy(st, state3_fr32, sizeof st);
    host::PoseidonWidth3::get().permute(st);
    memcpy(state3_fr32, st, sizeof st);
    return ZK_OK;
}

// ---- dev::MockProver restated for the device ------------------------------------------------------------------
// halo2 `MockProver::run(k, &circuit, instances)` + `verify_par / verify_at_rows_par` [REF zkevm-circuits/src/test_util.rs:272],
// [REF prover/src/common/prover/mock.rs:18-19]: no commitments, no transcript -- every gate polynomial must vanish on the selected
// usable rows, every lookup input must occur among the usable rows of its table, every cell of a permutation column must equal
// the cell sigma maps it to.  What upstream derives from its region bookkeeping (CellNotAssigned, ConstraintPoisoned) has no
// counterpart here: the witness arrives as finished columns.
//   gates: one pass over all constraints folded with a random y finds out WHETHER any selected row fails (a satisfied witness
//     costs that one pass); only then one pass per constraint lists them (exact: no randomness in what is reported);
//   lookups: theta-compressed table and inputs (random theta), the hash join of the multiplicity computation with a probe that
//     reports instead of counting;
//   copies: sigma inverted with the same hash over the identity values delta^j w^i -- the key carries no cell mapping.
int zk_host_mock_challenges(uint32_t count, void* out_fr32) {
    if (count && !out_fr32) return ZK_ERR_INVALID_ARG;
    // halo2 dev.rs: hash = blake2b("Halo2-MockProver"); challenge_i = Fr::from_uniform_bytes(hash = blake2b(hash))   (golden G3: the third one)
    uint8_t h[64];
    host::Blake2b b;
    b.init(nullptr);
    b.update("Halo2-MockProver", 16);
    b.finalize(h);
    for (uint32_t i = 0; i < count; ++i) {
        host::Blake2b c;
        c.init(nullptr);
        c.update(h, 64);
        c.finalize(h);
        const F4 v = host::fr_from_uniform(h);
        memcpy((uint8_t*)out_fr32 + (size_t)i * 32, &v, 32);
    }
    return ZK_OK;
}

// y and theta of one call: fresh randomness, nothing a witness could have been fitted to
static void mock_randomise(Env& lag) {
    std::random_device rd;
    uint8_t b[128];
    for (size_t i = 0; i < sizeof b; i += 4) { const uint32_t v = rd(); memcpy(b + i, &v, 4); }
    lag.y = host::fr_from_uniform(b);
    lag.theta = host::fr_from_uniform(b + 64);
    lag.beta = lag.gamma = host::fr_zero();
}
// the checks themselves, over columns that are on the device already (lag: advice, instance, challenges, theta and y set)
static int mock_verify_core(zk_ctx* ctx, const zk_pk* pk, const Env& lag, const uint32_t* gate_rows, size_t num_gate_rows, const uint32_t* lookup_rows, size_t num_lookup_rows,
                            zk_mock_failure* out, size_t cap, size_t* count) {
    const size_t n = (size_t)1 << pk->k;
    // upstream panics on a row id outside the usable rows ("invalid gate row id")
    for (size_t i = 0; i < num_gate_rows; ++i) if (gate_rows[i] >= pk->u) return ctx->fail(ZK_ERR_INVALID_ARG, "mock verify: gate row id %u is not a usable row (%u of them)", gate_rows[i], pk->u);
    for (size_t i = 0; i < num_lookup_rows; ++i) if (lookup_rows[i] >= pk->u) return ctx->fail(ZK_ERR_INVALID_ARG, "mock verify: lookup row id %u is not a usable row (%u of them)", lookup_rows[i], pk->u);
    // failure records and counters on the device; selected rows
    const uint32_t cap32 = (uint32_t)cap;
    DevBuf fails, ctrs, rows_g, rows_l, vals;
    if (!fails.alloc((cap ? cap : 1) * sizeof(MockFail)) || !ctrs.alloc(64) || !vals.alloc(n * 32)) return ctx->fail(ZK_ERR_OOM, "mock verify: alloc failed");
    ZK_HIP(ctx, hipMemsetAsync(ctrs.p, 0, 64, ctx->stream));
    uint32_t* d_total = (uint32_t*)ctrs.p;            // every failure
    uint32_t* d_any = d_total + 1;                    // rows the folded gate pass flags
    const uint32_t* d_rows_g = nullptr;
    const uint32_t* d_rows_l = nullptr;
    const uint32_t cnt_g = gate_rows ? (uint32_t)num_gate_rows : pk->u, cnt_l = lookup_rows ? (uint32_t)num_lookup_rows : pk->u;
    if (gate_rows && num_gate_rows) {
        if (!rows_g.alloc(num_gate_rows * 4)) return ctx->fail(ZK_ERR_OOM, "mock verify: alloc failed");
        ZK_HIP(ctx, hipMemcpyAsync(rows_g.p, gate_rows, num_gate_rows * 4, hipMemcpyHostToDevice, ctx->stream));
        d_rows_g = (const uint32_t*)rows_g.p;
    }
    if (lookup_rows && num_lookup_rows) {
        if (!rows_l.alloc(num_lookup_rows * 4)) return ctx->fail(ZK_ERR_OOM, "mock verify: alloc failed");
        ZK_HIP(ctx, hipMemcpyAsync(rows_l.p, lookup_rows, num_lookup_rows * 4, hipMemcpyHostToDevice, ctx->stream));
        d_rows_l = (const uint32_t*)rows_l.p;
    }
    MockFail* d_fails = (MockFail*)fails.p;

    // ---- gates
    if (!pk->gates.empty() && cnt_g) {
        Prog all;
        for (const Prog& g : pk->gates) { all.insert(all.end(), g.begin(), g.end()); all.push_back({Q_FOLD, C_Y, 0}); }       // in order: an intermediate is parked before it is read
        PK_TRY(run_program(ctx, lag, all, vals.p));
        PK_TRY(mock_nonzero_enqueue(ctx, vals.fr(), d_rows_g, cnt_g, 0, 0, 0, d_fails, 0, d_any));
        uint32_t any = 0;
        PK_TRY(zk_d2h(ctx, &any, d_any, 4));
        if (any) {
            // one pass per constraint; a constraint that reads intermediates other constraints parked computes them itself
            // (TmpSplit re-materialises their definitions).  A key that REUSES a slot across constraints (a later TEE_TMP of a
            // slot an earlier constraint's intermediate still depends on) cannot be re-materialised that way -- the latest
            // definition would be expanded: for such keys constraint i is evaluated by running constraints 0 .. i in order, every
            // value but the last folded away (acc = acc * 0 + value), exactly the sequence the folded pass above saw.
            const bool reuse = tmp_slots_conflict(pk->gates);
            TmpSplit tmps(1);
            for (uint32_t i = 0; i < pk->gates.size(); ++i) {
                for (auto& h : tmps.have) std::fill(h.begin(), h.end(), 0u);
                Prog one;
                if (reuse) {
                    for (uint32_t j = 0; j <= i; ++j) { one.insert(one.end(), pk->gates[j].begin(), pk->gates[j].end()); one.push_back({Q_FOLD, C_ZERO, 0}); }
                    PK_TRY(run_program(ctx, lag, one, vals.p));
                    PK_TRY(mock_nonzero_enqueue(ctx, vals.fr(), d_rows_g, cnt_g, ZK_MOCK_GATE, i, 0, d_fails, cap32, d_total));
                    continue;
                }
                tmps.append(pk->gates[i], 0, one);
                one.push_back({Q_FOLD, C_ONE, 0});
                PK_TRY(run_program(ctx, lag, one, vals.p));
                PK_TRY(mock_nonzero_enqueue(ctx, vals.fr(), d_rows_g, cnt_g, ZK_MOCK_GATE, i, 0, d_fails, cap32, d_total));
            }
            if (tmps.conflict) return ctx->fail(ZK_ERR_INVALID_ARG, "mock verify: a gate reads an intermediate no earlier gate defined");
        }
    }
    // ---- lookups
    if (pk->L && cnt_l) {
        DevBuf tab, inp;
        if (!tab.alloc(n * 32) || !inp.alloc(n * 32)) return ctx->fail(ZK_ERR_OOM, "mock verify: alloc failed");
        for (uint32_t l = 0; l < pk->L; ++l) {
            const auto& lk = pk->lookups[l];
            PB pt;
            push_compressed(pt, lk.tables); pt.fold(C_ONE);
            PK_TRY(run_program(ctx, lag, pt.g, tab.p));
            const uint32_t* slots = nullptr;
            uint32_t mask = 0;
            PK_TRY(mock_hash_build(ctx, tab.fr(), pk->u, SC_TMP, &slots, &mask));
            for (size_t a = 0; a < lk.inputs.size(); ++a) {
                PB pf;
                push_compressed(pf, lk.inputs[a]); pf.fold(C_ONE);
                PK_TRY(run_program(ctx, lag, pf.g, inp.p));
                PK_TRY(mock_probe_enqueue(ctx, inp.fr(), tab.fr(), slots, mask, d_rows_l, cnt_l, ZK_MOCK_LOOKUP, l, (uint32_t)a, d_fails, cap32, d_total));
            }
        }
    }
    // ---- copy constraints (all rows: upstream walks the whole mapping, unusable rows map to themselves)
    if (pk->P) {
        const size_t cells = (size_t)pk->P << pk->k;
        if (cells > ((size_t)1 << 30)) return ctx->fail(ZK_ERR_UNSUPPORTED, "mock verify: %u permutation columns of 2^%u rows exceed the 2^30 cells one device hash holds", pk->P, pk->k);
        DevBuf ids, ptrs;
        if (!ids.alloc(cells * 32) || !ptrs.alloc((size_t)pk->P * 16)) return ctx->fail(ZK_ERR_OOM, "mock verify: alloc failed");
        const F4 omega_h = [&] { Fr w = fr_root_of_unity(pk->k); F4 o; memcpy(&o, &w, 32); return o; }();
        const F4 delta = host::fr_pow(host::fr_from_u64(7), 1ull << 28);
        F4 dj = host::fr_one();
        std::vector<const void*> hp(2 * (size_t)pk->P);
        for (uint32_t j = 0; j < pk->P; ++j) {
            PK_TRY(zk_fr_powers(ctx, &omega_h, &dj, (char*)ids.p + ((size_t)j << pk->k) * 32, n));                // delta^j w^i
            dj = host::fr_mul(dj, delta);
            hp[j] = pk->sigma_lag[j].p;
            hp[pk->P + j] = resolve_col(lag, colref(pk->perm_cols[j].first, pk->perm_cols[j].second));
            if (!hp[pk->P + j]) return ctx->fail(ZK_ERR_INVALID_ARG, "mock verify: unresolved permutation column %u", j);
        }
        ZK_HIP(ctx, hipMemcpyAsync(ptrs.p, hp.data(), hp.size() * 8, hipMemcpyHostToDevice, ctx->stream));
        const uint32_t* slots = nullptr;
        uint32_t mask = 0;
        PK_TRY(mock_hash_build(ctx, ids.fr(), cells, SC_TMP, &slots, &mask));
        PK_TRY(mock_perm_enqueue(ctx, (const Fr* const*)ptrs.p, (const Fr* const*)ptrs.p + pk->P, ids.fr(), slots, mask, pk->P, pk->k, ZK_MOCK_PERMUTATION, d_fails, cap32, d_total));
        ZK_HIP(ctx, hipStreamSynchronize(ctx->stream));           // hp is stack-owned
    }
    uint32_t total = 0;
    PK_TRY(zk_d2h(ctx, &total, d_total, 4));
    const size_t got = std::min<size_t>(total, cap);
    std::vector<MockFail> h(got);
    if (got) PK_TRY(zk_d2h(ctx, h.data(), d_fails, got * sizeof(MockFail)));
    // the device appends in whatever order its waves finish: sort (kind, index, sub, row) so that equal inputs give equal outputs
    // (when more failures exist than `cap` holds, WHICH ones were kept is still up to the device; *count says so)
    std::sort(h.begin(), h.end(), [](const MockFail& a, const MockFail& b) { return std::tie(a.kind, a.index, a.sub, a.row) < std::tie(b.kind, b.index, b.sub, b.row); });
    if (got) memcpy(out, h.data(), got * sizeof(MockFail));
    *count = total;
    return ZK_OK;
}


int zk_mock_verify(zk_ctx* ctx, const zk_pk* pk, const void* const* h_advice, const void* const* h_instance, const void* h_challenges,
                   const uint32_t* gate_rows, size_t num_gate_rows, const uint32_t* lookup_rows, size_t num_lookup_rows,
                   zk_mock_failure* out, size_t cap, size_t* count) {
    if (!ctx) return ZK_ERR_INVALID_ARG;
    ZK_REQUIRE(ctx, pk && count && (out || !cap) && (h_advice || !pk->A) && (h_instance || !pk->I), "null pointer");
    ZK_REQUIRE(ctx, (gate_rows || !num_gate_rows) && (lookup_rows || !num_lookup_rows), "row list without rows");
    ZK_REQUIRE(ctx, cap <= ((size_t)1 << 24), "at most 2^24 failure records");
    static_assert(sizeof(zk_mock_failure) == sizeof(MockFail), "failure records are copied as they are");
    *count = 0;
    const size_t n = (size_t)1 << pk->k;
    PoolScope pool(ctx);
    std::vector<DevBuf> adv(pk->A), inst(pk->I);
    // the uploads read the caller's columns asynchronously: whatever way this function is left, they are through before the device
    // buffers above go back to the pool (declared after them: destroyed first) and before the caller gets its columns back
    struct DrainOnExit { zk_ctx* c; ~DrainOnExit() { (void)hipStreamSynchronize(c->stream); } } drain{ctx};
    for (uint32_t c = 0; c < pk->A; ++c) {
        ZK_REQUIRE(ctx, h_advice[c], "null advice column");
        if (!adv[c].alloc(n * 32)) return ctx->fail(ZK_ERR_OOM, "mock verify: alloc failed");
        ZK_HIP(ctx, hipMemcpyAsync(adv[c].p, h_advice[c], n * 32, hipMemcpyHostToDevice, ctx->stream));
    }
    for (uint32_t c = 0; c < pk->I; ++c) {
        ZK_REQUIRE(ctx, h_instance[c], "null instance column");
        if (!inst[c].alloc(n * 32)) return ctx->fail(ZK_ERR_OOM, "mock verify: alloc failed");
        ZK_HIP(ctx, hipMemcpyAsync(inst[c].p, h_instance[c], n * 32, hipMemcpyHostToDevice, ctx->stream));
    }
    Env lag{};
    lag.pk = pk;
    lag.advice = &adv;
    lag.instance = &inst;
    lag.challenges.resize(pk->chal_phase.size());
    if (h_challenges) memcpy(lag.challenges.data(), h_challenges, lag.challenges.size() * 32);
    else PK_TRY(zk_host_mock_challenges((uint32_t)lag.challenges.size(), lag.challenges.data()));
    mock_randomise(lag);
    return mock_verify_core(ctx, pk, lag, gate_rows, num_gate_rows, lookup_rows, num_lookup_rows, out, cap, count);
}

// The same checks inside a proving session, after its last advice phase: the columns the session holds on the device, the
// challenges its transcript produced.  What a failed verify_proof leaves open -- WHICH constraint the witness breaks -- without
// a second upload.
int zk_proof_mock_verify(zk_ctx* ctx, zk_proof* pr, const uint32_t* gate_rows, size_t num_gate_rows, const uint32_t* lookup_rows, size_t num_lookup_rows,
                         zk_mock_failure* out, size_t cap, size_t* count) {
    if (!ctx) return ZK_ERR_INVALID_ARG;
    ZK_REQUIRE(ctx, pr && count && (out || !cap), "null pointer");
    ZK_REQUIRE(ctx, (gate_rows || !num_gate_rows) && (lookup_rows || !num_lookup_rows), "row list without rows");
    ZK_REQUIRE(ctx, cap <= ((size_t)1 << 24), "at most 2^24 failure records");
    const zk_pk* pk = pr->pk;
    *count = 0;
    if (pr->phase < pk->num_phases) return ctx->fail(ZK_ERR_INVALID_ARG, "mock verify: %u of the session's %u advice phases are committed", pr->phase, pk->num_phases);
    PoolScope pool(ctx);
    ZK_HIP(ctx, hipStreamSynchronize(ctx->stream));           // uploads and transforms of the last phase (copy / auxiliary streams are joined by the phase itself)
    if (pr->lag_partial) return ctx->fail(ZK_ERR_UNSUPPORTED, "mock verify: this rank of a sharded session holds some advice columns in coefficient form only (ZK_SHARD_COEFF=0 ships Lagrange values)");
    Env lag{};
    lag.pk = pk;
    lag.advice = &pr->adv_lag;
    lag.instance = &pr->inst_lag;
    lag.challenges = pr->challenges;
    mock_randomise(lag);
    return mock_verify_core(ctx, pk, lag, gate_rows, num_gate_rows, lookup_rows, num_lookup_rows, out, cap, count);
}

// One-shot create_proof: every advice column is known up front (no column depends on a challenge,
// or the caller derived them already); runs the phases back to back.
int zk_create_proof(zk_ctx* ctx, const zk_pk* pk, const void* const* h_advice, const void* const* h_instance, const uint8_t* seed16,
                    void* h_proof, size_t proof_cap, size_t* proof_len) {
    if (!ctx) return ZK_ERR_INVALID_ARG;
    ZK_REQUIRE(ctx, pk && seed16 && h_proof && proof_len && (h_advice || !pk->A) && (h_instance || !pk->I), "null pointer");
    zk_proof* pr = nullptr;
    PK_TRY(zk_proof_begin(ctx, pk, h_instance, seed16, &pr));
    for (uint32_t ph = 0; ph < pk->num_phases; ++ph) {
        std::vector<uint32_t> idx;
        std::vector<const void*> cols;
        for (uint32_t c = 0; c < pk->A; ++c) if (pk->adv_phase[c] == ph) { idx.push_back(c); cols.push_back(h_advice[c]); }
        const int rc = zk_proof_advice_phase(ctx, pr, idx.data(), cols.data(), (uint32_t)idx.size(), nullptr, nullptr);
        if (rc) { zk_proof_abort(ctx, pr); return rc; }
    }
    return zk_proof_finish(ctx, pr, h_proof, proof_cap, proof_len);
}

}  // extern "C"

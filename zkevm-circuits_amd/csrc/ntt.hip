// BN254 Fr NTT for gfx950: halo2_proofs::arithmetic::best_fft / poly::EvaluationDomain
// (external crate; reference call sites A1-A4).
//
// Definition (natural order in -> natural order out):  out[i] = sum_j a[j] * omega^(i*j).
//
// MI355X design: mixed-radix Cooley-Tukey in P <= 3 passes of <= 2^10 points each.  A pass stages
// a [digit x T] tile in LDS (T consecutive elements of the fastest-varying remaining index, so
// every global access is a T*32-byte contiguous run), runs all log2(n_p) radix-2 stages out of
// LDS, applies the inter-pass twiddle omega^(j''*i_p) on the way out (two-level table) and writes
// back.  Input index is read big-endian in the digits, output little-endian; the last pass writes
// to the digit-reversed position, so no separate transpose / bit-reversal kernel exists.
//
// Arithmetic: inside a pass elements live in LDS as nine 29-bit limbs (ff29.hip.hpp; one u32 plane
// per limb, so a wave's accesses are 4-byte strided and bank-conflict-free on contiguous runs).
// Butterflies use the carry-free 29-bit Montgomery product with twiddles held in R' = 2^261 form,
// so data stays in halo2curves' R = 2^256 form with no conversion; sums are kept lazily reduced
// and only the value written back to HBM is brought to the canonical representative.
#include <climits>
#include <type_traits>

#include "ctx.hpp"
#include "ff29.hip.hpp"

namespace zk {

constexpr int NTT_MAX_DIGIT = 10;
constexpr int NTT_TILE = 4096;         // elements staged per workgroup (9 x 4 B x 4096 = 144 KiB LDS)
constexpr int NTT_THREADS = 1024;
constexpr int NTT_LDS_BYTES_PER_ELT = 36;

struct Tw29;        // one butterfly twiddle split into 29-bit limbs (48 B), defined with the kernels

// One launch transforms up to NTT_BATCH columns over the same domain: blockIdx.y selects the column.  A 2^18 column
// is 64 tiles -- a quarter of the CUs --, and a prover transforms hundreds of columns per stage.
constexpr int NTT_BATCH = 16;
struct NttIo { const Fr* src[NTT_BATCH]; Fr* dst[NTT_BATCH]; };

struct NttPass {
    int log_np;     // digit size
    int log_m;      // stride of the digit (non-last)
    const Tw29* tw; // n_p/2 butterfly twiddles (omega^(n/n_p))^x, R' form, 29-bit limbs
    const Fr* out_tw = nullptr;   // non-last passes: inter-pass twiddle of every output element, in output order (R' form)
};

struct NttDomain {
    uint32_t log_n = 0;
    int npass = 0;
    NttPass pass[3];
    int h = 0;                // two-level split: omega^e = lo[e & (2^h-1)] * hi[e >> h]
    Fr* d_lo = nullptr;       // 2^h entries, R' form
    Fr* d_hi = nullptr;       // 2^(log_n-h) entries, R' form
    Fr* d_tw[3] = {nullptr, nullptr, nullptr};
    Tw29* d_tw29[3] = {nullptr, nullptr, nullptr};
    Fr* d_out_tw[2] = {nullptr, nullptr};
    Fr final_mul;             // (scale or 1) in R' form: last-pass output multiplier
    bool fin_folded = false;  // final_mul is already part of the last inter-pass twiddle table: the last pass only reduces
    ~NttDomain() {
        if (d_lo) (void)hipFree(d_lo);
        if (d_hi) (void)hipFree(d_hi);
        for (auto p : d_tw) if (p) (void)hipFree(p);
        for (auto p : d_tw29) if (p) (void)hipFree((void*)p);
        for (auto p : d_out_tw) if (p) (void)hipFree(p);
    }
};

// ------------------------------------------------------------------------------------- helpers
__device__ __forceinline__ uint32_t bitrev(uint32_t x, int bits) { return bits ? (__brev(x) >> (32 - bits)) : 0u; }

// R (2^256) Montgomery form -> R' (2^261) form: multiply by 32
__host__ __device__ __forceinline__ Fr to_rprime(Fr x) {
#pragma unroll
    for (int i = 0; i < 5; ++i) x = dbl(x);
    return x;
}

struct Lds29 {
    uint32_t* p;     // 9 planes of `stride` u32
    int stride;
    __device__ __forceinline__ Fr29 load(int idx) const {
        Fr29 r;
#pragma unroll
        for (int k = 0; k < 9; ++k) r.l[k] = p[k * stride + idx];
        return r;
    }
    __device__ __forceinline__ void store(int idx, const Fr29& v) const {
#pragma unroll
        for (int k = 0; k < 9; ++k) p[k * stride + idx] = v.l[k];
    }
};

// out[j] = base^j * mul   (table builder; one thread per entry, square-and-multiply).
// rprime != 0: store in R' = 2^261 Montgomery form; rprime == 2: as a coset record of `count` rows (ff29.hip.hpp).
__global__ void k_powers(Fr base, Fr mul, Fr* out, uint32_t count, int rprime) {
    uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= count) return;
    Fr r = mul, b = base;
    uint32_t e = j;
    while (e) {
        if (e & 1) r = r * b;
        b = sqr(b);
        e >>= 1;
    }
    if (rprime == 2) rec29_store<Fr29P>(out, count, j, unpack29<Fr29P>(to_rprime(r)));
    else stg(out + j, rprime ? to_rprime(r) : r);
}

__device__ __forceinline__ Fr two_level(const Fr* __restrict__ lo, const Fr* __restrict__ hi, int h, uint32_t e) {
    return ldg(lo + (e & ((1u << h) - 1))) * ldg(hi + (e >> h));
}
// both tables in R' form -> product in R' form, normalised, < 2p
__device__ __forceinline__ Fr29 two_level29(const Fr* __restrict__ lo, const Fr* __restrict__ hi, int h, uint32_t e) {
    return mul29(unpack29<Fr29P>(ldg(lo + (e & ((1u << h) - 1)))), unpack29<Fr29P>(ldg(hi + (e >> h))));
}

// out_tw[base + d*m + c] = omega^(((blk*T + c) * d) << tw_shift): the twiddle a non-last pass applies to
// each element it writes, tabulated once per domain in output order
__global__ void k_build_out_twiddles(Fr* __restrict__ out_tw, const Fr* __restrict__ lo, const Fr* __restrict__ hi, int h, int log_np, int log_m, int tw_shift, uint64_t n,
                                     Fr fin, int apply_fin) {
    const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n) return;
    const uint64_t m = 1ull << log_m;
    const uint32_t jpp = (uint32_t)(g & (m - 1)), d = (uint32_t)(g >> log_m) & ((1u << log_np) - 1);
    Fr29 v = two_level29(lo, hi, h, (jpp * d) << tw_shift);
    if (apply_fin) v = mul29(v, unpack29<Fr29P>(fin));      // the transform's output scale rides on the last inter-pass twiddle
    stg(out_tw + g, pack29_lt2p(v));
}

// ------------------------------------------------------------------------------- butterflies
// (u, x) -> (u + x w, u - x w); x w is reduced below 2p by the product, the sums stay lazy
__device__ __forceinline__ void bfly29(Fr29& u, Fr29& x, const Fr29& w) {
    const Fr29 v = mul29(x, w);
    Fr29 a0 = add29(u, v), a1 = sub29k<4>(u, v);
    normalize29(a0);
    normalize29(a1);
    u = a0;
    x = a1;
}
// butterfly twiddles are tabulated already split into 29-bit limbs (12 words = 48 B per entry, three
// 16-byte loads): no 8 x 32 -> 9 x 29 repacking in front of every product
struct Tw29 { uint4 q[3]; };
__device__ __forceinline__ Fr29 tw29(const Tw29* __restrict__ tw, uint32_t idx) {
    const uint4 a = tw[idx].q[0], b = tw[idx].q[1], c = tw[idx].q[2];
    return Fr29{{a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w, c.x}};
}
__global__ void k_split_twiddles(const Fr* __restrict__ in, Tw29* __restrict__ out, uint32_t count) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    const Fr29 v = unpack29<Fr29P>(ldg(in + i));
    out[i].q[0] = make_uint4(v.l[0], v.l[1], v.l[2], v.l[3]);
    out[i].q[1] = make_uint4(v.l[4], v.l[5], v.l[6], v.l[7]);
    out[i].q[2] = make_uint4(v.l[8], 0u, 0u, 0u);
}
// DIT stages s (and s+1 when R == 2) on the 2^R elements at digit offsets {0, h, 2h, 3h}, h = 2^s,
// j = digit mod h.  Radix-4 keeps both stages in registers: half the LDS round trips and barriers
// of two radix-2 stages, same four products.
// Inside a step the sums are not carry-propagated between the two stages.  Limb bounds with
// N = 2^29 (operands enter normalised, limbs < N; x w is normalised and < 1.4 p; the balanced
// limbs of 2p are < 2N):  stage 1 leaves u + v < 2N and u + 2p - v < 3N; stage 2 multiplies such
// an operand -- mul29 takes limbs up to 2^31.2 (9 N (X + N) < 2^64) -- and leaves sums < 5N < 2^32.
// One normalisation per element at the end of the step instead of one per butterfly output.
__device__ __forceinline__ void bfly29_lazy(Fr29& u, Fr29& x, const Fr29& w) {
    const Fr29 v = mul29(x, w);
    const Fr29 a0 = add29(u, v), a1 = sub29k<2>(u, v);
    u = a0;
    x = a1;
}
template <int R>
__device__ __forceinline__ void dit_step(Fr29 (&e)[4], const Tw29* __restrict__ tw, int log_np, int s, int j) {
    const Fr29 w0 = tw29(tw, (uint32_t)j << (log_np - 1 - s));
    bfly29_lazy(e[0], e[1], w0);
    if (R == 2) {
        bfly29_lazy(e[2], e[3], w0);
        bfly29_lazy(e[0], e[2], tw29(tw, (uint32_t)j << (log_np - 2 - s)));
        bfly29_lazy(e[1], e[3], tw29(tw, (uint32_t)(j + (1 << s)) << (log_np - 2 - s)));
        normalize29(e[2]);
        normalize29(e[3]);
    }
    normalize29(e[0]);
    normalize29(e[1]);
}
// (u, x) -> (u + x, u - x) for reduced operands (< 2p each, or sums of two such: x < 4p)
__device__ __forceinline__ void bfly29_one(Fr29& u, Fr29& x) {
    Fr29 a0 = add29(u, x), a1 = sub29k<4>(u, x);
    normalize29(a0);
    normalize29(a1);
    u = a0;
    x = a1;
}
// First step of a pass (s = 0): its operands come reduced from global memory and every twiddle of
// stage 0 is omega^0 = 1, as is the j = 0 twiddle of stage 1 -- three of the four products of a
// radix-4 step (the one of a radix-2 step) are products by one and are skipped.
template <int R>
__device__ __forceinline__ void dit_first_step(Fr29 (&e)[4], const Tw29* __restrict__ tw, int log_np) {
    bfly29_one(e[0], e[1]);
    if (R == 2) {
        bfly29_one(e[2], e[3]);
        bfly29_one(e[0], e[2]);
        bfly29(e[1], e[3], tw29(tw, 1u << (log_np - 2)));
    }
}

// ------------------------------------------------------------------ the steps of a pass, written once per pass kind
// A pass is a sequence of DIT steps with a workgroup barrier between them: radix 4, with one radix-2 step in front when the digit
// size is odd.  The body of a step is templated on what shapes its instruction stream: the radix, whether it is the first step
// (operands from global memory) or the last (results to global memory), and the optional operands.  The digit size and the step
// index are ordinary arguments.  Each pass kind has two kinds of kernel around the same body:
//   k_ntt_pass_f<LOG_NP, HAS_PRE> / k_ntt_last_f<LOG_NP>   recurse over the steps at compile time and hand the body constants:
//       straight-line code per step, every option decided (Opt OPT_NO / OPT_YES);
//   k_ntt_pass / k_ntt_last   loop over the steps at run time and select among the instantiations of the body; the options
//       are OPT_RUNTIME, a uniform branch on a kernel argument.  They serve every shape without an instance: single-pass sizes,
//       digits of 2^6 and less, domains without an inter-pass table, and everything under ZK_NTT_FIXED=0.
// All operands of a step (the 2^R elements, their coset shifts, the inter-pass twiddles of the outputs) are requested before the
// first of them is used: the first step waits for global memory once, not once per element and table.
// Same arithmetic in the same order whatever the instantiation: the kernels of a pass kind are bit-identical.
enum Opt { OPT_NO, OPT_YES, OPT_RUNTIME };
template <Opt O>
__device__ __forceinline__ bool opt_on(bool at_run_time) { return O == OPT_YES || (O == OPT_RUNTIME && at_run_time); }
template <int V> using Int = std::integral_constant<int, V>;
template <bool V> using Bool = std::integral_constant<bool, V>;

// ------------------------------------------------------------------------------ non-last pass
// Tile = [n_p digits][T columns], element (d, c) lives at base + d*m + c with
// base = hi_idx * (n_p*m) + blk*T.  DIT: the first step reads its operands straight from global
// memory (digit bit-reversed), the steps in between go through LDS, the last step multiplies by
// the inter-pass twiddle omega^((j'' * i_p) << tw_shift), j'' = blk*T + c, and writes to global
// memory: no staging copy on either side.
// LDS invariant: limbs 0..7 < 2^29 (normalised), value < 2^261.
// PRE: the coset shift a[i] * g^i is fused into the load (table `pre`, R' form).  TABLE: the inter-pass twiddle is one load from
// the per-domain table in output order (one product); without it, two entries of the two-level table and two products.
// A strided pass only exists for log_n >= 11, so its digit is 2^5 at least and no step is the first and the last at once.
template <int R, bool FIRST, bool LAST, Opt PRE, Opt TABLE>
__device__ __forceinline__ void ntt_pass_step(const Lds29& L, const Fr* __restrict__ src, Fr* __restrict__ dst, const Tw29* __restrict__ tw, const Fr* __restrict__ pre,
                                              const Fr* __restrict__ out_tw, const Fr* __restrict__ lo, const Fr* __restrict__ hi, const int h, const int tw_shift,
                                              const int log_np, const int s, const int log_t, const uint64_t m, const uint64_t base, const uint32_t blk) {
    static_assert(!(FIRST && LAST) && (R == 2 || FIRST), "a strided pass has two steps at least, and only its first can be radix 2");
    constexpr int NE = 1 << R;
    const int hgt = 1 << s, T = 1 << log_t, items = (1 << (log_np + log_t)) >> R;
    const bool has_pre = opt_on<PRE>(pre != nullptr), has_table = opt_on<TABLE>(out_tw != nullptr);
    for (int it = threadIdx.x; it < items; it += blockDim.x) {
        const int c = it & (T - 1), b = it >> log_t;      // c fastest: T-element contiguous runs in global memory
        const int j = b & (hgt - 1);
        const int lo_d = ((b >> s) << (s + R)) | j;
        Fr otw[NE];
        if (LAST && has_table) {
#pragma unroll
            for (int k = 0; k < NE; ++k) otw[k] = ldg(out_tw + base + (uint64_t)(lo_d + k * hgt) * m + c);
        }
        Fr29 e[4];
        if (FIRST) {
            Fr raw[NE], praw[NE];
            uint64_t gi[NE];
#pragma unroll
            for (int k = 0; k < NE; ++k) {
                gi[k] = base + (uint64_t)bitrev(lo_d + k * hgt, log_np) * m + c;
                raw[k] = ldg(src + gi[k]);
                if (PRE == OPT_YES) praw[k] = ldg(pre + gi[k]);
            }
#pragma unroll
            for (int k = 0; k < NE; ++k) {
                e[k] = unpack29<Fr29P>(raw[k]);
                if (has_pre) e[k] = mul29(e[k], unpack29<Fr29P>(PRE == OPT_YES ? praw[k] : ldg(pre + gi[k])));      // decided at run time: loaded behind the branch
            }
            dit_first_step<R>(e, tw, log_np);
        } else {
#pragma unroll
            for (int k = 0; k < NE; ++k) e[k] = L.load(((lo_d + k * hgt) << log_t) | c);
            dit_step<R>(e, tw, log_np, s, j);
        }
#pragma unroll
        for (int k = 0; k < NE; ++k) {
            const int dl = lo_d + k * hgt;
            if (LAST) {
                const Fr29 w = has_table ? unpack29<Fr29P>(otw[k]) : two_level29(lo, hi, h, ((((uint32_t)blk << log_t) + c) * (uint32_t)dl) << tw_shift);
                stg(dst + base + (uint64_t)dl * m + c, pack29_raw(mul29(e[k], w)));      // an intermediate (the next pass reads it): any representative below 2p will do, no conditional subtraction
            } else {
                L.store((dl << log_t) | c, e[k]);
            }
        }
    }
}

// One-dimensional grid over (tile, column).  The per-element tables (inter-pass twiddles, coset shifts: 32 B per element of the
// TILE, the same for every column) are read by every column's workgroup of a tile: those workgroups are numbered so that they
// are consecutive workgroups of ONE XCD (workgroups go to the eight XCDs round-robin, each XCD has its own L2) -- the table
// lines are fetched from HBM once per tile instead of once per (tile, column).  One more level (log_grp > 0): a tile of T < 4
// columns reads and writes runs shorter than a 128-byte line, and the 2^log_grp = 4 / T tiles that share those lines are consecutive
// workgroups of ONE XCD as well (same L2: the line is fetched once and its parts are written back together), ahead of the columns
// of the launch.
struct PassTile { uint32_t col, blk; uint64_t base; };
__device__ __forceinline__ PassTile pass_tile(int log_np, int log_t, int log_m, uint32_t ncols, int xcd_cols, int log_grp) {
    uint32_t tile_id, col;
    if (xcd_cols) {
        const uint32_t slot = blockIdx.x >> 3, sub = slot & ((1u << log_grp) - 1u), s2 = slot >> log_grp;
        col = s2 % ncols;
        tile_id = ((((s2 / ncols) << 3) + (blockIdx.x & 7u)) << log_grp) + sub;
    } else { col = blockIdx.x % ncols; tile_id = blockIdx.x / ncols; }
    const uint32_t tiles_per_hi = (uint32_t)((1ull << log_m) >> log_t);
    const uint32_t hi_idx = tile_id / tiles_per_hi, blk = tile_id % tiles_per_hi;
    return PassTile{col, blk, ((uint64_t)hi_idx << (log_np + log_m)) + ((uint64_t)blk << log_t)};
}

// every strided-pass kernel takes the same arguments (one launch site, launch_pass); an instance leaves unused what its options rule out
__global__ void __launch_bounds__(NTT_THREADS)
k_ntt_pass(NttIo io, const Tw29* __restrict__ tw, const Fr* __restrict__ lo, const Fr* __restrict__ hi, int h, int log_np, int log_t, int log_m, int tw_shift,
           const Fr* __restrict__ pre, const Fr* __restrict__ out_tw, uint32_t ncols, int xcd_cols, int log_grp) {
    extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
    const PassTile t = pass_tile(log_np, log_t, log_m, ncols, xcd_cols, log_grp);
    const Lds29 L{smem, 1 << (log_np + log_t)};
    const Fr* __restrict__ src = io.src[t.col];
    Fr* __restrict__ dst = io.dst[t.col];
    for (int s = 0; s < log_np;) {
        const int r = ((log_np - s) & 1) ? 1 : 2;      // radix 2 only in front of an odd digit
        auto step = [&](auto R, auto FIRST, auto LAST) {
            ntt_pass_step<decltype(R)::value, decltype(FIRST)::value, decltype(LAST)::value, OPT_RUNTIME, OPT_RUNTIME>(L, src, dst, tw, pre, out_tw, lo, hi, h, tw_shift, log_np, s, log_t, 1ull << log_m, t.base, t.blk);
        };
        if (s == 0) { if (r == 1) step(Int<1>{}, Bool<true>{}, Bool<false>{}); else step(Int<2>{}, Bool<true>{}, Bool<false>{}); }
        else if (s + r == log_np) step(Int<2>{}, Bool<false>{}, Bool<true>{});
        else step(Int<2>{}, Bool<false>{}, Bool<false>{});
        s += r;
        if (s < log_np) __syncthreads();
    }
}
template <int LOG_NP, int S, bool HAS_PRE>
__device__ __forceinline__ void ntt_pass_steps(const Lds29& L, const Fr* __restrict__ src, Fr* __restrict__ dst, const Tw29* __restrict__ tw,
                                               const Fr* __restrict__ pre, const Fr* __restrict__ out_tw, const int log_t, const uint64_t m, const uint64_t base) {
    constexpr int R = ((LOG_NP - S) & 1) ? 1 : 2;
    constexpr bool LAST = S + R == LOG_NP;
    ntt_pass_step<R, S == 0, LAST, HAS_PRE ? OPT_YES : OPT_NO, OPT_YES>(L, src, dst, tw, pre, out_tw, nullptr, nullptr, 0, 0, LOG_NP, S, log_t, m, base, 0u);
    if constexpr (!LAST) {
        __syncthreads();
        ntt_pass_steps<LOG_NP, S + R, HAS_PRE>(L, src, dst, tw, pre, out_tw, log_t, m, base);
    }
}
template <int LOG_NP, bool HAS_PRE>
__global__ void __launch_bounds__(NTT_THREADS)
k_ntt_pass_f(NttIo io, const Tw29* __restrict__ tw, const Fr* __restrict__ lo, const Fr* __restrict__ hi, int h, int /* LOG_NP */, int log_t, int log_m, int tw_shift,
             const Fr* __restrict__ pre, const Fr* __restrict__ out_tw, uint32_t ncols, int xcd_cols, int log_grp) {
    extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
    const PassTile t = pass_tile(LOG_NP, log_t, log_m, ncols, xcd_cols, log_grp);
    ntt_pass_steps<LOG_NP, 0, HAS_PRE>(Lds29{smem, 1 << (LOG_NP + log_t)}, io.src[t.col], io.dst[t.col], tw, pre, out_tw, log_t, 1ull << log_m, t.base);
}

__host__ __device__ __forceinline__ int ntt_row_pad(int log_np) { return log_np >= 8 ? 8 : 0; }     // <= 16 rows per tile then: at most 128 extra elements
// ----------------------------------------------------------------------------------- last pass
// Rows of n_P contiguous elements; tile = T rows i1 = blk*T + c (row stride = midN * n_P) at a
// fixed middle digit `mid`.  LDS layout [c][d].  Same step structure as the other passes: the
// first step reads the bit-reversed digits of its rows from global memory (32-byte sectors of a
// 32 KiB row, all consumed by this workgroup in the same sweep), the last step writes
// output index = i1 + n1 * (mid + midN * i_P) with c fastest (T consecutive outputs).
// Rows are padded by 8 words (`row`): the last step reads with c fastest (coalesced output), and with a row
// stride that is a multiple of the 32 banks the T rows of a wave would collide on every bank.
// PRE: the coset shift, only when this is the only pass.  FOLDED: the output scale rode on the last inter-pass twiddle and the
// outputs are only reduced; otherwise every output is multiplied by `fin` (1 or the inverse-transform scale, R' form), which
// also brings the lazy sums back below 2p.  A digit of 2 or 4 (log_n = 1, 2) is one step, first and last at once.
// REC: the outputs leave as coset records (ff29.hip.hpp: canonical limbs, split layout over the 2^log_n rows of dst) instead of packed
// elements -- what the quotient evaluator computes on.  Records are only ever a destination, never read back by a transform.
template <int R, bool FIRST, bool LAST, Opt PRE, Opt FOLDED, Opt REC>
__device__ __forceinline__ void ntt_last_step(const Lds29& L, const Fr* __restrict__ src, Fr* __restrict__ dst, const Tw29* __restrict__ tw, const Fr* __restrict__ pre,
                                              const Fr29& fin29, const bool fin_folded, const int log_np, const int s, const int log_t, const int row,
                                              const uint32_t blk, const uint32_t mid, const int log_mid, const int log_n1, const bool records) {
    static_assert(R == 2 || FIRST, "only the first step of a pass can be radix 2");
    constexpr int NE = 1 << R;
    const int hgt = 1 << s, T = 1 << log_t, items = (1 << (log_np + log_t)) >> R;
    const bool has_pre = opt_on<PRE>(pre != nullptr), folded = opt_on<FOLDED>(fin_folded), rec = opt_on<REC>(records);
    for (int it = threadIdx.x; it < items; it += blockDim.x) {
        int c, b;
        if (LAST) { c = it & (T - 1); b = it >> log_t; }                              // c fastest: coalesced output
        else { b = it & ((1 << (log_np - R)) - 1); c = it >> (log_np - R); }          // d fastest: conflict-free LDS
        const int j = b & (hgt - 1);
        const int lo_d = ((b >> s) << (s + R)) | j;
        const uint64_t i1 = ((uint64_t)blk << log_t) + c;
        Fr29 e[4];
        if (FIRST) {
            Fr raw[NE], praw[NE];
            uint64_t gi[NE];
#pragma unroll
            for (int k = 0; k < NE; ++k) {
                gi[k] = (((i1 << log_mid) + mid) << log_np) + bitrev(lo_d + k * hgt, log_np);
                raw[k] = ldg(src + gi[k]);
                if (PRE == OPT_YES) praw[k] = ldg(pre + gi[k]);
            }
#pragma unroll
            for (int k = 0; k < NE; ++k) {
                e[k] = unpack29<Fr29P>(raw[k]);
                if (has_pre) e[k] = mul29(e[k], unpack29<Fr29P>(PRE == OPT_YES ? praw[k] : ldg(pre + gi[k])));      // decided at run time: loaded behind the branch
            }
            dit_first_step<R>(e, tw, log_np);
        } else {
#pragma unroll
            for (int k = 0; k < NE; ++k) e[k] = L.load(c * row + lo_d + k * hgt);
            dit_step<R>(e, tw, log_np, s, j);
        }
#pragma unroll
        for (int k = 0; k < NE; ++k) {
            const int dl = lo_d + k * hgt;
            if (LAST) {
                const uint64_t oi = i1 + (((uint64_t)mid + ((uint64_t)dl << log_mid)) << log_n1);
                if (rec) rec29_store<Fr29P>(dst, 1ull << (log_np + log_mid + log_n1), oi, canon29_lt2p(folded ? reduce_lazy29_limbs(e[k]) : mul29(e[k], fin29)));
                else stg(dst + oi, folded ? reduce_lazy29(e[k]) : pack29_lt2p(mul29(e[k], fin29)));
            } else L.store(c * row + dl, e[k]);
        }
    }
}

// Workgroups go to the eight XCDs round-robin and each XCD has its own L2.  A tile of T rows writes T * 32-byte runs
// (64 B at T = 2), i.e. HALF of every 128-byte line it touches; the other half belongs to the tile next to it.  With the
// plain numbering those two tiles run on different XCDs and each L2 writes its half back on its own (masked partial
// writes); renumbered so that neighbouring tiles are consecutive workgroups of ONE XCD, the halves meet in that L2.
__device__ __forceinline__ uint32_t last_tile(int xcd_remap) {
    return xcd_remap ? (blockIdx.x & 7u) * (gridDim.x >> 3) + (blockIdx.x >> 3) : blockIdx.x;
}

// blockIdx.y = column; the same arguments for every last-pass kernel, as for the strided pass
__global__ void __launch_bounds__(NTT_THREADS)
k_ntt_last(NttIo io, const Tw29* __restrict__ tw, int log_np, int log_t, int log_n1, int log_mid, Fr fin, const Fr* __restrict__ pre, int fin_folded, int xcd_remap, int records) {
    extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
    const Fr* __restrict__ src = io.src[blockIdx.y];
    Fr* __restrict__ dst = io.dst[blockIdx.y];
    const int row = (1 << log_np) + ntt_row_pad(log_np);
    const Lds29 L{smem, row << log_t};
    const uint32_t bx = last_tile(xcd_remap), mid = bx & ((1u << log_mid) - 1), blk = bx >> log_mid;
    const Fr29 fin29 = unpack29<Fr29P>(fin);
    for (int s = 0; s < log_np;) {
        const int r = ((log_np - s) & 1) ? 1 : 2;
        const bool last = s + r == log_np;
        auto step = [&](auto R, auto FIRST, auto LAST) {
            ntt_last_step<decltype(R)::value, decltype(FIRST)::value, decltype(LAST)::value, OPT_RUNTIME, OPT_RUNTIME, OPT_RUNTIME>(L, src, dst, tw, pre, fin29, fin_folded != 0, log_np, s, log_t, row, blk, mid, log_mid, log_n1, records != 0);
        };
        if (s == 0 && last) { if (r == 1) step(Int<1>{}, Bool<true>{}, Bool<true>{}); else step(Int<2>{}, Bool<true>{}, Bool<true>{}); }
        else if (s == 0) { if (r == 1) step(Int<1>{}, Bool<true>{}, Bool<false>{}); else step(Int<2>{}, Bool<true>{}, Bool<false>{}); }
        else if (last) step(Int<2>{}, Bool<false>{}, Bool<true>{});
        else step(Int<2>{}, Bool<false>{}, Bool<false>{});
        s += r;
        if (s < log_np) __syncthreads();
    }
}
// the instances exist for digits of 2^7 and more: at least two steps, no coset shift (not the only pass), the scale folded
template <int LOG_NP, int S, bool REC>
__device__ __forceinline__ void ntt_last_steps(const Lds29& L, const Fr* __restrict__ src, Fr* __restrict__ dst, const Tw29* __restrict__ tw,
                                               const int log_t, const int row, const uint32_t blk, const uint32_t mid, const int log_mid, const int log_n1) {
    constexpr int R = ((LOG_NP - S) & 1) ? 1 : 2;
    constexpr bool LAST = S + R == LOG_NP;
    ntt_last_step<R, S == 0, LAST, OPT_NO, OPT_YES, REC ? OPT_YES : OPT_NO>(L, src, dst, tw, nullptr, Fr29{}, true, LOG_NP, S, log_t, row, blk, mid, log_mid, log_n1, REC);
    if constexpr (!LAST) {
        __syncthreads();
        ntt_last_steps<LOG_NP, S + R, REC>(L, src, dst, tw, log_t, row, blk, mid, log_mid, log_n1);
    }
}
template <int LOG_NP, bool REC>
__global__ void __launch_bounds__(NTT_THREADS)
k_ntt_last_f(NttIo io, const Tw29* __restrict__ tw, int /* LOG_NP */, int log_t, int log_n1, int log_mid, Fr fin, const Fr* __restrict__ pre, int fin_folded, int xcd_remap, int /* REC */) {
    extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
    const int row = (1 << LOG_NP) + ntt_row_pad(LOG_NP);
    const uint32_t bx = last_tile(xcd_remap), mid = bx & ((1u << log_mid) - 1), blk = bx >> log_mid;
    ntt_last_steps<LOG_NP, 0, REC>(Lds29{smem, row << log_t}, io.src[blockIdx.y], io.dst[blockIdx.y], tw, log_t, row, blk, mid, log_mid, log_n1);
}

__global__ void k_scale(Fr* a, Fr s, uint64_t n) {
    uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) stg(a + i, ldg(a + i) * s);
}
int fr_scale_run(zk_ctx* ctx, Fr* d_a, const Fr& s, uint64_t n) {
    if (!n) return ZK_OK;
    hipLaunchKernelGGL(k_scale, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, d_a, s, n);
    ZK_CHECK_LAUNCH(ctx);
    return ZK_OK;
}

// a[i] *= g^i   (EvaluationDomain::distribute_powers_zeta generalised), two-level table of g
__global__ void k_distribute_powers(const Fr* src, Fr* dst, const Fr* __restrict__ lo, const Fr* __restrict__ hi, int h, uint64_t n) {
    uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    stg(dst + i, ldg(src + i) * two_level(lo, hi, h, (uint32_t)i));
}

// ----------------------------------------------------------------------------------- host side
static int build_powers(zk_ctx* ctx, const Fr& base, const Fr& mul, Fr* d_out, uint32_t count, int rprime) {
    hipLaunchKernelGGL(k_powers, dim3((count + 255) / 256), dim3(256), 0, ctx->stream, base, mul, d_out, count, rprime);
    ZK_CHECK_LAUNCH(ctx);
    return ZK_OK;
}

static uint64_t domain_key(uint32_t log_n, const Fr& omega, const Fr* scale) {
    uint64_t hsh = 1469598103934665603ull;
    auto mix = [&](uint32_t v) { hsh = (hsh ^ v) * 1099511628211ull; };
    mix(log_n);
    for (int i = 0; i < 8; ++i) mix(omega.l[i]);
    if (scale) for (int i = 0; i < 8; ++i) mix(scale->l[i] ^ 0x9e3779b9u);
    return hsh;
}

// Measurement knobs (environment variables): read once at the top of a call (ntt_run_many) into this struct, never kept between
// calls -- tests flip them inside one process.  KNOB_UNSET: not set; the range of a knob is checked where it is applied.
constexpr int KNOB_UNSET = INT_MIN;
struct NttKnobs {
    bool fixed;                          // ZK_NTT_FIXED (0: the run-time kernels everywhere)
    bool out_table;                      // ZK_NTT_OUT_TABLE (0: a domain built under it gets no inter-pass twiddle tables, as above 2^24; a cached domain stays as it is)
    int batch;                           // ZK_NTT_BATCH: columns per launch, 1 .. NTT_BATCH
    int pass_logtile, last_logtile;      // ZK_NTT_PASS_LOGTILE, ZK_NTT_LAST_LOGTILE: 10 .. 12
    bool xcd_last;                       // ZK_NTT_XCD (1: last_tile's renumbering; off: neutral at every size, profiles/r03_ntt_xcd.md)
    bool xcd_cols;                       // ZK_NTT_XCD_COLS (0: plain numbering of the strided passes' workgroups)
};
static NttKnobs read_ntt_knobs() {
    auto num = [](const char* name) { const char* e = getenv(name); return e ? atoi(e) : KNOB_UNSET; };
    NttKnobs k;
    k.fixed = num("ZK_NTT_FIXED") != 0;
    k.out_table = num("ZK_NTT_OUT_TABLE") != 0;
    k.batch = num("ZK_NTT_BATCH");
    k.pass_logtile = num("ZK_NTT_PASS_LOGTILE");
    k.last_logtile = num("ZK_NTT_LAST_LOGTILE");
    k.xcd_last = num("ZK_NTT_XCD") == 1;
    k.xcd_cols = num("ZK_NTT_XCD_COLS") != 0;
    return k;
}

// The digit split of a size: P <= 3 passes of at most 2^NTT_MAX_DIGIT points each (log_n, npass and every pass's log_np / log_m).
static void split_digits(NttDomain& d, uint32_t log_n) {
    d.log_n = log_n;
    const int P = log_n <= NTT_MAX_DIGIT ? 1 : (log_n <= 2 * NTT_MAX_DIGIT ? 2 : 3);
    d.npass = P;
    int rem = (int)log_n;
    for (int p = 0; p < P; ++p) {
        int b = (rem + (P - p) - 1) / (P - p);   // ceil split, big digits first
        d.pass[p].log_np = b;
        rem -= b;
        d.pass[p].log_m = rem;
    }
}
// full inter-pass twiddle tables (n x 32 B per non-last pass) while the domain is not huge
static bool tables_fit(uint32_t log_n, int npass) { return npass > 1 && log_n <= 24; }

static int get_domain(zk_ctx* ctx, const NttKnobs& kn, uint32_t log_n, const Fr& omega, const Fr* scale, std::shared_ptr<NttDomain>* out) {
    const uint64_t key = domain_key(log_n, omega, scale);
    auto it = ctx->domains.find(key);
    if (it != ctx->domains.end()) { *out = it->second; return ZK_OK; }
    auto d = std::make_shared<NttDomain>();
    split_digits(*d, log_n);
    d->final_mul = to_rprime(scale ? *scale : Fr::one());
    const int P = d->npass;
    // two-level tables (only needed when P > 1)
    if (P > 1) {
        d->h = (int)(log_n + 1) / 2;
        const uint32_t nlo = 1u << d->h, nhi = 1u << (log_n - d->h);
        ZK_HIP(ctx, hipMalloc(&d->d_lo, sizeof(Fr) * nlo));
        ZK_HIP(ctx, hipMalloc(&d->d_hi, sizeof(Fr) * nhi));
        int rc = build_powers(ctx, omega, Fr::one(), d->d_lo, nlo, 1);
        if (rc) return rc;
        Fr step = omega;
        for (int i = 0; i < d->h; ++i) step = sqr(step);
        rc = build_powers(ctx, step, Fr::one(), d->d_hi, nhi, 1);
        if (rc) return rc;
    }
    for (int p = 0; p < P; ++p) {
        const int b = d->pass[p].log_np;
        const uint32_t cnt = b ? (1u << (b - 1)) : 1u;
        ZK_HIP(ctx, hipMalloc(&d->d_tw[p], sizeof(Fr) * cnt));
        Fr w = omega;
        for (uint32_t i = 0; i < log_n - (uint32_t)b; ++i) w = sqr(w);   // omega^(n/n_p)
        int rc = build_powers(ctx, w, Fr::one(), d->d_tw[p], cnt, 1);
        if (rc) return rc;
        ZK_HIP(ctx, hipMalloc((void**)&d->d_tw29[p], sizeof(Tw29) * cnt));
        hipLaunchKernelGGL(k_split_twiddles, dim3((cnt + 255) / 256), dim3(256), 0, ctx->stream, (const Fr*)d->d_tw[p], d->d_tw29[p], cnt);
        ZK_CHECK_LAUNCH(ctx);
        d->pass[p].tw = d->d_tw29[p];
    }
    if (tables_fit(log_n, P) && kn.out_table) {
        const uint64_t n = 1ull << log_n;
        for (int p = 0; p + 1 < P; ++p) {
            if (hipMalloc(&d->d_out_tw[p], sizeof(Fr) * n) != hipSuccess) { (void)hipGetLastError(); d->d_out_tw[p] = nullptr; break; }
            const NttPass& ps = d->pass[p];
            hipLaunchKernelGGL(k_build_out_twiddles, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, d->d_out_tw[p], (const Fr*)d->d_lo, (const Fr*)d->d_hi, d->h,
                               ps.log_np, ps.log_m, (int)log_n - ps.log_np - ps.log_m, n, d->final_mul, p == P - 2 ? 1 : 0);
            ZK_CHECK_LAUNCH(ctx);
            d->pass[p].out_tw = d->d_out_tw[p];
            if (p == P - 2) d->fin_folded = true;
        }
    }
    if (ctx->domains.size() > 64) ctx->domains.clear();
    ctx->domains[key] = d;
    *out = d;
    return ZK_OK;
}

// Cached power tables of a coset generator g, keyed by (log_n, g, kind); null when there is no memory for a new one.
//   POW_TWO_LEVEL: g^e = tab[e & (2^h - 1)] * tab[2^h + (e >> h)], h = ceil(log_n / 2), R form (k_distribute_powers)
//   POW_FULL:      tab[i] = g^i for every i < n, R' form: the first pass of a transform multiplies it in as it loads
// The coset generators are a handful of constants (zeta, zeta^-1): the tables stay with the context.
enum PowKind { POW_TWO_LEVEL, POW_FULL };
static int get_pow_table(zk_ctx* ctx, uint32_t log_n, const Fr& g, PowKind kind, const Fr** out) {
    *out = nullptr;
    const uint64_t key = domain_key(log_n, g, nullptr) ^ (kind == POW_FULL ? 0xF0117ABull : 0xC05E7ull);
    auto it = ctx->pow_tables.find(key);
    if (it != ctx->pow_tables.end()) { *out = (const Fr*)it->second; return ZK_OK; }
    const int h = (int)(log_n + 1) / 2;
    const uint32_t nlo = kind == POW_FULL ? 1u << log_n : 1u << h, nhi = kind == POW_FULL ? 0u : 1u << (log_n - h);
    Fr* tab = nullptr;
    if (hipMalloc(&tab, sizeof(Fr) * ((size_t)nlo + nhi)) != hipSuccess) { (void)hipGetLastError(); return ZK_OK; }
    int rc = build_powers(ctx, g, Fr::one(), tab, nlo, kind == POW_FULL ? 1 : 0);
    if (!rc && nhi) {
        Fr step = g;
        for (int i = 0; i < h; ++i) step = sqr(step);
        rc = build_powers(ctx, step, Fr::one(), tab + nlo, nhi, 0);
    }
    if (rc) { (void)hipFree(tab); return rc; }
    ctx->pow_tables[key] = tab;
    *out = tab;
    return ZK_OK;
}
// a[i] *= g^i as a pass of its own (EvaluationDomain::distribute_powers_zeta generalised)
static int run_distribute(zk_ctx* ctx, uint32_t log_n, const Fr& g, const Fr* from, Fr* to) {
    const Fr* tab = nullptr;
    int rc = get_pow_table(ctx, log_n, g, POW_TWO_LEVEL, &tab);
    if (rc) return rc;
    if (!tab) return ctx->fail(ZK_ERR_OOM, "coset table allocation failed");
    const int h = (int)(log_n + 1) / 2;
    const uint64_t n = 1ull << log_n;
    hipLaunchKernelGGL(k_distribute_powers, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, from, to, tab, tab + (1u << h), h, n);
    ZK_CHECK_LAUNCH(ctx);
    return ZK_OK;
}

// ---- launch plans: the geometry of one launch, decided on the host before anything is enqueued
struct NttPlan {
    int log_t, tile;          // T = 2^log_t runs (strided pass) or rows (last pass) per workgroup; tile = elements per workgroup
    unsigned blocks;          // tiles per column
    dim3 grid;                // strided pass: (blocks * nb); last pass: (blocks, nb)
    unsigned threads;
    size_t lds;
    int xcd, log_grp;         // XCD-aware workgroup numbering (pass_tile / last_tile), and the tiles per 128-byte line that go with it
    bool fixed;               // a compile-time instance serves this launch
};
static bool has_fixed_instance(int log_np) { return log_np >= 7 && log_np <= NTT_MAX_DIGIT; }      // 7, 8: the three-pass sizes (2^21 .. 2^24)
static unsigned plan_threads(int tile, bool fixed) {
    if (fixed) return (unsigned)std::max(64, std::min(1024, tile >> 2));      // one radix-4 item per thread and step
    return tile >= 4096 ? 1024 : (tile >= 1024 ? 512 : (tile >= 256 ? 128 : 64));
}
// `table`: the pass has its inter-pass twiddle table (NttPass::out_tw)
static NttPlan plan_pass(const NttDomain& dom, int p, size_t nb, const NttKnobs& kn, bool table) {
    const NttPass& ps = dom.pass[p];
    NttPlan pl{};
    // tile of the strided passes: 4096 elements (T = 4: 128-byte runs) when there are two passes; with three passes
    // 2048 elements measured 8-10 % faster (two workgroups per CU: one loads while the other computes)
    int log_tile = dom.npass == 3 ? 11 : 12;
    if (kn.pass_logtile >= 10 && kn.pass_logtile <= 12) log_tile = kn.pass_logtile;
    pl.log_t = std::min(std::max(log_tile - ps.log_np, 0), ps.log_m);
    pl.tile = 1 << (ps.log_np + pl.log_t);
    pl.blocks = (unsigned)((1ull << dom.log_n) >> (ps.log_np + pl.log_t));
    pl.fixed = kn.fixed && table && has_fixed_instance(ps.log_np);
    pl.grid = dim3(pl.blocks * (unsigned)nb);
    pl.threads = plan_threads(pl.tile, pl.fixed);
    pl.lds = (size_t)pl.tile * NTT_LDS_BYTES_PER_ELT;
    const int log_grp = pl.log_t < 2 ? 2 - pl.log_t : 0;           // tiles per 128-byte line of a run
    if (pl.fixed) {
        pl.xcd = (kn.xcd_cols && pl.blocks % (8u << log_grp) == 0 && (nb > 1 || log_grp > 0)) ? 1 : 0;
        pl.log_grp = pl.xcd ? log_grp : 0;
    } else {
        pl.xcd = (nb > 1 && pl.blocks % 8 == 0 && kn.xcd_cols) ? 1 : 0;
    }
    return pl;
}
static NttPlan plan_last(const NttDomain& dom, size_t nb, const NttKnobs& kn) {
    const int P = dom.npass;
    const NttPass& ps = dom.pass[P - 1];
    const int log_n1 = P == 1 ? 0 : dom.pass[0].log_np, log_mid = P == 3 ? dom.pass[1].log_np : 0;
    NttPlan pl{};
    // the last pass reads whole rows: a 2048-element tile (two rows of 2^10, 72 KiB of LDS) lets two workgroups share a CU
    // and overlap their load / compute / store phases: -4 % at 2^20, -5 % at 2^22
    int log_tile = 11;
    if (kn.last_logtile >= 10 && kn.last_logtile <= 12) log_tile = kn.last_logtile;
    pl.log_t = std::min(std::max(log_tile - ps.log_np, 0), log_n1);
    pl.tile = 1 << (ps.log_np + pl.log_t);
    pl.blocks = (unsigned)((1ull << dom.log_n) >> (ps.log_np + pl.log_t));
    pl.fixed = kn.fixed && P > 1 && dom.fin_folded && has_fixed_instance(ps.log_np);      // the instances only reduce: the scale must have been folded
    pl.grid = dim3(pl.blocks, (unsigned)nb);
    pl.threads = plan_threads(pl.tile, pl.fixed);
    pl.lds = (size_t)(pl.tile + (ntt_row_pad(ps.log_np) << pl.log_t)) * NTT_LDS_BYTES_PER_ELT;
    pl.xcd = (log_mid == 0 && pl.blocks % 8 == 0 && pl.blocks >= 16 && kn.xcd_last) ? 1 : 0;
    return pl;
}

// hipFuncSetAttribute (dynamic LDS beyond 64 KiB) is per device: done once per kernel and context.  false: the device refuses the
// size (not a gfx950, a lowered limit) -- an instance then stays unused and the launch takes the generic kernel.
static bool pass_kernel_ready(zk_ctx* ctx, const void* kernel, size_t max_lds) {
    auto it = ctx->ntt_fixed_attr.find(kernel);
    if (it != ctx->ntt_fixed_attr.end()) return it->second;
    const bool ok = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)max_lds) == hipSuccess;
    if (!ok) (void)hipGetLastError();
    return ctx->ntt_fixed_attr[kernel] = ok;
}
constexpr size_t NTT_PASS_MAX_LDS = (size_t)NTT_TILE * NTT_LDS_BYTES_PER_ELT, NTT_LAST_MAX_LDS = (size_t)(NTT_TILE + 128) * NTT_LDS_BYTES_PER_ELT;

using PassKernel = decltype(&k_ntt_pass);
using LastKernel = decltype(&k_ntt_last);
static PassKernel pass_instance(int log_np, bool pre) {
    switch (log_np) {
        case 7: return pre ? k_ntt_pass_f<7, true> : k_ntt_pass_f<7, false>;
        case 8: return pre ? k_ntt_pass_f<8, true> : k_ntt_pass_f<8, false>;
        case 9: return pre ? k_ntt_pass_f<9, true> : k_ntt_pass_f<9, false>;
        default: return pre ? k_ntt_pass_f<10, true> : k_ntt_pass_f<10, false>;
    }
}
static LastKernel last_instance(int log_np, bool rec) {
    switch (log_np) {
        case 7: return rec ? k_ntt_last_f<7, true> : k_ntt_last_f<7, false>;
        case 8: return rec ? k_ntt_last_f<8, true> : k_ntt_last_f<8, false>;
        case 9: return rec ? k_ntt_last_f<9, true> : k_ntt_last_f<9, false>;
        default: return rec ? k_ntt_last_f<10, true> : k_ntt_last_f<10, false>;
    }
}
// strided pass p of the domain; `pre`: the coset shift table of a first pass, or null
static int launch_pass(zk_ctx* ctx, const NttDomain& dom, int p, size_t nb, const NttKnobs& kn, const NttIo& io, const Fr* pre) {
    const NttPass& ps = dom.pass[p];
    if (ps.log_np < 3) return ctx->fail(ZK_ERR_INVALID_ARG, "NTT: a strided pass over a digit of 2^%d", ps.log_np);      // its steps have no first-and-last instantiation
    NttPlan pl = plan_pass(dom, p, nb, kn, ps.out_tw != nullptr);
    PassKernel kernel = pl.fixed ? pass_instance(ps.log_np, pre != nullptr) : k_ntt_pass;
    if (pl.fixed && !pass_kernel_ready(ctx, (const void*)kernel, NTT_PASS_MAX_LDS)) {
        NttKnobs generic = kn;
        generic.fixed = false;
        pl = plan_pass(dom, p, nb, generic, ps.out_tw != nullptr);
        kernel = k_ntt_pass;
    }
    if (!pl.fixed && !pass_kernel_ready(ctx, (const void*)kernel, NTT_PASS_MAX_LDS)) return ctx->fail(ZK_ERR_HIP, "NTT: the device refuses %zu bytes of LDS per workgroup", NTT_PASS_MAX_LDS);
    ZkProfScope pscope(ctx, "ntt_pass");
    pscope.bytes = (uint64_t)nb * (1ull << dom.log_n) * 64 / (uint64_t)dom.npass;      // a transform's algorithmic 64 B per element (read once, write once), spread over its P launches
    hipLaunchKernelGGL(kernel, pl.grid, dim3(pl.threads), pl.lds, ctx->stream, io, ps.tw, (const Fr*)dom.d_lo, (const Fr*)dom.d_hi, dom.h, ps.log_np, pl.log_t, ps.log_m,
                       (int)dom.log_n - ps.log_np - ps.log_m, pre, ps.out_tw, (uint32_t)nb, pl.xcd, pl.log_grp);
    ZK_CHECK_LAUNCH(ctx);
    return ZK_OK;
}
// `pre`: the coset shift table when this is the only pass, or null; `records`: the outputs are coset records (36 bytes per row at io.dst)
static int launch_last(zk_ctx* ctx, const NttDomain& dom, size_t nb, const NttKnobs& kn, const NttIo& io, const Fr* pre, bool records) {
    const int P = dom.npass;
    const NttPass& ps = dom.pass[P - 1];
    NttPlan pl = plan_last(dom, nb, kn);
    LastKernel kernel = pl.fixed ? last_instance(ps.log_np, records) : k_ntt_last;
    if (pl.fixed && !pass_kernel_ready(ctx, (const void*)kernel, NTT_LAST_MAX_LDS)) {
        NttKnobs generic = kn;
        generic.fixed = false;
        pl = plan_last(dom, nb, generic);
        kernel = k_ntt_last;
    }
    if (!pl.fixed && !pass_kernel_ready(ctx, (const void*)kernel, NTT_LAST_MAX_LDS)) return ctx->fail(ZK_ERR_HIP, "NTT: the device refuses %zu bytes of LDS per workgroup", NTT_LAST_MAX_LDS);
    ZkProfScope pscope(ctx, "ntt_last");
    pscope.bytes = (uint64_t)nb * (1ull << dom.log_n) * 64 / (uint64_t)P;
    hipLaunchKernelGGL(kernel, pl.grid, dim3(pl.threads), pl.lds, ctx->stream, io, ps.tw, ps.log_np, pl.log_t, P == 1 ? 0 : dom.pass[0].log_np, P == 3 ? dom.pass[1].log_np : 0,
                       dom.final_mul, pre, dom.fin_folded ? 1 : 0, pl.xcd, records ? 1 : 0);
    ZK_CHECK_LAUNCH(ctx);
    return ZK_OK;
}

// Columns per launch of a call over `count` columns: enough tiles to give every CU a few workgroups (ntt_run_many lowers it when the
// scratch for that many columns cannot be had).  A coset shift that is a pass of its own is per column: one column per launch.
static size_t columns_per_launch(uint32_t log_n, size_t count, bool coset_pass, const NttKnobs& kn) {
    if (count <= 1 || coset_pass) return 1;
    const uint64_t tiles = std::max<uint64_t>(1, (1ull << log_n) >> 12);
    size_t per_launch = (size_t)std::min<uint64_t>(NTT_BATCH, std::max<uint64_t>(1, 4096 / tiles));       // sixteen columns at 2^20: a launch's last round of workgroups and the 10-20 us between dependent launches are paid once per sixteen columns (headline proof, alternating A/B on one box: 1.006 s with four, 0.9855 with eight, 0.9793 with sixteen; alone the transform does not care: 94.8 / 94.6 us)
    if (kn.batch >= 1 && kn.batch <= NTT_BATCH) per_launch = (size_t)kn.batch;
    return per_launch;
}

// Generic driver.  `scale` (nullable) multiplies every output; coset_pre (nullable): a[i] *= g^i
// before the transform; coset_post (nullable): out[i] *= g^i after it.  d_src (nullable): the input
// is read from d_src and d_data only receives the result (out of place, no extra copy).
// `count` transforms over the same domain, in place (d_srcs == nullptr) or from d_srcs[i] to d_datas[i]; launched
// NTT_BATCH columns at a time.  The coset shifts that are passes of their own (coset_post, and coset_pre when it is not
// fused into the first pass) are per column: those transforms go one column per launch group.
int ntt_run(zk_ctx* ctx, Fr* d_data, uint32_t log_n, const Fr& omega, const Fr* scale, const Fr* coset_pre, const Fr* coset_post, const Fr* d_src, bool fuse_pre) {
    return ntt_run_many(ctx, &d_data, d_src ? &d_src : nullptr, 1, log_n, omega, scale, coset_pre, coset_post, fuse_pre);
}
int ntt_run_many(zk_ctx* ctx, Fr* const* d_datas, const Fr* const* d_srcs, size_t count, uint32_t log_n, const Fr& omega, const Fr* scale, const Fr* coset_pre, const Fr* coset_post, bool fuse_pre) {
    return ntt_run_many_fmt(ctx, d_datas, d_srcs, count, log_n, omega, scale, coset_pre, coset_post, fuse_pre, false);
}
// records: d_datas[i] (36 bytes per row, ff29.hip.hpp) receives the transform as coset records, written by the last pass alone: every
// transform needs a source of its own and no pass may follow the last one (coset_post).  Until then the buffer serves as it always did
// (the first of three passes and a coset shift without a table park packed elements in its first 32 bytes per row).
int ntt_run_many_fmt(zk_ctx* ctx, Fr* const* d_datas, const Fr* const* d_srcs, size_t count, uint32_t log_n, const Fr& omega, const Fr* scale, const Fr* coset_pre, const Fr* coset_post, bool fuse_pre,
                     bool records) {
    if (count == 0) return ZK_OK;
    if (records) {
        if (coset_post || log_n == 0 || !d_srcs) return ctx->fail(ZK_ERR_INVALID_ARG, "NTT: record output needs a source of its own, one row at least and no pass behind the transform");
        for (size_t i = 0; i < count; ++i) if (!d_srcs[i] || d_srcs[i] == d_datas[i]) return ctx->fail(ZK_ERR_INVALID_ARG, "NTT: record output in place");
    }
    const NttKnobs kn = read_ntt_knobs();
    if (log_n == 0) {   // size-1 transforms: identity (times the scale)
        for (size_t i = 0; i < count; ++i) {
            if (d_srcs && d_srcs[i] && d_srcs[i] != d_datas[i]) ZK_HIP(ctx, hipMemcpyAsync(d_datas[i], d_srcs[i], sizeof(Fr), hipMemcpyDeviceToDevice, ctx->stream));
            if (scale) {
                hipLaunchKernelGGL(k_scale, dim3(1), dim3(64), 0, ctx->stream, d_datas[i], *scale, (uint64_t)1);
                ZK_CHECK_LAUNCH(ctx);
            }
        }
        return ZK_OK;
    }
    const uint64_t n = 1ull << log_n;
    const Fr* pre_table = nullptr;       // full table g^i (R' form), multiplied in by the first pass as it loads; no memory for it: the separate pass
    int rc = (coset_pre && fuse_pre) ? get_pow_table(ctx, log_n, *coset_pre, POW_FULL, &pre_table) : ZK_OK;
    if (rc) return rc;
    const bool pre_apart = coset_pre && !pre_table;
    std::shared_ptr<NttDomain> dom;
    rc = get_domain(ctx, kn, log_n, omega, scale, &dom);
    if (rc) return rc;
    const int P = dom->npass;
    size_t per_launch = columns_per_launch(log_n, count, pre_apart || coset_post, kn);       // fewer below when the scratch for them cannot be had
    Fr* scratch = nullptr;
    if (P > 1) {
        // transforms on the auxiliary stream run BESIDE transforms of the main stream (coset transforms ahead of the quotient,
        // prover.hip): the intermediate buffer of a multi-pass transform is per stream
        // sixteen columns per launch take 512 MiB of scratch per stream at 2^20: on a device that cannot spare it, fewer columns per launch (slower, not fatal)
        const int slot = ctx->stream_aux && ctx->stream == ctx->stream_aux ? SC_NTT_AUX : SC_NTT;
        for (;;) {
            scratch = (Fr*)ctx->get_scratch(slot, sizeof(Fr) * n * per_launch);
            if (scratch || per_launch == 1) break;
            (void)hipGetLastError();
            per_launch = (per_launch + 1) / 2;
        }
        if (!scratch) return ZK_ERR_OOM;
    }
    for (size_t first = 0; first < count; first += per_launch) {
        const size_t nb = std::min(per_launch, count - first);
        // buffers: P=1: data->data (whole transform inside one workgroup, safe in place)
        //          P=2: data->scratch, scratch->data;   P=3: data->data, data->scratch, scratch->data
        NttIo io{};                                            // .src = where the next pass reads
        for (size_t j = 0; j < nb; ++j) {
            Fr* dd = d_datas[first + j];
            io.src[j] = d_srcs && d_srcs[first + j] ? d_srcs[first + j] : dd;
            if (pre_apart) { rc = run_distribute(ctx, log_n, *coset_pre, io.src[j], dd); if (rc) return rc; io.src[j] = dd; }
        }
        for (int p = 0; p + 1 < P; ++p) {
            for (size_t j = 0; j < nb; ++j) io.dst[j] = (p == P - 2) ? scratch + j * n : d_datas[first + j];
            rc = launch_pass(ctx, *dom, p, nb, kn, io, p == 0 ? pre_table : nullptr);
            if (rc) return rc;
            for (size_t j = 0; j < nb; ++j) io.src[j] = io.dst[j];
        }
        for (size_t j = 0; j < nb; ++j) io.dst[j] = d_datas[first + j];
        rc = launch_last(ctx, *dom, nb, kn, io, P == 1 ? pre_table : nullptr, records);
        if (rc) return rc;
        if (coset_post) for (size_t j = 0; j < nb; ++j) { rc = run_distribute(ctx, log_n, *coset_post, io.dst[j], io.dst[j]); if (rc) return rc; }
    }
    return ZK_OK;
}

// `count` polynomials on the coset g H, packed or as the records the quotient's class programs read: 32 x the value, the factor
// being the transform's output scale (one more cached domain per size; it rides on the last inter-pass twiddle table for nothing)
int coeff_to_coset_batch_fmt(zk_ctx* ctx, const void* const* d_coeffs, uint32_t k, const Fr& g, void* const* d_outs, size_t count, bool records) {
    const Fr s32 = fr_from_u64(32);
    return ntt_run_many_fmt(ctx, (Fr* const*)d_outs, (const Fr* const*)d_coeffs, count, k, fr_root_of_unity(k), records ? &s32 : nullptr, &g, nullptr, /*fuse_pre=*/true, records);
}

// ---- one transform spread over several GPUs (SURVEY 8e "domain halves": the 4-step split) ------
// n = W * m with W = world.  Write i = i1 + W * i2 and j = j2 + m * j1:
//   X[j2 + m j1] = sum_{i1} w_W^(i1 j1) * [ w_n^(i1 j2) * sum_{i2} x[i1 + W i2] w_m^(i2 j2) ]
// Rank i1 owns the residue class x[i1 + W i2]: a local size-m transform with the twiddle
// w_n^(i1 j2) folded in as its output scaling, ONE all-to-all (rank c receives the j2 slice
// [c m/W, (c+1) m/W) from everyone), and W-point butterflies across the received rows.
template <int W>
__global__ void __launch_bounds__(256) k_ntt_cross(const Fr* __restrict__ recv, Fr* __restrict__ out, size_t cols, const Fr* __restrict__ tw /* w_W^t, t < W/2 */, Fr scale, int scaled) {
    const size_t c = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= cols) return;
    constexpr int LOGW = W == 2 ? 1 : W == 4 ? 2 : W == 8 ? 3 : 4;
    Fr a[W];
#pragma unroll
    for (int i = 0; i < W; ++i) {
        int rev = 0;
#pragma unroll
        for (int b = 0; b < LOGW; ++b) rev |= ((i >> b) & 1) << (LOGW - 1 - b);
        a[rev] = ldg(recv + (size_t)i * cols + c);
    }
#pragma unroll
    for (int st = 1; st <= LOGW; ++st) {
#pragma unroll
        for (int h = 0; h < W / 2; ++h) {                  // butterfly h of this stage: block h / half, lane t
            const int half = 1 << (st - 1), t = h & (half - 1), lo = ((h >> (st - 1)) << st) + t, hi = lo + half;
            const Fr u = a[lo];
            const Fr v = t == 0 ? a[hi] : a[hi] * tw[t << (LOGW - st)];
            a[lo] = u + v;
            a[hi] = u - v;
        }
    }
#pragma unroll
    for (int j = 0; j < W; ++j) stg(out + (size_t)j * cols + c, scaled ? a[j] * scale : a[j]);
}

}  // namespace zk

using namespace zk;
// Host only: the launch plans a transform of `columns` columns of 2^log_n elements follows under the knobs in force, out of the same
// split_digits / columns_per_launch / plan_pass / plan_last as ntt_run_many and its launch sites.  What it leaves out is what only
// a device decides: ntt_run_many's fewer columns per launch when the scratch for them cannot be had, a domain whose tables found no
// memory, and the generic kernel a launch takes when the device refuses an instance its LDS size (the plan BEFORE that fallback).
// The records describe the first launch group; the smaller group that ends a call of, say, 17 columns has the plans of a call with
// that many columns.  `tables` states what the domain is: kn.out_table only acts when get_domain builds one and is not consulted.
extern "C" int zk_host_ntt_plan(uint32_t log_n, size_t columns, int tables, int coset_pass, uint32_t* out_head, uint32_t* out_records, size_t cap_records, uint32_t* out_launches) {
    if (!out_head || !out_launches || log_n < 1 || log_n > 28 || columns < 1 || (!out_records && cap_records)) return ZK_ERR_INVALID_ARG;
    const NttKnobs kn = read_ntt_knobs();
    NttDomain dom;
    split_digits(dom, log_n);
    const int P = dom.npass;
    const bool table = tables && tables_fit(log_n, P);
    dom.fin_folded = table;
    const size_t per_launch = columns_per_launch(log_n, columns, coset_pass != 0, kn), nb = std::min(per_launch, columns);
    out_head[0] = (uint32_t)per_launch;
    out_head[1] = (uint32_t)nb;
    out_head[2] = (uint32_t)P;
    out_head[3] = table ? 1u : 0u;
    *out_launches = (uint32_t)P;
    if (cap_records < (size_t)P) return out_records ? ZK_ERR_INVALID_ARG : ZK_OK;
    for (int p = 0; p < P; ++p) {
        const bool last = p == P - 1;
        const NttPlan pl = last ? plan_last(dom, nb, kn) : plan_pass(dom, p, nb, kn, table);
        const uint32_t rec[ZK_NTT_PLAN_WORDS] = {last ? 1u : 0u, (uint32_t)p, (uint32_t)P, (uint32_t)dom.pass[p].log_np, (uint32_t)dom.pass[p].log_m, (uint32_t)pl.log_t, pl.blocks,
                                                 pl.grid.x, pl.grid.y, pl.threads, (uint32_t)pl.lds, pl.fixed ? 1u : 0u, (uint32_t)pl.xcd, (uint32_t)pl.log_grp};
        memcpy(out_records + (size_t)p * ZK_NTT_PLAN_WORDS, rec, sizeof rec);
    }
    return ZK_OK;
}
extern "C" int zk_ntt_sharded(zk_ctx* ctx, void* d_local, uint32_t log_n, int inverse, uint32_t rank, uint32_t world, zk_alltoall_fn exchange, void* user) {
    if (!ctx) return ZK_ERR_INVALID_ARG;
    ZK_REQUIRE(ctx, d_local, "null pointer");
    ZK_REQUIRE(ctx, exchange || world == 1 || (comm_ready(ctx) && ctx->comm_world == world && ctx->comm_rank == rank), "no all-to-all callback and no matching communicator (zk_comm_init)");
    ZK_REQUIRE(ctx, world >= 1 && world <= 16 && (world & (world - 1)) == 0 && rank < world, "world must be a power of two <= 16, rank < world");
    ZK_REQUIRE(ctx, log_n <= 28, "log_n exceeds the two-adicity of Fr (28)");
    uint32_t log_w = 0;
    while ((1u << log_w) < world) ++log_w;
    ZK_REQUIRE(ctx, log_n >= 2 * log_w, "need n >= world^2");
    if (world == 1) return zk_ntt(ctx, d_local, log_n, inverse);
    const uint32_t log_m = log_n - log_w;
    const size_t m = (size_t)1 << log_m, cols = m >> log_w;
    Fr w_n = fr_root_of_unity(log_n), w_m = fr_root_of_unity(log_m), w_w = fr_root_of_unity(log_w);
    if (inverse) { w_n = fr_inv_host(w_n); w_m = fr_inv_host(w_m); w_w = fr_inv_host(w_w); }
    // steps 1 + 2: local transform over <w_m>, then element j2 times w_n^(rank * j2)
    const Fr g = fr_pow(w_n, rank);
    int rc = ntt_run(ctx, (Fr*)d_local, log_m, w_m, nullptr, nullptr, rank ? &g : nullptr);
    if (rc) return rc;
    // step 3: the exchange.  d_local is already [peer][cols]; the callback returns with d_recv complete
    Fr* recv = (Fr*)ctx->pool_get(m * sizeof(Fr));
    Fr* d_tw = (Fr*)ctx->pool_get(16 * sizeof(Fr));
    if (!recv || !d_tw) { ctx->pool_put(recv, m * sizeof(Fr)); ctx->pool_put(d_tw, 16 * sizeof(Fr)); return ctx->fail(ZK_ERR_OOM, "sharded NTT: exchange buffer of %zu bytes", m * sizeof(Fr)); }
    auto done = [&](int code) { ctx->pool_put(recv, m * sizeof(Fr)); ctx->pool_put(d_tw, 16 * sizeof(Fr)); return code; };
    hipError_t e = hipSuccess;
    if (exchange) {
        e = hipStreamSynchronize(ctx->stream);       // a callback runs on the caller's own stream
        if (e != hipSuccess) return done(ctx->fail(ZK_ERR_HIP, "sharded NTT: %s", hipGetErrorString(e)));
        if (exchange(user, d_local, cols * sizeof(Fr), recv) != 0) return done(ctx->fail(ZK_ERR_INVALID_ARG, "sharded NTT: the all-to-all callback failed"));
    } else {
        // in-library RCCL: W - 1 grouped send / receive pairs on this stream, no host synchronisation between
        // the local transform, the exchange and the cross butterflies
        rc = comm_alltoall_dev(ctx, d_local, cols * sizeof(Fr), recv);
        if (rc) return done(rc);
    }
    // step 4: W-point transforms across the received rows, 1/n folded in for the inverse
    Fr tw[8];
    tw[0] = Fr::one();
    for (uint32_t t = 1; t < (world > 1 ? world / 2 : 1); ++t) tw[t] = tw[t - 1] * w_w;
    e = hipMemcpyAsync(d_tw, tw, sizeof(Fr) * (world / 2 ? world / 2 : 1), hipMemcpyHostToDevice, ctx->stream);
    if (e != hipSuccess) return done(ctx->fail(ZK_ERR_HIP, "sharded NTT: %s", hipGetErrorString(e)));
    const Fr ninv = inverse ? fr_inv_host(fr_from_u64(1ull << log_n)) : Fr::one();
    const dim3 grid((unsigned)((cols + 255) / 256)), block(256);
    switch (world) {
        case 2: hipLaunchKernelGGL(k_ntt_cross<2>, grid, block, 0, ctx->stream, (const Fr*)recv, (Fr*)d_local, cols, (const Fr*)d_tw, ninv, inverse); break;
        case 4: hipLaunchKernelGGL(k_ntt_cross<4>, grid, block, 0, ctx->stream, (const Fr*)recv, (Fr*)d_local, cols, (const Fr*)d_tw, ninv, inverse); break;
        case 8: hipLaunchKernelGGL(k_ntt_cross<8>, grid, block, 0, ctx->stream, (const Fr*)recv, (Fr*)d_local, cols, (const Fr*)d_tw, ninv, inverse); break;
        default: hipLaunchKernelGGL(k_ntt_cross<16>, grid, block, 0, ctx->stream, (const Fr*)recv, (Fr*)d_local, cols, (const Fr*)d_tw, ninv, inverse); break;
    }
    e = hipGetLastError();
    if (e != hipSuccess) return done(ctx->fail(ZK_ERR_HIP, "sharded NTT: %s", hipGetErrorString(e)));
    e = hipStreamSynchronize(ctx->stream);     // tw lives on this frame
    if (e != hipSuccess) return done(ctx->fail(ZK_ERR_HIP, "sharded NTT: %s", hipGetErrorString(e)));
    return done(ZK_OK);
}

// Quotient-polynomial evaluation over the extended domain: halo2_proofs
// plonk::evaluation::{Evaluator::evaluate_h, GraphEvaluator} + vanishing divide_by_vanishing_poly
// (external crate; reached from create_proof, reference call sites A1-A3).
//
// The host flattens every constraint of the circuit -- custom gates, permutation and lookup
// identities alike -- into one postfix program over *columns in extended-coset evaluation form*
// (halo2's `Calculation` / `ValueSource` list, restated as a stack machine):
//
//      PUSH_COL c, rot     push column c at row (i + rot * 2^(ext_k - k)) mod 2^ext_k
//      PUSH_CONST j        push consts[j]              (constants, challenges, beta/gamma/theta)
//      ADD SUB MUL NEG SQUARE DOUBLE MUL_CONST j ADD_CONST j
//      FOLD j              acc = acc * consts[j] + pop()     (the `acc * y + term` folding)
//      TEE_TMP t           tmp[t] = top (stack unchanged)    -- halo2's GraphEvaluator keeps every shared
//      PUSH_TMP t          push tmp[t]                          sub-expression as an intermediate; a value used by
//                                                               several gates is computed once and parked here
//      END
//
// One lane per extended-domain row; control flow is uniform across the grid (every lane runs the
// same instruction), so there is no divergence.  The two topmost operands live in registers, deeper
// ones in LDS laid out [slot][limb][lane] (4-byte strided: bank-conflict-free), column reads are fully coalesced for
// rot = 0 and shifted-coalesced for rot != 0.  The result is multiplied by the precomputed
// 1/(X^n - 1) on the coset (period 2^(ext_k-k)) before it is written.
// HBM side: 32 B per (column, rotation) read + 32 B written per row -- the streaming-bound member
// of the path.
//
// Arithmetic: the stack machine computes on nine 29-bit limbs (ff29.hip.hpp) -- the carry-free
// Montgomery product runs 1.6x faster than the 8 x 32 CIOS one.  Stack values stay in halo2curves'
// R = 2^256 Montgomery form.  mul29 divides by R' = 2^261, so a product of two R-form values
// multiplies one operand by 32 first (a 5-bit limb shift, folded into the unpacking of a memory
// operand); constants that only ever multiply (MUL_CONST, FOLD, the vanishing inverses) are
// tabulated in R' form instead and need no shift.
//
// Lowering (host, `lower_program` in quotient_lower.hpp): the caller's postfix program is rebuilt as expression trees and
// re-emitted for the machine the kernel really implements --
//   * every binary operation whose right (or, for ADD / MUL / SUB, left) operand is a column, a
//     parked intermediate or a constant takes that operand from memory (ADD_COL, SUB_COL, RSUB_COL,
//     MUL_COL, FOLD_COL, ADD_CONST, MUL_CONST): a gate like q * (a * b - c) runs as
//     PUSH a, MUL_COL b, SUB_COL c, MUL_COL q, FOLD with no stack traffic at all;
//   * the memory operand of instruction pc + 1 is loaded before instruction pc executes (its ~1000
//     ALU cycles cover the load), instruction words are fetched two ahead;
//   * sums are not reduced when they are produced: the lowering tracks, per stack entry, a bound on
//     the value (in multiples of p) and on the limbs (in multiples of 2^29) and sets "settle this
//     operand first" bits only where the consumer's precondition would fail (the bounds: head of quotient_lower.hpp).
// Results are bit-identical to the plain evaluation: every step is exact arithmetic mod p and the
// value written is the canonical representative.
//
// Round 6: two kernels run a lowered program -- k_quotient_eval2 (the default: one stack entry in registers, in-place products, the loop
// body a flat chain of single-armed ifs over a host-made class mask) and k_quotient_eval (round 5's, ZK_QUOTIENT_KERNEL=1), bit-identical.
// A large program that is a sum of terms and reads its operands many times is cut into slices that run side by side over the same rows
// and find each other's operands in the caches (plan_slices).
//
// The instruction set, the lowering with its bounds, the slicer, the knobs and the launch plan are host-only code in quotient_lower.hpp;
// this file has the kernels and the short host path that follows a plan.
#include "ctx.hpp"
#include "ff29.hip.hpp"
#include "quotient_lower.hpp"

namespace zk {

using Q29 = F29<Fr29P>;
static_assert(QL_OK == ZK_OK && QL_INVALID_ARG == ZK_ERR_INVALID_ARG && QL_UNSUPPORTED == ZK_ERR_UNSUPPORTED, "quotient_lower.hpp restates the statuses");
static_assert(Q_REC_ROW_BYTES == REC29_BYTES && Q_ROW_BYTES == sizeof(Fr), "quotient_lower.hpp restates the row sizes");

// limb idx of K*p, normalised (limbs 0..7 < 2^29)
template <class P>
__host__ __device__ constexpr uint32_t kp_norm(int K, int idx) {
    uint64_t carry = 0;
    uint32_t out = 0;
    for (int i = 0; i <= idx; ++i) {
        const uint64_t v = (uint64_t)K * P::M(i) + carry;
        out = i < 8 ? (uint32_t)(v & MASK29) : (uint32_t)v;
        carry = v >> 29;
    }
    return out;
}
// r (limbs < 2^31, value < 4p) -> normalised representative below 2p: carry-propagate, then subtract
// 2p with a signed borrow chain and keep the difference unless it went negative
__device__ __forceinline__ Q29 q_settle(Q29 r) {
    normalize29(r);
    Q29 d;
    int32_t c = 0;
#pragma unroll
    for (int i = 0; i < 9; ++i) {
        const int32_t s_ = (int32_t)r.l[i] - (int32_t)kp_norm<Fr29P>(2, i) + c;
        d.l[i] = i < 8 ? ((uint32_t)s_ & MASK29) : (uint32_t)s_;
        c = s_ >> 29;
    }
    const bool neg_ = (int32_t)d.l[8] < 0;
#pragma unroll
    for (int i = 0; i < 9; ++i) r.l[i] = neg_ ? r.l[i] : d.l[i];
    return r;
}
// r (limbs < 2^31, value < 8p) -> normalised representative below 2p: one more round for the values the relaxed bounds let grow past 4p
__device__ __forceinline__ Q29 q_settle8(Q29 r) {
    normalize29(r);
    Q29 d;
    int32_t c = 0;
#pragma unroll
    for (int i = 0; i < 9; ++i) {
        const int32_t s_ = (int32_t)r.l[i] - (int32_t)kp_norm<Fr29P>(4, i) + c;
        d.l[i] = i < 8 ? ((uint32_t)s_ & MASK29) : (uint32_t)s_;
        c = s_ >> 29;
    }
    const bool neg_ = (int32_t)d.l[8] < 0;
#pragma unroll
    for (int i = 0; i < 9; ++i) r.l[i] = neg_ ? r.l[i] : d.l[i];
    return q_settle(r);
}
__device__ __forceinline__ Q29 q_add(const Q29& a, const Q29& b) { return q_settle(add29(a, b)); }          // a, b < 2p
__device__ __forceinline__ Q29 q_sub(const Q29& a, const Q29& b) { return q_settle(sub29k<2>(a, b)); }      // a - b + 2p in (0, 4p)
// x * 32 for a normalised x < 2p: limbs stay normalised, value < 64p < 2^260
__device__ __forceinline__ Q29 q_shl5(const Q29& x) {
    Q29 r;
    r.l[0] = (x.l[0] << 5) & MASK29;
#pragma unroll
    for (int i = 1; i < 8; ++i) r.l[i] = ((x.l[i] << 5) & MASK29) | (x.l[i - 1] >> 24);
    r.l[8] = (x.l[8] << 5) | (x.l[7] >> 24);
    return r;
}
__device__ __forceinline__ Q29 q_mul(const Q29& a, const Q29& b) { return mul29(a, q_shl5(b)); }            // R-form x R-form -> R-form, < 2p

// A program constant as the kernel reads it: the nine 29-bit limbs, unpacked on the host once per launch (the kernel used to
// spend 27 vector instructions per constant operand on it).  The index is wave-uniform, so the limbs arrive by scalar loads
// and stay in scalar registers (mul29_ub).  64-byte records.
struct QC29 { uint32_t l[16]; };
static_assert(sizeof(QC29) == Q_CONST_BYTES, "quotient_lower.hpp restates the size of a constant record");

struct QStack {
    uint32_t* base;   // [slot][limb][lane], nine raw limbs: a spilled value keeps its (possibly unsettled) form
    __device__ __forceinline__ Q29 get(int slot) const {
        Q29 r;
#pragma unroll
        for (int k = 0; k < 9; ++k) r.l[k] = base[(slot * 9 + k) * Q_THREADS + threadIdx.x];
        return r;
    }
    __device__ __forceinline__ void put(int slot, const Q29& v) const {
#pragma unroll
        for (int k = 0; k < 9; ++k) base[(slot * 9 + k) * Q_THREADS + threadIdx.x] = v.l[k];
    }
};
// limbs of 32 * a for a < 2^256 (the R -> R' step of a product, folded into the unpacking)
__device__ __forceinline__ Q29 unpack29_x32(const Fr& a) {
    Q29 r;
    r.l[0] = (a.l[0] << 5) & MASK29;
#pragma unroll
    for (int i = 1; i < 9; ++i) {
        const int bit = 29 * i - 5, w = bit >> 5, sh = bit & 31;
        uint32_t v = a.l[w] >> sh;
        if (sh > 3 && w + 1 < 8) v |= a.l[w + 1] << (32 - sh);
        r.l[i] = i == 8 ? v : (v & MASK29);
    }
    return r;
}

// Runs a LOWERED program (lower_program, quotient_lower.hpp): `prog` holds prog_len instructions followed by two END triples.
// FULL: the grid covers the domain exactly (2^ext_k >= Q_THREADS), no lane needs masking.
#ifdef Q_WAVES_PER_EU
#define Q_OCC_ATTR __attribute__((amdgpu_waves_per_eu(Q_WAVES_PER_EU, Q_WAVES_PER_EU)))
#else
#define Q_OCC_ATTR
#endif
// ACC_MEM (round 6): the accumulator of the FOLD instructions lives in memory ([limb][row], raw limbs), not in registers.  A compiled
// class program folds once per factor group -- 82 FOLDs in 34 185 instructions of the EVM-style program -- yet as a loop-carried
// register value the accumulator was copied (nine v_mov) at the end of EVERY case of the interpreter's switch, whichever instruction
// ran.  Programs that fold on most instructions (linear combinations: FOLD_COL chains) keep it in registers (ACC_MEM = false).
// K_FIRST_FOLD marks the first fold of a program: the accumulator is zero there, nothing is read.
template <bool FULL, bool ACC_MEM>
__global__ void __launch_bounds__(Q_THREADS) Q_OCC_ATTR
k_quotient_eval(const uint32_t* __restrict__ prog, uint32_t prog_len, const Fr* const* __restrict__ cols, const QC29* __restrict__ consts,
                const QC29* __restrict__ consts_rp /* the same constants in R' form */, const Fr* __restrict__ t_evals /* R' form */, uint32_t ext_k, uint32_t k,
                Fr* __restrict__ out, Fr* tmp /* [slot][row]: the row's intermediates, written and read by its own lane */, uint32_t* acc_mem /* ACC_MEM: [limb][row] */) {
    extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
    QStack st{smem};
    const uint64_t ne = 1ull << ext_k;
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;            // ext_k <= 28: row indices fit 32 bits
    const bool live = FULL || i < (uint32_t)ne;
    const uint32_t rot_scale = 1u << (ext_k - k), row_mask = (uint32_t)ne - 1u;
    const Q29 zero29 = unpack29<Fr29P>(Fr::zero());
    Q29 acc = zero29;                         // ACC_MEM: unused (dead), the folds go through acc_mem
    // The two topmost stack elements live in registers (t0 = top, t1 = second); element j < sp - 2
    // lives in LDS slot j.
    Q29 t0 = zero29, t1 = zero29;
    int sp = 0;
    auto push_shift = [&]() {                 // makes room on top: the caller writes t0 next
        if (sp >= 2) st.put(sp - 2, t1);
        t1 = t0;
        ++sp;
    };
    auto drop_to = [&](const Q29& top) {      // two operands consumed, `top` is the new top of stack
        --sp;
        t0 = top;
        if (sp >= 2) t1 = st.get(sp - 2);
    };
    // A column pointer comes out of a table in memory, so the compiler cannot tell its address space and would emit FLAT loads;
    // those count on lgkmcnt as well as vmcnt, and every wait for a scalar load (instruction words, constants) would then also wait
    // for the operand that is being prefetched.  The columns are device memory: say so (global_load, vmcnt only).
    typedef uint32_t U32x4 __attribute__((ext_vector_type(4)));
    using GU4 = const U32x4 __attribute__((address_space(1)));
    using GU1 = uint32_t __attribute__((address_space(1)));
    auto load_row = [&](uint32_t a, uint32_t row) -> Fr {
        GU4* q = (GU4*)(uintptr_t)(cols[a] + row);
        const U32x4 lo = q[0], hi = q[1];
        Fr r;
        r.l[0] = lo.x; r.l[1] = lo.y; r.l[2] = lo.z; r.l[3] = lo.w;
        r.l[4] = hi.x; r.l[5] = hi.y; r.l[6] = hi.z; r.l[7] = hi.w;
        return r;
    };
    auto load = [&](uint32_t a, uint32_t b) -> Fr {
        const uint32_t row = (i + b * rot_scale) & row_mask;          // b = the rotation as a two's complement word: wraps like the domain
        if (FULL) return load_row(a, row);
        return live ? load_row(a, row) : Fr::zero();
    };
    auto cst = [&](const QC29* __restrict__ tab, uint32_t j) -> Q29 {
        Q29 r;
#pragma unroll
        for (int q = 0; q < 9; ++q) r.l[q] = tab[j].l[q];
        return r;
    };
    auto acc_get = [&](uint32_t w0_) -> Q29 {
        if (!ACC_MEM) return acc;
        Q29 r = zero29;
        if (!(w0_ & K_FIRST_FOLD) && live) {
            GU1* q = (GU1*)(uintptr_t)(acc_mem + i);
#pragma unroll
            for (int l = 0; l < 9; ++l) r.l[l] = q[(uint64_t)l << ext_k];
        }
        return r;
    };
    auto acc_put = [&](const Q29& v) {
        if (!ACC_MEM) { acc = v; return; }
        if (live) {
            GU1* q = (GU1*)(uintptr_t)(acc_mem + i);
#pragma unroll
            for (int l = 0; l < 9; ++l) q[(uint64_t)l << ext_k] = v.l[l];
        }
    };
    // Instruction words are fetched two ahead, the memory operand one ahead: the load of instruction pc + 1 is in flight while
    // instruction pc computes.  The raw operand `m` of instruction pc is unpacked into limbs FIRST, then the same registers take the
    // load for pc + 1 (no m_cur = m_next rotation: eight register copies an iteration).
    uint32_t w0 = prog[0], w1 = prog[1], w2 = prog[2];
    uint32_t n0 = prog[3], n1 = prog[4], n2 = prog[5];
    Fr m;                                      // only read by instructions that have a memory operand, which loaded it
    if (k_has_mem(w0)) m = load(w1, w2);
    for (uint32_t pc = 0; pc < prog_len; ++pc) {
        const uint32_t f0 = prog[3 * pc + 6], f1 = prog[3 * pc + 7], f2 = prog[3 * pc + 8];
        const uint32_t op = w0 & 0xffu;
        if (op == Q_END) break;
        Q29 mq = zero29;
        if (k_has_mem(w0)) mq = op == K_MUL_COL ? unpack29_x32(m) : unpack29<Fr29P>(m);
        if (k_has_mem(n0)) m = load(n1, n2);
        if (w0 & (K_SETTLE0 | K_SETTLE1 | K_NORM0 | K_NORM1 | K_SETTLE0_8 | K_SETTLE1_8)) {        // one test on the common path (three instructions in four carry no flag)
            if (w0 & K_SETTLE0) t0 = q_settle(t0);
            if (w0 & K_SETTLE1) t1 = q_settle(t1);
            if (w0 & K_NORM0) normalize29(t0);
            if (w0 & K_NORM1) normalize29(t1);
            if (w0 & K_SETTLE0_8) t0 = q_settle8(t0);
            if (w0 & K_SETTLE1_8) t1 = q_settle8(t1);
        }
        switch (op) {
            case Q_PUSH_COL: push_shift(); t0 = mq; break;
            case Q_PUSH_CONST: push_shift(); t0 = cst(consts, w1); break;
            case Q_ADD: drop_to(add29(t1, t0)); break;
            case Q_SUB: { Q29 d = sub29k<2>(t1, t0); normalize29(d); drop_to(d); break; }     // the top limb of a settled subtrahend may borrow: carry it out before anyone multiplies
            case Q_MUL: drop_to(mul29(t1, q_shl5(t0))); break;
            case Q_NEG: t0 = sub29k<2>(zero29, t0); normalize29(t0); break;
            case Q_SQUARE: t0 = mul29(t0, q_shl5(t0)); break;
            case Q_DOUBLE: t0 = add29(t0, t0); break;
            case Q_FOLD: acc_put(add29(mul29_ub(acc_get(w0), cst(consts_rp, w1)), t0)); drop_to(t1); break;
            case Q_MUL_CONST: t0 = mul29_ub(t0, cst(consts_rp, w1)); break;
            case Q_ADD_CONST: t0 = add29(t0, cst(consts, w1)); break;
            case Q_TEE_TMP: if (live) stg(tmp + (((uint64_t)w1 << ext_k) + i), pack29_lt2p(t0)); break;             // parked canonical: read back as a column
            case K_ADD_COL: t0 = add29(t0, mq); break;
            case K_SUB_COL: t0 = sub29k<2>(t0, mq); break;                                  // canonical subtrahend: its top limb is below that of 2p, no borrow (with K = 1 the top limb of p - b could borrow)
            case K_RSUB_COL: t0 = sub29k<2>(mq, t0); normalize29(t0); break;
            case K_MUL_COL: t0 = mul29(t0, mq); break;
            case K_FOLD_COL: acc_put(add29(mul29_ub(acc_get(w0), cst(consts_rp, w0 >> K_CONST_SHIFT)), mq)); break;
            default: break;
        }
        w0 = n0; w1 = n1; w2 = n2;
        n0 = f0; n1 = f1; n2 = f2;
    }
    if (live) {
        Q29 a = acc_get(0);
        if (t_evals) stg(out + i, pack29_lt2p(mul29(a, unpack29<Fr29P>(ldg(t_evals + (i & (rot_scale - 1u)))))));
        else { normalize29(a); stg(out + i, reduce_lazy29(a)); }       // acc < 6p, never settled on the way
    }
}

// ---- the interpreter with fixed register roles (round 6, second half) ----------------------------------------------------------
// k_quotient_eval above keeps the two topmost stack entries in registers and lets every case of its switch produce NEW values for
// them: the ISA carries 18 + 18 v_mov per interpreted instruction (the phi copies of t0 and t1 at the join, whichever case ran) on top
// of the rotations t1 = t0 of a push -- 1.3 M of the 5.3 M vector instructions a wave spends on the EVM-style class program.  Here
//   * ONE stack entry lives in registers (t0); every deeper entry is in LDS (a binary stack operation reads its other operand from
//     there: nine ds_read instead of eighteen v_mov);
//   * every operation UPDATES t0 IN PLACE -- the products through asm statements whose result takes the first factor's registers
//     (mul29_ipa / mul29_ub_ipa / mul29_ipb: limb j of the factor is last read one column before result limb j is written), sums and
//     differences limb by limb -- and the loop body is a flat chain of single-armed ifs over a class mask (QClass below), so its joins have nothing to copy;
//   * the second operand B (a memory operand unpacked on arrival, or the stack entry below the top) has its own nine registers and
//     dies with the instruction;
//   * memory operands are unpacked with v_alignbit (16 / 17 instructions instead of 27).
// Same instruction set, same lowering, same bounds (quotient_lower.hpp); bit-identical results.  ZK_QUOTIENT_KERNEL=1 runs the older kernel.
__device__ __forceinline__ void q_unpack_to(Q29& r, const Fr& a) {
    r.l[0] = a.l[0] & MASK29;
#pragma unroll
    for (int i = 1; i < 8; ++i) {
        const int bit = 29 * i, w = bit >> 5, sh = bit & 31;
        r.l[i] = __builtin_amdgcn_alignbit(a.l[w + 1], a.l[w], sh) & MASK29;
    }
    r.l[8] = a.l[7] >> 8;
}
__device__ __forceinline__ void q_unpack_x32_to(Q29& r, const Fr& a) {       // limbs of 32 * a
    r.l[0] = (a.l[0] << 5) & MASK29;
#pragma unroll
    for (int i = 1; i < 8; ++i) {
        const int bit = 29 * i - 5, w = bit >> 5, sh = bit & 31;
        r.l[i] = __builtin_amdgcn_alignbit(a.l[w + 1], a.l[w], sh) & MASK29;
    }
    r.l[8] = a.l[7] >> 3;
}
__device__ __forceinline__ void q_shl5_ip(Q29& x) {                          // x <- 32 x (normalised x < 2p), top down so that no limb is read after it is written
    x.l[8] = (x.l[8] << 5) | (x.l[7] >> 24);
#pragma unroll
    for (int i = 7; i >= 1; --i) x.l[i] = ((x.l[i] << 5) & MASK29) | (x.l[i - 1] >> 24);
    x.l[0] = (x.l[0] << 5) & MASK29;
}
__device__ __forceinline__ void q_settle_ip(Q29& r) {
    normalize29(r);
    uint32_t d[9];
    int32_t c = 0;
#pragma unroll
    for (int i = 0; i < 9; ++i) {
        const int32_t s_ = (int32_t)r.l[i] - (int32_t)kp_norm<Fr29P>(2, i) + c;
        d[i] = i < 8 ? ((uint32_t)s_ & MASK29) : (uint32_t)s_;
        c = s_ >> 29;
    }
    const bool neg_ = (int32_t)d[8] < 0;
#pragma unroll
    for (int i = 0; i < 9; ++i) r.l[i] = neg_ ? r.l[i] : d[i];
}
__device__ __forceinline__ void q_settle8_ip(Q29& r) {
    normalize29(r);
    uint32_t d[9];
    int32_t c = 0;
#pragma unroll
    for (int i = 0; i < 9; ++i) {
        const int32_t s_ = (int32_t)r.l[i] - (int32_t)kp_norm<Fr29P>(4, i) + c;
        d[i] = i < 8 ? ((uint32_t)s_ & MASK29) : (uint32_t)s_;
        c = s_ >> 29;
    }
    const bool neg_ = (int32_t)d[8] < 0;
#pragma unroll
    for (int i = 0; i < 9; ++i) r.l[i] = neg_ ? r.l[i] : d[i];
    q_settle_ip(r);
}


// `prog`: 4-word instructions (word 0: opcode + settle bits [+ constant of FOLD_COL], 1 / 2: operands, 3: class mask), prog_len of them
// followed by END quadruples for the fetch-ahead.
// REC (the class programs of a proof): every column, parked intermediates included, is a coset record buffer of 2^ext_k rows (ff29.hip.hpp)
// holding 32 x the value, i.e. the R' = 2^261 form of what a packed column holds in R form.  A memory operand then arrives as the limbs the
// products take: no unpacking.  With EVERY value in R' form -- operands, stack, accumulator, additive constants (consts_rp) -- a product
// reduced by 2^261 is R' again and sums are linear, so the x 32 variants are the plain ones and no stack product shifts: the same lowered
// words, the result 32 x what the packed program gives (the caller's scale takes the 1/32).  Operands are canonical where the packed ones
// were up to 32 p: every bound of lower_bounds holds as it stands.
template <bool FULL, bool ACC_MEM, bool REC>
__global__ void __launch_bounds__(Q_THREADS) Q_OCC_ATTR
k_quotient_eval2(const uint32_t* __restrict__ prog, uint32_t prog_len, const Fr* const* __restrict__ cols, const QC29* __restrict__ consts,
                 const QC29* __restrict__ consts_rp /* the same constants in R' form */, const Fr* __restrict__ t_evals /* R' form */, uint32_t ext_k, uint32_t k,
                 Fr* __restrict__ out, Fr* tmp /* [slot][row] */, uint32_t* acc_mem /* ACC_MEM: [limb][row] */, uint32_t tile_alias /* measurement only, see the launch */,
                 const uint32_t* __restrict__ slice_tab /* per slice: first word of its instructions, their number */, uint32_t num_slices /* 0: one program for every workgroup */) {
    extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
    // stack entry j < sp - 1 lives in LDS slot j ([slot][limb][lane]); entry sp - 1 is t0.  ONE address register (slot and lane; made opaque so
    // that the compiler does not split it into nine loop-invariant lane addresses + nine adds per access), the limb in the instruction's offset field.
    auto st_addr = [&](int slot) -> uint32_t {
        uint32_t a = (uint32_t)slot * (9u * Q_THREADS * 4u) + threadIdx.x * 4u;
        asm volatile("" : "+v"(a));
        return a;
    };
    auto st_put = [&](int slot, const Q29& v) {
        const uint32_t a = st_addr(slot);
#pragma unroll
        for (int q = 0; q < 9; ++q) *(uint32_t*)((char*)smem + a + q * (Q_THREADS * 4)) = v.l[q];
    };
    auto st_get = [&](int slot, Q29& v) {
        const uint32_t a = st_addr(slot);
#pragma unroll
        for (int q = 0; q < 9; ++q) v.l[q] = *(const uint32_t*)((const char*)smem + a + q * (Q_THREADS * 4));
    };
    const uint64_t ne = 1ull << ext_k;
    uint32_t blk = blockIdx.x;
    if (tile_alias) { const uint32_t xcd = blk & 7u, j = blk >> 3; blk = ((j >> tile_alias) << 3) | xcd; }       // 2^tile_alias consecutive workgroups of an XCD share one row tile (results wrong)
    if (num_slices) {
        // A sliced program (see zk_quotient_eval): workgroup ids go round the XCDs, so ids 8 j + x, j = t S ... t S + S - 1, are S workgroups that start
        // together on XCD x -- they take the S slices of ONE row tile and find each other's operands in that XCD's L2 / the Infinity Cache.
        const uint32_t xcd = blk & 7u, j = blk >> 3, sl = j % num_slices;
        blk = ((j / num_slices) << 3) | xcd;
        prog += slice_tab[2 * sl];
        prog_len = slice_tab[2 * sl + 1];
        out += (size_t)sl << ext_k;
    }
    // The trip count is the same for every lane; said outright, because the record-mode instantiations otherwise keep the loop counter in a
    // vector register (decrement, compare and three stray v_readfirstlane: five vector instructions per interpreted instruction).
    prog_len = __builtin_amdgcn_readfirstlane(prog_len);
    const uint32_t i = blk * blockDim.x + threadIdx.x;
    const bool live = FULL || i < (uint32_t)ne;
    const uint32_t rot_scale = 1u << (ext_k - k), row_mask = (uint32_t)ne - 1u;
    Q29 t0, acc, B;
#pragma unroll
    for (int q = 0; q < 9; ++q) { t0.l[q] = 0; acc.l[q] = 0; B.l[q] = 0; }        // acc: registers only when !ACC_MEM
    int sp = 0;
    typedef uint32_t U32x4 __attribute__((ext_vector_type(4)));
    using GU4 = const U32x4 __attribute__((address_space(1)));
    using GU1 = uint32_t __attribute__((address_space(1)));
    // The raw memory operand stays in the two 4-register tuples the loads write (unpacked from there: no copies between the load and its use)
    struct Raw { U32x4 lo, hi; uint32_t top; };                       // top: the ninth limb of a record (REC only)
    auto load = [&](uint32_t a, uint32_t b, Raw& r) {
        const uint32_t row = (i + b * rot_scale) & row_mask;          // b = the rotation as a two's complement word: wraps like the domain
        if (FULL || live) {
            const Fr* col = cols[a];
            if (REC && ZK_REC29_AOS) {                                 // 36-byte rows (A/B builds, ff29.hip.hpp)
                typedef U32x4 U32x4A __attribute__((aligned(4)));
                using GU4A = const U32x4A __attribute__((address_space(1)));
                const char* p = (const char*)col + (size_t)row * REC29_BYTES;
                r.lo = *(GU4A*)(uintptr_t)p; r.hi = *(GU4A*)(uintptr_t)(p + 16);
                r.top = *(const GU1*)(uintptr_t)(p + 32);
            } else if (REC) {
                // record buffers have 2^26 rows at most (the host refuses more): the row's byte offsets fit 32 bits, and a wave-uniform base with
                // a 32-bit lane offset is an addressing mode of the load -- no 64-bit address arithmetic per operand
                using GC = const char __attribute__((address_space(1)));
                GC* base = (GC*)(uintptr_t)col;
                GC* p = base + (uint32_t)(row << 5);
                r.lo = *(GU4*)p; r.hi = *(GU4*)(p + 16);
                r.top = *(const GU1*)(base + (ne << 5) + (uint32_t)(row << 2));
            } else {
                GU4* q = (GU4*)(uintptr_t)(col + row);
                r.lo = q[0]; r.hi = q[1];
            }
        }
    };
    auto raw_limbs = [](Q29& d, Raw& r) {   // REC: the operand as it arrived (opaque for the same reason as raw_fr)
        asm volatile("" : "+v"(r.lo), "+v"(r.hi), "+v"(r.top));
        d.l[0] = r.lo.x; d.l[1] = r.lo.y; d.l[2] = r.lo.z; d.l[3] = r.lo.w;
        d.l[4] = r.hi.x; d.l[5] = r.hi.y; d.l[6] = r.hi.z; d.l[7] = r.hi.w;
        d.l[8] = r.top;
    };
    auto raw_fr = [](Raw& r) -> Fr {        // opaque: each unpack site unpacks for itself (the compiler otherwise unpacks on EVERY instruction and copies)
        asm volatile("" : "+v"(r.lo), "+v"(r.hi));
        Fr x;
        x.l[0] = r.lo.x; x.l[1] = r.lo.y; x.l[2] = r.lo.z; x.l[3] = r.lo.w;
        x.l[4] = r.hi.x; x.l[5] = r.hi.y; x.l[6] = r.hi.z; x.l[7] = r.hi.w;
        return x;
    };
    auto cst = [&](const QC29* __restrict__ tab, uint32_t j) -> Q29 {       // wave-uniform index: scalar loads, the limbs stay in scalar registers
        Q29 r;
#pragma unroll
        for (int q = 0; q < 9; ++q) r.l[q] = tab[j].l[q];
        return r;
    };
    // acc <- acc * c + v  (v: limbs below 3 x 2^29)
    auto fold = [&](uint32_t w0_, const Q29& c, const Q29& v) {
        if (!ACC_MEM) {
            mul29_ub_ipa(acc, c);
#pragma unroll
            for (int q = 0; q < 9; ++q) acc.l[q] += v.l[q];
            return;
        }
        Q29 a;
#pragma unroll
        for (int q = 0; q < 9; ++q) a.l[q] = 0;
        uint32_t ii = i;
        asm volatile("" : "+v"(ii));              // the nine limb addresses are made here, not kept in eighteen registers across the loop
        GU1* qa = (GU1*)(uintptr_t)(acc_mem + ii);
        if (!(w0_ & K_FIRST_FOLD) && live) {
#pragma unroll
            for (int l = 0; l < 9; ++l) a.l[l] = qa[(uint64_t)l << ext_k];
        }
        mul29_ub_ipa(a, c);
        if (live) {
#pragma unroll
            for (int l = 0; l < 9; ++l) qa[(uint64_t)l << ext_k] = a.l[l] + v.l[l];
        }
    };
    uint32_t w0 = prog[0], w1 = prog[1], w2 = prog[2], w3 = prog[3];
    uint32_t n0 = prog[4], n1 = prog[5], n2 = prog[6], n3 = prog[7];
    Raw m;
    m.lo = U32x4{0, 0, 0, 0}; m.hi = U32x4{0, 0, 0, 0}; m.top = 0;
    if (w3 & C_HASMEM) load(w1, w2, m);
    for (uint32_t pc = 0; pc < prog_len; ++pc) {
        const uint32_t f0 = prog[4 * pc + 8], f1 = prog[4 * pc + 9], f2 = prog[4 * pc + 10], f3 = prog[4 * pc + 11];
        // no test for END: it is the last of the prog_len instructions (the host counts it in) and its class mask is empty, so it runs as a
        // step that does nothing.  A second way out of the loop made the record-mode instantiations keep the trip count in a vector register.
        // 1. operands: a memory operand leaves its raw registers (which then take the load for instruction pc + 1), a binary stack operation
        //    takes the entry below the top
        if (w3 & C_SPILL) { if (sp >= 1) st_put(sp - 1, t0); ++sp; }
        if (w3 & C_UNPACK_T) { if (REC) raw_limbs(t0, m); else q_unpack_to(t0, raw_fr(m)); }
        if (w3 & C_UNPACK_T32) {                                            // PUSH_COL32: the flags are for the entry that leaves the registers (X of the MAC2_COL to come)
            if (w0 & K_SETTLE0) q_settle_ip(t0);
            if (w0 & K_NORM0) normalize29(t0);
            if (w0 & K_SETTLE0_8) q_settle8_ip(t0);
            st_put(sp - 1, t0);
            ++sp;
            if (REC) raw_limbs(t0, m); else q_unpack_x32_to(t0, raw_fr(m));
        }
        if (REC) { if (w3 & (C_UNPACK_B | C_UNPACK_B32)) raw_limbs(B, m); }
        else {
            if (w3 & C_UNPACK_B) q_unpack_to(B, raw_fr(m));
            if (w3 & C_UNPACK_B32) q_unpack_x32_to(B, raw_fr(m));
        }
        if (w3 & C_POP_B) { st_get(sp - 2, B); --sp; }
        if (!REC) { if (n3 & C_HASMEM) load(n1, n2, m); }
        // 2. settle / carry-propagation requests of the lowering (bit 0: the top, bit 1: the entry below it = B)
        if (w3 & C_FLAGS) {
            if (w0 & K_SETTLE0) q_settle_ip(t0);
            if (w0 & K_SETTLE1) q_settle_ip(B);
            if (w0 & K_NORM0) normalize29(t0);
            if (w0 & K_NORM1) normalize29(B);
            if (w0 & K_SETTLE0_8) q_settle8_ip(t0);
            if (w0 & K_SETTLE1_8) q_settle8_ip(B);
        }
        if (REC) {
            // ADD_COL / SUB_COL read the operand where it arrived (behind the requests for t0: one instruction in four has any), and only
            // then do those registers take the load for instruction pc + 1
            // (two single-armed ifs like every other step: an if / else has a join, and the join copies t0)
            if (w3 & C_ADDM) {
                Q29 M;
                raw_limbs(M, m);                       // names for the arrived registers: read once each, no copy survives
#pragma unroll
                for (int q = 0; q < 9; ++q) t0.l[q] += M.l[q];
            }
            if (w3 & C_SUBM) {                         // canonical subtrahend: its top limb is below that of 2p, no borrow
                Q29 M;
                raw_limbs(M, m);
#pragma unroll
                for (int q = 0; q < 9; ++q) t0.l[q] = t0.l[q] + kp_balanced<Fr29P>(2, q) - M.l[q];
            }
            if (n3 & C_HASMEM) load(n1, n2, m);
        }
        // 3. the operation, on t0 in place
        if (w3 & C_MULV) mul29_ipa(t0, B);
        if (w3 & C_MULC) mul29_ub_ipa(t0, cst(consts_rp, w1));
        if (w3 & C_MACC) {                                                  // S = the entry below the top: its bounds never ask for a settle (lower_bounds)
            Q29 S;
            st_get(sp - 2, S);
            --sp;
            mul2add29_ub_ipa(t0, B, S, cst(consts_rp, w0 >> K_CONST_SHIFT));
        }
        if (w3 & C_MAC2) {                                                  // below the top: 32 m1, X, S -- none of them ever carries a settle request here (lower_bounds)
            Q29 M1, X, S;
            st_get(sp - 2, M1);
            st_get(sp - 3, X);
            st_get(sp - 4, S);
            sp -= 3;
            mul3add29_ub_ipa(t0, B, X, M1, S, cst(consts_rp, w0 >> K_CONST_SHIFT));
        }
        if (w3 & C_ADDV) {
#pragma unroll
            for (int q = 0; q < 9; ++q) t0.l[q] += B.l[q];
        }
        if (w3 & C_SUBV) {                                                  // canonical subtrahend: its top limb is below that of 2p, no borrow
#pragma unroll
            for (int q = 0; q < 9; ++q) t0.l[q] = t0.l[q] + kp_balanced<Fr29P>(2, q) - B.l[q];
        }
        if (w3 & C_FOLDC) fold(w0, cst(consts_rp, w0 >> K_CONST_SHIFT), B);
        if (w3 & C_RARE) {
            if (w3 & C_PUSHC) {
                const Q29 c = cst(REC ? consts_rp : consts, w1);
#pragma unroll
                for (int q = 0; q < 9; ++q) t0.l[q] = c.l[q];
            }
            if (w3 & C_ADDC) {
                const Q29 c = cst(REC ? consts_rp : consts, w1);
#pragma unroll
                for (int q = 0; q < 9; ++q) t0.l[q] += c.l[q];
            }
            if (w3 & C_RSUB) {                                              // B - t0 (t0 settled): carry the borrow of the top limb out before anyone multiplies
#pragma unroll
                for (int q = 0; q < 9; ++q) t0.l[q] = B.l[q] + kp_balanced<Fr29P>(2, q) - t0.l[q];
                normalize29(t0);
            }
            if (w3 & C_MULS) { if (!REC) q_shl5_ip(t0); mul29_ipb(t0, B); }  // t0 <- mul29(B, 32 t0)
            if (w3 & C_MACS) {                                              // t0 <- mul2add29(B, 32 t0, S, const): t0 settled, B popped above, S below it
                Q29 S;
                st_get(sp - 2, S);
                --sp;
                if (!REC) q_shl5_ip(t0);
                mul2add29_ub_ipb(t0, B, S, cst(consts_rp, w0 >> K_CONST_SHIFT));
            }
            if (w3 & C_NEG) {
#pragma unroll
                for (int q = 0; q < 9; ++q) t0.l[q] = kp_balanced<Fr29P>(2, q) - t0.l[q];
                normalize29(t0);
            }
            if (w3 & C_SQ) { Q29 s2 = t0; if (!REC) q_shl5_ip(s2); mul29_ipa(t0, s2); }
            if (w3 & C_DBL) {
#pragma unroll
                for (int q = 0; q < 9; ++q) t0.l[q] <<= 1;
            }
            if (w3 & C_TEE) {
                if (live) {
                    if (REC) rec29_store<Fr29P>((Fr*)((char*)tmp + (((uint64_t)w1 << ext_k) * REC29_BYTES)), ne, i, canon29_lt2p(t0));      // slot w1 of the record-sized slots
                    else stg(tmp + (((uint64_t)w1 << ext_k) + i), pack29_lt2p(t0));
                }
            }
            if (w3 & C_FOLD) { fold(w0, cst(consts_rp, w1), t0); --sp; if (sp >= 1) st_get(sp - 1, t0); }
        }
        w0 = n0; w1 = n1; w2 = n2; w3 = n3;
        n0 = f0; n1 = f1; n2 = f2; n3 = f3;
    }
    if (live) {
        Q29 a = acc;
        if (ACC_MEM) {
            GU1* qa = (GU1*)(uintptr_t)(acc_mem + i);
#pragma unroll
            for (int l = 0; l < 9; ++l) a.l[l] = qa[(uint64_t)l << ext_k];
        }
        if (t_evals) stg(out + i, pack29_lt2p(mul29(a, unpack29<Fr29P>(ldg(t_evals + (i & (rot_scale - 1u)))))));
        else { normalize29(a); stg(out + i, reduce_lazy29(a)); }
    }
}


// t_evaluations[j] = 1 / ((zeta * w_ext^j)^n - 1), j < 2^(ext_k - k)   (EvaluationDomain::new)
static void vanishing_inverses(uint32_t k, uint32_t ext_k, std::vector<Fr>* out) {
    const uint32_t cnt = 1u << (ext_k - k);
    Fr zn = fr_zeta();
    for (uint32_t i = 0; i < k; ++i) zn = sqr(zn);            // zeta^n
    Fr step = fr_root_of_unity(ext_k);
    for (uint32_t i = 0; i < k; ++i) step = sqr(step);        // w_ext^n
    out->resize(cnt);
    Fr cur = zn;
    for (uint32_t j = 0; j < cnt; ++j) {
        (*out)[j] = fr_inv_host(cur - Fr::one());
        cur = cur * step;
    }
}

}  // namespace zk

using namespace zk;

// The lowering as a host-only entry point (no device involved): what the kernel will run for a program.  Used by the
// CPU tests, which execute the lowered stream limb by limb and check every bound the kernel relies on.
extern "C" int zk_host_quotient_lower(const uint32_t* h_program, uint32_t num_instr, uint32_t num_cols, int fuse, uint32_t* out_words, size_t cap_words,
                                      uint32_t* out_instr, int* out_depth) {
    return zk_host_quotient_lower2(h_program, num_instr, num_cols, fuse, out_words, cap_words, out_instr, out_depth, nullptr);
}
// ... and how many MAC2_COL fusions (fuse & 4) were declined because they would have deepened the stack
extern "C" int zk_host_quotient_lower2(const uint32_t* h_program, uint32_t num_instr, uint32_t num_cols, int fuse, uint32_t* out_words, size_t cap_words,
                                       uint32_t* out_instr, int* out_depth, uint32_t* out_declined) {
    if (!h_program || !out_instr || !out_depth) return ZK_ERR_INVALID_ARG;
    if (out_declined) *out_declined = 0;
    if (check_program(h_program, num_instr, false).status) return ZK_ERR_INVALID_ARG;
    std::vector<LowInstr> low;
    int depth = 0;
    if (lower_program(h_program, num_instr, num_cols, fuse, QuotientEvalKnobs::read().relaxed != 0, &low, &depth, out_declined)) return ZK_ERR_INVALID_ARG;
    *out_instr = (uint32_t)low.size();
    *out_depth = depth;
    if (out_words) {
        if (cap_words < low.size() * 3) return ZK_ERR_INVALID_ARG;
        for (size_t i = 0; i < low.size(); ++i) { out_words[3 * i] = low[i].w0; out_words[3 * i + 1] = low[i].a; out_words[3 * i + 2] = low[i].b; }
    }
    return ZK_OK;
}

// where a launch over packed columns would cut the program (a record session cuts for its larger rows: zk_host_quotient_launch shows those)
extern "C" int zk_host_quotient_slices(const uint32_t* program, uint32_t num_instr, uint32_t ext_k, uint32_t* out_cuts, size_t cap, uint32_t* out_count) {
    if (!program || !out_count) return ZK_ERR_INVALID_ARG;
    SlicePlan plan;
    *out_count = 0;
    if (!plan_slices(program, num_instr, ext_k, &plan, sizeof(Fr), QuotientEvalKnobs::read().slices)) return ZK_OK;
    *out_count = (uint32_t)plan.cut.size();
    if (out_cuts) {
        if (cap < plan.cut.size()) return ZK_ERR_INVALID_ARG;
        for (size_t i = 0; i < plan.cut.size(); ++i) out_cuts[i] = plan.cut[i];
    }
    return ZK_OK;
}

// The launch plan as a host-only entry point: zkmi355.h gives the head record
extern "C" int zk_host_quotient_launch(const uint32_t* program, uint32_t num_instr, uint32_t num_cols, uint32_t num_consts, uint32_t ext_k, int records,
                                       uint32_t* out_head, uint32_t* out_words, size_t cap_words, size_t* out_count) {
    if (!program || !out_head || !out_count || ext_k > 28 || (!out_words && cap_words)) return ZK_ERR_INVALID_ARG;
    QuotientLaunch q;
    const int rc = plan_quotient_launch(program, num_instr, num_cols, num_consts, ext_k, records != 0, QuotientEvalKnobs::read(), &q, nullptr);
    if (rc) return rc;
    const uint32_t head[ZK_QUOTIENT_LAUNCH_HEAD] = {(uint32_t)q.kernel, q.records, q.full, q.acc_in_mem, q.sliced, q.S, (uint32_t)q.depth, (uint32_t)q.lds, q.num_tmp, q.low_len, q.folds,
                                                    q.words_per_instr, (uint32_t)q.comb_at, (uint32_t)q.slice_tab_at, (uint32_t)q.prog_bytes, (uint32_t)q.col_bytes, (uint32_t)q.const_bytes, q.tile_alias};
    std::copy(head, head + ZK_QUOTIENT_LAUNCH_HEAD, out_head);
    *out_count = q.words.size();
    if (q.words.size() > cap_words) return cap_words ? ZK_ERR_INVALID_ARG : ZK_OK;
    std::copy(q.words.begin(), q.words.end(), out_words);
    return ZK_OK;
}

// packed column of n rows -> coset record buffer: row i <- the canonical limbs of 32 src[i]
__global__ void k_to_records(const Fr* __restrict__ src, Fr* __restrict__ dst, uint64_t n) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    Fr x = ldg(src + i);
    for (int j = 0; j < 5; ++j) x = dbl(x);
    rec29_store<Fr29P>(dst, n, i, unpack29<Fr29P>(x));
}

extern "C" int zk_quotient_eval(zk_ctx* ctx, const uint32_t* h_program, uint32_t num_instr, const void* const* h_col_ptrs, uint32_t num_cols,
                                const void* h_consts, uint32_t num_consts, uint32_t k, uint32_t ext_k, int divide_by_vanishing, void* d_out) {
    if (!ctx) return ZK_ERR_INVALID_ARG;
    // Measurement knob (tools/quot_evm_loop.py): ZK_QUOTIENT_LOOP_RECORDS=1 runs the program in record mode over images of the caller's
    // columns, converted ONCE per buffer address and kept until the context goes -- a buffer rewritten in between keeps its stale image,
    // so this is for timing loops over fixed columns only.  The result is brought back from 32 x the value by one scaling pass.
    if (QuotientEvalKnobs::read().loop_records && h_program && d_out && (h_col_ptrs || !num_cols) && ext_k >= 2 && ext_k <= 28) {
        const uint64_t ne = 1ull << ext_k;
        std::vector<const void*> recs(num_cols);
        for (uint32_t c = 0; c < num_cols; ++c) {
            ZK_REQUIRE(ctx, h_col_ptrs[c], "null column pointer");
            auto it = ctx->loop_records.find(h_col_ptrs[c]);
            if (it == ctx->loop_records.end()) {
                void* img = nullptr;
                ZK_HIP(ctx, hipMalloc(&img, ne * REC29_BYTES));
                it = ctx->loop_records.emplace(h_col_ptrs[c], img).first;
                hipLaunchKernelGGL(k_to_records, dim3((unsigned)((ne + 255) / 256)), dim3(256), 0, ctx->stream, (const Fr*)h_col_ptrs[c], (Fr*)img, ne);
                ZK_CHECK_LAUNCH(ctx);
            }
            recs[c] = it->second;
        }
        int rc = zk::quotient_eval_fmt(ctx, h_program, num_instr, recs.data(), num_cols, h_consts, num_consts, k, ext_k, divide_by_vanishing, d_out, true);
        if (rc) return rc;
        return fr_scale_run(ctx, (Fr*)d_out, fr_inv_host(fr_from_u64(32)), ne);
    }
    return zk::quotient_eval_fmt(ctx, h_program, num_instr, h_col_ptrs, num_cols, h_consts, num_consts, k, ext_k, divide_by_vanishing, d_out, false);
}

// The twelve interpreter instantiations by what selects them; the large dynamic LDS is allowed on each once per context, and a launch takes its
// kernel from here.  k_quotient_eval's parameters are the first eleven of k_quotient_eval2's, so one argument list serves both.
static const struct { int kernel; bool rec, full, acc_mem; const void* fn; } Q_KERNELS[] = {
    {1, false, true, false, (const void*)k_quotient_eval<true, false>},        {1, false, false, false, (const void*)k_quotient_eval<false, false>},
    {1, false, true, true, (const void*)k_quotient_eval<true, true>},          {1, false, false, true, (const void*)k_quotient_eval<false, true>},
    {2, false, true, false, (const void*)k_quotient_eval2<true, false, false>}, {2, false, false, false, (const void*)k_quotient_eval2<false, false, false>},
    {2, false, true, true, (const void*)k_quotient_eval2<true, true, false>},   {2, false, false, true, (const void*)k_quotient_eval2<false, true, false>},
    {2, true, true, false, (const void*)k_quotient_eval2<true, false, true>},   {2, true, false, false, (const void*)k_quotient_eval2<false, false, true>},
    {2, true, true, true, (const void*)k_quotient_eval2<true, true, true>},     {2, true, false, true, (const void*)k_quotient_eval2<false, true, true>},
};

int zk::quotient_eval_fmt(zk_ctx* ctx, const uint32_t* h_program, uint32_t num_instr, const void* const* h_col_ptrs, uint32_t num_cols, const void* h_consts, uint32_t num_consts, uint32_t k,
                          uint32_t ext_k, int divide_by_vanishing, void* d_out, bool records) {
    ZK_REQUIRE(ctx, h_program && d_out && (h_col_ptrs || !num_cols) && (h_consts || !num_consts), "null pointer");
    ZK_REQUIRE(ctx, k <= ext_k && ext_k <= 28, "need k <= ext_k <= 28");
    QuotientLaunch q;
    {
        std::string err;
        const int rc = plan_quotient_launch(h_program, num_instr, num_cols, num_consts, ext_k, records, QuotientEvalKnobs::read(), &q, &err);
        if (rc) return ctx->fail(rc, "%s", err.c_str());
    }
    const uint64_t ne = 1ull << ext_k;
    const uint32_t S = q.S, nc_all = num_consts + (q.sliced ? S : 0);
    const size_t tmp_row_bytes = records ? REC29_BYTES : sizeof(Fr);         // a parked intermediate is read back as a column: it has the columns' format
    Fr* d_tmp = nullptr;
    if (q.num_tmp) {
        d_tmp = (Fr*)ctx->get_scratch(SC_QTMP, ((size_t)q.num_tmp << ext_k) * tmp_row_bytes);
        if (!d_tmp) return ZK_ERR_OOM;
    }
    uint32_t* d_acc = nullptr;
    if (q.acc_in_mem) {
        d_acc = (uint32_t*)ctx->get_scratch(SC_QACC, ((size_t)9 << ext_k) * sizeof(uint32_t));
        if (!d_acc) return ZK_ERR_OOM;
    }
    Fr* d_part = nullptr;                     // sliced: the slices' sums, [slice][row]
    if (q.sliced) {
        d_part = (Fr*)ctx->get_scratch(SC_QSLICE, ((size_t)S << ext_k) * sizeof(Fr));
        if (!d_part) return ZK_ERR_OOM;
    }
    std::vector<Fr> tev;
    if (divide_by_vanishing) vanishing_inverses(k, ext_k, &tev);
    // constants that multiply (MUL_CONST, FOLD) and the vanishing inverses go to the device in R' = 2^261 form too: x 32
    auto times32 = [](Fr x) { for (int j = 0; j < 5; ++j) x = dbl(x); return x; };
    std::vector<Fr> consts_r((const Fr*)h_consts, (const Fr*)h_consts + num_consts);
    for (const std::vector<uint32_t>& folds : q.slice_folds) {      // constants num_consts + s: what the accumulator coming into slice s is multiplied by, the product of its fold constants
        Fr prod = Fr::one();
        for (uint32_t j : folds) prod = prod * ((const Fr*)h_consts)[j];
        consts_r.push_back(prod);
    }
    std::vector<Fr> consts_rp(consts_r);
    for (Fr& c : consts_rp) c = times32(c);
    for (Fr& t : tev) t = times32(t);
    // column table = the caller's columns, then one pseudo-column per parked intermediate, then (sliced) the slices' sums
    std::vector<const void*> col_tab(h_col_ptrs, h_col_ptrs + num_cols);
    for (uint32_t t = 0; t < q.num_tmp; ++t) col_tab.push_back((const char*)d_tmp + ((size_t)t << ext_k) * tmp_row_bytes);
    if (q.sliced) for (uint32_t sl = 0; sl < S; ++sl) col_tab.push_back(d_part + ((size_t)sl << ext_k));
    const size_t tev_bytes = tev.size() * sizeof(Fr);
    auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
    const size_t cols_at = al(q.prog_bytes), consts_at = cols_at + al(q.col_bytes), tev_at = consts_at + al(q.const_bytes), total_bytes = tev_at + al(tev_bytes);
    char* d = (char*)ctx->get_scratch(SC_POLY, total_bytes + 256);
    if (!d) return ZK_ERR_OOM;
    const uint32_t* d_prog = (const uint32_t*)d;
    const Fr* const* d_cols = (const Fr* const*)(d + cols_at);
    const QC29* d_consts = (const QC29*)(d + consts_at);
    // program, column table, constants (R and R' forms) and vanishing inverses travel as ONE upload: the proof makes hundreds of
    // these calls (compressions, linear combinations, class programs), and five small copies each were 2 500 copies per
    // SuperCircuit-shape proof at ~8 us of device time apiece
    std::vector<char> staging(total_bytes, 0);
    memcpy(staging.data(), q.words.data(), q.prog_bytes);
    if (!col_tab.empty()) memcpy(staging.data() + cols_at, col_tab.data(), col_tab.size() * 8);
    QC29* hq = (QC29*)(staging.data() + consts_at);         // limb form: the R-form constants, then their R' images
    for (uint32_t j = 0; j < nc_all; ++j) {
        const Q29 a = unpack29<Fr29P>(consts_r[j]), b = unpack29<Fr29P>(consts_rp[j]);
        for (int l = 0; l < 9; ++l) { hq[j].l[l] = a.l[l]; hq[nc_all + j].l[l] = b.l[l]; }
    }
    if (!tev.empty()) memcpy(staging.data() + tev_at, tev.data(), tev_bytes);
    ZK_HIP(ctx, hipMemcpyAsync(d, staging.data(), total_bytes, hipMemcpyHostToDevice, ctx->stream));
    ZK_HIP(ctx, hipStreamSynchronize(ctx->stream));   // staging vectors are stack-owned
    if (!ctx->quotient_attr_set) {
        for (const auto& kn : Q_KERNELS) ZK_HIP(ctx, hipFuncSetAttribute(kn.fn, hipFuncAttributeMaxDynamicSharedMemorySize, Q_MAX_STACK * 9 * Q_THREADS * 4));
        ctx->quotient_attr_set = true;
    }
    ZkProfScope ps(ctx, ctx->prof_tag ? ctx->prof_tag : "quotient_eval");
    if (ctx->prof_on) {
        // algorithmic bytes of this launch: every distinct (column, rotation) operand is read once per row, parked
        // intermediates are written and read back once each, one result per row is written
        std::vector<uint64_t> ops;
        uint64_t tmp_moves = 0;
        for (uint32_t i = 0; i < num_instr; ++i) {
            const uint32_t op = h_program[3 * i];
            if (op == Q_PUSH_COL) ops.push_back(((uint64_t)h_program[3 * i + 1] << 32) | h_program[3 * i + 2]);
            else if (op == Q_TEE_TMP || op == Q_PUSH_TMP) ++tmp_moves;
        }
        std::sort(ops.begin(), ops.end());
        ops.erase(std::unique(ops.begin(), ops.end()), ops.end());
        ps.bytes = (ops.size() + tmp_moves + 1) * ne * 32;
    }
    const Fr* d_tev = tev.empty() ? nullptr : (const Fr*)(d + tev_at);
    const dim3 tiles((unsigned)((ne + Q_THREADS - 1) / Q_THREADS)), block(Q_THREADS);
    {
        // a sliced launch leaves the slices' sums in d_part and the vanishing division to the combining program
        uint32_t prog_len = q.low_len + 1, k_ = k, ext_k_ = ext_k, tile_alias = q.tile_alias, num_slices = q.sliced ? S : 0u;
        const QC29* d_consts_rp = d_consts + nc_all;
        const Fr* t_evals = q.sliced ? nullptr : d_tev;
        Fr* out = q.sliced ? d_part : (Fr*)d_out;
        const uint32_t* d_slice_tab = d_prog + q.slice_tab_at;
        void* args[] = {&d_prog, &prog_len, &d_cols, &d_consts, &d_consts_rp, &t_evals, &ext_k_, &k_, &out, &d_tmp, &d_acc, &tile_alias, &d_slice_tab, &num_slices};
        const void* fn = nullptr;
        for (const auto& kn : Q_KERNELS) if (kn.kernel == q.kernel && kn.rec == q.records && kn.full == q.full && kn.acc_mem == q.acc_in_mem) fn = kn.fn;
        ZK_HIP(ctx, hipLaunchKernel(fn, dim3(tiles.x * S), block, args, q.lds, ctx->stream));
    }
    ZK_CHECK_LAUNCH(ctx);
    if (q.sliced) {                 // the slices' sums are packed elements whatever the operands were: this launch reads forty-odd of them per row
        hipLaunchKernelGGL((k_quotient_eval2<true, false, false>), tiles, block, (size_t)9 * Q_THREADS * 4, ctx->stream, d_prog + q.comb_at, S + 1, d_cols, d_consts,
                           d_consts + nc_all, d_tev, ext_k, k, (Fr*)d_out, d_tmp, (uint32_t*)nullptr, 0u, (const uint32_t*)nullptr, 0u);
        ZK_CHECK_LAUNCH(ctx);
    }
    return ZK_OK;
}

namespace zk { __global__ void k_powers(Fr base, Fr mul, Fr* out, uint32_t count, int rprime); }

extern "C" int zk_fr_powers(zk_ctx* ctx, const void* h_base, const void* h_mul, void* d_out, size_t n) {
    if (!ctx) return ZK_ERR_INVALID_ARG;
    ZK_REQUIRE(ctx, h_base && h_mul && d_out, "null pointer");
    return zk::fr_powers_fmt(ctx, *(const Fr*)h_base, *(const Fr*)h_mul, d_out, n, false);
}
// records: d_out (REC29_BYTES per row) receives 32 x the powers as a coset record buffer of n rows
int zk::fr_powers_fmt(zk_ctx* ctx, const Fr& base, const Fr& mul, void* d_out, size_t n, bool records) {
    ZK_REQUIRE(ctx, n <= (1ull << 28), "too many powers");
    ZK_REQUIRE(ctx, !records || (n & 3) == 0, "a record buffer has a multiple of four rows");
    if (!n) return ZK_OK;
    hipLaunchKernelGGL(zk::k_powers, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, base, mul, (Fr*)d_out, (uint32_t)n, records ? 2 : 0);
    ZK_CHECK_LAUNCH(ctx);
    return ZK_OK;
}

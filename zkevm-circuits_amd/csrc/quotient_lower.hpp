// The quotient evaluator's host side (quotient.hip has the kernels): the lowered instruction set, the lowering of a caller's postfix program
// (lower_fuse, lower_bounds), the slicer (plan_slices), the program check, the knobs (QuotientEvalKnobs) and the launch plan
// (plan_quotient_launch) -- what a launch of a program looks like, as a function of the program words, the counts of columns and constants,
// the domain size, the operand format and the knobs.  Host only: no HIP, no context, no field arithmetic; a C++17 compiler takes it alone.
// quotient.hip follows the plan, quotient_plan.hip counts fused steps with the lowering, zk_host_quotient_launch shows the plan.
//
// Bounds (V = value bound in units of p, L = limb bound in units of 2^29; settled = (2, 1); a column,
// constant or parked intermediate is canonical = (1, 1)):
//   mul29(a, b)    needs b normalised, limbs of a < 2^31.2 (L <= 4), a * b < 2^261 p  (V_a V_b < 168);
//                  result (2, 1).  b = 32 x (a canonical operand): V_a <= 5;  b = 32 x (settled): V_a V_b <= 5.
//   add29          (V_a + V_b, L_a + L_b), kept <= (4, 4) so that the value can always be settled
//   a - b          = a + K p (balanced limbs) - b with b normalised and below K p: (V_a + K, L_a + 2),
//                  K = 1 for canonical b, 2 for settled b
//   FOLD           acc = mul29(acc, y) + t: acc is only ever the first operand of a product by a
//                  constant, so it is never settled: L_t <= 3
//   MAC_COL        t0 * 32 m + S c' under one reduction: 32 V_t0 + V_S <= 168 < 2^261 / p = 169.3 (V_t0 <= 5, V_S <= 8); a column
//                  holds 18 limb products + 9 of the reduction, below 9 (L_t0 + L_S + 1) 2^58 + 2^35 < 2^64 for L_t0 + L_S <= 6
//   MAC2_COL       t0 * 32 m2 + X * 32 m1 + S c' (t0 = Y): 32 (V_X + V_Y) + V_S <= 168 needs V_X + V_Y <= 5; 27 limb products + 9 a
//                  column, below 9 (L_X + L_Y + L_S + 1) 2^58 + 2^35 < 2^64 for L_X + L_Y + L_S <= 6.  X and S are in LDS by then: X is
//                  brought to V <= 3, L_X + L_S <= 5 by requests on the PUSH_COL32 that spills it, Y by MAC2_COL's own (lower_bounds)
//   MAC_STK        B * 32 t0 + S c' (t0 settled, B popped into registers): V_B V_t0 <= 5 as for MUL, L_B + L_S <= 6
//   No request is ever made for an entry that is in LDS when the instruction runs: the kernel has no step for it.
#pragma once
#include <algorithm>
#include <climits>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <unordered_map>
#include <vector>

#include "cs.hpp"

namespace zk {

// the caller's opcodes (cs.hpp)
using cs::Q_END; using cs::Q_PUSH_COL; using cs::Q_PUSH_CONST; using cs::Q_ADD; using cs::Q_SUB; using cs::Q_MUL; using cs::Q_NEG; using cs::Q_SQUARE; using cs::Q_DOUBLE;
using cs::Q_FOLD; using cs::Q_MUL_CONST; using cs::Q_ADD_CONST; using cs::Q_TEE_TMP; using cs::Q_PUSH_TMP;
// statuses of the functions below: the values of ZK_OK, ZK_ERR_INVALID_ARG and ZK_ERR_UNSUPPORTED (include/zkmi355.h; quotient.hip asserts it)
constexpr int QL_OK = 0, QL_INVALID_ARG = -1, QL_UNSUPPORTED = -5;
constexpr size_t Q_REC_ROW_BYTES = 36;      // a row of a coset record buffer: REC29_BYTES of ff29.hip.hpp, which owns it (quotient.hip asserts it)
constexpr size_t Q_ROW_BYTES = 32;          // a packed field element
constexpr size_t Q_CONST_BYTES = 64;        // a program constant as the kernels read it (QC29 of quotient.hip)

enum KOp : uint32_t { // produced by the lowering only (never part of a caller's program): the second operand comes from memory
                      K_ADD_COL = 16, K_SUB_COL = 17, K_RSUB_COL = 18, K_MUL_COL = 19, K_FOLD_COL = 20, K_NOP = 21,
                      // t0 <- t0 * 32 mem + st[sp - 2] * const, pop (the constant index in word 0 above K_CONST_SHIFT, as K_FOLD_COL): a Horner step
                      // S y^gap + X mem in one reduction (lower_fuse with mac; k_quotient_eval2 only)
                      K_MAC_COL = 22,
                      // Sums of two column products under one reduction (lower_fuse with mac2; k_quotient_eval2 only).  The stream of such a term is
                      //   <S> <X> PUSH_COL32 m1 <Y> MAC2_COL(m2, const):  t0 <- t0 * 32 m2 + st[sp - 3] * st[sp - 2] + st[sp - 4] * const, three entries popped
                      // (t0 = Y, st[sp - 2] = 32 m1 as PUSH_COL32 left it, st[sp - 3] = X, st[sp - 4] = S): one memory operand per instruction, m1 travels over
                      // the stack.  PUSH_COL32 pushes 32 x its memory operand; ITS settle / carry bits (bit 0 forms only) act on the entry it spills, X.
                      K_PUSH_COL32 = 23, K_MAC2_COL = 24,
                      // t0 <- st[sp - 2] * 32 t0 + st[sp - 3] * const, two entries popped: a Horner step over a stack product, S y^gap + U V
                      K_MAC_STK = 25 };
constexpr uint32_t K_SETTLE0 = 0x100, K_SETTLE1 = 0x200;      // word 0 of a lowered instruction: settle t0 / t1 before executing
constexpr uint32_t K_NORM0 = 0x400, K_NORM1 = 0x800;          // ... or only propagate its carries (limbs back below 2^29, value unchanged): a third of a settle
constexpr uint32_t K_SETTLE0_8 = 0x1000, K_SETTLE1_8 = 0x2000; // ... or settle a value that may have reached 8p (q_settle8)
constexpr int K_CONST_SHIFT = 16;                              // K_FOLD_COL keeps its constant index in the bits above
#ifndef Q_THREADS_N
#define Q_THREADS_N 256
#endif
constexpr int Q_THREADS = Q_THREADS_N;      // lanes per workgroup (no cooperation between waves: the size only sets the granularity of the LDS allocation)
// how many instructions ahead of its use a memory operand is requested (1: while the previous instruction computes; 2: one more)
#ifndef Q_PREFETCH_DIST
#define Q_PREFETCH_DIST 1
#endif
constexpr int Q_MAX_STACK = 16;
constexpr uint32_t Q_MAX_TMP = 4096;     // intermediates live in HBM, [slot][row]: 32 MiB per slot at 2^20 rows
constexpr bool k_has_mem(uint32_t w0) {      // the instruction has a memory operand (constexpr: the kernels and the host share it)
    const uint32_t o = w0 & 0xffu;
    return o == Q_PUSH_COL || (o >= K_ADD_COL && o <= K_FOLD_COL) || o == K_MAC_COL || o == K_PUSH_COL32 || o == K_MAC2_COL;
}
constexpr uint32_t K_FIRST_FOLD = 0x4000;    // word 0 of the first fold of a program: the accumulator is zero there, nothing is read
// What an instruction does, as one bit per step of the interpreter's loop body (word 3 of the 4-word instructions k_quotient_eval2 reads; made by
// q_class_mask on the host).  The loop body is a flat sequence of `if (mask & bit) { step }`: every step updates its registers in place and the
// only joins are those of single-armed ifs, which the register coalescer resolves without copies -- a `switch (op)` does not survive the
// compiler (cases merged and re-split around shared tails, phi copies of the whole top-of-stack at every join), and tests on separate bits of a
// word cannot be threaded into one another the way comparisons of one opcode are.
enum QClass : uint32_t {
    C_SPILL = 1u << 0,       // make room on top: PUSH_COL, PUSH_CONST
    C_UNPACK_T = 1u << 1,    // t0 <- memory operand                       PUSH_COL
    C_UNPACK_B = 1u << 2,    // B <- memory operand                        ADD_COL SUB_COL RSUB_COL FOLD_COL
    C_UNPACK_B32 = 1u << 3,  // B <- 32 x memory operand                   MUL_COL
    C_POP_B = 1u << 4,       // B <- the entry below the top               ADD SUB MUL
    C_HASMEM = 1u << 5,      // the instruction has a memory operand (tested on the NEXT instruction: its load is issued one instruction early)
    C_FLAGS = 1u << 6,       // any settle / carry-propagation request in word 0
    C_MULV = 1u << 7,        // t0 <- t0 * B                               MUL_COL
    C_MULC = 1u << 8,        // t0 <- t0 * const                           MUL_CONST
    C_ADDV = 1u << 9,        // t0 <- t0 + B                               ADD ADD_COL
    C_SUBV = 1u << 10,       // t0 <- t0 - B                               SUB_COL
    C_FOLDC = 1u << 11,      // acc <- acc * const + B                     FOLD_COL
    C_RARE = 1u << 12,       // any of the steps below
    C_PUSHC = 1u << 13,      // t0 <- const                                PUSH_CONST
    C_ADDC = 1u << 14,       // t0 <- t0 + const                           ADD_CONST
    C_RSUB = 1u << 15,       // t0 <- B - t0                               SUB RSUB_COL
    C_MULS = 1u << 16,       // t0 <- B * t0 (stack product)               MUL
    C_NEG = 1u << 17, C_SQ = 1u << 18, C_DBL = 1u << 19, C_TEE = 1u << 20,
    C_FOLD = 1u << 21,       // acc <- acc * const + t0, pop               FOLD
    C_MACC = 1u << 22,       // t0 <- t0 * B + (entry below) * const, pop  MAC_COL
    C_UNPACK_T32 = 1u << 23, // spill (word 0's flags on the spilled entry), t0 <- 32 x memory operand     PUSH_COL32
    C_MAC2 = 1u << 24,       // t0 <- t0 * B + X * m1 + S * const, pop 3   MAC2_COL
    C_MACS = 1u << 25,       // t0 <- B * 32 t0 + S * const, pop (B popped by C_POP_B)   MAC_STK (under C_RARE)
    // record mode only: a sum or difference takes its memory operand from the registers it arrived in, before the load of the next
    // instruction is issued into them (no copy into B: nine v_mov for nine additions)
    C_ADDM = 1u << 26,       // t0 <- t0 + memory operand                  ADD_COL
    C_SUBM = 1u << 27,       // t0 <- t0 - memory operand                  SUB_COL
};
inline uint32_t q_class_mask(uint32_t w0, bool records = false) {
    uint32_t m = 0;
    if (records && ((w0 & 0xffu) == K_ADD_COL || (w0 & 0xffu) == K_SUB_COL)) {
        m = C_HASMEM | ((w0 & 0xffu) == K_ADD_COL ? C_ADDM : C_SUBM);
        if (w0 & (K_SETTLE0 | K_SETTLE1 | K_NORM0 | K_NORM1 | K_SETTLE0_8 | K_SETTLE1_8)) m |= C_FLAGS;
        return m;
    }
    switch (w0 & 0xffu) {
        case Q_PUSH_COL: m = C_SPILL | C_UNPACK_T | C_HASMEM; break;
        case Q_PUSH_CONST: m = C_SPILL | C_RARE | C_PUSHC; break;
        case Q_ADD: m = C_POP_B | C_ADDV; break;
        case Q_SUB: m = C_POP_B | C_RARE | C_RSUB; break;
        case Q_MUL: m = C_POP_B | C_RARE | C_MULS; break;
        case Q_NEG: m = C_RARE | C_NEG; break;
        case Q_SQUARE: m = C_RARE | C_SQ; break;
        case Q_DOUBLE: m = C_RARE | C_DBL; break;
        case Q_FOLD: m = C_RARE | C_FOLD; break;
        case Q_MUL_CONST: m = C_MULC; break;
        case Q_ADD_CONST: m = C_RARE | C_ADDC; break;
        case Q_TEE_TMP: m = C_RARE | C_TEE; break;
        case K_ADD_COL: m = C_UNPACK_B | C_HASMEM | C_ADDV; break;
        case K_SUB_COL: m = C_UNPACK_B | C_HASMEM | C_SUBV; break;
        case K_RSUB_COL: m = C_UNPACK_B | C_HASMEM | C_RARE | C_RSUB; break;
        case K_MUL_COL: m = C_UNPACK_B32 | C_HASMEM | C_MULV; break;
        case K_FOLD_COL: m = C_UNPACK_B | C_HASMEM | C_FOLDC; break;
        case K_MAC_COL: m = C_UNPACK_B32 | C_HASMEM | C_MACC; break;
        case K_PUSH_COL32: return C_UNPACK_T32 | C_HASMEM;       // its flags are X's: handled where X is spilled, not by the C_FLAGS step
        case K_MAC2_COL: m = C_UNPACK_B32 | C_HASMEM | C_MAC2; break;
        case K_MAC_STK: m = C_POP_B | C_RARE | C_MACS; break;
        default: break;            // K_NOP, Q_END
    }
    if (w0 & (K_SETTLE0 | K_SETTLE1 | K_NORM0 | K_NORM1 | K_SETTLE0_8 | K_SETTLE1_8)) m |= C_FLAGS;
    return m;
}
// ---- lowering: caller's postfix program -> the kernel's instruction stream -------------------------------------
struct LNode {
    enum Kind : uint8_t { MEM, CONST, UN, BIN, CONSTOP, TEE, MAT } kind;
    bool has_tee;           // the subtree parks an intermediate (evaluation order then matters for readers of that slot)
    bool is_tmp;            // MEM: a parked intermediate read back
    uint32_t op, a, b;      // UN / BIN / CONSTOP: opcode; MEM: column, rotation; CONST / CONSTOP: constant; TEE: slot
    int32_t x, y;
};
struct LowInstr { uint32_t w0, a, b; };

// expression trees of the program, re-emitted with memory operands (see the header comment).
// mac (k_quotient_eval2 only): a Horner step of a compiled class program, (S MUL_CONST c) + T with T = X * mem followed by a chain of sums with
// memory / constant operands (T = X * m - n, the regrouped `sel * expr`, ...), is re-associated into  K_MAC_COL(m, c)  (t0 = X * m + S * c, ONE
// reduction for both products) followed by T's chain: every operand is read in the order it was, only the product by c moves.
// mac2 (with mac): where T's chain ends in a SUM OF TWO products by memory operands, X * m1 + Y * m2, the step becomes
//   S, X, PUSH_COL32 m1, Y, MAC2_COL(m2, c)   (three products, one reduction; operands read in the order they were),
// and where it ends in a product of two computed values, U * V:  S, U, V, MAC_STK(c)  (two products, one reduction).  MAC2_COL holds one entry
// more on the stack while Y is computed than the unfused stream does.  The LDS stack caps the waves per SIMD of a class launch, so a fusion
// that would take the program deeper than its mac-only stream goes is declined (first tried with the two products swapped, where no parked
// intermediate pins the order); *declined counts them.
inline void lower_fuse(const uint32_t* prog, uint32_t len, uint32_t num_cols, std::vector<LowInstr>* out, bool mac = false, bool mac2 = false, uint32_t* declined = nullptr) {
    std::vector<LNode> nodes;
    nodes.reserve(len);
    std::vector<int32_t> st;
    auto leafish = [&](int32_t n) { return nodes[n].kind == LNode::MEM || nodes[n].kind == LNode::CONST; };
    // per node: du = entries the mac-only emission of the subtree holds at its peak, above those there when it starts; net = by how many the
    // stack has grown when it is done (1, less the already materialised entries it consumes).  Children precede parents, so one pass makes them.
    std::vector<int16_t> du, net;
    du.reserve(len); net.reserve(len);
    auto plan_of = [&](const LNode& n) {         // bin_plan below, needed here first
        const LNode &x = nodes[n.x], &y = nodes[n.y];
        if (y.kind == LNode::MEM) return 1;
        if (y.kind == LNode::CONST && (n.op == Q_ADD || n.op == Q_MUL)) return 2;
        if (x.kind == LNode::MEM && !leafish(n.y) && !(x.is_tmp && y.has_tee)) return 3;
        if (x.kind == LNode::CONST && !leafish(n.y) && (n.op == Q_ADD || n.op == Q_MUL)) return 4;
        return 0;
    };
    auto add = [&](LNode n) {
        int d = 0, g = 0;
        switch (n.kind) {
            case LNode::MAT: break;
            case LNode::MEM: case LNode::CONST: d = 1; g = 1; break;
            case LNode::UN: case LNode::CONSTOP: case LNode::TEE: d = du[n.x]; g = net[n.x]; break;
            case LNode::BIN: {
                const int plan = plan_of(n);
                if (plan == 0) { d = std::max<int>(du[n.x], net[n.x] + du[n.y]); g = net[n.x] + net[n.y] - 1; }
                else if (plan == 1 || plan == 2) { d = du[n.x]; g = net[n.x]; }
                else { d = du[n.y]; g = net[n.y]; }
                break;
            }
        }
        nodes.push_back(n); du.push_back((int16_t)d); net.push_back((int16_t)g);
        return (int32_t)nodes.size() - 1;
    };
    struct Work { int32_t node; int plan; LowInstr raw; };        // plan 5: emit `raw` as it stands
    std::vector<Work> work;
    // plans of a BIN node after its operands: 0 = stack op, 1 = y from memory, 2 = y constant, 3 = x from memory (operands swapped), 4 = x constant (swapped)
    auto bin_plan = [&](const LNode& n) { return plan_of(n); };
    // mac: T = X * mem under a chain of sums with a memory / constant operand, emitted the way the plans above emit it -> X, the product's
    // memory operand, the chain's instructions innermost last
    std::vector<LowInstr> chain;
    // a product by a memory operand: the other factor, the operand
    auto mul_mem = [&](int32_t t, int32_t* xo, LowInstr* mo) -> bool {
        const LNode& n = nodes[t];
        if (n.kind != LNode::BIN || n.op != Q_MUL) return false;
        const int plan = bin_plan(n);
        if (plan == 1) { *xo = n.x; *mo = {0, nodes[n.y].a, nodes[n.y].b}; return true; }
        if (plan == 3) { *xo = n.y; *mo = {0, nodes[n.x].a, nodes[n.x].b}; return true; }
        return false;
    };
    int32_t yo2 = -1;             // mac_shape's second outputs: MAC2_COL's Y and m2, MAC_STK's V
    LowInstr mo2{};
    uint32_t cur_depth = 0;       // stack entries of the stream emitted so far (kept by depth_now)
    size_t counted = out->size();
    int limit = 0;                // mac2: the mac-only stream's depth
    auto depth_now = [&]() {
        for (; counted < out->size(); ++counted) {
            const uint32_t o = (*out)[counted].w0 & 0xffu;
            if (o == Q_PUSH_COL || o == Q_PUSH_CONST || o == K_PUSH_COL32) ++cur_depth;
            else if (o == Q_ADD || o == Q_SUB || o == Q_MUL || o == Q_FOLD || o == K_MAC_COL) --cur_depth;
            else if (o == K_MAC_STK) cur_depth -= 2;
            else if (o == K_MAC2_COL) cur_depth -= 3;
        }
        return (int)cur_depth;
    };
    // walks down a chain of sums with a memory / constant operand (pushed on `ch`, outermost first, as the plans above emit them); returns the node under it
    auto walk = [&](int32_t t, std::vector<LowInstr>& ch) -> int32_t {
        for (int guard = 0; guard < 64; ++guard) {
            const LNode& n = nodes[t];
            if (n.kind == LNode::CONSTOP && n.op == Q_ADD_CONST) { ch.push_back({Q_ADD_CONST, n.a, 0}); t = n.x; continue; }
            if (n.kind != LNode::BIN) return t;
            const int plan = bin_plan(n);
            const LNode &x = nodes[n.x], &y = nodes[n.y];
            if (n.op == Q_SUB && plan == 1) { ch.push_back({K_SUB_COL, y.a, y.b}); t = n.x; continue; }
            if (n.op != Q_ADD) return t;
            if (plan == 1) { ch.push_back({K_ADD_COL, y.a, y.b}); t = n.x; }
            else if (plan == 2) { ch.push_back({Q_ADD_CONST, y.a, 0}); t = n.x; }
            else if (plan == 3) { ch.push_back({K_ADD_COL, x.a, x.b}); t = n.y; }
            else if (plan == 4) { ch.push_back({Q_ADD_CONST, x.a, 0}); t = n.y; }
            else return t;
        }
        return -1;
    };
    std::vector<LowInstr> chain_a, chain_b, chain_in;      // chain_in: shape 4's sums right behind its MAC_COL
    int32_t z_node = -1;                                    // shape 4's other addend
    // returns 0: no fusable shape, 1: MAC_COL (xo, mo), 2: MAC2_COL (xo, mo = X, m1; yo2, mo2 = Y, m2), 3: MAC_STK (xo, yo2 = U, V),
    // 4 (mac2): T = (X * m [sums]) + Z with any Z, run as  S, X, MAC_COL(m, c), [sums], Z, ADD  -- what a sum of two column products falls back to
    // when MAC2_COL would deepen the stack, and what serves when only one addend is a product by memory: one reduction fewer, never deeper
    auto mac_shape = [&](int32_t t, int32_t s_node, int32_t* xo, LowInstr* mo) -> int {
        chain.clear();
        t = walk(t, chain);
        if (t < 0 || nodes[t].kind != LNode::BIN) return 0;
        const LNode& n = nodes[t];
        const int plan = bin_plan(n);
        const LNode &x = nodes[n.x], &y = nodes[n.y];
        if (n.op == Q_MUL) {
            if (plan == 1) { *xo = n.x; *mo = {K_MAC_COL, y.a, y.b}; return 1; }
            if (plan == 3) { *xo = n.y; *mo = {K_MAC_COL, x.a, x.b}; return 1; }
            if (plan == 0 && mac2) { *xo = n.x; yo2 = n.y; return 3; }          // same depth as S MUL_CONST, U, V, MUL, ADD
            return 0;
        }
        if (n.op != Q_ADD || plan != 0 || !mac2) return 0;
        chain_a.clear(); chain_b.clear();
        int32_t xa = -1, xb = -1;
        LowInstr ma{}, mb{};
        const int32_t ta = walk(n.x, chain_a), tb = walk(n.y, chain_b);
        const bool ok_a = ta >= 0 && mul_mem(ta, &xa, &ma), ok_b = tb >= 0 && mul_mem(tb, &xb, &mb);
        const bool free_order = !x.has_tee && !y.has_tee;          // no parked intermediate pins the order of the two addends' reads
        if (ok_a && ok_b && (chain_a.empty() || free_order)) {
            // Y is computed on top of S, X and 32 m1
            const int base = depth_now() + net[s_node];
            const bool fits = base + net[xa] + 1 + du[xb] <= limit;
            const bool swapped = !fits && free_order && base + net[xb] + 1 + du[xa] <= limit;
            if (fits || swapped) {
                if (fits) { *xo = xa; *mo = ma; yo2 = xb; mo2 = mb; }
                else { *xo = xb; *mo = mb; yo2 = xa; mo2 = ma; }
                chain.insert(chain.end(), chain_b.begin(), chain_b.end());       // all the sums run behind the product, the inner ones first
                chain.insert(chain.end(), chain_a.begin(), chain_a.end());
                return 2;
            }
            if (declined) ++*declined;
        }
        if (ok_a) { *xo = xa; *mo = {K_MAC_COL, ma.a, ma.b}; chain_in = chain_a; z_node = n.y; return 4; }
        if (ok_b && free_order) { *xo = xb; *mo = {K_MAC_COL, mb.a, mb.b}; chain_in = chain_b; z_node = n.x; return 4; }
        return 0;
    };
    auto emit = [&](int32_t root) {
        work.push_back({root, -1, {}});
        while (!work.empty()) {
            const Work wk = work.back();
            work.pop_back();
            if (wk.plan == 5) { out->push_back(wk.raw); continue; }
            const LNode& n = nodes[wk.node];
            switch (n.kind) {
                case LNode::MAT: break;
                case LNode::MEM: out->push_back({Q_PUSH_COL, n.a, n.b}); break;
                case LNode::CONST: out->push_back({Q_PUSH_CONST, n.a, 0}); break;
                case LNode::UN:
                    if (wk.plan < 0) { work.push_back({wk.node, 0}); work.push_back({n.x, -1}); }
                    else out->push_back({n.op, 0, 0});
                    break;
                case LNode::CONSTOP:
                    if (wk.plan < 0) { work.push_back({wk.node, 0}); work.push_back({n.x, -1}); }
                    else out->push_back({n.op, n.a, 0});
                    break;
                case LNode::TEE:
                    if (wk.plan < 0) { work.push_back({wk.node, 0}); work.push_back({n.x, -1}); }
                    else out->push_back({Q_TEE_TMP, n.a, 0});
                    break;
                case LNode::BIN: {
                    const LNode &x = nodes[n.x], &y = nodes[n.y];
                    if (wk.plan < 0) {
                        int32_t xm = -1;
                        LowInstr mi{};
                        const int shape = mac && n.op == Q_ADD && x.kind == LNode::CONSTOP && x.op == Q_MUL_CONST && x.a < (1u << (32 - K_CONST_SHIFT)) ? mac_shape(n.y, x.x, &xm, &mi) : 0;
                        if (shape) {
                            // S, X, MAC_COL(m, c), the chain: pushed in reverse
                            for (const LowInstr& c : chain) work.push_back({-1, 5, c});
                            if (shape == 1) {
                                work.push_back({-1, 5, {mi.w0 | (x.a << K_CONST_SHIFT), mi.a, mi.b}});
                                work.push_back({xm, -1, {}});
                            } else if (shape == 4) {      // S, X, MAC_COL(m, c), its sums, Z, ADD
                                work.push_back({-1, 5, {Q_ADD, 0, 0}});
                                work.push_back({z_node, -1, {}});
                                for (const LowInstr& c : chain_in) work.push_back({-1, 5, c});
                                work.push_back({-1, 5, {mi.w0 | (x.a << K_CONST_SHIFT), mi.a, mi.b}});
                                work.push_back({xm, -1, {}});
                            } else if (shape == 2) {      // S, X, PUSH_COL32 m1, Y, MAC2_COL(m2, c)
                                work.push_back({-1, 5, {K_MAC2_COL | (x.a << K_CONST_SHIFT), mo2.a, mo2.b}});
                                work.push_back({yo2, -1, {}});
                                work.push_back({-1, 5, {K_PUSH_COL32, mi.a, mi.b}});
                                work.push_back({xm, -1, {}});
                            } else {                      // S, U, V, MAC_STK(c)
                                work.push_back({-1, 5, {K_MAC_STK | (x.a << K_CONST_SHIFT), 0, 0}});
                                work.push_back({yo2, -1, {}});
                                work.push_back({xm, -1, {}});
                            }
                            work.push_back({x.x, -1, {}});
                            break;
                        }
                        const int plan = bin_plan(n);
                        work.push_back({wk.node, plan});
                        if (plan == 0) { work.push_back({n.y, -1}); work.push_back({n.x, -1}); }
                        else if (plan == 1 || plan == 2) work.push_back({n.x, -1});
                        else work.push_back({n.y, -1});
                    } else if (wk.plan == 0) out->push_back({n.op, 0, 0});
                    else if (wk.plan == 1) out->push_back({n.op == Q_ADD ? K_ADD_COL : n.op == Q_SUB ? K_SUB_COL : K_MUL_COL, y.a, y.b});
                    else if (wk.plan == 2) out->push_back({n.op == Q_ADD ? Q_ADD_CONST : Q_MUL_CONST, y.a, 0});
                    else if (wk.plan == 3) out->push_back({n.op == Q_ADD ? K_ADD_COL : n.op == Q_SUB ? K_RSUB_COL : K_MUL_COL, x.a, x.b});
                    else out->push_back({n.op == Q_ADD ? Q_ADD_CONST : Q_MUL_CONST, x.a, 0});
                    break;
                }
            }
        }
    };
    // the statements in order: an expression to emit (node >= 0) or an instruction as it stands.  Kept until the whole program is read: the
    // depth the mac-only stream reaches (the limit of mac2's fusions) is known only then.
    struct Ev { int32_t node; LowInstr raw; };
    std::vector<Ev> evs;
    auto materialise_pending = [&]() {
        for (int32_t& e : st)
            if (nodes[e].kind != LNode::MAT) { evs.push_back({e, {}}); e = add({LNode::MAT, false, false, 0, 0, 0, -1, -1}); }
    };
    for (uint32_t pc = 0; pc < len; ++pc) {
        const uint32_t op = prog[3 * pc], a = prog[3 * pc + 1], b = prog[3 * pc + 2];
        if (op == Q_END) break;
        switch (op) {
            case Q_PUSH_COL: st.push_back(add({LNode::MEM, false, false, 0, a, b, -1, -1})); break;
            case Q_PUSH_TMP: st.push_back(add({LNode::MEM, false, true, 0, num_cols + a, 0, -1, -1})); break;     // parked intermediates are columns num_cols + slot
            case Q_PUSH_CONST: st.push_back(add({LNode::CONST, false, false, 0, a, 0, -1, -1})); break;
            case Q_ADD: case Q_SUB: case Q_MUL: {
                const int32_t y = st.back(); st.pop_back();
                const int32_t x = st.back(); st.pop_back();
                st.push_back(add({LNode::BIN, nodes[x].has_tee || nodes[y].has_tee, false, op, 0, 0, x, y}));
                break;
            }
            case Q_NEG: case Q_SQUARE: case Q_DOUBLE: { const int32_t x = st.back(); st.back() = add({LNode::UN, nodes[x].has_tee, false, op, 0, 0, x, -1}); break; }
            case Q_MUL_CONST: case Q_ADD_CONST: { const int32_t x = st.back(); st.back() = add({LNode::CONSTOP, nodes[x].has_tee, false, op, a, 0, x, -1}); break; }
            case Q_TEE_TMP: { const int32_t x = st.back(); st.back() = add({LNode::TEE, true, false, 0, a, 0, x, -1}); break; }
            case Q_FOLD: {
                const int32_t r = st.back(); st.pop_back();
                materialise_pending();
                if (nodes[r].kind == LNode::MEM && a < (1u << (32 - K_CONST_SHIFT))) evs.push_back({-1, {K_FOLD_COL | (a << K_CONST_SHIFT), nodes[r].a, nodes[r].b}});
                else { evs.push_back({r, {}}); evs.push_back({-1, {Q_FOLD, a, 0}}); }
                break;
            }
            default: break;     // validate_program has refused everything else
        }
    }
    materialise_pending();
    if (mac2) {
        int cur = 0;
        for (const Ev& e : evs) {
            if (e.node >= 0) { limit = std::max(limit, cur + du[e.node]); cur += net[e.node]; }
            else if ((e.raw.w0 & 0xffu) == Q_FOLD) --cur;
        }
    }
    for (const Ev& e : evs) {
        if (e.node >= 0) emit(e.node);
        else out->push_back(e.raw);
    }
}

// Settle / normalise bits, prefetch hazards and stack depth of a fused program (bounds: header comment).  V in units of p, L in
// units of 2^29.  Round 6: a stack entry may grow to (8, 4) -- sums only ever need limbs below 2^31 (carries are propagated where a
// limb bound is in the way: K_NORM, 24 instructions) and the consumers that care about the VALUE say so: the first operand of a
// product by a memory operand takes V <= 5, by a constant anything here, the second operand of a stack product / a subtrahend / a
// value being parked must be settled.  A value above 4p that has to be settled after all takes q_settle8 (one more conditional
// subtraction).  The Horner steps S = S y^g + term of the compiled class programs run without a single settle that way; round 5's
// rule (everything within (4, 4), settle on every excess: ZK_QUOTIENT_RELAXED=0) spent 8 024 settles on the 12 289 products of the
// EVM-style class program.
inline int lower_bounds(std::vector<LowInstr>* prog_io, uint32_t num_cols, int* max_depth, bool relaxed) {
    struct Bd { int V, L; };
    std::vector<Bd> bs;
    std::vector<LowInstr> out;
    out.reserve(prog_io->size() + 8);
    int mx = 0;
    const int capV = relaxed ? 8 : 4;
    for (size_t ii = 0; ii < prog_io->size(); ++ii) {
        LowInstr in = (*prog_io)[ii];
        const uint32_t op = in.w0 & 0xffu;
        auto settle0 = [&]() { in.w0 &= ~(K_NORM0 | K_SETTLE0 | K_SETTLE0_8); in.w0 |= bs.back().V > 4 ? K_SETTLE0_8 : K_SETTLE0; bs.back() = {2, 1}; };
        auto settle1 = [&]() { in.w0 &= ~(K_NORM1 | K_SETTLE1 | K_SETTLE1_8); in.w0 |= bs[bs.size() - 2].V > 4 ? K_SETTLE1_8 : K_SETTLE1; bs[bs.size() - 2] = {2, 1}; };
        auto norm0 = [&]() { if (!relaxed) { settle0(); return; } if (!(in.w0 & (K_SETTLE0 | K_SETTLE0_8))) in.w0 |= K_NORM0; bs.back().L = 1; };
        auto norm1 = [&]() { if (!relaxed) { settle1(); return; } if (!(in.w0 & (K_SETTLE1 | K_SETTLE1_8))) in.w0 |= K_NORM1; bs[bs.size() - 2].L = 1; };
        auto settled0 = [&]() { if (bs.back().V > 2 || bs.back().L > 1) settle0(); };          // t0 must be a settled value
        // t0 op= something of bounds (dV, dL): make room in t0
        auto room0 = [&](int dV, int dL) {
            if (bs.back().L + dL > 4) norm0();
            if (bs.back().V + dV > capV) settle0();
        };
        const size_t need = op == K_MAC2_COL ? 4 : op == K_MAC_STK ? 3 : (op == Q_ADD || op == Q_SUB || op == Q_MUL || op == K_MAC_COL || op == K_PUSH_COL32) ? 2 : (op == Q_PUSH_COL || op == Q_PUSH_CONST || op == K_FOLD_COL || op == K_NOP) ? 0 : 1;
        if (bs.size() < need) return -1;
        switch (op) {
            case Q_PUSH_COL: case Q_PUSH_CONST: bs.push_back({1, 1}); break;
            case Q_ADD: {
                Bd &x = bs[bs.size() - 2], &y = bs.back();
                if (x.L + y.L > 4) { if (y.L >= x.L) norm0(); else norm1(); }
                if (x.L + y.L > 4) { if (y.L > 1) norm0(); else norm1(); }
                if (x.V + y.V > capV) { if (y.V >= x.V) settle0(); else settle1(); }
                if (x.V + y.V > capV) { if (y.V > 2) settle0(); else settle1(); }
                if (x.V + y.V > capV || x.L + y.L > 4) return -1;
                const Bd r{x.V + y.V, x.L + y.L};
                bs.pop_back(); bs.back() = r;
                break;
            }
            case Q_SUB: {
                settled0();
                if (bs[bs.size() - 2].L + 2 > 4) norm1();
                if (bs[bs.size() - 2].V + 2 > capV) settle1();
                const Bd r{bs[bs.size() - 2].V + 2, 1};
                bs.pop_back(); bs.back() = r;
                break;
            }
            case Q_MUL: {
                settled0();
                if (bs[bs.size() - 2].V * bs.back().V > 5) settle1();
                bs.pop_back(); bs.back() = {2, 1};
                break;
            }
            case Q_NEG: settled0(); bs.back() = {3, 1}; break;       // 2p - t0 reaches 2p itself (t0 = 0): not below 2p
            case Q_SQUARE: settled0(); bs.back() = {2, 1}; break;
            case Q_DOUBLE: if (bs.back().L > 2) norm0(); if (2 * bs.back().V > capV) settle0(); bs.back() = {2 * bs.back().V, 2 * bs.back().L}; break;
            case Q_FOLD: if (bs.back().L > 3) norm0(); bs.pop_back(); break;
            case Q_MUL_CONST: bs.back() = {2, 1}; break;
            case Q_ADD_CONST: case K_ADD_COL: room0(1, 1); bs.back() = {bs.back().V + 1, bs.back().L + 1}; break;
            case Q_TEE_TMP: settled0(); break;
            case K_SUB_COL: room0(2, 2); bs.back() = {bs.back().V + 2, bs.back().L + 2}; break;
            case K_RSUB_COL: settled0(); bs.back() = {3, 1}; break;
            case K_MUL_COL: if (bs.back().V > 5) settle0(); bs.back() = {2, 1}; break;
            case K_MAC_COL: {
                // t0 * 32 m + S c' < (32 V_t0 + V_S) p^2 <= 168 p^2 < 2^261 p (V_t0 <= 5 as for MUL_COL, V_S <= 8); columns below
                // 9 (L_t0 + L_S + 1) 2^58 + 2^35 < 2^64 for L_t0 + L_S <= 6 -- carries of t0 propagated where not (L_S <= 4): S never needs a flag
                if (bs.back().V > 5) settle0();
                if (bs.back().L + bs[bs.size() - 2].L > 6) norm0();
                bs.pop_back(); bs.back() = {2, 1};
                break;
            }
            // The three-product step  t0 * 32 m2 + X * 32 m1 + S c'  (t0 = Y; m1, m2, c' canonical):
            //   value   (32 (V_X + V_Y) + V_S) p^2 must stay below 2^261 p = 169.3 p^2: V_X + V_Y <= 5 with V_S <= 8 (168);
            //   columns 27 limb products + 9 of the reduction: 9 (L_Y + L_X + L_S + 1) 2^58 + 2^35 < 2^64 for L_X + L_Y + L_S <= 6.
            // X and S are in LDS when the product runs and the kernel has no step that settles them there.  S is whatever the stack holds (V <= 8, L <= 4).
            // X is still in registers when PUSH_COL32 spills it, so the requests for X ride on that instruction: V_X <= 3 and L_X + L_S <= 5 leave
            // room for a Y that MAC2_COL's own bit-0 requests can always reach (settled: V 2, L 1).
            case K_PUSH_COL32: {
                if (bs.back().V > 3) settle0();
                if (bs.back().L + bs[bs.size() - 2].L > 5) norm0();
                bs.push_back({32, 1});
                break;
            }
            case K_MAC2_COL: {
                const Bd S = bs[bs.size() - 4], X = bs[bs.size() - 3];
                if (X.V + bs.back().V > 5) settle0();
                if (X.L + S.L + bs.back().L > 6) norm0();
                if (X.V + bs.back().V > 5 || X.L + S.L + bs.back().L > 6 || S.V > 8) return -1;
                bs.pop_back(); bs.pop_back(); bs.pop_back(); bs.back() = {2, 1};
                break;
            }
            // B * 32 t0 + S c'  (B = the entry below the top, popped into registers: bit-1 requests reach it; t0 settled, then shifted in place --
            // 17 instructions on 211 steps a row; a constant in another Montgomery form instead would leave U V a factor 32 short of S c', and
            // carrying that factor to a later product by a constant needs a form tag on every stack entry: not worth 0.1 % of the instructions):
            //   value (32 V_B V_t0 + V_S) p^2 <= 168 p^2 for V_B V_t0 <= 5 (Q_MUL's rule); columns 9 (L_B + L_S + 1) 2^58 + 2^35 < 2^64 for L_B + L_S <= 6
            case K_MAC_STK: {
                settled0();
                if (bs[bs.size() - 2].V * bs.back().V > 5) settle1();
                if (bs[bs.size() - 2].L + bs[bs.size() - 3].L > 6) norm1();
                bs.pop_back(); bs.pop_back(); bs.back() = {2, 1};
                break;
            }
            case K_FOLD_COL: case K_NOP: break;
            default: return -1;
        }
        // the memory operand of an instruction is loaded while its predecessor runs: a parked intermediate must not be
        // read back by the instruction right behind the one that parks it
        if (k_has_mem(in.w0) && in.a >= num_cols) {
            for (int back = 1; back <= Q_PREFETCH_DIST; ++back) {
                if ((int)out.size() < back) break;
                const LowInstr& pv = out[out.size() - back];
                if ((pv.w0 & 0xffu) == Q_TEE_TMP && pv.a == in.a - num_cols) { for (int q = back; q <= Q_PREFETCH_DIST; ++q) out.push_back({K_NOP, 0, 0}); break; }
            }
        }
        out.push_back(in);
        if ((int)bs.size() > mx) mx = (int)bs.size();
    }
    *max_depth = mx;
    prog_io->swap(out);
    return 0;
}

// Check of a caller's program: stack discipline and, with `operands`, operand ranges, parking order and the evaluator's stack (zk_quotient_eval;
// the lowering's own entry points know no ranges and check the discipline alone).  status QL_OK, or the pc and the message of the first fault.
struct ProgramCheck { int status = QL_OK; uint32_t pc = 0; std::string msg; int depth = 0; uint32_t num_tmp = 0; };
inline ProgramCheck check_program(const uint32_t* prog, uint32_t len, bool operands, uint32_t ncols = 0, uint32_t nconsts = 0) {
    ProgramCheck r;
    int sp = 0;
    std::vector<bool> defined;
    auto fail = [&](int status, uint32_t pc, const char* fmt, ...) -> ProgramCheck& {
        char buf[160];
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(buf, sizeof buf, fmt, ap);
        va_end(ap);
        r.status = status; r.pc = pc; r.msg = buf;
        return r;
    };
    for (uint32_t pc = 0; pc < len; ++pc) {
        const uint32_t op = prog[3 * pc], a = prog[3 * pc + 1];
        switch (op) {
            case Q_END: return r;
            case Q_PUSH_COL: if (operands && a >= ncols) return fail(QL_INVALID_ARG, pc, "quotient program: column %u out of range at pc %u", a, pc); ++sp; break;
            case Q_PUSH_CONST: if (operands && a >= nconsts) return fail(QL_INVALID_ARG, pc, "quotient program: constant %u out of range at pc %u", a, pc); ++sp; break;
            case Q_ADD: case Q_SUB: case Q_MUL: if (sp < 2) return fail(QL_INVALID_ARG, pc, "quotient program: stack underflow at pc %u", pc); --sp; break;
            case Q_NEG: case Q_SQUARE: case Q_DOUBLE: if (sp < 1) return fail(QL_INVALID_ARG, pc, "quotient program: stack underflow at pc %u", pc); break;
            case Q_MUL_CONST: case Q_ADD_CONST: if (sp < 1 || (operands && a >= nconsts)) return fail(QL_INVALID_ARG, pc, "quotient program: bad operand at pc %u", pc); break;
            case Q_FOLD: if (sp < 1 || (operands && a >= nconsts)) return fail(QL_INVALID_ARG, pc, "quotient program: bad FOLD at pc %u", pc); --sp; break;
            case Q_TEE_TMP:
                if (sp < 1 || (operands && a >= Q_MAX_TMP)) return fail(QL_INVALID_ARG, pc, "quotient program: bad TEE_TMP at pc %u", pc);
                if (!operands) break;
                if (a >= defined.size()) defined.resize(a + 1, false);
                defined[a] = true;
                if (a + 1 > r.num_tmp) r.num_tmp = a + 1;
                break;
            case Q_PUSH_TMP:
                if (operands && (a >= defined.size() || !defined[a])) return fail(QL_INVALID_ARG, pc, "quotient program: intermediate %u read before it is written (pc %u)", a, pc);
                ++sp;
                break;
            default: return fail(QL_INVALID_ARG, pc, "quotient program: unknown opcode %u at pc %u", op, pc);
        }
        if (sp > r.depth) r.depth = sp;
        if (operands && sp > Q_MAX_STACK) return fail(QL_UNSUPPORTED, pc, "quotient program: stack deeper than %d", Q_MAX_STACK);
    }
    return r;
}

// The caller's program lowered for the kernels: fuse = 0 keeps its instruction sequence (parked intermediates as columns num_cols + slot), bit 0
// takes operands from memory, bit 1 adds the fused Horner steps (K_MAC_COL), bit 2 (with bit 1) sums of two column products and stack products;
// then the bounds pass.  Nonzero: the bounds pass refused the stream.
inline int lower_program(const uint32_t* prog, uint32_t len, uint32_t num_cols, int fuse, bool relaxed, std::vector<LowInstr>* low, int* depth, uint32_t* declined = nullptr) {
    if (fuse) lower_fuse(prog, len, num_cols, low, (fuse & 2) != 0, (fuse & 6) == 6, declined);
    else
        for (uint32_t pc = 0; pc < len && prog[3 * pc] != Q_END; ++pc) {
            const uint32_t op = prog[3 * pc], a_ = prog[3 * pc + 1], b_ = prog[3 * pc + 2];
            if (op == Q_PUSH_TMP) low->push_back({Q_PUSH_COL, num_cols + a_, 0});
            else low->push_back({op, a_, b_});
        }
    return lower_bounds(low, num_cols, depth, relaxed);
}

// ---- slicing a large program for the caches (round 6) --------------------------------------------------------------------------
// A class program of the EVM-style constraint system reads each of its operands ~70 times per row, hundreds of instructions apart, and the
// rows of the ~5 000 resident waves x their few hundred columns are gigabytes: every read goes to HBM (5 TB/s of operand loads for 5 KB of
// distinct operands per row).  Made to evaluate ONE row tile with four to sixteen workgroups at a time (ZK_QUOTIENT_TILE_ALIAS) the same
// launch takes 116 ... 107 ms instead of 139: with a sixteenth of the rows in flight their operands stay in the Infinity Cache.  So a program
// that is a top-level sum  acc = acc * c_f + term_f  is cut at fold boundaries into S slices, slice s is evaluated from acc = 0 by its own
// workgroup over the same rows at the same time (k_quotient_eval2: slice_tab), and
//      acc_out(slice s) = acc_in * prod_{f in s} c_f + P_s
// puts the partial sums P_s together afterwards (an S-term FOLD_COL chain through this same function).  A cut is only made where no parked
// intermediate is alive; parking slots are renumbered per slice (slices run concurrently).  ZK_QUOTIENT_SLICES=0 turns it off, =N asks for N.
struct SlicePlan { std::vector<uint32_t> cut; };       // cut[s] .. cut[s + 1]: the caller's instructions of slice s
// row_bytes: what one operand of one row takes in memory (32, or REC29_BYTES where the columns are coset records: the working set that has
// to fit the caches is an eighth larger then, and the headline's large class is cut into 20 slices instead of 17 -- measured, 88.1 -> 86.8 ms
// per launch on the loop tool, where the packed program gains nothing from more slices)
// knob: ZK_QUOTIENT_SLICES (QuotientEvalKnobs::slices; -1 unset)
inline bool plan_slices(const uint32_t* prog, uint32_t len, uint32_t ext_k, SlicePlan* out, size_t row_bytes, int knob) {
    if (knob == 0 || (knob < 0 && (len < 2048 || ext_k < 16)) || ext_k < 11) return false;     // a forced count (tests) slices small programs too
    std::vector<uint32_t> bpos;           // instruction index behind a top-level FOLD
    std::vector<uint64_t> bcost;          // cost of everything in front of it
    std::vector<int32_t> blocked(len + 2, 0);
    std::vector<uint32_t> last_tee;
    std::vector<uint64_t> ops;
    std::vector<uint32_t> colset;
    uint64_t cost = 0, reads = 0;
    int sp = 0;
    uint32_t n = 0;
    for (; n < len && prog[3 * n] != Q_END; ++n) {
        const uint32_t op = prog[3 * n], a = prog[3 * n + 1];
        switch (op) {
            case Q_PUSH_COL: ++sp; cost += 3; ++reads; ops.push_back(((uint64_t)a << 32) | prog[3 * n + 2]); colset.push_back(a); break;
            case Q_PUSH_CONST: ++sp; cost += 1; break;
            case Q_PUSH_TMP:
                ++sp; cost += 3;
                if (a < last_tee.size()) { ++blocked[last_tee[a] + 1]; --blocked[n + 1]; }       // no cut between the parking and this read
                break;
            case Q_TEE_TMP: if (a >= last_tee.size()) last_tee.resize(a + 1, 0); last_tee[a] = n; cost += 4; break;
            case Q_ADD: case Q_SUB: --sp; cost += 1; break;
            case Q_MUL: --sp; cost += 24; break;
            case Q_SQUARE: case Q_MUL_CONST: cost += 24; break;
            case Q_FOLD: --sp; cost += 24; if (sp == 0) { bpos.push_back(n + 1); bcost.push_back(cost); } break;
            default: cost += 1; break;
        }
    }
    if (bpos.size() < 2 || bpos.back() != n) return false;          // not a sum of terms (or something trails the last fold)
    std::sort(ops.begin(), ops.end()); ops.erase(std::unique(ops.begin(), ops.end()), ops.end());
    std::sort(colset.begin(), colset.end()); colset.erase(std::unique(colset.begin(), colset.end()), colset.end());
    if (knob < 0 && reads < 4 * ops.size()) return false;           // operands read once or twice: nothing to keep in a cache
    // slices wanted: the operands of the rows in flight (~5 000 waves x 64) should be well inside the 256 MiB Infinity Cache
    const uint64_t rows_in_flight = std::min<uint64_t>(1ull << ext_k, 327680);
    const uint64_t ws = colset.size() * (uint64_t)row_bytes * rows_in_flight;
    uint32_t want = knob > 0 ? (uint32_t)knob : (uint32_t)std::min<uint64_t>(64, (ws + (96ull << 20) - 1) / (96ull << 20));
    if (want < 2) return false;
    // cuts at unblocked boundaries, by cost
    std::vector<char> ok(bpos.size(), 1);
    {
        int32_t run = 0;
        size_t b = 0;
        for (uint32_t q = 0; q <= n && b < bpos.size(); ++q) {
            run += blocked[q];
            if (bpos[b] == q) { ok[b] = run == 0; ++b; }
        }
    }
    out->cut.assign(1, 0);
    uint32_t made = 1;
    for (size_t b = 0; b + 1 < bpos.size() && made < want; ++b) {
        if (!ok[b]) continue;
        if (bcost[b] * want >= cost * made) { out->cut.push_back(bpos[b]); ++made; }
    }
    out->cut.push_back(n);
    return out->cut.size() > 2;
}

// ---- the knobs -----------------------------------------------------------------------------------------------------------------
// Every environment variable the evaluator's launch depends on; read() walks ONE table of (name, member, parser, when).  The knobs the tests
// flip inside one process, and the trace, are read at every call; the measurement knobs once per process, at the first read().
struct QuotientEvalKnobs {
    int kernel = 2;         // ZK_QUOTIENT_KERNEL=1: round 5's kernel (k_quotient_eval); anything else: k_quotient_eval2 (one stack entry in registers, 4-word instructions)
    int mac = 2;            // ZK_QUOTIENT_MAC (k_quotient_eval2 only): 0 the stream without fused Horner steps, 1 K_MAC_COL alone, unset / else K_MAC2_COL and K_MAC_STK as well
    int fuse = 1;           // ZK_QUOTIENT_FUSE=0 keeps the caller's instruction sequence (measurement: only the bounds pass runs; a sliced launch lowers all the same)
    int relaxed = 1;        // ZK_QUOTIENT_RELAXED=0: round 5's bounds, everything within (4, 4) (lower_bounds)
    int slices = -1;        // ZK_QUOTIENT_SLICES: 0 no slicing, N asks for N slices, unset: by size and reuse (plan_slices)
    int trace = 0;          // ZK_QUOTIENT_TRACE set: one line per launch of 64 lowered instructions or more on stderr
    int acc_mem = -1;       // ZK_QUOTIENT_ACC_MEM (measurement): 0 / 1 force the accumulator's home
    int lds_pad = 0;        // ZK_QUOTIENT_LDS_PAD (measurement): pad the workgroup's LDS to this many bytes, i.e. cap the workgroups resident per CU (160 KB / pad)
    int tile_alias = 0;     // ZK_QUOTIENT_TILE_ALIAS (measurement, results WRONG): 2^a consecutive workgroups of an XCD evaluate the same row tile
    int loop_records = 0;   // ZK_QUOTIENT_LOOP_RECORDS=1 (measurement): zk_quotient_eval runs in record mode over images of the caller's columns
    bool v2() const { return kernel != 1; }
    // the `fuse` argument of lower_program: for a whole program, and for a slice (which ZK_QUOTIENT_FUSE does not reach)
    int fuse_bits() const { return fuse ? slice_fuse_bits() : 0; }
    int slice_fuse_bits() const { return 1 | (v2() && mac != 0 ? 2 : 0) | (v2() && mac != 0 && mac != 1 ? 4 : 0); }
    static QuotientEvalKnobs read();
};
namespace qknob {
inline int num_or_2(const char* v) { return v ? atoi(v) : 2; }
inline int num_or_unset(const char* v) { return v ? atoi(v) : -1; }
inline int num_or_0(const char* v) { return v ? atoi(v) : 0; }
inline int on_unless_zero(const char* v) { return !(v && atoi(v) == 0); }
inline int on_if_one(const char* v) { return v && atoi(v) == 1; }
inline int is_set(const char* v) { return v != nullptr; }
inline int bytes(const char* v) { const long b = v ? atol(v) : 0; return b < 0 ? 0 : b > INT_MAX ? INT_MAX : (int)b; }
struct Entry { const char* env; int QuotientEvalKnobs::*member; int (*parse)(const char*); bool once; };
inline constexpr Entry TABLE[] = {
    {"ZK_QUOTIENT_KERNEL", &QuotientEvalKnobs::kernel, num_or_2, false},        {"ZK_QUOTIENT_MAC", &QuotientEvalKnobs::mac, num_or_2, false},
    {"ZK_QUOTIENT_FUSE", &QuotientEvalKnobs::fuse, on_unless_zero, false},      {"ZK_QUOTIENT_RELAXED", &QuotientEvalKnobs::relaxed, on_unless_zero, false},
    {"ZK_QUOTIENT_SLICES", &QuotientEvalKnobs::slices, num_or_unset, false},    {"ZK_QUOTIENT_TRACE", &QuotientEvalKnobs::trace, is_set, false},
    {"ZK_QUOTIENT_ACC_MEM", &QuotientEvalKnobs::acc_mem, num_or_unset, true},   {"ZK_QUOTIENT_LDS_PAD", &QuotientEvalKnobs::lds_pad, bytes, true},
    {"ZK_QUOTIENT_TILE_ALIAS", &QuotientEvalKnobs::tile_alias, num_or_0, true}, {"ZK_QUOTIENT_LOOP_RECORDS", &QuotientEvalKnobs::loop_records, on_if_one, true},
};
inline QuotientEvalKnobs read_all(QuotientEvalKnobs k, bool once) {
    for (const Entry& d : TABLE) if (d.once == once) k.*d.member = d.parse(getenv(d.env));
    return k;
}
}  // namespace qknob
inline QuotientEvalKnobs QuotientEvalKnobs::read() {
    static const QuotientEvalKnobs once = qknob::read_all(QuotientEvalKnobs(), true);
    return qknob::read_all(once, false);
}

// Coset records as operands (REC instantiations): k_quotient_eval2 alone reads them, and it addresses a row with 32-bit byte offsets
inline bool records_supported(const QuotientEvalKnobs& knobs, uint32_t ext_k) { return knobs.v2() && ext_k >= 2 && ext_k <= 26; }

// ---- the launch plan -----------------------------------------------------------------------------------------------------------
// Everything zk_quotient_eval decides about a launch before it touches the device.  `words` is the program section of the one upload, as it
// travels: per slice (one for a whole program) the lowered instructions -- words_per_instr words each: w0, a, b and, for k_quotient_eval2, the
// class mask -- and four END records for the fetch-ahead; at comb_at, for a sliced launch, the combining program  acc = acc * k_s + P_s  over the
// slices' sums (K_FOLD_COL with constant num_consts + s, reading column num_cols + num_tmp + s) and its four ENDs; at slice_tab_at the slice
// table, (first word, instructions + 1) per slice.  The caller supplies what the plan never sees: column pointers, and the field elements --
// constant num_consts + s is the product of the constants slice_folds[s] names, in that order.
struct QuotientLaunch {
    int kernel = 2;                 // 1: k_quotient_eval, 2: k_quotient_eval2
    bool records = false;           // REC
    bool full = false;              // FULL: the grid covers the domain exactly
    bool acc_in_mem = false;        // ACC_MEM: registers for programs that fold on most instructions (and for slices), memory for the rest
    bool sliced = false;
    uint32_t S = 1;                 // slices (1: the whole program)
    int depth = 1;                  // of the lowered stream(s), at least 1
    size_t lds = 0;                 // bytes of LDS per workgroup, ZK_QUOTIENT_LDS_PAD applied
    uint32_t num_tmp = 0;           // parking slots, renumbered per slice for a sliced launch
    uint32_t low_len = 0, folds = 0;   // lowered instructions and the folds among them, over all slices
    uint32_t words_per_instr = 4;
    uint32_t tile_alias = 0;        // what the kernel is passed (0 for a sliced launch)
    size_t comb_at = 0, slice_tab_at = 0;                  // word offsets into `words`
    size_t prog_bytes = 0, col_bytes = 0, const_bytes = 0; // staging regions, in this order; the caller's vanishing inverses follow (k and the division are no inputs of the plan)
    std::vector<uint32_t> words;                            // prog_bytes / 4 of them
    std::vector<std::vector<uint32_t>> slice_folds;         // sliced: per slice, the constant indices of its folds in order
};

inline void trace_quotient_launch(const QuotientLaunch& q, uint32_t ext_k, const std::vector<std::vector<LowInstr>>& lows) {
    static const char* names[26] = {"END", "PUSH_COL", "PUSH_CONST", "ADD", "SUB", "MUL", "NEG", "SQUARE", "DOUBLE", "FOLD", "MUL_CONST", "ADD_CONST", "TEE_TMP", "PUSH_TMP", "?", "?",
                                    "ADD_COL", "SUB_COL", "RSUB_COL", "MUL_COL", "FOLD_COL", "NOP", "MAC_COL", "PUSH_COL32", "MAC2_COL", "MAC_STK"};
    uint32_t hist[26] = {0}, settles = 0, norms = 0;
    for (const std::vector<LowInstr>& low : lows) for (const LowInstr& in : low) { const uint32_t o = in.w0 & 0xffu; if (o < 26) ++hist[o]; settles += ((in.w0 & (K_SETTLE0 | K_SETTLE0_8)) ? 1 : 0) + ((in.w0 & (K_SETTLE1 | K_SETTLE1_8)) ? 1 : 0); norms += ((in.w0 & K_NORM0) ? 1 : 0) + ((in.w0 & K_NORM1) ? 1 : 0); }
    fprintf(stderr, "[zk quotient] 2^%u rows, %u lowered instructions%s, depth %d, %u settles, %u carry propagations:", ext_k, q.low_len, q.sliced ? (" in " + std::to_string(q.S) + " slices").c_str() : "", q.depth, settles, norms);
    for (int o = 0; o < 26; ++o) if (hist[o]) fprintf(stderr, " %s %u", names[o], hist[o]);
    if (q.sliced) { fprintf(stderr, "; slice lengths"); for (const std::vector<LowInstr>& low : lows) fprintf(stderr, " %zu", low.size()); fprintf(stderr, "; %u parking slots", q.num_tmp); }
    fprintf(stderr, "\n");
}

// QL_OK and *out, or the status and *err of the first thing in the way: a fault of the program (check_program), record operands where
// records_supported says no, a slice that reads an intermediate parked outside it, a stream the bounds pass refuses, a lowered stack deeper than
// Q_MAX_STACK, more constants than a sliced launch's combining program can name.
inline int plan_quotient_launch(const uint32_t* prog, uint32_t num_instr, uint32_t num_cols, uint32_t num_consts, uint32_t ext_k, bool records, const QuotientEvalKnobs& knobs,
                                QuotientLaunch* out, std::string* err) {
    auto fail = [&](int status, const std::string& msg) { if (err) *err = msg; return status; };
    const ProgramCheck chk = check_program(prog, num_instr, true, num_cols, num_consts);
    if (chk.status) return fail(chk.status, chk.msg);
    if (records && !records_supported(knobs, ext_k)) return fail(QL_UNSUPPORTED, "quotient program: record operands need k_quotient_eval2 and 2^2 .. 2^26 rows");
    QuotientLaunch q;
    const bool v2 = knobs.v2();
    const uint64_t ne = 1ull << ext_k;
    q.kernel = v2 ? 2 : 1;
    q.records = records;
    q.full = ne >= (uint64_t)Q_THREADS;
    q.words_per_instr = v2 ? 4 : 3;
    q.depth = chk.depth;
    q.num_tmp = chk.num_tmp;
    // a large sum of terms whose operands are read many times is cut into slices that share their rows' operands through the caches (plan_slices)
    SlicePlan plan;
    q.sliced = v2 && ((ne / Q_THREADS) & 7) == 0 && plan_slices(prog, num_instr, ext_k, &plan, records ? Q_REC_ROW_BYTES : Q_ROW_BYTES, knobs.slices);
    const uint32_t S = q.S = q.sliced ? (uint32_t)plan.cut.size() - 1 : 1;
    // lower the program for the kernel (memory operands, settle bits, prefetch hazards)
    std::vector<std::vector<LowInstr>> lows(S);
    if (q.sliced) {
        uint32_t next_slot = 0;
        int dmax = 0;
        q.slice_folds.resize(S);
        for (uint32_t sl = 0; sl < S; ++sl) {
            std::vector<uint32_t> sub(prog + 3 * plan.cut[sl], prog + 3 * plan.cut[sl + 1]);
            std::unordered_map<uint32_t, uint32_t> slot_of;        // parking slots of this slice -> its own range (slices run at the same time)
            for (size_t i = 0; i < sub.size() / 3; ++i) {
                const uint32_t op = sub[3 * i];
                if (op == Q_TEE_TMP || op == Q_PUSH_TMP) {
                    auto it = slot_of.find(sub[3 * i + 1]);
                    if (it == slot_of.end()) {
                        if (op == Q_PUSH_TMP) return fail(QL_INVALID_ARG, "quotient program: slice " + std::to_string(sl) + " reads an intermediate parked outside it");
                        it = slot_of.emplace(sub[3 * i + 1], next_slot++).first;
                    }
                    sub[3 * i + 1] = it->second;
                }
                if (op == Q_FOLD) q.slice_folds[sl].push_back(sub[3 * i + 1]);       // EVERY fold multiplies the accumulator, whatever lies below it on the stack
            }
            sub.push_back(Q_END); sub.push_back(0); sub.push_back(0);
            int dsl = 0;
            if (lower_program(sub.data(), (uint32_t)(sub.size() / 3), num_cols, knobs.slice_fuse_bits(), knobs.relaxed != 0, &lows[sl], &dsl)) return fail(QL_INVALID_ARG, "quotient program: lowering failed");
            dmax = std::max(dmax, dsl);
        }
        q.depth = dmax;
        q.num_tmp = next_slot;
    } else if (lower_program(prog, num_instr, num_cols, knobs.fuse_bits(), knobs.relaxed != 0, &lows[0], &q.depth)) return fail(QL_INVALID_ARG, "quotient program: lowering failed");
    if (q.depth > Q_MAX_STACK) return fail(QL_UNSUPPORTED, "quotient program: stack deeper than " + std::to_string(Q_MAX_STACK));
    if (q.depth < 1) q.depth = 1;
    for (std::vector<LowInstr>& low : lows) {
        bool first = true;
        for (LowInstr& in : low) {
            const uint32_t o = in.w0 & 0xffu;
            if (o == Q_FOLD || o == K_FOLD_COL) { if (first) in.w0 |= K_FIRST_FOLD; first = false; ++q.folds; }
        }
        q.low_len += (uint32_t)low.size();
    }
    q.acc_in_mem = !q.sliced && q.folds > 0 && (knobs.acc_mem < 0 ? (uint64_t)q.folds * 16 <= q.low_len : knobs.acc_mem == 1);
    if (knobs.trace && q.low_len >= 64) trace_quotient_launch(q, ext_k, lows);       // what the kernel will run: lowered instructions by opcode, settle bits, stack depth
    const uint32_t nc_all = num_consts + (q.sliced ? S : 0);      // sliced: constants num_consts + s are what the accumulator coming into slice s is multiplied by
    if (q.sliced && nc_all >= (1u << (32 - K_CONST_SHIFT))) return fail(QL_UNSUPPORTED, "quotient program: too many constants for a sliced launch");
    // column table = the caller's columns, then one pseudo-column per parked intermediate, then (sliced) one per slice's sum
    const size_t ncol_all = (size_t)num_cols + q.num_tmp + (q.sliced ? S : 0), ncomb = q.sliced ? S : 0;
    q.prog_bytes = (size_t)(q.low_len + 4 * S + ncomb + 4) * q.words_per_instr * 4 + (q.sliced ? S * 8 : 0);
    q.col_bytes = (ncol_all ? ncol_all : 1) * 8;
    q.const_bytes = (size_t)(nc_all ? nc_all : 1) * Q_CONST_BYTES * 2;
    q.words.assign(q.prog_bytes / 4, 0);
    uint32_t* hp = q.words.data();
    size_t w = 0;
    std::vector<uint32_t> slice_tab(2 * S);
    for (uint32_t sl = 0; sl < S; ++sl) {
        slice_tab[2 * sl] = (uint32_t)w; slice_tab[2 * sl + 1] = (uint32_t)lows[sl].size() + 1;
        for (const LowInstr& in : lows[sl]) { hp[w++] = in.w0; hp[w++] = in.a; hp[w++] = in.b; if (v2) hp[w++] = q_class_mask(in.w0, records); }
        w += 4 * q.words_per_instr;      // END + the instructions the kernel fetches ahead (Q_END = 0, empty class mask)
    }
    q.comb_at = w;
    if (q.sliced) {
        // the partial sums are columns num_cols + num_tmp + s of a last little program, acc = acc * k_s + P_s over the slices (and the vanishing division the
        // caller asked for), which rides in the same upload and is launched right behind the slices: no second call, no host synchronisation in between
        for (uint32_t sl = 0; sl < S; ++sl) {
            const uint32_t w0 = K_FOLD_COL | ((num_consts + sl) << K_CONST_SHIFT) | (sl ? 0u : K_FIRST_FOLD);
            hp[w++] = w0; hp[w++] = num_cols + q.num_tmp + sl; hp[w++] = 0; hp[w++] = q_class_mask(w0);
        }
        w += 4 * q.words_per_instr;
    }
    q.slice_tab_at = w;
    if (q.sliced) for (uint32_t i = 0; i < 2 * S; ++i) hp[w++] = slice_tab[i];
    q.lds = (size_t)(v2 ? (q.depth > 1 ? q.depth - 1 : 1) : (q.depth > 2 ? q.depth - 2 : 1)) * 9 * Q_THREADS * 4;    // the topmost element(s) are in registers
    if (knobs.lds_pad > 0 && (size_t)knobs.lds_pad > q.lds && (size_t)knobs.lds_pad <= (size_t)Q_MAX_STACK * 9 * Q_THREADS * 4) q.lds = (size_t)knobs.lds_pad;
    q.tile_alias = q.sliced ? 0u : (uint32_t)knobs.tile_alias;
    *out = std::move(q);
    return QL_OK;
}

}  // namespace zk

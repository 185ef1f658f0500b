// The constraint-system part of a key blob (INTEGRATION.md has the layout): the shape, phases, query lists, permutation
// columns, constants and the gate / lookup programs -- everything a key holds before its column data.  One parser, parse_cs
// (cs.hip), reads it for the proving key (zk_pk_create), the verifying key (zk_vk_create) and the host-only hooks.
// The programs are postfix over abstract column and constant references; the prover lowers them for the device evaluator
// (quotient.hip), the verifier evaluates them at one point (verifier.hip).
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "host_f4.hpp"

namespace zk {
namespace cs {

using host::F4;

enum ColType : uint32_t { CT_FIXED = 0, CT_ADVICE = 1, CT_INSTANCE = 2, CT_SPECIAL = 3, CT_PERM_Z = 4, CT_SIGMA = 5, CT_LK_M = 6, CT_LK_PHI = 7, CT_RANDOM = 8, CT_H = 9, CT_SPLIT_R = 10 /* remainder polynomials of the additive split (zk_proof_finish) */ };
enum Special : uint32_t { SP_X = 0, SP_L0 = 1, SP_LLAST = 2, SP_LACTIVE = 3 };
enum QOp : uint32_t { Q_END = 0, Q_PUSH_COL = 1, Q_PUSH_CONST = 2, Q_ADD = 3, Q_SUB = 4, Q_MUL = 5, Q_NEG = 6, Q_SQUARE = 7, Q_DOUBLE = 8, Q_FOLD = 9, Q_MUL_CONST = 10, Q_ADD_CONST = 11, Q_TEE_TMP = 12, Q_PUSH_TMP = 13 };
// abstract constant operands: user constants are [0, num_consts); challenges live above
constexpr uint32_t C_THETA = 0xFFFF0000u, C_BETA = 0xFFFF0001u, C_GAMMA = 0xFFFF0002u, C_Y = 0xFFFF0003u, C_ONE = 0xFFFF0004u, C_ZERO = 0xFFFF0005u, C_DELTA0 = 0xFFFE0000u,   // C_DELTA0 + j = beta * delta^j
                   C_CHAL0 = 0xFFFD0000u,                                                                                      // C_CHAL0 + i = user challenge i
                   C_YPOW0 = 0xFFFC0000u;                                                                                      // C_YPOW0 + g = y^g (folding constraints that are g positions apart)

inline uint32_t colref(uint32_t type, uint32_t idx) { return (type << 24) | idx; }

struct Instr { uint32_t op, a, b; };
inline bool operator==(const Instr& x, const Instr& y) { return x.op == y.op && x.a == y.a && x.b == y.b; }
typedef std::vector<Instr> Prog;

struct Query { uint32_t type, idx; int32_t rot; };

struct Reader {
    const uint8_t* p; size_t left; bool ok = true;
    uint32_t u32() { if (left < 4) { ok = false; return 0; } uint32_t v; memcpy(&v, p, 4); p += 4; left -= 4; return v; }
    const uint8_t* bytes(size_t n) { if (left < n) { ok = false; return nullptr; } const uint8_t* r = p; p += n; left -= n; return r; }
    // a count of records of `each` bytes that the rest of the blob can actually hold (a truncated or
    // hostile header must not drive allocations)
    uint32_t count(size_t each) { const uint32_t c = u32(); if (ok && (size_t)c * each > left) ok = false; return ok ? c : 0; }
    Prog prog() { Prog g; const uint32_t len = count(12); g.reserve(len); for (uint32_t i = 0; i < len && ok; ++i) { Instr in; in.op = u32(); in.a = u32(); in.b = u32(); g.push_back(in); } return g; }
    void queries(std::vector<Query>* out, uint32_t type, uint32_t ncols) {
        const uint32_t cnt = count(8);
        for (uint32_t i = 0; i < cnt && ok; ++i) { const uint32_t c = u32(); const int32_t rot = (int32_t)u32(); if (c >= ncols) ok = false; out->push_back(Query{type, c, rot}); }
    }
};

// Degree of a postfix program as halo2's Expression::degree computes it (columns 1, constants and
// challenges 0, sums the maximum, products the sum); -1 on a malformed program.
inline int program_degree(const Prog& g, std::vector<int>* tmp_degree) {
    std::vector<int> st;
    for (const Instr& in : g) {
        switch (in.op) {
            case Q_PUSH_COL: st.push_back(1); break;
            case Q_PUSH_CONST: st.push_back(0); break;
            case Q_ADD: case Q_SUB: if (st.size() < 2) return -1; { const int b_ = st.back(); st.pop_back(); st.back() = std::max(st.back(), b_); } break;
            case Q_MUL: if (st.size() < 2) return -1; { const int b_ = st.back(); st.pop_back(); st.back() += b_; } break;
            case Q_NEG: case Q_DOUBLE: case Q_ADD_CONST: case Q_MUL_CONST: if (st.empty()) return -1; break;
            case Q_SQUARE: if (st.empty()) return -1; st.back() *= 2; break;
            case Q_TEE_TMP: if (st.empty()) return -1; if (in.a >= tmp_degree->size()) tmp_degree->resize(in.a + 1, 0); (*tmp_degree)[in.a] = st.back(); break;
            case Q_PUSH_TMP: if (in.a >= tmp_degree->size()) return -1; st.push_back((*tmp_degree)[in.a]); break;
            default: return -1;
        }
    }
    return st.size() == 1 ? st[0] : -1;
}

struct ConstraintSystem {
    uint32_t version = 3;               // of the blob it was read from: 3 (Montgomery columns follow) or 4 (typed fixed cells and the permutation mapping follow)
    uint32_t k = 0, bf = 0, d = 0, ext_k = 0, F = 0, A = 0, I = 0, P = 0, L = 0;
    uint32_t chunk = 0, C = 0, u = 0;   // permutation chunk size, #chunks, last usable row index
    std::vector<std::pair<uint32_t, uint32_t>> perm_cols;
    std::vector<F4> consts;
    std::vector<Prog> gates;
    struct Lookup { std::vector<Prog> tables; std::vector<std::vector<Prog>> inputs; };      // mv_lookup::Argument: table_expressions, inputs_expressions
    std::vector<Lookup> lookups;
    std::vector<Query> adv_q, fix_q;         // evaluation queries, in proof order
    uint32_t num_phases = 1;
    std::vector<uint32_t> adv_phase;         // phase of every advice column (halo2 FirstPhase/SecondPhase/...)
    std::vector<uint32_t> chal_phase;        // challenge i becomes available after this phase
    std::vector<Query> inst_q;               // instance queries (verifier side; carried for the vk)
};

// Reads the constraint-system part of a blob from `r` into `cs`, every count checked against what the blob can hold
// (with_columns: the column data of that version must follow as well -- version 3: F + P columns of n Montgomery elements;
// version 4: F cell widths, F payloads of at least one byte per cell, P x n mapping pairs).  ZK_OK, or ZK_ERR_INVALID_ARG with *err set; `r` is left
// at the first byte after the constraint system.
int parse_cs(Reader& r, ConstraintSystem* cs, size_t blob_len, bool with_columns, std::string* err);

}  // namespace cs
}  // namespace zk

// The quotient's planner (quotient_plan.hpp): constraint system and knobs in, degree-class programs out.  Host only, so that it
// links with cs.hip alone into a stand-alone program (tools/quotient_plan_check.cpp); the evaluator's lowering comes from quotient_lower.hpp.
#include <algorithm>
#include <array>
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <unordered_map>
#include <unordered_set>

#include "../../include/zkmi355.h"
#include "quotient_plan.hpp"
#include "quotient_lower.hpp"
#include "class_compile.hpp"

namespace zk {
namespace qplan {

static int on_unless_zero(const char* v) { return !(v && atoi(v) == 0); }
static int on_if_one(const char* v) { return v && atoi(v) == 1; }
static int mac_level(const char* v) { const int l = v ? atoi(v) : 2; return l == 0 || l == 1 ? l : 2; }
static int chunk_choice(const char* v) { return v ? atoi(v) != 0 : -1; }
static const struct { const char* env; int QuotientKnobs::*member; int (*parse)(const char*); } KNOB_TABLE[] = {
    {"ZK_QUOTIENT_SPLIT", &QuotientKnobs::split, on_unless_zero},       {"ZK_QUOTIENT_ADDSPLIT", &QuotientKnobs::addsplit, on_unless_zero},
    {"ZK_QUOTIENT_GROUP", &QuotientKnobs::group, on_unless_zero},       {"ZK_QUOTIENT_DAG", &QuotientKnobs::dag, on_unless_zero},
    {"ZK_QUOTIENT_COSTGATE", &QuotientKnobs::costgate, on_unless_zero}, {"ZK_QUOTIENT_MAC", &QuotientKnobs::mac, mac_level},
    {"ZK_QUOTIENT_CHUNK", &QuotientKnobs::chunk, chunk_choice},         {"ZK_LOOKUP_PLAIN", &QuotientKnobs::lookup_plain, on_if_one},
};
QuotientKnobs QuotientKnobs::read() {
    QuotientKnobs k;
    for (const auto& d : KNOB_TABLE) k.*d.member = d.parse(getenv(d.env));
    return k;
}
std::string QuotientKnobs::key() const {
    std::string s;
    for (const auto& d : KNOB_TABLE) { s += std::to_string(this->*d.member); s += '|'; }
    return s;
}

static Prog prog_from_words(const uint32_t* words, size_t num_instr) {
    Prog g(num_instr);
    for (size_t j = 0; j < num_instr; ++j) g[j] = {words[3 * j], words[3 * j + 1], words[3 * j + 2]};
    return g;
}
// false: `cap_words` cannot hold the program
static bool prog_to_words(const Prog& g, uint32_t* out_words, size_t cap_words) {
    if (cap_words < 3 * g.size()) return false;
    for (size_t j = 0; j < g.size(); ++j) { out_words[3 * j] = g[j].op; out_words[3 * j + 1] = g[j].a; out_words[3 * j + 2] = g[j].b; }
    return true;
}

bool split_leaf_factor(const Prog& g, bool factor_first, Prog* rest, Instr* factor) {
    if (g.size() < 3 || g.back().op != Q_MUL) return false;
    if (factor_first) {
        if (g[0].op != Q_PUSH_COL) return false;
        *factor = g[0];
        rest->assign(g.begin() + 1, g.end() - 1);
    } else {
        if (g[g.size() - 2].op != Q_PUSH_COL) return false;
        *factor = g[g.size() - 2];
        rest->assign(g.begin(), g.end() - 2);
    }
    // `rest` must be ONE complete expression (the other operand of the product at the root)
    int sp = 0;
    for (const Instr& in : *rest) {
        switch (in.op) {
            case Q_PUSH_COL: case Q_PUSH_CONST: case Q_PUSH_TMP: ++sp; break;
            case Q_ADD: case Q_SUB: case Q_MUL: if (sp < 2) return false; --sp; break;
            case Q_TEE_TMP: return false;
            default: if (sp < 1) return false; break;
        }
    }
    return sp == 1;
}
void push_compressed(PB& b, const std::vector<Prog>& exprs) {
    // sum_i theta^(N-1-i) (F x_i) = F * sum_i theta^(N-1-i) x_i: one product by F instead of N (exact: same polynomial)
    if (exprs.size() >= 2) {
        for (int first = 1; first >= 0; --first) {
            std::vector<Prog> rest(exprs.size());
            Instr f0{0, 0, 0};
            bool all = true;
            for (size_t i = 0; i < exprs.size() && all; ++i) {
                Instr f{0, 0, 0};
                all = split_leaf_factor(exprs[i], first != 0, &rest[i], &f) && (i == 0 || (f.a == f0.a && f.b == f0.b));
                if (i == 0) f0 = f;
            }
            if (!all) continue;
            for (size_t i = 0; i < rest.size(); ++i) {
                if (i) b.mulc(C_THETA);
                b.append(rest[i]);
                if (i) b.op(Q_ADD);
            }
            b.g.push_back(f0);
            b.op(Q_MUL);
            return;
        }
    }
    for (size_t i = 0; i < exprs.size(); ++i) {
        if (i) b.mulc(C_THETA);
        b.append(exprs[i]);
        if (i) b.op(Q_ADD);
    }
}

// The quotient's constraints in halo2's order: gates, permutation, lookups (folded with y by the caller).  A pure function of
// the constraint system: challenges enter as constant indices, so the programs -- and with them which column is read on which coset --
// are known before any witness exists (the advice phase uses that to transform columns ahead of time, advice_coset_masks).
static void build_constraints(const ConstraintSystem& cs, bool lk_plain, std::vector<Prog>& cons) {
    PB q;
    auto end_c = [&] { cons.push_back(std::move(q.g)); q.g.clear(); };
    for (const Prog& g : cs.gates) cons.push_back(g);
    const int32_t rot_last = -(int32_t)(cs.bf + 1);
    if (cs.C) {
        q.col(CT_SPECIAL, SP_L0).cst(C_ONE).col(CT_PERM_Z, 0).op(Q_SUB).op(Q_MUL); end_c();                                   // l0 (1 - Z_0)
        q.col(CT_SPECIAL, SP_LLAST).col(CT_PERM_Z, cs.C - 1).op(Q_SQUARE).col(CT_PERM_Z, cs.C - 1).op(Q_SUB).op(Q_MUL); end_c();   // l_last (Z^2 - Z)
        for (uint32_t c = 1; c < cs.C; ++c) {
            q.col(CT_SPECIAL, SP_L0).col(CT_PERM_Z, c).col(CT_PERM_Z, c - 1, rot_last).op(Q_SUB).op(Q_MUL);          // l0 (Z_c - Z_{c-1}(w^last X))
            end_c();
        }
        for (uint32_t c = 0; c < cs.C; ++c) {
            const uint32_t j0 = c * cs.chunk, j1 = std::min(cs.P, j0 + cs.chunk);
            q.col(CT_SPECIAL, SP_LACTIVE);
            q.col(CT_PERM_Z, c, 1);
            for (uint32_t j = j0; j < j1; ++j) q.col(cs.perm_cols[j]).col(CT_SIGMA, j).mulc(C_BETA).op(Q_ADD).addc(C_GAMMA).op(Q_MUL);
            q.col(CT_PERM_Z, c, 0);
            for (uint32_t j = j0; j < j1; ++j) q.col(cs.perm_cols[j]).col(CT_SPECIAL, SP_X).mulc(C_DELTA0 + j).op(Q_ADD).addc(C_GAMMA).op(Q_MUL);
            q.op(Q_SUB).op(Q_MUL); end_c();
        }
    }
    // lookup identities (plonk::evaluation, mv-lookup): with phi_a = f_a + beta and tau = t + beta,
    //   l_active * ( tau * prod_a phi_a * (phi(wX) - phi(X))  -  prod_a phi_a * (tau * sum_a 1/phi_a - m) )
    // An argument with several input tuples parks tau and the phi_a of a row in intermediates (slots
    // above the ones the gate programs use) and forms sum_a prod_{b != a} phi_b from them.
    uint32_t tmp_base = 0;
    for (const Prog& g : cs.gates) for (const Instr& in : g) if (in.op == Q_TEE_TMP || in.op == Q_PUSH_TMP) tmp_base = std::max(tmp_base, in.a + 1);
    // Single-tuple lookups share the table side: tau = t + beta of a table is parked by the first lookup into it and read back by the
    // others (slots above the ones the multi-tuple form reuses; defined once each, so degree classes re-materialise them, TmpSplit).
    uint32_t max_tuples = 0;
    for (uint32_t l = 0; l < cs.L; ++l) if (cs.lookups[l].inputs.size() > 1) max_tuples = std::max<uint32_t>(max_tuples, (uint32_t)cs.lookups[l].inputs.size());
    const uint32_t table_slot0 = tmp_base + (max_tuples ? max_tuples + 2 : 0);
    std::vector<const std::vector<Prog>*> parked_tables;               // table of slot table_slot0 + i
    for (uint32_t l = 0; l < cs.L; ++l) {
        const auto& lk = cs.lookups[l];
        const uint32_t N = (uint32_t)lk.inputs.size();
        q.col(CT_SPECIAL, SP_L0).col(CT_LK_PHI, l).op(Q_MUL); end_c();
        q.col(CT_SPECIAL, SP_LLAST).col(CT_LK_PHI, l).op(Q_MUL); end_c();
        q.col(CT_SPECIAL, SP_LACTIVE);
        if (N == 1 && lk_plain) {                                        // measurement knob: the identity as halo2 writes it
            // (phi(wX) - phi(X)) (f+beta)(t+beta) - ((t+beta) - m (f+beta))
            q.col(CT_LK_PHI, l, 1).col(CT_LK_PHI, l, 0).op(Q_SUB);
            push_compressed(q, lk.inputs[0]); q.addc(C_BETA).op(Q_MUL);
            push_compressed(q, lk.tables); q.addc(C_BETA).op(Q_MUL);
            push_compressed(q, lk.tables); q.addc(C_BETA);
            q.col(CT_LK_M, l); push_compressed(q, lk.inputs[0]); q.addc(C_BETA).op(Q_MUL);
            q.op(Q_SUB).op(Q_SUB).op(Q_MUL); end_c();
            continue;
        }
        if (N == 1) {
            // the same polynomial with phi_f = f + beta and tau = t + beta each computed once:
            //   (phi(wX) - phi(X)) phi_f tau - (tau - m phi_f)  =  phi_f ((phi(wX) - phi(X)) tau + m) - tau
            // four products instead of twelve on a two-column tuple under one selector (push_compressed takes the selector out)
            size_t ti = 0;
            while (ti < parked_tables.size() && !(*parked_tables[ti] == lk.tables)) ++ti;
            const bool first_use = ti == parked_tables.size();
            if (first_use) parked_tables.push_back(&lk.tables);
            const uint32_t slot = table_slot0 + (uint32_t)ti;
            q.col(CT_LK_PHI, l, 1).col(CT_LK_PHI, l, 0).op(Q_SUB);
            if (first_use) { push_compressed(q, lk.tables); q.addc(C_BETA); q.g.push_back({Q_TEE_TMP, slot, 0}); }
            else q.g.push_back({Q_PUSH_TMP, slot, 0});
            q.op(Q_MUL);
            q.col(CT_LK_M, l).op(Q_ADD);
            push_compressed(q, lk.inputs[0]); q.addc(C_BETA).op(Q_MUL);
            q.g.push_back({Q_PUSH_TMP, slot, 0});
            q.op(Q_SUB).op(Q_MUL); end_c();
            continue;
        }
        const uint32_t t_tau = tmp_base, t_phi = tmp_base + 1;          // reused by every multi-input lookup: a row's values are consumed right away
        auto tmp = [&](uint32_t op, uint32_t slot) { q.g.push_back({op, slot, 0}); };
        // prod = phi_0 * ... * phi_{N-1}, each factor parked on the way
        for (uint32_t a = 0; a < N; ++a) {
            push_compressed(q, lk.inputs[a]); q.addc(C_BETA);
            tmp(Q_TEE_TMP, t_phi + a);
            if (a) q.op(Q_MUL);
        }
        tmp(Q_TEE_TMP, t_phi + N);                                       // prod
        // lhs = tau * prod * (phi(wX) - phi(X))
        push_compressed(q, lk.tables); q.addc(C_BETA);
        tmp(Q_TEE_TMP, t_tau);
        q.op(Q_MUL);
        q.col(CT_LK_PHI, l, 1).col(CT_LK_PHI, l, 0).op(Q_SUB).op(Q_MUL);
        // rhs = tau * sum_a prod_{b != a} phi_b - prod * m
        for (uint32_t a = 0; a < N; ++a) {
            bool first = true;
            for (uint32_t b2 = 0; b2 < N; ++b2) {
                if (b2 == a) continue;
                tmp(Q_PUSH_TMP, t_phi + b2);
                if (!first) q.op(Q_MUL);
                first = false;
            }
            if (a) q.op(Q_ADD);
        }
        tmp(Q_PUSH_TMP, t_tau); q.op(Q_MUL);
        tmp(Q_PUSH_TMP, t_phi + N); q.col(CT_LK_M, l).op(Q_MUL);
        q.op(Q_SUB);
        q.op(Q_SUB).op(Q_MUL); end_c();
    }
}
// operands an instruction takes off the stack (each leaves one value)
static int arity(uint32_t op) {
    switch (op) {
        case Q_PUSH_COL: case Q_PUSH_CONST: case Q_PUSH_TMP: return 0;
        case Q_ADD: case Q_SUB: case Q_MUL: return 2;
        default: return 1;                        // NEG, DOUBLE, SQUARE, ADD_CONST, MUL_CONST, TEE_TMP (peeks: one in, one out)
    }
}
static uint32_t class_of_degree(int dg, uint32_t E) {
    uint32_t e = 0;
    while (e < E && ((uint32_t)1 << e) < (uint32_t)std::max(dg - 1, 1)) ++e;
    return e;
}
// e = ceil(log2(degree - 1)) of every constraint (its degree class, see zk_proof_finish), or E for all when classes are off
static int classify_constraints(std::string* err, const ConstraintSystem& cs, const std::vector<Prog>& cons, bool split, uint32_t E, std::vector<uint32_t>& cls) {
    cls.assign(cons.size(), E);
    std::vector<int> tmp_deg;
    char msg[160];
    for (uint32_t i = 0; i < cons.size(); ++i) {
        const int dg = program_degree(cons[i], &tmp_deg);
        if (dg < 0) { snprintf(msg, sizeof msg, "prover: malformed constraint program %u", i); *err = msg; return ZK_ERR_INVALID_ARG; }
        if ((uint32_t)dg > cs.d) { snprintf(msg, sizeof msg, "prover: constraint %u has degree %d above the circuit degree %u", i, dg, cs.d); *err = msg; return ZK_ERR_INVALID_ARG; }
        cls[i] = split ? class_of_degree(dg, E) : E;
    }
    return ZK_OK;
}
// Additive split of a constraint over degree classes.  h is linear in the constraints, so a constraint that is a SUM of terms of
// different degrees -- q (a b - c): the product is of degree 3, q c of degree 2 -- may put each term into the class of ITS degree,
// all with the constraint's own power of y: the term q c is then evaluated on one coset instead of two, and a column that occurs
// only in such low-degree terms (the outputs of multiplication gates, every linearly constrained cell) is transformed to fewer
// cosets.  Recognised shapes (the program's top): SUM, F * SUM and SUM * F with SUM a tree of + / - / negations; the factor F (a
// selector, as a rule) multiplies every group.  The groups sum to the constraint, but only the constraint vanishes on H: what a group
// that moves to a lower class is on H travels with it as a remainder polynomial (zk_proof_finish, CT_SPLIT_R), so that every class
// still divides by X^n - 1 exactly.  Exact field arithmetic: h and every proof byte stay what they were.  Programs that park or
// read shared intermediates are left whole.  ZK_QUOTIENT_ADDSPLIT=0 turns it off.
static bool additive_split(const Prog& g, uint32_t E, std::vector<std::pair<uint32_t, Prog>>& out) {
    struct Node { Instr in; int l, r; };
    std::vector<Node> nd;
    std::vector<int> st;
    for (const Instr& in : g) {
        if (in.op == Q_TEE_TMP || in.op == Q_PUSH_TMP || in.op == Q_FOLD || in.op == Q_END) return false;
        const int ar = arity(in.op);
        Node n_{in, -1, -1};
        if (ar == 2) { if (st.size() < 2) return false; n_.r = st.back(); st.pop_back(); n_.l = st.back(); st.pop_back(); }
        else if (ar == 1) { if (st.empty()) return false; n_.l = st.back(); st.pop_back(); }
        nd.push_back(n_);
        st.push_back((int)nd.size() - 1);
    }
    if (st.size() != 1) return false;
    const int root = st[0];
    std::function<void(int, Prog&)> emit = [&](int v, Prog& o) {
        if (nd[v].l >= 0) emit(nd[v].l, o);
        if (nd[v].r >= 0) emit(nd[v].r, o);
        o.push_back(nd[v].in);
    };
    auto is_sum = [&](int v) { return nd[v].in.op == Q_ADD || nd[v].in.op == Q_SUB || nd[v].in.op == Q_NEG; };
    int factor = -1, sum = root;
    if (nd[root].in.op == Q_MUL) {
        if (is_sum(nd[root].r)) { factor = nd[root].l; sum = nd[root].r; }
        else if (is_sum(nd[root].l)) { factor = nd[root].r; sum = nd[root].l; }
        else return false;
    } else if (!is_sum(root)) return false;
    std::vector<std::pair<int, bool>> terms;            // (node, negative)
    std::function<void(int, bool)> collect = [&](int v, bool neg_) {
        const uint32_t op = nd[v].in.op;
        if (op == Q_ADD) { collect(nd[v].l, neg_); collect(nd[v].r, neg_); }
        else if (op == Q_SUB) { collect(nd[v].l, neg_); collect(nd[v].r, !neg_); }
        else if (op == Q_NEG) collect(nd[v].l, !neg_);
        else terms.push_back({v, neg_});
    };
    collect(sum, false);
    if (terms.size() < 2 || terms.size() > 4096) return false;
    std::vector<int> no_tmps;
    Prog fprog;
    int fdeg = 0;
    if (factor >= 0) { emit(factor, fprog); fdeg = program_degree(fprog, &no_tmps); if (fdeg < 0) return false; }
    std::vector<Prog> tprog(terms.size());
    std::vector<uint32_t> tcls(terms.size());
    for (size_t t = 0; t < terms.size(); ++t) {
        emit(terms[t].first, tprog[t]);
        const int tdeg = program_degree(tprog[t], &no_tmps);
        if (tdeg < 0) return false;
        tcls[t] = class_of_degree(fdeg + tdeg, E);
    }
    std::vector<Prog> group(E + 1);
    for (uint32_t e = 0; e <= E; ++e) {
        int lead = -1;                                   // a positive term first (no negation to spend), else the first term negated
        for (size_t t = 0; t < terms.size() && lead < 0; ++t) if (tcls[t] == e && !terms[t].second) lead = (int)t;
        for (size_t t = 0; t < terms.size() && lead < 0; ++t) if (tcls[t] == e) lead = (int)t;
        if (lead < 0) continue;
        group[e] = tprog[lead];
        if (terms[lead].second) group[e].push_back({Q_NEG, 0, 0});
        for (size_t t = 0; t < terms.size(); ++t) {
            if (tcls[t] != e || (int)t == lead) continue;
            group[e].insert(group[e].end(), tprog[t].begin(), tprog[t].end());
            group[e].push_back({terms[t].second ? Q_SUB : Q_ADD, 0, 0});
        }
    }
    uint32_t used = 0;
    for (uint32_t e = 0; e <= E; ++e) used += !group[e].empty();
    if (used < 2) return false;
    for (uint32_t e = 0; e <= E; ++e) {
        if (group[e].empty()) continue;
        Prog pg = fprog;
        pg.insert(pg.end(), group[e].begin(), group[e].end());
        if (factor >= 0) pg.push_back({Q_MUL, 0, 0});
        out.push_back({e, std::move(pg)});
    }
    return true;
}
// the pieces the classes evaluate, in constraint order (a constraint's pieces by ascending class)
static void class_pieces(const std::vector<Prog>& cons, const std::vector<uint32_t>& cls, bool split, bool addsplit, uint32_t E, std::vector<ClassPiece>& out) {
    const bool on = split && addsplit;
    for (uint32_t i = 0; i < cons.size(); ++i) {
        std::vector<std::pair<uint32_t, Prog>> parts;
        if (on && cls[i] > 0 && additive_split(cons[i], E, parts)) {
            for (auto& pt : parts) out.push_back({i, pt.first, std::move(pt.second)});
        } else out.push_back({i, cls[i], cons[i]});
    }
}
// A class program as ONE weighted sum (round 5).  The class's accumulator used to fold its terms one by one, acc = acc * y^gap + term:
// a product per term, and every term carried its selector -- q (a b), q' c, l_active (...) -- as a product of its own.  The sum
//      sum_i y^(K-1-i) t_i      (t_i = the terms of this class, i = the constraint a term belongs to)
// is the same polynomial when the terms that share a single-column factor F are collected first:
//      sum_F F * (sum_{i in F} y^(K-1-i) r_i) + sum_{others} y^(K-1-i) t_i,        t_i = F r_i
// -- one product by F per group instead of one per term, and no product for the folding.  Exact field arithmetic: h and every proof
// byte are unchanged (tests/test_quotient_classes.py evaluates both forms; the GPU proof tests compare bytes with the oracle prover).
// A term may use parked intermediates: it joins a group only if everything it reads was parked before the group's first term, and a
// term that parks something only ever opens a group, so definitions stay ahead of their readers when later terms move up.
// ZK_QUOTIENT_GROUP=0 keeps the folded form.
static bool assemble_grouped(const std::vector<ClassTerm>& terms, uint32_t K, Prog& out) {
    if (terms.empty() || K >= 0xFFFFu) return false;
    struct Info { bool has_factor[2] = {false, false}; Instr factor[2]; Prog rest[2]; std::vector<uint32_t> reads, defs; int pick = -1; };
    std::vector<Info> info(terms.size());
    auto key = [](const Instr& f) { return ((uint64_t)f.a << 32) | f.b; };
    std::unordered_map<uint64_t, uint32_t> count;
    for (size_t t = 0; t < terms.size(); ++t) {
        const Prog& g = terms[t].prog;
        for (const Instr& in : g) {
            if (in.op == Q_PUSH_TMP) info[t].reads.push_back(in.a);
            else if (in.op == Q_TEE_TMP) info[t].defs.push_back(in.a);
            else if (in.op == Q_FOLD || in.op == Q_END) return false;
        }
        for (int first = 0; first < 2; ++first) {
            info[t].has_factor[first] = split_leaf_factor(g, first != 0, &info[t].rest[first], &info[t].factor[first]);
            if (info[t].has_factor[first] && !(first == 1 && info[t].has_factor[0] && key(info[t].factor[0]) == key(info[t].factor[1]))) ++count[key(info[t].factor[first])];
        }
    }
    for (size_t t = 0; t < terms.size(); ++t) {
        uint32_t best = 1;          // a factor no other term shares is left where it is
        for (int first = 1; first >= 0; --first)
            if (info[t].has_factor[first] && count[key(info[t].factor[first])] > best) { best = count[key(info[t].factor[first])]; info[t].pick = first; }
    }
    // groups in the order of their first terms
    struct Group { std::vector<uint32_t> members; bool factored; std::vector<uint32_t> known; };       // known: what was parked before (and by) the first term
    std::vector<Group> groups;
    std::unordered_map<uint64_t, uint32_t> open;
    std::vector<uint32_t> parked;                      // slots parked by the terms seen so far (original order)
    std::unordered_map<uint32_t, uint32_t> ndefs;      // a slot that is parked more than once (reused) is only read where it stands
    for (const Info& ti : info) for (uint32_t d : ti.defs) ++ndefs[d];
    auto stable = [&](const std::vector<uint32_t>& reads) { for (uint32_t v : reads) { auto it = ndefs.find(v); if (it == ndefs.end() || it->second != 1) return false; } return true; };
    auto subset = [](const std::vector<uint32_t>& x, const std::vector<uint32_t>& of) { for (uint32_t v : x) if (std::find(of.begin(), of.end(), v) == of.end()) return false; return true; };
    for (size_t t = 0; t < terms.size(); ++t) {
        const Info& ti = info[t];
        bool joined = false;
        if (ti.pick >= 0 && ti.defs.empty() && stable(ti.reads)) {
            auto it = open.find(key(ti.factor[ti.pick]));
            if (it != open.end() && subset(ti.reads, groups[it->second].known)) { groups[it->second].members.push_back((uint32_t)t); joined = true; }
        }
        if (!joined) {
            Group gnew;
            gnew.members.push_back((uint32_t)t);
            gnew.factored = ti.pick >= 0;
            gnew.known = parked;
            // what the first term parks inside its OWN co-factor is computed before any other member's co-factor is
            if (ti.pick >= 0) for (const Instr& in : ti.rest[ti.pick]) if (in.op == Q_TEE_TMP) gnew.known.push_back(in.a);
            groups.push_back(std::move(gnew));
            if (ti.pick >= 0) open[key(ti.factor[ti.pick])] = (uint32_t)groups.size() - 1;
        }
        for (uint32_t d : ti.defs) parked.push_back(d);
    }
    out.clear();
    auto weight = [&](uint32_t cons) { if (K - 1 - cons) out.push_back({Q_MUL_CONST, C_YPOW0 + (K - 1 - cons), 0}); };
    bool first_item = true;
    for (const Group& gr : groups) {
        if (gr.factored && gr.members.size() >= 2) {
            const Info& lead = info[gr.members[0]];
            for (size_t j = 0; j < gr.members.size(); ++j) {
                const uint32_t t = gr.members[j];
                const Prog& r = info[t].rest[info[t].pick];
                out.insert(out.end(), r.begin(), r.end());
                weight(terms[t].cons);
                if (j) out.push_back({Q_ADD, 0, 0});
            }
            out.push_back(lead.factor[lead.pick]);
            out.push_back({Q_MUL, 0, 0});
        } else {
            for (size_t j = 0; j < gr.members.size(); ++j) {          // a lone term (a group nobody joined)
                const uint32_t t = gr.members[j];
                out.insert(out.end(), terms[t].prog.begin(), terms[t].prog.end());
                weight(terms[t].cons);
                if (j) out.push_back({Q_ADD, 0, 0});
            }
        }
        if (!first_item) out.push_back({Q_ADD, 0, 0});
        first_item = false;
    }
    out.push_back({Q_FOLD, C_ONE, 0});                  // acc = 0 * 1 + the sum
    return fits_evaluator_stack(out);                   // beyond the evaluator's stack the folded form is kept
}
// ---- TmpSplit (quotient_plan.hpp): shared intermediates re-materialised per degree class
// the sub-expression whose value is on top of the stack after instruction t - 1 of g
static Prog sub_expression(const Prog& g, size_t t) {
    int need = 1;
    size_t start = t;
    while (start > 0 && need > 0) { --start; need += arity(g[start].op) - 1; }
    return Prog(g.begin() + start, g.begin() + t);
}
void TmpSplit::grow(uint32_t s) {
    if (s >= ver.size()) { ver.resize(s + 1, 0); defs.resize(s + 1); }
    for (auto& h : have) if (s >= h.size()) h.resize(s + 1, 0);
}
void TmpSplit::emit_push(uint32_t s, uint32_t e, Prog& out, int depth) {
    grow(s);
    if (have[e][s] == ver[s] && ver[s]) { out.push_back({Q_PUSH_TMP, s, 0}); return; }
    if (!ver[s] || depth > 64) { conflict = true; out.push_back({Q_PUSH_TMP, s, 0}); return; }     // read before any definition: malformed
    for (const Instr& in : defs[s]) {
        if (in.op == Q_PUSH_TMP) emit_push(in.a, e, out, depth + 1);
        else {
            if (in.op == Q_TEE_TMP) { grow(in.a); have[e][in.a] = ver[in.a]; }
            out.push_back(in);
        }
    }
    out.push_back({Q_TEE_TMP, s, 0});
    have[e][s] = ver[s];
}
void TmpSplit::append(const Prog& g, uint32_t e, Prog& out) {
    for (size_t t = 0; t < g.size(); ++t) {
        const Instr& in = g[t];
        if (in.op == Q_TEE_TMP) {
            grow(in.a);
            defs[in.a] = sub_expression(g, t);
            ++ver[in.a];
            have[e][in.a] = ver[in.a];
            out.push_back(in);
        } else if (in.op == Q_PUSH_TMP) emit_push(in.a, e, out);
        else out.push_back(in);
    }
}
// slot reuse with cross-constraint lifetime (see TmpSplit): such keys keep the single-class evaluation
bool tmp_slots_conflict(const std::vector<Prog>& cons) {
    std::vector<uint32_t> ndef, def_at;
    std::vector<uint8_t> cross;
    auto grow = [&](uint32_t s) { if (s >= ndef.size()) { ndef.resize(s + 1, 0); def_at.resize(s + 1, 0); cross.resize(s + 1, 0); } };
    for (uint32_t i = 0; i < cons.size(); ++i)
        for (const Instr& in : cons[i]) {
            if (in.op == Q_TEE_TMP) { grow(in.a); ++ndef[in.a]; def_at[in.a] = i; }
            else if (in.op == Q_PUSH_TMP) { grow(in.a); if (!ndef[in.a]) return true; if (def_at[in.a] != i) cross[in.a] = 1; }
        }
    for (size_t s_ = 0; s_ < ndef.size(); ++s_) if (ndef[s_] > 1 && cross[s_]) return true;
    return false;
}
// Horner steps of a class program that the evaluator runs as one fused multiply-accumulate (K_MAC_COL of csrc/quotient_lower.hpp: two products, one
// reduction) when ZK_QUOTIENT_MAC is on: the program lowered as zk_quotient_eval lowers it, constants numbered densely first
// fuse = 3: K_MAC_COL alone (out4 unused); fuse = 7: out4 = { MAC2_COL, MAC_STK, MAC2_COL fusions declined for stack depth, MAC_COL } of that stream
static uint32_t count_fused(const Prog& g, int fuse = 3, uint32_t* out4 = nullptr) {
    std::vector<uint32_t> w;
    w.reserve(3 * g.size() + 3);
    std::unordered_map<uint32_t, uint32_t> cix;
    for (const Instr& in : g) {
        const bool c = in.op == Q_PUSH_CONST || in.op == Q_MUL_CONST || in.op == Q_ADD_CONST || in.op == Q_FOLD;
        w.push_back(in.op); w.push_back(c ? cix.emplace(in.a, (uint32_t)cix.size()).first->second : in.a); w.push_back(in.b);
    }
    int depth = 0;
    uint32_t decl = 0;
    std::vector<LowInstr> low;
    if (check_program(w.data(), (uint32_t)g.size(), false).status) return 0;
    if (lower_program(w.data(), (uint32_t)g.size(), 0x80000000u, fuse, QuotientEvalKnobs::read().relaxed != 0, &low, &depth, &decl)) return 0;
    uint32_t f = 0, f2 = 0, fs = 0;
    for (const LowInstr& in : low) { const uint32_t o = in.w0 & 0xffu; f += o == K_MAC_COL; f2 += o == K_MAC2_COL; fs += o == K_MAC_STK; }
    if (out4) { out4[0] = f2; out4[1] = fs; out4[2] = decl; out4[3] = f; }
    return f;
}
int make_quotient_plan(const ConstraintSystem& cs, const QuotientKnobs& knobs, bool split_req, bool addsplit_req, QuotientPlan& qp, std::string* err) {
    std::vector<Prog> cons;
    build_constraints(cs, knobs.lookup_plain != 0, cons);
    const uint32_t E = cs.ext_k - cs.k, K = (uint32_t)cons.size();
    const bool conflict = tmp_slots_conflict(cons);
    const bool split = split_req && !conflict;
    qp.K = K; qp.E = E; qp.split = split; qp.addsplit = split && addsplit_req; qp.dag = knobs.dag != 0;
    qp.cls.assign(E + 1, QPlanClass());
    qp.rems.clear();
    qp.refs.clear();
    std::vector<uint32_t> cls;
    if (const int rc = classify_constraints(err, cs, cons, split, E, cls)) return rc;
    TmpSplit tmps(E + 1);
    std::vector<ClassPiece> cpieces;
    class_pieces(cons, cls, split, qp.addsplit, E, cpieces);
    // A constraint vanishes on H; a PART of it does not, and only multiples of X^n - 1 may be divided class by class.  So the
    // parts that leave their constraint's class t for a lower class e take their values on H along: R_(t,e) = the polynomial of
    // degree < n that agrees on H with the y-weighted sum of those parts (evaluated over the Lagrange forms, one pass, one
    // inverse transform).  Class e evaluates (its parts - R), class t (its parts + R): both vanish on H again, the total is
    // unchanged.  R is read like a column (CT_SPLIT_R) on the cosets of the two classes.
    std::vector<std::vector<ClassTerm>> cterms(E + 1);       // the terms of every class in constraint order: (constraint, program)
    {
        std::vector<uint32_t> top(K, 0);
        for (const ClassPiece& pc : cpieces) top[pc.cons] = std::max(top[pc.cons], pc.cls);
        for (const ClassPiece& pc : cpieces) {
            const uint32_t i = pc.cons;
            cterms[pc.cls].emplace_back();
            cterms[pc.cls].back().cons = i;
            tmps.append(pc.prog, pc.cls, cterms[pc.cls].back().prog);                   // the constraint (or its terms of this class), shared intermediates resolved for this class
            if (pc.cls < top[i]) {
                size_t at = 0;
                while (at < qp.rems.size() && !(qp.rems[at].t == top[i] && qp.rems[at].e == pc.cls)) ++at;
                if (at == qp.rems.size()) { qp.rems.emplace_back(); qp.rems.back().t = top[i]; qp.rems.back().e = pc.cls; }
                QPlanRem& rm = qp.rems[at];
                rm.prog.insert(rm.prog.end(), pc.prog.begin(), pc.prog.end());
                rm.prog.push_back({Q_FOLD, rm.used ? C_YPOW0 + (i - rm.last) : C_Y, 0});
                rm.last = i;
                rm.used = true;
            }
        }
    }
    if (tmps.conflict) { *err = "prover: a constraint reads an intermediate before any constraint parked it"; return ZK_ERR_INVALID_ARG; }
    for (size_t j = 0; j < qp.rems.size(); ++j) {
        // both classes take R in as one more term at the very end of the constraint list (weight y^0)
        const uint32_t ref = colref(CT_SPLIT_R, (uint32_t)j);
        cterms[qp.rems[j].e].push_back({K - 1, Prog{{Q_PUSH_COL, ref, 0}, {Q_NEG, 0, 0}}});
        cterms[qp.rems[j].t].push_back({K - 1, Prog{{Q_PUSH_COL, ref, 0}}});
        qp.rems[j].products = count_products(qp.rems[j].prog);
    }
    // the class programs: compiled through the expression graph (class_compile.hpp); knob off or a program too deep for the evaluator's
    // stack: one weighted sum (assemble_grouped, round 5) or the terms folded one by one, acc = acc * y^gap + term
    const bool grouped = knobs.group && !conflict;
    for (uint32_t e = 0; e <= E; ++e) {
        QPlanClass& c = qp.cls[e];
        if (cterms[e].empty()) continue;
        c.used = true;
        ClassCompileStats st;
        bool done = qp.dag && compile_class(cterms[e], K, knobs.chunk, c.prog, &c.last, &st);
        if (done) { c.parked = st.parked; c.max_live = st.max_live; c.groups = st.groups; }
        if (!done && grouped && assemble_grouped(cterms[e], K, c.prog)) { c.last = K - 1; done = true; }
        if (!done) {
            c.prog.clear();
            bool any = false;
            for (const ClassTerm& t : cterms[e]) {
                c.prog.insert(c.prog.end(), t.prog.begin(), t.prog.end());
                c.prog.push_back({Q_FOLD, any ? C_YPOW0 + (t.cons - c.last) : C_Y, 0});       // acc = acc * y^(gap) + g_i
                c.last = t.cons;
                any = true;
            }
        }
        c.products = count_products(c.prog);
        c.fused = knobs.mac ? count_fused(c.prog) : 0;
        c.reductions = c.products - c.fused;
        if (knobs.mac == 2) {
            uint32_t f4[4] = {0, 0, 0, 0};
            count_fused(c.prog, 7, f4);
            c.mac2 = f4[0]; c.mac_stk = f4[1]; c.declined = f4[2];
            c.reductions = c.products - f4[3] - 2 * f4[0] - f4[1];
        }
    }
    for (QPlanClass& c : qp.cls) {
        std::unordered_set<uint32_t> seen;
        for (const Instr& in : c.prog)
            if (in.op == Q_PUSH_COL && seen.insert(in.a).second) {
                c.refs.push_back(in.a);
                if (std::find(qp.refs.begin(), qp.refs.end(), in.a) == qp.refs.end()) qp.refs.push_back(in.a);
            }
    }
    // What the plan executes per proof, in units of one field product over n rows (~10 us at k = 20): a coset transform of a
    // witness-side column ~ 10 of them (the key's own columns are transformed once per key and cached), a remainder its program
    // over H, an inverse transform, and the transforms the two classes that read it already count.
    const double C_T = 10.0;
    qp.cost = 0;
    for (uint32_t e = 0; e <= E; ++e) {
        if (!qp.cls[e].used) continue;
        uint32_t moving = 0;
        for (uint32_t ref : qp.cls[e].refs) moving += !key_column(ref);
        qp.cost += (double)(1u << e) * (moving * C_T + (double)qp.cls[e].products + 2.0);
    }
    for (const QPlanRem& rm : qp.rems) qp.cost += (double)rm.products + C_T + 4.0;
    return ZK_OK;
}
int choose_quotient_plan(const ConstraintSystem& cs, const QuotientKnobs& knobs, std::shared_ptr<const QuotientPlan>* out, std::string* err) {
    const bool split_on = knobs.split, add_on = knobs.addsplit, gate = knobs.costgate;
    std::shared_ptr<QuotientPlan> best;
    std::vector<std::pair<bool, bool>> cand;
    if (split_on && add_on) cand.push_back({true, true});
    if (split_on && (gate || !add_on)) cand.push_back({true, false});
    if (!split_on || gate) cand.push_back({false, false});
    for (const auto& c : cand) {
        auto qp = std::make_shared<QuotientPlan>();
        if (const int rc = make_quotient_plan(cs, knobs, c.first, c.second, *qp, err)) return rc;
        if (getenv("ZK_QUOTIENT_TRACE")) {
            fprintf(stderr, "[zk quotient] plan split=%d addsplit=%d dag=%d: cost %.0f, %zu remainders;", (int)qp->split, (int)qp->addsplit, (int)qp->dag, qp->cost, qp->rems.size());
            for (uint32_t e = 0; e <= qp->E; ++e) if (qp->cls[e].used) fprintf(stderr, " class %u: %zu instr, %u products, %zu columns, %u parked (%u live), %u groups;", e, qp->cls[e].prog.size(), qp->cls[e].products, qp->cls[e].refs.size(), qp->cls[e].parked, qp->cls[e].max_live, qp->cls[e].groups);
            fprintf(stderr, "\n");
        }
        if (!best || (gate && qp->cost < best->cost)) best = qp;
        if (!gate) break;
    }
    best->key = knobs.key();
    *out = best;
    return ZK_OK;
}
void advice_coset_masks(const ConstraintSystem& cs, const QuotientPlan& qp, std::vector<uint32_t>& mask, size_t* key_slots) {
    const uint32_t E = qp.E;
    mask.assign(cs.A, 0u);
    if (E > 5) return;                 // more than 32 cosets: no plan (the quotient transforms everything itself)
    std::unordered_map<uint32_t, uint32_t> key_mask;
    for (uint32_t e = 0; e <= E; ++e) {
        uint32_t cosets = 0;
        for (uint32_t r = 0; r < (1u << E); ++r) if (class_on_coset(E, e, r)) cosets |= 1u << r;
        for (uint32_t ref : qp.cls[e].refs) {
            const uint32_t t = ref >> 24;
            if (t == CT_ADVICE && (ref & 0xFFFFFFu) < cs.A) mask[ref & 0xFFFFFFu] |= cosets;
            else if (key_column(ref)) key_mask[ref] |= cosets;
        }
    }
    if (key_slots) {
        size_t cnt = 0;
        for (const auto& kv : key_mask) cnt += (size_t)__builtin_popcount(kv.second);
        *key_slots = cnt;
    }
}
void advice_lagrange_readers(const ConstraintSystem& cs, const QuotientPlan& qp, std::vector<uint8_t>* need) {
    need->assign(cs.A, 0);
    auto scan = [&](const Prog& g) {
        for (const Instr& in : g)
            if (in.op == Q_PUSH_COL && (in.a >> 24) == CT_ADVICE && (in.a & 0xFFFFFFu) < cs.A) (*need)[in.a & 0xFFFFFFu] = 1;
    };
    for (const auto& lk : cs.lookups) {
        for (const Prog& g : lk.tables) scan(g);
        for (const auto& tuple : lk.inputs) for (const Prog& g : tuple) scan(g);
    }
    for (const auto& pc : cs.perm_cols) if (pc.first == CT_ADVICE && pc.second < cs.A) (*need)[pc.second] = 1;
    for (const QPlanRem& r : qp.rems) scan(r.prog);
}

int write_plan_summary(const QuotientPlan& qp, uint32_t* out_summary, size_t cap_summary, uint32_t class_index, uint32_t* out_words, size_t out_cap_words, uint32_t* out_instr) {
    if (cap_summary < 8 + 8 * (size_t)(qp.E + 1)) return ZK_ERR_INVALID_ARG;
    out_summary[0] = qp.E; out_summary[1] = qp.K; out_summary[2] = qp.split; out_summary[3] = qp.addsplit; out_summary[4] = qp.dag;
    out_summary[5] = (uint32_t)qp.rems.size(); out_summary[6] = (uint32_t)std::min(qp.cost, 4.0e9); out_summary[7] = (uint32_t)qp.refs.size();
    for (uint32_t e = 0; e <= qp.E; ++e) {
        const QPlanClass& c = qp.cls[e];
        uint32_t* o = out_summary + 8 + 8 * e;
        o[0] = c.used; o[1] = (uint32_t)c.prog.size(); o[2] = c.products; o[3] = (uint32_t)c.refs.size(); o[4] = c.parked; o[5] = c.max_live; o[6] = c.groups; o[7] = c.last;
    }
    if (cap_summary >= 8 + 10 * (size_t)(qp.E + 1))         // a caller that asks for them: 2 more words per class -- reductions, fused multiply-accumulates
        for (uint32_t e = 0; e <= qp.E; ++e) {
            uint32_t* o = out_summary + 8 + 8 * (qp.E + 1) + 2 * e;
            o[0] = qp.cls[e].products - qp.cls[e].fused; o[1] = qp.cls[e].fused;
        }
    if (cap_summary >= 8 + 14 * (size_t)(qp.E + 1))         // ... and 4 more for the stream in force: MAC2_COL, MAC_STK, fusions declined for stack depth, its reductions
        for (uint32_t e = 0; e <= qp.E; ++e) {
            uint32_t* o = out_summary + 8 + 10 * (qp.E + 1) + 4 * e;
            o[0] = qp.cls[e].mac2; o[1] = qp.cls[e].mac_stk; o[2] = qp.cls[e].declined; o[3] = qp.cls[e].reductions;
        }
    if (out_instr && class_index <= qp.E) {
        const Prog& g = qp.cls[class_index].prog;
        *out_instr = (uint32_t)g.size();
        if (out_words && !prog_to_words(g, out_words, out_cap_words)) return ZK_ERR_INVALID_ARG;
    }
    return ZK_OK;
}

// the terms of one class as the hooks below receive them: `count` programs back to back, lens[t] instructions of constraint cons[t] < K each
static bool terms_from_words(const uint32_t* words, const uint32_t* lens, const uint32_t* cons, uint32_t count, uint32_t K, std::vector<ClassTerm>& terms) {
    terms.resize(count);
    size_t at = 0;
    for (uint32_t t = 0; t < count; at += lens[t], ++t) {
        if (cons[t] >= K) return false;
        terms[t] = {cons[t], prog_from_words(words + 3 * at, lens[t])};
    }
    return true;
}

}  // namespace qplan
}  // namespace zk

using namespace zk::qplan;

extern "C" {

// ---- the host-only hooks (no device, no SRS; include/zkmi355.h documents them) ----
// TmpSplit over `count` constraints dealt to `classes` classes; every constraint is followed by the marker {Q_FOLD, i, 0}
int zk_host_split_programs(const uint32_t* words, const uint32_t* lens, const uint32_t* cls, uint32_t count, uint32_t classes,
                           uint32_t* out_words, size_t out_cap_words, uint32_t* out_lens, int* conflict) {
    if (!words || !lens || !cls || !out_lens || !conflict || classes == 0) return ZK_ERR_INVALID_ARG;
    std::vector<Prog> cons(count);
    size_t at = 0;
    for (uint32_t i = 0; i < count; at += lens[i], ++i) {
        if (cls[i] >= classes) return ZK_ERR_INVALID_ARG;
        cons[i] = prog_from_words(words + 3 * at, lens[i]);
    }
    *conflict = tmp_slots_conflict(cons) ? 1 : 0;
    std::vector<Prog> progs(classes);
    TmpSplit tmps(classes);
    for (uint32_t i = 0; i < count; ++i) {
        tmps.append(cons[i], cls[i], progs[cls[i]]);
        progs[cls[i]].push_back({Q_FOLD, i, 0});
    }
    if (tmps.conflict) *conflict = 1;
    size_t total = 0;
    for (uint32_t e = 0; e < classes; ++e) { out_lens[e] = (uint32_t)progs[e].size(); total += progs[e].size(); }
    if (!out_words) return ZK_OK;
    if (3 * total > out_cap_words) return ZK_ERR_INVALID_ARG;
    size_t w = 0;
    for (const Prog& pg : progs) { prog_to_words(pg, out_words + w, out_cap_words - w); w += 3 * pg.size(); }
    return ZK_OK;
}

// additive_split of one constraint; one piece, the program itself in the class of its degree, when it is not split
int zk_host_additive_split(const uint32_t* words, uint32_t num_instr, uint32_t E, uint32_t* out_words, size_t out_cap_words, uint32_t* out_cls, uint32_t* out_lens,
                           uint32_t cap_pieces, uint32_t* num_pieces) {
    if (!words || !num_pieces || E > 8) return ZK_ERR_INVALID_ARG;
    const Prog g = prog_from_words(words, num_instr);
    std::vector<int> tmp_deg;
    const int dg = program_degree(g, &tmp_deg);
    if (dg < 0) return ZK_ERR_INVALID_ARG;
    std::vector<std::pair<uint32_t, Prog>> parts;
    const uint32_t whole = class_of_degree(dg, E);
    if (!(whole > 0 && additive_split(g, E, parts))) { parts.clear(); parts.push_back({whole, g}); }
    *num_pieces = (uint32_t)parts.size();
    if (!out_words) return ZK_OK;
    if (!out_cls || !out_lens || parts.size() > cap_pieces) return ZK_ERR_INVALID_ARG;
    size_t w = 0;
    for (size_t j = 0; j < parts.size(); ++j) {
        out_cls[j] = parts[j].first;
        out_lens[j] = (uint32_t)parts[j].second.size();
        if (!prog_to_words(parts[j].second, out_words + w, out_cap_words - w)) return ZK_ERR_INVALID_ARG;
        w += 3 * parts[j].second.size();
    }
    return ZK_OK;
}

// assemble_grouped; ZK_ERR_UNSUPPORTED where the prover would keep the folded form
int zk_host_group_terms(const uint32_t* words, const uint32_t* lens, const uint32_t* cons, uint32_t count, uint32_t K, uint32_t* out_words, size_t out_cap_words, uint32_t* out_instr) {
    if (!words || !lens || !cons || !out_instr) return ZK_ERR_INVALID_ARG;
    std::vector<ClassTerm> terms;
    if (!terms_from_words(words, lens, cons, count, K, terms)) return ZK_ERR_INVALID_ARG;
    Prog out;
    if (!assemble_grouped(terms, K, out)) return ZK_ERR_UNSUPPORTED;
    *out_instr = (uint32_t)out.size();
    if (!out_words) return ZK_OK;
    return prog_to_words(out, out_words, out_cap_words) ? ZK_OK : ZK_ERR_INVALID_ARG;
}

// compile_class under the chunk knob in force; out_stats[0..5] = nodes, parked, max_live, products, groups, depth
int zk_host_compile_class(const uint32_t* words, const uint32_t* lens, const uint32_t* cons, uint32_t count, uint32_t K, uint32_t* out_words, size_t out_cap_words, uint32_t* out_instr,
                          uint32_t* out_last, uint32_t* out_stats) {
    if (!words || !lens || !cons || !out_instr || !out_last) return ZK_ERR_INVALID_ARG;
    std::vector<ClassTerm> terms;
    if (!terms_from_words(words, lens, cons, count, K, terms)) return ZK_ERR_INVALID_ARG;
    Prog out;
    ClassCompileStats st;
    if (!compile_class(terms, K, QuotientKnobs::read().chunk, out, out_last, &st)) return ZK_ERR_UNSUPPORTED;
    *out_instr = (uint32_t)out.size();
    if (out_stats) { out_stats[0] = st.nodes; out_stats[1] = st.parked; out_stats[2] = st.max_live; out_stats[3] = st.products; out_stats[4] = st.groups; out_stats[5] = (uint32_t)st.depth; }
    if (!out_words) return ZK_OK;
    return prog_to_words(out, out_words, out_cap_words) ? ZK_OK : ZK_ERR_INVALID_ARG;
}

// parse_cs, choose_quotient_plan under the knobs in force, write_plan_summary
int zk_host_quotient_plan(const void* cs_blob, size_t blob_len, uint32_t* out_summary, size_t cap_summary, uint32_t class_index, uint32_t* out_words, size_t out_cap_words, uint32_t* out_instr) {
    if (!cs_blob || !out_summary) return ZK_ERR_INVALID_ARG;
    Reader r{(const uint8_t*)cs_blob, blob_len};
    ConstraintSystem cs;
    std::string err;
    int rc = parse_cs(r, &cs, blob_len, false, &err);
    if (rc) { fprintf(stderr, "zk_host_quotient_plan: %s\n", err.c_str()); return rc; }
    std::shared_ptr<const QuotientPlan> qp;
    rc = choose_quotient_plan(cs, QuotientKnobs::read(), &qp, &err);
    if (rc) { fprintf(stderr, "zk_host_quotient_plan: %s\n", err.c_str()); return rc; }
    return write_plan_summary(*qp, out_summary, cap_summary, class_index, out_words, out_cap_words, out_instr);
}

}  // extern "C"

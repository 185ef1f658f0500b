// The quotient's plan: which constraint (or part of one) is evaluated in which degree class, and each class's program.  A pure function of a
// constraint system (cs.hpp) and of the measurement knobs (QuotientKnobs), made by quotient_plan.hip on the host alone -- no device, no context, no
// key.  prover.hip keeps one plan per key; the program builder below also serves its finishing stages and the mock verifier.
#pragma once
#include <algorithm>
#include <memory>
#include <string>
#include <utility>
#include <vector>

#include "cs.hpp"

namespace zk {
namespace qplan {

using namespace zk::cs;

// ---- small program builder ----------------------------------------------------------------------
struct PB {
    Prog g;
    PB& col(uint32_t type, uint32_t idx, int32_t rot = 0) { g.push_back({Q_PUSH_COL, colref(type, idx), (uint32_t)rot}); return *this; }
    PB& col(const std::pair<uint32_t, uint32_t>& c) { return col(c.first, c.second, 0); }      // a permutation column (type, index)
    PB& cst(uint32_t ref) { g.push_back({Q_PUSH_CONST, ref, 0}); return *this; }
    PB& op(uint32_t o) { g.push_back({o, 0, 0}); return *this; }
    PB& mulc(uint32_t ref) { g.push_back({Q_MUL_CONST, ref, 0}); return *this; }
    PB& addc(uint32_t ref) { g.push_back({Q_ADD_CONST, ref, 0}); return *this; }
    PB& fold(uint32_t ref) { g.push_back({Q_FOLD, ref, 0}); return *this; }
    PB& append(const Prog& o) { g.insert(g.end(), o.begin(), o.end()); return *this; }
};
// An expression of the form F * X or X * F with F a single column read: X (postfix) and F; false for any other shape.
// (The inputs of a zkEVM lookup are `q_enable * value`, all of a tuple under the same q_enable.)
bool split_leaf_factor(const Prog& g, bool factor_first, Prog* rest, Instr* factor);
// theta-compression of a list of expressions: ((e0 * theta + e1) * theta + e2) ...
void push_compressed(PB& b, const std::vector<Prog>& exprs);

// What the evaluator's stack machine can run (Q_MAX_STACK in quotient_lower.hpp is 16): the program leaves nothing on the stack and never
// holds more than 14 values.  *depth: the most it holds, *left: what it leaves.
inline bool fits_evaluator_stack(const Prog& g, int* depth = nullptr, int* left = nullptr) {
    int sp = 0, mx = 0;
    for (const Instr& in : g) {
        if (in.op == Q_PUSH_COL || in.op == Q_PUSH_CONST || in.op == Q_PUSH_TMP) ++sp;
        else if (in.op == Q_ADD || in.op == Q_SUB || in.op == Q_MUL || in.op == Q_FOLD) --sp;
        mx = std::max(mx, sp);
    }
    if (depth) *depth = mx;
    if (left) *left = sp;
    return sp == 0 && mx <= 14;
}

// a column of the key (transformed to a coset once per key and cached), not of a session
inline bool key_column(uint32_t ref) { const uint32_t t = ref >> 24; return t == CT_FIXED || t == CT_SIGMA || t == CT_SPECIAL; }
// Degree class e of 0 .. E is evaluated on the cosets r that are multiples of 2^(E - e) (see the quotient stage).
inline bool class_on_coset(uint32_t E, uint32_t e, uint32_t r) { return (r & ((1u << (E - e)) - 1u)) == 0; }

// Intermediates shared between constraints (TEE_TMP in one gate, PUSH_TMP in a later one: the common-subexpression elimination of halo2's
// GraphEvaluator as it survives the export) and degree classes: a class evaluates only ITS constraints, so a class that reads an intermediate
// another class parked must compute it itself.  `TmpSplit` re-materialises: walking the constraints in order, a PUSH_TMP whose definition this
// class has not emitted yet is replaced by the defining sub-expression (its own PUSH_TMPs resolved the same way) followed by the TEE_TMP;
// afterwards the class reads the slot like any other.  Classes run as separate launches over the same parking area, each defining what it
// reads before reading it.  Not handled (tmp_slots_conflict: the caller evaluates everything as one class): a slot that is defined more than
// once AND read by a constraint other than the one that defined it (slot reuse with cross-constraint lifetime).
struct TmpSplit {
    std::vector<Prog> defs;                       // slot -> defining sub-expression (postfix, without the TEE)
    std::vector<uint32_t> ver;                    // slot -> number of definitions seen so far
    std::vector<std::vector<uint32_t>> have;      // class -> slot -> version this class has emitted (0 = none)
    bool conflict = false;
    explicit TmpSplit(size_t classes) : have(classes) {}
    // appends constraint g (class e) to out with its intermediates resolved for that class
    void append(const Prog& g, uint32_t e, Prog& out);
private:
    void grow(uint32_t s);
    void emit_push(uint32_t s, uint32_t e, Prog& out, int depth = 0);
};
bool tmp_slots_conflict(const std::vector<Prog>& cons);

// ---- the knobs ------------------------------------------------------------------------------------
// Every input of the plan besides the constraint system, read from the environment once per plan request (the tests flip them inside one
// process).  read() and key() walk ONE table of (environment name, member, parser): a knob cannot be read without being part of the key.
struct QuotientKnobs {
    int split = 1;          // ZK_QUOTIENT_SPLIT=0: one class for everything
    int addsplit = 1;       // ZK_QUOTIENT_ADDSPLIT=0: no additive split of constraints over the classes
    int group = 1;          // ZK_QUOTIENT_GROUP=0: class programs folded term by term where the compiler is off or gives up
    int dag = 1;            // ZK_QUOTIENT_DAG=0: class programs not compiled through the expression graph (class_compile.hpp)
    int costgate = 1;       // ZK_QUOTIENT_COSTGATE=0: the most split candidate the knobs allow, whatever it costs
    int mac = 2;            // ZK_QUOTIENT_MAC: 0 no fused steps counted, 1 K_MAC_COL alone, unset or anything else all (csrc/quotient_lower.hpp: lower_fuse)
    int chunk = -1;         // ZK_QUOTIENT_CHUNK: 0 / 1 class programs emitted in one parking scope / term by term, unset: by node count
    int lookup_plain = 0;   // ZK_LOOKUP_PLAIN=1: the single-tuple lookup identity as halo2 writes it
    static QuotientKnobs read();
    std::string key() const;
};

// ---- the plan -------------------------------------------------------------------------------------
inline uint32_t count_products(const Prog& g) { uint32_t c = 0; for (const Instr& in : g) c += in.op == Q_MUL || in.op == Q_SQUARE || in.op == Q_MUL_CONST || in.op == Q_FOLD; return c; }
struct ClassPiece { uint32_t cons, cls; Prog prog; };       // a constraint, or the terms of one that the additive split put into class `cls`
struct ClassTerm { uint32_t cons; Prog prog; };             // a term of a class: (constraint it belongs to, program)
struct QPlanClass { Prog prog; std::vector<uint32_t> refs; uint32_t last = 0; bool used = false; uint32_t products = 0, parked = 0, max_live = 0, groups = 0, fused = 0, mac2 = 0, mac_stk = 0, declined = 0, reductions = 0; };
struct QPlanRem { uint32_t t = 0, e = 0; Prog prog; uint32_t last = 0; bool used = false; uint32_t products = 0; };
struct QuotientPlan {
    std::string key;                 // QuotientKnobs::key() of the knob values the plan was made under
    uint32_t K = 0, E = 0;
    bool split = false, addsplit = false, dag = false;
    std::vector<QPlanClass> cls;     // E + 1 classes
    std::vector<QPlanRem> rems;      // remainder polynomials of the additive split: evaluated per proof over the Lagrange forms
    std::vector<uint32_t> refs;      // every column any class reads
    double cost = 0;                 // the estimate the candidates were compared by (units: one product over n rows)
};

// One candidate: degree classes (split_req) and the additive split (addsplit_req) as asked for, where the constraints allow them.
int make_quotient_plan(const ConstraintSystem& cs, const QuotientKnobs& knobs, bool split_req, bool addsplit_req, QuotientPlan& qp, std::string* err);
// The plan the prover follows: of degree classes with the additive split, degree classes alone, one class, the cheapest by a count of what
// each would execute; knobs.costgate off takes the most split one the knobs allow.
int choose_quotient_plan(const ConstraintSystem& cs, const QuotientKnobs& knobs, std::shared_ptr<const QuotientPlan>* out, std::string* err);

// For every advice column: the cosets r (bit r) of the extended domain on which some class active there reads it (all zero above 32 cosets: the
// quotient transforms everything itself); *key_slots: the (column of the key, coset) pairs the quotient reads -- what the key's coset cache will hold.
void advice_coset_masks(const ConstraintSystem& cs, const QuotientPlan& qp, std::vector<uint32_t>& mask, size_t* key_slots);
// Which advice columns some program over the LAGRANGE domain reads inside a session: the tuples of the lookup arguments, the permutation argument's
// columns, the remainder polynomials of the additive split.  Everything else -- gates only -- is read through coefficient forms (cosets, evaluations).
void advice_lagrange_readers(const ConstraintSystem& cs, const QuotientPlan& qp, std::vector<uint8_t>* need);

// The summary words of zk_host_quotient_plan / zk_pk_quotient_plan (include/zkmi355.h) and, with out_instr and class_index <= E, that class's program.
int write_plan_summary(const QuotientPlan& qp, uint32_t* out_summary, size_t cap_summary, uint32_t class_index, uint32_t* out_words, size_t out_cap_words, uint32_t* out_instr);

}  // namespace qplan
}  // namespace zk

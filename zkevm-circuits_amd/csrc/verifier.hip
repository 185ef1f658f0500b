// halo2_proofs::plonk::verify_proof for KZG (VerifierGWC / VerifierSHPLONK), for the proofs
// zk_proof_* writes: Blake2b, Poseidon or EVM transcript, either vanishing "random" polynomial.  The reference verifies every
// proof it makes through it [REF prover/src/common/verifier.rs:35] (verify_snark_shplonk, reached from
// [REF prover/src/zkevm/verifier.rs:45] and [REF prover/src/aggregator/verifier.rs:57]).  The statement this file follows
// is oracle/plonk_verifier.py:verify, the verifier the tests judge every proof by.
//
// What runs where:
//   device : decoding every point of every proof of the batch (one k_g1_decode launch: a square root per compressed point,
//            a range and curve check per EVM point) and the final DualMSM of the whole batch (proofs weighted by powers of
//            a batching scalar, the key's commitments once with summed coefficients); for zk_verify_accumulators the DualMSM
//            of every proof on its own, all of them in one segmented MSM
//   host   : transcript replay and the scalar work of one proof (instance and Lagrange evaluations, the folded identity at
//            x, the multi-open's rotation sets) -- proofs are independent up to the MSM and are replayed on up to 16
//            threads; the 2-term pairing check
//
// zk_vk is the constraint system of the key blob (cs.hpp, parsed by the same parse_cs as zk_pk_create) with the key's
// commitments and vk_repr: no device, no column data, any k <= 27.
#include <algorithm>
#include <array>
#include <atomic>
#include <chrono>
#include <map>
#include <memory>
#include <string>
#include <thread>
#include <tuple>
#include <vector>

#include "ctx.hpp"
#include "cs.hpp"
#include "host_hash.hpp"
#include "host_pairing.hpp"

using namespace zk;
using namespace zk::cs;
using zk::host::F4;

struct zk_vk : zk::cs::ConstraintSystem {
    std::vector<G1Affine> fixed_com, sigma_com;
    F4 vk_repr;
};

namespace {

using namespace zk::host;

// Where the key puts things in a proof of one transcript kind and multi-open scheme.
struct Layout {
    uint32_t point_len = 32;      // 32 B compressed (Blake2b, Poseidon) or 64 B x || y (EVM)
    uint32_t pre_points = 0;      // advice, m, Z, phi, random, h pieces: every point before the evaluations
    uint32_t evals = 0;           // scalars
    uint32_t open_points = 0;     // GWC: one witness per distinct point; SHPLONK: h1, h2
    uint32_t points() const { return pre_points + open_points; }
    size_t len() const { return (size_t)points() * point_len + (size_t)evals * 32; }
    size_t point_offset(uint32_t j) const { return j < pre_points ? (size_t)j * point_len : (size_t)pre_points * point_len + (size_t)evals * 32 + (size_t)(j - pre_points) * point_len; }
};

uint64_t rot_mod(int64_t rot, uint64_t n) { return (uint64_t)(((rot % (int64_t)n) + (int64_t)n) % (int64_t)n); }

// the rotations of every query of the multi-open, in halo2's order (the point set of a GWC proof)
std::vector<int64_t> query_rotations(const ConstraintSystem& cs) {
    std::vector<int64_t> r;
    for (const Query& q : cs.adv_q) r.push_back(q.rot);
    for (uint32_t c = 0; c < cs.C; ++c) { r.push_back(0); r.push_back(1); }
    if (cs.C > 1) r.push_back(-(int64_t)cs.bf - 1);
    for (uint32_t l = 0; l < cs.L; ++l) { r.push_back(0); r.push_back(1); }
    for (const Query& q : cs.fix_q) r.push_back(q.rot);
    r.push_back(0);          // sigma, h and the random polynomial are opened at x
    return r;
}

Layout layout_of(const ConstraintSystem& cs, int kind, int multiopen) {
    Layout lo;
    lo.point_len = kind == ZK_TRANSCRIPT_EVM ? 64 : 32;
    lo.pre_points = cs.A + cs.L + cs.C + cs.L + 1 + (cs.d - 1);
    lo.evals = (uint32_t)cs.adv_q.size() + (uint32_t)cs.fix_q.size() + 1 + cs.P + (cs.C ? 3 * cs.C - 1 : 0) + 3 * cs.L;
    if (multiopen == ZK_MULTIOPEN_SHPLONK) {
        lo.open_points = 2;
    } else {
        const uint64_t n = (uint64_t)1 << cs.k;
        std::vector<uint64_t> pts;
        for (int64_t r : query_rotations(cs)) pts.push_back(rot_mod(r, n));
        std::sort(pts.begin(), pts.end());
        lo.open_points = (uint32_t)(std::unique(pts.begin(), pts.end()) - pts.begin());
    }
    return lo;
}

F4 fr_neg(const F4& a) { return fr_sub(fr_zero(), a); }
bool fr_canon_less(const F4& a, const F4& b) {     // BTreeSet<Fr> order: by canonical value
    const F4 x = fr_canon(a), y = fr_canon(b);
    for (int i = 3; i >= 0; --i) if (x.l[i] != y.l[i]) return x.l[i] < y.l[i];
    return false;
}
F4 fr_from_device(const Fr& v) { F4 r; memcpy(r.l, &v, 32); return r; }

// One proof's verdict and DualMSM: coefficients over [its M points | F fixed and P sigma commitments | the generator].
struct ProofWork {
    bool ok = false;
    std::vector<F4> right, left;     // e(left, [s]) == e(right, [1])
};

struct Replay {
    const zk_vk& vk;
    const Layout& lo;
    int kind, multiopen;
    F4 omega, delta;
    uint32_t M, G;                   // points per proof; index of the generator in the coefficient vectors

    // proof: the bytes; pts: its M decoded points; bad: their decode flags
    void run(const uint8_t* proof, const G1Affine* pts, const uint8_t* bad, const F4* const* inst, const uint32_t* inst_len, ProofWork* out) const {
        out->ok = false;
        for (uint32_t j = 0; j < M; ++j) if (bad[j]) return;
        const ConstraintSystem& cs = vk;
        const uint64_t n = (uint64_t)1 << cs.k;
        for (uint32_t i = 0; i < cs.I; ++i) if (inst_len[i] > cs.u) return;       // more values than usable rows (InstanceTooLarge)
        Transcript tr;
        tr.reset(kind);
        tr.common_scalar(vk.vk_repr);
        for (uint32_t i = 0; i < cs.I; ++i)
            for (uint32_t row = 0; row < inst_len[i]; ++row) tr.common_scalar(inst[i][row]);
        uint32_t pj = 0;
        auto read_point = [&]() { const uint32_t j = pj++; tr.common_point(pts[j]); return j; };
        const uint8_t* sp = proof + (size_t)lo.pre_points * lo.point_len;
        bool canonical = true;
        auto read_scalar = [&]() {
            F4 v;
            if (kind == ZK_TRANSCRIPT_EVM) for (int b = 0; b < 32; ++b) ((uint8_t*)v.l)[b] = sp[31 - b];
            else memcpy(v.l, sp, 32);
            sp += 32;
            if (geq_mod<FrC>(v.l)) { canonical = false; return fr_zero(); }
            const F4 m = fr_to_mont(v);
            tr.common_scalar(m);
            return m;
        };

        std::vector<uint32_t> adv_com(cs.A);
        std::vector<F4> challenges(cs.chal_phase.size(), fr_zero());
        for (uint32_t ph = 0; ph < cs.num_phases; ++ph) {
            for (uint32_t i = 0; i < cs.A; ++i) if (cs.adv_phase[i] == ph) adv_com[i] = read_point();
            for (size_t c = 0; c < cs.chal_phase.size(); ++c) if (cs.chal_phase[c] == ph) challenges[c] = tr.squeeze();
        }
        const F4 theta = tr.squeeze();
        std::vector<uint32_t> m_com(cs.L), z_com(cs.C), phi_com(cs.L);
        for (auto& j : m_com) j = read_point();
        const F4 beta = tr.squeeze(), gamma = tr.squeeze();
        for (auto& j : z_com) j = read_point();
        for (auto& j : phi_com) j = read_point();
        const uint32_t random_com = read_point();
        const F4 y = tr.squeeze();
        const uint32_t h0 = pj;
        for (uint32_t i = 0; i + 1 < cs.d; ++i) read_point();
        const F4 x = tr.squeeze();

        std::vector<F4> adv_ev(cs.adv_q.size()), fix_ev(cs.fix_q.size()), sigma_ev(cs.P);
        for (auto& e : adv_ev) e = read_scalar();
        for (auto& e : fix_ev) e = read_scalar();
        const F4 random_ev = read_scalar();
        for (auto& e : sigma_ev) e = read_scalar();
        std::vector<std::array<F4, 3>> z_ev(cs.C);
        for (uint32_t c = 0; c < cs.C; ++c) {
            z_ev[c][0] = read_scalar();
            z_ev[c][1] = read_scalar();
            z_ev[c][2] = c + 1 < cs.C ? read_scalar() : fr_zero();
        }
        std::vector<std::array<F4, 3>> lk_ev(cs.L);        // phi(x), phi(wx), m(x)
        for (auto& e : lk_ev) for (F4& v : e) v = read_scalar();
        if (!canonical || tr.err) return;

        // ---- the point x * omega^rot, Lagrange basis values at it, instance evaluations (KZG does not query instance columns)
        const F4 one = fr_one();
        auto omega_pow = [&](uint64_t e) { return fr_pow(omega, e); };
        auto point = [&](int64_t rot) { return fr_mul(x, omega_pow(rot_mod(rot, n))); };
        const F4 n_fr = host::fr_from_u64(n), xn = fr_pow(x, n);
        auto lagrange_at = [&](uint64_t i, const F4& pt, const F4& ptn) {       // L_i(pt) = w^i (pt^n - 1) / (n (pt - w^i))
            const F4 wi = omega_pow(i);
            return fr_mul(fr_mul(wi, fr_sub(ptn, one)), fr_inv(fr_mul(n_fr, fr_sub(pt, wi))));
        };
        std::map<std::pair<uint32_t, int64_t>, F4> inst_cache;
        auto instance_eval = [&](uint32_t i, int64_t rot) {
            auto it = inst_cache.find({i, rot});
            if (it != inst_cache.end()) return it->second;
            const F4 pt = point(rot), ptn = fr_pow(pt, n);
            // sum_row v_row w^row / (pt - w^row) * (pt^n - 1) / n, one batch inversion over the rows
            const uint32_t len = inst_len[i];
            std::vector<F4> den(len), wrow(len);
            F4 w = one;
            for (uint32_t row = 0; row < len; ++row) { wrow[row] = w; den[row] = fr_sub(pt, w); w = fr_mul(w, omega); }
            std::vector<F4> pre(len + 1);
            pre[0] = one;
            for (uint32_t row = 0; row < len; ++row) pre[row + 1] = fr_is_zero(den[row]) ? pre[row] : fr_mul(pre[row], den[row]);
            F4 inv = fr_inv(pre[len]), acc = fr_zero();
            for (uint32_t row = len; row-- > 0;) {
                if (fr_is_zero(den[row])) continue;           // fr_inv(0) = 0, as the oracle's pow(0, r - 2)
                const F4 d_inv = fr_mul(inv, pre[row]);
                inv = fr_mul(inv, den[row]);
                if (!fr_is_zero(inst[i][row])) acc = fr_add(acc, fr_mul(inst[i][row], fr_mul(wrow[row], d_inv)));
            }
            const F4 v = fr_mul(acc, fr_mul(fr_sub(ptn, one), fr_inv(n_fr)));
            inst_cache[{i, rot}] = v;
            return v;
        };
        bool missing = false;
        auto col_eval = [&](uint32_t type, uint32_t idx, int64_t rot) -> F4 {
            if (type == CT_INSTANCE) return idx < cs.I ? instance_eval(idx, rot) : (missing = true, fr_zero());
            const std::vector<Query>& qs = type == CT_ADVICE ? cs.adv_q : cs.fix_q;
            const std::vector<F4>& ev = type == CT_ADVICE ? adv_ev : fix_ev;
            if (type == CT_ADVICE || type == CT_FIXED)
                for (size_t q = 0; q < qs.size(); ++q) if (qs[q].idx == idx && qs[q].rot == rot) return ev[q];
            missing = true;
            return fr_zero();
        };
        std::vector<F4> tmps;
        auto eval = [&](const Prog& g) -> F4 {      // a key program at x: the stack machine of the blob (cs.hpp)
            std::vector<F4> st;
            auto cst = [&](uint32_t a) -> F4 {
                if (a < cs.consts.size()) return cs.consts[a];
                if (a >= C_CHAL0 && a - C_CHAL0 < challenges.size()) return challenges[a - C_CHAL0];
                missing = true;
                return fr_zero();
            };
            for (const Instr& in : g) {
                if (missing) return fr_zero();
                switch (in.op) {
                    case Q_PUSH_COL: st.push_back(col_eval(in.a >> 24, in.a & 0xFFFFFFu, (int32_t)in.b)); break;
                    case Q_PUSH_CONST: st.push_back(cst(in.a)); break;
                    case Q_PUSH_TMP: if (in.a >= tmps.size()) { missing = true; break; } st.push_back(tmps[in.a]); break;
                    case Q_ADD: case Q_SUB: case Q_MUL: {
                        if (st.size() < 2) { missing = true; break; }
                        const F4 b = st.back(); st.pop_back();
                        F4& a = st.back();
                        a = in.op == Q_ADD ? fr_add(a, b) : in.op == Q_SUB ? fr_sub(a, b) : fr_mul(a, b);
                        break;
                    }
                    default: {
                        if (st.empty()) { missing = true; break; }
                        F4& a = st.back();
                        switch (in.op) {
                            case Q_NEG: a = fr_neg(a); break;
                            case Q_SQUARE: a = fr_mul(a, a); break;
                            case Q_DOUBLE: a = fr_add(a, a); break;
                            case Q_MUL_CONST: a = fr_mul(a, cst(in.a)); break;
                            case Q_ADD_CONST: a = fr_add(a, cst(in.a)); break;
                            case Q_TEE_TMP: if (in.a >= tmps.size()) tmps.resize(in.a + 1, fr_zero()); tmps[in.a] = a; break;
                            default: missing = true;
                        }
                    }
                }
            }
            if (st.size() != 1) { missing = true; return fr_zero(); }
            return st[0];
        };

        const F4 l0 = lagrange_at(0, x, xn), l_last = lagrange_at(cs.u, x, xn);
        F4 l_blind = fr_zero();
        for (uint64_t i = cs.u + 1; i < n; ++i) l_blind = fr_add(l_blind, lagrange_at(i, x, xn));
        const F4 l_active = fr_sub(fr_sub(one, l_last), l_blind);

        // ---- expected h(x): gates, permutation argument, lookup arguments, folded with y
        F4 acc = fr_zero();
        auto fold = [&](const F4& t) { acc = fr_add(fr_mul(acc, y), t); };
        for (const Prog& g : cs.gates) fold(eval(g));
        if (cs.C) {
            fold(fr_mul(l0, fr_sub(one, z_ev[0][0])));
            const F4 zl = z_ev[cs.C - 1][0];
            fold(fr_mul(l_last, fr_sub(fr_mul(zl, zl), zl)));
            for (uint32_t c = 1; c < cs.C; ++c) fold(fr_mul(l0, fr_sub(z_ev[c][0], z_ev[c - 1][2])));
            F4 dj = fr_mul(beta, x);       // beta * delta^j * x
            for (uint32_t c = 0; c < cs.C; ++c) {
                F4 left = z_ev[c][1], right = z_ev[c][0];
                for (uint32_t j = c * cs.chunk; j < std::min(cs.P, (c + 1) * cs.chunk); ++j) {
                    const F4 v = col_eval(cs.perm_cols[j].first, cs.perm_cols[j].second, 0);
                    left = fr_mul(left, fr_add(fr_add(v, fr_mul(beta, sigma_ev[j])), gamma));
                    right = fr_mul(right, fr_add(fr_add(v, dj), gamma));
                    dj = fr_mul(dj, delta);
                }
                fold(fr_mul(l_active, fr_sub(left, right)));
            }
        }
        auto compress = [&](const std::vector<Prog>& ps) {
            F4 a = fr_zero();
            for (const Prog& p : ps) a = fr_add(fr_mul(a, theta), eval(p));
            return fr_add(a, beta);
        };
        for (uint32_t l = 0; l < cs.L; ++l) {       // mv_lookup::verifier::Evaluated::expressions
            const auto& lk = cs.lookups[l];
            const F4 p0 = lk_ev[l][0], p1 = lk_ev[l][1], me = lk_ev[l][2];
            F4 prod_fi = one, sum_inv = fr_zero();
            std::vector<F4> f;
            for (const auto& ins : lk.inputs) { f.push_back(compress(ins)); prod_fi = fr_mul(prod_fi, f.back()); }
            const F4 tau = compress(lk.tables);
            if (fr_is_zero(prod_fi) || fr_is_zero(tau)) return;      // batch_invert / invert().unwrap() of the Rust verifier
            for (const F4& v : f) sum_inv = fr_add(sum_inv, fr_inv(v));
            const F4 tp = fr_mul(tau, prod_fi);
            const F4 lhs = fr_mul(tp, fr_sub(p1, p0));
            const F4 rhs = fr_mul(tp, fr_sub(sum_inv, fr_mul(me, fr_inv(tau))));
            fold(fr_mul(l0, p0));
            fold(fr_mul(l_last, p0));
            fold(fr_mul(fr_sub(lhs, rhs), l_active));
        }
        if (missing) return;                        // a program reads what the proof does not open
        const F4 h_eval = fr_mul(acc, fr_inv(fr_sub(xn, one)));

        // ---- the multi-open queries, in halo2's order: advice, permutation products, lookups, fixed, sigma, h, random.
        // A polynomial is a base index: [0, M) proof points, M + i the key's commitment i; H_POLY the combination
        // sum_i xn^i h_i of the quotient pieces.
        const uint32_t H_POLY = 0xFFFFFFFFu;
        struct Q { uint32_t poly; int64_t rot; F4 ev; };
        std::vector<Q> qs;
        for (size_t q = 0; q < cs.adv_q.size(); ++q) qs.push_back({adv_com[cs.adv_q[q].idx], cs.adv_q[q].rot, adv_ev[q]});
        for (uint32_t c = 0; c < cs.C; ++c) { qs.push_back({z_com[c], 0, z_ev[c][0]}); qs.push_back({z_com[c], 1, z_ev[c][1]}); }
        for (uint32_t c = cs.C > 1 ? cs.C - 1 : 0; c-- > 0;) qs.push_back({z_com[c], -(int64_t)cs.bf - 1, z_ev[c][2]});
        for (uint32_t l = 0; l < cs.L; ++l) {
            qs.push_back({phi_com[l], 0, lk_ev[l][0]});
            qs.push_back({phi_com[l], 1, lk_ev[l][1]});
            qs.push_back({m_com[l], 0, lk_ev[l][2]});
        }
        for (size_t q = 0; q < cs.fix_q.size(); ++q) qs.push_back({M + cs.fix_q[q].idx, cs.fix_q[q].rot, fix_ev[q]});
        for (uint32_t j = 0; j < cs.P; ++j) qs.push_back({M + cs.F + j, 0, sigma_ev[j]});
        qs.push_back({H_POLY, 0, h_eval});
        qs.push_back({random_com, 0, random_ev});

        out->right.assign(G + 1, fr_zero());
        out->left.assign(M, fr_zero());
        std::vector<F4> xn_pow(cs.d - 1);
        xn_pow[0] = one;
        for (uint32_t i = 1; i + 1 < cs.d; ++i) xn_pow[i] = fr_mul(xn_pow[i - 1], xn);
        auto add = [&](std::vector<F4>& v, uint32_t poly, const F4& c) {
            if (poly == H_POLY) { for (uint32_t i = 0; i + 1 < cs.d; ++i) v[h0 + i] = fr_add(v[h0 + i], fr_mul(c, xn_pow[i])); }
            else v[poly] = fr_add(v[poly], c);
        };
        if (multiopen == ZK_MULTIOPEN_SHPLONK) {
            // construct_intermediate_sets: polynomials in order of first appearance with their points (first appearance), rotation
            // sets keyed by the sorted point set in order of first appearance
            std::vector<uint32_t> polys;
            std::vector<std::vector<int64_t>> prots;
            for (const Q& q : qs) {
                auto it = std::find(polys.begin(), polys.end(), q.poly);
                if (it == polys.end()) { polys.push_back(q.poly); prots.push_back({q.rot}); continue; }
                auto& pr = prots[it - polys.begin()];
                if (std::find(pr.begin(), pr.end(), q.rot) == pr.end()) pr.push_back(q.rot);
            }
            auto sorted_points = [&](const std::vector<int64_t>& rots) {
                std::vector<std::pair<F4, int64_t>> v;
                for (int64_t r : rots) v.push_back({point(r), r});
                std::sort(v.begin(), v.end(), [](const auto& a, const auto& b) { return fr_canon_less(a.first, b.first); });
                return v;
            };
            struct Set { std::vector<std::pair<F4, int64_t>> pts; std::vector<uint32_t> members; };
            std::vector<Set> sets;
            for (size_t i = 0; i < polys.size(); ++i) {
                auto key = sorted_points(prots[i]);
                bool placed = false;
                for (Set& s : sets) {
                    if (s.pts.size() != key.size()) continue;
                    bool same = true;
                    for (size_t t = 0; t < key.size() && same; ++t) same = fr_eq(s.pts[t].first, key[t].first);
                    if (same) { s.members.push_back(polys[i]); placed = true; break; }
                }
                if (!placed) sets.push_back({key, {polys[i]}});
            }
            std::vector<int64_t> all_rots;
            for (const Q& q : qs) all_rots.push_back(q.rot);
            std::vector<std::pair<F4, int64_t>> super_pts;
            for (auto& p : sorted_points(all_rots)) if (super_pts.empty() || !fr_eq(super_pts.back().first, p.first)) super_pts.push_back(p);
            auto eval_of = [&](uint32_t poly, int64_t rot) {
                for (const Q& q : qs) if (q.poly == poly && rot_mod(q.rot, n) == rot_mod(rot, n)) return q.ev;
                return fr_zero();
            };
            const F4 sy = tr.squeeze(), v = tr.squeeze();
            const uint32_t h1 = read_point();
            const F4 uu = tr.squeeze();
            const uint32_t h2 = read_point();
            if (tr.err) return;
            F4 z_0 = fr_zero(), z_0_diff_inv = fr_zero(), r_outer = fr_zero(), vpow = one;
            for (size_t i = 0; i < sets.size(); ++i) {
                const Set& s = sets[i];
                F4 z_diff = one;
                for (const auto& sp_ : super_pts) {
                    bool in = false;
                    for (const auto& p : s.pts) in = in || fr_eq(p.first, sp_.first);
                    if (!in) z_diff = fr_mul(z_diff, fr_sub(uu, sp_.first));
                }
                if (i == 0) {
                    z_0 = one;
                    for (const auto& p : s.pts) z_0 = fr_mul(z_0, fr_sub(uu, p.first));
                    z_0_diff_inv = fr_inv(z_diff);
                    z_diff = one;
                } else {
                    z_diff = fr_mul(z_diff, z_0_diff_inv);
                }
                // Lagrange basis of the set's points at u: r_x(u) = sum_a e_a prod_{c != a} (u - x_c) / (x_a - x_c)
                std::vector<F4> basis(s.pts.size());
                for (size_t a = 0; a < s.pts.size(); ++a) {
                    F4 num = one, den = one;
                    for (size_t c = 0; c < s.pts.size(); ++c) {
                        if (c == a) continue;
                        num = fr_mul(num, fr_sub(uu, s.pts[c].first));
                        den = fr_mul(den, fr_sub(s.pts[a].first, s.pts[c].first));
                    }
                    basis[a] = fr_mul(num, fr_inv(den));
                }
                const F4 scale = fr_mul(vpow, z_diff);
                F4 r_inner = fr_zero(), ypow = one;
                for (uint32_t poly : s.members) {
                    F4 r_u = fr_zero();
                    for (size_t a = 0; a < s.pts.size(); ++a) r_u = fr_add(r_u, fr_mul(eval_of(poly, s.pts[a].second), basis[a]));
                    r_inner = fr_add(r_inner, fr_mul(ypow, r_u));
                    add(out->right, poly, fr_mul(ypow, scale));
                    ypow = fr_mul(ypow, sy);
                }
                r_outer = fr_add(r_outer, fr_mul(r_inner, scale));
                vpow = fr_mul(vpow, v);
            }
            out->right[G] = fr_add(out->right[G], fr_neg(r_outer));
            out->right[h1] = fr_add(out->right[h1], fr_neg(z_0));
            out->right[h2] = fr_add(out->right[h2], uu);
            out->left[h2] = fr_add(out->left[h2], one);
        } else {
            // VerifierGWC: queries grouped by point in order of first appearance
            const F4 v = tr.squeeze();
            std::vector<uint64_t> grp_rot;
            std::vector<std::vector<size_t>> grp;
            for (size_t q = 0; q < qs.size(); ++q) {
                const uint64_t r = rot_mod(qs[q].rot, n);
                auto it = std::find(grp_rot.begin(), grp_rot.end(), r);
                if (it == grp_rot.end()) { grp_rot.push_back(r); grp.push_back({q}); }
                else grp[it - grp_rot.begin()].push_back(q);
            }
            std::vector<uint32_t> wit;
            for (size_t g = 0; g < grp.size(); ++g) wit.push_back(read_point());
            const F4 uu = tr.squeeze();
            if (tr.err) return;
            F4 upow = one;
            for (size_t g = 0; g < grp.size(); ++g) {
                F4 vpow = one, eb = fr_zero();
                for (size_t q : grp[g]) {
                    add(out->right, qs[q].poly, fr_mul(upow, vpow));
                    eb = fr_add(eb, fr_mul(vpow, qs[q].ev));
                    vpow = fr_mul(vpow, v);
                }
                out->right[G] = fr_add(out->right[G], fr_neg(fr_mul(upow, eb)));
                out->right[wit[g]] = fr_add(out->right[wit[g]], fr_mul(upow, point((int64_t)grp_rot[g])));
                out->left[wit[g]] = fr_add(out->left[wit[g]], upow);
                upow = fr_mul(upow, uu);
            }
        }
        if (pj != M) return;
        out->ok = true;
    }
};

struct DevMem {
    void* p = nullptr;
    ~DevMem() { if (p) (void)hipFree(p); }
    bool alloc(size_t bytes) { return hipMalloc(&p, bytes ? bytes : 1) == hipSuccess; }
};

// ZK_VERIFY_TRACE=1: wall-clock per step of zk_verify_proofs (setup, decode, replay, msm, pairing) and zk_verify_accumulators (setup,
// decode, replay, carried, gather, msm_seg -- msm_loop under ZK_ACC_MSM_LOOP=1) on stderr (tools/verify_time.py, tools/acc_time.py read it)
struct VerifyTrace {
    bool on = getenv("ZK_VERIFY_TRACE") != nullptr;
    std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    void mark(const char* what) {
        if (!on) return;
        const auto t1 = std::chrono::steady_clock::now();
        fprintf(stderr, "[zk verify] %-10s %10.3f ms\n", what, std::chrono::duration<double, std::milli>(t1 - t0).count());
        t0 = t1;
    }
};

// What zk_verify_proofs and zk_verify_accumulators share: every point of every proof decoded on the device in one launch
// (the key's commitments and the generator follow them in d_bases), every proof replayed on the host.
struct Front {
    Layout lo;
    uint32_t M = 0, KP = 0;
    size_t npts = 0, nbases = 0;
    DevMem d_enc, d_bases;
    std::vector<G1Affine> pts, tail;       // decoded proof points; fixed and sigma commitments, then the generator
    std::vector<uint8_t> bad;
    std::vector<ProofWork> work;
};

int check_verify_args(zk_ctx* ctx, const zk_vk* vk, size_t count, const void* const* const* h_instances, const uint32_t* const* h_instance_lens,
                      const void* const* h_proofs, const size_t* h_proof_lens, int transcript_kind, int multiopen) {
    ZK_REQUIRE(ctx, vk && h_proofs && h_proof_lens, "null pointer");
    ZK_REQUIRE(ctx, count >= 1, "no proofs");
    ZK_REQUIRE(ctx, !vk->I || (h_instances && h_instance_lens), "null instance pointer");
    ZK_REQUIRE(ctx, transcript_kind == ZK_TRANSCRIPT_BLAKE2B || transcript_kind == ZK_TRANSCRIPT_POSEIDON || transcript_kind == ZK_TRANSCRIPT_EVM, "unknown transcript kind");
    ZK_REQUIRE(ctx, multiopen == ZK_MULTIOPEN_GWC || multiopen == ZK_MULTIOPEN_SHPLONK, "unknown multi-open scheme");
    for (size_t b = 0; b < count; ++b) {
        ZK_REQUIRE(ctx, h_proofs[b] || !h_proof_lens[b], "null proof");
        if (vk->I) {
            ZK_REQUIRE(ctx, h_instances[b] && h_instance_lens[b], "null instance pointer");
            for (uint32_t i = 0; i < vk->I; ++i) ZK_REQUIRE(ctx, h_instances[b][i] || !h_instance_lens[b][i], "null instance column");
        }
    }
    return ZK_OK;
}

// f.lo is set.  A proof whose length is not the layout's is not looked at: its points decode from zero bytes and its work stays !ok.
int decode_and_replay(zk_ctx* ctx, const zk_vk* vk, size_t count, const void* const* const* h_instances, const uint32_t* const* h_instance_lens,
                      const void* const* h_proofs, const size_t* h_proof_lens, int transcript_kind, int multiopen, VerifyTrace& trace, Front& f) {
    const Layout& lo = f.lo;
    const uint32_t M = f.M = lo.points(), KP = f.KP = vk->F + vk->P;
    // ---- every point of every proof: gathered, decoded in one launch; the key's commitments and the generator follow them,
    // so the MSM reads its bases where the decoder left them
    const size_t npts = f.npts = count * M, enc_bytes = npts * lo.point_len;
    f.nbases = npts + KP + 1;
    if (!f.d_enc.alloc(enc_bytes + npts) || !f.d_bases.alloc(f.nbases * sizeof(G1Affine))) {
        (void)hipGetLastError();
        return ctx->fail(ZK_ERR_OOM, "verifier: device allocation failed");
    }
    std::vector<uint8_t> enc(enc_bytes);
    for (size_t b = 0; b < count; ++b) {
        if (h_proof_lens[b] != lo.len()) continue;
        for (uint32_t j = 0; j < M; ++j) memcpy(&enc[(b * M + j) * lo.point_len], (const uint8_t*)h_proofs[b] + lo.point_offset(j), lo.point_len);
    }
    std::vector<G1Affine>& tail = f.tail;
    tail.resize(KP + 1);
    for (uint32_t i = 0; i < vk->F; ++i) tail[i] = vk->fixed_com[i];
    for (uint32_t i = 0; i < vk->P; ++i) tail[vk->F + i] = vk->sigma_com[i];
    {   // the generator (1, 2)
        F4 gx = fone<FqC>(), gy = fadd<FqC>(gx, gx);
        memcpy(&tail[KP].x, gx.l, 32);
        memcpy(&tail[KP].y, gy.l, 32);
    }
    uint8_t* d_in = (uint8_t*)f.d_enc.p;
    uint8_t* d_bad_at = d_in + enc_bytes;
    G1Affine* bases = (G1Affine*)f.d_bases.p;
    std::vector<G1Affine>& pts = f.pts;
    std::vector<uint8_t>& bad = f.bad;
    pts.resize(npts);
    bad.resize(npts);
    trace.mark("setup");
    {
        DevMem d_cnt;
        if (!d_cnt.alloc(4)) { (void)hipGetLastError(); return ctx->fail(ZK_ERR_OOM, "verifier: device allocation failed"); }
        ZK_HIP(ctx, hipMemsetAsync(d_cnt.p, 0, 4, ctx->stream));
        if (enc_bytes) ZK_HIP(ctx, hipMemcpyAsync(d_in, enc.data(), enc_bytes, hipMemcpyHostToDevice, ctx->stream));
        ZK_HIP(ctx, hipMemcpyAsync(bases + npts, tail.data(), tail.size() * sizeof(G1Affine), hipMemcpyHostToDevice, ctx->stream));
        if (int rc = g1_decode_run(ctx, d_in, transcript_kind == ZK_TRANSCRIPT_EVM ? G1_ENC_BE_XY : G1_ENC_COMPRESSED, bases, npts, (uint32_t*)d_cnt.p, d_bad_at)) return rc;
        if (npts) {
            ZK_HIP(ctx, hipMemcpyAsync(pts.data(), bases, npts * sizeof(G1Affine), hipMemcpyDeviceToHost, ctx->stream));
            ZK_HIP(ctx, hipMemcpyAsync(bad.data(), d_bad_at, npts, hipMemcpyDeviceToHost, ctx->stream));
        }
        ZK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    }
    trace.mark("decode");

    // ---- transcript replay, one proof per task, up to 16 threads
    Replay rp{*vk, lo, transcript_kind, multiopen, fr_from_device(fr_root_of_unity(vk->k)), host::fr_pow(host::fr_from_u64(7), 1ull << 28), M, M + KP};
    std::vector<ProofWork>& work = f.work;
    work.resize(count);
    {
        std::atomic<size_t> next{0};
        auto worker = [&]() {
            for (size_t b; (b = next.fetch_add(1)) < count;) {
                if (h_proof_lens[b] != lo.len()) continue;
                const F4* const* inst = vk->I ? (const F4* const*)h_instances[b] : nullptr;
                const uint32_t* lens = vk->I ? h_instance_lens[b] : nullptr;
                rp.run((const uint8_t*)h_proofs[b], pts.data() + b * M, bad.data() + b * M, inst, lens, &work[b]);
            }
        };
        const size_t nthreads = std::min<size_t>(count, 16);
        std::vector<std::thread> pool;
        for (size_t t = 1; t < nthreads; ++t) pool.emplace_back(worker);
        worker();
        for (auto& t : pool) t.join();
    }
    trace.mark("replay");
    return ZK_OK;
}

}  // namespace

extern "C" {

// keygen_vk's product without the columns: the constraint system of a key blob (version 3 or 4: the same key), the key's F fixed and P sigma commitments,
// vk.transcript_repr.  Host only.
int zk_vk_create(const void* h_cs_blob, size_t len, const void* h_commitments, size_t num_commitments, const void* h_vk_repr_fr32, zk_vk** out) {
    if (!h_cs_blob || !h_vk_repr_fr32 || !out || (!h_commitments && num_commitments)) return ZK_ERR_INVALID_ARG;
    std::unique_ptr<zk_vk> vk(new zk_vk());
    Reader r{(const uint8_t*)h_cs_blob, len};
    std::string err;
    if (int rc = parse_cs(r, vk.get(), len, false, &err)) return rc;
    // the constraint-system part alone, or the whole key blob (its F + P columns are not read); nothing else may follow
    if (r.left && vk->version == 3u && r.left != ((size_t)vk->F + vk->P) * ((size_t)32 << vk->k)) return ZK_ERR_INVALID_ARG;
    if (r.left && vk->version == 4u) {           // F cell widths, F payloads of n cells, P x n mapping pairs
        size_t want = (size_t)vk->P * ((size_t)8 << vk->k);
        for (uint32_t i = 0; i < vk->F; ++i) {
            const uint32_t w = r.u32();
            if (!r.ok || (w != 1 && w != 2 && w != 4 && w != 8 && w != 16 && w != 32)) return ZK_ERR_INVALID_ARG;
            want += (size_t)w << vk->k;
        }
        if (r.left != want) return ZK_ERR_INVALID_ARG;
    }
    if (num_commitments != (size_t)vk->F + vk->P) return ZK_ERR_INVALID_ARG;
    const G1Affine* c = (const G1Affine*)h_commitments;
    for (size_t i = 0; i < num_commitments; ++i) {
        // the key's own points: canonical limbs, on the curve (or the identity)
        F4 x, y;
        memcpy(x.l, &c[i].x, 32);
        memcpy(y.l, &c[i].y, 32);
        if (geq_mod<FqC>(x.l) || geq_mod<FqC>(y.l)) return ZK_ERR_INVALID_ARG;
        if (!c[i].is_identity() && !fr_eq(q_mul(y, y), q_add(q_mul(q_mul(x, x), x), q_from_u64(3)))) return ZK_ERR_INVALID_ARG;
        (i < vk->F ? vk->fixed_com : vk->sigma_com).push_back(c[i]);
    }
    memcpy(vk->vk_repr.l, h_vk_repr_fr32, 32);
    *out = vk.release();
    return ZK_OK;
}

void zk_vk_destroy(zk_vk* vk) { delete vk; }

int zk_vk_proof_len(const zk_vk* vk, int transcript_kind, int multiopen, size_t* len) {
    if (!vk || !len) return ZK_ERR_INVALID_ARG;
    if (transcript_kind != ZK_TRANSCRIPT_BLAKE2B && transcript_kind != ZK_TRANSCRIPT_POSEIDON && transcript_kind != ZK_TRANSCRIPT_EVM) return ZK_ERR_INVALID_ARG;
    if (multiopen != ZK_MULTIOPEN_GWC && multiopen != ZK_MULTIOPEN_SHPLONK) return ZK_ERR_INVALID_ARG;
    *len = layout_of(*vk, transcript_kind, multiopen).len();
    return ZK_OK;
}

// Shape of a verifying key: the 16 words of zk_pk_shape, derived from the constraint system alone.
int zk_vk_shape(const zk_vk* vk, uint32_t* out16) {
    if (!vk || !out16) return ZK_ERR_INVALID_ARG;
    const zk_vk& p = *vk;
    const uint32_t evals = (uint32_t)p.adv_q.size() + (uint32_t)p.fix_q.size() + 1 + p.P + (p.C ? 3 * p.C - 1 : 0) + 3 * p.L;
    const uint32_t v[16] = {p.k, p.d, p.ext_k, p.F, p.A, p.I, p.P, p.C, p.L, p.num_phases, (uint32_t)p.chal_phase.size(), p.bf,
                            (uint32_t)p.adv_q.size(), (uint32_t)p.fix_q.size(), p.A + 2 * p.L + p.C + 1 + (p.d - 1), evals};
    memcpy(out16, v, sizeof v);
    return ZK_OK;
}

int zk_verify_proofs(zk_ctx* ctx, const zk_vk* vk, size_t count, const void* const* const* h_instances, const uint32_t* const* h_instance_lens,
                     const void* const* h_proofs, const size_t* h_proof_lens, int transcript_kind, int multiopen, const void* g2_128, const void* s_g2_128, int* ok) {
    if (!ctx) return ZK_ERR_INVALID_ARG;
    ZK_REQUIRE(ctx, ok && g2_128 && s_g2_128, "null pointer");
    if (int rc = check_verify_args(ctx, vk, count, h_instances, h_instance_lens, h_proofs, h_proof_lens, transcript_kind, multiopen)) return rc;
    *ok = 0;
    VerifyTrace trace;
    Front f;
    f.lo = layout_of(*vk, transcript_kind, multiopen);
    // a proof of the wrong length is a reject before anything else is looked at
    for (size_t b = 0; b < count; ++b) if (h_proof_lens[b] != f.lo.len()) return ZK_OK;
    if (int rc = decode_and_replay(ctx, vk, count, h_instances, h_instance_lens, h_proofs, h_proof_lens, transcript_kind, multiopen, trace, f)) return rc;
    const uint32_t M = f.M, KP = f.KP;
    const size_t npts = f.npts, nbases = f.nbases;
    const std::vector<G1Affine>&pts = f.pts, &tail = f.tail;
    const std::vector<ProofWork>& work = f.work;
    G1Affine* bases = (G1Affine*)f.d_bases.p;
    for (const ProofWork& w : work) if (!w.ok) return ZK_OK;
    DevMem d_scalars;
    if (!d_scalars.alloc(2 * nbases * sizeof(Fr))) {
        (void)hipGetLastError();
        return ctx->fail(ZK_ERR_OOM, "verifier: device allocation failed");
    }

    // ---- one DualMSM for the batch: proof b weighted by rho^b, rho from Blake2b over the key, every proof and every instance
    F4 rho = fr_one();
    if (count > 1) {
        Blake2b h;
        h.init("zkmi355-VerifyRho");
        h.update(vk->vk_repr.l, 32);
        for (size_t b = 0; b < count; ++b) {
            const uint64_t len = h_proof_lens[b];
            h.update(&len, 8);
            h.update(h_proofs[b], len);
            for (uint32_t i = 0; i < vk->I; ++i) {
                const uint64_t il = h_instance_lens[b][i];
                h.update(&il, 8);
                if (il) h.update(h_instances[b][i], il * 32);
            }
        }
        uint8_t dg[64];
        h.finalize(dg);
        rho = fr_from_uniform(dg);
    }
    std::vector<F4> sc(2 * nbases, fr_zero());       // [right over every base | left over every base]
    F4* right = sc.data();
    F4* left = sc.data() + nbases;
    F4 rp_b = fr_one();
    for (size_t b = 0; b < count; ++b) {
        const ProofWork& w = work[b];
        for (uint32_t j = 0; j < M; ++j) {
            if (pts[b * M + j].is_identity()) continue;        // (Blake2b only) nothing to add
            right[b * M + j] = fr_mul(rp_b, w.right[j]);
            left[b * M + j] = fr_mul(rp_b, w.left[j]);
        }
        for (uint32_t t = 0; t <= KP; ++t) right[npts + t] = fr_add(right[npts + t], fr_mul(rp_b, w.right[M + t]));
        rp_b = fr_mul(rp_b, rho);
    }
    for (uint32_t t = 0; t < KP; ++t) if (tail[t].is_identity()) right[npts + t] = fr_zero();
    G1Affine acc[2];
    ZK_HIP(ctx, hipMemcpyAsync(d_scalars.p, sc.data(), sc.size() * sizeof(F4), hipMemcpyHostToDevice, ctx->stream));
    if (int rc = zk_msm_g1(ctx, d_scalars.p, bases, nbases, &acc[0])) return rc;
    if (int rc = zk_msm_g1(ctx, (const F4*)d_scalars.p + nbases, bases, npts, &acc[1])) return rc;
    if (int rc = zk_ctx_sync(ctx)) return rc;
    trace.mark("msm");

    // e(-right, [1]) * e(left, [s]) == 1
    G1Affine neg_right = acc[0];
    if (!neg_right.is_identity()) {
        F4 yy;
        memcpy(yy.l, &neg_right.y, 32);
        yy = q_neg(yy);
        memcpy(&neg_right.y, yy.l, 32);
    }
    const G1Affine P[2] = {neg_right, acc[1]};
    G2Affine Q[2];
    memcpy(&Q[0], g2_128, 128);
    memcpy(&Q[1], s_g2_128, 128);
    *ok = pairing_check(P, Q, 2) ? 1 : 0;
    trace.mark("pairing");
    return ZK_OK;
}

// PlonkSuccinctVerifier::verify for a batch, as extract_accumulators_and_proof runs it on the child snarks of an aggregation
// layer [REF aggregator/src/core.rs:48-107]: per proof the KZG accumulator of its own openings (lhs = MSM of `right`, rhs = MSM of
// `left`, Replay::run's normalisation) and the accumulators its instances carry, NO pairing.  The statement followed is
// oracle/snark_verifier.py:succinct_verify.  Decode and replay are zk_verify_proofs'; the 2 * count coefficient vectors then go
// through ONE segmented MSM (zero coefficients and identity points dropped, so `left` is one to a few terms).
// ZK_ACC_MSM_LOOP=1 (measurement only) sends the same vectors through 2 * count zk_msm_g1 calls instead, the only route there
// was before zk_msm_g1_segments.
int zk_verify_accumulators(zk_ctx* ctx, const zk_vk* vk, size_t count, const void* const* const* h_instances, const uint32_t* const* h_instance_lens,
                           const void* const* h_proofs, const size_t* h_proof_lens, int transcript_kind, int multiopen, const uint32_t* acc_indices, size_t num_prior,
                           void* h_lhs, void* h_rhs, int* ok) {
    if (!ctx) return ZK_ERR_INVALID_ARG;
    ZK_REQUIRE(ctx, ok && h_lhs && h_rhs && (acc_indices || !num_prior), "null pointer");
    if (int rc = check_verify_args(ctx, vk, count, h_instances, h_instance_lens, h_proofs, h_proof_lens, transcript_kind, multiopen)) return rc;
    const size_t per = 1 + num_prior;
    G1Affine* lhs = (G1Affine*)h_lhs;
    G1Affine* rhs = (G1Affine*)h_rhs;
    memset(h_lhs, 0, count * per * sizeof(G1Affine));
    memset(h_rhs, 0, count * per * sizeof(G1Affine));
    for (size_t b = 0; b < count; ++b) ok[b] = 0;
    VerifyTrace trace;
    Front f;
    f.lo = layout_of(*vk, transcript_kind, multiopen);
    if (int rc = decode_and_replay(ctx, vk, count, h_instances, h_instance_lens, h_proofs, h_proof_lens, transcript_kind, multiopen, trace, f)) return rc;
    const uint32_t M = f.M, KP = f.KP;

    // ---- the accumulators carried in the instances: 12 limbs each, cell (column, row) per limb
    for (size_t b = 0; b < count; ++b) {
        bool good = f.work[b].ok;
        for (size_t a = 0; a < num_prior && good; ++a) {
            F4 limbs[12];
            for (int l = 0; l < 12 && good; ++l) {
                const uint32_t col = acc_indices[(a * 12 + l) * 2], row = acc_indices[(a * 12 + l) * 2 + 1];
                good = col < vk->I && row < h_instance_lens[b][col];
                if (good) memcpy(limbs[l].l, (const uint8_t*)h_instances[b][col] + (size_t)32 * row, 32);
            }
            int dec = 0;
            if (good) (void)zk_host_accumulator_from_limbs(limbs, &lhs[b * per + 1 + a], &rhs[b * per + 1 + a], &dec);
            good = good && dec;
        }
        ok[b] = good ? 1 : 0;
    }
    trace.mark("carried");

    // ---- segment 2b: `right` over [the proof's points | the key's commitments | the generator]; segment 2b + 1: `left` over
    // the proof's points.  A rejected proof has two empty segments.
    std::vector<uint32_t> off(2 * count + 1, 0);
    std::vector<F4> sc;
    std::vector<G1Affine> bs;
    for (size_t b = 0; b < count; ++b) {
        if (ok[b]) {
            const ProofWork& w = f.work[b];
            auto term = [&](const F4& c, const G1Affine& p) { if (!fr_is_zero(c) && !p.is_identity()) { sc.push_back(c); bs.push_back(p); } };
            for (uint32_t j = 0; j < M; ++j) term(w.right[j], f.pts[b * M + j]);
            for (uint32_t t = 0; t <= KP; ++t) term(w.right[M + t], f.tail[t]);
            off[2 * b + 1] = (uint32_t)sc.size();
            for (uint32_t j = 0; j < M; ++j) term(w.left[j], f.pts[b * M + j]);
        } else {
            off[2 * b + 1] = (uint32_t)sc.size();
        }
        off[2 * b + 2] = (uint32_t)sc.size();
    }
    std::vector<G1Affine> sums(2 * count);
    if (!sc.empty()) {
        DevMem d_sc, d_bs;
        if (!d_sc.alloc(sc.size() * sizeof(F4)) || !d_bs.alloc(bs.size() * sizeof(G1Affine))) {
            (void)hipGetLastError();
            return ctx->fail(ZK_ERR_OOM, "verifier: device allocation failed");
        }
        ZK_HIP(ctx, hipMemcpyAsync(d_sc.p, sc.data(), sc.size() * sizeof(F4), hipMemcpyHostToDevice, ctx->stream));
        ZK_HIP(ctx, hipMemcpyAsync(d_bs.p, bs.data(), bs.size() * sizeof(G1Affine), hipMemcpyHostToDevice, ctx->stream));
        trace.mark("gather");
        const char* loop = getenv("ZK_ACC_MSM_LOOP");
        if (loop && atoi(loop) == 1) {
            for (size_t s = 0; s < 2 * count; ++s)
                if (int rc = zk_msm_g1(ctx, (const F4*)d_sc.p + off[s], (const G1Affine*)d_bs.p + off[s], off[s + 1] - off[s], &sums[s])) return rc;
            if (int rc = zk_ctx_sync(ctx)) return rc;
            trace.mark("msm_loop");
        } else {
            if (int rc = msm_segments_run(ctx, (const Fr*)d_sc.p, (const G1Affine*)d_bs.p, off.data(), 2 * count, sums.data())) return rc;
            trace.mark("msm_seg");
        }
    }
    for (size_t b = 0; b < count; ++b) {
        if (!ok[b]) {       // nothing of a rejected proof goes out, carried accumulators that did decode included
            memset((void*)&lhs[b * per], 0, per * sizeof(G1Affine));
            memset((void*)&rhs[b * per], 0, per * sizeof(G1Affine));
            continue;
        }
        lhs[b * per] = sums[2 * b];
        rhs[b * per] = sums[2 * b + 1];
    }
    return ZK_OK;
}

}  // extern "C"

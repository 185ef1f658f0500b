// parse_cs (cs.hpp).  Host only: what works on constraint systems alone (verifying key, quotient planner) links without the prover.
#include <algorithm>
#include <cstdio>

#include "../../include/zkmi355.h"
#include "cs.hpp"

using namespace zk::cs;

// The constraint-system part of a key blob (everything before the column data) into `cs`: shape, phases, query lists,
// permutation columns, constants, gate and lookup programs -- with every count checked against what the blob can hold and the
// declared degree against what the programs need.  No device, no SRS (zk_pk_create goes on from here; zk_vk_create and the host-only hooks stop here).
int zk::cs::parse_cs(Reader& r, ConstraintSystem* pk, size_t blob_len, bool with_columns, std::string* err) {
    char msg[256];
    auto fail = [&](int code, const char* fmt, auto... args) { snprintf(msg, sizeof msg, fmt, args...); *err = msg; return code; };
    if (r.u32() != 0x4B505A4Bu) return fail(ZK_ERR_INVALID_ARG, "pk blob: bad magic");
    const uint32_t version = r.u32();
    if (version != 3u && version != 4u) return fail(ZK_ERR_INVALID_ARG, "pk blob: unsupported version %u (this library reads versions 3 and 4)", version);
    pk->version = version;
    pk->k = r.u32(); pk->bf = r.u32(); pk->d = r.u32(); pk->F = r.u32(); pk->A = r.u32(); pk->I = r.u32(); pk->P = r.u32(); pk->L = r.u32();
    const uint32_t ngates = r.u32(), nconsts = r.u32();
    // halo2: cs.degree() >= 3 (the permutation argument); the extended domain has at most 2^28 rows
    if (!r.ok || pk->k < 2 || pk->k > 27 || pk->d < 3 || pk->d > 17) return fail(ZK_ERR_INVALID_ARG, "pk blob: bad header (k=%u, degree=%u)", pk->k, pk->d);
    const size_t n = (size_t)1 << pk->k;
    if (pk->bf + 2 >= n) return fail(ZK_ERR_INVALID_ARG, "pk blob: too many blinding rows");
    // every count of the header is checked against what the blob can hold before anything is sized by it
    if ((size_t)pk->A * 4 > r.left || (size_t)pk->P * 8 > r.left || (size_t)nconsts * 32 > r.left || (size_t)ngates * 4 > r.left || (size_t)pk->L * 8 > r.left ||
        (with_columns && version == 3u && ((size_t)pk->F + pk->P) > r.left / (n * 32)) ||
        (with_columns && version == 4u && ((size_t)pk->F > r.left / (n + 4) || (size_t)pk->P > (r.left - (size_t)pk->F * (n + 4)) / (n * 8))) ||      // a width word and at least one byte per fixed cell, eight per mapping pair
        pk->A > 0xFFFFFFu || pk->F > 0xFFFFFFu || pk->I > 0xFFFFFFu)
        return fail(ZK_ERR_INVALID_ARG, "pk blob: header counts exceed the blob (%zu bytes)", blob_len);
    pk->u = (uint32_t)n - pk->bf - 1;
    pk->chunk = pk->d - 2;
    pk->C = pk->P ? (pk->P + pk->chunk - 1) / pk->chunk : 0;
    pk->ext_k = pk->k;
    while (((size_t)1 << pk->ext_k) < n * (pk->d - 1)) ++pk->ext_k;
    if (pk->ext_k > 28) return fail(ZK_ERR_INVALID_ARG, "pk blob: extended domain 2^%u exceeds the two-adicity of Fr", pk->ext_k);
    pk->adv_phase.assign(pk->A, 0);
    {   // phases: [num_challenges][A x advice phase][num_challenges x challenge phase]
        const uint32_t nch = r.count(4);
        if (nch > 4096) return fail(ZK_ERR_INVALID_ARG, "pk blob: too many challenges");
        for (uint32_t i = 0; i < pk->A && r.ok; ++i) { pk->adv_phase[i] = r.u32(); if (pk->adv_phase[i] + 1 > pk->num_phases) pk->num_phases = pk->adv_phase[i] + 1; }
        for (uint32_t i = 0; i < nch && r.ok; ++i) { pk->chal_phase.push_back(r.u32()); if (pk->chal_phase[i] + 1 > pk->num_phases) pk->num_phases = pk->chal_phase[i] + 1; }
        if (!r.ok || pk->num_phases > 16) return fail(ZK_ERR_INVALID_ARG, "pk blob: bad phase table");
    }
    // cs.advice_queries / fixed_queries / instance_queries: (column, rotation) in registration order
    r.queries(&pk->adv_q, CT_ADVICE, pk->A);
    r.queries(&pk->fix_q, CT_FIXED, pk->F);
    r.queries(&pk->inst_q, CT_INSTANCE, pk->I);
    if (!r.ok) return fail(ZK_ERR_INVALID_ARG, "pk blob: bad query lists");
    for (uint32_t i = 0; i < pk->P && r.ok; ++i) { uint32_t t = r.u32(), x = r.u32(); pk->perm_cols.push_back({t, x}); }
    for (uint32_t i = 0; i < nconsts && r.ok; ++i) { const uint8_t* b = r.bytes(32); F4 v; if (b) memcpy(v.l, b, 32); pk->consts.push_back(v); }
    for (uint32_t i = 0; i < ngates && r.ok; ++i) pk->gates.push_back(r.prog());
    for (uint32_t i = 0; i < pk->L && r.ok; ++i) {
        ConstraintSystem::Lookup lk;
        const uint32_t m = r.u32(), ninputs = r.count(4);
        if (!r.ok || m == 0 || ninputs == 0 || (size_t)m * 4 > r.left || (size_t)m * ninputs > r.left / 4) { r.ok = false; break; }
        for (uint32_t j = 0; j < m && r.ok; ++j) lk.tables.push_back(r.prog());
        for (uint32_t a = 0; a < ninputs && r.ok; ++a) {
            lk.inputs.emplace_back();
            for (uint32_t j = 0; j < m && r.ok; ++j) lk.inputs.back().push_back(r.prog());
        }
        pk->lookups.push_back(std::move(lk));
    }
    if (!r.ok) return fail(ZK_ERR_INVALID_ARG, "pk blob: truncated or malformed constraint system");
    // The degree the blob declares must cover what its own programs need (halo2 ConstraintSystem::degree:
    // permutation argument 3, mv_lookup::Argument::required_degree, every gate polynomial): with a
    // smaller one the quotient would not fit its d - 1 pieces and the proof would be rejected.
    {
        uint32_t need = 3;
        std::vector<int> tmp_deg;
        for (const Prog& g : pk->gates) {
            const int dg = program_degree(g, &tmp_deg);
            if (dg < 0) return fail(ZK_ERR_INVALID_ARG, "pk blob: malformed gate program");
            need = std::max(need, (uint32_t)dg);
        }
        for (const auto& lk : pk->lookups) {
            std::vector<int> none;
            int table_degree = 0, inputs_degree = 0;
            for (const Prog& g : lk.tables) { const int dg = program_degree(g, &none); if (dg < 0) return fail(ZK_ERR_INVALID_ARG, "pk blob: malformed lookup table program"); table_degree = std::max(table_degree, dg); }
            for (const auto& in : lk.inputs) {
                int one = 0;
                for (const Prog& g : in) { const int dg = program_degree(g, &none); if (dg < 0) return fail(ZK_ERR_INVALID_ARG, "pk blob: malformed lookup input program"); one = std::max(one, dg); }
                inputs_degree += one;
            }
            need = std::max(need, std::max((uint32_t)(3 + lk.inputs.size()), (uint32_t)(table_degree + inputs_degree + 2)));
        }
        if (pk->d < need) return fail(ZK_ERR_INVALID_ARG, "pk blob: declared degree %u is below the %u its gates and lookup arguments require", pk->d, need);
    }
    for (const auto& pc : pk->perm_cols) {          // halo2: enable_equality queries the column at Rotation::cur()
        if (pc.first > CT_INSTANCE) return fail(ZK_ERR_INVALID_ARG, "pk blob: bad permutation column type %u", pc.first);
        if (pc.first == CT_INSTANCE) continue;
        const std::vector<Query>& qs = pc.first == CT_ADVICE ? pk->adv_q : pk->fix_q;
        bool seen = false;
        for (const Query& q : qs) if (q.idx == pc.second && q.rot == 0) { seen = true; break; }
        if (!seen) return fail(ZK_ERR_INVALID_ARG, "pk blob: permutation column (%u, %u) is not queried at rotation 0", pc.first, pc.second);
    }
    return ZK_OK;
}

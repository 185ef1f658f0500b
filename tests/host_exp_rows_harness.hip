// Host harness of csrc/exp_rows.hip.hpp, the lane-free code of ZK_OP_EXP_ROWS: a stand-alone program that drives whole small inputs
// serially through exactly the functions the kernels call -- the widths and their saturating sums, the chain of every event into step
// slots, then the step slots tile by tile, lane by lane as loops -- and prints every cell.  tests/test_exp_rows_host.py builds it with
// hipcc --cuda-host-only, plain and with the address and undefined-behaviour sanitizers, and compares the output with the model.
// Every buffer is a heap block of its exact size, so a read or write outside it is an error the sanitizer reports.
//
// input:  "case <n> <count>" followed by count lines of 128 hex digits (base, then exponent, 32 little-endian bytes each)
// output: "starts ..", "needed <rows>", then per column "col <name> <hex cell> .." (n cells)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../zkevm-circuits_amd/csrc/exp_rows.hip.hpp"

using namespace zk;

static ExWord word_at(const uint8_t* p) {
    ExWord v;
    for (int k = 0; k < 4; ++k) memcpy(&v.w[k], p + 8 * k, 8);          // little-endian host
    return v;
}
static void print_cells(const char* name, int plane, const std::vector<ExCell>& v) {
    if (plane < 0) printf("col %s", name);
    else printf("col %s.%d", name, plane);
    for (const ExCell& c : v) {
        if (c.hi) printf(" %llx%016llx", (unsigned long long)c.hi, (unsigned long long)c.lo);
        else printf(" %llx", (unsigned long long)c.lo);
    }
    printf("\n");
}

static int run_case(uint64_t n, const std::vector<uint8_t>& events, uint32_t count) {
    // k_exp_widths, bc_scan, k_exp_total
    std::vector<uint32_t> starts(count + 1);
    uint32_t run = 0;
    uint64_t steps_sum = 0;
    for (uint32_t e = 0; e <= count; ++e) {
        starts[e] = run;
        if (e == count) break;
        const uint32_t steps = ex_steps(word_at(events.data() + (size_t)e * EX_EVENT_BYTES + 32));
        steps_sum += steps;
        run = bc_sat_add(run, ex_rows_of(steps, (uint32_t)n), (uint32_t)n);
    }
    printf("starts");
    for (uint32_t s : starts) printf(" %u", s);
    printf("\nneeded %llu\n", (unsigned long long)(EX_STEP_ROWS * steps_sum + EX_UNUSABLE));
    // k_exp_chain: slot -> d, and whether it was written
    std::vector<ExWord> slots(n / EX_STEP_ROWS + 1);
    std::vector<uint8_t> written(slots.size(), 0);
    for (uint32_t e = 0; e < count; ++e) {
        const uint64_t start = starts[e];
        if (!ex_kept(start, n)) continue;
        const ExWord x = word_at(events.data() + (size_t)e * EX_EVENT_BYTES + 32);
        if (ex_lt2(x)) continue;
        const ExWord base = word_at(events.data() + (size_t)e * EX_EVENT_BYTES);
        ExChain c = ex_chain_begin(base, x);
        while (c.j) {
            ex_chain_next(c, base, x);
            const uint64_t o = start + (uint64_t)EX_STEP_ROWS * c.j;
            if (ex_kept(o, n)) {
                slots.at(o / EX_STEP_ROWS) = c.acc;
                written.at(o / EX_STEP_ROWS) = 1;
            }
        }
    }
    // k_exp_rows
    std::vector<ExCell> is_last(n), base_limb(n), exponent(n), out(n), cols[2][4], u64[2][4], u128[2][8];
    for (int chip = 0; chip < 2; ++chip) {
        for (auto& v : cols[chip]) v.resize(n);
        for (auto& v : u64[chip]) v.resize(n);
        for (auto& v : u128[chip]) v.resize(n);
    }
    for (uint64_t r0 = 0; r0 < n; r0 += EX_TILE) {
        const uint32_t rows = n - r0 < EX_TILE ? (uint32_t)(n - r0) : EX_TILE;
        const uint32_t lo = bc_find(starts.data(), 0, count, (uint32_t)r0), hi = bc_find(starts.data(), lo, count, (uint32_t)r0 + rows - 1);
        for (uint32_t lane = 0; lane < EX_TILE_STEPS; ++lane) {
            const uint64_t o = r0 + EX_STEP_ROWS * lane;
            ExStep s = ex_zero_step();
            if (ex_live(o, n)) {
                const uint32_t e = bc_find(starts.data(), lo, hi, (uint32_t)o);
                if (e < count) {
                    const ExWord x = word_at(events.data() + (size_t)e * EX_EVENT_BYTES + 32);
                    const uint32_t j = ((uint32_t)o - starts[e]) / EX_STEP_ROWS;
                    if (!written.at(o / EX_STEP_ROWS)) return fprintf(stderr, "slot of row %llu read but never written\n", (unsigned long long)o), 1;
                    ExWord next = ex_word(0);
                    if (j + 1u < ex_steps(x)) {
                        if (!written.at(o / EX_STEP_ROWS + 1)) return fprintf(stderr, "slot behind row %llu read but never written\n", (unsigned long long)o), 1;
                        next = slots.at(o / EX_STEP_ROWS + 1);
                    }
                    s = ex_event_step(word_at(events.data() + (size_t)e * EX_EVENT_BYTES), x, j, slots.at(o / EX_STEP_ROWS), next);
                } else {
                    s = ex_pad_step();
                }
            }
            const ExMulAdd chips[2] = {ex_mul_chip(s), ex_parity_chip(s)};
            for (uint32_t r = 0; r < EX_STEP_ROWS && o + r < n; ++r) {
                const ExRow row = exp_row(s, chips[0], chips[1], r);
                is_last.at(o + r) = ExCell{row.is_last, 0};
                base_limb.at(o + r) = ExCell{row.base_limb, 0};
                exponent.at(o + r) = row.exponent_lo_hi;
                out.at(o + r) = row.exponentiation_lo_hi;
                for (int c = 0; c < 4; ++c) {
                    cols[0][c].at(o + r) = row.mul_cols[c];
                    cols[1][c].at(o + r) = row.parity_cols[c];
                    u64[0][c].at(o + r) = ExCell{row.mul_u16_64[c], 0};
                    u64[1][c].at(o + r) = ExCell{row.parity_u16_64[c], 0};
                }
                for (int c = 0; c < 8; ++c) {
                    u128[0][c].at(o + r) = ExCell{row.mul_u16_128[c], 0};
                    u128[1][c].at(o + r) = ExCell{row.parity_u16_128[c], 0};
                }
            }
        }
    }
    print_cells("is_last", -1, is_last);
    print_cells("base_limb", -1, base_limb);
    print_cells("exponent_lo_hi", -1, exponent);
    print_cells("exponentiation_lo_hi", -1, out);
    for (int chip = 0; chip < 2; ++chip) {
        const std::string p = chip ? "parity_" : "mul_";
        for (int c = 0; c < 4; ++c) print_cells((p + "cols").c_str(), c, cols[chip][c]);
        for (int c = 0; c < 4; ++c) print_cells((p + "u16_64").c_str(), c, u64[chip][c]);
        for (int c = 0; c < 8; ++c) print_cells((p + "u16_128").c_str(), c, u128[chip][c]);
    }
    return 0;
}

int main(int argc, char** argv) {
    if (argc != 2) return fprintf(stderr, "usage: %s cases.txt\n", argv[0]), 2;
    FILE* f = fopen(argv[1], "r");
    if (!f) return fprintf(stderr, "cannot open %s\n", argv[1]), 2;
    unsigned long long n;
    unsigned count;
    while (fscanf(f, " case %llu %u", &n, &count) == 2) {
        std::vector<uint8_t> events((size_t)count * EX_EVENT_BYTES);
        for (size_t i = 0; i < events.size(); ++i) {
            unsigned v;
            if (fscanf(f, "%2x", &v) != 1) return fprintf(stderr, "short event record\n"), 2;
            events[i] = (uint8_t)v;
        }
        if (const int rc = run_case(n, events, count)) return rc;
    }
    fclose(f);
    return 0;
}

// Stand-alone host program: the lane-free code of ZK_OP_COPY_ROWS and ZK_OP_COPY_RLC (csrc/copy_rows.hip.hpp) driven serially, lanes as
// loops, through exactly the functions the kernels call.  usage: host_copy_rows <cases>.  A case in the file:
//   case <n> <count> <total_bytes> <hex of the heap, or -> <hex of r_word, 32 B Montgomery> <hex of r_in>
//   then count lines, each the hex of one 88-byte zk_copy_event
// Every buffer is a heap block of its exact size.  For every case:
//   starts <start_0 .. start_count>
//   col <name> <n values>                        the rows tile by tile, every row found by bc_find in the tile's window
//   fr <name> <n x 64 hex digits>                value_acc from the maps of cp_acc_step composed per lane of eight steps and per block of
//                                                five lanes (the sum is associative: any grouping), word_rlc and word_rlc_prev carried
//                                                along lanes of eight steps that enter a word at any offset (cp_word_from)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../zkevm-circuits_amd/csrc/copy_rows.hip.hpp"

using namespace zk;

struct Map { Fr A, B; };                                                // z -> A z + B
static Map then(const Map& p, const Map& q) { return Map{q.A * p.A, q.A * p.B + q.B}; }

static std::vector<uint8_t> unhex(const char* s) {
    std::vector<uint8_t> out;
    if (!strcmp(s, "-")) return out;
    for (size_t i = 0; s[i] && s[i + 1]; i += 2) {
        char two[3] = {s[i], s[i + 1], 0};
        out.push_back((uint8_t)strtoul(two, nullptr, 16));
    }
    return out;
}
static Fr fr_of(const std::vector<uint8_t>& b) {
    Fr x;
    memcpy(x.l, b.data(), 32);
    return x;
}
static Fr mont_of(uint32_t v) {
    Fr x = Fr::zero();
    x.l[0] = v;
    return to_mont(x);
}
static void print_fr(const char* name, const std::vector<Fr>& col) {
    printf("fr %s", name);
    for (const Fr& x : col) {
        printf(" ");
        for (int i = 0; i < 32; ++i) printf("%02x", ((const uint8_t*)x.l)[i]);
    }
    printf("\n");
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    FILE* f = fopen(argv[1], "r");
    if (!f) return 2;
    static char line[1 << 22], hex[1 << 22], h1[80], h2[80];
    while (fgets(line, sizeof line, f)) {
        unsigned long long n64, count64, total;
        if (sscanf(line, "case %llu %llu %llu %s %79s %79s", &n64, &count64, &total, hex, h1, h2) != 6) return 3;
        const std::vector<uint8_t> heap = unhex(hex);
        if (heap.size() != total) return 3;
        const Fr r_word = fr_of(unhex(h1)), r_in = fr_of(unhex(h2));
        const uint32_t n = (uint32_t)n64, count = (uint32_t)count64;
        std::vector<uint8_t> records;
        for (uint32_t e = 0; e < count; ++e) {
            if (!fgets(line, sizeof line, f) || sscanf(line, "%s", hex) != 1) return 3;
            const std::vector<uint8_t> r = unhex(hex);
            if (r.size() != CP_EVENT_BYTES) return 3;
            records.insert(records.end(), r.begin(), r.end());
        }
        records.shrink_to_fit();
        std::vector<CpEvent> ev(count);
        for (uint32_t e = 0; e < count; ++e) {
            uint64_t w[CP_EVENT_WORDS];
            memcpy(w, records.data() + (size_t)e * CP_EVENT_BYTES, CP_EVENT_BYTES);
            ev[e] = cp_event(w);
            if (!cp_event_ok(ev[e], total)) ev[e].len = 0;
        }
        // start: the exclusive saturating scan, grouped by seven to show that the grouping does not matter
        std::vector<uint32_t> starts(count + 1, 0), w(count + 1, 0);
        for (uint32_t e = 0; e < count; ++e) w[e] = cp_rows_of(ev[e].len, n);
        {
            const uint32_t group = 7;
            std::vector<uint32_t> sums;
            for (uint32_t g0 = 0; g0 <= count; g0 += group) {
                uint32_t s = 0;
                for (uint32_t e = g0; e < g0 + group && e <= count; ++e) s = bc_sat_add(s, w[e], n);
                sums.push_back(s);
            }
            uint32_t base = 0;
            for (uint32_t g = 0, g0 = 0; g0 <= count; ++g, g0 += group) {
                uint32_t run = base;
                for (uint32_t e = g0; e < g0 + group && e <= count; ++e) { starts[e] = run; run = bc_sat_add(run, w[e], n); }
                base = bc_sat_add(base, sums[g], n);
            }
        }
        printf("starts");
        for (uint32_t e = 0; e <= count; ++e) printf(" %u", starts[e]);
        printf("\n");
        // the rows, tile by tile
        std::vector<CpRow> rows(n);
        for (uint32_t r0 = 0; r0 < n; r0 += CP_TILE) {
            const uint32_t last = n - r0 > CP_TILE ? r0 + CP_TILE - 1 : n - 1;
            const uint32_t lo = bc_find(starts.data(), 0, count, r0), hi = bc_find(starts.data(), lo, count, last);
            for (uint32_t i = r0; i <= last; ++i) {
                const uint32_t e = bc_find(starts.data(), lo, hi, i);
                rows[i] = cp_padding_row(i);
                if (e >= count) continue;
                const uint32_t j = i - starts[e], s = j >> 1;
                const uint32_t v = heap[(j & 1u ? ev[e].dst_off : ev[e].src_off) + s];
                rows[i] = cp_row(ev[e], j, v, j & 1u ? heap[ev[e].prev_off + s] : v);
            }
        }
#define COL(name, expr)                                                   \
    printf("col " name);                                                  \
    for (uint32_t i = 0; i < n; ++i) { const CpRow& r = rows[i]; printf(" %llu", (unsigned long long)(expr)); } \
    printf("\n");
        COL("is_first", r.is_first) COL("is_last", r.is_last) COL("tag", r.tag) COL("value", r.value) COL("value_prev", r.value_prev) COL("mask", r.mask)
        COL("front_mask", r.front_mask) COL("word_index", r.word_index) COL("is_pad", r.is_pad) COL("non_pad_non_mask", r.non_pad_non_mask) COL("src_end_rows", r.src_end_row)
        COL("addr", r.addr) COL("src_addr_end", r.src_addr_end) COL("real_bytes_left", r.real_bytes_left) COL("rw_counter", r.rw_counter) COL("rwc_inc_left", r.rwc_inc_left)
        COL("tag_bits0", r.tag >> 2 & 1) COL("tag_bits1", r.tag >> 1 & 1) COL("tag_bits2", r.tag & 1)
        COL("types0", r.tag == 1) COL("types1", r.tag == 2) COL("types2", r.tag == 3) COL("types3", r.tag == 4) COL("types4", r.memory_copy)
#undef COL
        // value_acc and the word RLCs in step space, per thread
        std::vector<Fr> acc(n, Fr::zero()), word(n, Fr::zero()), prev(n, Fr::zero());
        const uint32_t per = 8, lanes = 5;
        for (uint32_t t = 0; t < 2; ++t) {
            const uint64_t steps = n > t ? ((uint64_t)n - t + 1) / 2 : 0;
            const auto map_of = [&](uint64_t g) {                       // the map of step g
                const uint32_t row = (uint32_t)(2 * g + t), e = bc_find(starts.data(), 0, count, row);
                if (e >= count) return Map{Fr::zero(), Fr::zero()};
                const uint32_t s = (row - starts[e]) >> 1;
                uint32_t x;
                const uint32_t kind = cp_acc_step(ev[e], s, t, heap[(t ? ev[e].dst_off : ev[e].src_off) + s], x);
                return kind == CP_CONST ? Map{Fr::zero(), mont_of(x)} : kind == CP_STEP ? Map{r_in, mont_of(x)} : Map{Fr::one(), Fr::zero()};
            };
            // lane maps, block maps, the value entering every block, every lane, every step
            Fr enter_block = Fr::zero();
            for (uint64_t b0 = 0; b0 < steps; b0 += per * lanes) {
                Fr enter_lane = enter_block;
                Map block{Fr::one(), Fr::zero()};
                for (uint64_t g0 = b0; g0 < b0 + per * lanes && g0 < steps; g0 += per) {
                    Map lane{Fr::one(), Fr::zero()};
                    for (uint64_t g = g0; g < g0 + per && g < steps; ++g) lane = then(lane, map_of(g));
                    Fr z = enter_lane;
                    for (uint64_t g = g0; g < g0 + per && g < steps; ++g) { const Map m = map_of(g); z = m.A * z + m.B; acc[2 * g + t] = z; }
                    enter_lane = lane.A * enter_lane + lane.B;
                    if (!(z == enter_lane)) return 4;                   // the lane's composite map is its steps
                    block = then(block, lane);
                }
                enter_block = block.A * enter_block + block.B;
                if (!(enter_block == enter_lane)) return 4;
            }
            for (uint64_t g0 = 0; g0 < steps; g0 += per) {
                Fr wv = Fr::zero(), pv = Fr::zero();
                bool fresh = true;
                uint32_t before = 0xffffffffu;
                for (uint64_t g = g0; g < g0 + per && g < steps; ++g) {
                    const uint32_t row = (uint32_t)(2 * g + t), e = bc_find(starts.data(), 0, count, row);
                    if (e != before) fresh = true;
                    before = e;
                    if (e >= count) continue;
                    const uint32_t s = (row - starts[e]) >> 1, from = cp_word_from(s, fresh);
                    if (from != s || (s & 31u) == 0) wv = Fr::zero(), pv = Fr::zero();
                    for (uint32_t u = from; u <= s; ++u) {
                        wv = wv * r_word + mont_of(heap[(t ? ev[e].dst_off : ev[e].src_off) + u]);
                        if (t) pv = pv * r_word + mont_of(heap[ev[e].prev_off + u]);
                    }
                    fresh = false;
                    word[row] = wv, prev[row] = t ? pv : wv;
                }
            }
        }
        print_fr("value_acc", acc);
        print_fr("word_rlc", word);
        print_fr("word_rlc_prev", prev);
    }
    fclose(f);
    return 0;
}

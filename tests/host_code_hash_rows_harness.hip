// Stand-alone host program: the lane-free code of ZK_OP_CODE_HASH_ROWS and ZK_OP_CODE_HASH_TABLE (csrc/code_hash_rows.hip.hpp)
// driven serially, lanes as loops, through exactly the functions the kernels call.  usage: host_code_hash_rows <cases>.  A case in
// the file:
//   case <n> <table n> <count> <total_bytes> <hex of the bytes, or ->        then count lines  <offset> <length>
// Every input buffer is a heap block of its exact size.  Beside the shared buffer every bytecode is copied into blocks of its own in
// which it ends at the last byte, at each of the four alignments of its first byte, and every field is read from those too: a read
// in front of or behind a bytecode leaves the block (which the address sanitizer reports), and the values must agree.
// For every case one line per item, every cell as a hexadecimal integer (field elements out of Montgomery form):
//   starts <start_0 .. start_m>      tstarts <tstart_0 .. tstart_count>      needed <sum K_b>
//   col <name> <n values>            tab <name> <table n values>
//   consts <256^0 .. 256^31> <1/0 .. 1/30>     once, in front of the cases
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../zkevm-circuits_amd/csrc/code_hash_rows.hip.hpp"

using namespace zk;

struct Entry { uint64_t off, len; };

static uint8_t* exact_block(const uint8_t* src, size_t bytes) {
    uint8_t* p = (uint8_t*)malloc(bytes ? bytes : 1);
    if (bytes) memcpy(p, src, bytes);
    return p;
}
static bool unhex(const char* s, std::vector<uint8_t>& out) {
    if (!strcmp(s, "-")) return true;
    for (size_t i = 0; s[i] && s[i + 1]; i += 2) {
        char two[3] = {s[i], s[i + 1], 0};
        out.push_back((uint8_t)strtoul(two, nullptr, 16));
    }
    return true;
}
static void put_fr(const Fr& mont) {
    const Fr v = from_mont(mont);
    printf(" ");
    bool lead = true;
    for (int i = 7; i >= 0; --i) {
        if (lead && !v.l[i] && i) continue;
        printf(lead ? "%x" : "%08x", v.l[i]);
        lead = false;
    }
}
// the exclusive saturating scan in groups of seven: the sum is associative, any grouping gives the same starts
static std::vector<uint32_t> scan(const std::vector<uint32_t>& w, uint32_t cap) {
    const size_t group = 7, count = w.size();
    std::vector<uint32_t> starts(count, 0), sums;
    for (size_t g0 = 0; g0 < count; g0 += group) {
        uint32_t s = 0;
        for (size_t b = g0; b < g0 + group && b < count; ++b) s = bc_sat_add(s, w[b], cap);
        sums.push_back(s);
    }
    uint32_t base = 0;
    for (size_t g = 0, g0 = 0; g0 < count; ++g, g0 += group) {
        uint32_t run = base;
        for (size_t b = g0; b < g0 + group && b < count; ++b) { starts[b] = run; run = bc_sat_add(run, w[b], cap); }
        base = bc_sat_add(base, sums[g], cap);
    }
    return starts;
}
// owner of `row` and its offset from the owner's first row, as a lane finds them: the tile's window, then the row's own search
static void find(const std::vector<uint32_t>& starts, uint32_t m, uint32_t n, uint32_t row, uint32_t& b, uint32_t& d) {
    const uint32_t r0 = row / BC_TILE * BC_TILE, tile_last = n - r0 > BC_TILE ? r0 + BC_TILE - 1 : n - 1;
    const uint32_t b_lo = bc_find(starts.data(), 0, m, r0), b_hi = bc_find(starts.data(), b_lo, m, tile_last);
    b = bc_find(starts.data(), b_lo, b_hi, row);
    d = b < m ? row - starts[b] : 0;
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    FILE* f = fopen(argv[1], "r");
    if (!f) return 2;
    printf("consts");
    for (uint32_t k = 0; k <= CH_F; ++k) put_fr(ch_pow256(k));
    for (uint32_t k = 0; k < CH_F; ++k) put_fr(ch_inv_small(k));
    printf("\n");
    static char line[1 << 22], hex[1 << 22];
    while (fgets(line, sizeof line, f)) {
        unsigned long long n64, tn64, count64, total;
        if (sscanf(line, "case %llu %llu %llu %llu %s", &n64, &tn64, &count64, &total, hex) != 5) return 3;
        std::vector<uint8_t> parsed;
        unhex(hex, parsed);
        if (parsed.size() != total) return 3;
        uint8_t* bytes = exact_block(parsed.data(), parsed.size());
        std::vector<Entry> entries(count64);
        for (auto& e : entries) {
            if (!fgets(line, sizeof line, f)) return 3;
            unsigned long long off, len;
            if (sscanf(line, "%llu %llu", &off, &len) != 2) return 3;
            e = {off, len};
            if (!bc_entry_ok(e.off, e.len, total)) e = {0, 0};
        }
        // every bytecode in blocks of its own, its last byte the block's last, its first at address = sh mod 4
        std::vector<uint8_t*> own(4 * entries.size());
        for (size_t b = 0; b < entries.size(); ++b)
            for (uint32_t sh = 0; sh < 4; ++sh) {
                own[4 * b + sh] = (uint8_t*)malloc(sh + entries[b].len ? sh + entries[b].len : 1);
                if (entries[b].len) memcpy(own[4 * b + sh] + sh, bytes + entries[b].off, entries[b].len);
            }
        const uint32_t count = (uint32_t)count64;
        // ---- the circuit's rows
        {
            const uint32_t n = (uint32_t)n64, m = count64 < n64 ? count : n;
            std::vector<uint32_t> w(m + 1, 0);
            for (uint32_t b = 0; b < m; ++b) w[b] = bc_rows_of(entries[b].len, n);
            const std::vector<uint32_t> starts = scan(w, n);
            printf("starts");
            for (uint32_t b = 0; b <= m; ++b) printf(" %x", starts[b]);
            printf("\n");
            std::vector<ChRow> rows(n);
            std::vector<Fr> input(n);
            for (uint32_t row = 0; row < n; ++row) {
                uint32_t b, d;
                find(starts, m, n, row, b, d);
                const uint32_t kind = b >= m ? BC_PAD : d ? BC_BYTE : BC_HEADER;
                const uint64_t p = kind == BC_BYTE ? (uint64_t)d - 1 : 0, len = b < m ? entries[b].len : 0;
                if (kind == BC_BYTE && p >= len) return 4;                // a byte outside its bytecode
                rows[row] = ch_row(kind, p, len);
                input[row] = kind == BC_BYTE ? ch_field_input(bytes, entries[b].off, len, p, rows[row].m) : Fr::zero();
                if (kind == BC_BYTE)
                    for (uint32_t sh = 0; sh < 4; ++sh)
                        if (ch_field_input(own[4 * b + sh], sh, len, p, rows[row].m) != input[row]) return 6;
            }
#define COL(name, expr) printf("col " name); for (uint32_t i = 0; i < n; ++i) { const ChRow& r = rows[i]; printf(" %x", (unsigned)(expr)); } printf("\n");
            COL("control_length", r.control_length) COL("bytes_in_field_index", r.bytes_in_field_index) COL("is_field_border", r.is_field_border)
            COL("field_index", r.field_index) COL("field_index_inv", r.field_index_inv)
#undef COL
            printf("col field_input"); for (uint32_t i = 0; i < n; ++i) put_fr(input[i]); printf("\n");
            printf("col bytes_in_field_inv"); for (uint32_t i = 0; i < n; ++i) put_fr(ch_inv_small(rows[i].inv_of)); printf("\n");
            printf("col padding_shift"); for (uint32_t i = 0; i < n; ++i) put_fr(ch_pow256(rows[i].shift)); printf("\n");
        }
        // ---- the table's rows
        {
            const uint32_t n = (uint32_t)tn64, m = count;
            std::vector<uint32_t> w(m + 1, 0);
            uint64_t needed = 0;
            for (uint32_t b = 0; b < m; ++b) { w[b] = ch_table_rows_of(entries[b].len, n); needed += ch_blocks_of(entries[b].len); }
            const std::vector<uint32_t> starts = scan(w, n);
            printf("tstarts");
            for (uint32_t b = 0; b <= m; ++b) printf(" %x", starts[b]);
            printf("\nneeded %llx\n", (unsigned long long)needed);
            std::vector<ChTableRow> rows(n);
            std::vector<Fr> in0(n), in1(n);
            for (uint32_t row = 0; row < n; ++row) {
                uint32_t b, j;
                find(starts, m, n, row, b, j);
                const bool owned = b < m;
                const uint64_t len = owned ? entries[b].len : 0;
                if (owned && (uint64_t)CH_W * j >= len) return 4;         // a block outside its bytecode
                rows[row] = ch_table_row(owned, j, len);
                in0[row] = owned ? ch_table_input(bytes, entries[b].off, len, j, 0) : Fr::zero();
                in1[row] = owned ? ch_table_input(bytes, entries[b].off, len, j, 1) : Fr::zero();
                if (owned)
                    for (uint32_t sh = 0; sh < 4; ++sh)
                        if (ch_table_input(own[4 * b + sh], sh, len, j, 0) != in0[row] || ch_table_input(own[4 * b + sh], sh, len, j, 1) != in1[row]) return 6;
            }
            printf("tab input0"); for (uint32_t i = 0; i < n; ++i) put_fr(in0[i]); printf("\n");
            printf("tab input1"); for (uint32_t i = 0; i < n; ++i) put_fr(in1[i]); printf("\n");
            printf("tab control");                                      // control_hi 2^64
            for (uint32_t i = 0; i < n; ++i) {
                if (rows[i].control_hi) printf(" %llx0000000000000000", (unsigned long long)rows[i].control_hi);
                else printf(" 0");
            }
            printf("\n");
            printf("tab heading_mark"); for (uint32_t i = 0; i < n; ++i) printf(" %x", rows[i].heading_mark); printf("\n");
            printf("tab kinds"); for (uint32_t i = 0; i < n; ++i) printf(" %x", rows[i].kind); printf("\n");
            printf("tab cap"); for (uint32_t i = 0; i < n; ++i) printf(" %llx", (unsigned long long)rows[i].cap); printf("\n");
        }
        for (uint8_t* p : own) free(p);
        free(bytes);
    }
    fclose(f);
    return 0;
}

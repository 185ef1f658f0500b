// Test harness: the per-lane code of ZK_OP_POSEIDON (csrc/poseidon29.hip.hpp: psd_load, psd_in, psd_enter, psd_rounds -- psd_pow5 and
// psd_mds_row --, psd_out) compiled for the HOST as a stand-alone program, run directly by tests/test_poseidon_host.py (once plain,
// once under the address and undefined-behaviour sanitizers).  It does to a sequence of rows what a lane of k_poseidon_walk
// (csrc/poseidon.hip) does to the rows of its message, the state carried from row to row.
// Input (file named by argv[1]), numbers in hex:
//   tab <1836 words>                    the 204 limb records, once, first
//   state <fr> <fr> <fr>                sets the carried state: three canonical Montgomery Fr (as if a row had left them)
//   row <head: 0 | 1> <width0> <bytes0> <k0> <width1> <bytes1> <k1> <cap width or 0> <cap bytes or -> <kcap>
//                                       bytesN: the cell in memory order, 2 hex digits per byte; kN: the plain constant of psd_in
// Every cell is copied to index 1 of a heap buffer of exactly two cells (31-byte cells: 62 + 31 bytes), so that a read outside the
// cell's column is the address sanitizer's to find.
// Output, one line per row: <out> <word0> <word1> <27 limbs of the state the row leaves>.
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../zkevm-circuits_amd/csrc/poseidon29.hip.hpp"

using namespace zk;

static bool read_hex(FILE* f, Fr* out) {
    char buf[80];
    if (fscanf(f, "%79s", buf) != 1) return false;
    const size_t len = strlen(buf);
    if (len == 0 || len > 64) return false;
    *out = Fr::zero();
    for (size_t i = 0; i < len; ++i) {
        const char ch = buf[len - 1 - i];
        const uint32_t d = ch >= '0' && ch <= '9' ? ch - '0' : ch >= 'a' && ch <= 'f' ? ch - 'a' + 10 : 16;
        if (d > 15) return false;
        out->l[i / 8] |= d << (4 * (i % 8));
    }
    return true;
}

// the cell at index 1 of a buffer of two; the caller frees
static uint8_t* read_cell(FILE* f, unsigned width) {
    char buf[80];
    if (fscanf(f, "%79s", buf) != 1 || strlen(buf) != 2 * (size_t)width) return nullptr;
    const size_t stride = width == 31 ? 62 : width, size = stride + width;
    void* mem = nullptr;
    if (posix_memalign(&mem, 32, size)) return nullptr;                 // the exact size, for the sanitizer; aligned like a device buffer
    uint8_t* p = (uint8_t*)mem;
    memset(p, 0xA5, size);
    for (unsigned i = 0; i < width; ++i) {
        unsigned v;
        if (sscanf(buf + 2 * i, "%2x", &v) != 1) { free(p); return nullptr; }
        p[stride + i] = (uint8_t)v;
    }
    return p;
}

static bool good_width(unsigned w, bool cap) { return w == 1 || w == 2 || w == 4 || w == 8 || w == 16 || w == 32 || (!cap && w == 31); }

static void print_fr(const Fr& v) {
    for (int i = 7; i >= 0; --i) printf("%08" PRIx32, v.l[i]);
}

int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: %s cases.txt\n", argv[0]); return 2; }
    FILE* f = fopen(argv[1], "r");
    if (!f) { perror(argv[1]); return 2; }
    std::vector<uint32_t> tab;
    Fr29 s[3];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 9; ++j) s[i].l[j] = 0;
    const Fr c266 = [] { Fr c = Fr::one(); for (int i = 256; i < 266; ++i) c = dbl(c); return c; }();
    char word[16];
    while (fscanf(f, "%15s", word) == 1) {
        if (!strcmp(word, "tab")) {
            tab.resize(PSD_TAB_WORDS);
            for (uint32_t& w : tab)
                if (fscanf(f, "%" SCNx32, &w) != 1 || w > MASK29) { fprintf(stderr, "bad table word\n"); return 2; }
        } else if (!strcmp(word, "state")) {
            for (int i = 0; i < 3; ++i) {
                Fr v;
                if (!read_hex(f, &v)) { fprintf(stderr, "bad state\n"); return 2; }
                s[i] = psd_in<Fr29P>(v, unpack29<Fr29P>(c266));
            }
        } else if (!strcmp(word, "row")) {
            if (tab.empty()) { fprintf(stderr, "row before tab\n"); return 2; }
            unsigned head, width[3];
            uint8_t* cell[3] = {nullptr, nullptr, nullptr};
            Fr k[3];
            if (fscanf(f, "%u", &head) != 1 || head > 1) { fprintf(stderr, "bad row\n"); return 2; }
            for (int c = 0; c < 3; ++c) {
                if (fscanf(f, "%u", &width[c]) != 1) { fprintf(stderr, "bad width\n"); return 2; }
                if (c == 2 && width[c] == 0) {
                    char dash[8];
                    if (fscanf(f, "%7s", dash) != 1) return 2;
                } else {
                    if (!good_width(width[c], c == 2)) { fprintf(stderr, "bad width %u\n", width[c]); return 2; }
                    cell[c] = read_cell(f, width[c]);
                    if (!cell[c]) { fprintf(stderr, "bad cell\n"); return 2; }
                }
                if (!read_hex(f, &k[c])) { fprintf(stderr, "bad constant\n"); return 2; }
            }
            // as psd_row of csrc/poseidon.hip
            const Fr29 x0 = psd_in<Fr29P>(psd_load(cell[0], width[0], 1), unpack29<Fr29P>(k[0])), x1 = psd_in<Fr29P>(psd_load(cell[1], width[1], 1), unpack29<Fr29P>(k[1]));
            if (head) {
                for (int i = 0; i < 3; ++i)
                    for (int j = 0; j < 9; ++j) s[i].l[j] = 0;
                if (cell[2]) s[0] = psd_in<Fr29P>(psd_load(cell[2], width[2], 1), unpack29<Fr29P>(k[2]));
            }
            psd_enter<Fr29P>(s, x0, x1, tab.data());
            psd_rounds<Fr29P>(s, tab.data());
            print_fr(psd_out<Fr29P>(s[0]));
            printf(" ");
            print_fr(psd_out<Fr29P>(x0));
            printf(" ");
            print_fr(psd_out<Fr29P>(x1));
            for (int i = 0; i < 3; ++i)
                for (int j = 0; j < 9; ++j) printf(" %" PRIx32, s[i].l[j]);
            printf("\n");
            for (int c = 0; c < 3; ++c) free(cell[c]);
        } else { fprintf(stderr, "expected 'tab', 'state' or 'row'\n"); return 2; }
    }
    fclose(f);
    return 0;
}

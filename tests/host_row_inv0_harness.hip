// Test harness: the per-lane arithmetic of the inverse-or-zero row op (csrc/ff29.hip.hpp: inv0_29_den / inv0_29_prefix / inv29_rp /
// inv0_29_back / inv0_29_out over rlc29_init / rlc29_mac / rlc29_reduce) compiled for the HOST as a stand-alone program, run directly by
// tests/test_row_inv0_host.py (once plain, once under the address and undefined-behaviour sanitizers).  It does to the rows of one
// lane -- 4 (one tile of the kernel) or 16 (the four tiles a wave takes) -- what a lane of k_fr_row_inv0 (csrc/typed_rows.hip) does, the
// wave being this lane alone: the product that inv29_rp inverts is the lane's own.
// Input (file named by argv[1]), all numbers little-endian integers in hex:
//   lane <num kind: 0 none, 1 narrow, 2 Fr> <rows: 4 | 16> <2^261 mod p> <constant of inv29_rp>
//   the rows, each:
//     terms <in range: 0 | 1> <count> <k0>        then count lines  <width> <cell> <K>    (the K of the inverting launch)
//   or
//     raw <in range: 0 | 1> <T>                    the unreduced sum itself, T < 2^261 p (up to 131 hex digits)
//   <num 0> .. <num rows-1>                       the stored numerators (present for every kind; ignored for kind 0)
// Output, one line per row: <packed result> <limb 0> .. <limb 8 of rlc29_reduce, before the canonical form>, then `live <mask>`.
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../zkevm-circuits_amd/csrc/ff29.hip.hpp"

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

// T as 18 normalised column sums
static bool read_raw(FILE* f, Rlc29<Fr29P>* t) {
    char buf[160];
    if (fscanf(f, "%159s", buf) != 1) return false;
    const size_t len = strlen(buf);
    if (len == 0 || len > 131) return false;
    for (int i = 0; i < 18; ++i) t->c[i] = 0;
    t->load = 1;
    for (size_t i = 0; i < len; ++i) {
        const char ch = buf[len - 1 - i];
        const uint64_t d = ch >= '0' && ch <= '9' ? ch - '0' : ch >= 'a' && ch <= 'f' ? ch - 'a' + 10 : 16;
        if (d > 15) return false;
        for (int bit = 0; bit < 4; ++bit) {
            const size_t pos = 4 * i + bit;
            if ((d >> bit & 1) && pos / 29 >= 18) return false;
            if (d >> bit & 1) t->c[pos / 29] |= (uint64_t)1 << (pos % 29);
        }
    }
    return true;
}

template <int L>
static void term(Rlc29<Fr29P>& t, const Fr& cell, const Fr& k) {
    const Fr29 x = unpack29<Fr29P>(cell), kl = unpack29<Fr29P>(k);
    for (int i = L; i < 9; ++i)
        if (x.l[i]) { fprintf(stderr, "cell wider than its width\n"); exit(2); }
    rlc29_mac<L>(t, x.l, kl.l);
    if (t.load > RLC29_MAX_LOAD) { fprintf(stderr, "column load %u\n", t.load); exit(2); }
}

static void print_fr(const Fr& v) {
    for (int i = 7; i >= 0; --i) printf("%08" PRIx32, v.l[i]);
}

template <int ROWS>
static int run_lane(FILE* f, unsigned kind) {
    char word[16];
    Fr one_rp, cinv;
    if (!read_hex(f, &one_rp) || !read_hex(f, &cinv)) { fprintf(stderr, "bad lane constants\n"); return 2; }
    Fr29 d[ROWS], pre[ROWS], q[ROWS], num[ROWS], raw[ROWS];
    uint32_t live = 0;
    for (int s = 0; s < ROWS; ++s) {
        unsigned in_range;
        Rlc29<Fr29P> t;
        if (fscanf(f, "%15s %u", word, &in_range) != 2) { fprintf(stderr, "bad row line\n"); return 2; }
        if (!strcmp(word, "raw")) {
            if (!read_raw(f, &t)) { fprintf(stderr, "bad raw sum\n"); return 2; }
        } else if (!strcmp(word, "terms")) {
            unsigned count;
            Fr k0;
            if (fscanf(f, "%u", &count) != 1 || !read_hex(f, &k0)) { fprintf(stderr, "bad terms line\n"); return 2; }
            rlc29_init(t, unpack29<Fr29P>(k0).l);
            for (unsigned j = 0; j < count; ++j) {
                unsigned width;
                Fr cell, k;
                if (fscanf(f, "%u", &width) != 1 || !read_hex(f, &cell) || !read_hex(f, &k)) { fprintf(stderr, "bad column line\n"); return 2; }
                switch (width) {
                    case 1: case 2: term<1>(t, cell, k); break;
                    case 4: term<2>(t, cell, k); break;
                    case 8: term<3>(t, cell, k); break;
                    case 16: term<5>(t, cell, k); break;
                    case 32: term<9>(t, cell, k); break;
                    default: fprintf(stderr, "bad width %u\n", width); return 2;
                }
            }
        } else { fprintf(stderr, "expected 'terms' or 'raw'\n"); return 2; }
        raw[s] = rlc29_reduce(t);
        if (inv0_29_den(t, d[s]) && in_range) live |= 1u << s;          // as k_fr_row_inv0: zero rows and rows past n take no part
    }
    for (int s = 0; s < ROWS; ++s) {
        Fr n;
        if (!read_hex(f, &n)) { fprintf(stderr, "bad numerator\n"); return 2; }
        num[s] = unpack29<Fr29P>(n);
    }
    const Fr29 mine = inv0_29_prefix(d, live, unpack29<Fr29P>(one_rp), pre);
    const Fr29 iv = inv29_rp(mine, unpack29<Fr29P>(cinv));              // a wave of one lane: the total is this lane's product
    inv0_29_back(iv, d, pre, live, q);
    for (int s = 0; s < ROWS; ++s) {
        Fr out = Fr::zero();
        if (live >> s & 1u) out = kind == 0 ? inv0_29_out<INV0_NUM_ONE>(q[s], num[s]) : kind == 1 ? inv0_29_out<INV0_NUM_UINT>(q[s], num[s]) : inv0_29_out<INV0_NUM_FR>(q[s], num[s]);
        print_fr(out);
        for (int i = 0; i < 9; ++i) printf(" %" PRIx32, raw[s].l[i]);
        printf("\n");
    }
    printf("live %x\n", live);
    return 0;
}

int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: %s cases.txt\n", argv[0]); return 2; }
    FILE* f = fopen(argv[1], "r");
    if (!f) { perror(argv[1]); return 2; }
    char word[16];
    unsigned kind, rows;
    while (fscanf(f, "%15s %u %u", word, &kind, &rows) == 3) {
        if (strcmp(word, "lane") || kind > 2 || (rows != 4 && rows != 16)) { fprintf(stderr, "expected 'lane <0|1|2> <4|16>'\n"); return 2; }
        if (int e = rows == 4 ? run_lane<4>(f, kind) : run_lane<16>(f, kind)) return e;
    }
    fclose(f);
    return 0;
}

// Test harness: the row step and the chunk fold of the typed running RLC (csrc/ff29.hip.hpp: scan_rlc29_step / scan_rlc29_fold, the
// routines k_scan_rlc_a / k_scan_rlc_c of csrc/vec.hip run per row) compiled for the HOST as a stand-alone program, run directly by
// tests/test_scan_rlc_host.py (once plain, once under the address and undefined-behaviour sanitizers).  It does to a chain of rows
// what a thread does to its chunk: cells become limbs by unpack29 (1, 1, 2, 3, 5 or 9 of them by width), the row's kind picks one of
// four (M, K) records, the walk goes through scan_rlc29_step from z0 and the fold through scan_rlc29_fold from the identity map.
// Input (file named by argv[1]), all numbers little-endian integers in hex:
//   chain <width> <steps>
//   <z0>                                  the start value's Montgomery image (canonical)
//   <M_0> <K_0> .. <M_3> <K_3>            M = m 2^261 mod p, K = w 2^517 mod p (width <= 16) or w 2^261 mod p (width 32)
//   <kind> <cell>                         steps lines
// Output, one line per step: <packed z> <9 limbs of z> <9 limbs of A> <9 limbs of B>, then one line per chain: fold <packed A> <packed B>
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

static void print_packed(const Fr& v) {
    for (int i = 7; i >= 0; --i) printf("%08" PRIx32, v.l[i]);
}

template <int L>
static void row(Fr29& z, Fr29& A, Fr29& B, const Fr& cell, const Fr29& M, const Fr29& K) {
    const Fr29 x = unpack29<Fr29P>(cell);
    for (int i = L; i < 9; ++i)
        if (x.l[i]) { fprintf(stderr, "cell wider than its width\n"); exit(2); }
    z = scan_rlc29_step<L>(z, x.l, M.l, K.l);
    scan_rlc29_fold<L>(A, B, x.l, M.l, K.l);
}

int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: %s chains.txt\n", argv[0]); return 2; }
    FILE* f = fopen(argv[1], "r");
    if (!f) { perror(argv[1]); return 2; }
    char word[16];
    unsigned width, steps;
    while (fscanf(f, "%15s %u %u", word, &width, &steps) == 3) {
        if (strcmp(word, "chain")) { fprintf(stderr, "expected 'chain'\n"); return 2; }
        Fr z0, c;
        Fr29 M[4], K[4];
        if (!read_hex(f, &z0)) { fprintf(stderr, "bad start value\n"); return 2; }
        for (int s = 0; s < 4; ++s) {
            if (!read_hex(f, &c)) { fprintf(stderr, "bad M\n"); return 2; }
            M[s] = unpack29<Fr29P>(c);
            if (!read_hex(f, &c)) { fprintf(stderr, "bad K\n"); return 2; }
            K[s] = unpack29<Fr29P>(c);
        }
        Fr29 z = unpack29<Fr29P>(z0), A = unpack29<Fr29P>(Fr::one()), B = unpack29<Fr29P>(Fr::zero());
        for (unsigned j = 0; j < steps; ++j) {
            unsigned kind;
            Fr cell;
            if (fscanf(f, "%u", &kind) != 1 || kind > 3 || !read_hex(f, &cell)) { fprintf(stderr, "bad row line\n"); return 2; }
            switch (width) {
                case 1: case 2: row<1>(z, A, B, cell, M[kind], K[kind]); break;
                case 4: row<2>(z, A, B, cell, M[kind], K[kind]); break;
                case 8: row<3>(z, A, B, cell, M[kind], K[kind]); break;
                case 16: row<5>(z, A, B, cell, M[kind], K[kind]); break;
                case 32: row<9>(z, A, B, cell, M[kind], K[kind]); break;
                default: fprintf(stderr, "bad width %u\n", width); return 2;
            }
            print_packed(pack29_lt2p(z));
            for (int i = 0; i < 9; ++i) printf(" %" PRIx32, z.l[i]);
            for (int i = 0; i < 9; ++i) printf(" %" PRIx32, A.l[i]);
            for (int i = 0; i < 9; ++i) printf(" %" PRIx32, B.l[i]);
            printf("\n");
        }
        printf("fold ");
        print_packed(pack29_lt2p(A));
        printf(" ");
        print_packed(pack29_lt2p(B));
        printf("\n");
    }
    fclose(f);
    return 0;
}

// Test harness: the per-lane code of ZK_OP_SHA256 (csrc/sha256_32.hip.hpp: sha_row -- the range test, sha_hash with its blocks at
// any alignment, its padding and the 64 unrolled rounds, the digest words under kck_rlc8 --, kck_input_rlc and kck_pow_table of
// csrc/keccak64.hip.hpp) compiled for the HOST as a stand-alone program, run directly by tests/test_sha256_host.py (once plain, once
// under the address and undefined-behaviour sanitizers).  It does to every row what a lane of k_sha256 (csrc/sha256.hip) does, in
// both instantiations, and requires the two to agree on the digest and output_rlc.
// Input (file named by argv[1]), numbers in hex:
//   r <r_out> <r_in>                    the two challenges, canonical Montgomery Fr; the records are made by kck_pow_table
//   buf <total bytes> <bytes or ->      a heap block of EXACTLY total bytes (8-byte aligned, like nothing more than malloc promises),
//                                       2 hex digits per byte: a read past its last byte is the address sanitizer's to find
//   row <off> <len>                     one message of the current block (64-bit values; out-of-range rows give zeros)
//   zeros <len>                         sha_hash alone, no RLC, of len zero bytes in a block of their own (the long message)
// Output, one line per row: <1 in range | 0> <digest, 32 bytes in order> <output_rlc> <input_rlc>; per zeros line: the digest.
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../zkevm-circuits_amd/csrc/sha256_32.hip.hpp"

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

static void print_fr(const Fr& v) {
    for (int i = 7; i >= 0; --i) printf("%08" PRIx32, v.l[i]);
}

static void print_digest(const uint64_t (&words)[4]) {
    uint8_t d[32];
    memcpy(d, words, 32);
    for (int i = 0; i < 32; ++i) printf("%02x", d[i]);
}

int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: %s cases.txt\n", argv[0]); return 2; }
    FILE* f = fopen(argv[1], "r");
    if (!f) { perror(argv[1]); return 2; }
    KckPow pout, pin;
    bool have_r = false;
    uint8_t* buf = nullptr;
    uint64_t total = 0;
    char word[16];
    while (fscanf(f, "%15s", word) == 1) {
        if (!strcmp(word, "r")) {
            Fr r_out, r_in;
            if (!read_hex(f, &r_out) || !read_hex(f, &r_in)) { fprintf(stderr, "bad challenges\n"); return 2; }
            pout = kck_pow_table(r_out);
            pin = kck_pow_table(r_in);
            have_r = true;
        } else if (!strcmp(word, "buf")) {
            free(buf);
            buf = nullptr;
            if (fscanf(f, "%" SCNx64, &total) != 1 || total > (1u << 24)) { fprintf(stderr, "bad size\n"); return 2; }
            if (total) {
                void* mem = nullptr;
                if (posix_memalign(&mem, 8, total)) return 2;             // the exact size, for the sanitizer
                buf = (uint8_t*)mem;
            }
            int c;
            while ((c = fgetc(f)) == ' ') {}
            if (c == '-') {
                if (total) { fprintf(stderr, "bytes missing\n"); return 2; }
                continue;
            }
            ungetc(c, f);
            for (uint64_t i = 0; i < total; ++i) {
                unsigned v;
                if (fscanf(f, "%2x", &v) != 1) { fprintf(stderr, "bad byte\n"); return 2; }
                buf[i] = (uint8_t)v;
            }
        } else if (!strcmp(word, "row")) {
            if (!have_r) { fprintf(stderr, "row before r\n"); return 2; }
            uint64_t off, len;
            if (fscanf(f, "%" SCNx64 " %" SCNx64, &off, &len) != 2) { fprintf(stderr, "bad row\n"); return 2; }
            KckOut a, b;
            const bool ok = sha_row<true>(buf, total, off, len, pout, &pin, a);
            const bool ok2 = sha_row<false>(buf, total, off, len, pout, nullptr, b);
            if (ok != ok2 || memcmp(a.digest, b.digest, 32) || memcmp(&a.out, &b.out, sizeof(Fr))) { fprintf(stderr, "the two instantiations differ\n"); return 3; }
            printf("%d ", ok ? 1 : 0);
            print_digest(a.digest);
            printf(" ");
            print_fr(a.out);
            printf(" ");
            print_fr(a.in);
            printf("\n");
        } else if (!strcmp(word, "zeros")) {
            uint64_t len;
            if (fscanf(f, "%" SCNx64, &len) != 1 || len == 0 || len > (1ull << 30)) { fprintf(stderr, "bad length\n"); return 2; }
            uint8_t* z = (uint8_t*)calloc(len, 1);
            if (!z) { fprintf(stderr, "no memory for %" PRIu64 " bytes\n", len); return 2; }
            uint32_t H[8];
            uint64_t words[4];
            sha_hash(z, len, H);
            sha_digest_words(H, words);
            print_digest(words);
            printf("\n");
            free(z);
        } else { fprintf(stderr, "expected 'r', 'buf', 'row' or 'zeros'\n"); return 2; }
    }
    free(buf);
    fclose(f);
    return 0;
}

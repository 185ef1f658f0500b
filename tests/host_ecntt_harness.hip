// Test harness: the butterfly of the group FFT behind g_to_lagrange (csrc/ec29.hip.hpp: ecntt_butterfly29, mul_scalar29, neg29pt,
// add29pt, dbl29pt) compiled for the HOST as a stand-alone program, run directly by tests/test_ecntt_host.py (once plain, once
// under the address and undefined-behaviour sanitizers).  Not part of the product library.
//
//   host_ecntt fft FILE    FILE: k | omega^-1 and 1/n (Fr, Montgomery, hex) | 2^k lines "x y" (Fq, R = 2^256 Montgomery, hex; the
//                          identity is "0 0"): what k_ecntt_load reads.  Runs the kernels' schedule (csrc/ecntt.hip): bit-reversed
//                          load into R' XYZZ, stages s = 0 .. k-1 through ecntt_butterfly29 with w = from_mont(omega^-(j << (k-1-s))),
//                          then 1/n through mul_scalar29.  After every butterfly both outputs must keep the stored invariant
//                          (normalised limbs, x, y < 8p, zz, zzz < 2p); a violation is printed and ends the run with status 1.
//                          Prints "stage s doublings cancellations identity-operands" per stage -- each of the two additions of a
//                          butterfly classified from canonical cross products, not by the k p test under test -- then one line of
//                          36 limbs (x, y, zz, zzz) per output; the affine conversion is the caller's.
//   host_ecntt add FILE    FILE: lines of 72 limbs (P, Q), or "acc" and 36 limbs (P = the previous line's result).  Prints
//                          add29pt(P, Q), 36 limbs a line.
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../zkevm-circuits_amd/csrc/ec29.hip.hpp"

using namespace zk;

static bool read_word(FILE* f, char (&buf)[80]) { return fscanf(f, "%79s", buf) == 1; }
template <class F>
static F parse_hex(const char* buf) {
    const size_t len = strlen(buf);
    if (len == 0 || len > 64) { fprintf(stderr, "bad value '%s'\n", buf); exit(2); }
    F out = F::zero();
    for (size_t i = 0; i < len; ++i) {
        const char ch = buf[len - 1 - i];
        const uint32_t d = ch >= '0' && ch <= '9' ? ch - '0' : ch >= 'a' && ch <= 'f' ? ch - 'a' + 10 : 16;
        if (d > 15) { fprintf(stderr, "bad value '%s'\n", buf); exit(2); }
        out.l[i / 8] |= d << (4 * (i % 8));
    }
    return out;
}
template <class F>
static F need_hex(FILE* f) {
    char buf[80];
    if (!read_word(f, buf)) { fprintf(stderr, "input ends early\n"); exit(2); }
    return parse_hex<F>(buf);
}
static bool read_limbs(FILE* f, uint32_t* out, int count, const char* first) {
    char buf[80];
    for (int i = 0; i < count; ++i) {
        if (i == 0 && first) { memcpy(buf, first, sizeof buf); }
        else if (!read_word(f, buf)) { if (i == 0) return false; fprintf(stderr, "input ends early\n"); exit(2); }
        char* end = nullptr;
        const unsigned long v = strtoul(buf, &end, 16);
        if (*end || v > 0xFFFFFFFFul) { fprintf(stderr, "bad limb '%s'\n", buf); exit(2); }
        out[i] = (uint32_t)v;
    }
    return true;
}
static G1Xyzz29 point_of(const uint32_t* w) {
    G1Xyzz29 r;
    for (int i = 0; i < 9; ++i) { r.x.l[i] = w[i]; r.y.l[i] = w[9 + i]; r.zz.l[i] = w[18 + i]; r.zzz.l[i] = w[27 + i]; }
    return r;
}
static void print_point(const G1Xyzz29& p) {
    const Fq29* c[4] = {&p.x, &p.y, &p.zz, &p.zzz};
    for (int t = 0; t < 4; ++t) for (int i = 0; i < 9; ++i) printf("%" PRIx32 "%c", c[t]->l[i], t == 3 && i == 8 ? '\n' : ' ');
}

// v < K p, by value (v normalised)
static bool below_kp(const Fq29& v, int K) {
    unsigned __int128 acc = 0;
    uint32_t kp[9];
    for (int i = 0; i < 9; ++i) {                          // limbs of K p
        acc += (unsigned __int128)K * Fq29P::M(i);
        kp[i] = i < 8 ? (uint32_t)acc & MASK29 : (uint32_t)acc;
        acc >>= 29;
    }
    for (int i = 8; i >= 0; --i) {
        if (v.l[i] < kp[i]) return true;
        if (v.l[i] > kp[i]) return false;
    }
    return false;
}
static bool keeps_invariant(const G1Xyzz29& p) {
    if (is_identity29(p)) return true;
    const Fq29* c[4] = {&p.x, &p.y, &p.zz, &p.zzz};
    for (int t = 0; t < 4; ++t) {
        for (int i = 0; i < 8; ++i) if (c[t]->l[i] > MASK29) return false;
        if (!below_kp(*c[t], t < 2 ? 8 : 2)) return false;
    }
    return true;
}
// 0 generic, 1 doubling, 2 cancellation, 3 identity operand: p + q seen through canonical representatives of the cross products
static int classify(const G1Xyzz29& p, const G1Xyzz29& q) {
    if (is_identity29(p) || is_identity29(q)) return 3;
    if (!(pack29(mul29(p.x, q.zz)) == pack29(mul29(q.x, p.zz)))) return 0;
    return pack29(mul29(p.y, q.zzz)) == pack29(mul29(q.y, p.zzz)) ? 1 : 2;
}
static uint32_t bitrev(uint32_t x, int bits) {
    uint32_t r = 0;
    for (int i = 0; i < bits; ++i) r |= ((x >> i) & 1u) << (bits - 1 - i);
    return r;
}

static int run_fft(FILE* f) {
    unsigned k = 0;
    if (fscanf(f, "%u", &k) != 1 || k > 12) { fprintf(stderr, "bad k\n"); return 2; }
    const size_t n = (size_t)1 << k;
    const Fr omega_inv = need_hex<Fr>(f), n_inv = need_hex<Fr>(f);
    std::vector<G1Xyzz29> pts(n);
    for (size_t i = 0; i < n; ++i) {                       // k_ecntt_load
        G1Affine p{need_hex<Fq>(f), need_hex<Fq>(f)};
        G1Xyzz29 q = identity29();
        if (!p.is_identity()) {
            for (int t = 0; t < 5; ++t) { p.x = dbl(p.x); p.y = dbl(p.y); }
            q = G1Xyzz29{unpack29<Fq29P>(p.x), unpack29<Fq29P>(p.y), one29(), one29()};
        }
        pts[bitrev((uint32_t)i, (int)k)] = q;
    }
    std::vector<Fr> tw(n / 2 ? n / 2 : 1);                 // k_powers: Montgomery omega^-j
    tw[0] = Fr::one();
    for (size_t j = 1; j < tw.size(); ++j) tw[j] = tw[j - 1] * omega_inv;
    for (unsigned s = 0; s < k; ++s) {                     // k_ecntt_stage
        unsigned long kinds[4] = {0, 0, 0, 0};
        for (size_t b = 0; b < n / 2; ++b) {
            const size_t half = (size_t)1 << s, j = b & (half - 1);
            const size_t i0 = ((b >> s) << (s + 1)) | j, i1 = i0 + half;
            const G1Xyzz29 u = pts[i0], v = pts[i1];
            Fr w = Fr::zero();
            if (j) w = from_mont(tw[j << (k - 1 - s)]);
            const G1Xyzz29 wv = j ? mul_scalar29(v, w) : v;            // for the classification only
            ++kinds[classify(u, wv)];
            ++kinds[classify(u, neg29pt(wv))];
            G1Xyzz29 lo, hi;
            ecntt_butterfly29(u, v, w, j != 0, &lo, &hi);
            if (!keeps_invariant(lo) || !keeps_invariant(hi)) {
                printf("stored invariant broken at stage %u butterfly %zu\n", s, b);
                print_point(lo);
                print_point(hi);
                return 1;
            }
            pts[i0] = lo;
            pts[i1] = hi;
        }
        printf("stage %u %lu %lu %lu\n", s, kinds[1], kinds[2], kinds[3]);
    }
    const Fr scale = from_mont(n_inv);                     // k_ecntt_finish up to the affine conversion
    for (size_t i = 0; i < n; ++i) print_point(mul_scalar29(pts[i], scale));
    return 0;
}

static int run_add(FILE* f) {
    G1Xyzz29 prev = identity29();
    char buf[80];
    while (read_word(f, buf)) {
        uint32_t w[72];
        G1Xyzz29 p;
        if (!strcmp(buf, "acc")) {
            p = prev;
            read_limbs(f, w, 36, nullptr);
            prev = add29pt(p, point_of(w));
        } else {
            read_limbs(f, w, 72, buf);
            prev = add29pt(point_of(w), point_of(w + 36));
        }
        print_point(prev);
    }
    return 0;
}

int main(int argc, char** argv) {
    if (argc != 3 || (strcmp(argv[1], "fft") && strcmp(argv[1], "add"))) { fprintf(stderr, "usage: %s fft|add FILE\n", argv[0]); return 2; }
    FILE* f = fopen(argv[2], "r");
    if (!f) { perror(argv[2]); return 2; }
    const int rc = strcmp(argv[1], "fft") ? run_add(f) : run_fft(f);
    fclose(f);
    return rc;
}

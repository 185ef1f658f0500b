// The per-lane code of ZK_OP_KECCAK (csrc/keccak.hip): Keccak-256 of one message (pad byte 0x01, rate 136, as host::keccak256 of
// csrc/host_hash.hpp) with the 25 x 64-bit state in registers, and the two challenge-phase columns of the reference's KeccakTable on
// 9 x 29-bit limbs (csrc/ff29.hip.hpp).  __host__ __device__, so that tests/host_keccak_harness.hip runs it on the CPU against Python.
//
// Absorbing.  A block is 17 little-endian 64-bit words.  A word that lies wholly inside the message is ONE 8-byte load at the
// message's own alignment (memcpy of 8 bytes: gfx950 takes global loads at any byte address, the host compiler makes of it what its
// target allows) -- exactly the bytes p .. p + 7, so an aligned start needs no path of its own and no start address is assumed.  The
// word the message ends in is put together from byte loads, at most seven, with the pad byte 0x01 behind the last one; the words
// behind it are zero, and 0x80 goes to byte 135 (0x81 when the two meet).  A length that is a multiple of 136, zero included, gives
// a block of padding alone.  Nothing outside [p, p + len) is read.
//
// RLCs.  Both columns are Horner sums over bytes, sum_k b_k r^(L-1-k), held as Montgomery images.  They are taken EIGHT BYTES PER
// REDUCTION, in the form of scan_rlc29_step:  z <- (z M_8 + sum_(t<8) b_t K_(7-t)) 2^-261  with the plain constants M_e = r^e 2^261
// and K_e = r^e 2^517, which is the image of z r^8 + sum_t b_t r^(7-t): 81 + 72 products and the 81 of the one reduction.  A tail of
// k < 8 bytes is the same step with the bytes moved to the last k places (the places before them hold zero) and M_k in M_8's place.
// The sixteen records of a challenge (KckPow) are made on the host and are wave-uniform; only the tail's M_k is chosen per lane.
//   output_rlc = the sum over the 32 digest bytes (four steps; the 32 Horner steps in r are the same polynomial in r^8),
//   input_rlc  = the sum over the message bytes, in a walk of its own AHEAD of the hash (kck_input_rlc: a rolled loop, one step per
//                word, 17 per full block): the registers of a lane are then the larger of the two phases, not their sum, and the
//                step's code exists once.  The message is read twice; the second read comes from the caches.
// Bounds: z is normalised and below 2p (rlc29_reduce's result), T = z M + sum b K < 2p p + 8 * 256 p < 2^261 p, and the fullest
// column takes 1 + 9 + 8 products, far below RLC29_MAX_LOAD: rlc29_mac never runs a carry pass here.
#pragma once
#include <cstring>

#include "ff29.hip.hpp"
#include "op_check.hpp"

namespace zk {

constexpr uint32_t KCK_RATE = 136, KCK_WORDS = KCK_RATE / 8;

__host__ __device__ constexpr uint64_t kck_rc(int r) {
    constexpr uint64_t rc[24] = {0x0000000000000001ULL, 0x0000000000008082ULL, 0x800000000000808AULL, 0x8000000080008000ULL, 0x000000000000808BULL, 0x0000000080000001ULL,
                                 0x8000000080008081ULL, 0x8000000000008009ULL, 0x000000000000008AULL, 0x0000000000000088ULL, 0x0000000080008009ULL, 0x000000008000000AULL,
                                 0x000000008000808BULL, 0x800000000000008BULL, 0x8000000000008089ULL, 0x8000000000008003ULL, 0x8000000000008002ULL, 0x8000000000000080ULL,
                                 0x000000000000800AULL, 0x800000008000000AULL, 0x8000000080008081ULL, 0x8000000000008080ULL, 0x0000000080000001ULL, 0x8000000080008008ULL};
    return rc[r];
}
__host__ __device__ constexpr int kck_rot(int i) {          // [x + 5 y]
    constexpr int rot[25] = {0, 1, 62, 28, 27, 36, 44, 6, 55, 20, 3, 10, 43, 25, 39, 41, 45, 15, 21, 8, 18, 2, 61, 56, 14};
    return rot[i];
}
template <int N>
__host__ __device__ __forceinline__ uint64_t kck_rol(uint64_t v) {
    if constexpr (N == 0) return v;
    else return (v << N) | (v >> (64 - N));
}
// rho and pi for the lanes of one x: a compile-time recursion, so that every rotation count is a constant
template <int X, int Y>
__host__ __device__ __forceinline__ void kck_rho_pi(uint64_t (&b)[25], const uint64_t (&a)[25]) {
    b[Y + 5 * ((2 * X + 3 * Y) % 5)] = kck_rol<kck_rot(X + 5 * Y)>(a[X + 5 * Y]);
    if constexpr (Y < 4) kck_rho_pi<X, Y + 1>(b, a);
    else if constexpr (X < 4) kck_rho_pi<X + 1, 0>(b, a);
}
// Keccak-f[1600].  The round loop is kept rolled: the round counter is wave-uniform, so the round constant is a scalar load.
__host__ __device__ inline void kck_f1600(uint64_t (&a)[25]) {
#pragma unroll 1
    for (int r = 0; r < 24; ++r) {
        uint64_t c[5], b[25];
#pragma unroll
        for (int x = 0; x < 5; ++x) c[x] = a[x] ^ a[x + 5] ^ a[x + 10] ^ a[x + 15] ^ a[x + 20];
#pragma unroll
        for (int x = 0; x < 5; ++x) {
            const uint64_t d = c[(x + 4) % 5] ^ kck_rol<1>(c[(x + 1) % 5]);
#pragma unroll
            for (int y = 0; y < 5; ++y) a[x + 5 * y] ^= d;
        }
        kck_rho_pi<0, 0>(b, a);
#pragma unroll
        for (int y = 0; y < 5; ++y)
#pragma unroll
            for (int x = 0; x < 5; ++x) a[x + 5 * y] = b[x + 5 * y] ^ (~b[(x + 1) % 5 + 5 * y] & b[(x + 2) % 5 + 5 * y]);
        a[0] ^= kck_rc(r);
    }
}

// the sixteen limb records of one challenge r: m[e - 1] = r^e 2^261 (e = 1 .. 8), k[e] = r^e 2^517 (e = 0 .. 7); plain, canonical
struct KckPow {
    uint32_t m[8][9];
    uint32_t k[8][9];
};
// from the Montgomery image of r; host side, once per call
inline KckPow kck_pow_table(const Fr& r) {
    const Fr c261 = fr_pow2(261), c517 = fr_pow2(517);  // the integers 2^261 and 2^517 mod p
    KckPow t;
    Fr pw = Fr::one();
    for (int e = 0; e <= 8; ++e) {
        if (e < 8) { const Fr29 l = unpack29<Fr29P>(pw * c517); for (int j = 0; j < 9; ++j) t.k[e][j] = l.l[j]; }
        if (e > 0) { const Fr29 l = unpack29<Fr29P>(pw * c261); for (int j = 0; j < 9; ++j) t.m[e - 1][j] = l.l[j]; }
        pw = pw * r;
    }
    return t;
}

// z <- the image of z r^e + sum_(t<8) b_t r^(7-t), b_t = byte t of w (the byte at the lowest address first), M = r^e 2^261
__host__ __device__ __forceinline__ Fr29 kck_rlc8(const Fr29& z, uint64_t w, const uint32_t* M, const KckPow& pw) {
    Rlc29<Fr29P> t;
    const uint32_t zero[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    rlc29_init(t, zero);
    rlc29_mac<9>(t, z.l, M);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const uint32_t b = (uint32_t)(w >> (8 * i)) & 0xffu;
        rlc29_mac<1>(t, &b, pw.k[7 - i]);
    }
    return rlc29_reduce(t);
}

__host__ __device__ __forceinline__ uint64_t kck_load8(const uint8_t* p) {
    uint64_t w;
    memcpy(&w, p, 8);
    return w;
}
__host__ __device__ __forceinline__ void kck_store8(uint8_t* p, uint64_t w) { memcpy(p, &w, 8); }

// M |= m[E - 1] where k = E, for E .. 7 (a compile-time recursion; masks, so that the records stay scalar operands)
template <uint32_t E>
__host__ __device__ __forceinline__ void kck_pick(uint32_t (&M)[9], uint32_t k, const KckPow& pw) {
    const uint32_t mask = k == E ? ~0u : 0u;
#pragma unroll
    for (int j = 0; j < 9; ++j) M[j] |= pw.m[E - 1][j] & mask;
    if constexpr (E < 7) kck_pick<E + 1>(M, k, pw);
}

// Word J of a block and the words behind it (a compile-time recursion: the state index must be a constant): the first `full` words
// come whole from the message, word `full` is `end` (the last bytes and the pad byte), the rest stay as they are.
template <uint32_t J>
__host__ __device__ __forceinline__ void kck_absorb(const uint8_t* p, uint32_t full, uint64_t end, uint64_t (&a)[25]) {
    if (J < full) a[J] ^= kck_load8(p + 8 * J);
    else if (J == full) a[J] ^= end;
    if constexpr (J + 1 < KCK_WORDS) kck_absorb<J + 1>(p, full, end, a);
}

// the k < 8 bytes at q as the low bytes of a word, by byte loads
__host__ __device__ __forceinline__ uint64_t kck_tail(const uint8_t* q, uint32_t k) {
    uint64_t tail = 0;
#pragma unroll
    for (uint32_t t = 0; t < 7; ++t)
        if (t < k) tail |= (uint64_t)q[t] << (8 * t);
    return tail;
}

// Keccak-256 of the len bytes at p into the state a (which enters as zero): the digest is the first 32 bytes of a[0 .. 3]
__host__ __device__ inline void kck_hash(const uint8_t* p, uint64_t len, uint64_t (&a)[25]) {
    for (;;) {
        const bool last = len < KCK_RATE;
        uint32_t full = KCK_WORDS, k = 0;               // whole words of this block; bytes of the message in the word behind them
        uint64_t tail = 0;
        if (last) {
            full = (uint32_t)len >> 3;
            k = (uint32_t)len & 7u;
            tail = kck_tail(p + 8 * full, k);
        }
        kck_absorb<0>(p, full, tail | (1ull << (8 * k)), a);            // the pad byte 0x01 behind the last byte
        if (last) a[KCK_WORDS - 1] ^= 0x80ull << 56;
        kck_f1600(a);
        if (last) return;
        p += KCK_RATE;
        len -= KCK_RATE;
    }
}

// The image of input_rlc of the len bytes at p under the records pin: a walk of its own over the message, one 8-byte load and one
// step per word in a rolled loop (the next word is fetched while the step runs), then the tail of len mod 8 bytes.
__host__ __device__ inline Fr29 kck_input_rlc(const uint8_t* p, uint64_t len, const KckPow& pin) {
    Fr29 z;
#pragma unroll
    for (int j = 0; j < 9; ++j) z.l[j] = 0;
    const uint64_t words = len >> 3;
    const uint32_t k = (uint32_t)len & 7u;
    uint64_t w = words ? kck_load8(p) : 0;
#pragma unroll 1
    for (uint64_t j = 0; j < words; ++j) {
        const uint64_t next = j + 1 < words ? kck_load8(p + 8 * (j + 1)) : 0;
        z = kck_rlc8(z, w, pin.m[7], pin);
        w = next;
    }
    if (k) {                                            // the k bytes in the last k places under r^k
        uint32_t M[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};    // M_k, chosen per lane from seven wave-uniform records by masks
        kck_pick<1>(M, k, pin);
        z = kck_rlc8(z, kck_tail(p + 8 * words, k) << (64 - 8 * k), M, pin);
    }
    return z;
}

// whether the len bytes at offset off lie inside a buffer of total bytes; neither comparison can wrap
__host__ __device__ __forceinline__ bool kck_in_range(uint64_t total, uint64_t off, uint64_t len) { return off <= total && len <= total - off; }

// One message: the digest as four little-endian words (its 32 bytes in memory order), output_rlc and, with RLC, input_rlc (zero
// without); both canonical
template <bool RLC>
__host__ __device__ inline void kck_message(const uint8_t* p, uint64_t len, const KckPow& pout, const KckPow* pin, uint64_t (&digest)[4], Fr& out, Fr& in) {
    if constexpr (RLC) in = pack29_lt2p(kck_input_rlc(p, len, *pin));
    else in = Fr::zero();
    uint64_t a[25];
#pragma unroll
    for (int j = 0; j < 25; ++j) a[j] = 0;
    kck_hash(p, len, a);
    Fr29 h;
#pragma unroll
    for (int j = 0; j < 9; ++j) h.l[j] = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        digest[j] = a[j];
        h = kck_rlc8(h, a[j], pout.m[7], pout);
    }
    out = pack29_lt2p(h);
}

// what a row writes
struct KckOut {
    uint64_t digest[4];
    Fr out, in;
};
// Row i of the op as the host harness runs it (k_keccak makes the same two calls).  A message that does not lie inside [bytes, bytes +
// total) reads nothing and gives zeros; false is returned for it.
template <bool RLC>
__host__ __device__ inline bool kck_row(const uint8_t* bytes, uint64_t total, uint64_t off, uint64_t len, const KckPow& pout, const KckPow* pin, KckOut& o) {
    if (!kck_in_range(total, off, len)) {
        for (int j = 0; j < 4; ++j) o.digest[j] = 0;
        o.out = Fr::zero();
        o.in = Fr::zero();
        return false;
    }
    kck_message<RLC>(bytes + off, len, pout, pin, o.digest, o.out, o.in);
    return true;
}

// entry i of an index column of 4- or 8-byte little-endian unsigned integers, aligned to its width
__host__ __device__ __forceinline__ uint64_t kck_index(const void* p, uint32_t width, uint64_t i) {
    return width == 4 ? (uint64_t)reinterpret_cast<const uint32_t*>(p)[i] : reinterpret_cast<const uint64_t*>(p)[i];
}

}  // namespace zk

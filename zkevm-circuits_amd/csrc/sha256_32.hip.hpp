// The per-lane code of ZK_OP_SHA256 (csrc/sha256.hip): SHA-256 (FIPS 180-4) of one message with the eight 32-bit state words and a
// rolling schedule of 16 words in registers, and the two challenge-phase columns of the reference's SHA256Table, which are those of
// the KeccakTable: the RLC code is csrc/keccak64.hip.hpp's as it stands (KckPow, kck_rlc8, kck_input_rlc, kck_in_range, kck_index,
// kck_load8, kck_tail, kck_store8).  __host__ __device__, so that tests/host_sha256_harness.hip runs it on the CPU against Python.
//
// Blocks.  A block is sixteen BIG-endian 32-bit words.  Two of them that lie wholly inside the message are ONE 8-byte load at the
// message's own alignment (kck_load8: exactly the bytes p .. p + 7) and a byte swap of each half; the eight bytes the message ends in
// are put together from byte loads, at most seven (kck_tail), with the pad byte 0x80 behind the last one, under per-word tests as
// Keccak's absorbing makes them; the words behind are zero.  The last two words of the FINAL block hold the length in bits, 64-bit
// big-endian.  With len mod 64 < 56 the block the message ends in is the final one; otherwise (56 .. 63: no room behind the pad
// byte) a second block of zeros and the length follows.  A length that is a multiple of 64, zero included, gives a block of padding
// alone.  Nothing outside [p, p + len) is read.  len < 2^61 (the host side refuses more bytes than that), so len * 8 does not wrap.
//
// Rounds.  All 64 are unrolled by a compile-time recursion: the schedule index t & 15, the places of a .. h in the state and the
// round constant are constants of each round, nothing is indexed at run time and no word is moved between rounds.
//
// RLCs.  output_rlc = sum_k digest[k] r^(31-k) is four kck_rlc8 steps.  kck_rlc8 gives the byte in bits [8j, 8j + 8) of its word the
// power r^(7-j): the word has to hold the digest bytes in memory order, so each pair (H[2j], H[2j+1]) is byte-swapped into the
// little-endian word H[2j]'s most significant byte is the lowest byte of -- the same four words are the digest as it is stored.
// input_rlc is kck_input_rlc unchanged, a walk of its own ahead of the hash.
#pragma once
#include "keccak64.hip.hpp"

namespace zk {

// FIPS 180-4, 4.2.2 and 5.3.3
__host__ __device__ constexpr uint32_t sha_k(int t) {
    constexpr uint32_t k[64] = {0x428a2f98u, 0x71374491u, 0xb5c0fbcfu, 0xe9b5dba5u, 0x3956c25bu, 0x59f111f1u, 0x923f82a4u, 0xab1c5ed5u, 0xd807aa98u, 0x12835b01u, 0x243185beu,
                                0x550c7dc3u, 0x72be5d74u, 0x80deb1feu, 0x9bdc06a7u, 0xc19bf174u, 0xe49b69c1u, 0xefbe4786u, 0x0fc19dc6u, 0x240ca1ccu, 0x2de92c6fu, 0x4a7484aau,
                                0x5cb0a9dcu, 0x76f988dau, 0x983e5152u, 0xa831c66du, 0xb00327c8u, 0xbf597fc7u, 0xc6e00bf3u, 0xd5a79147u, 0x06ca6351u, 0x14292967u, 0x27b70a85u,
                                0x2e1b2138u, 0x4d2c6dfcu, 0x53380d13u, 0x650a7354u, 0x766a0abbu, 0x81c2c92eu, 0x92722c85u, 0xa2bfe8a1u, 0xa81a664bu, 0xc24b8b70u, 0xc76c51a3u,
                                0xd192e819u, 0xd6990624u, 0xf40e3585u, 0x106aa070u, 0x19a4c116u, 0x1e376c08u, 0x2748774cu, 0x34b0bcb5u, 0x391c0cb3u, 0x4ed8aa4au, 0x5b9cca4fu,
                                0x682e6ff3u, 0x748f82eeu, 0x78a5636fu, 0x84c87814u, 0x8cc70208u, 0x90befffau, 0xa4506cebu, 0xbef9a3f7u, 0xc67178f2u};
    return k[t];
}
__host__ __device__ constexpr uint32_t sha_h0(int i) {
    constexpr uint32_t h[8] = {0x6a09e667u, 0xbb67ae85u, 0x3c6ef372u, 0xa54ff53au, 0x510e527fu, 0x9b05688cu, 0x1f83d9abu, 0x5be0cd19u};
    return h[i];
}

template <int N>
__host__ __device__ __forceinline__ uint32_t sha_ror(uint32_t v) { return (v >> N) | (v << (32 - N)); }
__host__ __device__ __forceinline__ uint32_t sha_bswap(uint32_t v) { return __builtin_bswap32(v); }
// a ^ b ^ c.  gfx950 has no v_xor3_b32; its v_bitop3_b32 with the truth table 0x96 is that instruction, and the compiler does not
// choose it for two xors by itself (profiles/r26_sha256.md: 1 902 instructions per block without it, 1 725 with it).
__host__ __device__ __forceinline__ uint32_t sha_xor3(uint32_t a, uint32_t b, uint32_t c) {
#if defined(__HIP_DEVICE_COMPILE__) && __has_builtin(__builtin_amdgcn_bitop3_b32)
    return __builtin_amdgcn_bitop3_b32(a, b, c, 0x96);
#else
    return a ^ b ^ c;
#endif
}

// Round T and the rounds behind it.  The working variables a .. h of round T are s[(0 - T) & 7] .. s[(7 - T) & 7]: a round writes
// its d and its h, which are the next round's e and a.
template <int T>
__host__ __device__ __forceinline__ void sha_rounds(uint32_t (&s)[8], uint32_t (&w)[16]) {
    if constexpr (T >= 16) {
        const uint32_t w15 = w[(T - 15) & 15], w2 = w[(T - 2) & 15];
        w[T & 15] += sha_xor3(sha_ror<7>(w15), sha_ror<18>(w15), w15 >> 3) + w[(T - 7) & 15] + sha_xor3(sha_ror<17>(w2), sha_ror<19>(w2), w2 >> 10);
    }
    const uint32_t a = s[(0 - T) & 7], b = s[(1 - T) & 7], c = s[(2 - T) & 7], e = s[(4 - T) & 7], f = s[(5 - T) & 7], g = s[(6 - T) & 7];
    uint32_t& d = s[(3 - T) & 7];
    uint32_t& h = s[(7 - T) & 7];
    const uint32_t ab = a ^ b;
    h += sha_xor3(sha_ror<6>(e), sha_ror<11>(e), sha_ror<25>(e)) + ((e & f) | (~e & g)) + sha_k(T) + w[T & 15];
    d += h;
    h += sha_xor3(sha_ror<2>(a), sha_ror<13>(a), sha_ror<22>(a)) + ((ab & c) | (~ab & b));      // Maj: where a and b differ c decides
    if constexpr (T < 63) sha_rounds<T + 1>(s, w);
}

// one block: H <- H + the 64 rounds of H over the schedule that starts as w (w is used up)
__host__ __device__ __forceinline__ void sha_compress(uint32_t (&H)[8], uint32_t (&w)[16]) {
    uint32_t s[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) s[i] = H[i];
    sha_rounds<0>(s, w);
#pragma unroll
    for (int i = 0; i < 8; ++i) H[i] += s[i];
}

// Words 2J and 2J + 1 of a block and the pairs behind them (a compile-time recursion): the first `full` pairs come whole from the
// message, pair `full` is `end` (the last bytes and the pad byte, in memory order), the rest are zero.
template <uint32_t J>
__host__ __device__ __forceinline__ void sha_load(const uint8_t* p, uint32_t full, uint64_t end, uint32_t (&w)[16]) {
    uint64_t v = 0;
    if (J < full) v = kck_load8(p + 8 * J);
    else if (J == full) v = end;
    w[2 * J] = sha_bswap((uint32_t)v);
    w[2 * J + 1] = sha_bswap((uint32_t)(v >> 32));
    if constexpr (J + 1 < 8) sha_load<J + 1>(p, full, end, w);
}

// SHA-256 of the len bytes at p: H[0 .. 7], the digest being their big-endian bytes in this order
__host__ __device__ inline void sha_hash(const uint8_t* p, uint64_t len, uint32_t (&H)[8]) {
#pragma unroll
    for (int i = 0; i < 8; ++i) H[i] = sha_h0(i);
    const uint64_t bits = len << 3;
    uint64_t rem = len;                                 // bytes of the message not yet taken
    bool padded = false;                                // the pad byte went into the block before this one
    for (;;) {
        const bool ends = rem < 64;                     // the message ends in this block (or ended in the one before)
        uint32_t full = 8;                              // whole pairs of words of this block
        uint64_t end = 0;
        if (ends) {
            full = (uint32_t)rem >> 3;
            const uint32_t k = (uint32_t)rem & 7u;
            if (!padded) end = kck_tail(p + 8 * full, k) | (0x80ull << (8 * k));
        }
        uint32_t w[16];
        sha_load<0>(p, full, end, w);
        const bool final_block = rem < 56;              // room for the length behind the pad byte
        if (final_block) {
            w[14] = (uint32_t)(bits >> 32);
            w[15] = (uint32_t)bits;
        }
        sha_compress(H, w);
        if (final_block) return;
        if (ends) {                                     // 56 .. 63 bytes: a second block, zeros and the length
            padded = true;
            rem = 0;
        } else {
            p += 64;
            rem -= 64;
        }
    }
}

// the digest as four little-endian words: its 32 bytes in memory order, H[0]'s most significant byte first
__host__ __device__ __forceinline__ void sha_digest_words(const uint32_t (&H)[8], uint64_t (&digest)[4]) {
#pragma unroll
    for (int j = 0; j < 4; ++j) digest[j] = (uint64_t)sha_bswap(H[2 * j]) | (uint64_t)sha_bswap(H[2 * j + 1]) << 32;
}

// One message: the digest (as sha_digest_words), output_rlc and, with RLC, input_rlc (zero without); both canonical
template <bool RLC>
__host__ __device__ inline void sha_message(const uint8_t* p, uint64_t len, const KckPow& pout, const KckPow* pin, uint64_t (&digest)[4], Fr& out, Fr& in) {
    if constexpr (RLC) in = pack29_lt2p(kck_input_rlc(p, len, *pin));
    else in = Fr::zero();
    uint32_t H[8];
    sha_hash(p, len, H);
    sha_digest_words(H, digest);
    Fr29 h;
#pragma unroll
    for (int j = 0; j < 9; ++j) h.l[j] = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) h = kck_rlc8(h, digest[j], pout.m[7], pout);
    out = pack29_lt2p(h);
}

// Row i of the op as the host harness runs it (k_sha256 makes the same two calls; KckOut is what a row writes).  A message that does
// not lie inside [bytes, bytes + total) reads nothing and gives zeros; false is returned for it.
template <bool RLC>
__host__ __device__ inline bool sha_row(const uint8_t* bytes, uint64_t total, uint64_t off, uint64_t len, const KckPow& pout, const KckPow* pin, KckOut& o) {
    if (!kck_in_range(total, off, len)) {
        for (int j = 0; j < 4; ++j) o.digest[j] = 0;
        o.out = Fr::zero();
        o.in = Fr::zero();
        return false;
    }
    sha_message<RLC>(bytes + off, len, pout, pin, o.digest, o.out, o.in);
    return true;
}

}  // namespace zk

// Lane-free code of ZK_OP_KEY_SORT and ZK_OP_KEY_ORDER (csrc/keysort.hip holds the kernels and the host side): what one lane does to
// one key record, and every index the radix sort computes.  Nothing here names a thread, a wave or LDS, so the host compiles it as it
// stands: tests/host_key_order_harness.hip runs the per-row code on chosen records and drives whole small sorts serially, lanes as a
// loop, through exactly these functions.
// A key record is 64 bytes, compared as a big-endian 512-bit integer (byte 0 most significant); limb j is the big-endian 16-bit number
// in bytes 2j, 2j + 1.  A lane holds a record the way it loaded it: eight little-endian 64-bit words (key byte k is byte k & 7 of word
// k >> 3), or the same as sixteen 32-bit words.
#pragma once
#include "ff.hip.hpp"

namespace zk {

#define ZK_KO_HD __host__ __device__ __forceinline__

// ---- the sort: geometry and index arithmetic ------------------------------------------------------------------------------------------
// A pass orders the permutation by ONE key byte (an 8-bit digit), stably.  A workgroup of KS_LANES lanes takes a tile of KS_TILE
// consecutive places of the current permutation: wave w the KS_ITEMS * 64 places from w * KS_ITEMS * 64, round r of that wave the 64
// places from r * 64 of those, lane l the l-th.  The order of the places of a tile is therefore (wave, round, lane), the order in
// which the ranks are given out.
constexpr uint32_t KS_LANES = 256, KS_WAVES = KS_LANES / 64, KS_ITEMS = 8, KS_TILE = KS_LANES * KS_ITEMS, KS_BINS = 256;

ZK_KO_HD uint64_t ks_tiles(uint64_t n) { return n / KS_TILE + (n % KS_TILE ? 1 : 0); }
ZK_KO_HD uint64_t ks_pos(uint64_t tile, uint32_t wave, uint32_t round, uint32_t lane) { return tile * KS_TILE + (uint64_t)wave * (KS_ITEMS * 64) + round * 64 + lane; }
// the counts of a pass: bin-major, so that ONE exclusive scan along the array is the stable order (every smaller digit first, then the
// same digit in earlier tiles)
ZK_KO_HD uint64_t ks_count_at(uint32_t bin, uint64_t tile, uint64_t tiles) { return (uint64_t)bin * tiles + tile; }
// Masks of key bytes: bit j is key byte j.  `vary` (made on the device) has the bytes at which some record differs from record 0,
// `keep` (the host's mask) the bytes that take part; a pass is live when both have its byte.  The passes run from byte 63 up to byte 0
// and only a live pass moves the permutation to the other buffer, so the buffer a pass reads (0 or 1) is the parity of the live bytes
// below it in significance, which every workgroup works out for itself.
ZK_KO_HD uint64_t ks_live(uint64_t vary, uint64_t keep) { return vary & keep; }
ZK_KO_HD bool ks_pass_live(uint64_t live, uint32_t byte) { return (live >> byte & 1) != 0; }
ZK_KO_HD uint32_t ks_popc64(uint64_t x) { return (uint32_t)__builtin_popcountll(x); }
ZK_KO_HD uint32_t ks_source(uint64_t live, uint32_t byte) { return byte >= 63 ? 0u : ks_popc64(live >> (byte + 1)) & 1u; }
ZK_KO_HD uint32_t ks_result(uint64_t live) { return ks_popc64(live) & 1u; }
// the bytes at which x = record ^ record 0 is not zero
ZK_KO_HD uint64_t ks_vary_bits(const uint64_t (&x)[8]) {
    uint64_t m = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
#pragma unroll
        for (int b = 0; b < 8; ++b) m |= (uint64_t)((x[k] >> (8 * b) & 0xff) != 0) << (8 * k + b);
    }
    return m;
}
// The lanes of a wave that hold the digit of this lane: ballot[b] has the lanes that are valid and whose digit has bit b set, `valid`
// the lanes whose place lies below n.  The rank of a lane among its wave's 64 places is the number of such lanes below it.
ZK_KO_HD uint64_t ks_peers(const uint64_t (&ballot)[8], uint64_t valid, uint32_t digit) {
    uint64_t p = valid;
#pragma unroll
    for (int b = 0; b < 8; ++b) p &= (digit >> b & 1) ? ballot[b] : ~ballot[b];
    return p;
}
ZK_KO_HD uint32_t ks_rank_below(uint64_t peers, uint32_t lane) { return ks_popc64(peers & ((1ull << lane) - 1)); }
ZK_KO_HD uint32_t ks_leader(uint64_t peers) { return peers ? (uint32_t)__builtin_ctzll(peers) : 0u; }
// Where a place goes: records with a smaller digit (bin_base), with the same digit in earlier tiles (tile_base), in earlier waves of the
// tile (wave_base), in earlier rounds of the wave and below the lane in its round (rank).  The four are counts of disjoint sets of
// OTHER places, so their sum is below n; it is taken in 64 bits and compared with n before anything is stored.
ZK_KO_HD uint64_t ks_dest(uint32_t bin_base, uint32_t tile_base, uint32_t wave_base, uint32_t rank) { return (uint64_t)bin_base + tile_base + wave_base + rank; }

// ---- the order witness of one row ---------------------------------------------------------------------------------------------------------
ZK_KO_HD uint64_t ko_bswap64(uint64_t x) { return __builtin_bswap64(x); }
// first_different_limb (0..31; 31 for equal records) and the signed limb difference cur_j - prev_j, in -65535..65535: the first word
// that differs by selects from the last word down, the limb inside it from the leading zeros of the byte-swapped xor
ZK_KO_HD uint32_t key_first_diff(const uint64_t (&cur)[8], const uint64_t (&prev)[8], int32_t& d) {
    uint64_t x = 0, c = 0, p = 0;
    uint32_t w = 7;
#pragma unroll
    for (int k = 7; k >= 0; --k) {
        const uint64_t xk = cur[k] ^ prev[k];
        const bool hit = xk != 0;
        x = hit ? xk : x;
        c = hit ? cur[k] : c;
        p = hit ? prev[k] : p;
        w = hit ? (uint32_t)k : w;
    }
    d = 0;
    if (!x) return 31;
    x = ko_bswap64(x), c = ko_bswap64(c), p = ko_bswap64(p);
    const uint32_t limb = (uint32_t)__builtin_clzll(x) >> 4;            // 0: the most significant limb of the word
    const uint32_t sh = 48 - 16 * limb;
    d = (int32_t)(c >> sh & 0xffff) - (int32_t)(p >> sh & 0xffff);
    return 4 * w + limb;
}
// the difference as a canonical Montgomery element: d 2^256 mod r, r - |d| 2^256 mod r for a negative d
ZK_KO_HD Fr key_diff_fr(int32_t d) {
    const uint32_t a = d < 0 ? (uint32_t)(-d) : (uint32_t)d;
    const Fr m = to_mont(Fr{{a, 0, 0, 0, 0, 0, 0, 0}});
    return d < 0 ? neg(m) : m;
}
// entry a of the table of inverses: 1 / a as a canonical Montgomery element, 0 for a = 0
__host__ __device__ inline Fr key_inv_entry(uint32_t a) { return inv(to_mont(Fr{{a, 0, 0, 0, 0, 0, 0, 0}})); }
// limb_difference_inverse from the table entry of |d|
ZK_KO_HD Fr key_inv_signed(const Fr& entry, int32_t d) { return d < 0 ? neg(entry) : entry; }
// word s of sixteen by selects: the index is not a constant, and an indexed register array goes to scratch or to LDS.  Written out
// and started from 0, not from r[0]: a select between two LOADS is turned into a load through a selected pointer before this function
// is inlined, and the array is then indexed by a variable after all (16 KB of LDS per workgroup and 16-way bank conflicts, seen in the
// ISA).  s is the same for every lane, so these are selects on a scalar condition.
ZK_KO_HD uint32_t ko_word(const uint32_t (&r)[16], uint32_t s) {
    uint32_t v = 0;
#define ZK_KO_SEL(i) v = s == i##u ? r[i] : v;
    ZK_KO_SEL(0) ZK_KO_SEL(1) ZK_KO_SEL(2) ZK_KO_SEL(3) ZK_KO_SEL(4) ZK_KO_SEL(5) ZK_KO_SEL(6) ZK_KO_SEL(7) ZK_KO_SEL(8)
    ZK_KO_SEL(9) ZK_KO_SEL(10) ZK_KO_SEL(11) ZK_KO_SEL(12) ZK_KO_SEL(13) ZK_KO_SEL(14) ZK_KO_SEL(15)
#undef ZK_KO_SEL
    return v;
}
// the big-endian integer of key bytes [offset, offset + width), width 1, 2 or 4 and offset + width <= 64
ZK_KO_HD uint32_t key_gather(const uint32_t (&r)[16], uint32_t offset, uint32_t width) {
    const uint32_t s = offset >> 2;
    const uint64_t two = (uint64_t)ko_word(r, s) | (uint64_t)ko_word(r, s < 15 ? s + 1 : 15) << 32;
    const uint32_t bytes = (uint32_t)(two >> (8 * (offset & 3)));      // key byte offset in the low byte
    return __builtin_bswap32(bytes) >> (32 - 8 * width);
}
ZK_KO_HD bool key_col_ok(uint32_t offset, uint32_t width) { return (width == 1 || width == 2 || width == 4) && offset + width <= 64; }

}  // namespace zk

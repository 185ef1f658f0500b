// ZK_OP_KECCAK of zk_field_vec_op: the hash columns of the reference's KeccakTable from message bytes that live on the device, one
// lane per message.
//   digest_i = Keccak-256(the len_i bytes at d_bytes + off_i);  d_out[i] = sum_k digest_i[k] r_out^(31-k)  (output_rlc, hash_rlc);
//   d_digest[i] = the 32 digest bytes;  d_input_rlc[i] = sum_k m[k] r_in^(len-1-k).
// The per-lane code is csrc/keccak64.hip.hpp (absorbing at any alignment, the permutation with the state in registers, the RLCs eight
// bytes per reduction); the row, the checks and the launch are csrc/bytehash.hip.hpp, shared with ZK_OP_SHA256; this file holds the
// trait and the two kernels.
// Launch: one, lane = row.  k_keccak<false> is the plain call; k_keccak<true> also walks input_rlc and is a separate instantiation
// so that the plain call does not carry its registers.  The 16 + 16 limb records of the two challenges are made on the host per
// call and travel as kernel arguments: wave-uniform, fetched by scalar loads.  No LDS, no scratch, no host synchronisation: the
// offsets and lengths are device data, a row whose message does not lie inside the buffer writes zeros and reads nothing.
// Built and counted (gfx950 ISA, profiles/r25_keccak.md): a round of the permutation is 300 instructions, a permutation 7 200; an RLC
// step of eight bytes is 366 instructions (234 multiply-adds), the 17 steps of a full block 6 222.  k_keccak<false> takes 96 VGPRs,
// k_keccak<true> 90, five waves per SIMD either way.
// Lanes of a wave have different lengths and a wave takes as long as its longest message -- the trade ZK_OP_POSEIDON made; one long
// message among short ones costs its own blocks once per wave it sits in (profiles/r25_keccak.md has that measured).
#include "bytehash.hip.hpp"

namespace zk {

struct KeccakHash {
    using Desc = zk_keccak;
    static constexpr const char *name = "Keccak", *prof = "fr_keccak";
    static constexpr int TOTAL_LOG2 = 64;
};

template <bool RLC>
__global__ void __launch_bounds__(256) k_keccak(const HashArgs g, const KckPow pin) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= g.n) return;
    const uint64_t off = kck_index(g.offs, g.index_width, i), len = kck_index(g.lens, g.index_width, i);
    uint8_t* dg = g.digest ? g.digest + 32 * i : nullptr;
    if (!kck_in_range(g.total, off, len)) {             // zeros to every output of the row, nothing read
        if (dg) {
#pragma unroll
            for (int j = 0; j < 4; ++j) kck_store8(dg + 8 * j, 0);
        }
        stg(g.out + i, Fr::zero());
        if constexpr (RLC) stg(g.in_rlc + i, Fr::zero());
        return;
    }
    uint64_t digest[4];
    Fr out, in;
    kck_message<RLC>(g.bytes + off, len, g.pout, &pin, digest, out, in);
    if (dg) {
#pragma unroll
        for (int j = 0; j < 4; ++j) kck_store8(dg + 8 * j, digest[j]);
    }
    stg(g.out + i, out);
    if constexpr (RLC) stg(g.in_rlc + i, in);
}

int fr_keccak_run(zk_ctx* ctx, const zk_keccak* desc, const void* h_challenges, Fr* d_out, uint64_t n) { return byte_hash_run<KeccakHash>(ctx, desc, h_challenges, d_out, n, k_keccak<false>, k_keccak<true>); }

}  // namespace zk

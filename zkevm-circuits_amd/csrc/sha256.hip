// ZK_OP_SHA256 of zk_field_vec_op: the hash columns of the reference's SHA256Table from message bytes that live on the device, one
// lane per message.
//   digest_i = SHA-256(the len_i bytes at d_bytes + off_i);  d_out[i] = sum_k digest_i[k] r_out^(31-k)  (output_rlc, hashes_rlc);
//   d_digest[i] = the 32 digest bytes;  d_input_rlc[i] = sum_k m[k] r_in^(len-1-k).
// The per-lane code is csrc/sha256_32.hip.hpp (blocks at any alignment, the 64 unrolled rounds with state and schedule in
// registers) over the RLC code of csrc/keccak64.hip.hpp; the row, the checks and the launch are csrc/bytehash.hip.hpp, shared with
// ZK_OP_KECCAK; this file holds the trait and the two kernels.
// Launch: ZK_OP_KECCAK's.  One, lane = row, 256 lanes per workgroup.  k_sha256<false> is the plain call; k_sha256<true> also walks
// input_rlc ahead of the hash and is a separate instantiation so that the plain call does not carry its registers.  The 16 + 16 limb
// records of the two challenges are made on the host per call and travel as kernel arguments.  No LDS, no scratch, no host
// synchronisation: the offsets and lengths are device data, a row whose message does not lie inside the buffer writes zeros and
// reads nothing.
// Built and counted (gfx950 ISA, profiles/r26_sha256.md): a compression is 1 725 instructions, 27 per round, loading and padding a
// block 197; the four RLC steps on the digest and the stores 1 193 per message.  k_sha256<false> takes 87 VGPRs, k_sha256<true> 85,
// five waves per SIMD either way.
// Lanes of a wave have different lengths and a wave takes as long as its longest message -- the trade ZK_OP_KECCAK and
// ZK_OP_POSEIDON made; one long message among short ones costs its own blocks once per wave it sits in.
#include "bytehash.hip.hpp"
#include "sha256_32.hip.hpp"

namespace zk {

struct Sha256Hash {
    using Desc = zk_sha256;
    static constexpr const char *name = "SHA-256", *prof = "fr_sha256";
    static constexpr int TOTAL_LOG2 = 61;               // the length field of the padding holds a message's length in BITS as a 64-bit integer
};

template <bool RLC>
__global__ void __launch_bounds__(256) k_sha256(const HashArgs g, const KckPow pin) {
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
    sha_message<RLC>(g.bytes + off, len, g.pout, &pin, digest, out, in);
    if (dg) {
#pragma unroll
        for (int j = 0; j < 4; ++j) kck_store8(dg + 8 * j, digest[j]);
    }
    stg(g.out + i, out);
    if constexpr (RLC) stg(g.in_rlc + i, in);
}

int fr_sha256_run(zk_ctx* ctx, const zk_sha256* desc, const void* h_challenges, Fr* d_out, uint64_t n) { return byte_hash_run<Sha256Hash>(ctx, desc, h_challenges, d_out, n, k_sha256<false>, k_sha256<true>); }

}  // namespace zk

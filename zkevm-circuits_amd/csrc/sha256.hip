// ZK_OP_SHA256 of zk_field_vec_op: the hash columns of the reference's SHA256Table from message bytes that live on the device, one
// lane per message.
//   digest_i = SHA-256(the len_i bytes at d_bytes + off_i);  d_out[i] = sum_k digest_i[k] r_out^(31-k)  (output_rlc, hashes_rlc);
//   d_digest[i] = the 32 digest bytes;  d_input_rlc[i] = sum_k m[k] r_in^(len-1-k).
// The per-lane code is csrc/sha256_32.hip.hpp (blocks at any alignment, the 64 unrolled rounds with state and schedule in
// registers) over the RLC code of csrc/keccak64.hip.hpp; this file holds the two kernels and the host side.
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
#include "ctx.hpp"
#include "sha256_32.hip.hpp"

namespace zk {

struct ShaArgs {
    const uint8_t* bytes;
    uint64_t total;
    const void* offs;
    const void* lens;
    uint8_t* digest;                    // NULL: not wanted
    Fr* out;
    Fr* in_rlc;                         // k_sha256<true> only
    uint64_t n;
    uint32_t index_width;
    KckPow pout;
};

template <bool RLC>
__global__ void __launch_bounds__(256) k_sha256(const ShaArgs g, const KckPow pin) {
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

struct ShaSpan { uintptr_t lo, hi; const char* what; bool out; };

// h_challenges: r_out, then r_in, Montgomery Fr in host memory.  Everything is validated before n is looked at and before the
// launch, so a refused call has written nothing.
int fr_sha256_run(zk_ctx* ctx, const zk_sha256* desc, const void* h_challenges, Fr* d_out, uint64_t n) {
    const uint32_t iw = desc->index_width;
    if (desc->flags) return ctx->fail(ZK_ERR_INVALID_ARG, "SHA-256: flags 0x%x: must be 0", desc->flags);
    if (iw != 4 && iw != 8) return ctx->fail(ZK_ERR_INVALID_ARG, "SHA-256: index width %u: must be 4 or 8 bytes", iw);
    if (!desc->d_offsets || !desc->d_lens) return ctx->fail(ZK_ERR_INVALID_ARG, "SHA-256: NULL offsets or lengths");
    if ((uintptr_t)desc->d_offsets % iw || (uintptr_t)desc->d_lens % iw) return ctx->fail(ZK_ERR_INVALID_ARG, "SHA-256: offsets or lengths of %u bytes at a misaligned address", iw);
    if (!desc->d_bytes && desc->total_bytes) return ctx->fail(ZK_ERR_INVALID_ARG, "SHA-256: NULL d_bytes with %llu bytes", (unsigned long long)desc->total_bytes);
    // the length field of the padding holds a message's length in BITS as a 64-bit integer
    if (desc->total_bytes >> 61) return ctx->fail(ZK_ERR_INVALID_ARG, "SHA-256: %llu bytes: 2^61 or more", (unsigned long long)desc->total_bytes);
    if ((uintptr_t)d_out % 16 || (uintptr_t)desc->d_input_rlc % 16) return ctx->fail(ZK_ERR_INVALID_ARG, "SHA-256: an Fr output at an address that is no multiple of 16");
    const uint64_t blocks = n / 256 + (n % 256 ? 1 : 0);
    if (blocks > 0x7fffffffull) return ctx->fail(ZK_ERR_INVALID_ARG, "too many rows for one launch");
    // no output overlaps an input or another output
    ShaSpan span[6];
    int spans = 0;
    auto add = [&](const void* p, uint64_t len, const char* what, bool out) { if (p && len) span[spans++] = {(uintptr_t)p, (uintptr_t)p + len, what, out}; };
    add(d_out, n * sizeof(Fr), "d_out", true);
    add(desc->d_digest, n * 32, "d_digest", true);
    add(desc->d_input_rlc, n * sizeof(Fr), "d_input_rlc", true);
    add(desc->d_bytes, desc->total_bytes, "d_bytes", false);
    add(desc->d_offsets, n * iw, "d_offsets", false);
    add(desc->d_lens, n * iw, "d_lens", false);
    for (int a = 0; a < spans; ++a)
        for (int b = a + 1; b < spans; ++b)
            if ((span[a].out || span[b].out) && span[a].lo < span[b].hi && span[b].lo < span[a].hi)
                return ctx->fail(ZK_ERR_INVALID_ARG, "SHA-256: %s overlaps %s", span[a].what, span[b].what);
    if (!n) return ZK_OK;

    Fr r[2];
    memcpy(r, h_challenges, sizeof r);                  // all 64 bytes, whether r_in is used or not
    ShaArgs g;
    memset(&g, 0, sizeof g);
    g.bytes = (const uint8_t*)desc->d_bytes;
    g.total = desc->total_bytes;
    g.offs = desc->d_offsets;
    g.lens = desc->d_lens;
    g.digest = (uint8_t*)desc->d_digest;
    g.out = d_out;
    g.in_rlc = (Fr*)desc->d_input_rlc;
    g.n = n;
    g.index_width = iw;
    g.pout = kck_pow_table(r[0]);
    KckPow pin;
    memset(&pin, 0, sizeof pin);
    if (g.in_rlc) pin = kck_pow_table(r[1]);

    ZkProfScope prof(ctx, "fr_sha256");
    // the host cannot know the sum of the lengths: total_bytes stands in for the message bytes read
    prof.bytes = n * (2ull * iw + 32 + (g.digest ? 32 : 0) + (g.in_rlc ? 32 : 0)) + desc->total_bytes;
    if (g.in_rlc) hipLaunchKernelGGL(k_sha256<true>, dim3((unsigned)blocks), dim3(256), 0, ctx->stream, g, pin);
    else hipLaunchKernelGGL(k_sha256<false>, dim3((unsigned)blocks), dim3(256), 0, ctx->stream, g, pin);
    ZK_CHECK_LAUNCH(ctx);
    return ZK_OK;
}

}  // namespace zk

// What ZK_OP_KECCAK and ZK_OP_SHA256 of zk_field_vec_op share: the hash columns of a byte-hash table from message bytes that live on
// the device, one lane per message.
//   digest_i = H(the len_i bytes at d_bytes + off_i);  d_out[i] = sum_k digest_i[k] r_out^(31-k);  d_digest[i] = the 32 digest bytes;
//   d_input_rlc[i] = sum_k m[k] r_in^(len-1-k).
// A hash is a trait H:
//   H::Desc                 its descriptor in include/zkmi355.h (zk_keccak, zk_sha256: two types, one layout -- asserted below)
//   H::name, H::prof        the prefix of its messages, its zk_prof name
//   H::TOTAL_LOG2           total_bytes of 2^TOTAL_LOG2 or more are refused; 64: no bound
// keccak.hip and sha256.hip hold the trait, the two kernels (plain; RLC also walks input_rlc, a separate instantiation so that the
// plain call does not carry its registers) and the entry point as a call of byte_hash_run.  The kernel bodies differ in one call
// (kck_message, sha_message) and are written out in both files all the same: as wrappers of one forced-inline row body templated on
// the trait, k_keccak<true> and k_sha256<true> compiled to other instruction streams (profiles/r29_descriptor_ops.md).
// Launch: one, lane = row, 256 lanes per workgroup.  The 16 + 16 limb records of the two challenges are made on the host per call and
// travel as kernel arguments: wave-uniform, fetched by scalar loads.  No LDS, no scratch, no host synchronisation: the offsets and
// lengths are device data, a row whose message does not lie inside the buffer writes zeros and reads nothing.
#pragma once
#include <cstddef>

#include "ctx.hpp"
#include "keccak64.hip.hpp"
#include "op_check.hpp"

namespace zk {

#define ZK_SAME_MEMBER(m) (offsetof(zk_keccak, m) == offsetof(zk_sha256, m) && sizeof(zk_keccak::m) == sizeof(zk_sha256::m))
static_assert(sizeof(zk_keccak) == sizeof(zk_sha256) && ZK_SAME_MEMBER(d_bytes) && ZK_SAME_MEMBER(total_bytes) && ZK_SAME_MEMBER(d_offsets) && ZK_SAME_MEMBER(d_lens) &&
                  ZK_SAME_MEMBER(d_digest) && ZK_SAME_MEMBER(d_input_rlc) && ZK_SAME_MEMBER(index_width) && ZK_SAME_MEMBER(flags),
              "zk_sha256 is zk_keccak member for member");
#undef ZK_SAME_MEMBER

struct HashArgs {
    const uint8_t* bytes;
    uint64_t total;
    const void* offs;
    const void* lens;
    uint8_t* digest;                    // NULL: not wanted
    Fr* out;
    Fr* in_rlc;                         // the RLC kernels only
    uint64_t n;
    uint32_t index_width;
    KckPow pout;
};

// h_challenges: r_out, then r_in, Montgomery Fr in host memory.  Everything is validated before n is looked at and before the
// launch, so a refused call has written nothing.  plain, rlc: the two kernels of H.
template <class H>
int byte_hash_run(zk_ctx* ctx, const typename H::Desc* desc, const void* h_challenges, Fr* d_out, uint64_t n, void (*plain)(const HashArgs, const KckPow), void (*rlc)(const HashArgs, const KckPow)) {
    const uint32_t iw = desc->index_width;
    if (desc->flags) return ctx->fail(ZK_ERR_INVALID_ARG, "%s: flags 0x%x: must be 0", H::name, desc->flags);
    if (iw != 4 && iw != 8) return ctx->fail(ZK_ERR_INVALID_ARG, "%s: index width %u: must be 4 or 8 bytes", H::name, iw);
    if (!desc->d_offsets || !desc->d_lens) return ctx->fail(ZK_ERR_INVALID_ARG, "%s: NULL offsets or lengths", H::name);
    if ((uintptr_t)desc->d_offsets % iw || (uintptr_t)desc->d_lens % iw) return ctx->fail(ZK_ERR_INVALID_ARG, "%s: offsets or lengths of %u bytes at a misaligned address", H::name, iw);
    if (!desc->d_bytes && desc->total_bytes) return ctx->fail(ZK_ERR_INVALID_ARG, "%s: NULL d_bytes with %llu bytes", H::name, (unsigned long long)desc->total_bytes);
    // the trait's extra check; "& 63" only keeps the shift defined where the compiler sees it with TOTAL_LOG2 = 64, which the first test excludes
    if (H::TOTAL_LOG2 < 64 && desc->total_bytes >> (H::TOTAL_LOG2 & 63)) return ctx->fail(ZK_ERR_INVALID_ARG, "%s: %llu bytes: 2^%d or more", H::name, (unsigned long long)desc->total_bytes, H::TOTAL_LOG2);
    if ((uintptr_t)d_out % 16 || (uintptr_t)desc->d_input_rlc % 16) return ctx->fail(ZK_ERR_INVALID_ARG, "%s: an Fr output at an address that is no multiple of 16", H::name);
    const uint64_t blocks = n / 256 + (n % 256 ? 1 : 0);
    if (blocks > 0x7fffffffull) return ctx->fail(ZK_ERR_INVALID_ARG, "too many rows for one launch");
    // no output overlaps an input or another output
    SpanList<6> spans;
    spans.add(d_out, n * sizeof(Fr), "d_out", true);
    spans.add(desc->d_digest, n * 32, "d_digest", true);
    spans.add(desc->d_input_rlc, n * sizeof(Fr), "d_input_rlc", true);
    spans.add(desc->d_bytes, desc->total_bytes, "d_bytes", false);
    spans.add(desc->d_offsets, n * iw, "d_offsets", false);
    spans.add(desc->d_lens, n * iw, "d_lens", false);
    const char *what, *other;
    if (spans.overlap(&what, &other)) return ctx->fail(ZK_ERR_INVALID_ARG, "%s: %s overlaps %s", H::name, what, other);
    if (!n) return ZK_OK;

    Fr r[2];
    memcpy(r, h_challenges, sizeof r);                  // all 64 bytes, whether r_in is used or not
    HashArgs g;
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

    ZkProfScope prof(ctx, H::prof);
    // the host cannot know the sum of the lengths: total_bytes stands in for the message bytes read
    prof.bytes = n * (2ull * iw + 32 + (g.digest ? 32 : 0) + (g.in_rlc ? 32 : 0)) + desc->total_bytes;
    hipLaunchKernelGGL(g.in_rlc ? rlc : plain, dim3((unsigned)blocks), dim3(256), 0, ctx->stream, g, pin);
    ZK_CHECK_LAUNCH(ctx);
    return ZK_OK;
}

}  // namespace zk

// ZK_OP_POSEIDON of zk_field_vec_op: the width-3 Poseidon hash columns of the reference's PoseidonTable (hash_id, input0, input1)
// from packed typed cells, one lane per message.
//   out[i] = permute(s)[0],  s = (cap_scale cap[i], in0[i], in1[i]) on a head row, the state row i - 1 left + (0, in0[i], in1[i]) on a
//   continue row; an off row writes 0 and ends the message.  The permutation is host::PoseidonWidth3's (csrc/host_hash.hpp), run on
//   29-bit limbs by csrc/poseidon29.hip.hpp (forms, bounds and the table layout are described there).
// Constants: 195 round constants and 9 MDS entries, taken from PoseidonWidth3::get() once per context, converted to 204 nine-limb
// records (7 344 B) and kept in a device table that lives as long as the context.  The kernels READ THE TABLE WAVE-UNIFORMLY: the
// round counter is wave-uniform (every lane of a wave that is still walking is in the same round), the table is a const __restrict__
// kernel argument, so the compiler fetches a round's records with scalar loads into scalar registers, where the multiply-adds take
// them as their scalar operand like the modulus -- no LDS, no vector copies.
// Launches:
//   d_kinds == NULL   k_poseidon_dense: lane = row, every row a head, one launch.
//   otherwise         k_poseidon_heads: one lane per row writes the zeros of the off rows and appends the first row of every message
//                     (a head; a continue row at row 0 or behind an off row, which continues from the zero state) to a list in
//                     context scratch -- a ballot and a prefix per wave, ONE ordinary atomic add per workgroup; order in the list
//                     is free.  Then k_poseidon_walk: lane t owns the message at heads[t] and walks its rows in order with the state
//                     in registers; its grid covers the worst case (n messages), the count is read from device memory, workgroups
//                     beyond it exit: no host synchronisation.  Under ZK_POSEIDON_FINAL the lane stores its last value over its rows
//                     in a second sweep.  A wave takes as long as its longest message (profiles/r24_poseidon.md has that measured).
#include "ctx.hpp"
#include "host_hash.hpp"
#include "op_check.hpp"
#include "poseidon29.hip.hpp"

namespace zk {

struct PsdArgs {
    const uint8_t* in0;
    const uint8_t* in1;
    const uint8_t* cap;                 // NULL: capacity 0
    const uint8_t* kinds;               // NULL for k_poseidon_dense
    Fr* out;
    Fr* word0;                          // NULL: not wanted
    Fr* word1;
    uint64_t n;
    uint32_t width0, width1, cap_width, final_;
    Fr29 k0, k1, kcap;                  // plain constants of psd_in: 2^522 (unsigned cells) or 2^266 (32-byte cells); kcap times cap_scale
};

// one row: inputs in, state entered and permuted, word outputs written; s holds what the row before left and leaves this row's state
__device__ __forceinline__ void psd_row(const PsdArgs& g, const uint32_t* __restrict__ tab, uint64_t i, bool head, Fr29 (&s)[3]) {
    const Fr29 x0 = psd_in<Fr29P>(psd_load(g.in0, g.width0, i), g.k0), x1 = psd_in<Fr29P>(psd_load(g.in1, g.width1, i), g.k1);
    if (head) {
#pragma unroll
        for (int j = 0; j < 9; ++j) s[0].l[j] = s[1].l[j] = s[2].l[j] = 0;
        if (g.cap) s[0] = psd_in<Fr29P>(psd_load(g.cap, g.cap_width, i), g.kcap);
    }
    if (g.word0) stg(g.word0 + i, psd_out<Fr29P>(x0));
    if (g.word1) stg(g.word1 + i, psd_out<Fr29P>(x1));
    psd_enter<Fr29P>(s, x0, x1, tab);
    psd_rounds<Fr29P>(s, tab);
}

__global__ void __launch_bounds__(256) k_poseidon_dense(const PsdArgs g, const uint32_t* __restrict__ tab) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= g.n) return;
    Fr29 s[3];
    psd_row(g, tab, i, true, s);
    stg(g.out + i, psd_out<Fr29P>(s[0]));
}

// heads[0 .. *count): the first rows of the messages, in any order; off rows get their zeros here
__global__ void __launch_bounds__(256) k_poseidon_heads(const PsdArgs g, uint32_t* __restrict__ heads, uint32_t* __restrict__ count) {
    __shared__ uint32_t wave_total[4];
    __shared__ uint32_t base;
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    bool start = false;
    if (i < g.n) {
        const uint32_t kind = g.kinds[i] & 3u;
        if (kind >= 2) {
            stg(g.out + i, Fr::zero());
            if (g.word0) stg(g.word0 + i, Fr::zero());
            if (g.word1) stg(g.word1 + i, Fr::zero());
        } else {
            start = kind == 0 || i == 0 || (g.kinds[i - 1] & 3u) >= 2;
        }
    }
    const uint64_t mask = __ballot(start);
    if (lane == 0) wave_total[wave] = (uint32_t)__popcll(mask);
    __syncthreads();
    if (threadIdx.x == 0) {
        const uint32_t total = wave_total[0] + wave_total[1] + wave_total[2] + wave_total[3];
        base = total ? atomicAdd(count, total) : 0u;
    }
    __syncthreads();
    if (!start) return;
    uint32_t at = base + (uint32_t)__popcll(mask & ((1ull << lane) - 1));
    for (uint32_t w = 0; w < wave; ++w) at += wave_total[w];
    heads[at] = (uint32_t)i;            // at < the number of messages <= n: the list holds n entries
}

__global__ void __launch_bounds__(256) k_poseidon_walk(const PsdArgs g, const uint32_t* __restrict__ tab, const uint32_t* __restrict__ heads, const uint32_t* __restrict__ count) {
    const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= *count) return;
    const uint64_t first = heads[t];
    Fr29 s[3];
#pragma unroll
    for (int j = 0; j < 9; ++j) s[0].l[j] = s[1].l[j] = s[2].l[j] = 0;
    uint64_t i = first;
    bool head = (g.kinds[i] & 3u) == 0;
    for (;;) {
        psd_row(g, tab, i, head, s);
        if (!g.final_) stg(g.out + i, psd_out<Fr29P>(s[0]));
        ++i;
        if (i >= g.n || (g.kinds[i] & 3u) != 1) break;       // a head starts another lane's message, an off row ends this one
        head = false;
    }
    if (g.final_) {
        const Fr v = psd_out<Fr29P>(s[0]);
        for (uint64_t r = first; r < i; ++r) stg(g.out + r, v);
    }
}

// the 204 records of poseidon29.hip.hpp from the host's generator, uploaded once per context
static int poseidon_table(zk_ctx* ctx, const uint32_t** out) {
    if (!ctx->poseidon_tab) {
        const host::PoseidonWidth3& spec = host::PoseidonWidth3::get();
        const Fr c261 = fr_pow2(261), c522 = fr_pow2(522);
        std::vector<uint32_t> h((size_t)PSD_TAB_WORDS);
        auto put = [&](int rec, const host::F4& mont, const Fr& by) {    // plain canonical limbs of (value of mont) * by
            Fr v;
            memcpy(&v, &mont, sizeof v);
            const Fr29 l = unpack29<Fr29P>(v * by);
            for (int i = 0; i < 9; ++i) h[(size_t)9 * rec + i] = l.l[i];
        };
        for (int r = 0; r < PSD_ROUNDS; ++r)
            for (int i = 0; i < 3; ++i) put(3 * r + i, spec.constants[(size_t)3 * r + i], r ? c522 : c261);
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) put(PSD_MDS_AT + 3 * i + j, spec.mds[i][j], c261);
        void* d = nullptr;
        ZK_HIP(ctx, hipMalloc(&d, sizeof(uint32_t) * PSD_TAB_WORDS));
        hipError_t e = hipMemcpyAsync(d, h.data(), sizeof(uint32_t) * PSD_TAB_WORDS, hipMemcpyHostToDevice, ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);     // h leaves scope; once per context
        if (e != hipSuccess) { (void)hipFree(d); return ctx->fail(ZK_ERR_HIP, "Poseidon table upload failed: %s", hipGetErrorString(e)); }
        ctx->poseidon_tab = d;
    }
    *out = (const uint32_t*)ctx->poseidon_tab;
    return ZK_OK;
}

// h_scale: one Montgomery Fr in host memory.  Everything is validated before n is looked at and before the first launch, so a
// refused call has written nothing.
int fr_poseidon_run(zk_ctx* ctx, const zk_poseidon* desc, const void* h_scale, Fr* d_out, uint64_t n) {
    auto bytes = [](uint32_t w, uint64_t rows) -> uint64_t { return !rows ? 0 : w == 31 ? 62 * (rows - 1) + 31 : (uint64_t)w * rows; };
    if (desc->flags & ~(uint32_t)ZK_POSEIDON_FINAL) return ctx->fail(ZK_ERR_INVALID_ARG, "Poseidon: unknown flag bits 0x%x", desc->flags);
    const void* in[2] = {desc->d_in0, desc->d_in1};
    const uint32_t width[2] = {desc->width0, desc->width1};
    for (int c = 0; c < 2; ++c) {
        if (!typed_cell_width_ok(width[c], true) && width[c] != 31) return ctx->fail(ZK_ERR_INVALID_ARG, "Poseidon: input %d: cell width %u: must be 1, 2, 4, 8, 16, 31 or 32 bytes", c, width[c]);
        if (!in[c]) return ctx->fail(ZK_ERR_INVALID_ARG, "Poseidon: input %d: NULL pointer", c);
        if (width[c] != 31 && (uintptr_t)in[c] % typed_cell_align(width[c])) return ctx->fail(ZK_ERR_INVALID_ARG, "Poseidon: input %d: cells of %u bytes at a misaligned address", c, width[c]);
    }
    const uint32_t cap_width = desc->d_cap ? desc->cap_width : 0;
    if (desc->d_cap) {
        if (!typed_cell_width_ok(cap_width, true)) return ctx->fail(ZK_ERR_INVALID_ARG, "Poseidon: capacity cell width %u: must be 1, 2, 4, 8, 16 or 32 bytes", cap_width);
        if ((uintptr_t)desc->d_cap % typed_cell_align(cap_width)) return ctx->fail(ZK_ERR_INVALID_ARG, "Poseidon: capacity cells of %u bytes at a misaligned address", cap_width);
    }
    // no output overlaps an input or another output
    SpanList<7> spans;
    spans.add(d_out, n * sizeof(Fr), "d_out", true);
    spans.add(desc->d_word0, n * sizeof(Fr), "d_word0", true);
    spans.add(desc->d_word1, n * sizeof(Fr), "d_word1", true);
    spans.add(desc->d_in0, bytes(width[0], n), "d_in0", false);
    spans.add(desc->d_in1, bytes(width[1], n), "d_in1", false);
    spans.add(desc->d_cap, bytes(cap_width, n), "d_cap", false);
    spans.add(desc->d_kinds, n, "d_kinds", false);
    const char *what, *other;
    if (spans.overlap(&what, &other)) return ctx->fail(ZK_ERR_INVALID_ARG, "Poseidon: %s overlaps %s", what, other);
    if (!n) return ZK_OK;
    const uint64_t blocks = (n + 255) / 256;
    if ((desc->d_kinds && n > 0xffffffffull) || blocks > 0x7fffffffull) return ctx->fail(ZK_ERR_INVALID_ARG, "too many rows for one launch");   // the list holds 32-bit row numbers
    const uint32_t* tab = nullptr;
    if (int e = poseidon_table(ctx, &tab)) return e;

    static const Fr c522 = fr_pow2(522), c266 = fr_pow2(266);           // the integers 2^522, 2^266 mod r
    PsdArgs g;
    memset(&g, 0, sizeof g);
    g.in0 = (const uint8_t*)desc->d_in0;
    g.in1 = (const uint8_t*)desc->d_in1;
    g.cap = (const uint8_t*)desc->d_cap;
    g.kinds = desc->d_kinds;
    g.out = d_out;
    g.word0 = (Fr*)desc->d_word0;
    g.word1 = (Fr*)desc->d_word1;
    g.n = n;
    g.width0 = width[0];
    g.width1 = width[1];
    g.cap_width = cap_width;
    g.final_ = desc->flags & ZK_POSEIDON_FINAL;
    g.k0 = unpack29<Fr29P>(width[0] == 32 ? c266 : c522);
    g.k1 = unpack29<Fr29P>(width[1] == 32 ? c266 : c522);
    Fr scale;
    memcpy(&scale, h_scale, sizeof scale);
    g.kcap = unpack29<Fr29P>(scale * (cap_width == 32 ? c266 : c522));  // (value of cap_scale) 2^522 or 2^266, canonical: a Montgomery product by a plain integer

    uint32_t* count = nullptr;
    uint32_t* heads = nullptr;
    if (g.kinds) {                      // SC_TMP: the count, then the list; every user of the slot is enqueued on ctx->stream
        char* sc = (char*)ctx->get_scratch(SC_TMP, 256 + sizeof(uint32_t) * n);
        if (!sc) return ZK_ERR_OOM;
        count = (uint32_t*)sc;
        heads = (uint32_t*)(sc + 256);
    }
    ZkProfScope prof(ctx, "fr_poseidon");
    const uint64_t per_row = (width[0] == 31 ? 31 : width[0]) + (width[1] == 31 ? 31 : width[1]) + cap_width + (g.kinds ? 1 : 0);
    prof.bytes = n * (per_row + 32 + (g.word0 ? 32 : 0) + (g.word1 ? 32 : 0));
    if (!g.kinds) {
        hipLaunchKernelGGL(k_poseidon_dense, dim3((unsigned)blocks), dim3(256), 0, ctx->stream, g, tab);
    } else {
        ZK_HIP(ctx, hipMemsetAsync(count, 0, sizeof(uint32_t), ctx->stream));
        hipLaunchKernelGGL(k_poseidon_heads, dim3((unsigned)blocks), dim3(256), 0, ctx->stream, g, heads, count);
        hipLaunchKernelGGL(k_poseidon_walk, dim3((unsigned)blocks), dim3(256), 0, ctx->stream, g, tab, (const uint32_t*)heads, (const uint32_t*)count);
    }
    ZK_CHECK_LAUNCH(ctx);
    return ZK_OK;
}

}  // namespace zk

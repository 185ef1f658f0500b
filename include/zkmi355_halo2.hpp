// C++ host-side mirror of the halo2_proofs items on the hot path, over the C ABI (zkmi355.h).
//
// The reference is a Rust workspace and Rust is not available in this build image, so this header
// is the compiled-language counterpart of the shim crate described in INTEGRATION.md: same names,
// argument meaning and error behaviour as the halo2 items it mirrors, so call sites translate
// one-to-one.  Header-only; link with -lzkmi355.
//
//   halo2_proofs::arithmetic::best_fft            -> zk::halo2::best_fft
//   halo2_proofs::arithmetic::best_multiexp       -> zk::halo2::best_multiexp
//   halo2_proofs::arithmetic::eval_polynomial     -> zk::halo2::eval_polynomial
//   halo2_proofs::arithmetic::kate_division       -> zk::halo2::kate_division
//   halo2_proofs::poly::EvaluationDomain          -> zk::halo2::EvaluationDomain
//   halo2_proofs::poly::kzg::commitment::ParamsKZG-> zk::halo2::ParamsKZG
//   halo2_proofs::plonk::{keygen_pk, create_proof}-> zk::halo2::{ProvingKey, create_proof}
//   halo2_proofs::dev::MockProver::{run, verify_par, verify_at_rows_par} -> zk::halo2::mock_verify
//   halo2_proofs::plonk::{VerifyingKey, verify_proof} (KZG; SingleStrategy / AccumulatorStrategy)
//                                                 -> zk::halo2::{VerifyingKey, verify_proof}
//   (reference call sites: circuit-benchmarks/src/super_circuit.rs:104-132, zkevm-circuits/src/test_util.rs:272,
//    prover/src/common/prover/utils.rs:31,55, prover/src/utils.rs:77)
#pragma once
#include <algorithm>
#include <array>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

#include "zkmi355.h"

namespace zk {
namespace halo2 {

using Fr = std::array<uint64_t, 4>;        // Montgomery limbs, as halo2curves holds them
using G1Affine = std::array<uint64_t, 8>;  // {x, y}; identity = zeros

// halo2's plonk::Error / io errors surface as one exception type carrying the library message
struct Error : std::runtime_error {
    int status;
    Error(int st, const std::string& msg) : std::runtime_error(msg), status(st) {}
};

class Context {
   public:
    explicit Context(int device = 0) {
        int rc = zk_ctx_create(device, &ctx_);
        if (rc) throw Error(rc, rc == ZK_ERR_NO_DEVICE ? "no gfx950 device (there is no CPU fallback)" : "zk_ctx_create failed");
    }
    ~Context() { zk_ctx_destroy(ctx_); }
    Context(const Context&) = delete;
    Context& operator=(const Context&) = delete;
    zk_ctx* raw() const { return ctx_; }
    void check(int rc) const { if (rc) throw Error(rc, zk_last_error(ctx_)); }

    // RAII device column
    class Buffer {
       public:
        Buffer(const Context& c, size_t bytes) : c_(c), bytes_(bytes) { c_.check(zk_buf_alloc(c_.raw(), bytes, &p_)); }
        ~Buffer() { zk_buf_free(c_.raw(), p_); }
        Buffer(const Buffer&) = delete;
        Buffer& operator=(const Buffer&) = delete;
        void* ptr() const { return p_; }
        size_t bytes() const { return bytes_; }
        void upload(const void* h, size_t n) { c_.check(zk_h2d(c_.raw(), p_, h, n)); }
        void download(void* h, size_t n) const { c_.check(zk_d2h(c_.raw(), h, p_, n)); }
       private:
        const Context& c_;
        void* p_ = nullptr;
        size_t bytes_;
    };

   private:
    zk_ctx* ctx_ = nullptr;
};

// arithmetic::best_fft(a, omega, log_n): in place, natural order in and out
inline void best_fft(const Context& c, std::vector<Fr>& a, const Fr& omega, uint32_t log_n) {
    if (a.size() != (size_t(1) << log_n)) throw Error(ZK_ERR_INVALID_ARG, "best_fft: a.len() != 1 << log_n");
    Context::Buffer d(c, a.size() * sizeof(Fr));
    d.upload(a.data(), a.size() * sizeof(Fr));
    c.check(zk_ntt_omega(c.raw(), d.ptr(), log_n, omega.data()));
    d.download(a.data(), a.size() * sizeof(Fr));
}

// arithmetic::best_multiexp(coeffs, bases)
inline G1Affine best_multiexp(const Context& c, const std::vector<Fr>& coeffs, const std::vector<G1Affine>& bases) {
    if (coeffs.size() != bases.size()) throw Error(ZK_ERR_INVALID_ARG, "best_multiexp: coeffs.len() != bases.len()");
    G1Affine out{};
    c.check(zk_msm_g1_host(c.raw(), coeffs.data(), bases.data(), coeffs.size(), out.data()));
    return out;
}

// arithmetic::eval_polynomial(poly, point)
inline Fr eval_polynomial(const Context& c, const std::vector<Fr>& poly, const Fr& point) {
    Context::Buffer d(c, poly.size() * sizeof(Fr) + 32);
    d.upload(poly.data(), poly.size() * sizeof(Fr));
    Fr out{};
    c.check(zk_poly_eval(c.raw(), d.ptr(), poly.size(), point.data(), out.data()));
    return out;
}

// arithmetic::kate_division(a, b): quotient of (a(X) - a(b)) / (X - b)
inline std::vector<Fr> kate_division(const Context& c, const std::vector<Fr>& a, const Fr& b) {
    if (a.size() < 2) return {};
    Context::Buffer d(c, a.size() * sizeof(Fr)), q(c, (a.size() - 1) * sizeof(Fr));
    d.upload(a.data(), a.size() * sizeof(Fr));
    c.check(zk_kate_division(c.raw(), d.ptr(), a.size(), b.data(), q.ptr()));
    std::vector<Fr> out(a.size() - 1);
    q.download(out.data(), out.size() * sizeof(Fr));
    return out;
}

// d_out[i] = Fr::from(d_packed[i]) for n little-endian unsigned cells of cell_bytes = 1, 2, 4, 8 or 16 bytes each, device to device
// (zk_fr_from_uint; asynchronous on the context's stream).  With ProofSession::advice_phase_dev: a witness whose cells another
// kernel left on the device as integers.
inline void fr_from_uint(const Context& c, const void* d_packed, uint32_t cell_bytes, size_t n, void* d_out) {
    c.check(zk_fr_from_uint(c.raw(), d_packed, cell_bytes, n, d_out));
}
// the same for several columns of n cells each, sixteen per launch (zk_fr_from_uint_batch): cell_bytes[j] per column, one call may
// mix widths; outputs overlap neither each other nor any input
inline void fr_from_uint_batch(const Context& c, const std::vector<const void*>& d_packed, const std::vector<uint8_t>& cell_bytes, size_t n, const std::vector<void*>& d_out) {
    if (cell_bytes.size() != d_packed.size() || d_out.size() != d_packed.size()) throw Error(ZK_ERR_INVALID_ARG, "fr_from_uint_batch: one cell width and one output per column");
    c.check(zk_fr_from_uint_batch(c.raw(), d_packed.data(), cell_bytes.data(), d_packed.size(), n, d_out.data()));
}
// out[0] = b[0], out[i] = a[i] * out[i - 1] + b[i] over n Montgomery Fr, device to device (zk_field_vec_op with ZK_OP_SCAN_AFFINE;
// asynchronous on the context's stream); reverse: out[n - 1] = b[n - 1], out[i] = a[i] * out[i + 1] + b[i].  a[i] = 0 starts a new
// segment: the running RLC with resets of a challenge-phase column is a = r * (1 - is_first), b = x.  out overlaps neither input.
inline void scan_affine(const Context& c, const Context::Buffer& a, const Context::Buffer& b, Context::Buffer& out, size_t n, bool reverse = false) {
    if (n * sizeof(Fr) > a.bytes() || n * sizeof(Fr) > b.bytes() || n * sizeof(Fr) > out.bytes()) throw Error(ZK_ERR_INVALID_ARG, "scan_affine: a buffer holds fewer than n elements");
    c.check(zk_field_vec_op(c.raw(), ZK_FIELD_FR, reverse ? ZK_OP_SCAN_AFFINE_REV : ZK_OP_SCAN_AFFINE, a.ptr(), b.ptr(), out.ptr(), n));
}
// d_out[i] = constant + sum_j weights[j] * cell_j[i] for i < n, across typed columns on the device (zk_field_vec_op with
// ZK_OP_ROW_RLC and a zk_row_rlc table; asynchronous on the context's stream, 64 columns per launch): d_cols[j] holds n cells of
// cell_bytes[j] bytes -- 1, 2, 4, 8, 16: packed little-endian unsigned integers as for fr_from_uint; 32: Montgomery Fr.  rlc::value
// over the 32 byte columns of a word is weights[j] = r^j; an RwRow under a leading one is constant = r^11 with descending powers (or
// constant = 1 with weights[j] = r^(j + 1), the order RwRow::rlc folds in).  d_out (n x 32 B) may
// be one of the 32-byte columns itself and overlaps no other column.
inline void row_rlc(const Context& c, const std::vector<const void*>& d_cols, const std::vector<uint8_t>& cell_bytes, const std::vector<Fr>& weights, size_t n, void* d_out,
                    const Fr& constant = Fr{}) {
    if (cell_bytes.size() != d_cols.size() || weights.size() != d_cols.size()) throw Error(ZK_ERR_INVALID_ARG, "row_rlc: one cell width and one weight per column");
    std::vector<Fr> host(1, constant);                                  // the constant, then the weights: host memory, read by the call
    host.insert(host.end(), weights.begin(), weights.end());
    const zk_row_rlc table{(uint32_t)d_cols.size(), d_cols.data(), cell_bytes.data()};
    c.check(zk_field_vec_op(c.raw(), ZK_FIELD_FR, ZK_OP_ROW_RLC, &table, host.data(), d_out, n));
}
// d_out[i] = m[kind_i] * d_out[i - 1] + w[kind_i] * cell[i] for i < n with d_out[-1] = z0, along one typed column on the device
// (zk_field_vec_op with ZK_OP_SCAN_RLC and a zk_scan_rlc; asynchronous on the context's stream); reverse: from the last row down,
// d_out[i] = m[kind_i] * d_out[i + 1] + w[kind_i] * cell[i] with d_out[n] = z0 (ZK_OP_SCAN_RLC_REV).  d_cells holds n cells of
// cell_bytes bytes (1, 2, 4, 8, 16: packed little-endian unsigned integers as for fr_from_uint; 32: Montgomery Fr), d_kinds n bytes
// whose low two bits are the row's kind, or nullptr for kind 0 everywhere.  table = {m_0, w_0, m_1, w_1, m_2, w_2, m_3, w_3}: the
// running RLC with restarts and padding rows is step (r, 1), start (0, 1), hold (1, 0), clear (0, 0).  d_out (n x 32 B) overlaps
// neither the cells nor the kinds.
inline void scan_rlc(const Context& c, const void* d_cells, uint32_t cell_bytes, const uint8_t* d_kinds, const std::array<Fr, 8>& table, size_t n, void* d_out,
                     const Fr& z0 = Fr{}, bool reverse = false) {
    std::array<Fr, 9> host;                                             // z0, then the table: host memory, read by the call
    host[0] = z0;
    std::copy(table.begin(), table.end(), host.begin() + 1);
    const zk_scan_rlc desc{d_cells, cell_bytes, d_kinds};
    c.check(zk_field_vec_op(c.raw(), ZK_FIELD_FR, reverse ? ZK_OP_SCAN_RLC_REV : ZK_OP_SCAN_RLC, &desc, host.data(), d_out, n));
}
// d_out[i] = num[i] * inv0(constant + sum_j weights[j] * cell_j[i]) for i < n, inv0(0) = 0, across typed columns on the device
// (zk_field_vec_op with ZK_OP_ROW_INV0 and a zk_row_inv0; asynchronous on the context's stream) -- halo2's
// Assigned::Rational(num, den).evaluate() with a denominator that is linear in typed cells, the batch_invert_assigned of such a
// column.  d_cols, cell_bytes, weights and constant as for row_rlc: IsZeroChip's value_inv is one column with weight one, IsEqual's
// inverse of a difference the weights (1, -1), the inverse of a cell minus a constant k is constant = -k.  d_num: nullptr (every
// numerator is one) or n cells of num_bytes bytes (1, 2, 4, 8, 16 packed; 32: Montgomery Fr).  d_out (n x 32 B) may be one of the
// 32-byte columns or the 32-byte numerator itself and overlaps no other column.
inline void row_inv0(const Context& c, const std::vector<const void*>& d_cols, const std::vector<uint8_t>& cell_bytes, const std::vector<Fr>& weights, size_t n, void* d_out,
                     const Fr& constant = Fr{}, const void* d_num = nullptr, uint32_t num_bytes = 32) {
    if (cell_bytes.size() != d_cols.size() || weights.size() != d_cols.size()) throw Error(ZK_ERR_INVALID_ARG, "row_inv0: one cell width and one weight per column");
    std::vector<Fr> host(1, constant);                                  // the constant, then the weights: host memory, read by the call
    host.insert(host.end(), weights.begin(), weights.end());
    const zk_row_inv0 desc{(uint32_t)d_cols.size(), d_cols.data(), cell_bytes.data(), d_num, num_bytes};
    c.check(zk_field_vec_op(c.raw(), ZK_FIELD_FR, ZK_OP_ROW_INV0, &desc, host.data(), d_out, n));
}
// d_out[i] = permute(s)[0] for i < n: the width-3 Poseidon hash columns of the PoseidonTable from typed cells on the device
// (zk_field_vec_op with ZK_OP_POSEIDON and a zk_poseidon; asynchronous on the context's stream) -- Fr::hash_with_domain([a, b], domain)
// per row (d_kinds = nullptr, d_cap = the domain column, cap_scale = one) and the Poseidon code hash (cells of 31 bytes: cell i is the
// 31 big-endian bytes at ptr + 62 i, d_in1 = d_in0 + 31; d_cap = the byte lengths, cap_scale = 2^64; d_kinds: 0 head, 1 continue, 2 off;
// final_hash: every row of a message holds the hash of its last row, the table's hash_id).  d_word0 / d_word1: optional n x 32 B
// outputs, the Montgomery images of the inputs (input0, input1).  No output overlaps an input or another output.
inline void poseidon(const Context& c, const void* d_in0, uint8_t bytes0, const void* d_in1, uint8_t bytes1, size_t n, void* d_out, const void* d_cap = nullptr, uint8_t cap_bytes = 8,
                     const Fr* cap_scale = nullptr, const uint8_t* d_kinds = nullptr, bool final_hash = false, void* d_word0 = nullptr, void* d_word1 = nullptr) {
    const Fr one{{0xac96341c4ffffffbULL, 0x36fc76959f60cd29ULL, 0x666ea36f7879462eULL, 0x0e0a77c19a07df2fULL}};           // 2^256 mod r: Montgomery one
    const Fr scale = cap_scale ? *cap_scale : one;                      // host memory, read by the call
    const zk_poseidon desc{d_in0, d_in1, d_cap, d_kinds, d_word0, d_word1, bytes0, bytes1, (uint8_t)(d_cap ? cap_bytes : 0), (uint8_t)(final_hash ? ZK_POSEIDON_FINAL : 0)};
    c.check(zk_field_vec_op(c.raw(), ZK_FIELD_FR, ZK_OP_POSEIDON, &desc, &scale, d_out, n));
}
// d_out[i] = sum_k digest_i[k] r_out^(31-k) for i < n, digest_i = Keccak-256 of the len_i bytes at d_bytes + off_i: the hash columns
// of the KeccakTable from message bytes on the device (zk_field_vec_op with ZK_OP_KECCAK and a zk_keccak; asynchronous on the
// context's stream) -- output_rlc = rlc::value(Word::from_big_endian(digest).to_le_bytes(), evm_word) in d_out, and optionally the
// digest bytes (d_digest, n x 32 B) and input_rlc = rlc::value(input.iter().rev(), keccak_input) (d_input_rlc, n x 32 B, under r_in).
// d_offsets, d_lens: n unsigned integers of index_bytes (4 or 8) each; d_lens is the input_len column as it stands.  A message that
// does not lie inside the total_bytes at d_bytes writes zeros and reads nothing.  No output overlaps an input or another output.
inline void keccak(const Context& c, const void* d_bytes, uint64_t total_bytes, const void* d_offsets, const void* d_lens, uint8_t index_bytes, size_t n, void* d_out, const Fr& r_out,
                   const Fr& r_in = Fr{}, void* d_digest = nullptr, void* d_input_rlc = nullptr) {
    const Fr host[2] = {r_out, r_in};                                   // host memory, read by the call
    const zk_keccak desc{d_bytes, total_bytes, d_offsets, d_lens, d_digest, d_input_rlc, index_bytes, 0};
    c.check(zk_field_vec_op(c.raw(), ZK_FIELD_FR, ZK_OP_KECCAK, &desc, host, d_out, n));
}
// The same for the SHA256Table: digest_i = SHA-256 (FIPS 180-4) of the len_i bytes at d_bytes + off_i, d_out[i] = output_rlc =
// rlc::value(Word::from_big_endian(output).to_le_bytes(), challenge), optionally the digest bytes and input_rlc (zk_field_vec_op with
// ZK_OP_SHA256 and a zk_sha256; asynchronous on the context's stream).  The reference takes BOTH RLCs of this table under
// keccak_input: r_in = nullptr means r_in = r_out.  total_bytes stays below 2^61; every other rule is keccak()'s.
inline void sha256(const Context& c, const void* d_bytes, uint64_t total_bytes, const void* d_offsets, const void* d_lens, uint8_t index_bytes, size_t n, void* d_out, const Fr& r_out,
                   const Fr* r_in = nullptr, void* d_digest = nullptr, void* d_input_rlc = nullptr) {
    const Fr host[2] = {r_out, r_in ? *r_in : r_out};                   // host memory, read by the call
    const zk_sha256 desc{d_bytes, total_bytes, d_offsets, d_lens, d_digest, d_input_rlc, index_bytes, 0};
    c.check(zk_field_vec_op(c.raw(), ZK_FIELD_FR, ZK_OP_SHA256, &desc, host, d_out, n));
}
// The state circuit's row order: d_perm_out[i] = the uint32 index of the record at place i when the n 64-byte key records at d_keys
// (what rw_to_be_limbs packs of an RW row) are sorted as big-endian integers, stably (zk_field_vec_op with ZK_OP_KEY_SORT and a
// zk_key_sort; asynchronous on the context's stream).  mask: nullptr (all 64 bytes take part) or 64 host bytes, key byte j takes part
// iff mask[j] != 0 -- without bytes 60..63 this is sort_by_cached_key(Rw::as_key) over rows in rw_counter order.  d_sorted: optional
// n x 64 B, the records in that order.
inline void key_sort(const Context& c, const void* d_keys, size_t n, void* d_perm_out, const uint8_t* mask = nullptr, void* d_sorted = nullptr) {
    const zk_key_sort desc{d_keys, d_sorted, 0};
    c.check(zk_field_vec_op(c.raw(), ZK_FIELD_FR, ZK_OP_KEY_SORT, &desc, mask, d_perm_out, n));
}
// The ordering witness of adjacent rows, row i = record d_perm[i] (nullptr: record i): d_inv_out = limb_difference_inverse, and
// optionally limb_difference, first_different_limb as bytes and as the BinaryNumberChip's five bit planes, not_first_access
// (first_different_limb >= group_limbs) and `count` gathered typed columns -- cell i of column j is the big-endian integer of key
// bytes [cols[j].offset, cols[j].offset + cols[j].width) of row i's record (zk_field_vec_op with ZK_OP_KEY_ORDER and a zk_key_order).
// cols and d_cols are host arrays.  No output overlaps an input or another output.
inline void key_order(const Context& c, const void* d_keys, size_t n, void* d_inv_out, const void* d_perm = nullptr, void* d_diff = nullptr, void* d_index = nullptr,
                      void* d_bits = nullptr, void* d_not_first = nullptr, uint32_t group_limbs = 30, uint32_t count = 0, const zk_key_col* cols = nullptr,
                      void* const* d_cols = nullptr) {
    const zk_key_order desc{d_keys, d_perm, d_diff, d_index, d_bits, d_not_first, group_limbs, count, cols, d_cols, 0};
    c.check(zk_field_vec_op(c.raw(), ZK_FIELD_FR, ZK_OP_KEY_ORDER, &desc, nullptr, d_inv_out, n));
}
// The rows of the bytecode circuit from code bytes on the device (zk_field_vec_op with ZK_OP_BYTECODE_ROWS; asynchronous on the
// context's stream).  desc: a zk_bytecode_rows -- the bytes, offsets and lengths as for keccak(), the code hashes, and the outputs
// wanted (tag, index, value, is_code, push_data_left, push_data_size, length, the kind columns of push_acc and push_rlc), each a
// device pointer or nullptr.  d_hash_out[i] (n x 32 B) = the code hash of the bytecode of row i, empty_hash on the padding rows.
inline void bytecode_rows(const Context& c, const zk_bytecode_rows& desc, const Fr& empty_hash, size_t n, void* d_hash_out) {
    c.check(zk_field_vec_op(c.raw(), ZK_FIELD_FR, ZK_OP_BYTECODE_ROWS, &desc, &empty_hash, d_hash_out, n));
}
// The integer columns of the copy circuit and the copy table from copy events on the device (zk_field_vec_op with ZK_OP_COPY_ROWS;
// asynchronous on the context's stream).  desc: a zk_copy_rows -- the zk_copy_event records, the byte heap, and the typed outputs
// wanted, each a device pointer or nullptr.  d_addr (n x 8 B) receives the addr column.
inline void copy_rows(const Context& c, const zk_copy_rows& desc, size_t n, void* d_addr) {
    c.check(zk_field_vec_op(c.raw(), ZK_FIELD_FR, ZK_OP_COPY_ROWS, &desc, nullptr, d_addr, n));
}
// The challenge-phase columns of the same rows (ZK_OP_COPY_RLC).  desc: a zk_copy_rlc -- events and heap as above, the ids, and
// id, id_other, rlc_acc, word_rlc, word_rlc_prev, each n x 32 B or nullptr.  d_value_acc (n x 32 B) receives value_acc.
inline void copy_rlc(const Context& c, const zk_copy_rlc& desc, const Fr& r_word, const Fr& r_in, size_t n, void* d_value_acc) {
    const Fr challenges[2] = {r_word, r_in};
    c.check(zk_field_vec_op(c.raw(), ZK_FIELD_FR, ZK_OP_COPY_RLC, &desc, challenges, d_value_acc, n));
}
// The rows of the exponentiation circuit and the exponentiation table from (base, exponent) events on the device (zk_field_vec_op
// with ZK_OP_EXP_ROWS; asynchronous on the context's stream).  desc: a zk_exp_rows -- the zk_exp_event records and the typed outputs
// wanted, each a device pointer or nullptr; d_rows_needed receives 8 x the steps of all events + 10 for the caller to compare with n.
// d_exponentiation_lo_hi (n x 16 B) receives that column.
inline void exp_rows(const Context& c, const zk_exp_rows& desc, size_t n, void* d_exponentiation_lo_hi) {
    c.check(zk_field_vec_op(c.raw(), ZK_FIELD_FR, ZK_OP_EXP_ROWS, &desc, nullptr, d_exponentiation_lo_hi, n));
}
// The eight columns the Poseidon-hash extension adds to the rows of the bytecode circuit (zk_field_vec_op with ZK_OP_CODE_HASH_ROWS;
// asynchronous on the context's stream).  desc: a zk_code_hash_rows -- the bytes, offsets and lengths as for bytecode_rows(), and the
// typed outputs wanted, each a device pointer or nullptr.  d_field_input (n x 32 B) receives field_input.
inline void code_hash_rows(const Context& c, const zk_code_hash_rows& desc, size_t n, void* d_field_input) {
    c.check(zk_field_vec_op(c.raw(), ZK_FIELD_FR, ZK_OP_CODE_HASH_ROWS, &desc, nullptr, d_field_input, n));
}
// The code-hash rows of the Poseidon table from the same bytes (ZK_OP_CODE_HASH_TABLE).  desc: a zk_code_hash_table -- input1, control,
// heading_mark, the kinds and the capacity column of ZK_OP_POSEIDON, each a device pointer or nullptr; d_rows_needed receives the rows
// of all bytecodes for the caller to compare with n.  d_input0 (n x 32 B) receives input0.
inline void code_hash_table(const Context& c, const zk_code_hash_table& desc, size_t n, void* d_input0) {
    c.check(zk_field_vec_op(c.raw(), ZK_FIELD_FR, ZK_OP_CODE_HASH_TABLE, &desc, nullptr, d_input0, n));
}

// poly::EvaluationDomain::new(j, k)
class EvaluationDomain {
   public:
    EvaluationDomain(const Context& c, uint32_t j, uint32_t k) : c_(c), k_(k) {
        extended_k_ = k;
        while ((size_t(1) << extended_k_) < (size_t(1) << k) * (j - 1)) ++extended_k_;
    }
    uint32_t k() const { return k_; }
    uint32_t extended_k() const { return extended_k_; }
    void lagrange_to_coeff(Context::Buffer& a) const { c_.check(zk_ntt(c_.raw(), a.ptr(), k_, 1)); }
    void coeff_to_lagrange(Context::Buffer& a) const { c_.check(zk_ntt(c_.raw(), a.ptr(), k_, 0)); }
    void coeff_to_extended(const Context::Buffer& coeffs, Context::Buffer& out) const { c_.check(zk_coeff_to_extended(c_.raw(), coeffs.ptr(), k_, extended_k_, out.ptr())); }
    void extended_to_coeff(Context::Buffer& a) const { c_.check(zk_extended_to_coeff(c_.raw(), a.ptr(), extended_k_)); }
   private:
    const Context& c_;
    uint32_t k_, extended_k_;
};

// poly::kzg::commitment::ParamsKZG<Bn256>
class ParamsKZG {
   public:
    // ParamsKZG::unsafe_setup_with_s(k, s)
    static ParamsKZG unsafe_setup_with_s(const Context& c, uint32_t k, const Fr& s) {
        zk_srs* p = nullptr;
        c.check(zk_srs_setup_with_s(c.raw(), k, s.data(), &p));
        ParamsKZG out(c, p);
        out.g2_.resize(128);
        out.s_g2_.resize(128);
        c.check(zk_g2_setup(s.data(), out.g2_.data(), out.s_g2_.data()));
        return out;
    }
    // after ParamsKZG::read_custom on the host: g and g_lagrange in RawBytes layout
    static ParamsKZG from_points(const Context& c, uint32_t k, const std::vector<G1Affine>& g, const std::vector<G1Affine>& g_lagrange) {
        zk_srs* p = nullptr;
        c.check(zk_srs_create(c.raw(), k, g.data(), g_lagrange.empty() ? nullptr : g_lagrange.data(), &p));
        return ParamsKZG(c, p);
    }
    // ParamsKZG::read_custom(reader, format): `file` is the whole params{k} file; the G2 encodings are
    // kept as they came (the verifier side needs them, the prover does not)
    enum class SerdeFormat : int { Processed = ZK_SERDE_PROCESSED, RawBytes = ZK_SERDE_RAW, RawBytesUnchecked = ZK_SERDE_RAW_UNCHECKED };
    static ParamsKZG read_custom(const Context& c, const std::vector<uint8_t>& file, SerdeFormat format = SerdeFormat::RawBytesUnchecked) {
        zk_srs* p = nullptr;
        std::vector<uint8_t> g2(128), s_g2(128);
        c.check(zk_params_read(c.raw(), file.data(), file.size(), (int)format, &p, g2.data(), s_g2.data()));
        ParamsKZG out(c, p);
        const size_t gl = format == SerdeFormat::Processed ? 64 : 128;
        g2.resize(gl);
        s_g2.resize(gl);
        out.g2_ = std::move(g2);
        out.s_g2_ = std::move(s_g2);
        return out;
    }
    // ParamsKZG::write_custom(writer, format)
    std::vector<uint8_t> write_custom(SerdeFormat format = SerdeFormat::RawBytesUnchecked) const {
        size_t len = 0;
        c_.check(zk_params_write(c_.raw(), srs_, g2_.data(), s_g2_.data(), (int)format, nullptr, 0, &len));
        std::vector<uint8_t> out(len);
        c_.check(zk_params_write(c_.raw(), srs_, g2_.data(), s_g2_.data(), (int)format, out.data(), out.size(), &len));
        return out;
    }
    const std::vector<uint8_t>& g2() const { return g2_; }
    const std::vector<uint8_t>& s_g2() const { return s_g2_; }
    // ParamsKZG::downsize(k): g truncated, Lagrange basis of the smaller domain recomputed on the device
    ParamsKZG downsize(uint32_t new_k) const {
        zk_srs* p = nullptr;
        c_.check(zk_srs_downsize(c_.raw(), srs_, new_k, &p));
        ParamsKZG out(c_, p);
        out.g2_ = g2_;
        out.s_g2_ = s_g2_;
        return out;
    }
    ParamsKZG(ParamsKZG&& o) noexcept : c_(o.c_), srs_(o.srs_), g2_(std::move(o.g2_)), s_g2_(std::move(o.s_g2_)) { o.srs_ = nullptr; }
    ~ParamsKZG() { if (srs_) zk_srs_destroy(c_.raw(), srs_); }
    uint32_t k() const { return zk_srs_k(srs_); }
    uint64_t n() const { return uint64_t(1) << k(); }
    // ParamsKZG::commit (coefficient basis) / commit_lagrange
    G1Affine commit(const Context::Buffer& poly, size_t n) const { G1Affine o{}; c_.check(zk_commit(c_.raw(), srs_, 0, poly.ptr(), n, o.data())); return o; }
    G1Affine commit_lagrange(const Context::Buffer& poly, size_t n) const { G1Affine o{}; c_.check(zk_commit(c_.raw(), srs_, 1, poly.ptr(), n, o.data())); return o; }
    // every column of a phase in one pipelined batch
    std::vector<G1Affine> commit_lagrange_batch(const std::vector<const void*>& cols, size_t n) const {
        std::vector<G1Affine> o(cols.size());
        c_.check(zk_commit_batch(c_.raw(), srs_, 1, cols.data(), cols.size(), n, o.data()));
        return o;
    }
    const zk_srs* raw() const { return srs_; }
   private:
    ParamsKZG(const Context& c, zk_srs* p) : c_(c), srs_(p) {}
    const Context& c_;
    zk_srs* srs_;
    std::vector<uint8_t> g2_, s_g2_;   // G2 generator and s * generator, file encoding
};

// plonk::keygen_pk result.  circuit_blob: a key blob of version 3 (fixed and sigma columns as Montgomery elements) or version 4
// (typed fixed cells and halo2's Assembly::mapping; the sigma columns are built on the device) -- the same key either way
class ProvingKey {
   public:
    ProvingKey(const Context& c, const ParamsKZG& params, const std::vector<uint8_t>& circuit_blob) : c_(c) {
        c_.check(zk_pk_create(c_.raw(), params.raw(), circuit_blob.data(), circuit_blob.size(), &pk_));
    }
    ~ProvingKey() { zk_pk_destroy(c_.raw(), pk_); }
    ProvingKey(const ProvingKey&) = delete;
    ProvingKey& operator=(const ProvingKey&) = delete;
    const zk_pk* raw() const { return pk_; }
    // install upstream's `vk.transcript_repr()` (the first scalar every proof absorbs)
    void set_transcript_repr(const Fr& repr) { c_.check(zk_pk_set_transcript_repr(c_.raw(), pk_, repr.data())); }
   private:
    const Context& c_;
    zk_pk* pk_ = nullptr;
};

// plonk::create_proof(params, pk, circuits, instances, rng, transcript): the transcript bytes come back
inline std::vector<uint8_t> create_proof(const Context& c, const ProvingKey& pk, const std::vector<const void*>& advice_columns,
                                         const std::vector<const void*>& instance_columns, const std::array<uint8_t, 16>& rng_seed) {
    std::vector<uint8_t> proof(size_t(1) << 20);
    size_t len = 0;
    c.check(zk_create_proof(c.raw(), pk.raw(), advice_columns.data(), instance_columns.data(), rng_seed.data(), proof.data(), proof.size(), &len));
    proof.resize(len);
    return proof;
}

// The phase-by-phase session behind plonk::create_proof for circuits whose later phases depend on challenges (the SuperCircuit has
// three phases [REF zkevm-circuits/src/util.rs:120-133]): begin -> advice_phase per phase (the host synthesises that phase's columns
// with the challenges returned so far) -> finish.  What the Rust shim drives through ffi.rs.
class ProofSession {
   public:
    // instances as halo2 takes them: exactly these values are absorbed, the columns are zero-padded on the device
    ProofSession(const Context& c, const ProvingKey& pk, const std::vector<std::vector<Fr>>& instances, const std::array<uint8_t, 16>& rng_seed, bool shplonk = true) : c_(c) {
        std::vector<const void*> ptrs;
        std::vector<uint32_t> lens;
        for (const auto& col : instances) { ptrs.push_back(col.data()); lens.push_back((uint32_t)col.size()); }
        c_.check(zk_proof_begin_instances(c_.raw(), pk.raw(), ptrs.data(), lens.data(), rng_seed.data(), &s_));
        uint32_t shape[16] = {0};
        int rc = zk_pk_shape(c_.raw(), pk.raw(), shape);
        if (rc == ZK_OK) rc = zk_proof_set_multiopen(c_.raw(), s_, shplonk ? ZK_MULTIOPEN_SHPLONK : ZK_MULTIOPEN_GWC);
        if (rc != ZK_OK) { zk_proof_abort(c_.raw(), s_); s_ = nullptr; c_.check(rc); }
        num_challenges_ = shape[10];
    }
    ~ProofSession() { if (s_) zk_proof_abort(c_.raw(), s_); }
    ProofSession(const ProofSession&) = delete;
    ProofSession& operator=(const ProofSession&) = delete;
    // Poseidon (gen_snark_shplonk) or Keccak / EVM (gen_evm_proof_shplonk) instead of Blake2b: right after construction
    void set_transcript_kind(int kind) { c_.check(zk_proof_set_transcript_kind(c_.raw(), s_, kind)); }
    // commits the columns of the current phase (column_index[j] -> columns[j], n x 32 B each); returns the challenges that become usable after it
    std::vector<Fr> advice_phase(const std::vector<uint32_t>& column_index, const std::vector<const void*>& columns) {
        std::vector<Fr> ch(num_challenges_ ? num_challenges_ : 1);
        uint32_t cnt = (uint32_t)ch.size();
        c_.check(zk_proof_advice_phase(c_.raw(), s_, column_index.data(), columns.data(), (uint32_t)column_index.size(), ch.data(), &cnt));
        ch.resize(cnt);
        return ch;
    }
    // the same for columns resident on the device (device pointers); in_place: the session works in those buffers (it overwrites their
    // blinding rows) until finish() or the destructor returns
    std::vector<Fr> advice_phase_dev(const std::vector<uint32_t>& column_index, const std::vector<const void*>& device_columns, bool in_place = false) {
        std::vector<Fr> ch(num_challenges_ ? num_challenges_ : 1);
        uint32_t cnt = (uint32_t)ch.size();
        c_.check(zk_proof_advice_phase_dev(c_.raw(), s_, column_index.data(), device_columns.data(), (uint32_t)column_index.size(), in_place ? ZK_ADVICE_DEV_IN_PLACE : 0u, ch.data(), &cnt));
        ch.resize(cnt);
        return ch;
    }
    // the same for host columns held as the integers they are (zk_proof_advice_phase_typed): cell_bytes[j] = 1, 2, 4, 8 or 16 for n
    // little-endian unsigned cells of that size, 32 for Montgomery Fr.  Narrow columns cross PCIe at their own width and are expanded on
    // the device; same challenges, same proof.  Not for sharded sessions.  Packed cells that are already on the device:
    // advice_phase_typed_dev.
    std::vector<Fr> advice_phase_typed(const std::vector<uint32_t>& column_index, const std::vector<const void*>& columns, const std::vector<uint8_t>& cell_bytes) {
        if (cell_bytes.size() != column_index.size() || columns.size() != column_index.size()) throw Error(ZK_ERR_INVALID_ARG, "advice_phase_typed: one column and one cell width per column index");
        std::vector<Fr> ch(num_challenges_ ? num_challenges_ : 1);
        uint32_t cnt = (uint32_t)ch.size();
        c_.check(zk_proof_advice_phase_typed(c_.raw(), s_, column_index.data(), columns.data(), cell_bytes.data(), (uint32_t)column_index.size(), ch.data(), &cnt));
        ch.resize(cnt);
        return ch;
    }
    // the same for cells resident on the device (zk_proof_advice_phase_typed_dev; a witness kernel's output): device pointers to at
    // least usable_rows packed cells (cell_bytes[j] = 1, 2, 4, 8, 16) or to an n x 32 B Montgomery column (32).  Expanded straight into
    // the session's buffers, sixteen columns per launch; the caller's buffers are only read, and not after the call returns.
    std::vector<Fr> advice_phase_typed_dev(const std::vector<uint32_t>& column_index, const std::vector<const void*>& device_columns, const std::vector<uint8_t>& cell_bytes) {
        if (cell_bytes.size() != column_index.size() || device_columns.size() != column_index.size()) throw Error(ZK_ERR_INVALID_ARG, "advice_phase_typed_dev: one column and one cell width per column index");
        std::vector<Fr> ch(num_challenges_ ? num_challenges_ : 1);
        uint32_t cnt = (uint32_t)ch.size();
        c_.check(zk_proof_advice_phase_typed_dev(c_.raw(), s_, column_index.data(), device_columns.data(), cell_bytes.data(), (uint32_t)column_index.size(), ch.data(), &cnt));
        ch.resize(cnt);
        return ch;
    }
    // the vanishing argument's "random" polynomial: ZK_VANISHING_ONE (the reference's own proofs; default) or ZK_VANISHING_UNIFORM (upstream halo2)
    void set_vanishing_random(int kind) { c_.check(zk_proof_set_vanishing_random(c_.raw(), s_, kind)); }
    // MockProver's row checks over the columns the session holds, under its own challenges (after the last phase)
    std::vector<zk_mock_failure> mock_verify(size_t max_records = 4096) {
        std::vector<zk_mock_failure> out(max_records ? max_records : 1);
        size_t count = 0;
        c_.check(zk_proof_mock_verify(c_.raw(), s_, nullptr, 0, nullptr, 0, out.data(), max_records, &count));
        out.resize(count < max_records ? count : max_records);
        return out;
    }
    // the proof bytes; the session is gone afterwards
    std::vector<uint8_t> finish() {
        std::vector<uint8_t> proof(size_t(1) << 20);
        size_t len = 0;
        zk_proof* s = s_;
        s_ = nullptr;                       // zk_proof_finish consumes the session on success and on failure
        c_.check(zk_proof_finish(c_.raw(), s, proof.data(), proof.size(), &len));
        proof.resize(len);
        return proof;
    }
   private:
    const Context& c_;
    zk_proof* s_ = nullptr;
    uint32_t num_challenges_ = 0;
};

// dev::MockProver::run(k, &circuit, instances) + verify_par() / verify_at_rows_par(gate_rows, lookup_rows): the failures, sorted
// (empty = assert_satisfied_par passes).  challenges empty = MockProver's own chain (zk_host_mock_challenges).
inline std::vector<zk_mock_failure> mock_verify(const Context& c, const ProvingKey& pk, const std::vector<const void*>& advice_columns,
                                                const std::vector<const void*>& instance_columns, const std::vector<Fr>& challenges = {},
                                                const std::vector<uint32_t>* gate_rows = nullptr, const std::vector<uint32_t>* lookup_rows = nullptr,
                                                size_t max_records = 4096) {
    std::vector<zk_mock_failure> out(max_records ? max_records : 1);
    size_t count = 0;
    c.check(zk_mock_verify(c.raw(), pk.raw(), advice_columns.data(), instance_columns.data(), challenges.empty() ? nullptr : challenges.data(),
                           gate_rows ? gate_rows->data() : nullptr, gate_rows ? gate_rows->size() : 0, lookup_rows ? lookup_rows->data() : nullptr,
                           lookup_rows ? lookup_rows->size() : 0, out.data(), max_records, &count));
    out.resize(count < max_records ? count : max_records);
    return out;
}

// The same with `instances: &[&[Fr]]` as halo2 takes them -- exactly these values are absorbed into
// the transcript, the columns are zero-padded on the device -- for single-phase circuits (with
// several phases the host re-synthesises between zk_proof_advice_phase calls).
inline std::vector<uint8_t> create_proof(const Context& c, const ProvingKey& pk, const std::vector<const void*>& advice_columns,
                                         const std::vector<std::vector<Fr>>& instances, const std::array<uint8_t, 16>& rng_seed, bool shplonk = true) {
    std::vector<const void*> ptrs;
    std::vector<uint32_t> lens, index;
    for (const auto& col : instances) { ptrs.push_back(col.data()); lens.push_back((uint32_t)col.size()); }
    for (uint32_t i = 0; i < advice_columns.size(); ++i) index.push_back(i);
    zk_proof* sess = nullptr;
    c.check(zk_proof_begin_instances(c.raw(), pk.raw(), ptrs.data(), lens.data(), rng_seed.data(), &sess));
    std::vector<uint8_t> proof(size_t(1) << 20);
    size_t len = 0;
    uint32_t shape[16] = {0};
    int rc = zk_pk_shape(c.raw(), pk.raw(), shape);
    std::vector<Fr> challenges(shape[10] ? shape[10] : 1);              // sized from the key: a phase writes every challenge it yields
    uint32_t num_challenges = (uint32_t)challenges.size();
    if (rc == ZK_OK) rc = zk_proof_set_multiopen(c.raw(), sess, shplonk ? 1 : 0);
    if (rc == ZK_OK) rc = zk_proof_advice_phase(c.raw(), sess, index.data(), advice_columns.data(), (uint32_t)index.size(), challenges.data(), &num_challenges);
    if (rc != ZK_OK) { zk_proof_abort(c.raw(), sess); c.check(rc); }
    c.check(zk_proof_finish(c.raw(), sess, proof.data(), proof.size(), &len));
    proof.resize(len);
    return proof;
}

// plonk::VerifyingKey: the constraint system (a key blob, its column data not needed), the F fixed then P sigma commitments and
// vk.transcript_repr; host only
class VerifyingKey {
   public:
    VerifyingKey(const std::vector<uint8_t>& circuit_blob, const std::vector<G1Affine>& commitments, const Fr& transcript_repr) {
        const int rc = zk_vk_create(circuit_blob.data(), circuit_blob.size(), commitments.data(), commitments.size(), transcript_repr.data(), &vk_);
        if (rc) throw Error(rc, "zk_vk_create: malformed constraint system, or F + P commitments expected");
    }
    // the verifying key of a proving key (keygen_vk's commitments and repr, read back from the device key)
    static VerifyingKey from_pk(const Context& c, const ProvingKey& pk, const std::vector<uint8_t>& circuit_blob) {
        uint32_t shape[16] = {0};
        c.check(zk_pk_shape(c.raw(), pk.raw(), shape));
        std::vector<G1Affine> com(shape[3] + shape[6]);
        Fr repr{};
        c.check(zk_pk_vk(c.raw(), pk.raw(), com.data(), repr.data()));
        return VerifyingKey(circuit_blob, com, repr);
    }
    VerifyingKey(VerifyingKey&& o) noexcept : vk_(o.vk_) { o.vk_ = nullptr; }
    VerifyingKey(const VerifyingKey&) = delete;
    VerifyingKey& operator=(const VerifyingKey&) = delete;
    ~VerifyingKey() { zk_vk_destroy(vk_); }
    const zk_vk* raw() const { return vk_; }
    size_t proof_len(int transcript_kind, bool shplonk) const {
        size_t len = 0;
        const int rc = zk_vk_proof_len(vk_, transcript_kind, shplonk ? ZK_MULTIOPEN_SHPLONK : ZK_MULTIOPEN_GWC, &len);
        if (rc) throw Error(rc, "zk_vk_proof_len: bad argument");
        return len;
    }
   private:
    zk_vk* vk_ = nullptr;
};

// plonk::verify_proof: one proof = SingleStrategy, several = AccumulatorStrategy (one MSM, one pairing check).  instances[b][i]:
// the values of instance column i of proof b; g2 / s_g2 from the params (ParamsKZG::g2 / s_g2, RawBytes).  false = rejected.
inline bool verify_proof(const Context& c, const VerifyingKey& vk, const std::vector<std::vector<uint8_t>>& proofs,
                         const std::vector<std::vector<std::vector<Fr>>>& instances, int transcript_kind, bool shplonk,
                         const std::vector<uint8_t>& g2, const std::vector<uint8_t>& s_g2) {
    if (proofs.size() != instances.size() || g2.size() != 128 || s_g2.size() != 128) throw Error(ZK_ERR_INVALID_ARG, "verify_proof: one instance set per proof, 128-byte G2 points");
    std::vector<std::vector<const void*>> cols(proofs.size());
    std::vector<std::vector<uint32_t>> lens(proofs.size());
    std::vector<const void* const*> col_ptrs;
    std::vector<const uint32_t*> len_ptrs;
    std::vector<const void*> proof_ptrs;
    std::vector<size_t> proof_lens;
    for (size_t b = 0; b < proofs.size(); ++b) {
        for (const auto& col : instances[b]) { cols[b].push_back(col.data()); lens[b].push_back((uint32_t)col.size()); }
        col_ptrs.push_back(cols[b].data());
        len_ptrs.push_back(lens[b].data());
        proof_ptrs.push_back(proofs[b].data());
        proof_lens.push_back(proofs[b].size());
    }
    int ok = 0;
    c.check(zk_verify_proofs(c.raw(), vk.raw(), proofs.size(), col_ptrs.data(), len_ptrs.data(), proof_ptrs.data(), proof_lens.data(), transcript_kind,
                             shplonk ? ZK_MULTIOPEN_SHPLONK : ZK_MULTIOPEN_GWC, g2.data(), s_g2.data(), &ok));
    return ok == 1;
}

// PlonkSuccinctVerifier::verify for a batch (zk_verify_accumulators): per proof the KZG accumulator of its own openings, then the
// accumulators its instances carry at acc_indices (12 {column, row} cells each).  NO pairing is done: ok[b] says proof b is well
// formed, not that it is accepted -- decide every accumulator with zk_host_accumulator_check, or combine them with
// zk_host_accumulate first.
struct Accumulators {
    size_t per_proof = 0;                              // 1 + the number of carried accumulators
    std::vector<std::array<uint64_t, 8>> lhs, rhs;     // proofs x per_proof, 64 B affine Montgomery; zero where ok is false
    std::vector<bool> ok;
};
inline Accumulators verify_accumulators(const Context& c, const VerifyingKey& vk, const std::vector<std::vector<uint8_t>>& proofs,
                                        const std::vector<std::vector<std::vector<Fr>>>& instances, int transcript_kind, bool shplonk,
                                        const std::vector<std::array<std::array<uint32_t, 2>, 12>>& acc_indices = {}) {
    if (proofs.size() != instances.size()) throw Error(ZK_ERR_INVALID_ARG, "verify_accumulators: one instance set per proof");
    std::vector<std::vector<const void*>> cols(proofs.size());
    std::vector<std::vector<uint32_t>> lens(proofs.size());
    std::vector<const void* const*> col_ptrs;
    std::vector<const uint32_t*> len_ptrs;
    std::vector<const void*> proof_ptrs;
    std::vector<size_t> proof_lens;
    for (size_t b = 0; b < proofs.size(); ++b) {
        for (const auto& col : instances[b]) { cols[b].push_back(col.data()); lens[b].push_back((uint32_t)col.size()); }
        col_ptrs.push_back(cols[b].data());
        len_ptrs.push_back(lens[b].data());
        proof_ptrs.push_back(proofs[b].data());
        proof_lens.push_back(proofs[b].size());
    }
    Accumulators out;
    out.per_proof = 1 + acc_indices.size();
    out.lhs.resize(proofs.size() * out.per_proof);
    out.rhs.resize(proofs.size() * out.per_proof);
    std::vector<int> ok(proofs.size(), 0);
    c.check(zk_verify_accumulators(c.raw(), vk.raw(), proofs.size(), col_ptrs.data(), len_ptrs.data(), proof_ptrs.data(), proof_lens.data(), transcript_kind,
                                   shplonk ? ZK_MULTIOPEN_SHPLONK : ZK_MULTIOPEN_GWC, acc_indices.empty() ? nullptr : &acc_indices[0][0][0], acc_indices.size(),
                                   out.lhs.data(), out.rhs.data(), ok.data()));
    for (int v : ok) out.ok.push_back(v == 1);
    return out;
}
// the inverse of zk_host_accumulator_limbs; false (points zeroed) for a limb of 2^88 or more, a coordinate of p or more, a point off the curve
inline bool accumulator_from_limbs(const std::array<Fr, 12>& limbs, std::array<uint64_t, 8>& lhs, std::array<uint64_t, 8>& rhs) {
    int ok = 0;
    const int rc = zk_host_accumulator_from_limbs(limbs.data(), lhs.data(), rhs.data(), &ok);
    if (rc) throw Error(rc, "zk_host_accumulator_from_limbs: bad argument");
    return ok == 1;
}
// num_segments independent MSMs over arbitrary device bases in one pass (zk_msm_g1_segments): offsets.size() - 1 results
inline std::vector<std::array<uint64_t, 8>> msm_segments(const Context& c, const void* d_scalars, const void* d_bases, const std::vector<uint32_t>& offsets) {
    if (offsets.empty()) throw Error(ZK_ERR_INVALID_ARG, "msm_segments: one offset more than there are segments");
    std::vector<std::array<uint64_t, 8>> out(offsets.size() - 1);
    c.check(zk_msm_g1_segments(c.raw(), d_scalars, d_bases, offsets.data(), out.size(), out.data()));
    return out;
}

}  // namespace halo2
}  // namespace zk

//! `extern "C"` transcription of `include/zkmi355.h` — the subset the shim calls.
//! Kept in sync by `tests/test_abi.py::test_rust_ffi_block_matches_the_header` (every function
//! declared here must exist in the header with the same number of parameters).
//!
//! Layout contract: `Fr` / `Fq` cross the boundary as their in-memory form in
//! halo2curves — 4 × u64 little-endian limbs, Montgomery — so `&[Fr]` is passed as `*const c_void`
//! without conversion; `G1Affine` is `{x, y}` = 64 bytes, identity = all zero.
#![allow(non_camel_case_types, dead_code)]

use std::os::raw::{c_char, c_int, c_void};

#[repr(C)]
pub struct zk_ctx {
    _private: [u8; 0],
}
#[repr(C)]
pub struct zk_srs {
    _private: [u8; 0],
}
#[repr(C)]
pub struct zk_pk {
    _private: [u8; 0],
}
#[repr(C)]
pub struct zk_proof {
    _private: [u8; 0],
}
#[repr(C)]
pub struct zk_vk {
    _private: [u8; 0],
}

pub const ZK_OK: c_int = 0;
pub const ZK_ERR_INVALID_ARG: c_int = -1;
pub const ZK_ERR_HIP: c_int = -2;
pub const ZK_ERR_OOM: c_int = -3;
pub const ZK_ERR_NO_DEVICE: c_int = -4;
pub const ZK_ERR_UNSUPPORTED: c_int = -5;

pub const ZK_MULTIOPEN_GWC: c_int = 0;
pub const ZK_MULTIOPEN_SHPLONK: c_int = 1;

pub const ZK_TRANSCRIPT_BLAKE2B: c_int = 0;
pub const ZK_TRANSCRIPT_POSEIDON: c_int = 1;
pub const ZK_TRANSCRIPT_EVM: c_int = 2;

/// `zk_field_vec_op` op: `d_out[i] = c + sum_j w_j * cell_j[i]` across typed columns.  For this op `d_a` is a HOST pointer to a
/// `zk_row_rlc` and `d_b` a HOST pointer to `(count + 1) x 32 B` Montgomery Fr (`c`, then the weights).
pub const ZK_OP_ROW_RLC: c_int = 8;
/// `zk_row_rlc`: the column table of `ZK_OP_ROW_RLC`; `d_cols` and `widths` are host arrays of `count` entries, each `d_cols[j]` a
/// device pointer to `n` cells of `widths[j]` bytes (1, 2, 4, 8, 16: packed little-endian unsigned; 32: Montgomery Fr).
#[repr(C)]
pub struct zk_row_rlc {
    pub count: u32,
    pub d_cols: *const *const c_void,
    pub widths: *const u8,
}
/// `zk_field_vec_op` ops: `out[i] = m[kind_i] * out[i - 1] + w[kind_i] * cell[i]` along a typed column (`out[-1] = z0`), and the
/// same from the last row down (`out[n] = z0`).  For these ops `d_a` is a HOST pointer to a `zk_scan_rlc` and `d_b` a HOST pointer to
/// `9 x 32 B` Montgomery Fr: `z0`, then `m_0, w_0 .. m_3, w_3`.
pub const ZK_OP_SCAN_RLC: c_int = 9;
pub const ZK_OP_SCAN_RLC_REV: c_int = 10;
/// `zk_scan_rlc`: `d_cells` is a device pointer to `n` cells of `width` bytes (1, 2, 4, 8, 16: packed little-endian unsigned; 32:
/// Montgomery Fr), `d_kinds` a device pointer to `n` kind bytes (low two bits) or null (every row kind 0).
#[repr(C)]
pub struct zk_scan_rlc {
    pub d_cells: *const c_void,
    pub width: u32,
    pub d_kinds: *const u8,
}
/// `zk_field_vec_op` op: `d_out[i] = num[i] * inv0(c + sum_j w_j * cell_j[i])` across typed columns, `inv0(0) = 0` -- the
/// `Assigned::Rational(num, den)` cells that `batch_invert_assigned` would invert on the host.  For this op `d_a` is a HOST pointer
/// to a `zk_row_inv0` and `d_b` a HOST pointer to `(count + 1) x 32 B` Montgomery Fr (`c`, then the weights).
pub const ZK_OP_ROW_INV0: c_int = 12;
/// `zk_row_inv0`: `count`, `d_cols` and `widths` as in `zk_row_rlc`; `d_num` is null (every numerator is one) or a device pointer to
/// `n` cells of `num_width` bytes (1, 2, 4, 8, 16: packed little-endian unsigned; 32: Montgomery Fr).
#[repr(C)]
pub struct zk_row_inv0 {
    pub count: u32,
    pub d_cols: *const *const c_void,
    pub widths: *const u8,
    pub d_num: *const c_void,
    pub num_width: u32,
}
/// `zk_field_vec_op` op: the width-3 Poseidon hash columns of the `PoseidonTable` (`hash_id`, `input0`, `input1`) from typed cells --
/// `Fr::hash_with_domain([a, b], domain)` per row and the Poseidon code hash over 31-byte big-endian words.  For this op `d_a` is a
/// HOST pointer to a `zk_poseidon` and `d_b` a HOST pointer to 32 B, the Montgomery Fr `cap_scale` (2^64 for the code hash).
pub const ZK_OP_POSEIDON: c_int = 14;
/// `zk_poseidon.flags`: every row of a message holds the hash of its last row.
pub const ZK_POSEIDON_FINAL: u8 = 1;
/// `zk_poseidon`: device pointers.  `d_cap` may be null (capacity 0), `d_kinds` may be null (every row is a head; otherwise `n`
/// bytes, kind = byte & 3: 0 head, 1 continue, 2 / 3 off), `d_word0` / `d_word1` are optional `n x 32 B` outputs.  Widths 1, 2, 4, 8,
/// 16 (packed little-endian unsigned), 32 (Montgomery Fr) or, for `width0` / `width1`, 31: cell `i` is the 31 big-endian bytes at
/// `ptr + 62 * i`.
#[repr(C)]
pub struct zk_poseidon {
    pub d_in0: *const c_void,
    pub d_in1: *const c_void,
    pub d_cap: *const c_void,
    pub d_kinds: *const u8,
    pub d_word0: *mut c_void,
    pub d_word1: *mut c_void,
    pub width0: u8,
    pub width1: u8,
    pub cap_width: u8,
    pub flags: u8,
}
/// `zk_field_vec_op` op: the hash columns of the `KeccakTable` from message bytes on the device -- `d_out[i]` is `output_rlc`, the
/// Keccak-256 digest of message `i` under the `evm_word` challenge.  For this op `d_a` is a HOST pointer to a `zk_keccak` and `d_b` a
/// HOST pointer to `2 x 32 B` Montgomery Fr: `r_out` (`evm_word`), then `r_in` (`keccak_input`, used with `d_input_rlc`).
pub const ZK_OP_KECCAK: c_int = 16;
/// `zk_keccak`: device pointers.  Message `i` is the `d_lens[i]` bytes at `d_bytes + d_offsets[i]`; offsets and lengths are unsigned
/// little-endian integers of `index_width` (4 or 8) bytes; `d_lens` is the table's `input_len` column as it stands.  `d_digest` and
/// `d_input_rlc` are optional `n x 32 B` outputs.  `flags` must be 0.
#[repr(C)]
pub struct zk_keccak {
    pub d_bytes: *const c_void,
    pub total_bytes: u64,
    pub d_offsets: *const c_void,
    pub d_lens: *const c_void,
    pub d_digest: *mut c_void,
    pub d_input_rlc: *mut c_void,
    pub index_width: u8,
    pub flags: u8,
}
/// `zk_field_vec_op` op: the hash columns of the `SHA256Table` from message bytes on the device -- `d_out[i]` is `output_rlc`, the
/// SHA-256 digest of message `i` under `r_out`.  For this op `d_a` is a HOST pointer to a `zk_sha256` and `d_b` a HOST pointer to
/// `2 x 32 B` Montgomery Fr: `r_out`, then `r_in` (used with `d_input_rlc`).  The reference takes both RLCs of this table under
/// `keccak_input`: pass that challenge twice.
pub const ZK_OP_SHA256: c_int = 18;
/// `zk_sha256`: member for member `zk_keccak`.  `total_bytes` stays below `2^61`.  `flags` must be 0.
#[repr(C)]
pub struct zk_sha256 {
    pub d_bytes: *const c_void,
    pub total_bytes: u64,
    pub d_offsets: *const c_void,
    pub d_lens: *const c_void,
    pub d_digest: *mut c_void,
    pub d_input_rlc: *mut c_void,
    pub index_width: u8,
    pub flags: u8,
}
/// `zk_field_vec_op` op: the stable sort of `n` 64-byte key records (what `rw_to_be_limbs` packs of an RW row), as a permutation --
/// `d_out[i]` is the `u32` index of the record at place `i`.  For this op `d_a` is a HOST pointer to a `zk_key_sort` and `d_b` is
/// null or a HOST pointer to a 64-byte mask: key byte `j` takes part iff `mask[j] != 0`.
pub const ZK_OP_KEY_SORT: c_int = 20;
/// `zk_key_sort`: `d_sorted` may be null.  `flags` must be 0.
#[repr(C)]
pub struct zk_key_sort {
    pub d_keys: *const c_void,
    pub d_sorted: *mut c_void,
    pub flags: u8,
}
/// `zk_field_vec_op` op: the ordering witness of adjacent key records -- `d_out[i]` is `limb_difference_inverse` of rows `i` and
/// `i - 1`.  For this op `d_a` is a HOST pointer to a `zk_key_order` and `d_b` must be null.
pub const ZK_OP_KEY_ORDER: c_int = 22;
/// `zk_key_col`: key bytes `[offset, offset + width)` of a gathered column, width 1, 2 or 4.
#[repr(C)]
pub struct zk_key_col {
    pub offset: u8,
    pub width: u8,
}
/// `zk_key_order`: `cols` and `d_cols` are HOST arrays of `count <= 64` entries; every other pointer is a device pointer, and all
/// but `d_keys` may be null.  `group_limbs` is 30 for the state circuit.  `flags` must be 0.
#[repr(C)]
pub struct zk_key_order {
    pub d_keys: *const c_void,
    pub d_perm: *const c_void,
    pub d_diff: *mut c_void,
    pub d_index: *mut c_void,
    pub d_bits: *mut c_void,
    pub d_not_first: *mut c_void,
    pub group_limbs: u32,
    pub count: u32,
    pub cols: *const zk_key_col,
    pub d_cols: *const *mut c_void,
    pub flags: u8,
}
/// `zk_field_vec_op` op: the rows of the bytecode circuit from code bytes on the device -- `d_out[i]` is the code hash of the bytecode
/// row `i` belongs to, `empty_hash` on padding rows.  For this op `d_a` is a HOST pointer to a `zk_bytecode_rows` and `d_b` a HOST
/// pointer to `32 B`, one Montgomery Fr `empty_hash`.
pub const ZK_OP_BYTECODE_ROWS: c_int = 26;
/// `zk_bytecode_rows`: `d_bytes`, `total_bytes`, `d_offsets`, `d_lens` and `index_width` are those of `zk_keccak`, with `count`
/// entries; `d_hashes` and every output may be null.  `d_acc_kinds` and `d_rlc_kinds` are the kind columns of `ZK_OP_SCAN_RLC`
/// (`push_acc`) and `ZK_OP_SCAN_RLC_REV` (`push_rlc`).  `flags` must be 0.
#[repr(C)]
pub struct zk_bytecode_rows {
    pub d_bytes: *const c_void,
    pub total_bytes: u64,
    pub d_offsets: *const c_void,
    pub d_lens: *const c_void,
    pub d_hashes: *const c_void,
    pub d_tag: *mut c_void,
    pub d_index: *mut c_void,
    pub d_value: *mut c_void,
    pub d_is_code: *mut c_void,
    pub d_push_data_left: *mut c_void,
    pub d_push_data_size: *mut c_void,
    pub d_length: *mut c_void,
    pub d_acc_kinds: *mut c_void,
    pub d_rlc_kinds: *mut c_void,
    pub count: u32,
    pub index_width: u8,
    pub flags: u8,
}
/// `zk_field_vec_op` ops: the rows of the copy circuit and the copy table from copy events on the device.  `ZK_OP_COPY_ROWS` writes
/// the integer columns (`d_out` is the 8-byte `addr` column; `d_a` a HOST pointer to a `zk_copy_rows`, `d_b` null), `ZK_OP_COPY_RLC`
/// the challenge-phase columns (`d_out` is `value_acc`; `d_a` a HOST pointer to a `zk_copy_rlc`, `d_b` a HOST pointer to `2 x 32 B`,
/// Montgomery Fr `r_word` then `r_in`).
pub const ZK_OP_COPY_ROWS: c_int = 28;
pub const ZK_OP_COPY_RLC: c_int = 30;
/// bit 0 of `zk_copy_event::flags`: `src_id == dst_id` and both tags Memory
pub const ZK_COPY_MEMORY_COPY: u8 = 1;
/// `zk_copy_event`: the 88-byte record of one copy event, device data.  The three offsets name runs of `length` bytes in the byte
/// heap; the masks are counts of masked steps at the front and the back of each thread; tags are `CopyDataType` values 1..5.
#[repr(C)]
pub struct zk_copy_event {
    pub src_addr: u64,
    pub src_addr_end: u64,
    pub dst_addr: u64,
    pub dst_addr_bias: u64,
    pub rw_counter: u64,
    pub src_off: u64,
    pub dst_off: u64,
    pub prev_off: u64,
    pub length: u32,
    pub src_front: u32,
    pub src_back: u32,
    pub dst_front: u32,
    pub dst_back: u32,
    pub src_tag: u8,
    pub dst_tag: u8,
    pub flags: u8,
    pub reserved: u8,
}
/// `zk_copy_rows`: the events, the byte heap and the typed outputs of `ZK_OP_COPY_ROWS`; every output may be null.  `flags` must be 0.
#[repr(C)]
pub struct zk_copy_rows {
    pub d_events: *const c_void,
    pub count: u32,
    pub d_bytes: *const c_void,
    pub total_bytes: u64,
    pub flags: u8,
    pub d_is_first: *mut c_void,
    pub d_is_last: *mut c_void,
    pub d_tag: *mut c_void,
    pub d_tag_bits: *mut c_void,
    pub d_value: *mut c_void,
    pub d_value_prev: *mut c_void,
    pub d_mask: *mut c_void,
    pub d_front_mask: *mut c_void,
    pub d_word_index: *mut c_void,
    pub d_src_addr_end: *mut c_void,
    pub d_is_pad: *mut c_void,
    pub d_non_pad_non_mask: *mut c_void,
    pub d_real_bytes_left: *mut c_void,
    pub d_rw_counter: *mut c_void,
    pub d_rwc_inc_left: *mut c_void,
    pub d_types: *mut c_void,
    pub d_src_end_rows: *mut c_void,
}
/// `zk_copy_rlc`: the first five members are those of `zk_copy_rows`; `d_ids` (`count x 2 x 32 B`) and every output may be null.
#[repr(C)]
pub struct zk_copy_rlc {
    pub d_events: *const c_void,
    pub count: u32,
    pub d_bytes: *const c_void,
    pub total_bytes: u64,
    pub flags: u8,
    pub d_ids: *const c_void,
    pub d_id: *mut c_void,
    pub d_id_other: *mut c_void,
    pub d_rlc_acc: *mut c_void,
    pub d_word_rlc: *mut c_void,
    pub d_word_rlc_prev: *mut c_void,
}
/// `zk_field_vec_op` op: the rows of the exponentiation circuit and the exponentiation table from `(base, exponent)` events on the
/// device (`d_out` is the 16-byte `exponentiation_lo_hi` column; `d_a` a HOST pointer to a `zk_exp_rows`, `d_b` null).
pub const ZK_OP_EXP_ROWS: c_int = 32;
/// `zk_exp_event`: the 64-byte record of one exponentiation event, device data: little-endian 64-bit limbs.
#[repr(C)]
pub struct zk_exp_event {
    pub base: [u64; 4],
    pub exponent: [u64; 4],
}
/// `zk_exp_rows`: the events and the typed outputs of `ZK_OP_EXP_ROWS`; every output may be null.  `flags` must be 0.
/// `d_rows_needed` receives `8 x steps + 10` as one `u64` for the caller to compare with `n`.
#[repr(C)]
pub struct zk_exp_rows {
    pub d_events: *const c_void,
    pub count: u32,
    pub flags: u8,
    pub d_is_last: *mut c_void,
    pub d_base_limb: *mut c_void,
    pub d_exponent_lo_hi: *mut c_void,
    pub d_mul_cols: *mut c_void,
    pub d_mul_u16_64: *mut c_void,
    pub d_mul_u16_128: *mut c_void,
    pub d_parity_cols: *mut c_void,
    pub d_parity_u16_64: *mut c_void,
    pub d_parity_u16_128: *mut c_void,
    pub d_rows_needed: *mut c_void,
}
/// `zk_field_vec_op` ops: the eight columns the Poseidon-hash extension adds to the bytecode circuit (`d_out` is `field_input`) and
/// the code-hash rows of the Poseidon table (`d_out` is `input0`), from the code bytes of `zk_bytecode_rows`.  For both `d_a` is a
/// HOST pointer to the struct below and `d_b` null.
pub const ZK_OP_CODE_HASH_ROWS: c_int = 34;
pub const ZK_OP_CODE_HASH_TABLE: c_int = 36;
/// `zk_code_hash_rows`: `d_bytes`, `total_bytes`, `d_offsets`, `d_lens` and `index_width` are those of `zk_keccak`, with `count`
/// entries; every output may be null.  `flags` must be 0.
#[repr(C)]
pub struct zk_code_hash_rows {
    pub d_bytes: *const c_void,
    pub total_bytes: u64,
    pub d_offsets: *const c_void,
    pub d_lens: *const c_void,
    pub d_control_length: *mut c_void,
    pub d_bytes_in_field_index: *mut c_void,
    pub d_bytes_in_field_inv: *mut c_void,
    pub d_is_field_border: *mut c_void,
    pub d_padding_shift: *mut c_void,
    pub d_field_index: *mut c_void,
    pub d_field_index_inv: *mut c_void,
    pub count: u32,
    pub index_width: u8,
    pub flags: u8,
}
/// `zk_code_hash_table`: the same inputs; `d_kinds` and `d_cap` are the kinds and the capacity column of `ZK_OP_POSEIDON`,
/// `d_rows_needed` receives the rows of all bytecodes as one `u64` for the caller to compare with `n`.
#[repr(C)]
pub struct zk_code_hash_table {
    pub d_bytes: *const c_void,
    pub total_bytes: u64,
    pub d_offsets: *const c_void,
    pub d_lens: *const c_void,
    pub d_input1: *mut c_void,
    pub d_control: *mut c_void,
    pub d_heading_mark: *mut c_void,
    pub d_kinds: *mut c_void,
    pub d_cap: *mut c_void,
    pub d_rows_needed: *mut c_void,
    pub count: u32,
    pub index_width: u8,
    pub flags: u8,
}

/// `zk_transcript_vtable`: every transcript operation of a proving session is forwarded to the
/// caller's `T: TranscriptWrite<G1Affine, _>` (see `transcript.rs`).
#[repr(C)]
pub struct zk_transcript_vtable {
    pub common_point: unsafe extern "C" fn(user: *mut c_void, affine64: *const c_void) -> c_int,
    pub common_scalar: unsafe extern "C" fn(user: *mut c_void, fr32: *const c_void) -> c_int,
    pub write_point: unsafe extern "C" fn(user: *mut c_void, affine64: *const c_void) -> c_int,
    pub write_scalar: unsafe extern "C" fn(user: *mut c_void, fr32: *const c_void) -> c_int,
    pub squeeze_challenge: unsafe extern "C" fn(user: *mut c_void, fr32_out: *mut c_void) -> c_int,
}

/// `zk_mock_failure`: one record of `zk_mock_verify` (kind 1 gate polynomial / 2 lookup / 3 permutation; index; sub; row)
#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq, Eq)]
pub struct zk_mock_failure {
    pub kind: u32,
    pub index: u32,
    pub sub: u32,
    pub row: u32,
}
pub const ZK_MOCK_GATE: u32 = 1;
pub const ZK_MOCK_LOOKUP: u32 = 2;
pub const ZK_MOCK_PERMUTATION: u32 = 3;

pub type zk_allgather_fn = unsafe extern "C" fn(user: *mut c_void, send: *const c_void, bytes: usize, recv: *mut c_void) -> c_int;

extern "C" {
    // ---- context
    pub fn zk_ctx_create(device: c_int, out: *mut *mut zk_ctx) -> c_int;
    pub fn zk_ctx_destroy(ctx: *mut zk_ctx);
    /// joins every stream of the library (main, copy, auxiliary, MSM side streams)
    pub fn zk_ctx_sync(ctx: *mut zk_ctx) -> c_int;
    pub fn zk_ctx_streams_busy(ctx: *mut zk_ctx, busy: *mut c_int) -> c_int;
    pub fn zk_last_error(ctx: *const zk_ctx) -> *const c_char;

    // ---- ParamsKZG
    pub fn zk_srs_create(ctx: *mut zk_ctx, k: u32, h_g: *const c_void, h_g_lagrange: *const c_void, out: *mut *mut zk_srs) -> c_int;
    pub fn zk_srs_destroy(ctx: *mut zk_ctx, srs: *mut zk_srs);
    pub fn zk_commit(ctx: *mut zk_ctx, srs: *const zk_srs, basis: c_int, d_scalars: *const c_void, n: usize, h_out_affine: *mut c_void) -> c_int;
    pub fn zk_msm_g1_host(ctx: *mut zk_ctx, h_scalars: *const c_void, h_bases: *const c_void, n: usize, h_out_affine: *mut c_void) -> c_int;

    // ---- keygen_pk / create_proof
    pub fn zk_pk_create(ctx: *mut zk_ctx, srs: *const zk_srs, h_blob: *const c_void, blob_len: usize, out: *mut *mut zk_pk) -> c_int;
    pub fn zk_pk_destroy(ctx: *mut zk_ctx, pk: *mut zk_pk);
    pub fn zk_pk_vk(ctx: *mut zk_ctx, pk: *const zk_pk, h_commitments: *mut c_void, h_vk_repr: *mut c_void) -> c_int;
    pub fn zk_pk_set_transcript_repr(ctx: *mut zk_ctx, pk: *mut zk_pk, h_repr_fr32: *const c_void) -> c_int;
    pub fn zk_pk_shape(ctx: *mut zk_ctx, pk: *const zk_pk, out16: *mut u32) -> c_int;

    /// dev::MockProver::verify_par / verify_at_rows_par on the device (NULL row lists = every usable row)
    pub fn zk_mock_verify(ctx: *mut zk_ctx, pk: *const zk_pk, h_advice: *const *const c_void, h_instance: *const *const c_void, h_challenges: *const c_void,
                          gate_rows: *const u32, num_gate_rows: usize, lookup_rows: *const u32, num_lookup_rows: usize,
                          out: *mut zk_mock_failure, cap: usize, count: *mut usize) -> c_int;
    pub fn zk_proof_mock_verify(ctx: *mut zk_ctx, proof: *mut zk_proof, gate_rows: *const u32, num_gate_rows: usize, lookup_rows: *const u32, num_lookup_rows: usize,
                                out: *mut zk_mock_failure, cap: usize, count: *mut usize) -> c_int;
    pub fn zk_host_mock_challenges(count: u32, out_fr32: *mut c_void) -> c_int;

    pub fn zk_proof_begin_instances(ctx: *mut zk_ctx, pk: *const zk_pk, h_instance: *const *const c_void, h_instance_len: *const u32, seed16: *const u8, out: *mut *mut zk_proof) -> c_int;
    pub fn zk_proof_set_multiopen(ctx: *mut zk_ctx, proof: *mut zk_proof, kind: c_int) -> c_int;
    pub fn zk_proof_set_transcript(ctx: *mut zk_ctx, proof: *mut zk_proof, vtable: *const zk_transcript_vtable, user: *mut c_void) -> c_int;
    pub fn zk_proof_set_transcript_kind(ctx: *mut zk_ctx, proof: *mut zk_proof, kind: c_int) -> c_int;
    pub fn zk_proof_set_sharding(ctx: *mut zk_ctx, proof: *mut zk_proof, rank: u32, world: u32, gather: zk_allgather_fn, user: *mut c_void) -> c_int;
    pub fn zk_proof_advice_phase(ctx: *mut zk_ctx, proof: *mut zk_proof, col_index: *const u32, h_cols: *const *const c_void, ncols: u32, h_challenges: *mut c_void, num_challenges: *mut u32) -> c_int;
    pub fn zk_proof_finish(ctx: *mut zk_ctx, proof: *mut zk_proof, h_proof: *mut c_void, proof_cap: usize, proof_len: *mut usize) -> c_int;
    pub fn zk_proof_abort(ctx: *mut zk_ctx, proof: *mut zk_proof);

    // ---- pinned host memory for witness columns (optional: uploads at link rate)
    pub fn zk_host_register(ctx: *mut zk_ctx, ptr: *mut c_void, bytes: usize) -> c_int;
    pub fn zk_host_unregister(ctx: *mut zk_ctx, ptr: *mut c_void) -> c_int;

    // ---- succinct verification of child snarks (aggregation layers): accumulators per proof, no pairing
    pub fn zk_msm_g1_segments(ctx: *mut zk_ctx, d_scalars: *const c_void, d_bases: *const c_void, h_seg_offsets: *const u32, num_segments: usize, h_out_affine: *mut c_void) -> c_int;
    pub fn zk_verify_accumulators(ctx: *mut zk_ctx, vk: *const zk_vk, count: usize, h_instances: *const *const *const c_void, h_instance_lens: *const *const u32,
                                  h_proofs: *const *const c_void, h_proof_lens: *const usize, transcript_kind: c_int, multiopen: c_int, acc_indices: *const u32,
                                  num_prior: usize, h_lhs: *mut c_void, h_rhs: *mut c_void, ok: *mut c_int) -> c_int;
    pub fn zk_host_accumulator_from_limbs(limbs12_fr: *const c_void, lhs: *mut c_void, rhs: *mut c_void, ok: *mut c_int) -> c_int;
}

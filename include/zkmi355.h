/*
 * zkmi355 -- C ABI of the MI355X-native Halo2/KZG proving hot path (BN254).
 *
 * This is the drop-in boundary of SURVEY.md section 8(b): a thin Rust shim crate that keeps the
 * `halo2_proofs` API (create_proof / keygen_* / ParamsKZG, transcript + RNG + Circuit::synthesize
 * stay in Rust) binds exactly these symbols; see INTEGRATION.md for the `extern "C"` block.
 * The reference has no FFI for this path today; the interfaces each entry point replaces live in
 * the external crates pinned by the reference (`[REF Cargo.lock:2214-2216]` halo2_proofs 1.1.0 @
 * scroll-tech/halo2 e5ddf67, `[REF Cargo.lock:2239-2241]` halo2curves 0.1.0 @ a495a7b) and are
 * reached from the reference call sites listed per function below.
 *
 * Conventions
 *   - every function returns 0 (ZK_OK) or a negative zk_status; nothing unwinds across the ABI;
 *     zk_last_error(ctx) returns a human-readable message for the last failure on that ctx.
 *   - Fr / Fq element: 32 bytes = 4 x u64 little-endian limbs, MONTGOMERY form (R = 2^256):
 *     byte-identical to halo2curves' in-memory layout and to SerdeFormat::RawBytes.
 *   - G1Affine: 64 bytes {x, y}; identity = all zero.   G1 (Jacobian): 96 bytes {x, y, z}.
 *   - pointers named d_* are DEVICE pointers (from zk_buf_alloc or any hipMalloc / torch tensor);
 *     pointers named h_* are host pointers.  The caller owns every buffer it passes.
 *   - a zk_ctx is used by one host thread at a time; different contexts are independent.
 *   - all device work is enqueued on the context's stream (zk_ctx_set_stream); functions that
 *     return host results synchronise that stream before returning.
 */
#ifndef ZKMI355_H
#define ZKMI355_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct zk_ctx zk_ctx;
typedef struct zk_srs zk_srs;

typedef enum zk_status {
    ZK_OK = 0,
    ZK_ERR_INVALID_ARG = -1,  /* null pointer, n not a power of two, k > 28 (Fr two-adicity) ... */
    ZK_ERR_HIP = -2,          /* a HIP runtime call failed (message has the HIP error string)   */
    ZK_ERR_OOM = -3,          /* device allocation failed                                       */
    ZK_ERR_NO_DEVICE = -4,    /* no gfx950 device visible: there is NO CPU fallback            */
    ZK_ERR_UNSUPPORTED = -5
} zk_status;

enum { ZK_FIELD_FR = 0, ZK_FIELD_FQ = 1 };
enum { ZK_OP_ADD = 0, ZK_OP_SUB = 1, ZK_OP_MUL = 2, ZK_OP_SCAN_AFFINE = 3, ZK_OP_SCAN_AFFINE_REV = 4 };
/* the row RLC of zk_field_vec_op (described there): its d_a is a HOST pointer to this table, itself made of host arrays */
#define ZK_OP_ROW_RLC 8
typedef struct zk_row_rlc {
    uint32_t count;             /* columns                                                        */
    const void* const* d_cols;  /* count device pointers                                          */
    const uint8_t* widths;      /* count cell widths in bytes: 1, 2, 4, 8, 16 (packed) or 32 (Fr) */
} zk_row_rlc;
/* the running RLC of zk_field_vec_op (described there): its d_a is a HOST pointer to this struct */
#define ZK_OP_SCAN_RLC 9
#define ZK_OP_SCAN_RLC_REV 10
typedef struct zk_scan_rlc { const void* d_cells; uint32_t width; const uint8_t* d_kinds; } zk_scan_rlc;
/* the inverse-or-zero of a row RLC of zk_field_vec_op (described there): its d_a is a HOST pointer to this struct, whose first three
 * members are those of zk_row_rlc; d_num is a device pointer or NULL */
#define ZK_OP_ROW_INV0 12
typedef struct zk_row_inv0 { uint32_t count; const void* const* d_cols; const uint8_t* widths; const void* d_num; uint32_t num_width; } zk_row_inv0;
/* the width-3 Poseidon hash columns of zk_field_vec_op (described there): its d_a is a HOST pointer to this struct, whose pointers
 * are device pointers */
#define ZK_OP_POSEIDON 14
#define ZK_POSEIDON_FINAL 1
typedef struct zk_poseidon {
    const void* d_in0; const void* d_in1; const void* d_cap;
    const uint8_t* d_kinds;
    void* d_word0; void* d_word1;
    uint8_t width0, width1, cap_width;
    uint8_t flags;
} zk_poseidon;
/* the Keccak-256 table columns of zk_field_vec_op (described there): its d_a is a HOST pointer to this struct, whose pointers are
 * device pointers */
#define ZK_OP_KECCAK 16
typedef struct zk_keccak {
    const void* d_bytes;      /* device: the bytes the messages live in */
    uint64_t    total_bytes;  /* bytes readable at d_bytes */
    const void* d_offsets;    /* device: n unsigned little-endian offsets into d_bytes */
    const void* d_lens;       /* device: n unsigned little-endian byte lengths */
    void*       d_digest;     /* device, n x 32 B, or NULL: the digests, in digest byte order */
    void*       d_input_rlc;  /* device, n x 32 B Montgomery Fr, or NULL */
    uint8_t     index_width;  /* 4 or 8: width of an offset and of a length */
    uint8_t     flags;        /* must be 0 */
} zk_keccak;
/* the SHA-256 table columns of zk_field_vec_op (described there): its d_a is a HOST pointer to this struct, whose pointers are device
 * pointers; the members are zk_keccak's in name, type and order */
#define ZK_OP_SHA256 18
typedef struct zk_sha256 {
    const void* d_bytes;      /* device: the bytes the messages live in */
    uint64_t    total_bytes;  /* bytes readable at d_bytes; below 2^61 */
    const void* d_offsets;    /* device: n unsigned little-endian offsets into d_bytes */
    const void* d_lens;       /* device: n unsigned little-endian byte lengths */
    void*       d_digest;     /* device, n x 32 B, or NULL: the digests, in digest byte order */
    void*       d_input_rlc;  /* device, n x 32 B Montgomery Fr, or NULL */
    uint8_t     index_width;  /* 4 or 8: width of an offset and of a length */
    uint8_t     flags;        /* must be 0 */
} zk_sha256;
/* the stable sort of 64-byte key records of zk_field_vec_op (described there): its d_a is a HOST pointer to this struct, whose pointers
 * are device pointers */
#define ZK_OP_KEY_SORT 20
typedef struct zk_key_sort {
    const void* d_keys;    /* device: n records of 64 B, 8-byte aligned */
    void*       d_sorted;  /* device, n x 64 B, 8-byte aligned, or NULL: the records in sorted order */
    uint8_t     flags;     /* must be 0 */
} zk_key_sort;
/* the ordering witness of adjacent key records of zk_field_vec_op (described there): its d_a is a HOST pointer to this struct; cols and
 * d_cols are HOST arrays, every other pointer is a device pointer */
#define ZK_OP_KEY_ORDER 22
typedef struct zk_key_col { uint8_t offset; uint8_t width; } zk_key_col;   /* key bytes [offset, offset + width), width 1, 2 or 4 */
typedef struct zk_key_order {
    const void* d_keys;        /* device: n records of 64 B, 8-byte aligned */
    const void* d_perm;        /* device: n x uint32, 4-byte aligned, or NULL; row i is record d_perm[i] (NULL: record i) */
    void*       d_diff;        /* device, n x 32 B Montgomery Fr, or NULL: limb_difference */
    void*       d_index;       /* device, n bytes, or NULL: first_different_limb, 0..31 */
    void*       d_bits;        /* device, 5 x n bytes, or NULL: plane b (n bytes at d_bits + b * n) holds bit (4 - b) of the index */
    void*       d_not_first;   /* device, n bytes, or NULL: index >= group_limbs ? 1 : 0 */
    uint32_t    group_limbs;   /* 0..32; 30 for the state circuit: a difference in RwCounter1 or RwCounter0 alone is not a first access */
    uint32_t    count;         /* gathered columns, at most 64 */
    const zk_key_col* cols;    /* HOST array of count entries */
    void* const* d_cols;       /* HOST array of count device pointers: n cells of cols[j].width bytes, aligned to that width */
    uint8_t     flags;         /* must be 0 */
} zk_key_order;
/* the rows of the bytecode circuit of zk_field_vec_op (described there): its d_a is a HOST pointer to this struct, whose pointers are
 * device pointers; d_bytes, total_bytes, d_offsets, d_lens and index_width are those of zk_keccak */
#define ZK_OP_BYTECODE_ROWS 26
typedef struct zk_bytecode_rows {
    const void* d_bytes;          /* device: the bytes the bytecodes live in */
    uint64_t    total_bytes;      /* bytes readable at d_bytes */
    const void* d_offsets;        /* device: count unsigned little-endian offsets into d_bytes */
    const void* d_lens;           /* device: count unsigned little-endian byte lengths */
    const void* d_hashes;         /* device, count x 32 B Montgomery Fr, or NULL: code hash of each bytecode */
    void* d_tag;                  /* n x 1 B or NULL */
    void* d_index;                /* n x 4 B or NULL */
    void* d_value;                /* n x 4 B or NULL */
    void* d_is_code;              /* n x 1 B or NULL */
    void* d_push_data_left;       /* n x 1 B or NULL */
    void* d_push_data_size;       /* n x 1 B or NULL */
    void* d_length;               /* n x 4 B or NULL */
    void* d_acc_kinds;            /* n x 1 B or NULL: kind column for push_acc (ZK_OP_SCAN_RLC) */
    void* d_rlc_kinds;            /* n x 1 B or NULL: kind column for push_rlc (ZK_OP_SCAN_RLC_REV) */
    uint32_t count;               /* bytecodes */
    uint8_t  index_width;         /* 4 or 8 */
    uint8_t  flags;               /* must be 0 */
} zk_bytecode_rows;
/* the rows of the copy circuit and of the copy table of zk_field_vec_op (described there): d_a is a HOST pointer to a zk_copy_rows
 * (ZK_OP_COPY_ROWS, the integer columns) or a zk_copy_rlc (ZK_OP_COPY_RLC, the challenge-phase columns), whose pointers are device
 * pointers; the first five members of the two structs are the same in name, type and order.  zk_copy_event is the 88-byte
 * little-endian record d_events holds per copy event: device data that the host never reads */
#define ZK_OP_COPY_ROWS 28
#define ZK_OP_COPY_RLC 30
#define ZK_COPY_MEMORY_COPY 1
typedef struct zk_copy_event {
    uint64_t src_addr, src_addr_end, dst_addr;
    uint64_t dst_addr_bias;   /* added (mod 2^64) to the addr column on writer rows only */
    uint64_t rw_counter;      /* rw_counter_start() */
    uint64_t src_off, dst_off, prev_off;   /* offsets into d_bytes of three runs of `length` bytes */
    uint32_t length;          /* full_length(): steps; the event owns 2 * length rows */
    uint32_t src_front, src_back, dst_front, dst_back;   /* masked steps at the front / back of each thread */
    uint8_t  src_tag, dst_tag;   /* CopyDataType: 1 Bytecode, 2 Memory, 3 TxCalldata, 4 TxLog, 5 RlcAcc */
    uint8_t  flags;              /* bit 0 ZK_COPY_MEMORY_COPY: src_id == dst_id and both Memory */
    uint8_t  reserved;           /* 0 */
} zk_copy_event;
typedef struct zk_copy_rows {
    const void* d_events;     /* device: count records of 88 B (zk_copy_event), 8-byte aligned */
    uint32_t    count;
    const void* d_bytes;      /* device: the byte heap */
    uint64_t    total_bytes;  /* below 2^61 */
    uint8_t     flags;        /* must be 0 */
    void* d_is_first;         /* n x 1 B or NULL */
    void* d_is_last;          /* n x 1 B or NULL */
    void* d_tag;              /* n x 1 B or NULL */
    void* d_tag_bits;         /* 3 x n B or NULL: plane b (n bytes at d_tag_bits + b * n) holds bit (2 - b) of the tag */
    void* d_value;            /* n x 1 B or NULL */
    void* d_value_prev;       /* n x 1 B or NULL */
    void* d_mask;             /* n x 1 B or NULL */
    void* d_front_mask;       /* n x 1 B or NULL */
    void* d_word_index;       /* n x 1 B or NULL */
    void* d_src_addr_end;     /* n x 8 B or NULL */
    void* d_is_pad;           /* n x 1 B or NULL */
    void* d_non_pad_non_mask; /* n x 1 B or NULL */
    void* d_real_bytes_left;  /* n x 8 B or NULL */
    void* d_rw_counter;       /* n x 8 B or NULL */
    void* d_rwc_inc_left;     /* n x 8 B or NULL */
    void* d_types;            /* 5 x n B or NULL: planes is_bytecode, is_memory, is_tx_calldata, is_tx_log, is_memory_copy */
    void* d_src_end_rows;     /* n x 1 B or NULL: the d_num of ZK_OP_ROW_INV0 for is_src_end's inverse */
} zk_copy_rows;
typedef struct zk_copy_rlc {
    const void* d_events;     /* device: count records of 88 B (zk_copy_event), 8-byte aligned */
    uint32_t    count;
    const void* d_bytes;      /* device: the byte heap */
    uint64_t    total_bytes;  /* below 2^61 */
    uint8_t     flags;        /* must be 0 */
    const void* d_ids;        /* device, count x 2 x 32 B Montgomery Fr, or NULL: src id, then dst id of each event */
    void* d_id;               /* n x 32 B or NULL */
    void* d_id_other;         /* n x 32 B or NULL */
    void* d_rlc_acc;          /* n x 32 B or NULL */
    void* d_word_rlc;         /* n x 32 B or NULL */
    void* d_word_rlc_prev;    /* n x 32 B or NULL */
} zk_copy_rlc;
/* the rows of the exponentiation circuit and of the exponentiation table of zk_field_vec_op (described there): d_a is a HOST pointer
 * to a zk_exp_rows, whose pointers are device pointers.  zk_exp_event is the 64-byte little-endian record d_events holds per
 * exponentiation event: device data that the host never reads */
#define ZK_OP_EXP_ROWS 32
typedef struct zk_exp_event {
    uint64_t base[4];         /* little-endian 64-bit limbs */
    uint64_t exponent[4];
} zk_exp_event;
typedef struct zk_exp_rows {
    const void* d_events;      /* device: count records of 64 B, 8-byte aligned */
    uint32_t    count;
    uint8_t     flags;         /* must be 0 */
    void* d_is_last;           /* n x 1 B or NULL */
    void* d_base_limb;         /* n x 8 B or NULL */
    void* d_exponent_lo_hi;    /* n x 16 B or NULL */
    void* d_mul_cols;          /* 4 x n x 16 B or NULL: plane c (at + c * n * 16) is mul_gadget col c */
    void* d_mul_u16_64;        /* 4 x n x 2 B or NULL: planes of range_check_64.u16_repr */
    void* d_mul_u16_128;       /* 8 x n x 2 B or NULL */
    void* d_parity_cols;       /* as d_mul_cols */
    void* d_parity_u16_64;     /* as d_mul_u16_64 */
    void* d_parity_u16_128;    /* as d_mul_u16_128 */
    void* d_rows_needed;       /* one uint64_t, 8-byte aligned, or NULL */
} zk_exp_rows;
/* the columns the Poseidon-hash extension adds to the bytecode circuit, and the code-hash rows of the Poseidon table, of
 * zk_field_vec_op (described there): d_a is a HOST pointer to a zk_code_hash_rows (ZK_OP_CODE_HASH_ROWS) or a zk_code_hash_table
 * (ZK_OP_CODE_HASH_TABLE), whose pointers are device pointers; d_bytes, total_bytes, d_offsets, d_lens and index_width are those of
 * zk_keccak and zk_bytecode_rows, the first four members of the two structs are the same in name, type and order */
#define ZK_OP_CODE_HASH_ROWS 34
#define ZK_OP_CODE_HASH_TABLE 36
typedef struct zk_code_hash_rows {
    const void* d_bytes;            /* device: the bytes the bytecodes live in */
    uint64_t    total_bytes;        /* bytes readable at d_bytes; below 2^61 */
    const void* d_offsets;          /* device: count unsigned little-endian offsets into d_bytes */
    const void* d_lens;             /* device: count unsigned little-endian byte lengths */
    void* d_control_length;         /* n x 4 B or NULL */
    void* d_bytes_in_field_index;   /* n x 1 B or NULL */
    void* d_bytes_in_field_inv;     /* n x 32 B Montgomery Fr, 16-byte aligned, or NULL */
    void* d_is_field_border;        /* n x 1 B or NULL */
    void* d_padding_shift;          /* n x 32 B Montgomery Fr, 16-byte aligned, or NULL */
    void* d_field_index;            /* n x 1 B or NULL */
    void* d_field_index_inv;        /* n x 1 B or NULL */
    uint32_t count;                 /* bytecodes */
    uint8_t  index_width;           /* 4 or 8 */
    uint8_t  flags;                 /* must be 0 */
} zk_code_hash_rows;
typedef struct zk_code_hash_table {
    const void* d_bytes;            /* device: the bytes the bytecodes live in */
    uint64_t    total_bytes;        /* bytes readable at d_bytes; below 2^61 */
    const void* d_offsets;          /* device: count unsigned little-endian offsets into d_bytes */
    const void* d_lens;             /* device: count unsigned little-endian byte lengths */
    void* d_input1;                 /* n x 32 B Montgomery Fr, 16-byte aligned, or NULL */
    void* d_control;                /* n x 16 B, 16-byte aligned, or NULL */
    void* d_heading_mark;           /* n x 1 B or NULL */
    void* d_kinds;                  /* n x 1 B or NULL: the kinds column of ZK_OP_POSEIDON */
    void* d_cap;                    /* n x 8 B, 8-byte aligned, or NULL: the d_cap of ZK_OP_POSEIDON */
    void* d_rows_needed;            /* one uint64_t, 8-byte aligned, or NULL */
    uint32_t count;                 /* bytecodes */
    uint8_t  index_width;           /* 4 or 8 */
    uint8_t  flags;                 /* must be 0 */
} zk_code_hash_table;

/* ---- context / memory ----------------------------------------------------------------------- */
int zk_ctx_create(int device, zk_ctx** out);
void zk_ctx_destroy(zk_ctx* ctx);
const char* zk_last_error(const zk_ctx* ctx);
/* Use an existing hipStream_t (e.g. torch.cuda.current_stream().cuda_stream); NULL = own stream */
int zk_ctx_set_stream(zk_ctx* ctx, void* hip_stream);
/* Waits for EVERYTHING this context has enqueued: the library runs on six HIP streams (main, copy, auxiliary transforms,
 * three MSM side streams) and zk_ctx_sync joins all of them, not only the main one -- entry points that return host data
 * (commitments, proofs, downloads) are complete when they return; asynchronous ones (zk_ntt, zk_vec_*, zk_coeff_to_coset ...)
 * are complete after zk_ctx_sync.  A caller-supplied main stream (zk_ctx_set_stream) is synchronised as well. */
int zk_ctx_sync(zk_ctx* ctx);
/* Diagnostics for the contract above: the number of library streams with work still in flight (0 after zk_ctx_sync), and
 * a delay of about `usec` microseconds on one stream (role 0 main, 1 copy, 2 auxiliary, 3..5 MSM side streams). */
int zk_ctx_streams_busy(zk_ctx* ctx, int* busy);
int zk_ctx_debug_delay(zk_ctx* ctx, int role, uint32_t usec);
int zk_buf_alloc(zk_ctx* ctx, size_t bytes, void** d_ptr);
int zk_buf_free(zk_ctx* ctx, void* d_ptr);
/* Page-locked host memory for witness columns: uploads from it run at PCIe speed and overlap with
 * compute (zk_commit_batch_h2d, zk_proof_advice_phase); pageable memory works too, at about half. */
int zk_host_alloc(zk_ctx* ctx, size_t bytes, void** h_ptr);
int zk_host_free(zk_ctx* ctx, void* h_ptr);
/* Page-lock memory the caller already owns (e.g. the Vec<Fr> columns of a witness that is reused
 * across proofs) instead of copying it into zk_host_alloc memory; unregister before freeing it.   */
int zk_host_register(zk_ctx* ctx, void* h_ptr, size_t bytes);
int zk_host_unregister(zk_ctx* ctx, void* h_ptr);
int zk_h2d(zk_ctx* ctx, void* d_dst, const void* h_src, size_t bytes);
int zk_d2h(zk_ctx* ctx, void* h_dst, const void* d_src, size_t bytes);
int zk_d2d(zk_ctx* ctx, void* d_dst, const void* d_src, size_t bytes);
/* HIP-event timing on the context's stream (bench.py's roofline leg) */
int zk_timer_start(zk_ctx* ctx);
int zk_timer_stop_ms(zk_ctx* ctx, float* ms);   /* synchronises on the stop event */

/* Per-kernel HIP-event profiling on the context stream.  While enabled, every named kernel group
 * ("msm_digits", "msm_sort", "msm_buckets", "msm_reduce", "msm_tail_host", "ntt_pass", "ntt_last",
 * ...) is bracketed by an event pair; zk_prof_get drains the stream and returns the accumulated
 * device milliseconds and launch count for one name.  on = 2 records only the groups of the roofline
 * kernels ("msm_buckets", "ntt_*", "quotient*"): every event pair costs a little stream time, and a
 * throughput measurement should carry as few as it needs.
 * The structure-reading commitment paths (csrc/runs.hip) book, at on = 1 only: "runs_prefix_table"
 * (one per build of a basis's prefix-sum table), "runs_collect" (each run-end sweep, the count-only
 * one included), "runs_direct" (run ends summed by double-and-add), "runs_ends_msm" (the bucket
 * method over one column's run ends), "diff_fixed_table" (one per build of the fixed-point table),
 * "diff_mode" (each sampling of the common increment), "diff_sparse" (difference images plus
 * c times the fixed point, one per chunk of columns).                                            */
int zk_prof_enable(zk_ctx* ctx, int on);
int zk_prof_reset(zk_ctx* ctx);
int zk_prof_get(zk_ctx* ctx, const char* name, double* total_ms, uint64_t* count);
/* algorithmic HBM bytes of the launches booked under `name` (scopes that state them: the expression evaluator
 * counts 32 B per row for every distinct (column, rotation) operand, parked intermediate and result); 0 otherwise */
int zk_prof_get_bytes(zk_ctx* ctx, const char* name, uint64_t* bytes);
/* writes a ';'-separated list of the names seen so far into buf */
int zk_prof_names(zk_ctx* ctx, char* buf, size_t len);

/* Self-test of the device's Montgomery products (no reference counterpart: halo2curves' `Fr::mul` has one form; here the device runs
 * generated gfx950 asm -- csrc/mul29_asm.hip.hpp -- and the host / the definition the C forms of csrc/ff29.hip.hpp): `operand_sets`
 * lanes each run mul29 / mul29_ub / sqr29 / mul2add29 in both forms on pseudo-random operands AT the documented lazy-reduction
 * bounds and compare every limb, and so do the evaluator's in-place forms mul29_ipa / mul29_ipb / mul29_ub_ipa / mul2add29_ub_ipa.
 * out3 = {lanes with a difference, OR of the differing routines (1, 2, 4, 8; in-place 16, 32, 64, 128), lanes run}. */
int zk_selftest_products(zk_ctx* ctx, int field, uint32_t operand_sets, uint32_t seed, uint32_t* out3);

/* ---- field vectors (halo2curves Fr/Fq Add/Sub/Mul)  -- SURVEY 8a K4/K10 ------------------------ */
/* d_out = d_a (op) d_b over n Montgomery elements of 32 B, asynchronous on the context's stream; n = 0: ZK_OK.
 * ZK_OP_ADD / ZK_OP_SUB / ZK_OP_MUL are element-wise, over Fr or Fq, and d_out may be d_a or d_b.
 * The two scan ops run a first-order linear recurrence along the column, over Fr only (ZK_FIELD_FQ: ZK_ERR_INVALID_ARG):
 *   ZK_OP_SCAN_AFFINE       out[0]   = b[0],    out[i] = a[i] * out[i-1] + b[i]  for 0 < i < n
 *   ZK_OP_SCAN_AFFINE_REV   out[n-1] = b[n-1],  out[i] = a[i] * out[i+1] + b[i]  for i < n-1
 * The state before the first element is 0, so a[0] (a[n-1] for the reverse op) is never used; a caller with a start value z0
 * folds a * z0 into b[0] itself.  a[i] = 0 starts a new segment at i: a running RLC with resets z[i] = z[i-1] * r * (1 - is_first[i])
 * + x[i] is a = r * (1 - is_first), b = x.  Results are canonical.  d_out must overlap neither d_a nor d_b (n * 32 B each):
 * ZK_ERR_INVALID_ARG, nothing is launched.  Booked under the zk_prof name "fr_scan_affine" with n * 96 algorithmic bytes per call.
 * ZK_OP_ROW_RLC (a #define, value 8; Fr only) is the RLC across the columns of a row, straight from packed typed cells:
 *   d_out[i] = c + sum_j w_j * cell_j[i]  for i < n
 * For this op only, d_a and d_b are HOST pointers: d_a points to a zk_row_rlc {count, d_cols, widths} whose d_cols and widths are
 * host arrays of count entries (d_cols[j] itself is a device pointer), d_b to (count + 1) x 32 B Montgomery Fr in host memory: the
 * constant c, then w_0 .. w_(count-1).  They are read before the call returns; the call is asynchronous on the context's stream.
 * widths[j] in {1, 2, 4, 8, 16}: n little-endian unsigned cells at d_cols[j], aligned to the width, read like zk_fr_from_uint
 * (nothing outside n * width bytes is read); widths[j] = 32: n canonical Montgomery Fr, 8-byte aligned (a word RLC made by an
 * earlier call, say).  Several columns may name the same buffer; count = 0 gives the constant column; n = 0: ZK_OK.  A word RLC of 32
 * byte columns is w_j = r^j; the eleven mixed-width columns of an RwRow under a leading one are c = r^11 with descending powers (or
 * c = 1 with w_j = r^(j+1), the order RwRow::rlc folds in).  Results are canonical.
 * A 32-byte cell that is not canonical (at or above the modulus) gives an undefined VALUE in its row (the one reduction assumes
 * terms below p^2; no memory is touched that would not be otherwise) and no error.
 * d_out (n x 32 B) must not overlap a narrow column; it may BE a 32-byte column (same address: a lane reads its row before it writes
 * it; wherever such columns stand in the table, also past the 64th place, they are taken by the first launch) but not overlap one
 * partially.  ZK_FIELD_FQ, any other width, a NULL or misaligned column, a forbidden overlap, NULL d_cols or
 * widths with count > 0: ZK_ERR_INVALID_ARG before any launch, nothing is written.  64 columns per launch; a longer table runs as
 * further launches that take the sum so far from d_out.  Booked under the zk_prof name "fr_row_rlc" with n * (sum of widths + 32)
 * algorithmic bytes per launch (the sum so far counts as a 32-byte column).
 * ZK_OP_SCAN_RLC and ZK_OP_SCAN_RLC_REV (#defines, values 9 and 10; Fr only) are the RLC ALONG a column, straight from packed typed
 * cells and a one-byte kind column -- Keccak data_rlc, bytecode value_rlc, the copy circuit's reverse rlc_acc:
 *   kind_i = d_kinds ? (d_kinds[i] & 3) : 0      (only the low two bits of the byte are read; the others are ignored)
 *   ZK_OP_SCAN_RLC       out[-1] = z0,  out[i] = m[kind_i] * out[i-1] + w[kind_i] * cell[i]  for 0 <= i < n
 *   ZK_OP_SCAN_RLC_REV   out[n]  = z0,  out[i] = m[kind_i] * out[i+1] + w[kind_i] * cell[i]  for n > i >= 0
 * As for ZK_OP_ROW_RLC, d_a and d_b are HOST pointers for these ops: d_a points to a zk_scan_rlc {d_cells, width, d_kinds} (the two
 * pointers in it are device pointers), d_b to 9 x 32 B Montgomery Fr in host memory: z0, then the table m_0, w_0, m_1, w_1, m_2, w_2,
 * m_3, w_3.  Both are read before the call returns; the call is asynchronous on the context's stream.  The usual table is
 * step (r, 1), start (0, 1), hold (1, 0), clear (0, 0).  width in {1, 2, 4, 8, 16}: n little-endian unsigned cells at d_cells,
 * aligned to the width only, read like zk_fr_from_uint (nothing outside n * width bytes is read); width = 32: n canonical Montgomery
 * Fr, 8-byte aligned -- a non-canonical 32-byte cell gives undefined VALUES from its row on, in scan order, and touches no memory
 * that would not be touched otherwise.  d_kinds: n bytes at any alignment, or NULL (every row kind 0: the plain Horner running RLC);
 * d_cells and d_kinds may name the same or overlapping memory.  Results are canonical.  d_out (n x 32 B) overlaps neither the cells
 * nor the kinds.  ZK_FIELD_FQ, any other width, NULL or misaligned d_cells, a forbidden overlap: ZK_ERR_INVALID_ARG before any
 * launch, nothing is written; the arguments are validated before n is looked at, n = 0 is then ZK_OK.  Booked under the zk_prof
 * name "fr_scan_rlc" with n * (width + (d_kinds ? 1 : 0) + 32) algorithmic bytes per call.
 * ZK_OP_ROW_INV0 (a #define, value 12 -- 11 stays refused, as the tests of the ops above require; Fr only) is the inverse-or-zero
 * witness of a row RLC, straight from packed typed cells -- IsZeroChip's value_inv, IsEqual's inverse of a difference, halo2's
 * Assigned::Rational(num, den).evaluate() with a denominator that is linear in typed cells:
 *   d_out[i] = num[i] * inv0(c + sum_j w_j * cell_j[i])  for i < n,      inv0(0) = 0, inv0(x) = 1/x
 * As for ZK_OP_ROW_RLC, d_a and d_b are HOST pointers, read before the call returns; the call is asynchronous on the context's
 * stream.  d_a points to a zk_row_inv0 {count, d_cols, widths, d_num, num_width}, d_b to (count + 1) x 32 B Montgomery Fr: c, then
 * w_0 .. w_(count-1).  count, d_cols and widths mean exactly what they mean in zk_row_rlc (widths, alignment, nothing outside n *
 * width bytes is read, several columns may name one buffer); count = 0 gives the constant column num[i] * inv0(c).  value_inv of a
 * cell is count = 1, w = 1; IsEqual's inverse is w = (1, -1); the inverse of a cell minus a constant k is c = -k.  d_num = NULL:
 * every numerator is one (num_width is ignored); otherwise a device column of num_width in {1, 2, 4, 8, 16, 32} under the same
 * alignment and read rules.  Results are canonical; a row whose denominator is 0 modulo r gives 0 whatever its numerator.  One
 * inversion serves the 1024 consecutive rows [1024 k, 1024 k + 1024) of a wave: a 32-byte cell, denominator or numerator, that is
 * not canonical gives an undefined VALUE in each of the 1024 rows that share its wave's inversion, touches no memory that would not
 * be touched otherwise, and gives no error.  The overlap rule is ZK_OP_ROW_RLC's: d_out (n x 32 B) overlaps no narrow column; it may BE a
 * 32-byte column, denominator or numerator, at the same address, but not overlap one partially.  ZK_FIELD_FQ, any other width (of
 * a column or of a non-NULL numerator), a NULL or misaligned column, NULL d_cols or widths with count > 0, a forbidden overlap:
 * ZK_ERR_INVALID_ARG before any launch, nothing is written; the arguments are validated before n is looked at, n = 0 is then
 * ZK_OK.  64 columns per launch; a longer table runs as further launches -- the earlier ones are the row RLC into d_out (the sum so
 * far), only the last one inverts, columns that ARE d_out go to the first -- and then d_num may not be d_out (ZK_ERR_INVALID_ARG).
 * Every launch is booked under the zk_prof name "fr_row_inv0" with n * (sum of its widths, the sum so far counting as 32, + num_width
 * on the inverting launch when d_num is given, + 32) algorithmic bytes.
 * ZK_OP_POSEIDON (a #define, value 14 -- 13 stays refused, like 11; Fr only) makes the width-3 Poseidon hash columns of the
 * reference's PoseidonTable -- hash_id, input0, input1 -- from packed typed cells: zktrie's hash_with_domain([a, b], domain), one
 * permutation per row, and the Poseidon code hash, a rate-2 sponge over 31-byte big-endian words with capacity len * 2^64.  The
 * permutation is that of zk_host_poseidon_permute_width3 (x^5, R_F = 8, R_P = 57, the plain round schedule).  As for the other typed
 * ops, d_a and d_b are HOST pointers, read before the call returns; the call is asynchronous on the context's stream.  d_a points to
 * a zk_poseidon {d_in0, d_in1, d_cap, d_kinds, d_word0, d_word1, width0, width1, cap_width, flags} whose pointers are device
 * pointers, d_b to 32 B: one Montgomery Fr cap_scale (2^64 for the code hash, where the capacity cell is the byte length; 1 where it
 * is the zktrie domain).  Widths 1, 2, 4, 8, 16: packed little-endian unsigned cells at stride = width, read exactly like
 * zk_fr_from_uint, aligned to the width, nothing outside n * width bytes is read; 32: canonical Montgomery Fr, 8-byte aligned; 31
 * (width0, width1 only; cap_width = 31 is refused): cell i is the 31 bytes at ptr + 62 * i, BIG-endian, any alignment, exactly those
 * bytes are read -- the rows of unroll_to_hash_input_default: bytecodes laid end to end, each zero-padded to a multiple of 62 bytes,
 * d_in1 = d_in0 + 31.  d_cap = NULL: capacity 0 (cap_width is ignored).  d_kinds: n bytes, any alignment, row kind = d_kinds[i] & 3;
 * NULL: every row is a head.
 *   0 head      s = (cap_scale * cap[i], in0[i], in1[i])
 *   1 continue  s = s'(i-1) + (0, in0[i], in1[i]), s'(i-1) the full three-word state row i-1 left; cap[i] is not read; at row 0 or
 *               behind an off row it continues from the zero state
 *   2, 3 off    the row writes 0 (to d_out and to the word outputs) and ends the message
 * Then s' = permute(s) and d_out[i] = s'[0], canonical Montgomery Fr: the running hash.  With ZK_POSEIDON_FINAL in flags, d_out[i]
 * is the s'[0] of the LAST row of the message row i belongs to, on every row of that message (the table's hash_id).  d_word0 and
 * d_word1 (n x 32 B each, or NULL) receive the Montgomery images of in0[i] and in1[i] (the table's input0, input1).  A 32-byte cell
 * that is not canonical gives an undefined VALUE from its row to the end of its message, touches no memory that would not be touched
 * otherwise, and gives no error.  ZK_FIELD_FQ, any other width, a NULL or misaligned d_in0 or d_in1 (or misaligned d_cap), unknown
 * flag bits, any overlap between an output (d_out, d_word0, d_word1) and any input or another output: ZK_ERR_INVALID_ARG before any
 * launch, nothing is written; the arguments are validated before n is looked at, n = 0 is then ZK_OK.  One lane walks one message;
 * with d_kinds the first rows of the messages are first gathered into a list on the device (no host synchronisation), and more than
 * 2^32 - 1 rows are refused.  Booked under the zk_prof name "fr_poseidon" with n * (width0 + width1 + (d_cap ? cap_width : 0) +
 * (d_kinds ? 1 : 0) + 32 + 32 per word output given) algorithmic bytes per call.
 * ZK_OP_KECCAK (a #define, value 16 -- 15 stays refused, like 11 and 13; Fr only) makes the hash columns of the reference's
 * KeccakTable (zkevm-circuits/src/table.rs: is_final, input_rlc, input_len, output_rlc) from message bytes that live on the device:
 * Keccak-256 (pad byte 0x01, rate 136, the function of zk_host_keccak256) of n messages, one per row, and the two challenge-phase
 * columns.  As for the other typed ops, d_a and d_b are HOST pointers, read before the call returns; the call is asynchronous on the
 * context's stream.  d_a points to a zk_keccak {d_bytes, total_bytes, d_offsets, d_lens, d_digest, d_input_rlc, index_width, flags}
 * whose pointers are device pointers, d_b to 2 x 32 B of Montgomery Fr: r_out (the reference's evm_word challenge), then r_in
 * (keccak_input); r_in is used only when d_input_rlc is given, all 64 bytes are always read.  index_width 4 or 8: d_offsets and
 * d_lens are n unsigned little-endian integers of that width, aligned to it.  Message i is the len_i bytes at d_bytes + off_i;
 * messages may overlap, repeat, and start at any byte address.  For i < n:
 *   digest_i       = Keccak-256 of message i
 *   d_out[i]       = sum_(k<32) digest_i[k] * r_out^(31-k), canonical Montgomery Fr: rlc::value(Word::from_big_endian(digest)
 *                    .to_le_bytes(), evm_word), the table's output_rlc and the Keccak circuit's hash_rlc
 *   d_digest[i]    (n x 32 B at any alignment, or NULL) the 32 digest bytes, in digest order
 *   d_input_rlc[i] (n x 32 B, or NULL) = sum_(k<len) m[k] * r_in^(len-1-k), rlc::value(input.iter().rev(), keccak_input); 0 for the
 *                    empty message
 * The d_lens buffer itself IS the table's input_len column: a 4- or 8-byte typed cell column, ready for
 * zk_proof_advice_phase_typed_dev.  The offsets and lengths are device data that the host never sees: a message with off_i >
 * total_bytes or len_i > total_bytes - off_i (computed so that it cannot wrap) writes 0 to every output of its row and reads nothing,
 * and no error is reported for it, because there is no host synchronisation.  No byte outside [d_bytes, d_bytes + total_bytes) is
 * ever read, whatever the device data hold.  ZK_FIELD_FQ, an index_width other than 4 or 8, NULL or misaligned d_offsets or d_lens,
 * NULL d_bytes with total_bytes > 0, nonzero flags, NULL d_out, d_out or d_input_rlc at an address that is no multiple of 16, any
 * overlap between an output (d_out, d_digest, d_input_rlc) and any input or another output, more rows than one launch grid takes
 * (2^31 - 1 workgroups of 256): ZK_ERR_INVALID_ARG before any launch, nothing is written; the arguments are validated before n is
 * looked at, n = 0 is then ZK_OK.  One lane walks one message, so a wave takes as long as its longest message.  Booked under the
 * zk_prof name "fr_keccak" with n * (2 * index_width + 32 + 32 per optional output given) + total_bytes algorithmic bytes per call:
 * the host cannot know the sum of the lengths, total_bytes stands in for the message bytes read.
 * ZK_OP_SHA256 (a #define, value 18 -- 17 stays refused, like 11, 13 and 15; Fr only) makes the hash columns of the reference's
 * SHA256Table (zkevm-circuits/src/table.rs: is_final, input_rlc, input_len, output_rlc; what the SHA-256 precompile looks up) in the
 * same way: SHA-256 (FIPS 180-4) of n messages, one per row, and the two challenge-phase columns.  d_a is a HOST pointer to a
 * zk_sha256, whose eight members are zk_keccak's in name, type and order {d_bytes, total_bytes, d_offsets, d_lens, d_digest,
 * d_input_rlc, index_width, flags}, d_b a HOST pointer to 2 x 32 B of Montgomery Fr, r_out then r_in, both read before the call
 * returns; r_in is used only when d_input_rlc is given, all 64 bytes are always read.  In the reference BOTH RLCs of this table are
 * taken under keccak_input: a caller that builds the reference's table passes the same challenge twice.  For i < n:
 *   digest_i       = SHA-256 of message i, the len_i bytes at d_bytes + off_i
 *   d_out[i]       = sum_(k<32) digest_i[k] * r_out^(31-k), canonical Montgomery Fr: rlc::value(Word::from_big_endian(output)
 *                    .to_le_bytes(), challenge), the table's output_rlc and the SHA-256 circuit's hashes_rlc
 *   d_digest[i]    (n x 32 B at any alignment, or NULL) the 32 digest bytes in digest order, H0's most significant byte first
 *   d_input_rlc[i] (n x 32 B, or NULL) = sum_(k<len) m[k] * r_in^(len-1-k), rlc::value(input.iter().rev(), challenge); 0 for the
 *                    empty message
 * The d_lens buffer itself IS the table's input_len column, ready for zk_proof_advice_phase_typed_dev.  Every other rule is
 * ZK_OP_KECCAK's: messages may overlap, repeat and start at any byte address; a message with off_i > total_bytes or len_i >
 * total_bytes - off_i (computed so that it cannot wrap) writes 0 to every output of its row and reads nothing, without an error; no
 * byte outside [d_bytes, d_bytes + total_bytes) is ever read; the same arguments are ZK_ERR_INVALID_ARG before any launch with
 * nothing written, validated before n is looked at, n = 0 is then ZK_OK.  One refusal more: total_bytes of 2^61 or above, because a
 * message's length in bits would not fit the 64-bit length field of the padding.  One lane walks one message, so a wave takes as
 * long as its longest message.  Booked under the zk_prof name "fr_sha256" with n * (2 * index_width + 32 + 32 per optional output
 * given) + total_bytes algorithmic bytes per call.
 * ZK_OP_KEY_SORT and ZK_OP_KEY_ORDER (#defines, values 20 and 22 -- 19 and 21 stay refused, like 11, 13, 15 and 17; Fr only) put the
 * rows of the reference's RW table into the state circuit's order and make the ordering witness of adjacent rows, on the device.
 * Both work on n KEY RECORDS of 64 bytes at d_keys (8-byte aligned), compared as big-endian 512-bit integers, byte 0 most significant;
 * limb j (0..31) of a record is the big-endian 16-bit number in bytes 2j, 2j + 1.  The ops give no byte a meaning.  For the state
 * circuit a record is what rw_to_be_limbs packs (state_circuit/lexicographic_ordering.rs): byte 0 zero, 1 tag, 2-5 id (big-endian),
 * 6-25 address, 26 zero, 27 field_tag, 28-59 storage_key (big-endian), 60-63 rw_counter (big-endian); the limb index is then the
 * reference's LimbIndex, Tag = 0, Id1 = 1, ..., RwCounter1 = 30, RwCounter0 = 31.  d_a is a HOST pointer to the descriptor, read
 * before the call returns; the calls are asynchronous on the context's stream and never wait for the device.
 * ZK_OP_KEY_SORT: d_a points to a zk_key_sort {d_keys, d_sorted, flags}; d_b is NULL or a HOST pointer to a 64-byte mask, key byte j
 * takes part in the comparison if and only if mask[j] != 0 (NULL: all 64 take part); d_out is n x 4 B, 4-byte aligned, and d_out[i] is
 * the uint32 index of the record that stands at place i of the order; d_sorted (n x 64 B, 8-byte aligned, or NULL) receives the
 * records themselves in that order.  The sort is stable: records that agree in every compared byte keep their input order, and the
 * result is a pure function of the input (no placement depends on the order in which atomics arrive).  A mask without bytes 60-63
 * gives the reference's sort_by_cached_key(Rw::as_key) over rows handed over in rw_counter order; the full mask gives the same order
 * whenever the counters are distinct.  It is a least-significant-digit radix sort of the permutation, one key byte per pass from byte
 * 63 up to byte 0 over the bytes the mask keeps; a byte position at which all records agree is found on the device and its pass does
 * nothing.  Temporaries (two index buffers and 256 counts per 2048 records) come from the context's scratch, which grows on demand.
 * Booked under the zk_prof name "key_sort" with n * (76 + 14 per kept mask byte + 128 with d_sorted) algorithmic bytes per call: 64 +
 * 4 for the first look at the records, per pass an index and a key byte read twice and an index written, 4 + 4 for d_out, 64 + 64 for
 * d_sorted.
 * ZK_OP_KEY_ORDER: d_a points to a zk_key_order {d_keys, d_perm, d_diff, d_index, d_bits, d_not_first, group_limbs, count, cols,
 * d_cols, flags}; d_b must be NULL; d_out is n x 32 B.  Row i is record d_perm[i] (d_perm NULL: record i).  For 1 <= i < n, with j the
 * first limb at which the records of rows i and i - 1 differ:
 *   d_index[i]     (n bytes, or NULL) = j, the reference's first_different_limb
 *   d_bits         (5 x n bytes, or NULL) plane b, the n bytes at d_bits + b * n, holds bit (4 - b) of j: the BinaryNumberChip's five
 *                  columns, plane 0 the most significant bit (AsBits<5>)
 *   d_diff[i]      (n x 32 B, or NULL) = cur_j - prev_j in Fr, limb_difference; r - d when the rows are out of order
 *   d_out[i]       = d_diff[i]^-1, limb_difference_inverse
 *   d_not_first[i] (n bytes, or NULL) = j >= group_limbs ? 1 : 0; group_limbs 30 gives the state circuit's not_first_access
 * All Fr outputs are canonical Montgomery.  Two equal records give index 31, difference 0, inverse 0 and not_first 1 for group_limbs
 * <= 31, without an error.  Row 0 has no predecessor and writes 0 to every one of these outputs.  d_perm is device data that the host
 * never sees: a row whose index, or whose predecessor's index, is >= n writes 0 to every one of these outputs and reads no record;
 * nothing outside [d_keys, d_keys + 64 n) is ever read.  The gathered columns: cols and d_cols are HOST arrays of count <= 64 entries;
 * cell i of column c is the big-endian integer of key bytes [cols[c].offset, cols[c].offset + cols[c].width) of row i's record, stored
 * little-endian at width (1, 2 or 4) bytes at d_cols[c], a typed cell column ready for zk_proof_advice_phase_typed_dev.  Row 0 is
 * included; a row whose own index is >= n writes 0.  The inverse is a lookup in the inverses of 1..65535, which the context makes on
 * the device at the first call and keeps (2 MB).  Booked under the zk_prof name "key_order" with n * (192 + 8 with d_perm + 32 with
 * d_diff + 1 with d_index + 5 with d_bits + 1 with d_not_first + the sum of the column widths) algorithmic bytes per call.
 * For both ops ZK_FIELD_FQ, nonzero flags, NULL d_a, d_keys or d_out, a misaligned pointer (d_keys, d_sorted 8; d_out of the sort and
 * d_perm 4; d_out of the order and d_diff 16; a gathered column its width), n >= 2^32, a zk_key_col with a width other than 1, 2 or 4
 * or offset + width > 64, count > 64, NULL cols or d_cols with count > 0, a NULL entry of d_cols, group_limbs > 32, a non-NULL d_b for
 * ZK_OP_KEY_ORDER, any overlap between an output and any input or another output (d_sorted may not be d_keys): ZK_ERR_INVALID_ARG
 * before any launch, nothing is written; the arguments are validated before n is looked at, n = 0 is then ZK_OK.
 * ZK_OP_BYTECODE_ROWS (a #define, value 26 -- 23, 24, 25 and 27 stay refused; Fr only) makes the rows of the reference's bytecode
 * circuit (bytecode_circuit/bytecode_unroller.rs unroll_with_codehash, circuit.rs assign_bytecode and set_padding_row) from code bytes
 * that live on the device.  d_a is a HOST pointer to a zk_bytecode_rows {d_bytes, total_bytes, d_offsets, d_lens, d_hashes, d_tag,
 * d_index, d_value, d_is_code, d_push_data_left, d_push_data_size, d_length, d_acc_kinds, d_rlc_kinds, count, index_width, flags},
 * d_b a HOST pointer to 32 B, one Montgomery Fr empty_hash (the code hash of the padding rows: POSEIDON_CODE_HASH_EMPTY, or the RLC
 * of EMPTY_CODE_HASH_LE), both read before the call returns; the call is asynchronous on the context's stream and never waits for
 * the device.  d_bytes, total_bytes, d_offsets, d_lens and index_width mean exactly what they mean in zk_keccak, with count entries:
 * one set of device buffers feeds this op, the code hash (ZK_OP_POSEIDON) and ZK_OP_KECCAK.  Bytecode b of L_b = len_b bytes B owns
 * the L_b + 1 consecutive rows from start_b = sum_(c<b) (L_c + 1); with P(v) = v - 0x5f for 0x60 <= v <= 0x7f and 0 otherwise:
 *   header row start_b           tag 0, index 0, value L_b, is_code 0, push_data_left 0, push_data_size 0, length L_b
 *   byte row start_b + 1 + p     tag 1, index p, value B[p], length L_b, push_data_size P(B[p]) (data bytes included),
 *                                push_data_left s_p with s_0 = 0 and s_(p+1) = s_p == 0 ? P(B[p]) : s_p - 1, is_code = (s_p == 0)
 *   padding rows, up to n        every typed output 0 (tag 0 is Header)
 *   d_out[i]       (n x 32 B) d_hashes[b] on every row of bytecode b (0 there when d_hashes is NULL), empty_hash on padding rows
 *   d_acc_kinds[i] 1 on a data row (tag 1 and push_data_left > 0), else 0: ZK_OP_SCAN_RLC over the value column with z0 = 0 and the
 *                  table {0: (0, 0), 1: (r, 1)} is push_acc
 *   d_rlc_kinds[i] 1 on the last data row of an instruction (a data row with push_data_left == 1 or index == length - 1), 2 on every
 *                  other data row and on a code row with push_data_size > 0 and index < length - 1, else 0: ZK_OP_SCAN_RLC_REV over
 *                  the push_acc column with z0 = 0 and the table {0: (0, 0), 1: (0, 1), 2: (1, 0)} is push_rlc
 * Each typed output may be NULL.  The cells are little-endian at the width the struct names (value and length hold L mod 2^32),
 * aligned to it -- the 1-byte columns at any address --, ready for zk_proof_advice_phase_typed_dev.  Rows at or after n are not
 * written: a bytecode that does not fit is cut there without an error (the reference returns Error::Synthesis), and the kinds of the
 * cut instruction then describe a push_rlc nobody should use.  The offsets and lengths are device data that the host never sees: an
 * entry with off > total_bytes or len > total_bytes - off (computed so that it cannot wrap) counts as an empty bytecode everywhere in
 * this op and reads nothing; no byte outside [d_bytes, d_bytes + total_bytes) is ever read.  start_b is exact while it is <= n and
 * saturates there.  Bytecodes may overlap, repeat, and start at any address; the result is a pure function of the input.  No lane
 * walks a bytecode: the work is laid out by rows.  start is a device scan into the context's scratch; push_data_left is a state in
 * 0..32 whose 33-entry transition maps are made per tile of 1024 rows, composed up a 64-ary hierarchy and pushed down again, so a
 * single long bytecode costs what many short ones cost.  Stages whose outputs are all NULL are not launched: a call with only
 * d_hashes and d_out (the second call of a Keccak-code-hash build, in the challenge phase) never reads d_bytes.  ZK_FIELD_FQ, an
 * index_width other than 4 or 8, nonzero flags, NULL or misaligned d_offsets or d_lens with count > 0, NULL d_bytes with total_bytes
 * > 0, d_hashes at an address that is no multiple of 8, d_out at one that is no multiple of 16, d_index, d_value or d_length at one
 * that is no multiple of 4, n >= 2^32, total_bytes >= 2^61, any overlap between an output and any input or another output:
 * ZK_ERR_INVALID_ARG before any launch, nothing is written; the arguments are validated before n is looked at, n = 0 is then ZK_OK.
 * Booked under the zk_prof name "bytecode_rows" with count * (2 * index_width + 32 with d_hashes) + total_bytes (only if an output
 * reads the bytes) + n * (32 + the widths of the outputs given) algorithmic bytes per call.
 * ZK_OP_COPY_ROWS and ZK_OP_COPY_RLC (#defines, values 28 and 30 -- 27 and 29 stay refused; Fr only) make the rows of the reference's
 * copy circuit and copy table (table.rs CopyTable::assignments, copy_circuit.rs assign_copy_event and assign_padding_row) from one
 * zk_copy_event record per copy event and the byte heap, both on the device: ZK_OP_COPY_ROWS the integer columns as typed cells ready
 * for zk_proof_advice_phase_typed_dev, ZK_OP_COPY_RLC the challenge-phase columns.  d_a is a HOST pointer to a zk_copy_rows or a
 * zk_copy_rlc, read before the call returns; the first five members {d_events, count, d_bytes, total_bytes, flags} are the same in
 * both; the calls are asynchronous on the context's stream and never wait for the device.  A zk_copy_event {src_addr, src_addr_end,
 * dst_addr, dst_addr_bias, rw_counter, src_off, dst_off, prev_off, length, src_front, src_back, dst_front, dst_back, src_tag,
 * dst_tag, flags, reserved} is 88 little-endian bytes of device data that the host never reads: the run at src_off is the reader's
 * bytes (copy_bytes.bytes), the run at dst_off the writer's (aux_bytes, else src_off again), the run at prev_off bytes_write_prev
 * (else dst_off again), each of length bytes; dst_addr_bias carries build_tx_log_address, (TxLogFieldTag::Data << 32) + (log_id << 48)
 * for a log and 0 otherwise; the masks are counts of masked steps at the front and at the back of each thread, which is all that the
 * circuit's constrain_mask allows.  Event e of L = length steps owns the 2 L rows from start_e = sum_(c<e) 2 L_c; row j of it is step
 * s = j >> 1 of thread t = j & 1 (0 the reader, 1 the writer).  With (f, b) the front and back counts of the thread -- a thread whose
 * masks cover the whole event, f + b >= L, keeps front_mask = 1 and never advances its address: (f, b) := (L, 0) --, R = (src_tag ==
 * 2), W = (dst_tag == 2 or 4), delta = (R + W) (L / 32), cl = max(L - src_front - src_back, 0), q = s / 32, adv = max(0, s - f):
 *   is_first, is_last            j == 0, j == 2 L - 1
 *   tag, d_tag_bits, d_types     src_tag on reader rows, dst_tag on writer rows; the three planes of n bytes hold bit 2, 1, 0 of it; the
 *                                five planes tag == 1, tag == 2, tag == 3, tag == 4 and ZK_COPY_MEMORY_COPY (both rows)
 *   value, value_prev            d_bytes[src_off + s] (reader) or d_bytes[dst_off + s] (writer); value (reader) or d_bytes[prev_off + s]
 *   mask, front_mask             s < f or s >= L - b;  s < f
 *   word_index                   s mod 32
 *   addr (d_out, n x 8 B)        src_addr + adv (reader), dst_addr + adv + dst_addr_bias (writer), mod 2^64
 *   src_addr_end                 src_addr_end (reader), dst_addr + L (writer)
 *   is_pad, non_pad_non_mask     reader only: src_addr + adv >= src_addr_end;  !is_pad && !mask
 *   real_bytes_left              cl - min(adv, L - f - b), mod 2^64
 *   rw_counter, rwc_inc_left     memory copy: rw_counter + q and delta - q (reader), rw_counter + delta / 2 + q and delta - delta / 2 - q
 *                                (writer); otherwise, with inc = q (R + W) + (t == 1 && s mod 32 == 31 ? R : 0): rw_counter + inc, delta - inc
 *   d_src_end_rows               1 on reader rows and on padding rows, the rows on which the reference assigns is_src_end's inverse:
 *                                the d_num of ZK_OP_ROW_INV0 over (addr, src_addr_end)
 * The rows from start_count up to n are padding rows: is_last = i & 1, src_addr_end = 1, mask = front_mask = d_src_end_rows = 1, every
 * other typed output 0 (tag 0 is Padding).  Each typed output may be NULL; 1-byte columns and planes may stand at any address, 8-byte
 * columns at a multiple of 8.  ZK_OP_COPY_ROWS takes no second operand: d_b must be NULL.
 * ZK_OP_COPY_RLC: d_b is a HOST pointer to 2 x 32 B, Montgomery Fr r_word (evm_word) then r_in (keccak_input), all 64 bytes read
 * before the call returns.  Every output is n x 32 B canonical Montgomery Fr at a multiple of 16, d_out is value_acc, the others may
 * be NULL.  With A_t(-1) = 0, and W_t and V reset to 0 at every s mod 32 == 0:
 *   value_acc (d_out)            A_t(s) = mask ? A_t(s - 1) : A_t(s - 1) r_in + (is_pad ? 0 : value)
 *   d_word_rlc                   W_t(s) = W_t(s - 1) r_word + value
 *   d_word_rlc_prev              W_0(s) on reader rows; on writer rows V(s) = V(s - 1) r_word + value_prev
 *   d_rlc_acc                    on every row of the event A_1(L - 1) if src_tag == 5 or dst_tag == 5 or dst_tag == 1, else 0; 0 for an
 *                                event cut at n.  This is the value constrain_event_rlc_acc forces; it equals the reference's sum over
 *                                the reader's unmasked bytes whenever the writer's run and masks are the reader's, which holds for every
 *                                event with an RLC that the reference builds
 *   d_id, d_id_other             d_ids[2 e + t], d_ids[2 e + 1 - t] (d_ids: count x 2 x 32 B Montgomery Fr at a multiple of 8, the src id
 *                                then the dst id of each event as number_or_hash_to_field gives them; NULL: 0 for both).  ZK_OP_ROW_INV0
 *                                over (id, id_other) with the weights (1, -1) is the is_id_unchange inverse of every row
 * On padding rows every output is 0 except id_other, which is 1 (that inverse is -1 there).  An event counts as an empty event
 * everywhere in both ops and reads nothing when a tag lies outside 1..5, reserved is nonzero, flag bits other than bit 0 are set or one
 * of its three runs does not lie inside [0, total_bytes) (off > total_bytes or length > total_bytes - off: it cannot wrap).  Rows at
 * or after n are not written: an event that does not fit is cut there without an error.  start_e is exact while it
 * is <= n and saturates there.  No byte outside the two input buffers is ever read, whatever the device data hold; runs may overlap
 * and repeat; the result is a pure function of the input.  No lane walks an event: the work is laid out by rows.  start is a device
 * scan into the context's scratch; ZK_OP_COPY_ROWS evaluates the closed forms above per tile of 1024 rows; value_acc is an affine scan
 * in step space that carries both threads (a masked step is the identity map, an event's first step a constant map, so no segment
 * flags), the word RLCs look at most 31 steps back, rlc_acc and the ids are gathers behind the scan.  Stages whose outputs are all
 * NULL are not launched; ZK_OP_COPY_ROWS without d_value and d_value_prev never reads d_bytes.  ZK_FIELD_FQ, nonzero descriptor flags,
 * NULL or misaligned (8) d_events with count > 0, NULL d_bytes with total_bytes > 0, total_bytes >= 2^61, n >= 2^32, a misaligned
 * output or d_ids, a non-NULL d_b for ZK_OP_COPY_ROWS, any overlap between an output and any input or another output:
 * ZK_ERR_INVALID_ARG before any launch, nothing is written; the arguments are validated before n is looked at, n = 0 is then ZK_OK.
 * Booked under the zk_prof names "copy_rows" with count * 88 + total_bytes (only with d_value or d_value_prev) + n * (8 + the widths of
 * the outputs given; d_tag_bits 3, d_types 5) and "copy_rlc" with count * (88 + 64 with d_ids) + total_bytes + n * 32 * (1 + the outputs
 * given) algorithmic bytes per call.
 * ZK_OP_EXP_ROWS (#define, value 32 -- 31 stays refused; Fr only) makes the rows of the reference's exponentiation circuit and
 * exponentiation table (exp_circuit.rs assign_exp_events, table.rs ExpTable::assignments, gadgets MulAddChip::assign and
 * UIntRangeCheckChip::assign) from one zk_exp_event {base[4], exponent[4]} per event, 64 little-endian bytes of device data that the
 * host never reads: every cell is an integer of at most 128 bits, written as a typed cell ready for zk_proof_advice_phase_typed_dev.
 * d_a is a HOST pointer to a zk_exp_rows, read before the call returns; d_b must be NULL; the call is asynchronous on the context's
 * stream and never waits for the device.  d_out is exponentiation_lo_hi, n x 16 B at a multiple of 16; every other output may be
 * NULL, 16-byte cells at a multiple of 16, d_base_limb at one of 8, the u16 planes at one of 2, d_is_last anywhere.  An event with
 * exponent x < 2 has no steps and no rows; otherwise it has S = (bitlen(x) - 1) + (popcount(x) - 1) <= 510 steps of 8 rows from
 * start_e = sum_(c<e) 8 S_c, in the reference's reversed order (exp_by_squaring's steps, last first), all products mod 2^256.  With
 * P(i) = i + popcount(x mod 2^i) and i the largest index with P(i) <= j, step j holds x_j = x >> i, bit 0 cleared when j - P(i) == 1,
 * d_j = base^(x_j); x_j odd: a_j = base^(x_j - 1), b_j = base; x_j even: a_j = b_j = base^(x_j / 2).  The rows of step j at row o:
 *   d_is_last                    1 on row o of step S - 1, else 0
 *   d_base_limb                  the 64-bit limbs 0..3 of base on rows o .. o + 3, 0 on rows o + 4 .. o + 7
 *   d_exponent_lo_hi, d_out      the low and the high 128 bits of x_j, of d_j, on rows o and o + 1, 0 below
 *   d_mul_cols, d_parity_cols    MulAddChip::assign of [a_j, b_j, 0, d_j] and of [2, x_j >> 1, x_j & 1, x_j]: plane c (n x 16 B at
 *                                + c * n * 16) is the chip's col c.  Row o: the 64-bit limbs of a; o + 1: of b; o + 2: c_lo, c_hi,
 *                                d_lo, d_hi; o + 3 and col 0 of o + 4: the five u16 digits of carry_lo = (t0 + t1 2^64 + c_lo - d_lo)
 *                                >> 128; o + 5 and col 0 of o + 6: of carry_hi = (t2 + t3 2^64 + c_hi + carry_lo - d_hi) >> 128, with
 *                                t_k = sum_(i<=k) a_i b_(k-i); every other cell 0
 *   d_*_u16_64                   range_check_64.u16_repr: plane c (n x 2 B at + c * n * 2) holds digit c of a_0 .. a_3, b_0 .. b_3 on
 *                                rows o .. o + 7
 *   d_*_u16_128                  range_check_128.u16_repr: plane c of eight holds digit c of c_lo, c_hi, d_lo, d_hi on rows o .. o + 3,
 *                                0 below
 * Behind the events' rows the default event (base 2, exponent 2: one step, a = b = 2, d = 4, is_last = 1) is repeated while
 * offset + 8 <= n - 10, and every row behind that is 0 in every output; n is the caller's max_exp_rows, need not be a multiple of 8
 * and may be below 10 (all zeros).  Where the reference asserts that the events fit, the op writes whole steps only: a step whose 8
 * rows do not lie below n - 10 is not written and neither is anything behind it, zeros take over.  d_rows_needed, one uint64_t on the
 * device at a multiple of 8 or NULL, receives 8 sum S + 10, exact and unsaturated, for the caller to compare with n later; start_e is
 * exact while it is <= n and saturates there.  The fixed columns q_enable, is_step and is_final_step are key material, constant for
 * a given n, and not part of the op; the u16 cells are in range by construction.  No lane walks an event to find x_j, a_j or b_j:
 * start is a device scan into the context's scratch, one lane per event runs the chain d_(S - 1) .. d_0 of truncated multiplies into
 * (n / 8 + 1) x 32 B of scratch, and the rows are closed forms per tile of 1024 rows.  No atomics; no byte outside d_events is read
 * whatever the records hold; the result is a pure function of the input.  ZK_FIELD_FQ, nonzero flags, NULL or misaligned (8)
 * d_events with count > 0, n >= 2^32, a misaligned output, a non-NULL d_b, any overlap of an output with the events or another
 * output: ZK_ERR_INVALID_ARG before any launch, nothing is written; the arguments are validated before n is looked at, n = 0 is then
 * ZK_OK and writes nothing, d_rows_needed included.  Booked under the zk_prof name "exp_rows" with count * 64 + n * (16 + the widths of the outputs given: 1, 8, 16, 64, 8, 16,
 * 64, 8, 16) algorithmic bytes per call; inside it k_exp_chain and k_exp_rows are timed on their own under "exp_rows_chain" and
 * "exp_rows_tiles", with no bytes.
 * ZK_OP_CODE_HASH_ROWS and ZK_OP_CODE_HASH_TABLE (#defines, values 34 and 36 -- 33 and 35 stay refused; Fr only) make, from the code
 * bytes ZK_OP_KECCAK and ZK_OP_BYTECODE_ROWS read, the eight advice columns that the Poseidon-hash extension adds to the bytecode
 * circuit (bytecode_circuit/circuit/to_poseidon_hash.rs assign_extended_row, set_header_row) and the code-hash rows of the Poseidon
 * table (table.rs PoseidonTable::dev_load over unroll_to_hash_input_default) in the shape ZK_OP_POSEIDON reads.  d_a is a
 * HOST pointer to a zk_code_hash_rows or a zk_code_hash_table, read before the call returns; d_b must be NULL; the calls are asynchronous
 * on the context's stream, never wait for the device and allocate nothing once the context's scratch has grown to the size of the
 * call.  d_bytes, total_bytes, d_offsets, d_lens and index_width mean exactly what they mean in zk_keccak and zk_bytecode_rows,
 * with count entries and the same rule: an entry with off > total_bytes or len > total_bytes - off is an empty bytecode, and no
 * byte outside [d_bytes, d_bytes + total_bytes) -- indeed none outside a bytecode's own [off, off + len) -- is ever read.  With L
 * the length of a bytecode and B its bytes, 31 = HASHBLOCK_BYTES_IN_FIELD bytes to a field and two fields to a block:
 * ZK_OP_CODE_HASH_ROWS works in the row space of ZK_OP_BYTECODE_ROWS: bytecode b owns the L_b + 1 rows from start_b = sum_(c<b)
 * (L_c + 1), the scan saturates at n, a bytecode that does not fit is cut at n without an error, rows at or after n are not written.
 *   header row of b              control_length L, field_input 0, bytes_in_field_index 0, bytes_in_field_inv 0, is_field_border 0,
 *                                padding_shift 256^31, field_index 1, field_index_inv 0 (the reference's set_header_row, although
 *                                1 / (2 - 1) = 1)
 *   byte row p, m = p mod 31     control_length L - 62 (p div 62), field_input sum_(t=0..m) B[p - m + t] 256^(30 - t),
 *                                bytes_in_field_index m + 1, bytes_in_field_inv 1 / (30 - m) or 0, is_field_border (m == 30 or
 *                                p + 1 == L), padding_shift 256^(30 - m), field_index (p div 31) mod 2 + 1, field_index_inv
 *                                1 - (p div 31) mod 2
 *   padding rows, up to n        a header row of length 0
 * field_input is d_out, n x 32 B canonical Montgomery Fr at a multiple of 16, as are d_bytes_in_field_inv and d_padding_shift;
 * d_control_length is n x 4 B (L mod 2^32, as the bytecode op's length) at a multiple of 4; the four 1-byte columns stand at any
 * address; every typed output may be NULL, and the typed cells are ready for zk_proof_advice_phase_typed_dev.
 * ZK_OP_CODE_HASH_TABLE works in the row space of the table: bytecode b owns the K_b = ceil(L_b / 62) rows from tstart_b = sum_(c<b)
 * K_c -- an empty bytecode owns none --, under the same saturating scan.  Row j of b:
 *   d_out, d_input1              n x 32 B Montgomery Fr at a multiple of 16: the big-endian integers of B[62 j .. 62 j + 31) and
 *                                B[62 j + 31 .. 62 j + 62), bytes at or behind L read as 0 (and are not read from memory)
 *   d_control                    n x 16 B little-endian at a multiple of 16: (L - 62 j) 2^64 = HASHABLE_DOMAIN_SPEC * control_len,
 *                                the low eight bytes 0
 *   d_heading_mark, d_kinds      n x 1 B each: j == 0; 0 on j == 0 and 1 otherwise, the head and continue kinds of ZK_OP_POSEIDON
 *   d_cap                        n x 8 B at a multiple of 8: L
 * The rows from sum K_b up to n hold 0 in every output and kind 2 (off).  d_rows_needed, one uint64_t on the device at a multiple
 * of 8 or NULL, receives the unsaturated sum K_b: one store, no atomics.  The reference's two leading table rows are the caller's
 * pointer offset; domain_spec is always 0 and not written.  ZK_OP_POSEIDON over d_out and d_input1 with width0 = width1 = 32, d_cap
 * with cap_width = 8, cap_scale = 2^64, d_kinds and ZK_POSEIDON_FINAL gives the table's hash_id with no host re-packing.
 * No lane walks a bytecode: the starts are a device scan (that of ZK_OP_BYTECODE_ROWS) into a scratch slot of the two ops' own, a
 * workgroup takes a tile of 1024 rows and finds the bytecodes of its first and last row by one search each, each lane its own inside
 * that window; a field's bytes come as up to nine aligned dwords per lane, single bytes at the two ends of a bytecode; the powers
 * of 256 and the inverses of 1 .. 30 are compile-time constants.  No atomics; the result is a pure function of the input.  For both
 * ops ZK_FIELD_FQ, nonzero flags, a non-NULL d_b, an index_width other than 4 or 8, NULL or misaligned d_offsets or d_lens with
 * count > 0, NULL d_bytes with total_bytes > 0, an output at an address that is no multiple of its alignment above, n >= 2^32,
 * total_bytes >= 2^61, any overlap between an output and any input or another output: ZK_ERR_INVALID_ARG before any launch, nothing
 * is written; the arguments are validated before n is looked at, n = 0 is then ZK_OK and writes nothing, d_rows_needed included.
 * Booked under the zk_prof names "code_hash_rows" and "code_hash_table" with count * 2 * index_width + total_bytes + n * (32 + the
 * widths of the outputs given) algorithmic bytes per call, + 8 with d_rows_needed.
 * Other op values (5, 6, 7, 11, ...) are refused. */
int zk_field_vec_op(zk_ctx* ctx, int field, int op, const void* d_a, const void* d_b, void* d_out, size_t n);
/* out[i] = a[i] * s  (s: host pointer to one element) */
int zk_fr_scale(zk_ctx* ctx, void* d_a, const void* h_s, size_t n);
/* d_out[i] = Montgomery Fr of the unsigned little-endian integer d_packed[i] (width_bytes = 1, 2, 4, 8 or 16), i < n.
 * d_packed: n * width_bytes bytes, aligned to width_bytes.  d_out: n * 32 B, must not overlap d_packed.
 * Asynchronous on the context's stream like zk_fr_scale.  Any other width, or a misaligned pointer: ZK_ERR_INVALID_ARG.
 * Booked under the zk_prof name "fr_from_uint" with n * (width_bytes + 32) algorithmic bytes per launch.
 * A witness whose packed cells are already on the device (produced by another kernel) becomes an advice column by this call
 * followed by zk_proof_advice_phase_dev; host columns of packed cells go to zk_proof_advice_phase_typed. */
int zk_fr_from_uint(zk_ctx* ctx, const void* d_packed, uint32_t width_bytes, size_t n, void* d_out);
/* zk_fr_from_uint for several columns at once: count columns of n cells each; widths[j] in {1,2,4,8,16}; d_packed[j] aligned to
 * widths[j]; d_out[j] n x 32 B Montgomery Fr.  Asynchronous on the context's stream like zk_fr_from_uint; 16 columns per launch (a
 * workgroup works on one column, so one call may mix widths).  Outputs must not overlap each other or any input; several columns may
 * read the same packed cells.  Any other width, a misaligned or NULL pointer: ZK_ERR_INVALID_ARG and nothing is written.
 * count = 0: ZK_OK.  Booked under the zk_prof name "fr_from_uint_batch", per launch, with the sum of n * (widths[j] + 32) bytes. */
int zk_fr_from_uint_batch(zk_ctx* ctx, const void* const* d_packed, const uint8_t* widths, size_t count, size_t n, void* const* d_out);
/* ff::BatchInvert semantics (zeros stay zero), in place -- SURVEY 8a K12 */
int zk_fr_batch_invert(zk_ctx* ctx, void* d_a, size_t n);

/* ---- NTT: halo2_proofs::arithmetic::best_fft / poly::EvaluationDomain  -- SURVEY 8a K2, K3 ---- */
/* In-place size-2^log_n transform over <omega>, natural order in and out:
 *   out[i] = sum_j a[j] * omega^(i*j),   omega = ROOT_OF_UNITY^(2^(28-log_n))   (inverse = 0)
 *   inverse = 1: omega^-1 and the 1/n scale, i.e. EvaluationDomain::lagrange_to_coeff.          */
int zk_ntt(zk_ctx* ctx, void* d_data, uint32_t log_n, int inverse);
/* zk_ntt over `count` columns of the same size, in place, several columns per launch. */
int zk_ntt_batch(zk_ctx* ctx, void* const* d_datas, size_t count, uint32_t log_n, int inverse);
/* best_fft with an arbitrary primitive 2^log_n-th root (h_omega: one Fr), no scaling.  The root is not checked.  For a root
 * that is not primitive (omega^n = 1 but omega^(n/2) != -1) the result is best_fft's, bit for bit, and NOT the sum above:
 * like best_fft's, the butterflies subtract where the sum multiplies by omega^(n/2), so
 *   out[i] = sum_j (-1)^c a[j] omega^(i*j - c*n/2),   c = sum_s bit_s(i) * bit_(log_n-1-s)(j).
 * Every distinct root gets a domain (twiddle tables) of its own in the context's cache.            */
int zk_ntt_omega(zk_ctx* ctx, void* d_data, uint32_t log_n, const void* h_omega);
/* Host only (no context, no device): the launches of one launch group of a transform of `columns` columns of 2^log_n elements
 * (1 <= log_n <= 28), as zk_ntt_batch / zk_coeff_to_coset_batch / ... decide them under the ZK_NTT_* knobs in force at the call.
 * tables: the domain has its inter-pass twiddle tables (a domain built under ZK_NTT_OUT_TABLE=0 has none; no domain above 2^24 or
 * of a single pass has any, whatever is passed).  It states what the domain IS: ZK_NTT_OUT_TABLE, which only acts when a domain
 * is built and leaves a cached one as it is, is deliberately not consulted -- pass tables = 0 for a domain built under it.  coset_pass: a coset shift runs as a pass of its own (zk_coeff_to_extended,
 * zk_extended_to_coeff), which is per column.
 * out_head[4]: columns per launch group, columns in the first group (what the records describe), passes, tables in effect.
 * The records are those of a FULL group (the first); a call whose column count is no multiple of the group size ends with a
 * smaller group, whose plans are those of a call with that many columns (17 columns in groups of 16: ask for 1 as well).
 * out_records: ZK_NTT_PLAN_WORDS words per launch, in launch order -- kind (0 strided pass, 1 last pass), pass index, passes,
 * log2 of the digit, log2 of the digit's stride, log2 of the runs / rows per workgroup, workgroups per column, grid x, grid y,
 * threads, dynamic LDS bytes, 1 for a compile-time instance (0: the run-time kernel), XCD-aware numbering on, log2 of the tiles
 * grouped per 128-byte line.  *out_launches: the number of launches; out_records may be NULL with cap_records (in records) = 0.
 * Not in the plan, because only a device decides them: fewer columns per launch when scratch memory is short, tables that found
 * no memory, and the run-time kernel taken when the device refuses an instance's LDS size.                                    */
#define ZK_NTT_PLAN_WORDS 14
int zk_host_ntt_plan(uint32_t log_n, size_t columns, int tables, int coset_pass, uint32_t* out_head, uint32_t* out_records, size_t cap_records, uint32_t* out_launches);
/* ONE transform of size 2^log_n spread over `world` contexts, one per GPU (the
 * 4-step split with a single all-to-all).  On entry rank r holds the residue class
 * x[r + world * i], i < m = 2^log_n / world, in d_local; on return d_local[j1 * (m / world) + c]
 * = X[(r * (m / world) + c) + m * j1]: every rank owns the outputs whose index mod m falls in its
 * slice.  exchange(user, d_send, bytes_per_peer, d_recv) is an all-to-all of DEVICE buffers:
 * block p of d_send goes to rank p, block p of d_recv comes from rank p (RCCL all_to_all_single
 * over xGMI, see zkevm-circuits_amd/sharding.py); it must return 0 with d_recv complete.
 * world: power of two <= 16, 2^log_n >= world^2.  inverse = 1 applies omega^-1 and 1/n.
 * exchange == NULL: the context's own RCCL communicator does the all-to-all (zk_comm_init), with
 * no host synchronisation between the local transform, the exchange and the cross butterflies.
 * Worth it only for transforms far above 2^24: a 2^20 NTT takes 0.12 ms on one GPU.             */
typedef int (*zk_alltoall_fn)(void* user, const void* d_send, size_t bytes_per_peer, void* d_recv);
int zk_ntt_sharded(zk_ctx* ctx, void* d_local, uint32_t log_n, int inverse, uint32_t rank, uint32_t world, zk_alltoall_fn exchange, void* user);
/* EvaluationDomain::coeff_to_extended: d_coeffs (2^k) -> d_out (2^ext_k): scale by zeta^i,
 * zero-pad, NTT over the extended domain.                                                       */
int zk_coeff_to_extended(zk_ctx* ctx, const void* d_coeffs, uint32_t k, uint32_t ext_k, void* d_out);
/* One coset of the extended domain (EvaluationDomain::coeff_to_extended_part): d_out[i] =
 * f(g * omega^i) for i < 2^k, f given by 2^k coefficients; h_g is one Fr.  The extended domain of
 * halo2 is the union of the cosets g_r = zeta * omega_ext^r, r < 2^(ext_k-k): extended index
 * i * 2^(ext_k-k) + r  <->  element i of coset r.  d_out may alias d_coeffs.                       */
int zk_coeff_to_coset(zk_ctx* ctx, const void* d_coeffs, uint32_t k, const void* h_g, void* d_out);
/* The same for `count` polynomials on one coset, several columns per launch (the quotient reads hundreds of
 * columns on every coset; below 2^20 rows one column does not fill the device). */
int zk_coeff_to_coset_batch(zk_ctx* ctx, const void* const* d_coeffs, uint32_t k, const void* h_g, void* const* d_outs, size_t count);
/* d_dst[i * stride + offset] = d_src[i] * scale, i < n: interleaves coset values into extended order */
int zk_fr_scatter_scaled(zk_ctx* ctx, const void* d_src, size_t n, const void* h_scale, void* d_dst, size_t stride, size_t offset);
/* EvaluationDomain::extended_to_coeff: inverse NTT over the extended domain, unscale by zeta^-i;
 * in place on d_ext (2^ext_k); the caller truncates to n*(deg-1).                               */
int zk_extended_to_coeff(zk_ctx* ctx, void* d_ext, uint32_t ext_k);

/* ---- polynomial helpers: halo2_proofs::arithmetic  -- SURVEY 8a K9, K10 ------------------------ */
/* eval_polynomial(coeffs, x) -> one Fr on the host */
int zk_poly_eval(zk_ctx* ctx, const void* d_coeffs, size_t n, const void* h_x, void* h_out);
/* eval_polynomial of `count` polynomials (device pointers, n coefficients each) at one point:
 * one power table and one synchronisation for all of them; h_out receives count Fr               */
int zk_poly_eval_batch(zk_ctx* ctx, const void* const* d_coeff_ptrs, size_t count, size_t n, const void* h_x, void* h_out);
/* eval_polynomial for (polynomial, point) pairs in one pass: h_out[j] = d_coeff_ptrs[j](h_points[point_index[j]]).  The evaluations
 * of a proof (plonk/prover.rs: every advice / fixed / permutation / lookup query at x w^rot) open a dozen distinct points when a
 * column is read at many rotations; this is one table build, one Horner launch and one download for all of them.              */
int zk_poly_eval_pairs(zk_ctx* ctx, const void* const* d_coeff_ptrs, const uint32_t* point_index, size_t count, const void* h_points, size_t num_points, size_t n, void* h_out);
/* kate_division(coeffs, z): d_q receives n-1 coefficients of (f(X) - f(z)) / (X - z)             */
int zk_kate_division(zk_ctx* ctx, const void* d_coeffs, size_t n, const void* h_z, void* d_q);
/* z[0] = 1 (product) / 0 (sum); z[i+1] = z[i] (*|+) a[i]: the permutation / lookup grand product
 * and grand sum.  d_z may not alias d_a.                                      */
int zk_fr_prefix_product(zk_ctx* ctx, const void* d_a, void* d_z, size_t n);
int zk_fr_prefix_sum(zk_ctx* ctx, const void* d_a, void* d_z, size_t n);

/* ---- quotient / expression evaluation: halo2_proofs::plonk::evaluation (evaluate_h, GraphEvaluator)
 * + vanishing divide_by_vanishing_poly  -- SURVEY 8a K4, K5 ------------------------------------ */
/* Runs one postfix program per row i of a 2^ext_k domain and writes out[i] (see quotient.hip for
 * the instruction set: 3 x u32 per instruction {op, a, b}).  Columns are device pointers to
 * 2^ext_k Fr values each (extended-coset evaluations, or Lagrange values when ext_k == k);
 * PUSH_COL reads row (i + rot * 2^(ext_k-k)) mod 2^ext_k.  divide_by_vanishing != 0 multiplies the
 * result by 1/(X^n - 1) evaluated on the zeta-coset.  d_out must not alias any input column.
 * TEE_TMP t / PUSH_TMP t keep GraphEvaluator-style intermediates of the row in device scratch
 * (t < 4096, 2^ext_k x 32 B each); reading one before it is written is ZK_ERR_INVALID_ARG.          */
int zk_quotient_eval(zk_ctx* ctx, const uint32_t* h_program, uint32_t num_instr, const void* const* h_col_ptrs, uint32_t num_cols,
                     const void* h_consts, uint32_t num_consts, uint32_t k, uint32_t ext_k, int divide_by_vanishing, void* d_out);
/* Host only (no device): the instruction stream the evaluator's kernel runs for `program` -- memory operands fused
 * into the operations (ADD_COL 16, SUB_COL 17, RSUB_COL 18, MUL_COL 19, FOLD_COL 20 | const << 12, NOP 21), bit 8 / 9
 * of word 0 = "settle t0 / t1 first", parked intermediates as columns num_cols + slot.  fuse = 0 keeps the caller's
 * sequence; fuse & 2 also fuses Horner steps  (S MUL_CONST c) + X * mem (+ chain)  into MAC_COL 22 | const << 16 (t0 = t0 * mem + S * c,
 * one reduction), as zk_quotient_eval does unless ZK_QUOTIENT_MAC=0.  out_words may be NULL (sizes only).  For tests and for inspecting
 * what a key's gates compile to. */
int zk_host_quotient_lower(const uint32_t* program, uint32_t num_instr, uint32_t num_cols, int fuse, uint32_t* out_words, size_t cap_words,
                           uint32_t* out_instr, int* out_depth);
/* The same, and *out_declined (may be NULL) = the sums of two column products left unfused because fusing them would have taken the
 * stack deeper than the fuse = 3 stream goes.  fuse & 4 (with fuse & 2; zk_quotient_eval unless ZK_QUOTIENT_MAC=0 or 1): a Horner step over a sum
 * of two column products, S c + X * m1 + Y * m2, becomes  S, X, PUSH_COL32 23 (m1: pushes 32 m1; its settle bits act on the entry it spills, X), Y,
 * MAC2_COL 24 | const << 16 (m2)  -- three products, one reduction, three entries popped -- and one over a product of two computed values,
 * S c + U * V, becomes  S, U, V, MAC_STK 25 | const << 16  (two entries popped).  fuse = 0 ... 3 are unaffected by bit 2's existence. */
int zk_host_quotient_lower2(const uint32_t* program, uint32_t num_instr, uint32_t num_cols, int fuse, uint32_t* out_words, size_t cap_words,
                            uint32_t* out_instr, int* out_depth, uint32_t* out_declined);
/* Host only (no device): where zk_quotient_eval would cut `program` into slices for 2^ext_k rows (round 6: a large sum of terms
 * acc = acc * c_f + term_f whose operands are read many times is evaluated slice by slice over the same rows at the same time so
 * that the slices find each other's operands in the caches; cuts only at top-level FOLDs that no parked intermediate is alive
 * across).  out_cuts receives the first instruction of every slice and the end of the program (*out_count entries; 0 = the program
 * runs in one piece).  The cuts are those for packed columns (32-byte rows); a proof's class programs read coset records of 36-byte
 * rows and may be cut finer: zk_host_quotient_launch shows those.  ZK_QUOTIENT_SLICES=0 / N turns the slicing off / asks for N slices.  No counterpart in halo2's evaluate_h
 * (plonk/evaluation.rs, external crate), which walks one row at a time on the CPU.                                              */
int zk_host_quotient_slices(const uint32_t* program, uint32_t num_instr, uint32_t ext_k, uint32_t* out_cuts, size_t cap, uint32_t* out_count);
/* Host only (no context, no device): what a launch of `program` over 2^ext_k rows looks like under the ZK_QUOTIENT_* knobs in force at the
 * call -- everything zk_quotient_eval decides before it touches the device (csrc/quotient_lower.hpp: plan_quotient_launch).  records != 0: the
 * columns are coset record buffers, as in a proof's class programs (36-byte rows: the slicer cuts for those).  out_head receives
 * ZK_QUOTIENT_LAUNCH_HEAD words: kernel (1 k_quotient_eval, 2 k_quotient_eval2), record operands, the grid covers the domain exactly (FULL),
 * accumulator in memory (ACC_MEM), sliced, slices (1: whole), lowered stack depth, LDS bytes per workgroup, parking slots (renumbered per slice),
 * lowered instructions, folds among them, words per instruction (3 or 4), word offset of the combining program, word offset of the slice table,
 * bytes of the program / column-table / constant regions of the upload, the row-tile alias passed to the kernel.  *out_count receives the
 * length of the program region in words and out_words (cap_words of room; NULL with 0 to ask for the length) the region as uploaded: per slice
 * its lowered instructions (w0, a, b and, for kernel 2, the class mask) and four END records; for a sliced launch the combining program
 * (FOLD_COL | (num_consts + s) << 16 reading column num_cols + parking slots + s, s = 0 .. slices - 1), its four END records and the slice table,
 * (first word, instructions + 1) per slice.  A program zk_quotient_eval refuses gives that status. */
#define ZK_QUOTIENT_LAUNCH_HEAD 18
int zk_host_quotient_launch(const uint32_t* program, uint32_t num_instr, uint32_t num_cols, uint32_t num_consts, uint32_t ext_k, int records,
                            uint32_t* out_head, uint32_t* out_words, size_t cap_words, size_t* out_count);

/* Host only, for tests: how the prover distributes constraint programs over its degree classes when the programs share
 * intermediates (TEE_TMP in one constraint, PUSH_TMP in a later one -- halo2's GraphEvaluator intermediates as exported): a
 * class that reads an intermediate it has not computed re-materialises the defining sub-expression.  words: 3 per instruction,
 * `count` programs back to back; cls[i] < classes.  Output: the class programs back to back, each constraint followed by the
 * marker {FOLD (9), i, 0}.  *conflict = 1 for slot reuse across constraints (the prover then evaluates a single class). */
int zk_host_split_programs(const uint32_t* words, const uint32_t* lens, const uint32_t* cls, uint32_t count, uint32_t classes,
                           uint32_t* out_words, size_t out_cap_words, uint32_t* out_lens, int* conflict);
/* Host only, for tests: the additive split of ONE constraint program over the degree classes 0 .. E as the prover applies it: a
 * constraint that is a sum of terms of different degrees (q (a b - c): degree 3 and degree 2) hands each term to the class of its
 * own degree -- h is linear in the constraints -- so that columns occurring only in low-degree terms are transformed to fewer cosets
 * (halo2's evaluate_h, external crate, evaluates every constraint on the whole extended domain; same h: the prover carries what a
 * moved term is on H along as a remainder polynomial, so that every class stays divisible by X^n - 1).  Output: the pieces back to
 * back, out_lens[j] instructions of class out_cls[j]; one piece (the program itself) when it is not split.  out_words may be NULL
 * (count only). */
int zk_host_additive_split(const uint32_t* words, uint32_t num_instr, uint32_t E, uint32_t* out_words, size_t out_cap_words, uint32_t* out_cls, uint32_t* out_lens,
                           uint32_t cap_pieces, uint32_t* num_pieces);
/* Host only, for tests: the program of ONE degree class as the prover assembles it from the class's terms (term t belongs to
 * constraint cons[t] < K of the K constraints halo2's evaluate_h folds with y, external crate): the weighted sum
 * sum_t y^(K-1-cons[t]) term_t with the terms that share a single-column factor -- a selector, l_active -- collected under ONE product by
 * that factor, instead of folding the terms one by one (a product per term for the folding, another for its selector).  Same
 * polynomial, same h.  A weight is the constant 0xFFFC0000 + (K-1-cons[t]) (= that power of y).  Terms that park or read
 * intermediates keep their definitions ahead of their readers.  ZK_ERR_UNSUPPORTED when the prover would keep the folded form (a
 * stack deeper than the evaluator's).  out_words may be NULL (count only). */
int zk_host_group_terms(const uint32_t* words, const uint32_t* lens, const uint32_t* cons, uint32_t count, uint32_t K, uint32_t* out_words, size_t out_cap_words,
                        uint32_t* out_instr);

/* Host only, for tests: the program of ONE degree class as the prover COMPILES it (round 6; csrc/class_compile.hpp) -- what halo2's
 * GraphEvaluator (plonk/evaluation.rs, external crate) does for a circuit whose gates share sub-expressions, done on this side of the
 * boundary: the terms become one hash-consed expression graph (TEE_TMP / PUSH_TMP of the incoming programs resolved), the y-weighted
 * sum is regrouped under common FACTORS of any shape (a selector product q_usable * q_step * state_selector, a gadget's condition
 * [REF zkevm-circuits/src/evm_circuit/execution.rs:832-851]), sums run in Horner form over the constraint index, values still used
 * twice are parked in slots assigned by liveness.  The program leaves acc = sum_t y^(*out_last - cons[t]) term_t.  out_stats[0..5] =
 * graph nodes, values parked, slots alive at once, products, factor groups, stack depth.  ZK_ERR_UNSUPPORTED: stack too deep (the
 * prover then keeps zk_host_group_terms' form). */
int zk_host_compile_class(const uint32_t* words, const uint32_t* lens, const uint32_t* cons, uint32_t count, uint32_t K, uint32_t* out_words, size_t out_cap_words,
                          uint32_t* out_instr, uint32_t* out_last, uint32_t* out_stats);
/* Host only (no device, no SRS): the quotient plan of a constraint system -- degree classes, additive split, each class's compiled
 * program -- exactly as zk_proof_finish will follow it; cs_blob = the constraint-system part of a zk_pk_create blob (column data
 * not needed).  out_summary: [0] ext_k - k, [1] constraints, [2] classes on, [3] additive split on, [4] expression graph on,
 * [5] remainder polynomials, [6] cost estimate, [7] columns read; then 8 words per class: used, instructions, products, columns,
 * values parked, slots alive at once, factor groups, last.  With cap_summary >= 8 + 10 (E + 1): 2 more words per class after those,
 * reductions and fused multiply-accumulates (Horner steps evaluated as two products under one reduction; 0 with ZK_QUOTIENT_MAC=0).
 * Those two words describe the K_MAC_COL-only (fuse = 3) stream whatever the knob's other values: reductions + fused = products.  With
 * cap_summary >= 8 + 14 (E + 1): 4 more words per class after those, for the stream in force (ZK_QUOTIENT_MAC unset / 2: fuse = 7; 1: fuse = 3;
 * 0: none): sums of two column products fused (MAC2_COL), stack products fused (MAC_STK), MAC2_COL fusions declined for stack depth, reductions
 * of that stream (products - MAC_COL - 2 MAC2_COL - MAC_STK).  No word depends on the room given beyond its own presence.
 * class_index / out_words / out_instr: one class's program (optional). */
int zk_host_quotient_plan(const void* cs_blob, size_t blob_len, uint32_t* out_summary, size_t cap_summary, uint32_t class_index, uint32_t* out_words, size_t out_cap_words,
                          uint32_t* out_instr);

/* out[i] = base^i * mul for i < n (Montgomery form): omega-power / delta-power "columns"          */
int zk_fr_powers(zk_ctx* ctx, const void* h_base, const void* h_mul, void* d_out, size_t n);
/* logUp multiplicities (halo2 Scroll fork, plonk/mv_lookup/prover.rs: m(X)): d_m[i] = number of rows
 * r < usable_rows with d_inputs[r] == d_table[i] for i < usable_rows (a value that occurs in several
 * table rows is credited to the lowest one), 0 for usable_rows <= i < n.  *bad_row = lowest input
 * row whose value is not in the table, UINT64_MAX when every input is found.                        */
int zk_lookup_multiplicities(zk_ctx* ctx, const void* d_inputs, const void* d_table, size_t usable_rows, void* d_m, size_t n, uint64_t* bad_row);
/* n uniformly random Fr (Montgomery form) on the device: element i = Fr::from_uniform_bytes of
 * ChaCha20 block (first_block + i) under key32 / stream_id (64-bit counter in state words 12..13,
 * stream id in 14..15).  What the prover draws its blinding polynomial from (halo2 takes an RngCore
 * from the caller; plonk/vanishing/prover.rs fills the random poly from it element by element).    */
int zk_fr_random(zk_ctx* ctx, const uint8_t* key32, uint64_t stream_id, uint64_t first_block, void* d_out, size_t n);

/* ---- SRS: halo2_proofs::poly::kzg::commitment::ParamsKZG  -- SURVEY 8a A5 ---------------------- */
/* Upload g (n = 2^k G1Affine) and g_lagrange; host pointers.  h_g_lagrange may be NULL
 * (ParamsKZG::from_parts with None): the Lagrange basis is then derived on the device.            */
int zk_srs_create(zk_ctx* ctx, uint32_t k, const void* h_g, const void* h_g_lagrange, zk_srs** out);
/* ParamsKZG::unsafe_setup_with_s(k, s): g[i] = s^i * G, g_lagrange[i] = L_i(s) * G, on device.    */
int zk_srs_setup_with_s(zk_ctx* ctx, uint32_t k, const void* h_s, zk_srs** out);
/* ParamsKZG::downsize (prover/src/common/prover.rs:40-60: every layer shrinks the one params file
 * to its own degree): the first 2^new_k points of g, with the Lagrange basis of the smaller domain
 * recomputed on the device (g_to_lagrange: an inverse FFT over G1).                                 */
int zk_srs_downsize(zk_ctx* ctx, const zk_srs* srs, uint32_t new_k, zk_srs** out);
/* ---- SRS files: ParamsKZG::{read_custom, write_custom}; the reference loads `params{k}` through
 * prover::utils::load_params [REF prover/src/utils.rs:39-84], default format RawBytesUnchecked
 * [REF prover/src/utils.rs:32].  file = u32 k (LE) | g[n] | g_lagrange[n] | g2 | s_g2; G1 is 64 B
 * (formats 1, 2: the in-memory Montgomery image) or 32 B (format 0: x canonical LE, bit 254 = parity
 * of y, bit 255 = identity -- halo2curves @ a495a7b, pinned by the vk / proof bytes of
 * [REF aggregator/data/batch-task.json]); G2 is twice that and is handed through untouched.        */
#define ZK_SERDE_PROCESSED 0
#define ZK_SERDE_RAW 1            /* RawBytes: every point is checked (limbs < p, on the curve)      */
#define ZK_SERDE_RAW_UNCHECKED 2
/* 4 + 2 * 2^k * g1 + 2 * g2 bytes, the length load_params insists on; 0 for a bad k / format       */
size_t zk_params_file_len(uint32_t k, int format);
/* h_file: the whole file in host memory.  A length that does not match the k in its header is
 * refused before anything is parsed, like the reference.  h_g2 / h_s_g2 (nullable) receive the two
 * G2 encodings as they are in the file (128 B each, 64 B for Processed).                           */
int zk_params_read(zk_ctx* ctx, const void* h_file, size_t len, int format, zk_srs** out, void* h_g2, void* h_s_g2);
/* h_out = NULL: only *len is written (size query).  h_g2 / h_s_g2: the encodings to put in the file */
int zk_params_write(zk_ctx* ctx, const zk_srs* srs, const void* h_g2, const void* h_s_g2, int format, void* h_out, size_t cap, size_t* len);
/* unsafe_setup_with_s, G2 half (host only): the generator and s * generator as RawBytes
 * (x.c0 | x.c1 | y.c0 | y.c1, Montgomery limbs; 128 B each); h_s: one Montgomery Fr                */
int zk_g2_setup(const void* h_s, void* h_g2, void* h_s_g2);
void zk_srs_destroy(zk_ctx* ctx, zk_srs* srs);
uint32_t zk_srs_k(const zk_srs* srs);
const void* zk_srs_g(const zk_srs* srs);          /* device pointer, n G1Affine */
const void* zk_srs_g_lagrange(const zk_srs* srs); /* device pointer or NULL     */

/* ---- MSM: halo2_proofs::arithmetic::best_multiexp  -- SURVEY 8a K1 ----------------------------- */
/* sum_i scalars[i] * bases[i] over device buffers; the affine result (64 B) is written to the
 * host.  Scalars are Montgomery-form Fr exactly as halo2 holds them.                             */
int zk_msm_g1(zk_ctx* ctx, const void* d_scalars, const void* d_bases, size_t n, void* h_out_affine);
/* num_segments independent MSMs in one pass: out[s] = sum of scalars[i] * bases[i] over i in [h_seg_offsets[s],
 * h_seg_offsets[s + 1]) (num_segments + 1 offsets on the host, the first 0, non-decreasing).  Scalars: Montgomery Fr; bases: 64 B
 * affine Montgomery, arbitrary points (no table is built, nothing is cached), the identity as all zeros.  h_out_affine
 * receives num_segments x 64 B (identity: all zeros; an empty segment gives the identity).  All segments share one sequence
 * of three launches and one download -- no launch and no synchronisation per segment: what many sums of a few to a few
 * thousand points need (zk_verify_accumulators: two per proof), where one zk_msm_g1 call per sum would pay its sort, its
 * launches and its host tail every time.  It spends about one addition per scalar bit and point: one large sum belongs to
 * zk_msm_g1.                                                                                                            */
int zk_msm_g1_segments(zk_ctx* ctx, const void* d_scalars, const void* d_bases, const uint32_t* h_seg_offsets, size_t num_segments, void* h_out_affine);
/* ParamsKZG::commit (basis = 0, over g) / commit_lagrange (basis = 1, over g_lagrange).          */
int zk_commit(zk_ctx* ctx, const zk_srs* srs, int basis, const void* d_scalars, size_t n, void* h_out_affine);
/* `count` commitments over the same basis (ParamsKZG::commit_lagrange over every advice column
 * of a phase): d_scalar_ptrs[i] addresses n Fr on the device, h_out_affine receives count x 64 B.
 * Consecutive MSMs are pipelined on side streams.  Each column is judged on the device first (4096
 * sampled cells): columns with at most a quarter of field-sized cells (>= 2^64) take the per-window
 * path of zk_commit_batch_hint's hint 1 -- a choice that affects speed only, never the result.     */
int zk_commit_batch(zk_ctx* ctx, const zk_srs* srs, int basis, const void* const* d_scalar_ptrs, size_t count, size_t n, void* h_out_affine);
/* zk_commit_batch for columns still in host memory: column i+1 is uploaded (copy stream) while the
 * MSM of column i runs; d_cols[i] (n x 32 B device buffers) receive the columns.  This is the shape
 * of halo2's advice commitment loop (plonk/prover.rs: one commit_lagrange per witness column).     */
/* zk_commit_batch with a hint per column (nullable array).  narrow[i] = 1: column i holds small
 * integers (below 2^64: selectors, bytes, counters, lookup multiplicities), whose digits leave most
 * Pippenger windows empty; such a column takes the per-window MSM path, which skips empty windows,
 * instead of the merged-window path, which always pays for its 2^(c-1) shared buckets.
 * narrow[i] = 2: dense values in long runs of equal scalars (running products / sums that stay
 * constant over stretches of rows: permutation products of a circuit with few copy constraints).  A
 * column of at least 4096 rows with at most n / 16 runs is committed by its run ends -- Abel
 * summation against a prefix-sum table of the basis built on first use (64 B per SRS point,
 * csrc/runs.hip; ZK_MSM_RUNS=0 turns that off); otherwise the merged-window path with the sliced
 * bucket sort, whose four workgroups per partition stream a run-filled partition faster than the
 * one-launch sort does.
 * narrow[i] = 3: a running sum whose increments are mostly equal (a lookup's phi: the increment is
 * the same on every row where the lookup is switched off and the table row unused).  A full-length
 * column over the Lagrange basis is committed as an MSM of s_j = c - (z_{j+1} - z_j) -- zero wherever
 * the increment is the common value c -- over the prefix sums of the basis, plus c times a fixed
 * point (csrc/runs.hip; ZK_MSM_DIFF=0 turns that off); a column whose increments are not mostly
 * equal costs what a dense column costs.
 * 0: dense.  The hint affects speed only.  zk_commit_batch_h2d and zk_proof_advice_phase derive
 * 0 / 1 themselves from a sample of the host column.                                              */
int zk_commit_batch_hint(zk_ctx* ctx, const zk_srs* srs, int basis, const void* const* d_scalar_ptrs, size_t count, size_t n, const uint8_t* narrow, void* h_out_affine);
int zk_commit_batch_h2d(zk_ctx* ctx, const zk_srs* srs, int basis, const void* const* h_cols, void* const* d_cols, size_t count, size_t n, void* h_out_affine);
/* best_multiexp over HOST slices, exactly the reference signature (copies in, computes, copies
 * the affine result out).                                                                        */
int zk_msm_g1_host(zk_ctx* ctx, const void* h_scalars, const void* h_bases, size_t n, void* h_out_affine);
/* Introspection: Pippenger window size (bits) and window count that commitments of n points over
 * this SRS use -- with the SRS's fixed-base window tables all windows share one bucket set (c = 20,
 * 13 windows at k = 20); without them (tables beyond ZK_MSM_TABLE_GB, default 32 GiB per basis)
 * one bucket set per window (c <= 16).                                                            */
int zk_msm_plan(const zk_srs* srs, size_t n, int* window_bits, int* windows);
/* Host only: the merged-window plan for an SRS of 2^k points, with the shift applied to the top window's digit (the top window
 * holds only the leading bits of a scalar; its digit is scaled so that its entries spread over the bucket range). */
int zk_host_msm_plan(uint32_t k, int* window_bits, int* windows, int* top_shift);
/* Host only (no context, no device): the plan of one batch of `count` commitments of n points (1 <= n <= 2^k, k <= 28) over an
 * SRS of 2^k points that has its merged-window table, as the library decides it under the ZK_MSM_* knobs in force at the call.
 * hints (nullable): one byte per column, as zk_commit_batch_hint's; blinded_tail: the rows at the end of the hint-1 columns that
 * the prover commits apart; window_table: the SRS also has the per-window table of its small-valued columns; group_cap: 0, or the
 * bound on a group's columns that the retry with less memory applies; prof_on, graph_broken: the two context states that turn
 * graph replay off.  *out_count receives the length of the record in 64-bit words, out_words (cap_words of room; NULL with 0 to
 * ask for the length) the record:
 *   head, ZK_MSM_BATCH_PLAN_HEAD words: status (0; 1: the batch exceeds the 32-bit entry space -- the record ends with the head),
 *     any small-valued column, tail rows, rows in front of the tail, digit-matrix row stride, columns per group, groups take the
 *     GM sort, GM bucket sets, GM range bits, GM partitions per column, GM bucket numbering, GM partition workgroups, words of
 *     the per-window / GM / merged sort layouts, words per workspace copy, copies, one-launch partition sort, range bits, chunk,
 *     staged scatter, partition workgroups, pipelines, graph replay, points per bucket buffer, next group_cap to try (0: none),
 *     merged window bits / windows / top shift, per-window window bits / windows, reduction blocks per bucket set of a group
 *   three sort layouts (per-window, GM, merged): words, regions, then per region (id, offset, length) in words, ascending --
 *     ids: 0 slice counters, 1 slice offsets, 2 bucket counts, 3 the cleared region (size bins, counters, window flags,
 *     done-counters), 4 bucket offsets, 5 bucket order, 6 tasks per bucket, 7 task offsets, 8 / 9 / 10 block totals of the
 *     slice / bucket / histogram scans, 11 partition histogram, 12 its offsets, 13 sorted indices, 14 digit matrix, 15 entries;
 *     a layout the batch does not use has 0 words and 0 regions
 *   four bucket layouts, one per kind of step (0 per-window sort, 1 dense column with the one-launch sort, 2 dense column with the
 *     sliced sort, 3 GM group): buckets and task bound of a full group, points, regions, then per region (id, offset, length) in
 *     points -- ids: 0 buckets, 1 partials of the reduction, 2 task partials, 3 folded windows; all 0 for a kind the batch lacks
 *   steps: their number, then (first column, columns, kind) each
 *   graph key, the plan's part: its length, then n, merged window bits, per-window window bits, top shift, table stride, words
 *     per copy, staged scatter, range bits, rows in front of the tail, partition workgroups                                   */
#define ZK_MSM_BATCH_PLAN_HEAD 32
int zk_host_msm_batch_plan(uint32_t k, size_t n, size_t count, const uint8_t* hints, uint32_t blinded_tail, int window_table, uint32_t group_cap, int prof_on, int graph_broken,
                           uint64_t* out_words, size_t cap_words, size_t* out_count);

/* Host-only: out = sum of n affine points (no context, no device).  Used to finish a point-sharded
 * MSM: each rank's 64-byte partial result is all-gathered as bytes (RCCL has no EC reduce op) and
 * summed here.                                                                                   */
int zk_g1_sum_host(const void* h_points_affine, size_t n, void* h_out_affine);

/* ---- full proof: halo2_proofs::plonk::{keygen_pk, create_proof} with the GWC or SHPLONK multi-open
 * (poly::kzg::multiopen::{ProverGWC, ProverSHPLONK})  -- SURVEY 8a A1, A4, K6-K11; csrc/prover.hip -- */
typedef struct zk_pk zk_pk;
typedef struct zk_proof zk_proof;       /* a proving session, see below */
/* keygen_pk over a flat circuit description (the "pk blob", version 3 or 4, filled by the Rust shim from
 * halo2's ConstraintSystem / by zkevm-circuits_amd/plonk.py in tests: header, phases, the advice /
 * fixed / instance query lists in registration order, permutation columns, constants, gate programs,
 * mv-lookup arguments (one table tuple + N input tuples each, as chunk_lookups() leaves them
 * [REF zkevm-circuits/src/super_circuit/test.rs:59]), then the column data -- version 3: fixed and
 * sigma columns in Lagrange form, n Montgomery Fr each; version 4: fixed columns as n cells of 1, 2,
 * 4, 8, 16 bytes (unsigned integers) or 32 (Montgomery Fr) and the permutation as halo2's
 * Assembly::mapping, (u32 j', u32 i') per cell, from which the sigma columns are built on the
 * device: the same key, commitments and proofs as version 3.  A cell width outside that set, column
 * data shorter than the header and widths say, or a mapping entry outside [0, P) x [0, n) is
 * refused with ZK_ERR_INVALID_ARG; layout in INTEGRATION.md).  Commits fixed and sigma columns and keeps their Lagrange and
 * coefficient forms on the device.  srs must have the circuit's k (zk_srs_downsize).  A blob whose
 * declared degree is below what its gates and lookup arguments require (halo2
 * ConstraintSystem::degree) is refused.                                                            */
int zk_pk_create(zk_ctx* ctx, const zk_srs* srs, const void* h_blob, size_t blob_len, zk_pk** out);
void zk_pk_destroy(zk_ctx* ctx, zk_pk* pk);
/* verifying-key side: (F + P) x 64-byte affine commitments (fixed, then sigma) and vk_repr (Fr)  */
int zk_pk_vk(zk_ctx* ctx, const zk_pk* pk, void* h_commitments, void* h_vk_repr);
/* `vk.transcript_repr()`: the scalar create_proof absorbs first (halo2 VerifyingKey::hash_into).
 * halo2 derives it from the Debug string of the pinned verifying key -- the value the reference
 * pins for the SuperCircuit at [REF zkevm-circuits/src/super_circuit/test.rs:70-85] -- which only
 * the Rust side can produce: the shim computes it with upstream keygen_vk and installs it here (32 B
 * Montgomery Fr), after which proofs of this key are proofs for the reference's own verify_proof.
 * Without this call the key uses a stand-in (Blake2b-512 "Halo2-Verify-Key" over the
 * constraint-system part of the blob and the compressed fixed / sigma commitments).                */
int zk_pk_set_transcript_repr(zk_ctx* ctx, zk_pk* pk, const void* h_repr_fr32);
/* out16 = k, degree, extended k, F, A, I, permutation columns, permutation chunks, lookup arguments,
 * phases, challenges, blinding factors, advice queries, fixed queries, commitments per proof,
 * evaluations per proof                                                                            */
int zk_pk_shape(zk_ctx* ctx, const zk_pk* pk, uint32_t* out16);
/* The quotient plan of a key -- how its constraints are dealt to degree classes and what each class's program costs (halo2's
 * `Evaluator::new` builds the corresponding GraphEvaluator at keygen, plonk/evaluation.rs, external crate): zk_host_quotient_plan's
 * summary (8 + 8 x (extended_k - k + 1) words) for `pk` under the measurement knobs in force.  Made on first use, kept by the key. */
int zk_pk_quotient_plan(zk_ctx* ctx, const zk_pk* pk, uint32_t* out_summary, size_t cap_summary);
/* create_proof: h_advice / h_instance are arrays of host pointers to n x 32-byte Lagrange columns;
 * seed16 seeds the XorShift blinding RNG; the proof bytes (compressed points and canonical
 * scalars, halo2 encoding) are written to h_proof.  Fails with ZK_ERR_INVALID_ARG if the witness
 * does not satisfy the copy or lookup constraints.                                               */
int zk_create_proof(zk_ctx* ctx, const zk_pk* pk, const void* const* h_advice, const void* const* h_instance, const uint8_t* seed16,
                    void* h_proof, size_t proof_cap, size_t* proof_len);

/* ---- dev::MockProver on the device: halo2_proofs::dev::MockProver::{run, verify_par, verify_at_rows_par}
 * [REF zkevm-circuits/src/test_util.rs:272], [REF prover/src/common/prover/mock.rs:18-19], [REF testool/src/statetest/executor.rs:703-714]
 * -- SURVEY 8a A9.  No commitments, no transcript: checks that the witness satisfies the key's circuit and says where it does not.
 *   ZK_MOCK_GATE         VerifyFailure::ConstraintNotSatisfied: gate polynomial `index` (position in the key's flat list of
 *                        gate polynomials = the blob's order) is not zero at `row`
 *   ZK_MOCK_LOOKUP       VerifyFailure::Lookup: input tuple `sub` of lookup argument `index` at `row` occurs in no usable row of the table
 *   ZK_MOCK_PERMUTATION  VerifyFailure::Permutation: cell `row` of permutation column `index` (position in the key's list of
 *                        permutation columns) differs from the cell sigma maps it to (sub 0); sub 1: sigma names no cell (a broken key)
 * gate_rows / lookup_rows: the row ids of verify_at_rows_par (each must be a usable row, else ZK_ERR_INVALID_ARG -- upstream
 * panics); NULL = every usable row (verify_par).  Copy constraints are always checked on all rows, as upstream does.
 * h_advice / h_instance: host pointers to n x 32-byte columns (as zk_create_proof); h_challenges: the circuit's challenges
 * (32 B each, Montgomery Fr, zk_pk_shape's count) or NULL for MockProver's own (zk_host_mock_challenges).
 * out receives the first `cap` failures sorted by (kind, index, sub, row); *count the number found (may exceed cap: then
 * which ones were kept is unspecified).  Region bookkeeping (CellNotAssigned, ConstraintPoisoned) is not modelled: the
 * witness arrives as finished columns.  Gate failures are detected with a random fold first (a satisfied witness costs one
 * evaluation pass; a failing one is missed with probability < gates / 2^253) and then listed exactly, one pass per polynomial. */
typedef struct zk_mock_failure { uint32_t kind, index, sub, row; } zk_mock_failure;
enum { ZK_MOCK_GATE = 1, ZK_MOCK_LOOKUP = 2, ZK_MOCK_PERMUTATION = 3 };
int zk_mock_verify(zk_ctx* ctx, const zk_pk* pk, const void* const* h_advice, const void* const* h_instance, const void* h_challenges,
                   const uint32_t* gate_rows, size_t num_gate_rows, const uint32_t* lookup_rows, size_t num_lookup_rows,
                   zk_mock_failure* out, size_t cap, size_t* count);
/* The same checks inside a proving session, after its last advice phase and before zk_proof_finish: over the columns the
 * session holds on the device and with the challenges its transcript produced (no second upload).  What a rejected proof
 * leaves open -- which constraint the witness breaks, and where -- in one call; the session stays usable.            */
int zk_proof_mock_verify(zk_ctx* ctx, zk_proof* proof, const uint32_t* gate_rows, size_t num_gate_rows, const uint32_t* lookup_rows, size_t num_lookup_rows,
                         zk_mock_failure* out, size_t cap, size_t* count);
/* Host only: the challenges MockProver hands a circuit (halo2 dev.rs: h = Blake2b-512("Halo2-MockProver"), then
 * challenge i = Fr::from_uniform_bytes(h = Blake2b-512(h)); the third one is the constant the reference pins at
 * [REF zkevm-circuits/src/super_circuit.rs:729]).  out: count x 32 B Montgomery Fr.                       */
int zk_host_mock_challenges(uint32_t count, void* out_fr32);

/* Phase-by-phase proving session (what the Rust shim drives: Circuit::synthesize runs on the host
 * once per phase and needs the challenges of the earlier phases -- the SuperCircuit has three
 * phases, zkevm-circuits/src/util.rs:120-133).  begin -> zk_proof_advice_phase x num_phases ->
 * finish.  zk_create_proof is begin + all phases + finish for witnesses known up front.          */
/* multi-open scheme of the session: GWC (ProverGWC, what north_star names; default) or SHPLONK
 * (ProverSHPLONK / BDFG21, what the reference's call sites instantiate: two commitments in total) */
enum { ZK_MULTIOPEN_GWC = 0, ZK_MULTIOPEN_SHPLONK = 1 };
int zk_proof_set_multiopen(zk_ctx* ctx, zk_proof* proof, int kind);
/* The vanishing argument's "random" polynomial (halo2 vanishing::Argument::commit).  ONE (default): the constant 1, commitment
 * g[0], evaluation 1 -- what the reference's own prover emitted: in [REF aggregator/data/batch-task.json: chunk_proofs[0]] that
 * commitment is (1, 2) and that evaluation is 1 (Scroll's fork commits no blinding polynomial).  UNIFORM: n uniform coefficients
 * as upstream PSE halo2 draws them (one more dense commitment).  The verifier accepts either.  Any time before zk_proof_finish.  */
enum { ZK_VANISHING_UNIFORM = 0, ZK_VANISHING_ONE = 1 };
int zk_proof_set_vanishing_random(zk_ctx* ctx, zk_proof* proof, int kind);
int zk_proof_begin(zk_ctx* ctx, const zk_pk* pk, const void* const* h_instance, const uint8_t* seed16, zk_proof** out);
/* The same with halo2's instance slices as they are: h_instance[i] holds h_instance_len[i] values
 * (not n).  Exactly those values are absorbed into the transcript -- what create_proof and
 * verify_proof do: a circuit with a handful of public inputs absorbs a handful of scalars -- and the
 * column is zero-padded on the device.  More values than usable rows is Error::InstanceTooLarge
 * (status ZK_ERR_INVALID_ARG).  zk_proof_begin / zk_create_proof are the special case "every
 * usable row is a public input".                                                                  */
int zk_proof_begin_instances(zk_ctx* ctx, const zk_pk* pk, const void* const* h_instance, const uint32_t* h_instance_len, const uint8_t* seed16, zk_proof** out);
/* External transcript (halo2's `T: TranscriptWrite<G1Affine, Challenge255>` argument of
 * create_proof): by default the session runs halo2's Blake2bWrite itself and zk_proof_finish
 * returns the proof bytes.  With a vtable every transcript operation is forwarded to the host
 * language's own transcript object instead -- Poseidon for the aggregation layers
 * (aggregator/src/core.rs:25-28), Keccak for EVM proofs (prover/src/common/prover/evm.rs:67) --
 * which then also owns the proof bytes (zk_proof_finish reports length 0).  Points are 64 B
 * affine (x || y, Montgomery limbs, identity = zeros), scalars 32 B Montgomery Fr; a callback
 * returns 0 on success.  Call right after zk_proof_begin: what begin absorbed (vk representative,
 * instance values) is replayed into the external transcript.                                       */
/* Built-in transcripts of the session (the three the reference's call sites instantiate): Blake2b
 * (Blake2bWrite + Challenge255, the default [REF circuit-benchmarks/src/super_circuit.rs:112]),
 * Poseidon (snark-verifier PoseidonTranscript<NativeLoader, _> with POSEIDON_SPEC: gen_snark_shplonk
 * [REF prover/src/common/prover/utils.rs:31], [REF aggregator/src/core.rs:91-92]) and EVM (snark-verifier
 * EvmTranscript, Keccak-256, 64-byte big-endian points: gen_evm_proof_shplonk
 * [REF prover/src/common/prover/evm.rs:67]).  Call right after zk_proof_begin.  A Poseidon / EVM
 * transcript cannot absorb the identity point (as upstream): zk_proof_finish then fails.          */
enum { ZK_TRANSCRIPT_BLAKE2B = 0, ZK_TRANSCRIPT_POSEIDON = 1, ZK_TRANSCRIPT_EVM = 2 };
int zk_proof_set_transcript_kind(zk_ctx* ctx, zk_proof* proof, int kind);
/* The same transcripts as host-only objects (no context, no device): what a caller needs to run
 * halo2's verifier-side transcript logic, or to cross-check its own transcript, without Rust.
 * Points 64 B affine Montgomery, scalars 32 B Montgomery Fr; status 0 = OK.                        */
typedef struct zk_transcript zk_transcript;
zk_transcript* zk_transcript_new(int kind);
void zk_transcript_free(zk_transcript* t);
int zk_transcript_common_point(zk_transcript* t, const void* affine64);
int zk_transcript_common_scalar(zk_transcript* t, const void* fr32);
int zk_transcript_write_point(zk_transcript* t, const void* affine64);
int zk_transcript_write_scalar(zk_transcript* t, const void* fr32);
int zk_transcript_squeeze(zk_transcript* t, void* fr32_out);
/* bytes written so far (the proof); the pointer stays valid until the next write or free          */
size_t zk_transcript_proof(const zk_transcript* t, const void** data);
/* host-only hashes behind them: Keccak-256 and the Poseidon permutation (5 x 32 B Montgomery Fr)   */
int zk_host_keccak256(const void* data, size_t len, void* out32);
int zk_host_poseidon_permute(void* state5_fr32);
/* the same generator at width 3 (R_F = 8, R_P = 57): the permutation under the reference's Poseidon code hash; its value on
 * (0, 0, 0) is POSEIDON_CODE_HASH_EMPTY (eth-types/src/lib.rs:278), which is what pins the constant generation          */
int zk_host_poseidon_permute_width3(void* state3_fr32);
typedef struct zk_transcript_vtable {
    int (*common_point)(void* user, const void* affine64);
    int (*common_scalar)(void* user, const void* fr32);
    int (*write_point)(void* user, const void* affine64);
    int (*write_scalar)(void* user, const void* fr32);
    int (*squeeze_challenge)(void* user, void* fr32_out);
} zk_transcript_vtable;
int zk_proof_set_transcript(zk_ctx* ctx, zk_proof* proof, const zk_transcript_vtable* vtable, void* user);
/* ---- verifier: halo2_proofs::plonk::verify_proof (KZG) -- SURVEY 8a A6 -------------------------
 * The reference verifies what it proves through verify_snark_shplonk [REF prover/src/common/verifier.rs:35] (its verifier
 * services [REF prover/src/zkevm/verifier.rs:45], [REF prover/src/aggregator/verifier.rs:57]).
 * zk_vk: halo2 VerifyingKey (keygen_vk without the columns).  h_cs_blob: the constraint-system part of a key blob of version 3 or 4 (what
 * zk_pk_create reads before the column data, parsed by the same code) or the whole blob (its columns are not read); h_commitments: the F fixed then P sigma commitments,
 * 64 B affine each, as zk_pk_vk returns them (num_commitments must be F + P); h_vk_repr_fr32: vk.transcript_repr (Montgomery
 * Fr).  Host only, no column data, any k <= 27.  ZK_ERR_INVALID_ARG for a truncated, malformed or over-long blob.       */
typedef struct zk_vk zk_vk;
int zk_vk_create(const void* h_cs_blob, size_t len, const void* h_commitments, size_t num_commitments, const void* h_vk_repr_fr32, zk_vk** out);
void zk_vk_destroy(zk_vk* vk);
/* Proof length in bytes that this key gives under a transcript kind and multi-open scheme (host only). */
int zk_vk_proof_len(const zk_vk* vk, int transcript_kind, int multiopen, size_t* len);
/* The 16 words of zk_pk_shape, from the constraint system alone (host only). */
int zk_vk_shape(const zk_vk* vk, uint32_t* out16);
/* halo2 verify_proof, KZG, VerifierGWC / VerifierSHPLONK (multiopen), Blake2b / Poseidon / EVM transcript.  count = 1:
 * SingleStrategy.  count > 1: AccumulatorStrategy over proofs of the same vk -- every proof's DualMSM weighted by a power of a
 * batching scalar (Blake2b over the key, every proof and every instance: deterministic, no caller RNG) and summed, one MSM on
 * the device, one pairing check for all.  h_instances[b][i] / h_instance_lens[b][i]: the values of instance column i of proof
 * b (Montgomery Fr), absorbed exactly as given.  g2_128 / s_g2_128: [1]G2 and [s]G2 of the SRS (128 B, x.c0 | x.c1 | y.c0 |
 * y.c1 Montgomery).  *ok = 1 accept, 0 reject.  A malformed proof (wrong length, a point not on the curve or not decodable, a
 * non-canonical scalar, more instance values than usable rows) is a reject (ZK_OK, *ok = 0), not an error.
 * ZK_ERR_INVALID_ARG only for bad arguments (null pointers, unknown kind or scheme).  A batch holds proofs of one key: a proof
 * made with another key in it is rejected (its transcript and commitments are not this key's), never accepted.  A rejected
 * batch does not say which proof failed: verify them one at a time for that.                                           */
int zk_verify_proofs(zk_ctx* ctx, const zk_vk* vk, size_t count, const void* const* const* h_instances, const uint32_t* const* h_instance_lens,
                     const void* const* h_proofs, const size_t* h_proof_lens, int transcript_kind, int multiopen, const void* g2_128,
                     const void* s_g2_128, int* ok);
/* Succinct verification -- snark-verifier's PlonkSuccinctVerifier::verify as extract_accumulators_and_proof runs it on the
 * child snarks of an aggregation layer [REF aggregator/src/core.rs:48-107] (decider variant :111-147) -- for `count` proofs of
 * one key.  The arguments up to multiopen are zk_verify_proofs'.  acc_indices: for each of the num_prior accumulators a snark
 * of this key carries in its instances, 12 cells as {column, row} pairs (12 x num_prior x 2 words; snark-verifier's
 * accumulator_indices; limb layout of zk_host_accumulator_limbs); NULL with num_prior = 0.
 * Outputs: proof b writes 1 + num_prior accumulators at index b * (1 + num_prior) of h_lhs / h_rhs (64 B affine each, the
 * convention of zk_host_accumulator_check: e(lhs, g2) == e(rhs, s_g2)): first the accumulator of the proof's own openings,
 * then the carried ones in the order of acc_indices.  ok[b] (count entries) = 1 when proof b is well formed and every carried
 * accumulator decodes; 0, with all of that proof's outputs zeroed, for every reject reason of zk_verify_proofs, a limb of
 * 2^88 or more, a coordinate of p or more, a point off the curve, or an index outside the given instance values.  A reject
 * is ZK_OK, not an error status.
 * NO PAIRING IS DONE: ok[b] = 1 is NOT acceptance.  The caller decides each accumulator with zk_host_accumulator_check, or
 * first combines them with zk_host_accumulate and decides the result (then encodes it with zk_host_accumulator_limbs as the
 * next layer's instances).  The verdict is per proof, so this is also the way to find which proof of a batch that
 * zk_verify_proofs rejected is the bad one.
 * The points of all proofs are decoded in one launch, the proofs replayed on up to 16 host threads, and the 2 * count
 * coefficient vectors go through one zk_msm_g1_segments pass.                                                            */
int zk_verify_accumulators(zk_ctx* ctx, const zk_vk* vk, size_t count, const void* const* const* h_instances, const uint32_t* const* h_instance_lens,
                           const void* const* h_proofs, const size_t* h_proof_lens, int transcript_kind, int multiopen, const uint32_t* acc_indices,
                           size_t num_prior, void* h_lhs, void* h_rhs, int* ok);
/* Multi-GPU proving: one process per GPU, every rank runs the SAME session calls on
 * the same key, witness and seed.  Rank r then commits only columns r, r + world, ... and evaluates
 * only cosets r, r + world, ... of the quotient; commitments (64 B each) and finished cosets
 * (2^k x 32 B each) are exchanged through `gather`, so all ranks produce the same transcript and
 * the same proof bytes as an unsharded session.  gather(user, send, bytes, recv) must all-gather
 * `bytes` bytes from every rank into recv (world x bytes, rank-major) and return 0 -- e.g.
 * torch.distributed.all_gather_into_tensor over RCCL, see zkevm-circuits_amd/sharding.py.
 * Call between zk_proof_begin and the first advice phase.                                          */
typedef int (*zk_allgather_fn)(void* user, const void* h_send, size_t bytes, void* h_recv);
int zk_proof_set_sharding(zk_ctx* ctx, zk_proof* proof, uint32_t rank, uint32_t world, zk_allgather_fn gather, void* user);
/* ---- collectives inside the library: RCCL over xGMI, one process per GPU (csrc/comm.hip) ----------
 * For host languages without a collective library of their own (the Rust shim): rank 0 makes a
 * 128-byte unique id (zk_comm_unique_id) and hands it to every rank by any out-of-band channel;
 * zk_comm_init joins the communicator (ncclCommInitRank) on the context's device.  After that
 *   zk_proof_set_sharding_comm   shards a proving session over the communicator: commitments
 *                                all-gathered per transcript round, advice columns and finished
 *                                quotient cosets device to device, everything stream-ordered;
 *   zk_ntt_sharded(.., NULL, NULL) uses one grouped ncclSend / ncclRecv all-to-all;
 *   zk_comm_allgather / _alltoall  are the raw collectives over device buffers.
 * librccl is loaded on first use; a single-GPU deployment never needs it.                          */
int zk_comm_unique_id(void* out128);
int zk_comm_init(zk_ctx* ctx, const void* id128, uint32_t rank, uint32_t world);
int zk_comm_destroy(zk_ctx* ctx);
int zk_comm_allgather(zk_ctx* ctx, const void* d_send, size_t bytes, void* d_recv);
int zk_comm_alltoall(zk_ctx* ctx, const void* d_send, size_t bytes_per_peer, void* d_recv);
int zk_proof_set_sharding_comm(zk_ctx* ctx, zk_proof* proof);
/* Optional, after zk_proof_set_sharding: an all-gather of DEVICE buffers (same signature, device
 * pointers; RCCL over xGMI).  Each rank then uploads only its own 1/world of the advice columns and
 * the ranks exchange them over the fabric, instead of every rank pulling every column over its own
 * PCIe link.  The library drains its stream before each call; the callback must return only when
 * d_recv is complete.                                                                              */
int zk_proof_set_device_gather(zk_ctx* ctx, zk_proof* proof, zk_allgather_fn gather_dev, void* user);
/* commits the advice columns of the current phase (h_cols[j] = advice column col_index[j], exactly
 * the columns of that phase) and writes the challenges that become usable after it to
 * h_challenges (32 B each, Montgomery Fr, challenge-index order).  With h_challenges given,
 * *num_challenges must hold the buffer's capacity (in challenges) on entry -- a phase with more is
 * refused, nothing is written -- and receives the number written (zk_pk_shape: total challenges). */
int zk_proof_advice_phase(zk_ctx* ctx, zk_proof* proof, const uint32_t* col_index, const void* const* h_cols, uint32_t ncols,
                          void* h_challenges, uint32_t* num_challenges);
/* The same phase for witness columns RESIDENT ON THE DEVICE (device pointers, n x 32 B each, Montgomery form): a witness generated
 * on the GPU or uploaded ahead of the proof; small / dense columns are judged on the device.  Same proof bytes.  flags = 0: the
 * session copies the columns device to device into its own buffers (the caller's stay untouched).  ZK_ADVICE_DEV_IN_PLACE: the
 * session works in the caller's buffers -- it overwrites their last blinding_factors + 1 rows (halo2 puts blinding values there; a
 * witness holds nothing in them) and reads them until zk_proof_finish / zk_proof_abort returns; no copy, n x 32 B less device
 * memory per column.
 * Sharded session with a device all-gather (zk_proof_set_sharding_comm, or zk_proof_set_sharding + zk_proof_set_device_gather):
 * a rank needs only the columns it OWNS -- position j of the phase's columns in ascending column index, j % world == rank; those
 * it commits and sends to the other ranks over the fabric.  d_cols[j] of a column the rank does not own may be NULL (col_index
 * still lists every column of the phase on every rank).                                                                           */
#define ZK_ADVICE_DEV_IN_PLACE 1u
int zk_proof_advice_phase_dev(zk_ctx* ctx, zk_proof* proof, const uint32_t* col_index, const void* const* d_cols, uint32_t ncols, uint32_t flags,
                              void* h_challenges, uint32_t* num_challenges);
/* zk_proof_advice_phase for host columns given as typed cells: h_cols[j] holds n cells of widths[j] bytes each
 * (1, 2, 4, 8, 16: unsigned little-endian integers; 32: Montgomery Fr exactly as zk_proof_advice_phase takes it).
 * Same transcript, same proof bytes as passing the same values as Fr.  As there, the last blinding_factors + 1 rows are
 * the session's: whatever the caller put in them is neither uploaded nor read.
 * A column narrower than 32 crosses PCIe as usable_rows * width bytes and is expanded to Montgomery form on the device; one
 * call may mix widths.  Columns of 8 bytes or fewer take the small-value commitment path (zk_commit_batch_hint's hint 1)
 * without being sampled.  Any other width or a null `widths`: ZK_ERR_INVALID_ARG, nothing is uploaded and the phase can be
 * called again.  In a sharded session (world > 1): ZK_ERR_UNSUPPORTED.  Packed cells that are already on the device go to
 * zk_proof_advice_phase_typed_dev.                                                                                          */
int zk_proof_advice_phase_typed(zk_ctx* ctx, zk_proof* proof, const uint32_t* col_index, const void* const* h_cols, const uint8_t* widths,
                                uint32_t ncols, void* h_challenges, uint32_t* num_challenges);
/* zk_proof_advice_phase_typed for cells that are RESIDENT ON THE DEVICE (a witness kernel's output): d_cols[j] is a device pointer
 * aligned to widths[j] (8 for width 32).  widths[j] = 1, 2, 4, 8, 16: at least usable_rows (n - blinding_factors - 1) little-endian
 * unsigned cells of that width, and only those are read; widths[j] = 32: an n x 32 B Montgomery column, copied as
 * zk_proof_advice_phase_dev with flags = 0 copies it.  The rows from usable_rows on are the session's blinding values.
 * Narrow columns are expanded straight into the session's own buffers, 16 columns per launch, on the stream that orders the
 * commitments behind an upload: no n x 32 B copy on the caller's side, no staging buffer, no host synchronisation per column.
 * Columns of 8 bytes or fewer take the small-value commitment path without being sampled; 16- and 32-byte columns are judged on
 * the device.  The buffers are only read (several columns may name the same one) and not after the call returns.
 * Same transcript, same challenges, same proof bytes as zk_proof_advice_phase on the same values.
 * A bad width, a NULL or misaligned pointer, a column of another phase: ZK_ERR_INVALID_ARG, and the phase can be called again.
 * In a sharded session (world > 1): ZK_ERR_UNSUPPORTED, before any work.                                                        */
int zk_proof_advice_phase_typed_dev(zk_ctx* ctx, zk_proof* proof, const uint32_t* col_index, const void* const* d_cols, const uint8_t* widths,
                                    uint32_t ncols, void* h_challenges, uint32_t* num_challenges);
/* consumes the session (freed on success and on failure)                                         */
int zk_proof_finish(zk_ctx* ctx, zk_proof* proof, void* h_proof, size_t proof_cap, size_t* proof_len);
void zk_proof_abort(zk_ctx* ctx, zk_proof* proof);

/* ---- host-only wire formats and aggregation arithmetic (csrc/wire.hip, csrc/host_pairing.hpp) ------
 * No context, no device.  SerdeFormat codes: 0 Processed, 1 RawBytes, 2 RawBytesUnchecked.          */
/* instances <-> concatenated 32-byte big-endian words [REF prover/src/proof.rs:77-85,126-138]         */
int zk_host_instances_encode(const void* fr_mont, size_t n, void* out_be);
int zk_host_instances_decode(const void* in_be, size_t n, void* fr_mont_out);
/* The prover's `Proof` wire object [REF prover/src/proof.rs:25-35,99-104] -- the body of full_proof_<name>.json:
 * {"proof": base64, "instances": base64 of the 32-byte big-endian words (zk_host_instances_encode), "vk": base64 of
 * VerifyingKey::write(Processed) (zk_host_vk_write), "git_version": string or null}, serde_json's compact form in the struct's
 * field order; base64 as [REF eth-types/src/lib.rs:71-91] (standard alphabet, padded).  write: out may be NULL (size query);
 * git_version NULL = null.  read: accepts compact or pretty JSON with the four keys in any order (git_version may be absent);
 * every output buffer is optional, the *_len arguments hold capacities on entry and lengths on return.  The objects built
 * around it -- ChunkProof / BatchProof with snark-verifier's `protocol` -- stay on the Rust side. */
int zk_host_proof_json_write(const void* proof, size_t proof_len, const void* instances_be, size_t instances_len, const void* vk, size_t vk_len,
                             const char* git_version, char* out, size_t cap, size_t* len);
int zk_host_proof_json_read(const char* json, size_t json_len, void* proof, size_t* proof_len, void* instances_be, size_t* instances_len, void* vk, size_t* vk_len,
                            char* git_version, size_t git_cap, int* has_git_version);
/* Instances as the prover's JSON matrix [REF prover/src/io.rs:28-56]: `serialize_instance` = serde_json (compact) of
 * Vec<Vec<Vec<u8>>> -- per instance column a list of elements, each the 32 little-endian bytes of Fr::to_bytes as numbers.
 * (`load_instances` [REF prover/src/io.rs:128-142] holds a list of such matrices: one more pair of brackets.)  write: out may
 * be NULL (size query).  read: NULL outputs = counts only; values of all columns one after the other, Montgomery Fr. */
int zk_host_instances_json_write(const void* const* cols_fr_mont, const size_t* lens, size_t ncols, char* out, size_t cap, size_t* len);
int zk_host_instances_json_read(const char* json, size_t json_len, size_t* ncols, size_t* lens_out, size_t lens_cap, void* fr_mont_out, size_t fr_cap, size_t* total);
/* G1 points in halo2curves' SerdeFormat: 32 B compressed (Processed) or 64 B Montgomery limbs       */
int zk_host_g1_encode(const void* affine64, size_t n, int format, void* out);
int zk_host_g1_decode(const void* in, size_t n, int format, void* affine64_out);
/* halo2 VerifyingKey::write / read [REF prover/src/io.rs:97-106]: k and the commitment count as u32
 * big-endian, fixed then permutation commitments, then the selector assignments packed 8 rows/byte  */
int zk_host_vk_write(uint32_t k, const void* fixed_commitments, uint32_t num_fixed, const void* perm_commitments, uint32_t num_perm,
                     const uint8_t* selectors_packed, uint32_t num_selectors, int format, void* out, size_t cap, size_t* len);
int zk_host_vk_read(const void* in, size_t in_len, int format, uint32_t num_perm, uint32_t num_selectors, uint32_t* k, uint32_t* num_fixed,
                    void* fixed_commitments, size_t fixed_cap, void* perm_commitments, uint8_t* selectors_packed);
/* BN254 optimal-ate pairing product: prod e(P_i, Q_i) == 1 ?  (G2: 128 B = x.c0, x.c1, y.c0, y.c1)   */
int zk_host_pairing_check(const void* g1_points, const void* g2_points, size_t n, int* ok);
/* aggregation layers between two GPU proofs [REF aggregator/src/core.rs:48-147]: combine the child
 * snarks' KZG accumulators with powers of a Poseidon-transcript challenge (KzgAs::create_proof,
 * no blinding), decide e(lhs, g2) == e(rhs, s_g2), encode the result as 12 limbs of 88 bits          */
int zk_host_accumulate(const void* lhs_in, const void* rhs_in, size_t n, void* lhs_out, void* rhs_out, void* r_out);
int zk_host_accumulator_check(const void* lhs, const void* rhs, const void* g2, const void* s_g2, int* ok);
int zk_host_accumulator_limbs(const void* lhs, const void* rhs, void* out12_fr);
/* the inverse (LimbsEncoding::from_repr [REF aggregator/src/core.rs:120-135]): 12 Montgomery Fr cells -> lhs, rhs.  *ok = 0 and
 * both points zeroed for a limb of 2^88 or more, a coordinate of p or more, or a point off the curve (ZK_OK either way)   */
int zk_host_accumulator_from_limbs(const void* limbs12_fr, void* lhs, void* rhs, int* ok);

/* ---- G1 element-wise (tests of the group law; halo2curves G1 Add / Double / Mul) --------------- */
/* out[i] = a[i] + b[i], all affine (n x 64 B) */
int zk_g1_affine_add_vec(zk_ctx* ctx, const void* d_a, const void* d_b, void* d_out, size_t n);
/* out[i] = scalars[i] * bases[i], affine out */
int zk_g1_mul_vec(zk_ctx* ctx, const void* d_bases, const void* d_scalars, void* d_out, size_t n);

/* ---- introspection ------------------------------------------------------------------------------ */
const char* zk_version(void);
/* fills name (<= len) with the device name, CU count and HBM bytes of the ctx device */
int zk_device_info(zk_ctx* ctx, char* name, size_t len, int* cu_count, size_t* hbm_bytes);

#ifdef __cplusplus
}
#endif
#endif /* ZKMI355_H */

"""ctypes binding of libzkmi355.so (the C ABI in include/zkmi355.h) for tests and bench.py.

This is test/bench plumbing over the product library: the reference's host language (Rust) is not
available in this image, so the production host side is the C++ layer in ``csrc/``; see
INTEGRATION.md for the Rust ``extern "C"`` block a maintainer would add.

There is NO CPU fallback: if the shared library or a gfx950 device is missing, loading /
context creation raises.
"""
from __future__ import annotations

import ctypes
import os
import subprocess
from typing import Optional, Sequence, Tuple

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libzkmi355.so")
HEADER_PATH = os.path.join(_HERE, "..", "include", "zkmi355.h")

FIELD_FR, FIELD_FQ = 0, 1
OP_ADD, OP_SUB, OP_MUL = 0, 1, 2
OP_SCAN_AFFINE, OP_SCAN_AFFINE_REV = 3, 4            # out[i] = a[i] * out[i -+ 1] + b[i] along the column, Fr only
OP_ROW_RLC = 8                                        # out[i] = c + sum_j w_j * cell_j[i] across typed columns, Fr only (ZK_OP_ROW_RLC)
OP_SCAN_RLC, OP_SCAN_RLC_REV = 9, 10                 # out[i] = m[kind_i] * out[i -+ 1] + w[kind_i] * cell[i] along a typed column, Fr only
OP_ROW_INV0 = 12                                      # out[i] = num[i] * inv0(c + sum_j w_j * cell_j[i]) across typed columns, Fr only (ZK_OP_ROW_INV0)
OP_POSEIDON = 14                                      # out[i] = permute(state of row i)[0], width-3 Poseidon over typed cells, Fr only (ZK_OP_POSEIDON)
POSEIDON_FINAL = 1                                    # zk_poseidon.flags: every row of a message holds the hash of its last row
OP_KECCAK = 16                                        # out[i] = output_rlc of Keccak-256(message i), messages as bytes on the device, Fr only (ZK_OP_KECCAK)
OP_SHA256 = 18                                        # out[i] = output_rlc of SHA-256(message i), messages as bytes on the device, Fr only (ZK_OP_SHA256)
OP_KEY_SORT = 20                                      # out[i] = index of the 64-byte key record at place i of the stable order (ZK_OP_KEY_SORT)
OP_KEY_ORDER = 22                                     # out[i] = limb_difference_inverse of key records i and i - 1 in row order (ZK_OP_KEY_ORDER)
OP_BYTECODE_ROWS = 26                                 # out[i] = the code hash of the bytecode that row i of the bytecode circuit belongs to (ZK_OP_BYTECODE_ROWS)
OP_COPY_ROWS = 28                                     # out[i] = the addr cell (8 bytes) of row i of the copy circuit, from copy events on the device (ZK_OP_COPY_ROWS)
OP_COPY_RLC = 30                                      # out[i] = value_acc of row i of the copy circuit (ZK_OP_COPY_RLC)
OP_EXP_ROWS = 32                                      # out[i] = the exponentiation_lo_hi cell (16 bytes) of row i of the exponentiation circuit (ZK_OP_EXP_ROWS)
OP_CODE_HASH_ROWS = 34                                # out[i] = field_input of row i of the bytecode circuit's Poseidon-hash extension (ZK_OP_CODE_HASH_ROWS)
OP_CODE_HASH_TABLE = 36                               # out[i] = input0 of code-hash row i of the Poseidon table (ZK_OP_CODE_HASH_TABLE)
# quotient-program opcodes (csrc/quotient.hip)
Q_END, Q_PUSH_COL, Q_PUSH_CONST, Q_ADD, Q_SUB, Q_MUL, Q_NEG, Q_SQUARE, Q_DOUBLE, Q_FOLD, Q_MUL_CONST, Q_ADD_CONST, Q_TEE_TMP, Q_PUSH_TMP = range(14)

_lib = None


class ZkError(RuntimeError):
    pass


def build(force: bool = False) -> str:
    """Compile every HIP source for gfx950 into lib/libzkmi355.so (hipcc cross-compiles without a GPU)."""
    args = ["make", "-C", _HERE, "-j8", "-s"]
    if force:
        subprocess.check_call(["make", "-C", _HERE, "-s", "clean"])
    subprocess.check_call(args)
    return LIB_PATH


def lib():
    global _lib
    if _lib is None:
        path = os.environ.get("ZKMI355_LIB", LIB_PATH)       # A/B measurements against another build of the library
        if not os.path.exists(path):
            raise ZkError(f"{path} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` (no CPU fallback exists)")
        _lib = ctypes.CDLL(path)
        _lib.zk_last_error.restype = ctypes.c_char_p
        _lib.zk_version.restype = ctypes.c_char_p
        _lib.zk_srs_g.restype = ctypes.c_void_p
        _lib.zk_srs_g_lagrange.restype = ctypes.c_void_p
        _lib.zk_srs_k.restype = ctypes.c_uint32
        _lib.zk_params_file_len.restype = ctypes.c_size_t
        _lib.zk_ctx_destroy.restype = None
        _lib.zk_srs_destroy.restype = None
        _lib.zk_pk_destroy.restype = None
        _lib.zk_proof_abort.restype = None
        _lib.zk_transcript_new.restype = ctypes.c_void_p
        _lib.zk_transcript_free.restype = None
        _lib.zk_transcript_free.argtypes = [ctypes.c_void_p]
        _lib.zk_transcript_proof.restype = ctypes.c_size_t
        _lib.zk_vk_destroy.restype = None
        _lib.zk_vk_destroy.argtypes = [ctypes.c_void_p]
        vpp, u8p, u32p = ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(ctypes.c_uint32)
        _lib.zk_fr_from_uint_batch.restype = ctypes.c_int
        _lib.zk_fr_from_uint_batch.argtypes = [ctypes.c_void_p, vpp, u8p, ctypes.c_size_t, ctypes.c_size_t, vpp]
        _lib.zk_proof_advice_phase_typed_dev.restype = ctypes.c_int
        _lib.zk_proof_advice_phase_typed_dev.argtypes = [ctypes.c_void_p, ctypes.c_void_p, u32p, vpp, u8p, ctypes.c_uint32, ctypes.c_void_p, u32p]
    return _lib


class _RowRlc(ctypes.Structure):
    """zk_row_rlc: the column table of ZK_OP_ROW_RLC (host memory)"""
    _fields_ = [("count", ctypes.c_uint32), ("d_cols", ctypes.POINTER(ctypes.c_void_p)), ("widths", ctypes.POINTER(ctypes.c_uint8))]


class _ScanRlc(ctypes.Structure):
    """zk_scan_rlc: the cells and kinds of ZK_OP_SCAN_RLC / ZK_OP_SCAN_RLC_REV (host memory; both pointers are device pointers)"""
    _fields_ = [("d_cells", ctypes.c_void_p), ("width", ctypes.c_uint32), ("d_kinds", ctypes.c_void_p)]


class _RowInv0(ctypes.Structure):
    """zk_row_inv0: the column table and the numerator of ZK_OP_ROW_INV0 (host memory; d_num is a device pointer or NULL)"""
    _fields_ = [("count", ctypes.c_uint32), ("d_cols", ctypes.POINTER(ctypes.c_void_p)), ("widths", ctypes.POINTER(ctypes.c_uint8)),
                ("d_num", ctypes.c_void_p), ("num_width", ctypes.c_uint32)]


class _Poseidon(ctypes.Structure):
    """zk_poseidon: the columns of ZK_OP_POSEIDON (host memory; every pointer is a device pointer or NULL)"""
    _fields_ = [("d_in0", ctypes.c_void_p), ("d_in1", ctypes.c_void_p), ("d_cap", ctypes.c_void_p), ("d_kinds", ctypes.c_void_p),
                ("d_word0", ctypes.c_void_p), ("d_word1", ctypes.c_void_p),
                ("width0", ctypes.c_uint8), ("width1", ctypes.c_uint8), ("cap_width", ctypes.c_uint8), ("flags", ctypes.c_uint8)]


class _Keccak(ctypes.Structure):
    """zk_keccak: the messages and optional outputs of ZK_OP_KECCAK (host memory; every pointer is a device pointer or NULL)"""
    _fields_ = [("d_bytes", ctypes.c_void_p), ("total_bytes", ctypes.c_uint64), ("d_offsets", ctypes.c_void_p), ("d_lens", ctypes.c_void_p),
                ("d_digest", ctypes.c_void_p), ("d_input_rlc", ctypes.c_void_p), ("index_width", ctypes.c_uint8), ("flags", ctypes.c_uint8)]


class _Sha256(ctypes.Structure):
    """zk_sha256: the messages and optional outputs of ZK_OP_SHA256, member for member zk_keccak (host memory; every pointer is a
    device pointer or NULL)"""
    _fields_ = [("d_bytes", ctypes.c_void_p), ("total_bytes", ctypes.c_uint64), ("d_offsets", ctypes.c_void_p), ("d_lens", ctypes.c_void_p),
                ("d_digest", ctypes.c_void_p), ("d_input_rlc", ctypes.c_void_p), ("index_width", ctypes.c_uint8), ("flags", ctypes.c_uint8)]


class _KeySort(ctypes.Structure):
    """zk_key_sort: the records and the optional sorted copy of ZK_OP_KEY_SORT (host memory; both pointers are device pointers)"""
    _fields_ = [("d_keys", ctypes.c_void_p), ("d_sorted", ctypes.c_void_p), ("flags", ctypes.c_uint8)]


class _KeyCol(ctypes.Structure):
    """zk_key_col: key bytes [offset, offset + width) of a gathered column of ZK_OP_KEY_ORDER"""
    _fields_ = [("offset", ctypes.c_uint8), ("width", ctypes.c_uint8)]


class _KeyOrder(ctypes.Structure):
    """zk_key_order: the records, the row order and the outputs of ZK_OP_KEY_ORDER (host memory; cols and d_cols are host arrays, every
    other pointer is a device pointer or NULL)"""
    _fields_ = [("d_keys", ctypes.c_void_p), ("d_perm", ctypes.c_void_p), ("d_diff", ctypes.c_void_p), ("d_index", ctypes.c_void_p),
                ("d_bits", ctypes.c_void_p), ("d_not_first", ctypes.c_void_p), ("group_limbs", ctypes.c_uint32), ("count", ctypes.c_uint32),
                ("cols", ctypes.POINTER(_KeyCol)), ("d_cols", ctypes.POINTER(ctypes.c_void_p)), ("flags", ctypes.c_uint8)]


class _BytecodeRows(ctypes.Structure):
    """zk_bytecode_rows: the code bytes, the code hashes and the outputs of ZK_OP_BYTECODE_ROWS (host memory; every pointer is a device
    pointer or NULL)"""
    _fields_ = [("d_bytes", ctypes.c_void_p), ("total_bytes", ctypes.c_uint64), ("d_offsets", ctypes.c_void_p), ("d_lens", ctypes.c_void_p),
                ("d_hashes", ctypes.c_void_p), ("d_tag", ctypes.c_void_p), ("d_index", ctypes.c_void_p), ("d_value", ctypes.c_void_p),
                ("d_is_code", ctypes.c_void_p), ("d_push_data_left", ctypes.c_void_p), ("d_push_data_size", ctypes.c_void_p),
                ("d_length", ctypes.c_void_p), ("d_acc_kinds", ctypes.c_void_p), ("d_rlc_kinds", ctypes.c_void_p),
                ("count", ctypes.c_uint32), ("index_width", ctypes.c_uint8), ("flags", ctypes.c_uint8)]


COPY_ROWS_OUTPUTS = ("is_first", "is_last", "tag", "tag_bits", "value", "value_prev", "mask", "front_mask", "word_index", "src_addr_end", "is_pad", "non_pad_non_mask",
                     "real_bytes_left", "rw_counter", "rwc_inc_left", "types", "src_end_rows")
COPY_RLC_OUTPUTS = ("id", "id_other", "rlc_acc", "word_rlc", "word_rlc_prev")


class _CopyEvent(ctypes.Structure):
    """zk_copy_event: the 88-byte record of one copy event (device data; the host never reads it)"""
    _fields_ = [(name, ctypes.c_uint64) for name in ("src_addr", "src_addr_end", "dst_addr", "dst_addr_bias", "rw_counter", "src_off", "dst_off", "prev_off")] + \
               [(name, ctypes.c_uint32) for name in ("length", "src_front", "src_back", "dst_front", "dst_back")] + \
               [(name, ctypes.c_uint8) for name in ("src_tag", "dst_tag", "flags", "reserved")]


_COPY_SHARED = [("d_events", ctypes.c_void_p), ("count", ctypes.c_uint32), ("d_bytes", ctypes.c_void_p), ("total_bytes", ctypes.c_uint64), ("flags", ctypes.c_uint8)]


class _CopyRows(ctypes.Structure):
    """zk_copy_rows: the events, the byte heap and the typed outputs of ZK_OP_COPY_ROWS (host memory; every pointer is a device pointer
    or NULL)"""
    _fields_ = _COPY_SHARED + [("d_" + name, ctypes.c_void_p) for name in COPY_ROWS_OUTPUTS]


class _CopyRlc(ctypes.Structure):
    """zk_copy_rlc: the events, the byte heap, the ids and the outputs of ZK_OP_COPY_RLC"""
    _fields_ = _COPY_SHARED + [("d_ids", ctypes.c_void_p)] + [("d_" + name, ctypes.c_void_p) for name in COPY_RLC_OUTPUTS]


EXP_ROWS_OUTPUTS = ("is_last", "base_limb", "exponent_lo_hi", "mul_cols", "mul_u16_64", "mul_u16_128", "parity_cols", "parity_u16_64", "parity_u16_128", "rows_needed")


class _ExpEvent(ctypes.Structure):
    """zk_exp_event: the 64-byte record of one exponentiation event (device data; the host never reads it)"""
    _fields_ = [("base", ctypes.c_uint64 * 4), ("exponent", ctypes.c_uint64 * 4)]


class _ExpRows(ctypes.Structure):
    """zk_exp_rows: the events and the typed outputs of ZK_OP_EXP_ROWS (host memory; every pointer is a device pointer or NULL)"""
    _fields_ = [("d_events", ctypes.c_void_p), ("count", ctypes.c_uint32), ("flags", ctypes.c_uint8)] + [("d_" + name, ctypes.c_void_p) for name in EXP_ROWS_OUTPUTS]


CODE_HASH_ROWS_OUTPUTS = ("control_length", "bytes_in_field_index", "bytes_in_field_inv", "is_field_border", "padding_shift", "field_index", "field_index_inv")
CODE_HASH_TABLE_OUTPUTS = ("input1", "control", "heading_mark", "kinds", "cap", "rows_needed")
_CODE_HASH_SHARED = [("d_bytes", ctypes.c_void_p), ("total_bytes", ctypes.c_uint64), ("d_offsets", ctypes.c_void_p), ("d_lens", ctypes.c_void_p)]
_CODE_HASH_TAIL = [("count", ctypes.c_uint32), ("index_width", ctypes.c_uint8), ("flags", ctypes.c_uint8)]


class _CodeHashRows(ctypes.Structure):
    """zk_code_hash_rows: the code bytes and the typed outputs of ZK_OP_CODE_HASH_ROWS (host memory; every pointer is a device pointer
    or NULL)"""
    _fields_ = _CODE_HASH_SHARED + [("d_" + name, ctypes.c_void_p) for name in CODE_HASH_ROWS_OUTPUTS] + _CODE_HASH_TAIL


class _CodeHashTable(ctypes.Structure):
    """zk_code_hash_table: the code bytes and the outputs of ZK_OP_CODE_HASH_TABLE"""
    _fields_ = _CODE_HASH_SHARED + [("d_" + name, ctypes.c_void_p) for name in CODE_HASH_TABLE_OUTPUTS] + _CODE_HASH_TAIL


def _host_ptr(a: np.ndarray):
    assert a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(ctypes.c_void_p)


def typed_cell_width(a: np.ndarray) -> int:
    """bytes per cell of a typed witness column (zk_proof_advice_phase_typed, zk_fr_from_uint): 1, 2, 4, 8 for a one-dimensional
    uint8 / uint16 / uint32 / uint64 array, 16 for (n, 2) uint64 (low word first), 32 for (n, 4) uint64 (Montgomery Fr)"""
    a = np.asarray(a)
    if a.ndim == 1 and a.dtype in (np.uint8, np.uint16, np.uint32, np.uint64):
        return a.dtype.itemsize
    if a.ndim == 2 and a.dtype == np.uint64 and a.shape[1] in (2, 4):
        return 8 * a.shape[1]
    raise ZkError(f"not a typed witness column: dtype {a.dtype}, shape {a.shape} (uint8/16/32/64 of shape (n,), or uint64 of shape (n, 2) or (n, 4))")


class DeviceBuffer:
    """Owning handle of a device allocation made through the C ABI."""

    def __init__(self, ctx: "Context", nbytes: int):
        self.ctx = ctx
        self.nbytes = nbytes
        p = ctypes.c_void_p()
        ctx._ck(lib().zk_buf_alloc(ctx.h, ctypes.c_size_t(nbytes), ctypes.byref(p)))
        self.ptr = p.value

    def free(self):
        if self.ptr:
            lib().zk_buf_free(self.ctx.h, ctypes.c_void_p(self.ptr))
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass

    def upload(self, a: np.ndarray):
        a = np.ascontiguousarray(a)
        assert a.nbytes <= self.nbytes
        self.ctx._ck(lib().zk_h2d(self.ctx.h, ctypes.c_void_p(self.ptr), _host_ptr(a), ctypes.c_size_t(a.nbytes)))
        return self

    def download(self, shape, dtype=np.uint64) -> np.ndarray:
        out = np.empty(shape, dtype=dtype)
        assert out.nbytes <= self.nbytes
        self.ctx._ck(lib().zk_d2h(self.ctx.h, _host_ptr(out), ctypes.c_void_p(self.ptr), ctypes.c_size_t(out.nbytes)))
        return out


class Srs:
    def __init__(self, ctx: "Context", handle):
        self.ctx, self.h = ctx, handle

    @property
    def k(self) -> int:
        return lib().zk_srs_k(self.h)

    @property
    def g_ptr(self) -> int:
        return lib().zk_srs_g(self.h)

    @property
    def g_lagrange_ptr(self) -> Optional[int]:
        return lib().zk_srs_g_lagrange(self.h)

    def downsize(self, new_k: int) -> "Srs":
        """ParamsKZG::downsize: first 2^new_k points of g, Lagrange basis recomputed on the device."""
        h = ctypes.c_void_p()
        self.ctx._ck(lib().zk_srs_downsize(self.ctx.h, self.h, ctypes.c_uint32(new_k), ctypes.byref(h)))
        return Srs(self.ctx, h)

    def download_g(self) -> np.ndarray:
        n = 1 << self.k
        out = np.empty((n, 8), dtype=np.uint64)
        self.ctx._ck(lib().zk_d2h(self.ctx.h, _host_ptr(out), ctypes.c_void_p(self.g_ptr), ctypes.c_size_t(out.nbytes)))
        return out

    def download_g_lagrange(self) -> np.ndarray:
        n = 1 << self.k
        out = np.empty((n, 8), dtype=np.uint64)
        self.ctx._ck(lib().zk_d2h(self.ctx.h, _host_ptr(out), ctypes.c_void_p(self.g_lagrange_ptr), ctypes.c_size_t(out.nbytes)))
        return out

    def destroy(self):
        if self.h:
            lib().zk_srs_destroy(self.ctx.h, self.h)
            self.h = None


class ProvingKey:
    def __init__(self, ctx: "Context", handle):
        self.ctx, self.h = ctx, handle

    def vk(self, num_commitments: int):
        """(commitments (num, 8) u64 affine Montgomery, vk_repr (4,) u64 Montgomery)."""
        com = np.zeros((max(num_commitments, 1), 8), dtype=np.uint64)
        rep = np.zeros(4, dtype=np.uint64)
        self.ctx._ck(lib().zk_pk_vk(self.ctx.h, self.h, _host_ptr(com), _host_ptr(rep)))
        return com[:num_commitments], rep

    def set_transcript_repr(self, repr_mont: np.ndarray):
        """install halo2's `vk.transcript_repr()` ((4,) u64 Montgomery Fr): the first scalar every proof absorbs"""
        r = np.ascontiguousarray(repr_mont, dtype=np.uint64).reshape(4)
        self.ctx._ck(lib().zk_pk_set_transcript_repr(self.ctx.h, self.h, _host_ptr(r)))

    def shape(self) -> dict:
        out = (ctypes.c_uint32 * 16)()
        self.ctx._ck(lib().zk_pk_shape(self.ctx.h, self.h, out))
        names = ["k", "degree", "extended_k", "F", "A", "I", "P", "C", "L", "phases", "challenges", "blinding_factors",
                 "advice_queries", "fixed_queries", "commitments", "evaluations"]
        return dict(zip(names, list(out)))

    def quotient_plan(self) -> dict:
        """how the key's constraints are dealt to degree classes and what each class's compiled program costs (zk_pk_quotient_plan)"""
        out = (ctypes.c_uint32 * (8 + 8 * 16))()
        self.ctx._ck(lib().zk_pk_quotient_plan(self.ctx.h, self.h, out, ctypes.c_size_t(len(out))))
        return plan_summary(list(out))

    def destroy(self):
        if self.h:
            lib().zk_pk_destroy(self.ctx.h, self.h)
            self.h = None


class VerifyingKey:
    """halo2 VerifyingKey (zk_vk): the constraint system of a key blob with the key's commitments and vk_repr; host only.
    From `cs_blob` (plonk.Circuit.cs_blob(): a shape-only circuit is enough), the F fixed then P sigma commitments ((F + P, 8)
    u64 affine Montgomery) and vk_repr ((4,) u64 Montgomery) -- or from a ProvingKey (from_pk)."""

    SHAPE_NAMES = ["k", "degree", "extended_k", "F", "A", "I", "P", "C", "L", "phases", "challenges", "blinding_factors",
                   "advice_queries", "fixed_queries", "commitments", "evaluations"]

    def __init__(self, cs_blob: bytes, commitments: np.ndarray, vk_repr: np.ndarray):
        blob = cs_blob if isinstance(cs_blob, np.ndarray) else np.frombuffer(cs_blob, dtype=np.uint8)     # read by pointer, no copy
        com = np.ascontiguousarray(commitments, dtype=np.uint64).reshape(-1, 8)
        rep = np.ascontiguousarray(vk_repr, dtype=np.uint64).reshape(4)
        h = ctypes.c_void_p()
        rc = lib().zk_vk_create(_host_ptr(blob), ctypes.c_size_t(blob.size), _host_ptr(com) if len(com) else None, ctypes.c_size_t(len(com)),
                                _host_ptr(rep), ctypes.byref(h))
        if rc != 0:
            raise ZkError(f"zk_vk_create failed with status {rc} (truncated or malformed constraint system, or F + P commitments expected)")
        self.h = h
        self.shape_ = self.shape()

    @classmethod
    def from_pk(cls, pk: "ProvingKey", cs_blob: bytes) -> "VerifyingKey":
        """the verifying key of a proving key made from a blob whose constraint-system part is cs_blob"""
        sh = pk.shape()
        com, rep = pk.vk(sh["F"] + sh["P"])
        return cls(cs_blob, com, rep)

    def shape(self) -> dict:
        out = (ctypes.c_uint32 * 16)()
        rc = lib().zk_vk_shape(self.h, out)
        if rc != 0:
            raise ZkError(f"zk_vk_shape failed with status {rc}")
        return dict(zip(self.SHAPE_NAMES, list(out)))

    def proof_len(self, transcript_kind: int = 0, multiopen: int = 0) -> int:
        n = ctypes.c_size_t()
        rc = lib().zk_vk_proof_len(self.h, ctypes.c_int(transcript_kind), ctypes.c_int(multiopen), ctypes.byref(n))
        if rc != 0:
            raise ZkError(f"zk_vk_proof_len failed with status {rc}")
        return n.value

    def destroy(self):
        if self.h:
            lib().zk_vk_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass


def plan_summary(words) -> dict:
    """the summary words of zk_host_quotient_plan / zk_pk_quotient_plan as a dict"""
    E = int(words[0])
    names = ("used", "instructions", "products", "columns", "values_parked", "slots_alive", "factor_groups", "last")
    return {"classes_E": E, "constraints": int(words[1]), "degree_classes": int(words[2]), "additive_split": int(words[3]), "expression_graph": int(words[4]),
            "remainders": int(words[5]), "cost_estimate": int(words[6]), "columns": int(words[7]),
            "classes": [dict(zip(names, (int(v) for v in words[8 + 8 * e:16 + 8 * e]))) for e in range(E + 1)]}


NTT_PLAN_FIELDS = ("kind", "pass", "passes", "log_np", "log_m", "log_t", "blocks", "grid_x", "grid_y", "threads", "lds", "fixed", "xcd", "log_grp")


def host_ntt_plan(log_n: int, columns: int = 1, tables: bool = True, coset_pass: bool = False) -> dict:
    """zk_host_ntt_plan (no device): the launches of one launch group of a transform under the ZK_NTT_* knobs in force;
    kind is "strided" or "last", fixed / xcd are bools"""
    head, recs, cnt = (ctypes.c_uint32 * 4)(), (ctypes.c_uint32 * (3 * len(NTT_PLAN_FIELDS)))(), ctypes.c_uint32()
    rc = lib().zk_host_ntt_plan(ctypes.c_uint32(log_n), ctypes.c_size_t(columns), ctypes.c_int(1 if tables else 0), ctypes.c_int(1 if coset_pass else 0),
                                head, recs, ctypes.c_size_t(3), ctypes.byref(cnt))
    if rc != 0:
        raise ZkError(f"zk_host_ntt_plan({log_n}, {columns}) failed with status {rc}")
    w = len(NTT_PLAN_FIELDS)
    launches = [dict(zip(NTT_PLAN_FIELDS, recs[i * w:(i + 1) * w])) for i in range(cnt.value)]
    for r in launches:
        r["kind"], r["fixed"], r["xcd"] = ("strided", "last")[r["kind"]], bool(r["fixed"]), bool(r["xcd"])
    return {"per_launch": head[0], "columns": head[1], "passes": head[2], "tables": bool(head[3]), "launches": launches}


QUOTIENT_LAUNCH_HEAD = ("kernel", "records", "full", "acc_in_mem", "sliced", "S", "depth", "lds", "num_tmp", "low_len", "folds", "words_per_instr", "comb_at", "slice_tab_at",
                        "prog_bytes", "col_bytes", "const_bytes", "tile_alias")


def host_quotient_launch(prog, num_cols: int, num_consts: int, ext_k: int, records: bool = False) -> dict:
    """zk_host_quotient_launch (no device): the launch plan of a postfix program [(op, a, b), ...] under the ZK_QUOTIENT_* knobs in force -- the head's
    fields by name (full, acc_in_mem, sliced, records as bools) and `words`, the program region of the upload"""
    flat = [int(x) & 0xFFFFFFFF for ins in prog for x in ins]
    n = len(flat) // 3
    words = (ctypes.c_uint32 * max(len(flat), 1))(*flat)
    head, cnt = (ctypes.c_uint32 * len(QUOTIENT_LAUNCH_HEAD))(), ctypes.c_size_t()
    out = (ctypes.c_uint32 * (32 * (n + 16)))()       # room: at most 2 n lowered instructions of 4 words, and 22 words of END records, combining step and table entry per slice (two folds at least)
    rc = lib().zk_host_quotient_launch(words, ctypes.c_uint32(n), ctypes.c_uint32(num_cols), ctypes.c_uint32(num_consts), ctypes.c_uint32(ext_k), ctypes.c_int(1 if records else 0),
                                       head, out, ctypes.c_size_t(len(out)), ctypes.byref(cnt))
    if rc != 0:
        err = ZkError(f"zk_host_quotient_launch({n} instructions, 2^{ext_k} rows) failed with status {rc}")
        err.status = rc         # the status zk_quotient_eval would return for the program
        raise err
    plan = dict(zip(QUOTIENT_LAUNCH_HEAD, head))
    for name in ("records", "full", "acc_in_mem", "sliced"):
        plan[name] = bool(plan[name])
    plan["words"] = list(out[:cnt.value])
    return plan


MSM_BATCH_PLAN_HEAD = ("status", "any_narrow", "tail_rows", "n_narrow", "n_pad", "NG", "gm", "SG", "range_bits_G", "bpcG", "perm_G", "nwgG", "words_N", "words_G", "words_M", "words",
                       "copies", "binsort", "range_bits", "chunk", "staged_scatter", "nwg", "npipe", "graph", "npts29", "smaller_cap", "c", "W", "top_shift", "c_n", "W_n", "red_blocks_N")
MSM_SORT_REGIONS = ("slice_counts", "slice_off", "counts", "cleared", "offsets", "order", "ntasks", "toff", "block_tot_s", "block_tot", "block_tot_h", "hist", "hist_off", "idx", "dig", "entries")
MSM_BUCKET_REGIONS = ("buckets", "partial", "task_partial", "folded")
MSM_STEP_KINDS = ("window", "dense", "dense_sliced", "gm")


def host_msm_batch_plan_words(k: int, n: int, count: int, hints=None, blinded_tail: int = 0, window_table: bool = True, group_cap: int = 0,
                              prof_on: bool = False, graph_broken: bool = False) -> list:
    """zk_host_msm_batch_plan (no device): the raw record, a list of ints"""
    hb = bytes(hints) if hints is not None else None
    if hb is not None and len(hb) != count:
        raise ZkError(f"{len(hb)} hints for {count} columns")
    out, cnt = (ctypes.c_uint64 * (512 + 3 * count))(), ctypes.c_size_t()      # head, <= 43 regions of three words, the steps, the key part
    rc = lib().zk_host_msm_batch_plan(ctypes.c_uint32(k), ctypes.c_size_t(n), ctypes.c_size_t(count), hb, ctypes.c_uint32(blinded_tail), ctypes.c_int(1 if window_table else 0),
                                      ctypes.c_uint32(group_cap), ctypes.c_int(1 if prof_on else 0), ctypes.c_int(1 if graph_broken else 0), out, ctypes.c_size_t(len(out)), ctypes.byref(cnt))
    if rc != 0:
        raise ZkError(f"zk_host_msm_batch_plan({k}, {n}, {count}) failed with status {rc}")
    return list(out[:cnt.value])


def host_msm_batch_plan(*args, **kwargs) -> dict:
    """zk_host_msm_batch_plan as a dict: the head's fields by name, `sort` (layouts "N", "G", "M": words and regions name -> (offset, length)),
    `buckets` (per step kind: nb, tasks, points, regions), `steps` [(first, columns, kind)] and `key` (the plan's part of a graph key)"""
    w = host_msm_batch_plan_words(*args, **kwargs)
    plan = dict(zip(MSM_BATCH_PLAN_HEAD, w))
    for name in ("any_narrow", "gm", "binsort", "staged_scatter", "graph"):
        plan[name] = bool(plan[name])
    plan.update(sort={}, buckets={}, steps=[], key=[])
    if plan["status"]:
        return plan
    at = len(MSM_BATCH_PLAN_HEAD)

    def regions(names):
        nonlocal at
        total, cnt = w[at], w[at + 1]
        regs = {names[w[at + 2 + 3 * i]]: (w[at + 3 + 3 * i], w[at + 4 + 3 * i]) for i in range(cnt)}
        at += 2 + 3 * cnt
        return total, regs
    for layout in "NGM":
        words, regs = regions(MSM_SORT_REGIONS)
        plan["sort"][layout] = {"words": words, "regions": regs}
    for kind in MSM_STEP_KINDS:
        nb, tasks = w[at], w[at + 1]
        at += 2
        points, regs = regions(MSM_BUCKET_REGIONS)
        if regs:
            plan["buckets"][kind] = {"nb": nb, "tasks": tasks, "points": points, "regions": regs}
    nsteps = w[at]
    plan["steps"] = [(w[at + 1 + 3 * i], w[at + 2 + 3 * i], MSM_STEP_KINDS[w[at + 3 + 3 * i]]) for i in range(nsteps)]
    at += 1 + 3 * nsteps
    plan["key"] = w[at + 1:at + 1 + w[at]]
    return plan


TRANSCRIPT_BLAKE2B, TRANSCRIPT_POSEIDON, TRANSCRIPT_EVM = 0, 1, 2


class HostTranscript:
    """zk_transcript: the library's Blake2b / Poseidon / EVM transcript as a host-only object (no GPU)."""

    def __init__(self, kind: int):
        self.h = lib().zk_transcript_new(ctypes.c_int(kind))
        if not self.h:
            raise ZkError(f"unknown transcript kind {kind}")

    def _ck(self, rc):
        if rc != 0:
            raise ZkError(f"transcript operation failed with status {rc}")

    def common_point(self, affine64: bytes): self._ck(lib().zk_transcript_common_point(ctypes.c_void_p(self.h), ctypes.c_char_p(bytes(affine64))))
    def common_scalar(self, fr32: bytes): self._ck(lib().zk_transcript_common_scalar(ctypes.c_void_p(self.h), ctypes.c_char_p(bytes(fr32))))
    def write_point(self, affine64: bytes): self._ck(lib().zk_transcript_write_point(ctypes.c_void_p(self.h), ctypes.c_char_p(bytes(affine64))))
    def write_scalar(self, fr32: bytes): self._ck(lib().zk_transcript_write_scalar(ctypes.c_void_p(self.h), ctypes.c_char_p(bytes(fr32))))

    def squeeze_challenge(self) -> bytes:
        out = ctypes.create_string_buffer(32)
        self._ck(lib().zk_transcript_squeeze(ctypes.c_void_p(self.h), out))
        return out.raw

    def proof(self) -> bytes:
        p = ctypes.c_void_p()
        n = lib().zk_transcript_proof(ctypes.c_void_p(self.h), ctypes.byref(p))
        return ctypes.string_at(p.value, n) if n else b""

    def close(self):
        if self.h:
            lib().zk_transcript_free(ctypes.c_void_p(self.h))
            self.h = None


def host_keccak256(data: bytes) -> bytes:
    out = ctypes.create_string_buffer(32)
    rc = lib().zk_host_keccak256(ctypes.c_char_p(data), ctypes.c_size_t(len(data)), out)
    if rc != 0:
        raise ZkError(f"zk_host_keccak256 failed with status {rc}")
    return out.raw


def host_poseidon_permute(state_mont: np.ndarray) -> np.ndarray:
    """(5, 4) u64 Montgomery Fr in and out: one permutation of the transcript's Poseidon (T 5, R_F 8, R_P 60)"""
    st = np.ascontiguousarray(state_mont, dtype=np.uint64).reshape(5, 4).copy()
    rc = lib().zk_host_poseidon_permute(_host_ptr(st))
    if rc != 0:
        raise ZkError(f"zk_host_poseidon_permute failed with status {rc}")
    return st


def host_poseidon_permute_width3(state_mont: np.ndarray) -> np.ndarray:
    """(3, 4) u64 Montgomery Fr in and out: the same generator at T 3, R_F 8, R_P 57 (the reference's Poseidon code hash width)"""
    st = np.ascontiguousarray(state_mont, dtype=np.uint64).reshape(3, 4).copy()
    rc = lib().zk_host_poseidon_permute_width3(_host_ptr(st))
    if rc != 0:
        raise ZkError(f"zk_host_poseidon_permute_width3 failed with status {rc}")
    return st


_TR_IN = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p)
_TR_OUT = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p)


class _TranscriptVtable(ctypes.Structure):     # zk_transcript_vtable
    _fields_ = [("common_point", _TR_IN), ("common_scalar", _TR_IN), ("write_point", _TR_IN), ("write_scalar", _TR_IN), ("squeeze_challenge", _TR_OUT)]


class ProofSession:
    """begin -> advice_phase(...) per phase (returns that phase's challenges) -> finish()."""

    def __init__(self, ctx: "Context", pk: ProvingKey, instance: Sequence[np.ndarray], seed: bytes, instance_slices: bool = False):
        """instance: (n, 4) column images (every usable row is absorbed), or -- instance_slices=True --
        halo2's instance slices as they are: (len_i, 4) arrays, exactly len_i values absorbed each."""
        self.ctx, self.pk = ctx, pk
        ins = [np.ascontiguousarray(a, dtype=np.uint64).reshape(-1, 4) for a in instance]
        pi = (ctypes.c_void_p * max(len(ins), 1))(*[a.ctypes.data for a in ins])
        h = ctypes.c_void_p()
        assert len(seed) == 16
        if instance_slices:
            lens = (ctypes.c_uint32 * max(len(ins), 1))(*[a.shape[0] for a in ins])
            ctx._ck(lib().zk_proof_begin_instances(ctx.h, pk.h, pi, lens, ctypes.c_char_p(seed), ctypes.byref(h)))
        else:
            ctx._ck(lib().zk_proof_begin(ctx.h, pk.h, pi, ctypes.c_char_p(seed), ctypes.byref(h)))
        self.h = h

    def set_multiopen(self, kind: int):
        """0 = GWC (default), 1 = SHPLONK."""
        self.ctx._ck(lib().zk_proof_set_multiopen(self.ctx.h, self.h, ctypes.c_int(kind)))

    def set_vanishing_random(self, kind: int):
        """0 = n uniform coefficients (upstream PSE halo2), 1 = the constant 1 (the reference's own proofs; default)"""
        self.ctx._ck(lib().zk_proof_set_vanishing_random(self.ctx.h, self.h, ctypes.c_int(kind)))

    def set_transcript_kind(self, kind: int):
        """built-in transcript: TRANSCRIPT_BLAKE2B (default), TRANSCRIPT_POSEIDON or TRANSCRIPT_EVM"""
        self.ctx._ck(lib().zk_proof_set_transcript_kind(self.ctx.h, self.h, ctypes.c_int(kind)))

    def set_transcript(self, transcript):
        """Forward every transcript operation to `transcript`, an object with
        common_point(bytes64) / common_scalar(bytes32) / write_point(bytes64) / write_scalar(bytes32)
        (Montgomery limbs, as they cross the ABI) and squeeze_challenge() -> bytes32 (Montgomery Fr).
        The object then owns the proof bytes; finish() returns b''."""
        def wrap_in(fn, nbytes):
            def cb(_user, ptr):
                try:
                    fn(ctypes.string_at(ptr, nbytes))
                    return 0
                except Exception as e:       # never let an exception cross the C boundary
                    print(f"[zkmi355 transcript] callback failed: {e!r}", flush=True)
                    return 1
            return _TR_IN(cb)

        def squeeze(_user, out_ptr):
            try:
                ctypes.memmove(out_ptr, bytes(transcript.squeeze_challenge()), 32)
                return 0
            except Exception as e:
                print(f"[zkmi355 transcript] squeeze failed: {e!r}", flush=True)
                return 1
        vt = _TranscriptVtable(wrap_in(transcript.common_point, 64), wrap_in(transcript.common_scalar, 32),
                               wrap_in(transcript.write_point, 64), wrap_in(transcript.write_scalar, 32), _TR_OUT(squeeze))
        self._transcript = (transcript, vt)      # keep the thunks alive
        self.ctx._ck(lib().zk_proof_set_transcript(self.ctx.h, self.h, ctypes.byref(vt), None))

    def set_sharding(self, rank: int, world: int, allgather_cb):
        """This rank's share of a multi-GPU proof; allgather_cb is a sharding.ALLGATHER_FN instance."""
        self._gather_cb = allgather_cb          # keep the ctypes thunk alive
        self.ctx._ck(lib().zk_proof_set_sharding(self.ctx.h, self.h, ctypes.c_uint32(rank), ctypes.c_uint32(world), allgather_cb, None))

    def set_sharding_comm(self):
        """shard this session over the context's own RCCL communicator (Context.comm_init)"""
        self.ctx._ck(lib().zk_proof_set_sharding_comm(self.ctx.h, self.h))

    def set_device_gather(self, allgather_dev_cb):
        """After set_sharding: exchange the advice columns with a device all-gather (RCCL) instead of
        uploading every column on every rank; allgather_dev_cb is a sharding.ALLGATHER_FN over device pointers."""
        self._gather_dev_cb = allgather_dev_cb
        self.ctx._ck(lib().zk_proof_set_device_gather(self.ctx.h, self.h, allgather_dev_cb, None))

    def advice_phase(self, columns: dict) -> np.ndarray:
        """columns: {advice column index: (n, 4) u64 Montgomery array}; returns (num_challenges, 4) u64."""
        idx = sorted(columns)
        cols = [np.ascontiguousarray(columns[i], dtype=np.uint64) for i in idx]
        ci = (ctypes.c_uint32 * max(len(idx), 1))(*idx)
        pc = (ctypes.c_void_p * max(len(idx), 1))(*[c.ctypes.data for c in cols])
        cap = getattr(self, "_challenge_cap", None)
        if cap is None:
            cap = self._challenge_cap = max(1, self.pk.shape()["challenges"])      # sized from the key, never guessed
        out = np.zeros((cap, 4), dtype=np.uint64)
        cnt = ctypes.c_uint32(cap)
        self.ctx._ck(lib().zk_proof_advice_phase(self.ctx.h, self.h, ci, pc, ctypes.c_uint32(len(idx)), _host_ptr(out), ctypes.byref(cnt)))
        return out[:cnt.value].copy()

    def advice_phase_typed(self, columns: dict) -> np.ndarray:
        """advice_phase for columns held as the integers they are: {advice column index: array of n cells}, the cell width taken
        from the array (typed_cell_width): uint8 / uint16 / uint32 / uint64 of shape (n,), (n, 2) uint64 for 128-bit cells (low
        word first), (n, 4) uint64 for Montgomery Fr as advice_phase takes it.  Narrow columns cross PCIe at their own width and
        are expanded on the device; same challenges, same proof bytes.  Not available in a sharded session."""
        idx = sorted(columns)
        cols = [np.ascontiguousarray(columns[i]) for i in idx]
        wd = (ctypes.c_uint8 * max(len(idx), 1))(*[typed_cell_width(c) for c in cols])
        ci = (ctypes.c_uint32 * max(len(idx), 1))(*idx)
        pc = (ctypes.c_void_p * max(len(idx), 1))(*[c.ctypes.data for c in cols])
        cap = getattr(self, "_challenge_cap", None)
        if cap is None:
            cap = self._challenge_cap = max(1, self.pk.shape()["challenges"])
        out = np.zeros((cap, 4), dtype=np.uint64)
        cnt = ctypes.c_uint32(cap)
        self.ctx._ck(lib().zk_proof_advice_phase_typed(self.ctx.h, self.h, ci, pc, wd, ctypes.c_uint32(len(idx)), _host_ptr(out), ctypes.byref(cnt)))
        return out[:cnt.value].copy()

    def advice_phase_dev(self, columns: dict, in_place: bool = False) -> np.ndarray:
        """{advice column index: DeviceBuffer (n x 32 B, Montgomery)}: the phase's witness columns resident on the device.
        in_place: the session works in these buffers (it overwrites their blinding rows) until finish() / abort() returns.
        Sharded session with a device all-gather: a column this rank does not own (position j of the phase's columns in ascending
        index order, j % world != rank) may be None -- it arrives over the fabric from its owner."""
        idx = sorted(columns)
        ci = (ctypes.c_uint32 * max(len(idx), 1))(*idx)
        ptrs = (ctypes.c_void_p * max(len(idx), 1))(*[None if columns[i] is None else columns[i].ptr for i in idx])
        cap = getattr(self, "_challenge_cap", None)
        if cap is None:
            cap = self._challenge_cap = max(1, self.pk.shape()["challenges"])
        out = np.zeros((cap, 4), dtype=np.uint64)
        cnt = ctypes.c_uint32(cap)
        self.ctx._ck(lib().zk_proof_advice_phase_dev(self.ctx.h, self.h, ci, ptrs, ctypes.c_uint32(len(idx)), ctypes.c_uint32(1 if in_place else 0), _host_ptr(out), ctypes.byref(cnt)))
        return out[:cnt.value].copy()

    def advice_phase_typed_dev(self, columns: dict) -> np.ndarray:
        """advice_phase_typed for cells resident on the device: {advice column index: (device pointer or DeviceBuffer, cell width)}.
        Width 1, 2, 4, 8, 16: at least usable_rows packed little-endian unsigned cells; 32: an n x 32 B Montgomery column.  The
        buffers are only read, and not after the call returns; several columns may share one.  Narrow columns are expanded straight
        into the session's buffers, sixteen per launch; same challenges, same proof bytes.  Not available in a sharded session."""
        idx = sorted(columns)
        ptr_of = lambda b: b.ptr if isinstance(b, DeviceBuffer) else b
        ci = (ctypes.c_uint32 * max(len(idx), 1))(*idx)
        pc = (ctypes.c_void_p * max(len(idx), 1))(*[ptr_of(columns[i][0]) for i in idx])
        wd = (ctypes.c_uint8 * max(len(idx), 1))(*[columns[i][1] for i in idx])
        cap = getattr(self, "_challenge_cap", None)
        if cap is None:
            cap = self._challenge_cap = max(1, self.pk.shape()["challenges"])
        out = np.zeros((cap, 4), dtype=np.uint64)
        cnt = ctypes.c_uint32(cap)
        self.ctx._ck(lib().zk_proof_advice_phase_typed_dev(self.ctx.h, self.h, ci, pc, wd, len(idx), _host_ptr(out), ctypes.byref(cnt)))
        return out[:cnt.value].copy()

    def mock_verify(self, gate_rows: Optional[Sequence[int]] = None, lookup_rows: Optional[Sequence[int]] = None, cap: int = 4096):
        """zk_proof_mock_verify: MockProver's row checks over the columns this session holds, with the challenges its transcript
        produced; after the last advice phase, before finish().  Returns (records, total) like Context.mock_verify."""
        gr = None if gate_rows is None else np.ascontiguousarray(gate_rows, dtype=np.uint32)
        lr = None if lookup_rows is None else np.ascontiguousarray(lookup_rows, dtype=np.uint32)
        out = np.zeros((max(cap, 1), 4), dtype=np.uint32)
        total = ctypes.c_size_t()
        self.ctx._ck(lib().zk_proof_mock_verify(self.ctx.h, self.h, None if gr is None else _host_ptr(gr), ctypes.c_size_t(0 if gr is None else len(gr)),
                                            None if lr is None else _host_ptr(lr), ctypes.c_size_t(0 if lr is None else len(lr)),
                                            _host_ptr(out), ctypes.c_size_t(cap), ctypes.byref(total)))
        return [tuple(int(v) for v in r) for r in out[:min(total.value, cap)]], total.value

    def finish(self) -> bytes:
        cap = 1 << 20
        out = ctypes.create_string_buffer(cap)
        n = ctypes.c_size_t()
        h, self.h = self.h, None
        self.ctx._ck(lib().zk_proof_finish(self.ctx.h, h, out, ctypes.c_size_t(cap), ctypes.byref(n)))
        return out.raw[:n.value]

    def abort(self):
        if self.h:
            lib().zk_proof_abort(self.ctx.h, self.h)
            self.h = None


class Context:
    """One zk_ctx: one GPU, one stream, one host thread."""

    def __init__(self, device: int = 0, stream: Optional[int] = None):
        h = ctypes.c_void_p()
        rc = lib().zk_ctx_create(ctypes.c_int(device), ctypes.byref(h))
        if rc != 0:
            raise ZkError(f"zk_ctx_create failed with status {rc} (no gfx950 device? there is no CPU fallback)")
        self.h = h
        if stream is not None:
            self._ck(lib().zk_ctx_set_stream(self.h, ctypes.c_void_p(stream)))

    def _ck(self, rc: int):
        if rc != 0:
            raise ZkError(f"zkmi355 status {rc}: {lib().zk_last_error(self.h).decode()}")

    def close(self):
        if self.h:
            lib().zk_ctx_destroy(self.h)
            self.h = None

    def sync(self):
        """joins every stream of the library (main, copy, auxiliary, MSM side streams), not only the main one"""
        self._ck(lib().zk_ctx_sync(self.h))

    def streams_busy(self) -> int:
        n = ctypes.c_int()
        self._ck(lib().zk_ctx_streams_busy(self.h, ctypes.byref(n)))
        return n.value

    def debug_delay(self, role: int, usec: int):
        self._ck(lib().zk_ctx_debug_delay(self.h, ctypes.c_int(role), ctypes.c_uint32(usec)))

    def device_info(self):
        name = ctypes.create_string_buffer(256)
        cu = ctypes.c_int()
        hbm = ctypes.c_size_t()
        self._ck(lib().zk_device_info(self.h, name, ctypes.c_size_t(256), ctypes.byref(cu), ctypes.byref(hbm)))
        return name.value.decode(), cu.value, hbm.value

    # ---- memory
    def alloc(self, nbytes: int) -> DeviceBuffer:
        return DeviceBuffer(self, nbytes)

    def to_device(self, a: np.ndarray) -> DeviceBuffer:
        a = np.ascontiguousarray(a)
        return DeviceBuffer(self, max(a.nbytes, 1)).upload(a)

    def timer_start(self):
        self._ck(lib().zk_timer_start(self.h))

    def timer_stop_ms(self) -> float:
        ms = ctypes.c_float()
        self._ck(lib().zk_timer_stop_ms(self.h, ctypes.byref(ms)))
        return ms.value

    # ---- profiling
    def prof_enable(self, on=True):
        """True / 1: every kernel group; 2: only the roofline kernels' groups; False / 0: off"""
        self._ck(lib().zk_prof_enable(self.h, ctypes.c_int(int(on))))

    def prof_reset(self):
        self._ck(lib().zk_prof_reset(self.h))

    def prof_get(self, name: str):
        ms, cnt = ctypes.c_double(), ctypes.c_uint64()
        self._ck(lib().zk_prof_get(self.h, name.encode(), ctypes.byref(ms), ctypes.byref(cnt)))
        return ms.value, cnt.value

    def prof_get_bytes(self, name: str) -> int:
        b = ctypes.c_uint64()
        self._ck(lib().zk_prof_get_bytes(self.h, name.encode(), ctypes.byref(b)))
        return b.value

    def prof_names(self):
        buf = ctypes.create_string_buffer(4096)
        self._ck(lib().zk_prof_names(self.h, buf, ctypes.c_size_t(4096)))
        return [x for x in buf.value.decode().split(";") if x]

    # ---- field vectors
    def field_vec_op(self, field: int, op: int, a: DeviceBuffer, b: DeviceBuffer, out: DeviceBuffer, n: int):
        self._ck(lib().zk_field_vec_op(self.h, field, op, ctypes.c_void_p(a.ptr), ctypes.c_void_p(b.ptr), ctypes.c_void_p(out.ptr), ctypes.c_size_t(n)))

    def scan_affine(self, a: DeviceBuffer, b: DeviceBuffer, out: DeviceBuffer, n: int, reverse: bool = False):
        """out[0] = b[0], out[i] = a[i] * out[i - 1] + b[i] over n Montgomery Fr (zk_field_vec_op with ZK_OP_SCAN_AFFINE); reverse: from
        the last element down, out[i] = a[i] * out[i + 1] + b[i].  a[i] = 0 starts a new segment; out overlaps neither input."""
        self.field_vec_op(FIELD_FR, OP_SCAN_AFFINE_REV if reverse else OP_SCAN_AFFINE, a, b, out, n)

    def row_rlc(self, cols, widths, weights, n, out, constant=None):
        """out[i] = constant + sum_j weights[j] * cell_j[i] for i < n (zk_field_vec_op with ZK_OP_ROW_RLC), one launch per 64 columns.
        cols[j]: DeviceBuffer or device pointer of n cells of widths[j] bytes -- 1, 2, 4, 8, 16: packed little-endian unsigned cells,
        read like fr_from_uint; 32: Montgomery Fr.  weights: count x 4 uint64 Montgomery, constant: 4 uint64 Montgomery (default 0).
        out (DeviceBuffer or pointer, n x 32 B) may be one of the 32-byte columns itself and must not overlap any other column."""
        ptr_of = lambda b: b.ptr if isinstance(b, DeviceBuffer) else b
        cnt = len(cols)
        assert len(widths) == cnt
        hk = np.zeros((cnt + 1, 4), dtype=np.uint64)
        if constant is not None:
            hk[0] = np.asarray(constant, dtype=np.uint64).reshape(4)
        if cnt:
            hk[1:] = np.asarray(weights, dtype=np.uint64).reshape(cnt, 4)
        pp = (ctypes.c_void_p * max(cnt, 1))(*[ptr_of(p) for p in cols])
        wd = (ctypes.c_uint8 * max(cnt, 1))(*widths)
        desc = _RowRlc(cnt, ctypes.cast(pp, ctypes.POINTER(ctypes.c_void_p)), ctypes.cast(wd, ctypes.POINTER(ctypes.c_uint8)))
        self._ck(lib().zk_field_vec_op(self.h, FIELD_FR, OP_ROW_RLC, ctypes.byref(desc), _host_ptr(hk), ctypes.c_void_p(ptr_of(out)), ctypes.c_size_t(n)))

    def scan_rlc(self, cells, width, kinds, table, n, out, z0=None, reverse=False):
        """out[i] = m[kind_i] * out[i - 1] + w[kind_i] * cell[i] for i < n with out[-1] = z0 (zk_field_vec_op with ZK_OP_SCAN_RLC);
        reverse: from the last element down, out[i] = m[kind_i] * out[i + 1] + w[kind_i] * cell[i] with out[n] = z0.  cells: DeviceBuffer
        or device pointer of n cells of `width` bytes -- 1, 2, 4, 8, 16: packed little-endian unsigned cells, read like fr_from_uint;
        32: Montgomery Fr.  kinds: n bytes on the device (the low two bits of each are the row's kind) or None (every row kind 0).
        table: four (m, w) pairs, each 4 uint64 Montgomery -- e.g. step (r, 1), start (0, 1), hold (1, 0), clear (0, 0); z0: 4 uint64
        Montgomery (default 0).  out (DeviceBuffer or pointer, n x 32 B) overlaps neither the cells nor the kinds."""
        ptr_of = lambda b: b.ptr if isinstance(b, DeviceBuffer) else b
        hk = np.zeros((9, 4), dtype=np.uint64)
        if z0 is not None:
            hk[0] = np.asarray(z0, dtype=np.uint64).reshape(4)
        hk[1:] = np.asarray(table, dtype=np.uint64).reshape(8, 4)
        desc = _ScanRlc(ptr_of(cells), width, None if kinds is None else ptr_of(kinds))
        self._ck(lib().zk_field_vec_op(self.h, FIELD_FR, OP_SCAN_RLC_REV if reverse else OP_SCAN_RLC, ctypes.byref(desc), _host_ptr(hk), ctypes.c_void_p(ptr_of(out)), ctypes.c_size_t(n)))

    def row_inv0(self, cols, widths, weights, n, out, constant=None, num=None, num_width=32):
        """out[i] = num[i] * inv0(constant + sum_j weights[j] * cell_j[i]) for i < n, inv0(0) = 0 (zk_field_vec_op with ZK_OP_ROW_INV0):
        IsZeroChip's value_inv (one column, weight one), IsEqual's inverse of a difference (weights 1, -1), a rational cell (num).
        cols, widths, weights, constant: as for row_rlc.  num: None (every numerator is one) or a DeviceBuffer / device pointer of n
        cells of num_width bytes (1, 2, 4, 8, 16 packed, 32 Montgomery Fr).  A row whose denominator is zero gives zero.  out
        (DeviceBuffer or pointer, n x 32 B) may be one of the 32-byte columns or the 32-byte numerator itself and must not overlap
        any other column.  One launch per 64 columns; only the last one inverts."""
        ptr_of = lambda b: b.ptr if isinstance(b, DeviceBuffer) else b
        cnt = len(cols)
        assert len(widths) == cnt
        hk = np.zeros((cnt + 1, 4), dtype=np.uint64)
        if constant is not None:
            hk[0] = np.asarray(constant, dtype=np.uint64).reshape(4)
        if cnt:
            hk[1:] = np.asarray(weights, dtype=np.uint64).reshape(cnt, 4)
        pp = (ctypes.c_void_p * max(cnt, 1))(*[ptr_of(p) for p in cols])
        wd = (ctypes.c_uint8 * max(cnt, 1))(*widths)
        desc = _RowInv0(cnt, ctypes.cast(pp, ctypes.POINTER(ctypes.c_void_p)), ctypes.cast(wd, ctypes.POINTER(ctypes.c_uint8)),
                        None if num is None else ptr_of(num), 0 if num is None else num_width)
        self._ck(lib().zk_field_vec_op(self.h, FIELD_FR, OP_ROW_INV0, ctypes.byref(desc), _host_ptr(hk), ctypes.c_void_p(ptr_of(out)), ctypes.c_size_t(n)))

    def poseidon(self, in0, width0, in1, width1, n, out, cap=None, cap_width=8, cap_scale=None, kinds=None, final=False, word0=None, word1=None):
        """out[i] = permute(s)[0] for i < n, the width-3 Poseidon permutation of host_poseidon_permute_width3 over typed cells
        (zk_field_vec_op with ZK_OP_POSEIDON).  in0, in1, cap, kinds, out, word0, word1: DeviceBuffers or device pointers.  Widths 1, 2,
        4, 8, 16 (packed little-endian), 32 (Montgomery Fr) or, for in0 and in1, 31: cell i is the 31 BIG-endian bytes at ptr + 62 i.
        kinds: None (every row is a head) or n bytes, kind = byte & 3: 0 head, s = (cap_scale * cap[i], in0[i], in1[i]); 1 continue,
        s = the state row i - 1 left + (0, in0[i], in1[i]); 2, 3 off, the row writes 0.  cap None: capacity 0; cap_scale: (4,) u64
        Montgomery Fr, None: one.  final: every row of a message holds the value of its last row.  word0, word1: optional n x 32 B
        outputs, the Montgomery images of in0 and in1.  No output may overlap an input or another output."""
        ptr_of = lambda b: None if b is None else b.ptr if isinstance(b, DeviceBuffer) else b
        scale = np.zeros(4, dtype=np.uint64)
        if cap_scale is None:
            scale[:] = (0xac96341c4ffffffb, 0x36fc76959f60cd29, 0x666ea36f7879462e, 0x0e0a77c19a07df2f)      # 2^256 mod r: Montgomery one
        else:
            scale[:] = np.asarray(cap_scale, dtype=np.uint64).reshape(4)
        desc = _Poseidon(ptr_of(in0), ptr_of(in1), ptr_of(cap), ptr_of(kinds), ptr_of(word0), ptr_of(word1), width0, width1, cap_width if cap is not None else 0,
                         POSEIDON_FINAL if final else 0)
        self._ck(lib().zk_field_vec_op(self.h, FIELD_FR, OP_POSEIDON, ctypes.byref(desc), _host_ptr(scale), ctypes.c_void_p(ptr_of(out)), ctypes.c_size_t(n)))

    def _byte_hash(self, op, desc_type, data, total_bytes, offsets, lens, index_width, n, out, r_out, r_in, digest, input_rlc):
        """keccak() and sha256(): one descriptor layout, the two challenges behind each other"""
        ptr_of = lambda b: None if b is None else b.ptr if isinstance(b, DeviceBuffer) else b
        r = np.zeros((2, 4), dtype=np.uint64)
        r[0] = np.asarray(r_out, dtype=np.uint64).reshape(4)
        r[1] = np.asarray(r_in, dtype=np.uint64).reshape(4)
        desc = desc_type(ptr_of(data), total_bytes, ptr_of(offsets), ptr_of(lens), ptr_of(digest), ptr_of(input_rlc), index_width, 0)
        self._ck(lib().zk_field_vec_op(self.h, FIELD_FR, op, ctypes.byref(desc), _host_ptr(r), ctypes.c_void_p(ptr_of(out)), ctypes.c_size_t(n)))

    def keccak(self, data, total_bytes, offsets, lens, index_width, n, out, r_out, r_in=None, digest=None, input_rlc=None):
        """out[i] = sum_k digest_i[k] r_out^(31-k) for i < n, digest_i = Keccak-256 (the function of host_keccak256) of the lens[i]
        bytes at data + offsets[i]: the KeccakTable's output_rlc (zk_field_vec_op with ZK_OP_KECCAK).  data, offsets, lens, out, digest,
        input_rlc: DeviceBuffers or device pointers.  data: total_bytes readable bytes; offsets, lens: n unsigned little-endian
        integers of index_width (4 or 8) bytes, aligned to it -- lens is the table's input_len column as it stands.  Messages may
        overlap, repeat and start at any byte address; a message that does not lie inside the total_bytes writes 0 to every output
        of its row and reads nothing, without an error.  r_out, r_in: (4,) u64 Montgomery Fr (r_in None: zero; it is used only with
        input_rlc).  digest: optional n x 32 B, the digest bytes; input_rlc: optional n x 32 B, sum_k m[k] r_in^(len-1-k), 0 for
        the empty message.  No output may overlap an input or another output."""
        self._byte_hash(OP_KECCAK, _Keccak, data, total_bytes, offsets, lens, index_width, n, out, r_out, np.zeros(4, dtype=np.uint64) if r_in is None else r_in, digest, input_rlc)

    def sha256(self, data, total_bytes, offsets, lens, index_width, n, out, r_out, r_in=None, digest=None, input_rlc=None):
        """out[i] = sum_k digest_i[k] r_out^(31-k) for i < n, digest_i = SHA-256 (FIPS 180-4) of the lens[i] bytes at data +
        offsets[i]: the SHA256Table's output_rlc (zk_field_vec_op with ZK_OP_SHA256).  The arguments and rules are keccak()'s: data,
        offsets, lens, out, digest, input_rlc are DeviceBuffers or device pointers; data holds total_bytes (below 2^61) readable
        bytes; offsets, lens are n unsigned little-endian integers of index_width (4 or 8) bytes, aligned to it -- lens is the
        table's input_len column as it stands.  Messages may overlap, repeat and start at any byte address; a message that does not
        lie inside the total_bytes writes 0 to every output of its row and reads nothing, without an error.  r_out, r_in: (4,) u64
        Montgomery Fr; r_in None means r_in = r_out, because the reference's table takes both RLCs under one challenge
        (keccak_input); r_in is used only with input_rlc.  digest: optional n x 32 B, the digest bytes in digest order; input_rlc:
        optional n x 32 B, sum_k m[k] r_in^(len-1-k), 0 for the empty message.  No output may overlap an input or another output."""
        self._byte_hash(OP_SHA256, _Sha256, data, total_bytes, offsets, lens, index_width, n, out, r_out, r_out if r_in is None else r_in, digest, input_rlc)

    def key_sort(self, keys, n, perm_out, mask=None, sorted_keys=None):
        """perm_out[i] = the uint32 index of the record that stands at place i when the n 64-byte key records at keys are sorted as
        big-endian 512-bit integers, stably (zk_field_vec_op with ZK_OP_KEY_SORT).  keys, perm_out, sorted_keys: DeviceBuffers or
        device pointers; keys and sorted_keys 8-byte aligned, perm_out n x 4 B.  mask: None (all 64 bytes take part) or 64 bytes,
        key byte j takes part if and only if mask[j] != 0; without bytes 60-63 the order is the reference's
        sort_by_cached_key(Rw::as_key) over rows handed over in rw_counter order.  sorted_keys: optional n x 64 B, the records in
        sorted order.  No output may overlap the records or another output."""
        ptr_of = lambda b: None if b is None else b.ptr if isinstance(b, DeviceBuffer) else b
        desc = _KeySort(ptr_of(keys), ptr_of(sorted_keys), 0)
        m = None
        if mask is not None:
            m = np.ascontiguousarray(np.frombuffer(bytes(mask), dtype=np.uint8) if isinstance(mask, (bytes, bytearray)) else np.asarray(mask, dtype=np.uint8))
            if m.shape != (64,):
                raise ValueError("the key mask has 64 bytes")
        self._ck(lib().zk_field_vec_op(self.h, FIELD_FR, OP_KEY_SORT, ctypes.byref(desc), None if m is None else _host_ptr(m), ctypes.c_void_p(ptr_of(perm_out)), ctypes.c_size_t(n)))

    def key_order(self, keys, n, inv_out, perm=None, diff=None, index=None, bits=None, not_first=None, group_limbs=30, cols=None):
        """The ordering witness of adjacent key records (zk_field_vec_op with ZK_OP_KEY_ORDER).  Row i is record perm[i] (perm None:
        record i); for 1 <= i < n, with j the first 16-bit big-endian limb at which the records of rows i and i - 1 differ: index[i] = j
        (n bytes), bits plane b (n bytes at bits + b * n) = bit (4 - b) of j, diff[i] = cur_j - prev_j (n x 32 B Montgomery Fr),
        inv_out[i] = diff[i]^-1 (n x 32 B), not_first[i] = j >= group_limbs (n bytes; 30: the state circuit's not_first_access).
        Equal records give index 31, difference and inverse 0; row 0, and a row whose index or whose predecessor's index is >= n,
        writes 0 to all of these.  cols: a list of (offset, width, buffer): cell i of the buffer (n cells of width 1, 2 or 4 bytes)
        becomes the big-endian integer of key bytes [offset, offset + width) of row i's record, stored little-endian -- a typed cell
        column; a row whose own index is >= n writes 0.  keys, inv_out, perm, diff, index, bits, not_first and the column buffers:
        DeviceBuffers or device pointers.  No output may overlap an input or another output."""
        ptr_of = lambda b: None if b is None else b.ptr if isinstance(b, DeviceBuffer) else b
        cols = list(cols or [])
        table = (_KeyCol * max(1, len(cols)))(*[_KeyCol(off, width) for off, width, _ in cols])
        ptrs = (ctypes.c_void_p * max(1, len(cols)))(*[ptr_of(buf) for _, _, buf in cols])
        desc = _KeyOrder(ptr_of(keys), ptr_of(perm), ptr_of(diff), ptr_of(index), ptr_of(bits), ptr_of(not_first), group_limbs, len(cols),
                         table if cols else None, ptrs if cols else None, 0)
        self._ck(lib().zk_field_vec_op(self.h, FIELD_FR, OP_KEY_ORDER, ctypes.byref(desc), None, ctypes.c_void_p(ptr_of(inv_out)), ctypes.c_size_t(n)))

    def bytecode_rows(self, data, total_bytes, offsets, lens, index_width, count, n, hash_out, empty_hash, hashes=None, tag=None, index=None, value=None,
                      is_code=None, push_data_left=None, push_data_size=None, length=None, acc_kinds=None, rlc_kinds=None):
        """The n rows of the bytecode circuit from `count` bytecodes, bytecode b the lens[b] bytes at data + offsets[b] (zk_field_vec_op
        with ZK_OP_BYTECODE_ROWS).  data, offsets, lens, index_width mean what they mean for keccak(), with count entries.  A bytecode
        of L bytes owns L + 1 rows, a header row (tag 0, value L) and a row per byte (tag 1, index, value, push_data_size, push_data_left
        and is_code of the unroller); the rows behind the last bytecode, up to n, are padding, all zero.  hash_out (n x 32 B) receives
        hashes[b] (count x 32 B Montgomery Fr; None: zero) on every row of bytecode b and empty_hash ((4,) u64 Montgomery Fr) on the
        padding rows.  tag, is_code, push_data_left, push_data_size, acc_kinds, rlc_kinds: optional n x 1 B at any address; index,
        value, length: optional n x 4 B.  acc_kinds and rlc_kinds are the kind columns from which scan_rlc makes push_acc (forward, over
        value) and push_rlc (reverse, over push_acc).  An entry that does not lie inside the total_bytes counts as an empty bytecode;
        a bytecode that does not fit into the n rows is cut.  Every buffer: a DeviceBuffer or a device pointer.  No output may overlap
        an input or another output."""
        ptr_of = lambda b: None if b is None else b.ptr if isinstance(b, DeviceBuffer) else b
        empty = np.ascontiguousarray(np.asarray(empty_hash, dtype=np.uint64).reshape(4))
        desc = _BytecodeRows(ptr_of(data), total_bytes, ptr_of(offsets), ptr_of(lens), ptr_of(hashes), ptr_of(tag), ptr_of(index), ptr_of(value), ptr_of(is_code),
                             ptr_of(push_data_left), ptr_of(push_data_size), ptr_of(length), ptr_of(acc_kinds), ptr_of(rlc_kinds), count, index_width, 0)
        self._ck(lib().zk_field_vec_op(self.h, FIELD_FR, OP_BYTECODE_ROWS, ctypes.byref(desc), _host_ptr(empty), ctypes.c_void_p(ptr_of(hash_out)), ctypes.c_size_t(n)))

    def copy_rows(self, events, count, data, total_bytes, n, addr, **outputs):
        """The integer columns of the n rows of the copy circuit and the copy table from `count` copy events (zk_field_vec_op with
        ZK_OP_COPY_ROWS).  events: count records of 88 bytes (zk_copy_event) on the device, 8-byte aligned; data: the byte heap of
        total_bytes bytes that the events' three runs point into.  An event of L steps owns 2 L rows, a reader row and a writer row per
        step; the rows behind the last event, up to n, are padding rows.  addr (n x 8 B) receives the addr column; outputs: any of
        COPY_ROWS_OUTPUTS -- 1-byte columns at any address, tag_bits 3 and types 5 planes of n bytes, src_addr_end, real_bytes_left,
        rw_counter and rwc_inc_left n x 8 B at a multiple of 8.  An event that does not count (a tag outside 1..5, a nonzero reserved
        byte, unknown flag bits, a run outside the heap) is an empty event; an event that does not fit into the n rows is cut.  Every
        buffer: a DeviceBuffer or a device pointer.  No output may overlap an input or another output."""
        ptr_of = lambda b: None if b is None else b.ptr if isinstance(b, DeviceBuffer) else b
        unknown = set(outputs) - set(COPY_ROWS_OUTPUTS)
        if unknown:
            raise TypeError(f"copy_rows: unknown outputs {sorted(unknown)}")
        desc = _CopyRows(ptr_of(events), count, ptr_of(data), total_bytes, 0, *(ptr_of(outputs.get(name)) for name in COPY_ROWS_OUTPUTS))
        self._ck(lib().zk_field_vec_op(self.h, FIELD_FR, OP_COPY_ROWS, ctypes.byref(desc), None, ctypes.c_void_p(ptr_of(addr)), ctypes.c_size_t(n)))

    def copy_rlc(self, events, count, data, total_bytes, n, value_acc, r_word, r_in, ids=None, **outputs):
        """The challenge-phase columns of the same n rows (zk_field_vec_op with ZK_OP_COPY_RLC).  events, count, data, total_bytes: as
        for copy_rows.  r_word (evm_word) and r_in (keccak_input): (4,) u64 Montgomery Fr.  value_acc (n x 32 B) receives the running
        RLC of each thread's unmasked bytes; outputs: any of COPY_RLC_OUTPUTS, n x 32 B at a multiple of 16 -- word_rlc and
        word_rlc_prev restart every 32 steps, rlc_acc is the writer's last value_acc on every row of an event with an RLC, id and
        id_other are ids[2 e + t] and ids[2 e + 1 - t] (ids: count x 2 x 32 B Montgomery Fr or None) and 0 and 1 on padding rows."""
        ptr_of = lambda b: None if b is None else b.ptr if isinstance(b, DeviceBuffer) else b
        unknown = set(outputs) - set(COPY_RLC_OUTPUTS)
        if unknown:
            raise TypeError(f"copy_rlc: unknown outputs {sorted(unknown)}")
        ch = np.ascontiguousarray(np.concatenate([np.asarray(r_word, dtype=np.uint64).reshape(4), np.asarray(r_in, dtype=np.uint64).reshape(4)]))
        desc = _CopyRlc(ptr_of(events), count, ptr_of(data), total_bytes, 0, ptr_of(ids), *(ptr_of(outputs.get(name)) for name in COPY_RLC_OUTPUTS))
        self._ck(lib().zk_field_vec_op(self.h, FIELD_FR, OP_COPY_RLC, ctypes.byref(desc), _host_ptr(ch), ctypes.c_void_p(ptr_of(value_acc)), ctypes.c_size_t(n)))

    def exp_rows(self, events, count, n, exponentiation_lo_hi, **outputs):
        """The n rows of the exponentiation circuit and the exponentiation table from `count` events (zk_field_vec_op with
        ZK_OP_EXP_ROWS).  events: count records of 64 bytes (zk_exp_event: base, then exponent, four little-endian u64 each) on the
        device, 8-byte aligned.  An event with exponent x >= 2 owns 8 rows for each of its (bitlen(x) - 1) + (popcount(x) - 1) steps,
        last step of exp_by_squaring first; behind the events the default event (2, 2) is repeated while a step fits below the
        n - 10 rows in use, and the rest is zero.  exponentiation_lo_hi (n x 16 B at a multiple of 16) receives that column; outputs:
        any of EXP_ROWS_OUTPUTS -- is_last n x 1 B, base_limb n x 8 B, exponent_lo_hi n x 16 B, mul_cols and parity_cols 4 planes of
        n x 16 B, the u16_64 and u16_128 outputs 4 and 8 planes of n x 2 B, rows_needed one uint64 that receives 8 x the steps of
        all events + 10 for the caller to compare with n (events that do not fit are cut at a whole step, without an error).  Every
        buffer: a DeviceBuffer or a device pointer.  No output may overlap the events or another output."""
        ptr_of = lambda b: None if b is None else b.ptr if isinstance(b, DeviceBuffer) else b
        unknown = set(outputs) - set(EXP_ROWS_OUTPUTS)
        if unknown:
            raise TypeError(f"exp_rows: unknown outputs {sorted(unknown)}")
        desc = _ExpRows(ptr_of(events), count, 0, *(ptr_of(outputs.get(name)) for name in EXP_ROWS_OUTPUTS))
        self._ck(lib().zk_field_vec_op(self.h, FIELD_FR, OP_EXP_ROWS, ctypes.byref(desc), None, ctypes.c_void_p(ptr_of(exponentiation_lo_hi)), ctypes.c_size_t(n)))

    def code_hash_rows(self, data, total_bytes, offsets, lens, index_width, count, n, field_input, **outputs):
        """The eight columns the Poseidon-hash extension adds to the n rows of the bytecode circuit (zk_field_vec_op with
        ZK_OP_CODE_HASH_ROWS).  data, total_bytes, offsets, lens, index_width, count and the rows are those of bytecode_rows(): a
        bytecode of L bytes owns a header row and a row per byte, the rows behind the last bytecode are padding.  field_input
        (n x 32 B at a multiple of 16) receives the big-endian integer of the bytes of the row's 31-byte field up to the row's own;
        outputs: any of CODE_HASH_ROWS_OUTPUTS -- bytes_in_field_inv and padding_shift n x 32 B Montgomery Fr at a multiple of 16,
        control_length n x 4 B, bytes_in_field_index, is_field_border, field_index and field_index_inv n x 1 B at any address.  An
        entry that does not lie inside the total_bytes counts as an empty bytecode; a bytecode that does not fit into the n rows is
        cut.  Every buffer: a DeviceBuffer or a device pointer.  No output may overlap an input or another output."""
        ptr_of = lambda b: None if b is None else b.ptr if isinstance(b, DeviceBuffer) else b
        unknown = set(outputs) - set(CODE_HASH_ROWS_OUTPUTS)
        if unknown:
            raise TypeError(f"code_hash_rows: unknown outputs {sorted(unknown)}")
        desc = _CodeHashRows(ptr_of(data), total_bytes, ptr_of(offsets), ptr_of(lens), *(ptr_of(outputs.get(name)) for name in CODE_HASH_ROWS_OUTPUTS), count, index_width, 0)
        self._ck(lib().zk_field_vec_op(self.h, FIELD_FR, OP_CODE_HASH_ROWS, ctypes.byref(desc), None, ctypes.c_void_p(ptr_of(field_input)), ctypes.c_size_t(n)))

    def code_hash_table(self, data, total_bytes, offsets, lens, index_width, count, n, input0, **outputs):
        """The code-hash rows of the Poseidon table from the same code bytes (zk_field_vec_op with ZK_OP_CODE_HASH_TABLE): a bytecode
        of L bytes owns ceil(L / 62) of the n rows, an empty one none.  input0 (n x 32 B at a multiple of 16) receives the first
        31-byte word of each block; outputs: any of CODE_HASH_TABLE_OUTPUTS -- input1 n x 32 B, control n x 16 B ((L - 62 j) 2^64),
        heading_mark and kinds n x 1 B, cap n x 8 B (L), rows_needed one uint64 that receives the rows of all bytecodes for the caller
        to compare with n.  The rows behind the last bytecode hold 0 and kind 2.  poseidon(input0, 32, input1, 32, n, hash_id, cap=cap,
        cap_width=8, cap_scale=2^64 as Montgomery Fr, kinds=kinds, final=True) then is the table's hash_id."""
        ptr_of = lambda b: None if b is None else b.ptr if isinstance(b, DeviceBuffer) else b
        unknown = set(outputs) - set(CODE_HASH_TABLE_OUTPUTS)
        if unknown:
            raise TypeError(f"code_hash_table: unknown outputs {sorted(unknown)}")
        desc = _CodeHashTable(ptr_of(data), total_bytes, ptr_of(offsets), ptr_of(lens), *(ptr_of(outputs.get(name)) for name in CODE_HASH_TABLE_OUTPUTS), count, index_width, 0)
        self._ck(lib().zk_field_vec_op(self.h, FIELD_FR, OP_CODE_HASH_TABLE, ctypes.byref(desc), None, ctypes.c_void_p(ptr_of(input0)), ctypes.c_size_t(n)))

    def fr_scale(self, a: DeviceBuffer, s: np.ndarray, n: int):
        self._ck(lib().zk_fr_scale(self.h, ctypes.c_void_p(a.ptr), _host_ptr(np.ascontiguousarray(s)), ctypes.c_size_t(n)))

    def fr_from_uint(self, packed: DeviceBuffer, width_bytes: int, n: int, out: DeviceBuffer, offset_bytes: int = 0):
        """out[i] = Montgomery Fr of the unsigned little-endian integer of width_bytes (1, 2, 4, 8, 16) at packed + offset_bytes + i * width_bytes"""
        self._ck(lib().zk_fr_from_uint(self.h, ctypes.c_void_p(packed.ptr + offset_bytes), ctypes.c_uint32(width_bytes), ctypes.c_size_t(n), ctypes.c_void_p(out.ptr)))

    def fr_from_uint_batch(self, ptrs: Sequence[int], widths: Sequence[int], n: int, outs: Sequence[int]):
        """fr_from_uint for len(ptrs) columns of n cells each, sixteen columns per launch: ptrs[j] / outs[j] are device pointers (or
        DeviceBuffers) of the packed cells of widths[j] bytes and of the n x 32 B output; one call may mix widths"""
        ptr_of = lambda b: b.ptr if isinstance(b, DeviceBuffer) else b
        assert len(ptrs) == len(widths) == len(outs)
        cnt = len(ptrs)
        pp = (ctypes.c_void_p * max(cnt, 1))(*[ptr_of(p) for p in ptrs])
        po = (ctypes.c_void_p * max(cnt, 1))(*[ptr_of(p) for p in outs])
        wd = (ctypes.c_uint8 * max(cnt, 1))(*widths)
        self._ck(lib().zk_fr_from_uint_batch(self.h, pp, wd, cnt, n, po))

    def fr_batch_invert(self, a: DeviceBuffer, n: int):
        self._ck(lib().zk_fr_batch_invert(self.h, ctypes.c_void_p(a.ptr), ctypes.c_size_t(n)))

    def fr_prefix_product(self, a: DeviceBuffer, z: DeviceBuffer, n: int):
        self._ck(lib().zk_fr_prefix_product(self.h, ctypes.c_void_p(a.ptr), ctypes.c_void_p(z.ptr), ctypes.c_size_t(n)))

    def fr_prefix_sum(self, a: DeviceBuffer, z: DeviceBuffer, n: int):
        self._ck(lib().zk_fr_prefix_sum(self.h, ctypes.c_void_p(a.ptr), ctypes.c_void_p(z.ptr), ctypes.c_size_t(n)))

    # ---- NTT (halo2 best_fft / EvaluationDomain)
    def ntt(self, data: DeviceBuffer, log_n: int, inverse: bool = False):
        self._ck(lib().zk_ntt(self.h, ctypes.c_void_p(data.ptr), ctypes.c_uint32(log_n), ctypes.c_int(1 if inverse else 0)))

    def ntt_batch(self, datas: Sequence[DeviceBuffer], log_n: int, inverse: bool = False):
        """zk_ntt over several columns of the same size, several columns per launch"""
        ptrs = (ctypes.c_void_p * max(len(datas), 1))(*[ctypes.c_void_p(d.ptr) for d in datas])
        self._ck(lib().zk_ntt_batch(self.h, ptrs, ctypes.c_size_t(len(datas)), ctypes.c_uint32(log_n), ctypes.c_int(1 if inverse else 0)))

    def coeff_to_coset_batch(self, coeffs: Sequence[DeviceBuffer], k: int, g_mont: np.ndarray, outs: Sequence[DeviceBuffer]):
        cp = (ctypes.c_void_p * max(len(coeffs), 1))(*[ctypes.c_void_p(d.ptr) for d in coeffs])
        op = (ctypes.c_void_p * max(len(outs), 1))(*[ctypes.c_void_p(d.ptr) for d in outs])
        self._ck(lib().zk_coeff_to_coset_batch(self.h, cp, ctypes.c_uint32(k), _host_ptr(np.ascontiguousarray(g_mont)), op, ctypes.c_size_t(len(coeffs))))

    def ntt_sharded(self, local: DeviceBuffer, log_n: int, rank: int, world: int, alltoall_cb, inverse: bool = False):
        """This rank's part of ONE 2^log_n transform spread over `world` GPUs (zk_ntt_sharded):
        in: x[rank + world * i]; out: [j1][c] = X[(rank * m / world + c) + m * j1], m = n / world.
        alltoall_cb is a sharding.ALLTOALL_FN over device pointers."""
        self._ck(lib().zk_ntt_sharded(self.h, ctypes.c_void_p(local.ptr), ctypes.c_uint32(log_n), ctypes.c_int(1 if inverse else 0),
                                      ctypes.c_uint32(rank), ctypes.c_uint32(world), alltoall_cb, None))

    def ntt_omega(self, data: DeviceBuffer, log_n: int, omega_mont: np.ndarray):
        self._ck(lib().zk_ntt_omega(self.h, ctypes.c_void_p(data.ptr), ctypes.c_uint32(log_n), _host_ptr(np.ascontiguousarray(omega_mont))))

    def coeff_to_extended(self, coeffs: DeviceBuffer, k: int, ext_k: int, out: DeviceBuffer):
        self._ck(lib().zk_coeff_to_extended(self.h, ctypes.c_void_p(coeffs.ptr), ctypes.c_uint32(k), ctypes.c_uint32(ext_k), ctypes.c_void_p(out.ptr)))

    def coeff_to_coset(self, coeffs: DeviceBuffer, k: int, g_mont: np.ndarray, out: DeviceBuffer):
        """out[i] = f(g * omega^i): one coset of the extended domain (coeff_to_extended_part)."""
        self._ck(lib().zk_coeff_to_coset(self.h, ctypes.c_void_p(coeffs.ptr), ctypes.c_uint32(k), _host_ptr(np.ascontiguousarray(g_mont)), ctypes.c_void_p(out.ptr)))

    def fr_scatter_scaled(self, src: DeviceBuffer, n: int, scale_mont: np.ndarray, dst: DeviceBuffer, stride: int, offset: int):
        self._ck(lib().zk_fr_scatter_scaled(self.h, ctypes.c_void_p(src.ptr), ctypes.c_size_t(n), _host_ptr(np.ascontiguousarray(scale_mont)),
                                            ctypes.c_void_p(dst.ptr), ctypes.c_size_t(stride), ctypes.c_size_t(offset)))

    def extended_to_coeff(self, ext: DeviceBuffer, ext_k: int):
        self._ck(lib().zk_extended_to_coeff(self.h, ctypes.c_void_p(ext.ptr), ctypes.c_uint32(ext_k)))

    # ---- polynomial helpers
    def poly_eval(self, coeffs: DeviceBuffer, n: int, x_mont: np.ndarray) -> np.ndarray:
        out = np.empty(4, dtype=np.uint64)
        self._ck(lib().zk_poly_eval(self.h, ctypes.c_void_p(coeffs.ptr), ctypes.c_size_t(n), _host_ptr(np.ascontiguousarray(x_mont)), _host_ptr(out)))
        return out

    def poly_eval_batch(self, polys, n: int, x_mont: np.ndarray) -> np.ndarray:
        """eval_polynomial of several device polynomials (n coefficients each) at one point -> (count, 4) u64."""
        count = len(polys)
        out = np.empty((count, 4), dtype=np.uint64)
        ptrs = (ctypes.c_void_p * max(count, 1))(*[ctypes.c_void_p(p.ptr) for p in polys])
        self._ck(lib().zk_poly_eval_batch(self.h, ptrs, ctypes.c_size_t(count), ctypes.c_size_t(n), _host_ptr(np.ascontiguousarray(x_mont)), _host_ptr(out)))
        return out

    def poly_eval_pairs(self, polys, point_index: Sequence[int], points_mont: np.ndarray, n: int) -> np.ndarray:
        """zk_poly_eval_pairs: polys[j] (device, n coefficients) at points_mont[point_index[j]] -> (count, 4) u64, one pass"""
        count = len(polys)
        out = np.empty((max(count, 1), 4), dtype=np.uint64)
        ptrs = (ctypes.c_void_p * max(count, 1))(*[ctypes.c_void_p(p.ptr) for p in polys])
        idx = np.ascontiguousarray(point_index, dtype=np.uint32)
        pts = np.ascontiguousarray(points_mont, dtype=np.uint64).reshape(-1, 4)
        self._ck(lib().zk_poly_eval_pairs(self.h, ptrs, _host_ptr(idx), ctypes.c_size_t(count), _host_ptr(pts), ctypes.c_size_t(len(pts)), ctypes.c_size_t(n), _host_ptr(out)))
        return out[:count]

    def fr_random(self, key32: bytes, stream_id: int, first_block: int, out: DeviceBuffer, n: int):
        """n uniform Fr from ChaCha20 blocks (counter mode) + from_uniform_bytes."""
        assert len(key32) == 32
        self._ck(lib().zk_fr_random(self.h, ctypes.c_char_p(key32), ctypes.c_uint64(stream_id), ctypes.c_uint64(first_block), ctypes.c_void_p(out.ptr), ctypes.c_size_t(n)))

    def host_alloc(self, shape, dtype=np.uint64) -> np.ndarray:
        """numpy array over page-locked host memory (zk_host_alloc); freed with host_free(array)."""
        nbytes = int(np.prod(shape)) * np.dtype(dtype).itemsize
        p = ctypes.c_void_p()
        self._ck(lib().zk_host_alloc(self.h, ctypes.c_size_t(nbytes), ctypes.byref(p)))
        buf = (ctypes.c_uint8 * nbytes).from_address(p.value)
        arr = np.frombuffer(buf, dtype=dtype).reshape(shape)
        self._pinned = getattr(self, "_pinned", {})
        self._pinned[arr.ctypes.data] = p.value
        return arr

    def host_free(self, arr: np.ndarray):
        p = getattr(self, "_pinned", {}).pop(arr.ctypes.data, None)
        if p is not None:
            self._ck(lib().zk_host_free(self.h, ctypes.c_void_p(p)))

    def host_register(self, arr: np.ndarray):
        """Page-lock an array the caller owns (zk_host_register); pair with host_unregister(arr)."""
        assert arr.flags["C_CONTIGUOUS"]
        self._ck(lib().zk_host_register(self.h, ctypes.c_void_p(arr.ctypes.data), ctypes.c_size_t(arr.nbytes)))

    def host_unregister(self, arr: np.ndarray):
        self._ck(lib().zk_host_unregister(self.h, ctypes.c_void_p(arr.ctypes.data)))

    # ---- in-library RCCL collectives (csrc/comm.hip)
    @staticmethod
    def comm_unique_id() -> bytes:
        out = ctypes.create_string_buffer(128)
        rc = lib().zk_comm_unique_id(out)
        if rc != 0:
            raise ZkError(f"zk_comm_unique_id failed with status {rc} (librccl missing?)")
        return out.raw

    def comm_init(self, unique_id: bytes, rank: int, world: int):
        assert len(unique_id) == 128
        self._ck(lib().zk_comm_init(self.h, ctypes.c_char_p(unique_id), ctypes.c_uint32(rank), ctypes.c_uint32(world)))

    def comm_destroy(self):
        self._ck(lib().zk_comm_destroy(self.h))

    def comm_allgather(self, send: DeviceBuffer, nbytes: int, recv: DeviceBuffer):
        self._ck(lib().zk_comm_allgather(self.h, ctypes.c_void_p(send.ptr), ctypes.c_size_t(nbytes), ctypes.c_void_p(recv.ptr)))

    def comm_alltoall(self, send: DeviceBuffer, bytes_per_peer: int, recv: DeviceBuffer):
        self._ck(lib().zk_comm_alltoall(self.h, ctypes.c_void_p(send.ptr), ctypes.c_size_t(bytes_per_peer), ctypes.c_void_p(recv.ptr)))

    def msm_plan(self, srs, n: int) -> dict:
        c, w = ctypes.c_int(), ctypes.c_int()
        self._ck(lib().zk_msm_plan(srs.h, ctypes.c_size_t(n), ctypes.byref(c), ctypes.byref(w)))
        return {"c": c.value, "windows": w.value}

    def lookup_multiplicities(self, inputs: DeviceBuffer, table: DeviceBuffer, usable_rows: int, m: DeviceBuffer, n: int) -> Optional[int]:
        """logUp m(X) on the device; returns the lowest input row missing from the table, or None."""
        bad = ctypes.c_uint64()
        self._ck(lib().zk_lookup_multiplicities(self.h, ctypes.c_void_p(inputs.ptr), ctypes.c_void_p(table.ptr), ctypes.c_size_t(usable_rows),
                                                ctypes.c_void_p(m.ptr), ctypes.c_size_t(n), ctypes.byref(bad)))
        return None if bad.value == 0xFFFFFFFFFFFFFFFF else bad.value

    def commit_batch_h2d(self, srs: "Srs", basis: int, host_cols, dev_cols, n: int) -> np.ndarray:
        """commit `host_cols` (numpy (n,4) u64 each) while uploading them into dev_cols (overlapped)."""
        count = len(host_cols)
        hc = [np.ascontiguousarray(c, dtype=np.uint64) for c in host_cols]
        hp = (ctypes.c_void_p * max(count, 1))(*[ctypes.c_void_p(c.ctypes.data) for c in hc])
        dp = (ctypes.c_void_p * max(count, 1))(*[ctypes.c_void_p(d.ptr) for d in dev_cols])
        out = np.empty((count, 8), dtype=np.uint64)
        self._ck(lib().zk_commit_batch_h2d(self.h, srs.h, ctypes.c_int(basis), hp, dp, ctypes.c_size_t(count), ctypes.c_size_t(n), _host_ptr(out)))
        return out

    def kate_division(self, coeffs: DeviceBuffer, n: int, z_mont: np.ndarray, q: DeviceBuffer):
        self._ck(lib().zk_kate_division(self.h, ctypes.c_void_p(coeffs.ptr), ctypes.c_size_t(n), _host_ptr(np.ascontiguousarray(z_mont)), ctypes.c_void_p(q.ptr)))

    # ---- expression / quotient evaluation (halo2 evaluate_h)
    def quotient_eval(self, program: np.ndarray, col_ptrs, consts: np.ndarray, k: int, ext_k: int, out: DeviceBuffer, divide_by_vanishing: bool = False):
        prog = np.ascontiguousarray(program, dtype=np.uint32).reshape(-1, 3)
        ptrs = (ctypes.c_void_p * max(len(col_ptrs), 1))(*[ctypes.c_void_p(p) for p in col_ptrs])
        consts = np.ascontiguousarray(consts, dtype=np.uint64).reshape(-1, 4)
        self._ck(lib().zk_quotient_eval(self.h, prog.ctypes.data_as(ctypes.c_void_p), ctypes.c_uint32(prog.shape[0]), ptrs, ctypes.c_uint32(len(col_ptrs)),
                                        _host_ptr(consts) if consts.size else None, ctypes.c_uint32(consts.shape[0]), ctypes.c_uint32(k), ctypes.c_uint32(ext_k),
                                        ctypes.c_int(1 if divide_by_vanishing else 0), ctypes.c_void_p(out.ptr)))

    def fr_powers(self, base_mont: np.ndarray, mul_mont: np.ndarray, out: DeviceBuffer, n: int):
        self._ck(lib().zk_fr_powers(self.h, _host_ptr(np.ascontiguousarray(base_mont)), _host_ptr(np.ascontiguousarray(mul_mont)), ctypes.c_void_p(out.ptr), ctypes.c_size_t(n)))

    # ---- SRS / MSM (halo2 ParamsKZG / best_multiexp)
    def srs_create(self, k: int, g: np.ndarray, g_lagrange: Optional[np.ndarray] = None) -> Srs:
        h = ctypes.c_void_p()
        gl = _host_ptr(np.ascontiguousarray(g_lagrange)) if g_lagrange is not None else None
        self._ck(lib().zk_srs_create(self.h, ctypes.c_uint32(k), _host_ptr(np.ascontiguousarray(g)), gl, ctypes.byref(h)))
        return Srs(self, h)

    # ---- SRS files (ParamsKZG::read_custom / write_custom): format 0 Processed, 1 RawBytes, 2 RawBytesUnchecked
    def params_read(self, data: bytes, fmt: int = 2):
        """-> (Srs, g2 bytes, s_g2 bytes); refuses a length that does not match the header's k."""
        h = ctypes.c_void_p()
        g2len = 64 if fmt == 0 else 128
        g2, sg2 = ctypes.create_string_buffer(g2len), ctypes.create_string_buffer(g2len)
        buf = np.frombuffer(data, dtype=np.uint8)
        self._ck(lib().zk_params_read(self.h, _host_ptr(buf), ctypes.c_size_t(buf.size), ctypes.c_int(fmt), ctypes.byref(h), g2, sg2))
        return Srs(self, h), g2.raw, sg2.raw

    def params_write(self, srs: Srs, g2: bytes, s_g2: bytes, fmt: int = 2) -> bytes:
        need = ctypes.c_size_t()
        self._ck(lib().zk_params_write(self.h, srs.h, g2, s_g2, ctypes.c_int(fmt), None, ctypes.c_size_t(0), ctypes.byref(need)))
        out = np.empty(need.value, dtype=np.uint8)
        self._ck(lib().zk_params_write(self.h, srs.h, g2, s_g2, ctypes.c_int(fmt), _host_ptr(out), ctypes.c_size_t(out.size), ctypes.byref(need)))
        return out.tobytes()

    def srs_setup_with_s(self, k: int, s_mont: np.ndarray) -> Srs:
        h = ctypes.c_void_p()
        self._ck(lib().zk_srs_setup_with_s(self.h, ctypes.c_uint32(k), _host_ptr(np.ascontiguousarray(s_mont)), ctypes.byref(h)))
        return Srs(self, h)

    def msm(self, scalars_ptr: int, bases_ptr: int, n: int) -> np.ndarray:
        out = np.empty(8, dtype=np.uint64)
        self._ck(lib().zk_msm_g1(self.h, ctypes.c_void_p(scalars_ptr), ctypes.c_void_p(bases_ptr), ctypes.c_size_t(n), _host_ptr(out)))
        return out

    def msm_segments(self, scalars_ptr: int, bases_ptr: int, seg_offsets: Sequence[int]) -> np.ndarray:
        """zk_msm_g1_segments: out[s] = sum of scalars[i] * bases[i] over [seg_offsets[s], seg_offsets[s + 1]), all segments in one
        pass; device pointers, arbitrary bases; returns (len(seg_offsets) - 1, 8) u64 affine Montgomery."""
        off = np.ascontiguousarray(seg_offsets, dtype=np.uint32)
        if off.ndim != 1 or off.size < 1:
            raise ZkError("msm_segments: seg_offsets holds one offset more than there are segments")
        out = np.zeros((max(off.size - 1, 1), 8), dtype=np.uint64)
        self._ck(lib().zk_msm_g1_segments(self.h, ctypes.c_void_p(scalars_ptr), ctypes.c_void_p(bases_ptr), _host_ptr(off), ctypes.c_size_t(off.size - 1), _host_ptr(out)))
        return out[:off.size - 1]

    def commit(self, srs: Srs, scalars: DeviceBuffer, n: int, lagrange: bool = False) -> np.ndarray:
        out = np.empty(8, dtype=np.uint64)
        self._ck(lib().zk_commit(self.h, srs.h, ctypes.c_int(1 if lagrange else 0), ctypes.c_void_p(scalars.ptr), ctypes.c_size_t(n), _host_ptr(out)))
        return out

    def commit_batch(self, srs: Srs, scalar_ptrs: Sequence[int], n: int, lagrange: bool = False, narrow: Optional[Sequence[int]] = None) -> np.ndarray:
        """`len(scalar_ptrs)` commitments over one basis, pipelined on the device; returns (count, 8) u64.
        narrow: optional per-column hint (0 dense, 1 small integers: per-window MSM path, 2 long runs of equal
        values: sliced sort), speed only."""
        count = len(scalar_ptrs)
        out = np.empty((max(count, 1), 8), dtype=np.uint64)
        ptrs = (ctypes.c_void_p * max(count, 1))(*[ctypes.c_void_p(p) for p in scalar_ptrs])
        if narrow is None:
            self._ck(lib().zk_commit_batch(self.h, srs.h, ctypes.c_int(1 if lagrange else 0), ptrs, ctypes.c_size_t(count), ctypes.c_size_t(n), _host_ptr(out)))
        else:
            assert len(narrow) == count
            flags = (ctypes.c_uint8 * max(count, 1))(*[int(f) for f in narrow])
            self._ck(lib().zk_commit_batch_hint(self.h, srs.h, ctypes.c_int(1 if lagrange else 0), ptrs, ctypes.c_size_t(count), ctypes.c_size_t(n), flags, _host_ptr(out)))
        return out[:count]

    def best_multiexp(self, scalars: np.ndarray, bases: np.ndarray) -> np.ndarray:
        """halo2 ``best_multiexp(coeffs, bases)`` over host slices."""
        scalars = np.ascontiguousarray(scalars)
        bases = np.ascontiguousarray(bases)
        n = scalars.shape[0] if scalars.size else 0
        out = np.empty(8, dtype=np.uint64)
        self._ck(lib().zk_msm_g1_host(self.h, _host_ptr(scalars), _host_ptr(bases), ctypes.c_size_t(n), _host_ptr(out)))
        return out

    def best_fft(self, a: np.ndarray, log_n: int, inverse: bool = False) -> np.ndarray:
        """halo2 ``best_fft`` over a host slice (copy in, transform, copy out)."""
        buf = self.to_device(a)
        self.ntt(buf, log_n, inverse)
        out = buf.download(a.shape)
        buf.free()
        return out

    # ---- full proofs (halo2 keygen_pk / create_proof, GWC)
    def pk_create(self, srs: Srs, blob: bytes) -> "ProvingKey":
        h = ctypes.c_void_p()
        if isinstance(blob, np.ndarray):      # large keys: a uint8 array is passed by pointer, no copy
            assert blob.dtype == np.uint8 and blob.flags["C_CONTIGUOUS"]
            self._ck(lib().zk_pk_create(self.h, srs.h, _host_ptr(blob), ctypes.c_size_t(blob.nbytes), ctypes.byref(h)))
            return ProvingKey(self, h)
        view = np.frombuffer(blob, dtype=np.uint8)      # read-only view of the bytes object: no copy of a multi-GiB key
        self._ck(lib().zk_pk_create(self.h, srs.h, _host_ptr(view), ctypes.c_size_t(view.size), ctypes.byref(h)))
        return ProvingKey(self, h)

    def _proof_args(self, who: str, vk: "VerifyingKey", proofs: Sequence[bytes], instances: Sequence[Sequence[np.ndarray]]):
        """the (instances, lengths, proofs, proof lengths) arguments zk_verify_proofs and zk_verify_accumulators share; the first
        item returned keeps the buffers alive"""
        sh = vk.shape_
        n, u = 1 << sh["k"], (1 << sh["k"]) - sh["blinding_factors"] - 1
        if len(proofs) != len(instances) or not proofs:
            raise ZkError(f"{who}: one instance list per proof, at least one proof")
        keep = []
        inst_ptrs = (ctypes.c_void_p * len(proofs))()
        len_ptrs = (ctypes.c_void_p * len(proofs))()
        for b, cols in enumerate(instances):
            if len(cols) != sh["I"]:
                raise ZkError(f"{who}: proof {b} has {len(cols)} instance columns, the key {sh['I']}")
            arrs = []
            for c in cols:
                a = np.ascontiguousarray(c, dtype=np.uint64).reshape(-1, 4)
                arrs.append(a[:u] if len(a) == n else a)
            ptrs = (ctypes.c_void_p * max(len(arrs), 1))(*[a.ctypes.data for a in arrs])
            lens = (ctypes.c_uint32 * max(len(arrs), 1))(*[len(a) for a in arrs])
            keep += [arrs, ptrs, lens]
            inst_ptrs[b] = ctypes.cast(ptrs, ctypes.c_void_p)
            len_ptrs[b] = ctypes.cast(lens, ctypes.c_void_p)
        bufs = [ctypes.create_string_buffer(bytes(p_), max(len(p_), 1)) for p_ in proofs]
        proof_ptrs = (ctypes.c_void_p * len(proofs))(*[ctypes.cast(b_, ctypes.c_void_p) for b_ in bufs])
        proof_lens = (ctypes.c_size_t * len(proofs))(*[len(p_) for p_ in proofs])
        return keep + [bufs], inst_ptrs, len_ptrs, proof_ptrs, proof_lens

    def verify_accumulators(self, vk: "VerifyingKey", proofs: Sequence[bytes], instances: Sequence[Sequence[np.ndarray]], transcript_kind: int = 0,
                            multiopen: int = 0, acc_indices: Sequence[Sequence[Tuple[int, int]]] = ()):
        """succinct verification (zk_verify_accumulators): per proof the KZG accumulator of its openings, then the accumulators its
        instances carry at acc_indices (per accumulator 12 (column, row) cells).  Returns (lhs, rhs, ok): lhs / rhs of shape
        (count, 1 + len(acc_indices), 8) u64 affine Montgomery, ok a list of bools.  NO pairing is done: decide every accumulator
        with accumulator_check, or combine them with zk_host_accumulate first.  ok[b] False: proof b is malformed or a carried
        accumulator does not decode; its outputs are zero."""
        keep, inst_ptrs, len_ptrs, proof_ptrs, proof_lens = self._proof_args("verify_accumulators", vk, proofs, instances)
        num_prior = len(acc_indices)
        idx = np.ascontiguousarray([[int(c), int(r)] for acc in acc_indices for c, r in acc], dtype=np.uint32).reshape(-1, 2)
        if len(idx) != 12 * num_prior:
            raise ZkError("verify_accumulators: an accumulator is 12 (column, row) cells")
        lhs = np.zeros((len(proofs), 1 + num_prior, 8), dtype=np.uint64)
        rhs = np.zeros_like(lhs)
        ok = (ctypes.c_int * len(proofs))()
        self._ck(lib().zk_verify_accumulators(self.h, vk.h, ctypes.c_size_t(len(proofs)), inst_ptrs, len_ptrs, proof_ptrs, proof_lens,
                                              ctypes.c_int(transcript_kind), ctypes.c_int(multiopen), _host_ptr(idx) if num_prior else None,
                                              ctypes.c_size_t(num_prior), _host_ptr(lhs), _host_ptr(rhs), ok))
        return lhs, rhs, [v == 1 for v in ok]

    def verify_proofs(self, vk: "VerifyingKey", proofs: Sequence[bytes], instances: Sequence[Sequence[np.ndarray]], transcript_kind: int = 0,
                      multiopen: int = 0, g2: bytes = b"", s_g2: bytes = b"") -> bool:
        """halo2 verify_proof (zk_verify_proofs): one proof = SingleStrategy, several = AccumulatorStrategy (one MSM and one pairing
        check for all).  instances[b]: proof b's instance columns, (len, 4) u64 Montgomery each, absorbed as given -- a column of
        exactly 2^k rows is the full-column image zk_proof_begin takes and stands for its usable rows.  g2 / s_g2: [1]G2 / [s]G2,
        128 B Montgomery.  Malformed proofs are rejected (False); bad arguments raise."""
        keep, inst_ptrs, len_ptrs, proof_ptrs, proof_lens = self._proof_args("verify_proofs", vk, proofs, instances)
        g2b, sg2b = bytes(g2), bytes(s_g2)
        if len(g2b) != 128 or len(sg2b) != 128:
            raise ZkError("verify_proofs: g2 and s_g2 are 128-byte G2 points")
        ok = ctypes.c_int(-1)
        self._ck(lib().zk_verify_proofs(self.h, vk.h, ctypes.c_size_t(len(proofs)), inst_ptrs, len_ptrs, proof_ptrs, proof_lens,
                                        ctypes.c_int(transcript_kind), ctypes.c_int(multiopen), ctypes.c_char_p(g2b), ctypes.c_char_p(sg2b),
                                        ctypes.byref(ok)))
        return ok.value == 1

    def create_proof(self, pk: "ProvingKey", advice: Sequence[np.ndarray], instance: Sequence[np.ndarray], seed: bytes = bytes(16)) -> bytes:
        adv = [np.ascontiguousarray(a, dtype=np.uint64) for a in advice]
        ins = [np.ascontiguousarray(a, dtype=np.uint64) for a in instance]
        pa = (ctypes.c_void_p * max(len(adv), 1))(*[a.ctypes.data for a in adv])
        pi = (ctypes.c_void_p * max(len(ins), 1))(*[a.ctypes.data for a in ins])
        cap = 1 << 20
        out = ctypes.create_string_buffer(cap)
        n = ctypes.c_size_t()
        assert len(seed) == 16
        self._ck(lib().zk_create_proof(self.h, pk.h, pa, pi, ctypes.c_char_p(seed), out, ctypes.c_size_t(cap), ctypes.byref(n)))
        return out.raw[:n.value]

    def mock_verify(self, pk: "ProvingKey", advice: Sequence[np.ndarray], instance: Sequence[np.ndarray], challenges: Optional[np.ndarray] = None,
                    gate_rows: Optional[Sequence[int]] = None, lookup_rows: Optional[Sequence[int]] = None, cap: int = 4096):
        """zk_mock_verify (halo2 dev::MockProver::verify_par / verify_at_rows_par): (failures, total) with failures the first
        `cap` records (kind, index, sub, row), sorted; kinds 1 gate, 2 lookup, 3 permutation.  challenges: (c, 4) u64
        Montgomery or None for MockProver's own."""
        adv = [np.ascontiguousarray(a, dtype=np.uint64) for a in advice]
        ins = [np.ascontiguousarray(a, dtype=np.uint64) for a in instance]
        pa = (ctypes.c_void_p * max(len(adv), 1))(*[a.ctypes.data for a in adv])
        pi = (ctypes.c_void_p * max(len(ins), 1))(*[a.ctypes.data for a in ins])
        ch = None if challenges is None else np.ascontiguousarray(challenges, dtype=np.uint64)
        gr = None if gate_rows is None else np.ascontiguousarray(gate_rows, dtype=np.uint32)
        lr = None if lookup_rows is None else np.ascontiguousarray(lookup_rows, dtype=np.uint32)
        out = np.zeros((max(cap, 1), 4), dtype=np.uint32)
        total = ctypes.c_size_t()
        self._ck(lib().zk_mock_verify(self.h, pk.h, pa, pi, None if ch is None else _host_ptr(ch),
                                      None if gr is None else _host_ptr(gr), ctypes.c_size_t(0 if gr is None else len(gr)),
                                      None if lr is None else _host_ptr(lr), ctypes.c_size_t(0 if lr is None else len(lr)),
                                      _host_ptr(out), ctypes.c_size_t(cap), ctypes.byref(total)))
        return [tuple(int(v) for v in r) for r in out[:min(total.value, cap)]], total.value

    def proof_session(self, pk: "ProvingKey", instance: Sequence[np.ndarray], seed: bytes = bytes(16), instance_slices: bool = False) -> "ProofSession":
        return ProofSession(self, pk, instance, seed, instance_slices)

    # ---- G1 element-wise
    def g1_affine_add(self, a: DeviceBuffer, b: DeviceBuffer, out: DeviceBuffer, n: int):
        self._ck(lib().zk_g1_affine_add_vec(self.h, ctypes.c_void_p(a.ptr), ctypes.c_void_p(b.ptr), ctypes.c_void_p(out.ptr), ctypes.c_size_t(n)))

    def g1_mul(self, bases: DeviceBuffer, scalars: DeviceBuffer, out: DeviceBuffer, n: int):
        self._ck(lib().zk_g1_mul_vec(self.h, ctypes.c_void_p(bases.ptr), ctypes.c_void_p(scalars.ptr), ctypes.c_void_p(out.ptr), ctypes.c_size_t(n)))


def mock_challenges(count: int) -> np.ndarray:
    """zk_host_mock_challenges: the challenges halo2's MockProver hands a circuit, (count, 4) u64 Montgomery Fr (host only)"""
    out = np.zeros((max(count, 1), 4), dtype=np.uint64)
    rc = lib().zk_host_mock_challenges(ctypes.c_uint32(count), _host_ptr(out))
    if rc != 0:
        raise ZkError(f"zk_host_mock_challenges failed with status {rc}")
    return out[:count]


def accumulator_from_limbs(limbs: np.ndarray):
    """zk_host_accumulator_from_limbs: 12 Montgomery Fr cells, (12, 4) u64 -> (lhs, rhs, ok); lhs / rhs (8,) u64 affine Montgomery,
    zero when ok is False (a limb of 2^88 or more, a coordinate of p or more, a point off the curve).  Host only."""
    cells = np.ascontiguousarray(limbs, dtype=np.uint64).reshape(12, 4)
    lhs, rhs = np.zeros(8, dtype=np.uint64), np.zeros(8, dtype=np.uint64)
    ok = ctypes.c_int(-1)
    rc = lib().zk_host_accumulator_from_limbs(_host_ptr(cells), _host_ptr(lhs), _host_ptr(rhs), ctypes.byref(ok))
    if rc != 0:
        raise ZkError(f"zk_host_accumulator_from_limbs failed with status {rc}")
    return lhs, rhs, ok.value == 1


def version() -> str:
    return lib().zk_version().decode()


def g2_setup(s_mont: np.ndarray):
    """unsafe_setup_with_s, G2 half: (generator, s * generator) as 128-byte RawBytes each (host only)."""
    g2, sg2 = ctypes.create_string_buffer(128), ctypes.create_string_buffer(128)
    rc = lib().zk_g2_setup(_host_ptr(np.ascontiguousarray(s_mont)), g2, sg2)
    if rc != 0:
        raise ZkError(f"zk_g2_setup failed: {rc}")
    return g2.raw, sg2.raw


def params_file_len(k: int, fmt: int = 2) -> int:
    return int(lib().zk_params_file_len(ctypes.c_uint32(k), ctypes.c_int(fmt)))

"""CPU: the running RLC of typed cells (ZK_OP_SCAN_RLC = 9, ZK_OP_SCAN_RLC_REV = 10, zk_scan_rlc) is a pair of ops of zk_field_vec_op
-- in the header as #defines and a struct OUTSIDE the op enum (whose five names and values stay), described in the ONE comment in front
of the prototype, in the Python binding (constants, the ctypes struct, Context.scan_rlc), in the C++ mirror, the Rust declarations and
the documents -- and it came without a new entry point: the library still exports exactly the 146 functions the header declares, none
of them named after a scan or an RLC."""
import ctypes
import inspect
import os
import re
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header_body(zk):
    return re.sub(r"/\*.*?\*/", "", open(zk.binding.HEADER_PATH).read(), flags=re.S)


def _exported(zk):
    """the zk_* functions in the library's dynamic symbol table"""
    nm = shutil.which("nm") or shutil.which("llvm-nm") or "/opt/rocm/llvm/bin/llvm-nm"
    out = subprocess.run([nm, "-D", "--defined-only", zk.binding.LIB_PATH], capture_output=True, text=True, check=True).stdout
    return sorted({ln.split()[-1] for ln in out.splitlines() if len(ln.split()) >= 3 and ln.split()[-2] in "TW" and ln.split()[-1].startswith("zk_")})


def test_header_defines_the_ops_and_the_struct_outside_the_op_enum(zk):
    body = _header_body(zk)
    assert re.search(r"^#define\s+ZK_OP_SCAN_RLC\s+9\s*$", body, flags=re.M)
    assert re.search(r"^#define\s+ZK_OP_SCAN_RLC_REV\s+10\s*$", body, flags=re.M)
    struct = re.search(r"typedef\s+struct\s+zk_scan_rlc\s*\{([^}]*)\}\s*zk_scan_rlc\s*;", body)
    assert struct, "typedef struct zk_scan_rlc"
    fields = [re.sub(r"\s+", " ", f).strip() for f in struct.group(1).split(";") if f.strip()]
    assert fields == ["const void* d_cells", "uint32_t width", "const uint8_t* d_kinds"]
    enums = re.findall(r"\benum\s*\{([^}]*)\}", body)
    ops = [e for e in enums if "ZK_OP_ADD" in e]
    assert len(ops) == 1
    assert not any("SCAN_RLC" in e for e in enums)
    values = {name: int(v) for name, v in re.findall(r"\b(ZK_OP_[A-Z_]+)\s*=\s*(\d+)", ops[0])}
    assert values == {"ZK_OP_ADD": 0, "ZK_OP_SUB": 1, "ZK_OP_MUL": 2, "ZK_OP_SCAN_AFFINE": 3, "ZK_OP_SCAN_AFFINE_REV": 4}
    assert re.search(r"^#define\s+ZK_OP_ROW_RLC\s+8\s*$", body, flags=re.M)


def test_header_comment_describes_the_ops(zk):
    text = open(zk.binding.HEADER_PATH).read()
    comment = text[:text.index("int zk_field_vec_op(")].rsplit("/*", 1)[1]
    assert comment.rstrip().endswith("*/") and comment.count("*/") == 1, "one comment, directly in front of the prototype"
    for word in ("ZK_OP_SCAN_RLC", "ZK_OP_SCAN_RLC_REV", "zk_scan_rlc", "fr_scan_rlc", "HOST pointers", "d_kinds[i] & 3", "only the low two bits",
                 "out[-1] = z0", "out[n]  = z0", "m[kind_i] * out[i-1] + w[kind_i] * cell[i]", "m[kind_i] * out[i+1] + w[kind_i] * cell[i]",
                 "m_0, w_0, m_1, w_1, m_2, w_2,", "9 x 32 B", "n * (width + (d_kinds ? 1 : 0) + 32)", "undefined VALUES from its row on",
                 "validated before n is looked at", "overlaps neither the cells"):
        assert word in comment, word
    # what the comment said before stays
    for word in ("ZK_OP_ROW_RLC", "fr_row_rlc", "zk_row_rlc", "ZK_OP_SCAN_AFFINE", "ZK_OP_SCAN_AFFINE_REV", "a[i] * out[i-1] + b[i]", "a[i] * out[i+1] + b[i]", "fr_scan_affine"):
        assert word in comment, word
    assert re.sub(r"\s*\*/\s*$", "", comment).rstrip().endswith("Other op values (5, 6, 7, 11, ...) are refused.")


def test_binding_exposes_the_constants_the_struct_and_the_method(zk):
    assert (zk.OP_SCAN_RLC, zk.OP_SCAN_RLC_REV) == (zk.binding.OP_SCAN_RLC, zk.binding.OP_SCAN_RLC_REV) == (9, 10)
    assert zk.OP_ROW_RLC == 8 and (zk.OP_SCAN_AFFINE, zk.OP_SCAN_AFFINE_REV) == (3, 4) and (zk.OP_ADD, zk.OP_SUB, zk.OP_MUL) == (0, 1, 2)
    sig = inspect.signature(zk.binding.Context.scan_rlc)
    assert list(sig.parameters) == ["self", "cells", "width", "kinds", "table", "n", "out", "z0", "reverse"]
    assert sig.parameters["z0"].default is None and sig.parameters["reverse"].default is False
    desc = zk.binding._ScanRlc
    assert issubclass(desc, ctypes.Structure)
    assert [(name, ctype) for name, ctype in desc._fields_] == [("d_cells", ctypes.c_void_p), ("width", ctypes.c_uint32), ("d_kinds", ctypes.c_void_p)]
    assert (desc.d_cells.offset, desc.width.offset, desc.d_kinds.offset, ctypes.sizeof(desc)) == (0, 8, 16, 24)


def test_mirror_rust_declarations_and_documents_name_the_op():
    mirror = open(os.path.join(ROOT, "include", "zkmi355_halo2.hpp")).read()
    assert re.search(r"\binline void scan_rlc\(", mirror) and "ZK_OP_SCAN_RLC_REV" in mirror and "zk_scan_rlc" in mirror
    assert mirror.index("inline void row_rlc(") < mirror.index("inline void scan_rlc(")
    ffi = open(os.path.join(ROOT, "shim", "halo2_proofs", "src", "zkmi355", "ffi.rs")).read()
    assert re.search(r"pub const ZK_OP_SCAN_RLC:\s*\w+\s*=\s*9;", ffi) and re.search(r"pub const ZK_OP_SCAN_RLC_REV:\s*\w+\s*=\s*10;", ffi)
    assert re.search(r"pub struct zk_scan_rlc\b", ffi)
    assert not re.search(r"\bfn\s+zk_\w*(scan|rlc)", ffi), "no new function in the Rust declarations"
    for rel in ("README.md", "INTEGRATION.md", "DESIGN.md"):
        assert "ZK_OP_SCAN_RLC" in open(os.path.join(ROOT, rel)).read(), rel
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for word in ("value_rlc", "data_rlc", "rlc_acc", "ZK_OP_SCAN_RLC_REV"):
        assert word in integration, word
    assert os.path.exists(os.path.join(ROOT, "tools", "scan_rlc_time.py"))


def test_no_entry_point_was_added(zk):
    declared = sorted(set(re.findall(r"\b(zk_[a-z0-9_]+)\s*\(", _header_body(zk))))
    exported = _exported(zk)
    assert declared == exported, (sorted(set(declared) - set(exported)), sorted(set(exported) - set(declared)))
    assert len(exported) == 146
    assert not [name for name in exported if "scan" in name or "rlc" in name], "the running RLC is an op of zk_field_vec_op, not an entry point"
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "The C ABI has 146 entry points" in readme

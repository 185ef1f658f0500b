"""CPU: the inverse-or-zero of a row RLC of typed cells (ZK_OP_ROW_INV0 = 12, zk_row_inv0) is an op of zk_field_vec_op -- in the header
as a #define and a struct OUTSIDE the op enum (whose five names and values stay), described in the ONE comment in front of the
prototype, in the Python binding (constant, the ctypes struct, Context.row_inv0), in the C++ mirror, the Rust declarations, the
documents and the timing tool -- and it came without a new entry point: the library still exports exactly the 146 functions the
header declares, none of them named after an inverse-or-zero."""
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


def test_header_defines_the_op_and_the_struct_outside_the_op_enum(zk):
    body = _header_body(zk)
    assert re.search(r"^#define\s+ZK_OP_ROW_INV0\s+12\s*$", body, flags=re.M)
    struct = re.search(r"typedef\s+struct\s+zk_row_inv0\s*\{([^}]*)\}\s*zk_row_inv0\s*;", body)
    assert struct, "typedef struct zk_row_inv0"
    fields = [re.sub(r"\s+", " ", f).strip() for f in struct.group(1).split(";") if f.strip()]
    assert fields == ["uint32_t count", "const void* const* d_cols", "const uint8_t* widths", "const void* d_num", "uint32_t num_width"]
    enums = re.findall(r"\benum\s*\{([^}]*)\}", body)
    ops = [e for e in enums if "ZK_OP_ADD" in e]
    assert len(ops) == 1
    assert not any("INV0" in e for e in enums)
    values = {name: int(v) for name, v in re.findall(r"\b(ZK_OP_[A-Z_0-9]+)\s*=\s*(\d+)", ops[0])}
    assert values == {"ZK_OP_ADD": 0, "ZK_OP_SUB": 1, "ZK_OP_MUL": 2, "ZK_OP_SCAN_AFFINE": 3, "ZK_OP_SCAN_AFFINE_REV": 4}
    for name, value in (("ZK_OP_ROW_RLC", 8), ("ZK_OP_SCAN_RLC", 9), ("ZK_OP_SCAN_RLC_REV", 10)):
        assert re.search(rf"^#define\s+{name}\s+{value}\s*$", body, flags=re.M), name


def test_header_comment_describes_the_op(zk):
    text = open(zk.binding.HEADER_PATH).read()
    comment = text[:text.index("int zk_field_vec_op(")].rsplit("/*", 1)[1]
    assert comment.rstrip().endswith("*/") and comment.count("*/") == 1, "one comment, directly in front of the prototype"
    for word in ("ZK_OP_ROW_INV0", "zk_row_inv0", "fr_row_inv0", "inv0", "d_num", "num_width", "HOST pointers", "inv0(0) = 0", "value 12", "11 stays refused",
                 "validated before n is looked at", "undefined VALUE", "1024 rows"):
        assert word in comment, word
    # what the comment said before stays, in its order
    for word in ("ZK_OP_ROW_RLC", "fr_row_rlc", "zk_row_rlc", "ZK_OP_SCAN_RLC", "ZK_OP_SCAN_RLC_REV", "zk_scan_rlc", "fr_scan_rlc", "ZK_OP_SCAN_AFFINE", "fr_scan_affine"):
        assert word in comment, word
    assert comment.index("fr_scan_rlc") < comment.index("ZK_OP_ROW_INV0")
    assert re.sub(r"\s*\*/\s*$", "", comment).rstrip().endswith("Other op values (5, 6, 7, 11, ...) are refused.")


def test_binding_exposes_the_constant_the_struct_and_the_method(zk):
    assert zk.OP_ROW_INV0 == zk.binding.OP_ROW_INV0 == 12
    assert zk.OP_ROW_RLC == 8 and (zk.OP_SCAN_RLC, zk.OP_SCAN_RLC_REV) == (9, 10) and (zk.OP_SCAN_AFFINE, zk.OP_SCAN_AFFINE_REV) == (3, 4)
    sig = inspect.signature(zk.binding.Context.row_inv0)
    assert list(sig.parameters) == ["self", "cols", "widths", "weights", "n", "out", "constant", "num", "num_width"]
    assert sig.parameters["constant"].default is None and sig.parameters["num"].default is None and sig.parameters["num_width"].default == 32
    desc = zk.binding._RowInv0
    assert issubclass(desc, ctypes.Structure)
    assert [name for name, _ in desc._fields_] == ["count", "d_cols", "widths", "d_num", "num_width"]
    assert (desc.count.offset, desc.d_cols.offset, desc.widths.offset, desc.d_num.offset, desc.num_width.offset, ctypes.sizeof(desc)) == (0, 8, 16, 24, 32, 40)
    assert dict(desc._fields_)["count"] is ctypes.c_uint32 and dict(desc._fields_)["d_num"] is ctypes.c_void_p and dict(desc._fields_)["num_width"] is ctypes.c_uint32


def test_mirror_rust_declarations_documents_and_tool_name_the_op():
    mirror = open(os.path.join(ROOT, "include", "zkmi355_halo2.hpp")).read()
    assert re.search(r"\binline void row_inv0\(", mirror) and "ZK_OP_ROW_INV0" in mirror and "zk_row_inv0" in mirror
    assert mirror.index("inline void scan_affine(") < mirror.index("inline void row_rlc(") < mirror.index("inline void scan_rlc(") < mirror.index("inline void row_inv0(")
    ffi = open(os.path.join(ROOT, "shim", "halo2_proofs", "src", "zkmi355", "ffi.rs")).read()
    assert re.search(r"pub const ZK_OP_ROW_INV0:\s*\w+\s*=\s*12;", ffi)
    struct = re.search(r"pub struct zk_row_inv0\s*\{([^}]*)\}", ffi)
    assert struct and re.findall(r"pub (\w+):", struct.group(1)) == ["count", "d_cols", "widths", "d_num", "num_width"]
    assert not re.search(r"\bfn\s+zk_\w*(inv0|row_)", ffi), "no new function in the Rust declarations"
    for rel in ("README.md", "INTEGRATION.md", "DESIGN.md", os.path.join("profiles", "README.md"), os.path.join("tools", "README.md")):
        assert "ZK_OP_ROW_INV0" in open(os.path.join(ROOT, rel)).read() or "row_inv0" in open(os.path.join(ROOT, rel)).read(), rel
    for rel in ("README.md", "INTEGRATION.md", "DESIGN.md"):
        assert "ZK_OP_ROW_INV0" in open(os.path.join(ROOT, rel)).read(), rel
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for word in ("value_inv", "IsEqual", "Assigned::Rational", "batch_invert_assigned", "row_inv0"):
        assert word in integration, word
    tool = open(os.path.join(ROOT, "tools", "row_inv0_time.py")).read()
    assert "row_inv0" in tool and "fr_batch_invert" in tool and "row_rlc" in tool
    assert os.path.exists(os.path.join(ROOT, "profiles", "r23_row_inv0.md"))


def test_no_entry_point_was_added(zk):
    declared = sorted(set(re.findall(r"\b(zk_[a-z0-9_]+)\s*\(", _header_body(zk))))
    exported = _exported(zk)
    assert declared == exported, (sorted(set(declared) - set(exported)), sorted(set(exported) - set(declared)))
    assert len(exported) == 146
    assert not [name for name in exported if "inv0" in name], "the row inverse is an op of zk_field_vec_op, not an entry point"
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "The C ABI has 146 entry points" in readme

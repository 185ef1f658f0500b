"""CPU: the row RLC of typed cells (ZK_OP_ROW_RLC = 8, zk_row_rlc) is an op of zk_field_vec_op -- in the header as a #define and a
struct OUTSIDE the op enum (whose five names stay), described in the comment in front of the prototype together with the scan ops, in
the Python binding (constant and Context.row_rlc), in the C++ mirror, the Rust declarations and the documents -- and it came without a
new entry point: the library still exports exactly the functions the header declares (145 then, 146 since zk_host_quotient_launch)."""
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
    assert re.search(r"^#define\s+ZK_OP_ROW_RLC\s+8\s*$", body, flags=re.M)
    struct = re.search(r"typedef\s+struct\s+zk_row_rlc\s*\{([^}]*)\}\s*zk_row_rlc\s*;", body)
    assert struct, "typedef struct zk_row_rlc"
    fields = [re.sub(r"\s+", " ", f).strip() for f in struct.group(1).split(";") if f.strip()]
    assert fields == ["uint32_t count", "const void* const* d_cols", "const uint8_t* widths"]
    enums = re.findall(r"\benum\s*\{([^}]*)\}", body)
    ops = [e for e in enums if "ZK_OP_ADD" in e]
    assert len(ops) == 1 and "ROW_RLC" not in ops[0]
    assert not any("ZK_OP_ROW_RLC" in e for e in enums)
    assert [int(v) for v in re.findall(r"=\s*(\d+)", ops[0])] == [0, 1, 2, 3, 4]      # 5, 6, 7 stay free (and refused); 8 is not one of them


def test_header_comment_describes_the_op_beside_the_scan_ops(zk):
    text = open(zk.binding.HEADER_PATH).read()
    comment = text[:text.index("int zk_field_vec_op(")].rsplit("/*", 1)[1]
    for word in ("ZK_OP_ROW_RLC", "fr_row_rlc", "zk_row_rlc", "HOST pointers", "ZK_OP_SCAN_AFFINE", "ZK_OP_SCAN_AFFINE_REV", "fr_scan_affine"):
        assert word in comment, word
    assert comment.rstrip().endswith("*/") and comment.count("*/") == 1, "one comment, directly in front of the prototype"


def test_binding_exposes_the_constant_and_the_method(zk):
    assert zk.OP_ROW_RLC == zk.binding.OP_ROW_RLC == 8
    assert (zk.OP_SCAN_AFFINE, zk.OP_SCAN_AFFINE_REV) == (3, 4)
    sig = inspect.signature(zk.binding.Context.row_rlc)
    assert list(sig.parameters) == ["self", "cols", "widths", "weights", "n", "out", "constant"]
    assert sig.parameters["constant"].default is None


def test_mirror_rust_declarations_and_documents_name_the_op():
    mirror = open(os.path.join(ROOT, "include", "zkmi355_halo2.hpp")).read()
    assert re.search(r"\binline void row_rlc\(", mirror) and "ZK_OP_ROW_RLC" in mirror and "zk_row_rlc" in mirror
    assert mirror.index("inline void scan_affine(") < mirror.index("inline void row_rlc(")
    ffi = open(os.path.join(ROOT, "shim", "halo2_proofs", "src", "zkmi355", "ffi.rs")).read()
    assert re.search(r"pub const ZK_OP_ROW_RLC:\s*\w+\s*=\s*8;", ffi) and re.search(r"pub struct zk_row_rlc\b", ffi)
    assert not re.search(r"\bfn\s+zk_\w*row_rlc", ffi), "no new function in the Rust declarations"
    for rel in ("README.md", "INTEGRATION.md", "DESIGN.md"):
        assert "ZK_OP_ROW_RLC" in open(os.path.join(ROOT, rel)).read(), rel
    assert os.path.exists(os.path.join(ROOT, "tools", "row_rlc_time.py"))


def test_no_entry_point_was_added(zk):
    declared = sorted(set(re.findall(r"\b(zk_[a-z0-9_]+)\s*\(", _header_body(zk))))
    exported = _exported(zk)
    assert declared == exported, (sorted(set(declared) - set(exported)), sorted(set(exported) - set(declared)))
    assert len(exported) == 146          # 145 when the op was added; zk_host_quotient_launch since
    assert not [name for name in exported if "rlc" in name], "the row RLC is an op of zk_field_vec_op, not an entry point"
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "The C ABI has 146 entry points" in readme

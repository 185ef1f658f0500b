"""CPU: the affine scan ops of zk_field_vec_op (ZK_OP_SCAN_AFFINE = 3, ZK_OP_SCAN_AFFINE_REV = 4) are in the header's op enum, in the
Python binding (constants and Context.scan_affine), in the C++ mirror and in the documents -- and they came without a new entry point:
the library still exports exactly what the header declares."""
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


def test_header_op_enum_has_both_scan_ops(zk):
    enums = re.findall(r"\benum\s*\{([^}]*)\}", _header_body(zk))
    ops = [e for e in enums if "ZK_OP_ADD" in e]
    assert len(ops) == 1, "one op enum"
    values = {name: int(v) for name, v in re.findall(r"\b(ZK_OP_[A-Z_]+)\s*=\s*(\d+)", ops[0])}
    assert values == {"ZK_OP_ADD": 0, "ZK_OP_SUB": 1, "ZK_OP_MUL": 2, "ZK_OP_SCAN_AFFINE": 3, "ZK_OP_SCAN_AFFINE_REV": 4}


def test_header_comment_describes_the_scan_ops(zk):
    text = open(zk.binding.HEADER_PATH).read()
    comment = text[:text.index("int zk_field_vec_op(")].rsplit("/*", 1)[1]
    for word in ("ZK_OP_SCAN_AFFINE", "ZK_OP_SCAN_AFFINE_REV", "a[i] * out[i-1] + b[i]", "a[i] * out[i+1] + b[i]", "fr_scan_affine"):
        assert word in comment, word


def test_binding_exposes_constants_and_method(zk):
    assert (zk.OP_SCAN_AFFINE, zk.OP_SCAN_AFFINE_REV) == (3, 4)
    assert (zk.binding.OP_SCAN_AFFINE, zk.binding.OP_SCAN_AFFINE_REV) == (3, 4)
    assert (zk.OP_ADD, zk.OP_SUB, zk.OP_MUL) == (0, 1, 2)
    params = list(inspect.signature(zk.binding.Context.scan_affine).parameters)
    assert params == ["self", "a", "b", "out", "n", "reverse"]
    assert inspect.signature(zk.binding.Context.scan_affine).parameters["reverse"].default is False


def test_cpp_mirror_and_docs_name_the_op():
    mirror = open(os.path.join(ROOT, "include", "zkmi355_halo2.hpp")).read()
    assert re.search(r"\binline void scan_affine\(", mirror) and "ZK_OP_SCAN_AFFINE_REV" in mirror
    for rel in ("README.md", "INTEGRATION.md", "DESIGN.md"):
        assert "ZK_OP_SCAN_AFFINE" in open(os.path.join(ROOT, rel)).read(), rel


def test_no_entry_point_was_added(zk):
    declared = sorted(set(re.findall(r"\b(zk_[a-z0-9_]+)\s*\(", _header_body(zk))))
    exported = _exported(zk)
    assert declared == exported, (sorted(set(declared) - set(exported)), sorted(set(exported) - set(declared)))
    assert not [name for name in exported if "scan" in name], "the scan ops are ops of zk_field_vec_op, not entry points"
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert f"The C ABI has {len(exported)} entry points" in readme

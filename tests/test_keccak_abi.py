"""CPU: the Keccak table columns (ZK_OP_KECCAK = 16, zk_keccak) are an op of zk_field_vec_op -- in the header as a #define and a struct
OUTSIDE the op enum (whose five names and values stay), described in the ONE comment in front of the prototype behind the Poseidon
text, in the Python binding (the constant, the ctypes struct with the C layout, Context.keccak), in the C++ mirror, the Rust
declarations, the documents, the timing tool and the profile -- and it came without a new entry point: the library still exports
exactly the 146 functions the header declares, the host hash being the only one named after Keccak."""
import ctypes
import inspect
import os
import re
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ["d_bytes", "total_bytes", "d_offsets", "d_lens", "d_digest", "d_input_rlc", "index_width", "flags"]


def _header_body(zk):
    return re.sub(r"/\*.*?\*/", "", open(zk.binding.HEADER_PATH).read(), flags=re.S)


def _exported(zk):
    """the zk_* functions in the library's dynamic symbol table"""
    nm = shutil.which("nm") or shutil.which("llvm-nm") or "/opt/rocm/llvm/bin/llvm-nm"
    out = subprocess.run([nm, "-D", "--defined-only", zk.binding.LIB_PATH], capture_output=True, text=True, check=True).stdout
    return sorted({ln.split()[-1] for ln in out.splitlines() if len(ln.split()) >= 3 and ln.split()[-2] in "TW" and ln.split()[-1].startswith("zk_")})


def test_header_defines_the_op_and_the_struct_outside_the_op_enum(zk):
    body = _header_body(zk)
    assert re.search(r"^#define\s+ZK_OP_KECCAK\s+16\s*$", body, flags=re.M)
    struct = re.search(r"typedef\s+struct\s+zk_keccak\s*\{([^}]*)\}\s*zk_keccak\s*;", body)
    assert struct, "typedef struct zk_keccak"
    fields = [re.sub(r"\s+", " ", f).strip() for f in struct.group(1).split(";") if f.strip()]
    assert fields == ["const void* d_bytes", "uint64_t total_bytes", "const void* d_offsets", "const void* d_lens", "void* d_digest", "void* d_input_rlc",
                      "uint8_t index_width", "uint8_t flags"]
    enums = re.findall(r"\benum\s*\{([^}]*)\}", body)
    ops = [e for e in enums if "ZK_OP_ADD" in e]
    assert len(ops) == 1
    assert not any("KECCAK" in e for e in enums if "ZK_OP_" in e)
    values = {name: int(v) for name, v in re.findall(r"\b(ZK_OP_[A-Z_0-9]+)\s*=\s*(\d+)", ops[0])}
    assert values == {"ZK_OP_ADD": 0, "ZK_OP_SUB": 1, "ZK_OP_MUL": 2, "ZK_OP_SCAN_AFFINE": 3, "ZK_OP_SCAN_AFFINE_REV": 4}
    for name, value in (("ZK_OP_ROW_RLC", 8), ("ZK_OP_SCAN_RLC", 9), ("ZK_OP_SCAN_RLC_REV", 10), ("ZK_OP_ROW_INV0", 12), ("ZK_OP_POSEIDON", 14)):
        assert re.search(rf"^#define\s+{name}\s+{value}\s*$", body, flags=re.M), name


def test_header_comment_describes_the_op(zk):
    text = open(zk.binding.HEADER_PATH).read()
    comment = text[:text.index("int zk_field_vec_op(")].rsplit("/*", 1)[1]
    assert comment.rstrip().endswith("*/") and comment.count("*/") == 1, "one comment, directly in front of the prototype"
    for word in ("ZK_OP_KECCAK", "zk_keccak", "fr_keccak", "value 16", "15 stays refused", "HOST pointers", "r_out", "r_in", "d_digest", "d_input_rlc", "index_width",
                 "total_bytes", "input_len", "zk_proof_advice_phase_typed_dev", "validated before n is looked at", "cannot wrap", "reads nothing", "zk_host_keccak256",
                 "output_rlc", "hash_rlc", "total_bytes stands in"):
        assert word in comment, word
    # what the comment said before stays, in its order
    for word in ("ZK_OP_ROW_RLC", "fr_row_rlc", "ZK_OP_SCAN_RLC", "fr_scan_rlc", "ZK_OP_SCAN_AFFINE", "fr_scan_affine", "ZK_OP_ROW_INV0", "fr_row_inv0", "11 stays refused",
                 "ZK_OP_POSEIDON", "fr_poseidon", "13 stays refused"):
        assert word in comment, word
    assert comment.index("fr_row_inv0") < comment.index("ZK_OP_POSEIDON") < comment.index("fr_poseidon") < comment.index("ZK_OP_KECCAK")
    assert re.sub(r"\s*\*/\s*$", "", comment).rstrip().endswith("Other op values (5, 6, 7, 11, ...) are refused.")


def test_binding_exposes_the_constant_the_struct_and_the_method(zk):
    assert zk.OP_KECCAK == zk.binding.OP_KECCAK == 16
    assert zk.OP_POSEIDON == 14 and zk.OP_ROW_INV0 == 12 and zk.OP_ROW_RLC == 8 and (zk.OP_SCAN_RLC, zk.OP_SCAN_RLC_REV) == (9, 10)
    sig = inspect.signature(zk.binding.Context.keccak)
    assert list(sig.parameters) == ["self", "data", "total_bytes", "offsets", "lens", "index_width", "n", "out", "r_out", "r_in", "digest", "input_rlc"]
    defaults = {k: v.default for k, v in sig.parameters.items() if v.default is not inspect.Parameter.empty}
    assert defaults == {"r_in": None, "digest": None, "input_rlc": None}
    assert "ZK_OP_KECCAK" in zk.binding.Context.keccak.__doc__
    desc = zk.binding._Keccak
    assert issubclass(desc, ctypes.Structure)
    assert [name for name, _ in desc._fields_] == FIELDS
    # the C layout: five pointers and a 64-bit count at 8-byte steps, two bytes, padded to the pointer alignment
    assert [getattr(desc, name).offset for name, _ in desc._fields_] == [0, 8, 16, 24, 32, 40, 48, 49] and ctypes.sizeof(desc) == 56
    types = dict(desc._fields_)
    assert types["total_bytes"] is ctypes.c_uint64 and types["index_width"] is ctypes.c_uint8 and types["flags"] is ctypes.c_uint8
    assert all(types[name] is ctypes.c_void_p for name in FIELDS if name.startswith("d_"))


def test_the_struct_has_the_size_and_offsets_the_compiler_gives_it(zk, tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang") or "/opt/rocm/llvm/bin/clang"
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "zkmi355.h"\nint main(void) { printf("%zu", sizeof(zk_keccak));\n'
                   + "".join(f'printf(" %zu", offsetof(zk_keccak, {name}));\n' for name in FIELDS) + "return ZK_OP_KECCAK == 16 ? 0 : 1; }\n")
    exe = tmp_path / "layout"
    subprocess.run([cc, "-I", os.path.dirname(zk.binding.HEADER_PATH), str(src), "-o", str(exe)], check=True, timeout=120)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True, timeout=60).stdout.split()]
    desc = zk.binding._Keccak
    assert got == [ctypes.sizeof(desc)] + [getattr(desc, name).offset for name in FIELDS]


def test_mirror_rust_declarations_documents_tool_and_profile_name_the_op():
    mirror = open(os.path.join(ROOT, "include", "zkmi355_halo2.hpp")).read()
    assert re.search(r"\binline void keccak\(", mirror) and "ZK_OP_KECCAK" in mirror and "zk_keccak" in mirror
    assert mirror.index("inline void row_inv0(") < mirror.index("inline void poseidon(") < mirror.index("inline void keccak(")
    ffi = open(os.path.join(ROOT, "shim", "halo2_proofs", "src", "zkmi355", "ffi.rs")).read()
    assert re.search(r"pub const ZK_OP_KECCAK:\s*c_int\s*=\s*16;", ffi)
    struct = re.search(r"#\[repr\(C\)\]\s*pub struct zk_keccak\s*\{([^}]*)\}", ffi)
    assert struct and re.findall(r"pub (\w+):", struct.group(1)) == FIELDS
    assert len(re.findall(r"\bfn\s+zk_\w*keccak\w*", ffi)) == len(re.findall(r"\bfn\s+zk_host_keccak256\b", ffi)), "no new function in the Rust declarations"
    for rel in ("README.md", "INTEGRATION.md", "DESIGN.md"):
        assert "ZK_OP_KECCAK" in open(os.path.join(ROOT, rel)).read(), rel
    for rel in (os.path.join("profiles", "README.md"), os.path.join("tools", "README.md")):
        text = open(os.path.join(ROOT, rel)).read()
        assert "keccak_time.py" in text and "r25_keccak.md" in text, rel
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for word in ("KeccakTable::assignments", "input_len", "output_rlc", "input_rlc", "zk_keccak desc", "keccak("):
        assert word in integration, word
    assert "profiles/r25_keccak.md" in open(os.path.join(ROOT, "DESIGN.md")).read()
    tool = open(os.path.join(ROOT, "tools", "keccak_time.py")).read()
    assert "keccak(" in tool and "host_keccak256" in tool and "median" in tool and "timeout" in tool
    profile = open(os.path.join(ROOT, "profiles", "r25_keccak.md")).read()
    assert "VGPR" in profile and "scratch" in profile.lower()
    makefile = open(os.path.join(ROOT, "zkevm-circuits_amd", "Makefile")).read()
    assert "csrc/keccak.hip" in makefile and "csrc/keccak64.hip.hpp" in makefile
    for name in ("keccak.hip", "keccak64.hip.hpp"):
        assert os.path.exists(os.path.join(ROOT, "zkevm-circuits_amd", "csrc", name)), name


def test_no_entry_point_was_added(zk):
    declared = sorted(set(re.findall(r"\b(zk_[a-z0-9_]+)\s*\(", _header_body(zk))))
    exported = _exported(zk)
    assert declared == exported, (sorted(set(declared) - set(exported)), sorted(set(exported) - set(declared)))
    assert len(exported) == 146
    assert [name for name in exported if "keccak" in name] == ["zk_host_keccak256"]
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "The C ABI has 146 entry points" in readme

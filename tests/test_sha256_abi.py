"""CPU: the SHA-256 table columns (ZK_OP_SHA256 = 18, zk_sha256) are an op of zk_field_vec_op -- in the header as a #define and a struct
OUTSIDE the op enum (whose five names and values stay), described in the ONE comment in front of the prototype behind the Keccak
text, in the Python binding (the constant, the ctypes struct with the C layout, Context.sha256), in the C++ mirror, the Rust
declarations, the documents, the timing tool and the profile -- and it came without a new entry point: the library still exports
exactly the 146 functions the header declares, none of them named after SHA-256."""
import ctypes
import inspect
import os
import re
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ["d_bytes", "total_bytes", "d_offsets", "d_lens", "d_digest", "d_input_rlc", "index_width", "flags"]
C_FIELDS = ["const void* d_bytes", "uint64_t total_bytes", "const void* d_offsets", "const void* d_lens", "void* d_digest", "void* d_input_rlc", "uint8_t index_width", "uint8_t flags"]


def _header_body(zk):
    return re.sub(r"/\*.*?\*/", "", open(zk.binding.HEADER_PATH).read(), flags=re.S)


def _exported(zk):
    """the zk_* functions in the library's dynamic symbol table"""
    nm = shutil.which("nm") or shutil.which("llvm-nm") or "/opt/rocm/llvm/bin/llvm-nm"
    out = subprocess.run([nm, "-D", "--defined-only", zk.binding.LIB_PATH], capture_output=True, text=True, check=True).stdout
    return sorted({ln.split()[-1] for ln in out.splitlines() if len(ln.split()) >= 3 and ln.split()[-2] in "TW" and ln.split()[-1].startswith("zk_")})


def _struct_fields(body, name):
    struct = re.search(rf"typedef\s+struct\s+{name}\s*\{{([^}}]*)\}}\s*{name}\s*;", body)
    assert struct, f"typedef struct {name}"
    return [re.sub(r"\s+", " ", f).strip() for f in struct.group(1).split(";") if f.strip()]


def test_header_defines_the_op_and_the_struct_outside_the_op_enum(zk):
    body = _header_body(zk)
    assert re.search(r"^#define\s+ZK_OP_SHA256\s+18\s*$", body, flags=re.M)
    assert _struct_fields(body, "zk_sha256") == C_FIELDS == _struct_fields(body, "zk_keccak")          # zk_keccak's members in name, type and order
    assert body.index("} zk_keccak;") < body.index("#define ZK_OP_SHA256") < body.index("typedef struct zk_sha256")
    enums = re.findall(r"\benum\s*\{([^}]*)\}", body)
    ops = [e for e in enums if "ZK_OP_ADD" in e]
    assert len(ops) == 1
    assert not any("SHA256" in e for e in enums if "ZK_OP_" in e)
    values = {name: int(v) for name, v in re.findall(r"\b(ZK_OP_[A-Z_0-9]+)\s*=\s*(\d+)", ops[0])}
    assert values == {"ZK_OP_ADD": 0, "ZK_OP_SUB": 1, "ZK_OP_MUL": 2, "ZK_OP_SCAN_AFFINE": 3, "ZK_OP_SCAN_AFFINE_REV": 4}
    for name, value in (("ZK_OP_ROW_RLC", 8), ("ZK_OP_SCAN_RLC", 9), ("ZK_OP_SCAN_RLC_REV", 10), ("ZK_OP_ROW_INV0", 12), ("ZK_OP_POSEIDON", 14), ("ZK_OP_KECCAK", 16)):
        assert re.search(rf"^#define\s+{name}\s+{value}\s*$", body, flags=re.M), name


def test_header_comment_describes_the_op(zk):
    text = open(zk.binding.HEADER_PATH).read()
    comment = text[:text.index("int zk_field_vec_op(")].rsplit("/*", 1)[1]
    assert comment.rstrip().endswith("*/") and comment.count("*/") == 1, "one comment, directly in front of the prototype"
    new = comment[comment.index("ZK_OP_SHA256"):]
    for word in ("ZK_OP_SHA256", "zk_sha256", "fr_sha256", "value 18 -- 17 stays refused", "HOST pointer", "r_out", "r_in", "d_digest", "d_input_rlc", "index_width",
                 "total_bytes", "input_len", "zk_proof_advice_phase_typed_dev", "validated before n is looked at", "cannot wrap", "reads nothing", "FIPS 180-4",
                 "SHA256Table", "output_rlc", "hashes_rlc", "keccak_input", "same challenge twice", "2^61", "H0's most significant byte first", "longest message"):
        assert word in new, word
    # what the comment said before stays, in its order, and the new text stands behind the Keccak text
    for word in ("ZK_OP_ROW_RLC", "fr_row_rlc", "ZK_OP_SCAN_RLC", "fr_scan_rlc", "ZK_OP_SCAN_AFFINE", "fr_scan_affine", "ZK_OP_ROW_INV0", "fr_row_inv0", "11 stays refused",
                 "ZK_OP_POSEIDON", "fr_poseidon", "13 stays refused", "ZK_OP_KECCAK", "fr_keccak", "15 stays refused"):
        assert word in comment, word
    assert comment.index("fr_row_inv0") < comment.index("ZK_OP_POSEIDON") < comment.index("fr_poseidon") < comment.index("ZK_OP_KECCAK") < comment.index("fr_keccak")
    assert comment.index("fr_keccak") < comment.index("ZK_OP_SHA256") < comment.index("fr_sha256")
    assert re.sub(r"\s*\*/\s*$", "", comment).rstrip().endswith("Other op values (5, 6, 7, 11, ...) are refused.")


def test_binding_exposes_the_constant_the_struct_and_the_method(zk):
    assert zk.OP_SHA256 == zk.binding.OP_SHA256 == 18
    assert zk.OP_KECCAK == 16 and zk.OP_POSEIDON == 14 and zk.OP_ROW_INV0 == 12 and zk.OP_ROW_RLC == 8 and (zk.OP_SCAN_RLC, zk.OP_SCAN_RLC_REV) == (9, 10)
    sig = inspect.signature(zk.binding.Context.sha256)
    assert list(sig.parameters) == ["self", "data", "total_bytes", "offsets", "lens", "index_width", "n", "out", "r_out", "r_in", "digest", "input_rlc"]
    assert list(sig.parameters) == list(inspect.signature(zk.binding.Context.keccak).parameters)
    defaults = {k: v.default for k, v in sig.parameters.items() if v.default is not inspect.Parameter.empty}
    assert defaults == {"r_in": None, "digest": None, "input_rlc": None}
    doc = zk.binding.Context.sha256.__doc__
    assert "ZK_OP_SHA256" in doc and "r_in = r_out" in doc
    desc = zk.binding._Sha256
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
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "zkmi355.h"\nint main(void) { printf("%zu", sizeof(zk_sha256));\n'
                   + "".join(f'printf(" %zu", offsetof(zk_sha256, {name}));\n' for name in FIELDS) + "return ZK_OP_SHA256 == 18 && sizeof(zk_sha256) == sizeof(zk_keccak) ? 0 : 1; }\n")
    exe = tmp_path / "layout"
    subprocess.run([cc, "-I", os.path.dirname(zk.binding.HEADER_PATH), str(src), "-o", str(exe)], check=True, timeout=120)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True, timeout=60).stdout.split()]
    desc = zk.binding._Sha256
    assert got == [ctypes.sizeof(desc)] + [getattr(desc, name).offset for name in FIELDS] == [56, 0, 8, 16, 24, 32, 40, 48, 49]


def test_mirror_rust_declarations_documents_tool_and_profile_name_the_op():
    mirror = open(os.path.join(ROOT, "include", "zkmi355_halo2.hpp")).read()
    assert re.search(r"\binline void sha256\(", mirror) and "ZK_OP_SHA256" in mirror and "zk_sha256" in mirror
    assert mirror.index("inline void poseidon(") < mirror.index("inline void keccak(") < mirror.index("inline void sha256(")
    ffi = open(os.path.join(ROOT, "shim", "halo2_proofs", "src", "zkmi355", "ffi.rs")).read()
    assert re.search(r"pub const ZK_OP_SHA256:\s*c_int\s*=\s*18;", ffi)
    struct = re.search(r"#\[repr\(C\)\]\s*pub struct zk_sha256\s*\{([^}]*)\}", ffi)
    assert struct and re.findall(r"pub (\w+):", struct.group(1)) == FIELDS
    assert not re.findall(r"\bfn\s+\w*sha256\w*", ffi), "no new function in the Rust declarations"
    for rel in ("README.md", "INTEGRATION.md", "DESIGN.md"):
        assert "ZK_OP_SHA256" in open(os.path.join(ROOT, rel)).read(), rel
    for rel in (os.path.join("profiles", "README.md"), os.path.join("tools", "README.md")):
        text = open(os.path.join(ROOT, rel)).read()
        assert "sha256_time.py" in text and "r26_sha256.md" in text, rel
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for word in ("SHA256Table::assignments", "dev_load", "all-zero", "input_len", "output_rlc", "input_rlc", "zk_sha256 desc", "sha256("):
        assert word in integration, word
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "profiles/r26_sha256.md" in design and design.index("ZK_OP_KECCAK") < design.index("ZK_OP_SHA256")
    tool = open(os.path.join(ROOT, "tools", "sha256_time.py")).read()
    assert "sha256(" in tool and "hashlib" in tool and "median" in tool and "timeout" in tool
    profile = open(os.path.join(ROOT, "profiles", "r26_sha256.md")).read()
    assert "VGPR" in profile and "scratch" in profile.lower() and "proof_sha256" in profile
    makefile = open(os.path.join(ROOT, "zkevm-circuits_amd", "Makefile")).read()
    assert "csrc/sha256.hip" in makefile.split("HDR :=")[0] and "csrc/sha256_32.hip.hpp" in makefile.split("HDR :=")[1]
    for name in ("sha256.hip", "sha256_32.hip.hpp"):
        assert os.path.exists(os.path.join(ROOT, "zkevm-circuits_amd", "csrc", name)), name
    unit = open(os.path.join(ROOT, "zkevm-circuits_amd", "csrc", "sha256_32.hip.hpp")).read()
    assert '#include "keccak64.hip.hpp"' in unit and "struct KckPow" not in unit and "kck_rlc8(const" not in unit, "the RLC code is reused, not copied"


def test_no_entry_point_was_added(zk):
    declared = sorted(set(re.findall(r"\b(zk_[a-z0-9_]+)\s*\(", _header_body(zk))))
    exported = _exported(zk)
    assert declared == exported, (sorted(set(declared) - set(exported)), sorted(set(exported) - set(declared)))
    assert len(exported) == 146
    assert [name for name in exported if "sha256" in name] == []
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "The C ABI has 146 entry points" in readme

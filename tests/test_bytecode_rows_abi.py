"""CPU: ZK_OP_BYTECODE_ROWS = 26 (zk_bytecode_rows) is an op of zk_field_vec_op -- in the header as a #define and a struct OUTSIDE the
op enum behind zk_key_order, with nothing defined at 23, 24, 25 or 27, described in the ONE comment in front of the prototype behind
the key-order text, in the Python binding (the constant, the ctypes struct with the C layout, Context.bytecode_rows), in the C++
mirror, the Rust declarations, the documents, the timing tool, the profile and the Makefile -- and it came without a new entry point:
the library still exports exactly the 146 functions the header declares, none named after the op."""
import ctypes
import inspect
import os
import re
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ["d_bytes", "total_bytes", "d_offsets", "d_lens", "d_hashes", "d_tag", "d_index", "d_value", "d_is_code", "d_push_data_left", "d_push_data_size", "d_length",
          "d_acc_kinds", "d_rlc_kinds", "count", "index_width", "flags"]
FIELDS_C = ["const void* d_bytes", "uint64_t total_bytes", "const void* d_offsets", "const void* d_lens", "const void* d_hashes", "void* d_tag", "void* d_index", "void* d_value",
            "void* d_is_code", "void* d_push_data_left", "void* d_push_data_size", "void* d_length", "void* d_acc_kinds", "void* d_rlc_kinds", "uint32_t count",
            "uint8_t index_width", "uint8_t flags"]
OFFSETS = [8 * i for i in range(14)] + [112, 116, 117]
SIZE = 120


def _header_body(zk):
    return re.sub(r"/\*.*?\*/", "", open(zk.binding.HEADER_PATH).read(), flags=re.S)


def _exported(zk):
    """the zk_* functions in the library's dynamic symbol table"""
    nm = shutil.which("nm") or shutil.which("llvm-nm") or "/opt/rocm/llvm/bin/llvm-nm"
    out = subprocess.run([nm, "-D", "--defined-only", zk.binding.LIB_PATH], capture_output=True, text=True, check=True).stdout
    return sorted({ln.split()[-1] for ln in out.splitlines() if len(ln.split()) >= 3 and ln.split()[-2] in "TW" and ln.split()[-1].startswith("zk_")})


def test_header_defines_the_op_and_the_struct_outside_the_op_enum(zk):
    body = _header_body(zk)
    assert re.search(r"^#define\s+ZK_OP_BYTECODE_ROWS\s+26\s*$", body, flags=re.M)
    assert not re.search(r"^#define\s+ZK_OP_\w+\s+(23|24|25|27)\s*$", body, flags=re.M)
    struct = re.search(r"typedef\s+struct\s+zk_bytecode_rows\s*\{([^}]*)\}\s*zk_bytecode_rows\s*;", body)
    assert struct and [re.sub(r"\s+", " ", f).strip() for f in struct.group(1).split(";") if f.strip()] == FIELDS_C
    assert body.index("} zk_key_order;") < body.index("#define ZK_OP_BYTECODE_ROWS") < body.index("typedef struct zk_bytecode_rows") < body.index("int zk_ctx_create(")
    enums = re.findall(r"\benum\s*\{([^}]*)\}", body)
    ops = [e for e in enums if "ZK_OP_ADD" in e]
    assert len(ops) == 1 and not any("BYTECODE" in e for e in enums)
    values = {name: int(v) for name, v in re.findall(r"\b(ZK_OP_[A-Z_0-9]+)\s*=\s*(\d+)", ops[0])}
    assert values == {"ZK_OP_ADD": 0, "ZK_OP_SUB": 1, "ZK_OP_MUL": 2, "ZK_OP_SCAN_AFFINE": 3, "ZK_OP_SCAN_AFFINE_REV": 4}
    for name, value in (("ZK_OP_ROW_RLC", 8), ("ZK_OP_SCAN_RLC", 9), ("ZK_OP_SCAN_RLC_REV", 10), ("ZK_OP_ROW_INV0", 12), ("ZK_OP_POSEIDON", 14), ("ZK_OP_KECCAK", 16), ("ZK_OP_SHA256", 18),
                        ("ZK_OP_KEY_SORT", 20), ("ZK_OP_KEY_ORDER", 22)):
        assert re.search(rf"^#define\s+{name}\s+{value}\s*$", body, flags=re.M), name


def test_header_comment_describes_the_op(zk):
    text = open(zk.binding.HEADER_PATH).read()
    comment = text[:text.index("int zk_field_vec_op(")].rsplit("/*", 1)[1]
    assert comment.rstrip().endswith("*/") and comment.count("*/") == 1, "one comment, directly in front of the prototype"
    new = comment[comment.index("ZK_OP_BYTECODE_ROWS"):]
    for word in ("value 26", "23, 24, 25 and 27 stay refused", "Fr only", "zk_bytecode_rows", "HOST pointer", "empty_hash", "POSEIDON_CODE_HASH_EMPTY", "EMPTY_CODE_HASH_LE",
                 "unroll_with_codehash", "assign_bytecode", "set_padding_row", "zk_keccak", "header row", "byte row", "padding rows", "push_data_left", "push_data_size", "is_code",
                 "d_acc_kinds", "d_rlc_kinds", "ZK_OP_SCAN_RLC", "ZK_OP_SCAN_RLC_REV", "push_acc", "push_rlc", "{0: (0, 0), 1: (r, 1)}", "{0: (0, 0), 1: (0, 1), 2: (1, 0)}",
                 "zk_proof_advice_phase_typed_dev", "Error::Synthesis", "cannot wrap", "empty bytecode", "saturates", "pure function", "walks a bytecode",
                 "never reads d_bytes", "validated before n is looked at", "n >= 2^32", "total_bytes >= 2^61", "\"bytecode_rows\"", "L mod 2^32"):
        assert word in new, word
    # what the comment said before stays, in its order, and the new text stands behind the key-order text
    for word in ("ZK_OP_ROW_RLC", "fr_row_rlc", "ZK_OP_SCAN_RLC", "fr_scan_rlc", "ZK_OP_ROW_INV0", "fr_row_inv0", "ZK_OP_POSEIDON", "fr_poseidon", "ZK_OP_KECCAK", "fr_keccak",
                 "ZK_OP_SHA256", "fr_sha256", "ZK_OP_KEY_SORT", "\"key_sort\"", "ZK_OP_KEY_ORDER", "\"key_order\"", "19 and 21 stay refused"):
        assert word in comment, word
    assert comment.index("\"key_sort\"") < comment.index("\"key_order\"") < comment.index("d_sorted may not be d_keys") < comment.index("ZK_OP_BYTECODE_ROWS") < comment.index("\"bytecode_rows\"")
    assert re.sub(r"\s*\*/\s*$", "", comment).rstrip().endswith("Other op values (5, 6, 7, 11, ...) are refused.")


def test_binding_exposes_the_constant_the_struct_and_the_method(zk):
    assert zk.OP_BYTECODE_ROWS == zk.binding.OP_BYTECODE_ROWS == 26 and zk.OP_KEY_ORDER == 22
    sig = inspect.signature(zk.binding.Context.bytecode_rows)
    assert list(sig.parameters) == ["self", "data", "total_bytes", "offsets", "lens", "index_width", "count", "n", "hash_out", "empty_hash", "hashes", "tag", "index", "value",
                                    "is_code", "push_data_left", "push_data_size", "length", "acc_kinds", "rlc_kinds"]
    defaults = {k: v.default for k, v in sig.parameters.items() if v.default is not inspect.Parameter.empty}
    assert defaults == {k: None for k in ("hashes", "tag", "index", "value", "is_code", "push_data_left", "push_data_size", "length", "acc_kinds", "rlc_kinds")}
    assert "ZK_OP_BYTECODE_ROWS" in zk.binding.Context.bytecode_rows.__doc__
    s = zk.binding._BytecodeRows
    assert issubclass(s, ctypes.Structure) and [name for name, _ in s._fields_] == FIELDS
    assert [getattr(s, name).offset for name in FIELDS] == OFFSETS and ctypes.sizeof(s) == SIZE
    types = dict(s._fields_)
    assert types["total_bytes"] is ctypes.c_uint64 and types["count"] is ctypes.c_uint32 and types["index_width"] is ctypes.c_uint8 and types["flags"] is ctypes.c_uint8
    assert all(types[name] is ctypes.c_void_p for name in FIELDS if name.startswith("d_"))


def test_the_struct_has_the_size_and_offsets_the_compiler_gives_it(zk, tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang") or "/opt/rocm/llvm/bin/clang"
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "zkmi355.h"\nint main(void) { printf("%zu", sizeof(zk_bytecode_rows));\n'
                   + "".join(f'printf(" %zu", offsetof(zk_bytecode_rows, {name}));\n' for name in FIELDS)
                   + "".join(f'printf(" %zu", sizeof(((zk_bytecode_rows*)0)->{name}));\n' for name in FIELDS)
                   + 'printf(" %zu", offsetof(zk_bytecode_rows, d_bytes) == offsetof(zk_keccak, d_bytes) && offsetof(zk_bytecode_rows, total_bytes) == offsetof(zk_keccak, total_bytes)'
                   ' && offsetof(zk_bytecode_rows, d_offsets) == offsetof(zk_keccak, d_offsets) && offsetof(zk_bytecode_rows, d_lens) == offsetof(zk_keccak, d_lens) ? (size_t)1 : (size_t)0);\n'
                   + 'return ZK_OP_BYTECODE_ROWS == 26 ? 0 : 1; }\n')
    exe = tmp_path / "layout"
    subprocess.run([cc, "-I", os.path.dirname(zk.binding.HEADER_PATH), str(src), "-o", str(exe)], check=True, timeout=120)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True, timeout=60).stdout.split()]
    s = zk.binding._BytecodeRows
    sizes = [8] * 14 + [4, 1, 1]
    assert got == [ctypes.sizeof(s)] + [getattr(s, name).offset for name in FIELDS] + [getattr(s, name).size for name in FIELDS] + [1] == [SIZE] + OFFSETS + sizes + [1]


def test_mirror_rust_declarations_documents_tool_profile_and_makefile_name_the_op():
    mirror = open(os.path.join(ROOT, "include", "zkmi355_halo2.hpp")).read()
    assert re.search(r"\binline void bytecode_rows\(", mirror) and "ZK_OP_BYTECODE_ROWS" in mirror and "zk_bytecode_rows" in mirror
    assert mirror.index("inline void key_sort(") < mirror.index("inline void key_order(") < mirror.index("inline void bytecode_rows(")
    ffi = open(os.path.join(ROOT, "shim", "halo2_proofs", "src", "zkmi355", "ffi.rs")).read()
    assert re.search(r"pub const ZK_OP_BYTECODE_ROWS:\s*c_int\s*=\s*26;", ffi)
    struct = re.search(r"#\[repr\(C\)\]\s*pub struct zk_bytecode_rows\s*\{([^}]*)\}", ffi)
    assert struct and re.findall(r"pub (\w+):", struct.group(1)) == FIELDS
    assert not re.findall(r"\bfn\s+\w*bytecode_rows\w*", ffi), "no new function in the Rust declarations"
    for rel in ("README.md", "INTEGRATION.md", "DESIGN.md"):
        assert "ZK_OP_BYTECODE_ROWS" in open(os.path.join(ROOT, rel)).read(), rel
    for rel in (os.path.join("profiles", "README.md"), os.path.join("tools", "README.md")):
        text = open(os.path.join(ROOT, rel)).read()
        assert "bytecode_rows_time.py" in text and "r30_bytecode_rows.md" in text, rel
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for word in ("zk_bytecode_rows desc", "bytecode_rows(", "value_rlc", "push_acc", "push_rlc", "push_data_left_inv", "index_length_diff_inv", "ZK_OP_SCAN_RLC_REV", "ZK_OP_ROW_INV0",
                 "empty_hash", "phase 2", "d_acc_kinds", "d_rlc_kinds", "zk_proof_advice_phase_typed_dev"):
        assert word in integration, word
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "profiles/r30_bytecode_rows.md" in design and design.index("ZK_OP_KEY_SORT") < design.index("ZK_OP_BYTECODE_ROWS")
    tool = open(os.path.join(ROOT, "tools", "bytecode_rows_time.py")).read()
    assert "bytecode_rows(" in tool and "median" in tool and "timeout" in tool and "rows_numpy" in tool
    profile = open(os.path.join(ROOT, "profiles", "r30_bytecode_rows.md")).read()
    assert "VGPR" in profile and "scratch" in profile.lower() and "LDS" in profile and "k_bc_rows" in profile
    makefile = open(os.path.join(ROOT, "zkevm-circuits_amd", "Makefile")).read()
    assert "csrc/bytecode_rows.hip" in makefile.split("HDR :=")[0] and "csrc/bytecode_rows.hip.hpp" in makefile.split("HDR :=")[1]
    unit = open(os.path.join(ROOT, "zkevm-circuits_amd", "csrc", "bytecode_rows.hip.hpp")).read()
    assert "threadIdx" not in unit and "__shared__" not in unit and "__global__" not in unit, "the header is lane-free: the host compiles it"
    assert os.path.exists(os.path.join(ROOT, "zkevm-circuits_amd", "csrc", "bytecode_rows.hip"))


def test_no_entry_point_was_added(zk):
    declared = sorted(set(re.findall(r"\b(zk_[a-z0-9_]+)\s*\(", _header_body(zk))))
    exported = _exported(zk)
    assert declared == exported, (sorted(set(declared) - set(exported)), sorted(set(exported) - set(declared)))
    assert len(exported) == 146
    assert [name for name in exported if "bytecode" in name] == []
    assert "The C ABI has 146 entry points" in open(os.path.join(ROOT, "README.md")).read()

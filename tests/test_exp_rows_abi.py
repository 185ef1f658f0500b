"""CPU: ZK_OP_EXP_ROWS = 32 (zk_exp_rows, zk_exp_event) is an op of zk_field_vec_op -- in the header as a #define and structs OUTSIDE
the op enum behind zk_copy_rlc, with nothing defined at 31, described in the ONE comment in front of the prototype behind the copy-rows
text, in the Python binding (the constant, the ctypes structs with the C layout, Context.exp_rows), in the C++ mirror, the Rust
declarations, the documents, the timing tool, the profile and the Makefile -- and it came without a new entry point: the library still
exports exactly the 146 functions the header declares."""
import ctypes
import inspect
import os
import re
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = ["d_is_last", "d_base_limb", "d_exponent_lo_hi", "d_mul_cols", "d_mul_u16_64", "d_mul_u16_128", "d_parity_cols", "d_parity_u16_64", "d_parity_u16_128", "d_rows_needed"]
FIELDS = ["d_events", "count", "flags"] + OUT
FIELDS_C = ["const void* d_events", "uint32_t count", "uint8_t flags"] + ["void* " + f for f in OUT]
OFFSETS, SIZES, SIZE = [0, 8, 12] + [16 + 8 * i for i in range(10)], [8, 4, 1] + [8] * 10, 96
EVENT_FIELDS, EVENT_OFFSETS, EVENT_SIZES, EVENT_SIZE = ["base", "exponent"], [0, 32], [32, 32], 64


def _header_body(zk):
    return re.sub(r"/\*.*?\*/", "", open(zk.binding.HEADER_PATH).read(), flags=re.S)


def _exported(zk):
    """the zk_* functions in the library's dynamic symbol table"""
    nm = shutil.which("nm") or shutil.which("llvm-nm") or "/opt/rocm/llvm/bin/llvm-nm"
    out = subprocess.run([nm, "-D", "--defined-only", zk.binding.LIB_PATH], capture_output=True, text=True, check=True).stdout
    return sorted({ln.split()[-1] for ln in out.splitlines() if len(ln.split()) >= 3 and ln.split()[-2] in "TW" and ln.split()[-1].startswith("zk_")})


def _struct_fields(body, name):
    struct = re.search(rf"typedef\s+struct\s+{name}\s*\{{([^}}]*)\}}\s*{name}\s*;", body)
    assert struct, name
    return [re.sub(r"\s+", " ", f).strip() for f in struct.group(1).split(";") if f.strip()]


def test_header_defines_the_op_and_the_structs_outside_the_op_enum(zk):
    body = _header_body(zk)
    assert re.search(r"^#define\s+ZK_OP_EXP_ROWS\s+32\s*$", body, flags=re.M)
    assert not re.search(r"^#define\s+ZK_OP_\w+\s+31\s*$", body, flags=re.M)
    assert _struct_fields(body, "zk_exp_rows") == FIELDS_C
    assert _struct_fields(body, "zk_exp_event") == ["uint64_t base[4]", "uint64_t exponent[4]"]
    assert body.index("} zk_copy_rlc;") < body.index("#define ZK_OP_EXP_ROWS") < body.index("typedef struct zk_exp_event") < body.index("typedef struct zk_exp_rows") \
        < body.index("int zk_ctx_create(")
    enums = re.findall(r"\benum\s*\{([^}]*)\}", body)
    ops = [e for e in enums if "ZK_OP_ADD" in e]
    assert len(ops) == 1 and not any("EXP" in e for e in enums)
    values = {name: int(v) for name, v in re.findall(r"\b(ZK_OP_[A-Z_0-9]+)\s*=\s*(\d+)", ops[0])}
    assert values == {"ZK_OP_ADD": 0, "ZK_OP_SUB": 1, "ZK_OP_MUL": 2, "ZK_OP_SCAN_AFFINE": 3, "ZK_OP_SCAN_AFFINE_REV": 4}
    for name, value in (("ZK_OP_BYTECODE_ROWS", 26), ("ZK_OP_COPY_ROWS", 28), ("ZK_OP_COPY_RLC", 30)):
        assert re.search(rf"^#define\s+{name}\s+{value}\s*$", body, flags=re.M), name


def test_header_comment_describes_the_op(zk):
    text = open(zk.binding.HEADER_PATH).read()
    comment = text[:text.index("int zk_field_vec_op(")].rsplit("/*", 1)[1]
    assert comment.rstrip().endswith("*/") and comment.count("*/") == 1, "one comment, directly in front of the prototype"
    new = comment[comment.index("ZK_OP_EXP_ROWS"):]
    for word in ("value 32", "31 stays refused", "Fr only", "zk_exp_rows", "zk_exp_event", "HOST pointer", "assign_exp_events", "ExpTable::assignments", "MulAddChip::assign",
                 "UIntRangeCheckChip::assign", "zk_proof_advice_phase_typed_dev", "64 little-endian bytes", "d_b must be NULL", "bitlen(x) - 1", "popcount(x) - 1", "510", "mod 2^256",
                 "P(i) = i + popcount(x mod 2^i)", "d_is_last", "d_base_limb", "d_exponent_lo_hi", "d_mul_cols", "d_parity_cols", "carry_lo", "carry_hi", "u16_repr", "[2, x_j >> 1, x_j & 1, x_j]",
                 "base 2, exponent 2", "n - 10", "max_exp_rows", "whole steps only", "d_rows_needed", "unsaturated", "saturates", "q_enable", "is_final_step", "in range by construction",
                 "pure function", "walks an event", "No atomics", "validated before n is looked at", "n >= 2^32", "\"exp_rows\""):
        assert word in new, word
    assert comment.index("\"copy_rlc\"") < comment.index("ZK_OP_EXP_ROWS") < comment.index("\"exp_rows\"")
    assert re.sub(r"\s*\*/\s*$", "", comment).rstrip().endswith("Other op values (5, 6, 7, 11, ...) are refused.")


def test_binding_exposes_the_constant_the_structs_and_the_method(zk):
    b = zk.binding
    assert zk.OP_EXP_ROWS == b.OP_EXP_ROWS == 32 and zk.OP_COPY_RLC == 30
    sig = inspect.signature(b.Context.exp_rows)
    assert list(sig.parameters) == ["self", "events", "count", "n", "exponentiation_lo_hi", "outputs"] and sig.parameters["outputs"].kind is inspect.Parameter.VAR_KEYWORD
    assert ["d_" + name for name in b.EXP_ROWS_OUTPUTS] == OUT
    assert "ZK_OP_EXP_ROWS" in b.Context.exp_rows.__doc__
    for s, fields, offsets, size in ((b._ExpRows, FIELDS, OFFSETS, SIZE), (b._ExpEvent, EVENT_FIELDS, EVENT_OFFSETS, EVENT_SIZE)):
        assert issubclass(s, ctypes.Structure) and [name for name, _ in s._fields_] == fields
        assert [getattr(s, name).offset for name in fields] == offsets and ctypes.sizeof(s) == size
    types = dict(b._ExpRows._fields_)
    assert types["count"] is ctypes.c_uint32 and types["flags"] is ctypes.c_uint8 and all(types[name] is ctypes.c_void_p for name in types if name.startswith("d_"))


def test_the_structs_have_the_sizes_and_offsets_the_compiler_gives_them(zk, tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang") or "/opt/rocm/llvm/bin/clang"
    src = tmp_path / "layout.c"
    body = '#include <stdio.h>\n#include <stddef.h>\n#include "zkmi355.h"\nint main(void) {\n'
    for struct, fields in (("zk_exp_rows", FIELDS), ("zk_exp_event", EVENT_FIELDS)):
        body += f'printf(" %zu", sizeof({struct}));\n' + "".join(f'printf(" %zu", offsetof({struct}, {name}));\n' for name in fields)
        body += "".join(f'printf(" %zu", sizeof((({struct}*)0)->{name}));\n' for name in fields)
    body += 'return ZK_OP_EXP_ROWS == 32 ? 0 : 1; }\n'
    src.write_text(body)
    exe = tmp_path / "layout"
    subprocess.run([cc, "-I", os.path.dirname(zk.binding.HEADER_PATH), str(src), "-o", str(exe)], check=True, timeout=120)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True, timeout=60).stdout.split()]
    assert got == [SIZE] + OFFSETS + SIZES + [EVENT_SIZE] + EVENT_OFFSETS + EVENT_SIZES


def test_mirror_rust_declarations_documents_tool_profile_and_makefile_name_the_op():
    mirror = open(os.path.join(ROOT, "include", "zkmi355_halo2.hpp")).read()
    assert re.search(r"\binline void exp_rows\(", mirror) and "ZK_OP_EXP_ROWS" in mirror and "zk_exp_rows" in mirror
    assert mirror.index("inline void copy_rows(") < mirror.index("inline void copy_rlc(") < mirror.index("inline void exp_rows(")
    ffi = open(os.path.join(ROOT, "shim", "halo2_proofs", "src", "zkmi355", "ffi.rs")).read()
    assert re.search(r"pub const ZK_OP_EXP_ROWS:\s*c_int\s*=\s*32;", ffi)
    for name, fields in (("zk_exp_rows", FIELDS), ("zk_exp_event", EVENT_FIELDS)):
        struct = re.search(rf"#\[repr\(C\)\]\s*pub struct {name}\s*\{{([^}}]*)\}}", ffi)
        assert struct and re.findall(r"pub (\w+):", struct.group(1)) == fields, name
    assert not re.findall(r"\bfn\s+\w*exp_r\w*", ffi), "no new function in the Rust declarations"
    for rel in ("README.md", "INTEGRATION.md", "DESIGN.md"):
        assert "ZK_OP_EXP_ROWS" in open(os.path.join(ROOT, rel)).read(), rel
    for rel in (os.path.join("profiles", "README.md"), os.path.join("tools", "README.md")):
        text = open(os.path.join(ROOT, rel)).read()
        assert "exp_rows_time.py" in text and "r32_exp_rows.md" in text, rel
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for word in ("zk_exp_rows desc", "exp_rows(", "zk_exp_event", "zk_proof_advice_phase_typed_dev", "d_rows_needed", "q_enable", "is_step", "is_final_step", "36"):
        assert word in integration, word
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "profiles/r32_exp_rows.md" in design and design.index("ZK_OP_COPY_ROWS") < design.index("ZK_OP_EXP_ROWS")
    tool = open(os.path.join(ROOT, "tools", "exp_rows_time.py")).read()
    assert "exp_rows(" in tool and "median" in tool and "timeout" in tool and "closed" in tool
    profile = open(os.path.join(ROOT, "profiles", "r32_exp_rows.md")).read()
    assert "VGPR" in profile and "scratch" in profile.lower() and "LDS" in profile and "k_exp_rows" in profile and "k_exp_chain" in profile
    makefile = open(os.path.join(ROOT, "zkevm-circuits_amd", "Makefile")).read()
    assert "csrc/exp_rows.hip" in makefile.split("HDR :=")[0] and "csrc/exp_rows.hip.hpp" in makefile.split("HDR :=")[1]
    unit = open(os.path.join(ROOT, "zkevm-circuits_amd", "csrc", "exp_rows.hip.hpp")).read()
    assert "threadIdx" not in unit and "blockIdx" not in unit and "__shared__" not in unit and "__global__" not in unit, "the header is lane-free: the host compiles it"
    source = open(os.path.join(ROOT, "zkevm-circuits_amd", "csrc", "exp_rows.hip")).read()
    assert "SC_EXP" in source and "k_exp_widths" in source and "k_exp_chain" in source and "k_exp_rows" in source and "atomic" not in source.replace("No atomics", "")
    vec = open(os.path.join(ROOT, "zkevm-circuits_amd", "csrc", "vec.hip")).read()
    assert vec.count("{ZK_OP_EXP_ROWS,") == 1


def test_no_entry_point_was_added(zk):
    declared = sorted(set(re.findall(r"\b(zk_[a-z0-9_]+)\s*\(", _header_body(zk))))
    exported = _exported(zk)
    assert declared == exported, (sorted(set(declared) - set(exported)), sorted(set(exported) - set(declared)))
    assert len(exported) == 146
    assert [name for name in exported if "exp_r" in name] == []
    assert "The C ABI has 146 entry points" in open(os.path.join(ROOT, "README.md")).read()

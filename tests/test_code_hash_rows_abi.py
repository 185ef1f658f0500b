"""ZK_OP_CODE_HASH_ROWS = 34 (zk_code_hash_rows) and ZK_OP_CODE_HASH_TABLE = 36 (zk_code_hash_table) are ops of zk_field_vec_op -- in
the header as #defines and structs OUTSIDE the op enum behind zk_exp_rows, with nothing defined at 33 or 35, described in the ONE
comment in front of the prototype behind the exponentiation text, in the Python binding (the constants, the ctypes structs with the C
layout, Context.code_hash_rows and Context.code_hash_table), in the C++ mirror, the Rust declarations, the documents, the timing tool,
the profile and the Makefile -- and they came without a new entry point: the library still exports exactly the 146 functions the
header declares.  The refusals and n = 0 need a context and are marked gpu; the two GPU test files hold the full lists."""
import ctypes
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHARED = ["d_bytes", "total_bytes", "d_offsets", "d_lens"]
TAIL = ["count", "index_width", "flags"]
ROWS = SHARED + ["d_control_length", "d_bytes_in_field_index", "d_bytes_in_field_inv", "d_is_field_border", "d_padding_shift", "d_field_index", "d_field_index_inv"] + TAIL
TABLE = SHARED + ["d_input1", "d_control", "d_heading_mark", "d_kinds", "d_cap", "d_rows_needed"] + TAIL
LAYOUT = {"zk_code_hash_rows": (ROWS, [8 * i for i in range(11)] + [88, 92, 93], 96), "zk_code_hash_table": (TABLE, [8 * i for i in range(10)] + [80, 84, 85], 88)}


def _header_body(zk):
    return re.sub(r"/\*.*?\*/", "", open(zk.binding.HEADER_PATH).read(), flags=re.S)


def test_header_defines_the_ops_and_the_structs_outside_the_op_enum(zk):
    body = _header_body(zk)
    assert re.search(r"^#define\s+ZK_OP_CODE_HASH_ROWS\s+34\s*$", body, flags=re.M) and re.search(r"^#define\s+ZK_OP_CODE_HASH_TABLE\s+36\s*$", body, flags=re.M)
    assert not re.search(r"^#define\s+ZK_OP_\w+\s+(33|35)\s*$", body, flags=re.M)
    for name, (fields, _, _) in LAYOUT.items():
        struct = re.search(rf"typedef\s+struct\s+{name}\s*\{{([^}}]*)\}}\s*{name}\s*;", body)
        assert struct and [re.sub(r"\s+", " ", f).strip().split(" ")[-1] for f in struct.group(1).split(";") if f.strip()] == fields, name
    assert body.index("} zk_exp_rows;") < body.index("#define ZK_OP_CODE_HASH_ROWS") < body.index("typedef struct zk_code_hash_rows") < body.index("typedef struct zk_code_hash_table") < body.index("int zk_ctx_create(")
    assert not any("CODE_HASH" in e for e in re.findall(r"\benum\s*\{([^}]*)\}", body))


def test_header_comment_describes_the_ops(zk):
    text = open(zk.binding.HEADER_PATH).read()
    comment = text[:text.index("int zk_field_vec_op(")].rsplit("/*", 1)[1]
    assert comment.rstrip().endswith("*/") and comment.count("*/") == 1, "one comment, directly in front of the prototype"
    new = comment[comment.index("ZK_OP_CODE_HASH_ROWS"):]
    for word in ("values 34 and 36", "33 and 35 stay refused", "Fr only", "zk_code_hash_rows", "zk_code_hash_table", "HOST pointer", "d_b must be NULL", "to_poseidon_hash.rs",
                 "assign_extended_row", "set_header_row", "PoseidonTable::dev_load", "unroll_to_hash_input_default", "zk_keccak", "zk_bytecode_rows", "empty bytecode", "header row",
                 "byte row", "padding rows", "control_length", "field_input", "bytes_in_field_index", "bytes_in_field_inv", "is_field_border", "padding_shift", "256^31", "field_index_inv",
                 "zk_proof_advice_phase_typed_dev", "ceil(L_b / 62)", "d_input1", "d_control", "HASHABLE_DOMAIN_SPEC", "d_heading_mark", "d_kinds", "d_cap", "d_rows_needed", "unsaturated",
                 "ZK_OP_POSEIDON", "width0 = width1 = 32", "cap_width = 8", "cap_scale = 2^64", "ZK_POSEIDON_FINAL", "domain_spec", "saturates", "pure function", "walks a bytecode",
                 "validated before n is looked at", "n >= 2^32", "total_bytes >= 2^61", "\"code_hash_rows\"", "\"code_hash_table\"", "L mod 2^32"):
        assert word in new, word
    assert comment.index("\"exp_rows_tiles\"") < comment.index("ZK_OP_CODE_HASH_ROWS") < comment.index("\"code_hash_table\"")
    assert re.sub(r"\s*\*/\s*$", "", comment).rstrip().endswith("Other op values (5, 6, 7, 11, ...) are refused.")


def test_binding_exposes_the_constants_the_structs_and_the_methods(zk):
    assert zk.OP_CODE_HASH_ROWS == zk.binding.OP_CODE_HASH_ROWS == 34 and zk.OP_CODE_HASH_TABLE == zk.binding.OP_CODE_HASH_TABLE == 36
    for method, out, op in ((zk.binding.Context.code_hash_rows, "field_input", "ZK_OP_CODE_HASH_ROWS"), (zk.binding.Context.code_hash_table, "input0", "ZK_OP_CODE_HASH_TABLE")):
        assert list(inspect.signature(method).parameters) == ["self", "data", "total_bytes", "offsets", "lens", "index_width", "count", "n", out, "outputs"]
        assert op in method.__doc__
    assert ["d_" + name for name in zk.binding.CODE_HASH_ROWS_OUTPUTS] == ROWS[4:-3] and ["d_" + name for name in zk.binding.CODE_HASH_TABLE_OUTPUTS] == TABLE[4:-3]
    for s, (fields, offsets, size) in ((zk.binding._CodeHashRows, LAYOUT["zk_code_hash_rows"]), (zk.binding._CodeHashTable, LAYOUT["zk_code_hash_table"])):
        assert issubclass(s, ctypes.Structure) and [name for name, _ in s._fields_] == fields
        assert [getattr(s, name).offset for name in fields] == offsets and ctypes.sizeof(s) == size
        types = dict(s._fields_)
        assert types["total_bytes"] is ctypes.c_uint64 and types["count"] is ctypes.c_uint32 and types["index_width"] is ctypes.c_uint8 and types["flags"] is ctypes.c_uint8
        assert all(types[name] is ctypes.c_void_p for name in fields if name.startswith("d_"))


def test_the_structs_have_the_sizes_and_offsets_the_compiler_gives_them(zk, tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang") or "/opt/rocm/llvm/bin/clang"
    body = '#include <stdio.h>\n#include <stddef.h>\n#include "zkmi355.h"\nint main(void) {\n'
    for name, (fields, _, _) in LAYOUT.items():
        body += f'printf("%zu", sizeof({name}));\n' + "".join(f'printf(" %zu", offsetof({name}, {f}));\n' for f in fields)
        body += "".join(f'printf(" %d", offsetof({name}, {f}) == offsetof(zk_keccak, {f}) && offsetof({name}, {f}) == offsetof(zk_bytecode_rows, {f}));\n' for f in SHARED) + 'printf("\\n");\n'
    body += "return ZK_OP_CODE_HASH_ROWS == 34 && ZK_OP_CODE_HASH_TABLE == 36 ? 0 : 1; }\n"
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text(body)
    subprocess.run([cc, "-I", os.path.dirname(zk.binding.HEADER_PATH), str(src), "-o", str(exe)], check=True, timeout=120)
    lines = subprocess.run([str(exe)], capture_output=True, text=True, check=True, timeout=60).stdout.splitlines()
    for line, (name, (fields, offsets, size)) in zip(lines, LAYOUT.items()):
        assert [int(x) for x in line.split()] == [size] + offsets + [1, 1, 1, 1], name


def test_mirror_rust_declarations_documents_tool_profile_and_makefile_name_the_ops():
    mirror = open(os.path.join(ROOT, "include", "zkmi355_halo2.hpp")).read()
    assert re.search(r"\binline void code_hash_rows\(", mirror) and re.search(r"\binline void code_hash_table\(", mirror)
    assert "ZK_OP_CODE_HASH_ROWS" in mirror and "ZK_OP_CODE_HASH_TABLE" in mirror and mirror.index("inline void exp_rows(") < mirror.index("inline void code_hash_rows(")
    ffi = open(os.path.join(ROOT, "shim", "halo2_proofs", "src", "zkmi355", "ffi.rs")).read()
    assert re.search(r"pub const ZK_OP_CODE_HASH_ROWS:\s*c_int\s*=\s*34;", ffi) and re.search(r"pub const ZK_OP_CODE_HASH_TABLE:\s*c_int\s*=\s*36;", ffi)
    for name, (fields, _, _) in LAYOUT.items():
        struct = re.search(rf"#\[repr\(C\)\]\s*pub struct {name}\s*\{{([^}}]*)\}}", ffi)
        assert struct and re.findall(r"pub (\w+):", struct.group(1)) == fields, name
    assert not re.findall(r"\bfn\s+\w*code_hash\w*", ffi), "no new function in the Rust declarations"
    for rel in ("README.md", "INTEGRATION.md", "DESIGN.md"):
        text = open(os.path.join(ROOT, rel)).read()
        assert "ZK_OP_CODE_HASH_ROWS" in text and "ZK_OP_CODE_HASH_TABLE" in text, rel
    for rel in (os.path.join("profiles", "README.md"), os.path.join("tools", "README.md")):
        text = open(os.path.join(ROOT, rel)).read()
        assert "code_hash_rows_time.py" in text and "r33_code_hash_rows.md" in text, rel
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for word in ("zk_code_hash_rows", "zk_code_hash_table", "code_hash_rows(", "code_hash_table(", "hash_id", "d_rows_needed", "ZK_POSEIDON_FINAL", "zk_proof_advice_phase_typed_dev"):
        assert word in integration, word
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "profiles/r33_code_hash_rows.md" in design and "SC_CODE_HASH" in design and design.index("ZK_OP_EXP_ROWS") < design.index("ZK_OP_CODE_HASH_ROWS")
    tool = open(os.path.join(ROOT, "tools", "code_hash_rows_time.py")).read()
    assert "code_hash_rows(" in tool and "code_hash_table(" in tool and "bytecode_rows(" in tool and "median" in tool and "timeout" in tool and "rows_numpy" in tool
    profile = open(os.path.join(ROOT, "profiles", "r33_code_hash_rows.md")).read()
    assert "VGPR" in profile and "scratch" in profile.lower() and "LDS" in profile and "k_ch_rows" in profile and "k_ch_table" in profile
    makefile = open(os.path.join(ROOT, "zkevm-circuits_amd", "Makefile")).read()
    assert "csrc/code_hash_rows.hip" in makefile.split("HDR :=")[0] and "csrc/code_hash_rows.hip.hpp" in makefile.split("HDR :=")[1]
    unit = open(os.path.join(ROOT, "zkevm-circuits_amd", "csrc", "code_hash_rows.hip.hpp")).read()
    assert "threadIdx" not in unit and "__shared__" not in unit and "__global__" not in unit, "the header is lane-free: the host compiles it"
    assert "static_assert" in unit


def test_no_entry_point_was_added(zk):
    nm = shutil.which("nm") or shutil.which("llvm-nm") or "/opt/rocm/llvm/bin/llvm-nm"
    out = subprocess.run([nm, "-D", "--defined-only", zk.binding.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = sorted({ln.split()[-1] for ln in out.splitlines() if len(ln.split()) >= 3 and ln.split()[-2] in "TW" and ln.split()[-1].startswith("zk_")})
    declared = sorted(set(re.findall(r"\b(zk_[a-z0-9_]+)\s*\(", _header_body(zk))))
    assert declared == exported and len(exported) == 146 and [name for name in exported if "code_hash" in name] == []


@pytest.mark.gpu
def test_refusals_and_no_rows_through_the_abi(zk, ctx):
    """Fq, flags, a second operand and a bad index_width are refused by both ops before n is looked at; n = 0 is then ZK_OK"""
    src = ctx.to_device(np.arange(64, dtype=np.uint8))
    idx = ctx.to_device(np.array([0, 40], dtype=np.uint32))
    out = ctx.to_device(np.full(64, 0xC3, dtype=np.uint8))
    some = np.zeros(4, dtype=np.uint64)
    try:
        for op, struct in ((34, zk.binding._CodeHashRows), (36, zk.binding._CodeHashTable)):
            def call(field=0, d_b=None, n=2, **change):
                f = {name: None for name, _ in struct._fields_}
                f.update(d_bytes=src.ptr, total_bytes=64, d_offsets=idx.ptr, d_lens=idx.ptr + 4, count=1, index_width=4, flags=0)
                f.update(change)
                rc = zk.lib().zk_field_vec_op(ctx.h, field, op, ctypes.byref(struct(*[f[name] for name, _ in struct._fields_])), d_b, ctypes.c_void_p(out.ptr), ctypes.c_size_t(n))
                ctx.sync()
                return rc
            for n in (2, 0):
                assert call(field=1, n=n) == -1 and call(flags=1, n=n) == -1 and call(index_width=2, n=n) == -1 and call(d_b=some.ctypes.data_as(ctypes.c_void_p), n=n) == -1
            assert call(n=0) == 0
            assert (out.download(64, np.uint8) == 0xC3).all(), "nothing was written"
            assert call(n=2) == 0
            assert not (out.download(64, np.uint8) == 0xC3).all()
            out.upload(np.full(64, 0xC3, dtype=np.uint8))
    finally:
        for b in (src, idx, out):
            b.free()

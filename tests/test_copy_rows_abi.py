"""CPU: ZK_OP_COPY_ROWS = 28 (zk_copy_rows) and ZK_OP_COPY_RLC = 30 (zk_copy_rlc) are ops of zk_field_vec_op -- in the header as
#defines and structs OUTSIDE the op enum behind zk_bytecode_rows, with nothing defined at 27 or 29, described in the ONE comment in
front of the prototype behind the bytecode-rows text, in the Python binding (the constants, the ctypes structs with the C layout,
Context.copy_rows and Context.copy_rlc), in the C++ mirror, the Rust declarations, the documents, the timing tool, the profile and the
Makefile -- and they came without a new entry point: the library still exports exactly the 146 functions the header declares."""
import ctypes
import inspect
import os
import re
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHARED = ["d_events", "count", "d_bytes", "total_bytes", "flags"]
SHARED_C = ["const void* d_events", "uint32_t count", "const void* d_bytes", "uint64_t total_bytes", "uint8_t flags"]
ROWS_OUT = ["d_is_first", "d_is_last", "d_tag", "d_tag_bits", "d_value", "d_value_prev", "d_mask", "d_front_mask", "d_word_index", "d_src_addr_end", "d_is_pad",
            "d_non_pad_non_mask", "d_real_bytes_left", "d_rw_counter", "d_rwc_inc_left", "d_types", "d_src_end_rows"]
RLC_OUT = ["d_id", "d_id_other", "d_rlc_acc", "d_word_rlc", "d_word_rlc_prev"]
ROWS_FIELDS, RLC_FIELDS = SHARED + ROWS_OUT, SHARED + ["d_ids"] + RLC_OUT
ROWS_C = SHARED_C + ["void* " + f for f in ROWS_OUT]
RLC_C = SHARED_C + ["const void* d_ids"] + ["void* " + f for f in RLC_OUT]
SHARED_OFFSETS, SHARED_SIZES = [0, 8, 16, 24, 32], [8, 4, 8, 8, 1]
ROWS_OFFSETS, ROWS_SIZE = SHARED_OFFSETS + [40 + 8 * i for i in range(17)], 176
RLC_OFFSETS, RLC_SIZE = SHARED_OFFSETS + [40 + 8 * i for i in range(6)], 88
EVENT_FIELDS = ["src_addr", "src_addr_end", "dst_addr", "dst_addr_bias", "rw_counter", "src_off", "dst_off", "prev_off", "length", "src_front", "src_back", "dst_front", "dst_back",
                "src_tag", "dst_tag", "flags", "reserved"]
EVENT_OFFSETS, EVENT_SIZES, EVENT_SIZE = [8 * i for i in range(8)] + [64, 68, 72, 76, 80, 84, 85, 86, 87], [8] * 8 + [4] * 5 + [1] * 4, 88


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


def test_header_defines_the_ops_and_the_structs_outside_the_op_enum(zk):
    body = _header_body(zk)
    assert re.search(r"^#define\s+ZK_OP_COPY_ROWS\s+28\s*$", body, flags=re.M) and re.search(r"^#define\s+ZK_OP_COPY_RLC\s+30\s*$", body, flags=re.M)
    assert re.search(r"^#define\s+ZK_COPY_MEMORY_COPY\s+1\s*$", body, flags=re.M)
    assert not re.search(r"^#define\s+ZK_OP_\w+\s+(27|29)\s*$", body, flags=re.M)
    assert _struct_fields(body, "zk_copy_rows") == ROWS_C and _struct_fields(body, "zk_copy_rlc") == RLC_C
    assert _struct_fields(body, "zk_copy_event") == ["uint64_t src_addr, src_addr_end, dst_addr", "uint64_t dst_addr_bias", "uint64_t rw_counter", "uint64_t src_off, dst_off, prev_off",
                                                     "uint32_t length", "uint32_t src_front, src_back, dst_front, dst_back", "uint8_t src_tag, dst_tag", "uint8_t flags", "uint8_t reserved"]
    assert body.index("} zk_bytecode_rows;") < body.index("#define ZK_OP_COPY_ROWS") < body.index("typedef struct zk_copy_event") < body.index("typedef struct zk_copy_rows") \
        < body.index("typedef struct zk_copy_rlc") < body.index("int zk_ctx_create(")
    enums = re.findall(r"\benum\s*\{([^}]*)\}", body)
    ops = [e for e in enums if "ZK_OP_ADD" in e]
    assert len(ops) == 1 and not any("COPY" in e for e in enums)
    values = {name: int(v) for name, v in re.findall(r"\b(ZK_OP_[A-Z_0-9]+)\s*=\s*(\d+)", ops[0])}
    assert values == {"ZK_OP_ADD": 0, "ZK_OP_SUB": 1, "ZK_OP_MUL": 2, "ZK_OP_SCAN_AFFINE": 3, "ZK_OP_SCAN_AFFINE_REV": 4}
    for name, value in (("ZK_OP_ROW_RLC", 8), ("ZK_OP_SCAN_RLC", 9), ("ZK_OP_SCAN_RLC_REV", 10), ("ZK_OP_ROW_INV0", 12), ("ZK_OP_POSEIDON", 14), ("ZK_OP_KECCAK", 16), ("ZK_OP_SHA256", 18),
                        ("ZK_OP_KEY_SORT", 20), ("ZK_OP_KEY_ORDER", 22), ("ZK_OP_BYTECODE_ROWS", 26)):
        assert re.search(rf"^#define\s+{name}\s+{value}\s*$", body, flags=re.M), name


def test_header_comment_describes_the_ops(zk):
    text = open(zk.binding.HEADER_PATH).read()
    comment = text[:text.index("int zk_field_vec_op(")].rsplit("/*", 1)[1]
    assert comment.rstrip().endswith("*/") and comment.count("*/") == 1, "one comment, directly in front of the prototype"
    new = comment[comment.index("ZK_OP_COPY_ROWS"):]
    for word in ("values 28 and 30", "27 and 29 stay refused", "Fr only", "zk_copy_rows", "zk_copy_rlc", "zk_copy_event", "HOST pointer", "CopyTable::assignments", "assign_copy_event",
                 "assign_padding_row", "zk_proof_advice_phase_typed_dev", "88 little-endian bytes", "aux_bytes", "bytes_write_prev", "build_tx_log_address", "constrain_mask",
                 "(f, b) := (L, 0)", "is_first", "is_last", "d_tag_bits", "d_types", "value_prev", "front_mask", "word_index", "src_addr_end", "non_pad_non_mask", "real_bytes_left",
                 "rwc_inc_left", "d_src_end_rows", "ZK_OP_ROW_INV0", "d_b must be NULL", "r_word", "r_in", "value_acc", "d_word_rlc", "d_word_rlc_prev", "d_rlc_acc",
                 "constrain_event_rlc_acc", "whenever the writer's run and masks are the reader's", "d_id_other", "number_or_hash_to_field", "is_id_unchange", "empty event",
                 "cannot wrap", "saturates", "pure function", "walks an event", "identity map", "constant map", "never reads d_bytes", "validated before n is looked at",
                 "n >= 2^32", "total_bytes >= 2^61", "\"copy_rows\"", "\"copy_rlc\""):
        assert word in new, word
    # what the comment said before stays, in its order, and the new text stands behind the bytecode-rows text
    for word in ("ZK_OP_ROW_RLC", "fr_row_rlc", "ZK_OP_SCAN_RLC", "fr_scan_rlc", "ZK_OP_ROW_INV0", "fr_row_inv0", "ZK_OP_POSEIDON", "fr_poseidon", "ZK_OP_KECCAK", "fr_keccak",
                 "ZK_OP_SHA256", "fr_sha256", "ZK_OP_KEY_SORT", "\"key_sort\"", "ZK_OP_KEY_ORDER", "\"key_order\"", "ZK_OP_BYTECODE_ROWS", "23, 24, 25 and 27 stay refused"):
        assert word in comment, word
    assert comment.index("\"key_order\"") < comment.index("ZK_OP_BYTECODE_ROWS") < comment.index("\"bytecode_rows\"") < comment.index("ZK_OP_COPY_ROWS") < comment.index("\"copy_rows\"")
    assert re.sub(r"\s*\*/\s*$", "", comment).rstrip().endswith("Other op values (5, 6, 7, 11, ...) are refused.")


def test_binding_exposes_the_constants_the_structs_and_the_methods(zk):
    b = zk.binding
    assert zk.OP_COPY_ROWS == b.OP_COPY_ROWS == 28 and zk.OP_COPY_RLC == b.OP_COPY_RLC == 30 and zk.OP_BYTECODE_ROWS == 26
    sig = inspect.signature(b.Context.copy_rows)
    assert list(sig.parameters) == ["self", "events", "count", "data", "total_bytes", "n", "addr", "outputs"] and sig.parameters["outputs"].kind is inspect.Parameter.VAR_KEYWORD
    sig = inspect.signature(b.Context.copy_rlc)
    assert list(sig.parameters) == ["self", "events", "count", "data", "total_bytes", "n", "value_acc", "r_word", "r_in", "ids", "outputs"] and sig.parameters["ids"].default is None
    assert ["d_" + name for name in b.COPY_ROWS_OUTPUTS] == ROWS_OUT and ["d_" + name for name in b.COPY_RLC_OUTPUTS] == RLC_OUT
    assert "ZK_OP_COPY_ROWS" in b.Context.copy_rows.__doc__ and "ZK_OP_COPY_RLC" in b.Context.copy_rlc.__doc__
    for s, fields, offsets, size in ((b._CopyRows, ROWS_FIELDS, ROWS_OFFSETS, ROWS_SIZE), (b._CopyRlc, RLC_FIELDS, RLC_OFFSETS, RLC_SIZE), (b._CopyEvent, EVENT_FIELDS, EVENT_OFFSETS, EVENT_SIZE)):
        assert issubclass(s, ctypes.Structure) and [name for name, _ in s._fields_] == fields
        assert [getattr(s, name).offset for name in fields] == offsets and ctypes.sizeof(s) == size
    for s in (b._CopyRows, b._CopyRlc):
        types = dict(s._fields_)
        assert types["total_bytes"] is ctypes.c_uint64 and types["count"] is ctypes.c_uint32 and types["flags"] is ctypes.c_uint8
        assert all(types[name] is ctypes.c_void_p for name in types if name.startswith("d_"))
    assert [b._CopyRows._fields_[i] for i in range(5)] == [b._CopyRlc._fields_[i] for i in range(5)]


def test_the_structs_have_the_sizes_and_offsets_the_compiler_gives_them(zk, tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang") or "/opt/rocm/llvm/bin/clang"
    src = tmp_path / "layout.c"
    body = '#include <stdio.h>\n#include <stddef.h>\n#include "zkmi355.h"\nint main(void) {\n'
    for struct, fields in (("zk_copy_rows", ROWS_FIELDS), ("zk_copy_rlc", RLC_FIELDS), ("zk_copy_event", EVENT_FIELDS)):
        body += f'printf(" %zu", sizeof({struct}));\n' + "".join(f'printf(" %zu", offsetof({struct}, {name}));\n' for name in fields)
        body += "".join(f'printf(" %zu", sizeof((({struct}*)0)->{name}));\n' for name in fields)
    body += 'return ZK_OP_COPY_ROWS == 28 && ZK_OP_COPY_RLC == 30 && ZK_COPY_MEMORY_COPY == 1 ? 0 : 1; }\n'
    src.write_text(body)
    exe = tmp_path / "layout"
    subprocess.run([cc, "-I", os.path.dirname(zk.binding.HEADER_PATH), str(src), "-o", str(exe)], check=True, timeout=120)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True, timeout=60).stdout.split()]
    assert got == [ROWS_SIZE] + ROWS_OFFSETS + SHARED_SIZES + [8] * 17 + [RLC_SIZE] + RLC_OFFSETS + SHARED_SIZES + [8] * 6 + [EVENT_SIZE] + EVENT_OFFSETS + EVENT_SIZES


def test_mirror_rust_declarations_documents_tool_profile_and_makefile_name_the_ops():
    mirror = open(os.path.join(ROOT, "include", "zkmi355_halo2.hpp")).read()
    assert re.search(r"\binline void copy_rows\(", mirror) and re.search(r"\binline void copy_rlc\(", mirror)
    assert all(word in mirror for word in ("ZK_OP_COPY_ROWS", "ZK_OP_COPY_RLC", "zk_copy_rows", "zk_copy_rlc"))
    assert mirror.index("inline void bytecode_rows(") < mirror.index("inline void copy_rows(") < mirror.index("inline void copy_rlc(")
    ffi = open(os.path.join(ROOT, "shim", "halo2_proofs", "src", "zkmi355", "ffi.rs")).read()
    assert re.search(r"pub const ZK_OP_COPY_ROWS:\s*c_int\s*=\s*28;", ffi) and re.search(r"pub const ZK_OP_COPY_RLC:\s*c_int\s*=\s*30;", ffi)
    for name, fields in (("zk_copy_rows", ROWS_FIELDS), ("zk_copy_rlc", RLC_FIELDS), ("zk_copy_event", EVENT_FIELDS)):
        struct = re.search(rf"#\[repr\(C\)\]\s*pub struct {name}\s*\{{([^}}]*)\}}", ffi)
        assert struct and re.findall(r"pub (\w+):", struct.group(1)) == fields, name
    assert not re.findall(r"\bfn\s+\w*copy_r\w*", ffi), "no new function in the Rust declarations"
    for rel in ("README.md", "INTEGRATION.md", "DESIGN.md"):
        text = open(os.path.join(ROOT, rel)).read()
        assert "ZK_OP_COPY_ROWS" in text and "ZK_OP_COPY_RLC" in text, rel
    for rel in (os.path.join("profiles", "README.md"), os.path.join("tools", "README.md")):
        text = open(os.path.join(ROOT, rel)).read()
        assert "copy_rows_time.py" in text and "r31_copy_rows.md" in text, rel
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for word in ("zk_copy_rows desc", "zk_copy_rlc rlc", "copy_rows(", "copy_rlc(", "is_src_end", "is_word_end", "is_id_unchange", "d_src_end_rows", "-31", "ZK_OP_ROW_INV0", "value_acc",
                 "the upstream layout", "zk_proof_advice_phase_typed_dev", "d_id_other", "zk_copy_event"):
        assert word in integration, word
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "profiles/r31_copy_rows.md" in design and design.index("ZK_OP_BYTECODE_ROWS") < design.index("ZK_OP_COPY_ROWS")
    tool = open(os.path.join(ROOT, "tools", "copy_rows_time.py")).read()
    assert "copy_rows(" in tool and "copy_rlc(" in tool and "median" in tool and "timeout" in tool and "closed" in tool
    profile = open(os.path.join(ROOT, "profiles", "r31_copy_rows.md")).read()
    assert "VGPR" in profile and "scratch" in profile.lower() and "LDS" in profile and "k_cp_rows" in profile and "k_cp_acc_c" in profile
    makefile = open(os.path.join(ROOT, "zkevm-circuits_amd", "Makefile")).read()
    assert "csrc/copy_rows.hip" in makefile.split("HDR :=")[0] and "csrc/copy_rows.hip.hpp" in makefile.split("HDR :=")[1] and "csrc/affine.hip.hpp" in makefile.split("HDR :=")[1]
    unit = open(os.path.join(ROOT, "zkevm-circuits_amd", "csrc", "copy_rows.hip.hpp")).read()
    assert "threadIdx" not in unit and "__shared__" not in unit and "__global__" not in unit, "the header is lane-free: the host compiles it"
    source = open(os.path.join(ROOT, "zkevm-circuits_amd", "csrc", "copy_rows.hip")).read()
    assert "static_assert(offsetof(zk_copy_rows, d_events) == offsetof(zk_copy_rlc, d_events)" in source and "SC_COPY" in source
    vec = open(os.path.join(ROOT, "zkevm-circuits_amd", "csrc", "vec.hip")).read()
    assert "{ZK_OP_COPY_ROWS," in vec and "{ZK_OP_COPY_RLC," in vec


def test_no_entry_point_was_added(zk):
    declared = sorted(set(re.findall(r"\b(zk_[a-z0-9_]+)\s*\(", _header_body(zk))))
    exported = _exported(zk)
    assert declared == exported, (sorted(set(declared) - set(exported)), sorted(set(exported) - set(declared)))
    assert len(exported) == 146
    assert [name for name in exported if "copy_r" in name] == []
    assert "The C ABI has 146 entry points" in open(os.path.join(ROOT, "README.md")).read()

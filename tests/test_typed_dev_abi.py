"""CPU: the entry points for typed cells resident on the device (zk_fr_from_uint_batch, zk_proof_advice_phase_typed_dev) are
declared in include/zkmi355.h with the documented parameter lists, exported by the built library, prototyped in the Python binding
and mirrored in include/zkmi355_halo2.hpp; the header declares exactly the entry points the library exports, and README.md states
their number."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXPECTED = {
    "zk_fr_from_uint_batch": ["zk_ctx*", "const void* const*", "const uint8_t*", "size_t", "size_t", "void* const*"],
    "zk_proof_advice_phase_typed_dev": ["zk_ctx*", "zk_proof*", "const uint32_t*", "const void* const*", "const uint8_t*", "uint32_t", "void*", "uint32_t*"],
}


def _header_body(zk):
    return re.sub(r"/\*.*?\*/", "", open(zk.binding.HEADER_PATH).read(), flags=re.S)


def _exported(zk):
    """the zk_* functions in the library's dynamic symbol table"""
    nm = shutil.which("nm") or shutil.which("llvm-nm") or "/opt/rocm/llvm/bin/llvm-nm"
    out = subprocess.run([nm, "-D", "--defined-only", zk.binding.LIB_PATH], capture_output=True, text=True, check=True).stdout
    return sorted({ln.split()[-1] for ln in out.splitlines() if len(ln.split()) >= 3 and ln.split()[-2] in "TW" and ln.split()[-1].startswith("zk_")})


@pytest.mark.parametrize("name", sorted(EXPECTED))
def test_symbol_is_declared_and_exported(zk, name):
    m = re.search(r"\bint\s+" + name + r"\s*\((.*?)\)\s*;", _header_body(zk), flags=re.S)
    assert m, f"{name} is not declared in zkmi355.h"
    params = [" ".join(p.split()) for p in m.group(1).split(",")]
    assert len(params) == len(EXPECTED[name])
    for got, want in zip(params, EXPECTED[name]):
        assert got.rsplit(" ", 1)[0] == want, (name, got, want)      # the type; the last word is the parameter's name
    assert hasattr(zk.lib(), name), f"{name} is not exported by libzkmi355.so"
    assert name in _exported(zk)


@pytest.mark.parametrize("name", sorted(EXPECTED))
def test_binding_has_a_prototype(zk, name):
    fn = getattr(zk.lib(), name)
    assert fn.argtypes is not None and len(fn.argtypes) == len(EXPECTED[name])
    assert fn.restype is ctypes.c_int
    assert hasattr(zk.binding.Context, "fr_from_uint_batch") and hasattr(zk.binding.ProofSession, "advice_phase_typed_dev")


def test_cpp_mirror_and_docs_name_both_entry_points():
    for rel in ("include/zkmi355_halo2.hpp", "INTEGRATION.md", "DESIGN.md"):
        text = open(os.path.join(ROOT, rel)).read()
        for name in EXPECTED:
            assert name in text, (rel, name)
    mirror = open(os.path.join(ROOT, "include", "zkmi355_halo2.hpp")).read()
    assert re.search(r"\binline void fr_from_uint_batch\(", mirror) and re.search(r"\badvice_phase_typed_dev\(", mirror)


def test_header_and_library_have_the_same_entry_points(zk):
    declared = sorted(set(re.findall(r"\b(zk_[a-z0-9_]+)\s*\(", _header_body(zk))))
    exported = _exported(zk)
    assert declared == exported, (sorted(set(declared) - set(exported)), sorted(set(exported) - set(declared)))
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert f"The C ABI has {len(exported)} entry points" in readme and len(exported) == 146


def test_without_a_context_both_calls_fail_cleanly(zk):
    assert zk.lib().zk_fr_from_uint_batch(None, None, None, 1, 0, None) == -1
    assert zk.lib().zk_proof_advice_phase_typed_dev(None, None, None, None, None, 0, None, None) == -1

"""CPU: the typed-witness entry points (zk_fr_from_uint, zk_proof_advice_phase_typed) are exported by the built library and
declared in include/zkmi355.h with the documented parameter lists; the Python binding derives the cell width from the array."""
import re

import numpy as np
import pytest

EXPECTED = {
    "zk_fr_from_uint": ["zk_ctx*", "const void*", "uint32_t", "size_t", "void*"],
    "zk_proof_advice_phase_typed": ["zk_ctx*", "zk_proof*", "const uint32_t*", "const void* const*", "const uint8_t*", "uint32_t", "void*", "uint32_t*"],
}


def _header_params(zk, name):
    body = re.sub(r"/\*.*?\*/", "", open(zk.binding.HEADER_PATH).read(), flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\((.*?)\)\s*;", body, flags=re.S)
    assert m, f"{name} is not declared in zkmi355.h"
    return [" ".join(p.split()) for p in m.group(1).split(",")]


@pytest.mark.parametrize("name", sorted(EXPECTED))
def test_symbol_is_exported_and_declared(zk, name):
    assert hasattr(zk.lib(), name), f"{name} is not exported by libzkmi355.so"
    params = _header_params(zk, name)
    assert len(params) == len(EXPECTED[name])
    for got, want in zip(params, EXPECTED[name]):
        assert got.rsplit(" ", 1)[0] == want, (name, got, want)      # the type; the last word is the parameter's name


def test_cpp_mirror_and_docs_name_both_entry_points():
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for rel in ("include/zkmi355_halo2.hpp", "INTEGRATION.md"):
        text = open(os.path.join(root, rel)).read()
        for name in EXPECTED:
            assert name in text, (rel, name)


def test_binding_derives_the_width_from_the_array(zk):
    width = zk.binding.typed_cell_width
    n = 16
    assert [width(np.zeros(n, dtype=dt)) for dt in (np.uint8, np.uint16, np.uint32, np.uint64)] == [1, 2, 4, 8]
    assert width(np.zeros((n, 2), dtype=np.uint64)) == 16
    assert width(np.zeros((n, 4), dtype=np.uint64)) == 32
    for bad in (np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.float64), np.zeros((n, 3), dtype=np.uint64), np.zeros((n, 2), dtype=np.uint32),
                np.zeros((n, 4, 1), dtype=np.uint64)):
        with pytest.raises(zk.ZkError):
            width(bad)


def test_without_a_context_both_calls_fail_cleanly(zk):
    assert zk.lib().zk_fr_from_uint(None, None, 1, 0, None) == -1
    assert zk.lib().zk_proof_advice_phase_typed(None, None, None, None, None, 0, None, None) == -1

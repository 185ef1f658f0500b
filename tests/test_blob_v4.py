"""CPU: key blob version 4 -- typed fixed cells and halo2's permutation mapping in place of Montgomery fixed and sigma columns.
`Circuit.blob(version=4)` must carry exactly the circuit's fixed cells at their narrowest widths and `permutation_mapping()`,
its constraint-system part must be the version 3 one but for the version word, and the host-only verifying key must read it
as the same key.  `Circuit.blob()` without arguments stays the version 3 blob byte for byte."""
import ctypes
import os
import struct
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import zkevm_circuits_amd as z  # noqa: E402
from plonk_fixtures import build_circuit, build_evm_circuit, build_multi_lookup_circuit  # noqa: E402
from zkevm_circuits_amd import plonk  # noqa: E402

R = plonk.R_MOD
CIRCUITS = {
    "wide": lambda: build_circuit(6, seed=3, wide=True)[0],
    "evm": lambda: build_evm_circuit(7, seed=5)[0],
    "no_permutation": lambda: build_multi_lookup_circuit(5, seed=4)[0],
}


def widths_circuit(k=5):
    """fixed columns whose narrowest widths are 1, 2, 4, 8, 16 and 32 (each narrow one holds 0 and 2^(8w) - 1, the wide one
    r - 1) and one all-zero column; one gate so that every column is queried"""
    c = plonk.Circuit(k, num_fixed=7, num_advice=1, num_instance=0)
    for i, w in enumerate((1, 2, 4, 8, 16)):
        c.fixed[i][3] = (1 << (8 * w)) - 1
        c.fixed[i][c.n - 1] = (1 << (8 * w - 3)) + 5
    c.fixed[5][0], c.fixed[5][7] = R - 1, 1 << 128
    acc = c.fixed_col(0)
    for i in range(1, 7):
        acc = acc + c.fixed_col(i)
    c.add_gate(acc * c.advice_col(0) * 0)
    return c


def _cells(width, payload, n):
    if width == 32:
        rinv = pow(1 << 256, -1, R)
        return [int.from_bytes(payload[32 * i:32 * i + 32], "little") * rinv % R for i in range(n)]
    return [int.from_bytes(payload[width * i:width * (i + 1)], "little") for i in range(n)]


@pytest.mark.parametrize("name", sorted(CIRCUITS) + ["widths"])
def test_v4_blob_carries_the_fixed_cells_and_the_mapping(name):
    circ = widths_circuit() if name == "widths" else CIRCUITS[name]()
    blob = circ.blob(version=4)
    widths, payloads, mapping = plonk.Circuit.blob_v4_parts(blob)
    assert mapping == circ.permutation_mapping()
    assert len(widths) == circ.F
    for col, w, payload in zip(circ.fixed, widths, payloads):
        top = max(v % R for v in col)
        assert w == next((x for x in (1, 2, 4, 8, 16) if top < 1 << (8 * x)), 32)        # the narrowest that holds every cell
        assert _cells(w, payload, circ.n) == [v % R for v in col]
    cs3, cs4 = circ.cs_blob(), blob[:plonk.Circuit.cs_blob_len(blob)]
    assert len(cs3) == len(cs4) and cs4[:4] == cs3[:4] and cs4[8:] == cs3[8:]
    assert struct.unpack_from("<I", cs4, 4)[0] == 4 and struct.unpack_from("<I", cs3, 4)[0] == 3
    assert circ.cs_blob(version=4) == cs4
    assert len(blob) == len(cs3) + 4 * circ.F + sum(circ.n * w for w in widths) + 8 * len(circ.perm_cols) * circ.n


def test_widths_circuit_uses_every_width():
    widths, _, _ = plonk.Circuit.blob_v4_parts(widths_circuit().blob(version=4))
    assert widths == [1, 2, 4, 8, 16, 32, 1]


def test_v4_blob_makes_no_sigma_columns(monkeypatch):
    circ = CIRCUITS["wide"]()

    def refuse(self):
        raise AssertionError("sigma_columns() called for a version 4 blob")
    monkeypatch.setattr(plonk.Circuit, "sigma_columns", refuse)
    assert len(circ.blob(version=4)) > len(circ.cs_blob())
    with pytest.raises(AssertionError):
        circ.blob()


def test_default_blob_is_the_version_3_blob():
    assert plonk.BLOB_VERSION == 3
    for name in sorted(CIRCUITS):
        circ = CIRCUITS[name]()
        cs = circ.cs_blob()
        assert struct.unpack_from("<II", cs, 0) == (plonk.BLOB_MAGIC, 3)
        old_way = cs + b"".join(plonk.column_to_mont(col).tobytes() for col in circ.fixed) + b"".join(plonk.column_to_mont(col).tobytes() for col in circ.sigma_columns())
        assert circ.blob() == old_way == circ.blob(version=3)
        assert circ.blob(cse=True) == circ.cs_blob(cse=True) + old_way[len(cs):]


def _vk_create(data, ncom):
    lib = z.lib()
    buf = np.frombuffer(bytes(data), dtype=np.uint8).copy()
    com, rep, h = np.zeros((max(ncom, 1), 8), np.uint64), np.zeros(4, np.uint64), ctypes.c_void_p()
    rc = lib.zk_vk_create(buf.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(len(data)), com.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(ncom),
                          rep.ctypes.data_as(ctypes.c_void_p), ctypes.byref(h))
    if rc == 0:
        lib.zk_vk_destroy(h)
    return rc


@pytest.mark.parametrize("name", sorted(CIRCUITS))
def test_vk_from_a_v4_constraint_system_is_the_v3_key(name):
    circ = CIRCUITS[name]()
    ncom = circ.F + len(circ.perm_cols)
    com, rep = np.zeros((ncom, 8), np.uint64), np.zeros(4, np.uint64)
    v3 = z.VerifyingKey(circ.cs_blob(), com, rep)
    v4 = z.VerifyingKey(circ.cs_blob(version=4), com, rep)
    try:
        assert v4.shape() == v3.shape()
        for kind in (z.TRANSCRIPT_BLAKE2B, z.TRANSCRIPT_POSEIDON, z.TRANSCRIPT_EVM):
            for mo in (0, 1):
                assert v4.proof_len(kind, mo) == v3.proof_len(kind, mo)
    finally:
        v3.destroy()
        v4.destroy()
    assert _vk_create(circ.blob(version=4), ncom) == 0        # the whole key blob: its column data is sized, not read


def test_vk_refuses_other_versions_and_truncated_v4_headers():
    circ = CIRCUITS["wide"]()
    ncom = circ.F + len(circ.perm_cols)
    cs4 = circ.cs_blob(version=4)
    assert _vk_create(cs4, ncom) == 0
    for version in (2, 5, 0, 0xFFFFFFFF):
        bad = bytearray(cs4)
        bad[4:8] = struct.pack("<I", version)
        assert _vk_create(bad, ncom) == -1, version
    for cut in (4, 8, 40, 47, len(cs4) // 2, len(cs4) - 1):
        assert _vk_create(cs4[:cut], ncom) == -1, cut
    blob = circ.blob(version=4)
    assert _vk_create(blob[:-1], ncom) == -1 and _vk_create(blob + b"\0", ncom) == -1      # column data of another size than the widths say
    bad = bytearray(blob)
    bad[len(cs4):len(cs4) + 4] = struct.pack("<I", 3)                                      # no such cell width
    assert _vk_create(bad, ncom) == -1

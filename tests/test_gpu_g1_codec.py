"""GPU: the G1 codecs of SRS files (csrc/params.hip: k_g1_decode, k_g1_compress) on a container of chosen points instead of a
generic SRS: identities inside the file (at both ends of both workgroups), P next to -P, the generator, canonical x with bit 253
set right under the two flag bits, both parities of y.  All three serde formats are written and read back against the big-int
restatement of the format (oracle/params_file.py, oracle/bn254.py); then single encodings of a good file are replaced by every
kind of refused image, at workgroup boundaries of both bases and several at once, and the refusal must print the exact count.
After every refusal a good file is read on the same context: the refused read's srs, staging buffer and counter are released on
that path (zk_params_read's `fail`), and nothing of it may linger in the context.

The big-endian encoding (G1_ENC_BE_XY) is reached only through the verifier's EVM transcript: tests/test_gpu_verify.py."""
import numpy as np
import pytest

from oracle import bn254 as b
from oracle import params_file

pytestmark = pytest.mark.gpu
P = b.P_MOD
K, N = 9, 512                                                # two workgroups of 256 per basis
IDENTITIES = (0, 63, 64, 255, 256, 511)
G2, S_G2 = bytes(range(1, 129)), bytes(range(128, 0, -1))    # opaque to the library: handed through


def chosen_points(cref, seed):
    pts = cref.affine_from_mont(cref.srs_powers(seed, N))
    assert all(p is not None for p in pts) and len(set(pts)) == N
    high = [p for p in pts if p[0] >> 253]                   # canonical x in [2^253, p): bit 253 next to the flags
    assert len(high) >= 8
    for i in IDENTITIES:
        pts[i] = None
    pts[10], pts[11], pts[12] = pts[13], b.g1_neg(pts[13]), b.G1_GEN
    pts[100:108] = high[:8]
    pts[248:255] = high[:7]                                  # ... and at the end of the first workgroup
    assert pts[10][0] == pts[11][0] and pts[10][1] + pts[11][1] == P and (pts[10][1] ^ pts[11][1]) & 1
    assert sum(1 for p in pts if p and p[1] & 1) >= 8 and sum(1 for p in pts if p and not p[1] & 1) >= 8
    assert sum(1 for p in pts if p and p[0] >> 253) >= 8 and all(b.g1_is_on_curve(p) for p in pts if p)
    return pts


@pytest.fixture(scope="module")
def container(ctx, cref):
    g, lag = chosen_points(cref, 0x6A), chosen_points(cref, 0x1A6)
    assert g != lag
    srs = ctx.srs_create(K, cref.affine_to_mont(g), cref.affine_to_mont(lag))
    files = {fmt: params_file.write(K, g, lag, G2[:64 if fmt == 0 else 128], S_G2[:64 if fmt == 0 else 128], fmt) for fmt in (0, 1, 2)}
    yield srs, g, lag, files
    srs.destroy()


def read_good(ctx, cref, container, fmt):
    srs, g, lag, files = container
    back, g2, s_g2 = ctx.params_read(files[fmt], fmt)
    try:
        assert back.k == K and (g2, s_g2) == (G2[:len(g2)], S_G2[:len(s_g2)])
        assert np.array_equal(back.download_g(), srs.download_g()) and np.array_equal(back.download_g_lagrange(), srs.download_g_lagrange())
    finally:
        back.destroy()


@pytest.mark.parametrize("fmt", [0, 1, 2])
def test_written_bytes_equal_the_oracle_and_read_back(ctx, cref, container, fmt):
    srs, g, lag, files = container
    n2 = 64 if fmt == 0 else 128
    data = ctx.params_write(srs, G2[:n2], S_G2[:n2], fmt)
    assert data == files[fmt]
    if fmt == 0:                                             # the oracle's own reader takes them back too
        assert params_file.read(data, 0)[1:3] == (g, lag)
        enc = lambda i: int.from_bytes(data[4 + 32 * i:36 + 32 * i], "little")
        assert all(enc(i) == 1 << 255 for i in IDENTITIES) and enc(12) == 1 and enc(10) ^ enc(11) == 1 << 254
        assert all((enc(i) >> 253) & 1 and not enc(i) >> 255 for i in range(100, 108))
    read_good(ctx, cref, container, fmt)
    assert np.array_equal(srs.download_g(), cref.affine_to_mont(g)) and np.array_equal(srs.download_g_lagrange(), cref.affine_to_mont(lag))


def patched(data, size, edits):
    """edits: (basis 0 g / 1 g_lagrange, index, bytes)"""
    out = bytearray(data)
    for basis, i, enc in edits:
        assert len(enc) == size
        at = 4 + (basis * N + i) * size
        assert out[at:at + size] != enc
        out[at:at + size] = enc
    return bytes(out)


def refused(zk, ctx, data, fmt, count):
    with pytest.raises(zk.ZkError, match=rf"params file: {count} G1 encodings are not points of the curve"):
        ctx.params_read(data, fmt)


def no_root_x():
    return next(x for x in range(2, 200) if pow((x ** 3 + 3) % P, (P - 1) // 2, P) == P - 1)


def processed_rejects():
    le = lambda v: v.to_bytes(32, "little")
    return {"identity flag with x = 1": le(1 << 255 | 1), "identity flag with the sign bit": le(1 << 255 | 1 << 254), "x = p": le(P), "x = p + 1": le(P + 1),
            "x = 2^254 - 1": le((1 << 254) - 1), "x without a square root": le(no_root_x()), "x without a square root, sign bit": le(no_root_x() | 1 << 254)}


def test_processed_rejects_one_by_one_and_by_position(zk, ctx, cref, container):
    data = container[3][0]
    rejects = processed_rejects()
    assert P + 1 < (1 << 254) - 1 and (P + 1) % P == 1       # x = p + 1 would be the generator's x if it were reduced first
    for name, enc in rejects.items():
        refused(zk, ctx, patched(data, 32, [(0, 5, enc)]), 0, 1)
        read_good(ctx, cref, container, 0)
    enc = rejects["x = p"]
    for basis, i in ((0, 0), (0, 255), (0, 256), (0, 511), (1, 0), (1, 511)):       # first and last lane of each workgroup
        refused(zk, ctx, patched(data, 32, [(basis, i, enc)]), 0, 1)
        read_good(ctx, cref, container, 0)


def test_processed_counts_seven_rejects_over_both_bases(zk, ctx, cref, container):
    data = container[3][0]
    encs = list(processed_rejects().values())
    assert len(encs) == 7
    where = [(0, 0), (0, 255), (0, 256), (1, 1), (1, 255), (1, 300), (1, 511)]
    refused(zk, ctx, patched(data, 32, [(bs, i, e) for (bs, i), e in zip(where, encs)]), 0, 7)
    read_good(ctx, cref, container, 0)
    refused(zk, ctx, patched(data, 32, [(bs, i, e) for (bs, i), e in zip(where[:3], encs[:3])]), 0, 3)
    read_good(ctx, cref, container, 0)


def raw_images(g):
    m = lambda v: b.mont_bytes(v % P, P)
    plus_p = lambda raw: (int.from_bytes(raw, "little") + P).to_bytes(32, "little")          # the same residue, not below p
    x, y = g[20]
    tx = next(v for v in range(1, 200) if pow((v ** 3 + 2) % P, (P - 1) // 2, P) == 1 and pow((v ** 3 + 3) % P, (P - 1) // 2, P) != 1)
    ty = pow((tx ** 3 + 2) % P, (P + 1) // 4, P)
    assert ty * ty % P == (tx ** 3 + 2) % P and not b.g1_is_on_curve((tx, ty))
    return {"y + p": m(x) + plus_p(m(y)), "x + p": plus_p(m(x)) + m(y), "(0, y)": bytes(32) + m(y), "(x, 0)": m(x) + bytes(32),
            "a point of the twist y^2 = x^3 + 2": m(tx) + m(ty)}


def test_raw_rejects_and_unchecked_takes_them(zk, ctx, cref, container):
    srs, g, lag, files = container
    images = raw_images(g)
    for t, (name, enc) in enumerate(images.items()):
        basis, i = ((0, 20), (1, 255), (0, 256), (1, 511), (0, 0))[t]
        for fmt in (1, 2):
            data = patched(files[fmt], 64, [(basis, i, enc)])
            if fmt == 1:
                refused(zk, ctx, data, 1, 1)
            else:                                            # RawBytesUnchecked does not look: the bytes arrive as they are
                loose, _, _ = ctx.params_read(data, 2)
                got = (loose.download_g_lagrange() if basis else loose.download_g()).tobytes()
                loose.destroy()
                assert got[64 * i:64 * i + 64] == enc and got == data[4 + basis * N * 64:4 + (basis + 1) * N * 64], name
            read_good(ctx, cref, container, fmt)
    every = [((0, 20), (1, 255), (0, 256), (1, 511), (0, 0))[t] + (enc,) for t, enc in enumerate(images.values())]
    refused(zk, ctx, patched(files[1], 64, every), 1, 5)
    read_good(ctx, cref, container, 1)
    # (0, 0) is the identity's image: accepted wherever it stands
    zeroed = patched(files[1], 64, [(0, 20, bytes(64)), (1, 300, bytes(64))])
    back, _, _ = ctx.params_read(zeroed, 1)
    try:
        want = cref.affine_to_mont(g)
        want[20] = 0
        assert np.array_equal(back.download_g(), want) and not back.download_g_lagrange()[300].any()
    finally:
        back.destroy()

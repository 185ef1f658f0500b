"""Helper (not collected): one call of ZK_OP_CODE_HASH_ROWS or ZK_OP_CODE_HASH_TABLE on the device, every output inside one arena of
sentinels that is downloaded at once and compared byte for byte with the model of tests/code_hash_rows_cases.py."""
import numpy as np

import code_hash_rows_cases as ch

T = 1024                                     # the implementation's tile (BC_TILE of csrc/bytecode_rows.hip.hpp)
GUARD = 64                                   # sentinel bytes in front of and behind every buffer
SENT = 0xC3
OK, INVALID_ARG = 0, -1
OPS = {
    "rows": dict(op=34, out="field_input", columns=ch.ROW_COLUMNS, widths=ch.ROW_WIDTHS),
    "table": dict(op=36, out="input0", columns=ch.TABLE_COLUMNS, widths=dict(ch.TABLE_WIDTHS, rows_needed=8)),
}


def effective(buf, offs, lens, total):
    """what the ops take every entry for: an entry outside the buffer is an empty bytecode"""
    return [bytes(buf[o:o + ln]) if o <= total and ln <= total - o else b"" for o, ln in zip(offs, lens)]


class Call:
    def __init__(self, ctx, kind, n, buf, offs, lens, iw=4, outputs=None, odd=False, total=None, n_alloc=None):
        spec = OPS[kind]
        self.ctx, self.kind, self.n, self.iw, self.odd = ctx, kind, n, iw, odd
        self.out, self.widths = spec["out"], spec["widths"]
        every = tuple(c for c in spec["columns"] if c != self.out) + (("rows_needed",) if kind == "table" else ())
        self.outputs = every if outputs is None else tuple(outputs)
        self.buf = np.asarray(buf, dtype=np.uint8)
        self.total = len(self.buf) if total is None else total
        self.offs, self.lens, self.count = list(offs), list(lens), len(offs)
        self.idt = np.uint32 if iw == 4 else np.uint64
        # the bytes stand between sentinels of their own at an odd address: nothing of them is ever written
        self.src_image = np.concatenate([np.full(GUARD + 1, SENT, np.uint8), self.buf, np.full(GUARD, SENT, np.uint8)])
        self.src = ctx.to_device(self.src_image)
        self.d_offs = ctx.to_device(np.array(self.offs + [0], dtype=self.idt))
        self.d_lens = ctx.to_device(np.array(self.lens + [0], dtype=self.idt))
        cap = n if n_alloc is None else n_alloc
        self.at, size = {}, 0
        for name in (self.out,) + self.outputs:
            self.at[name] = size + GUARD + (1 if odd and self.widths[name] == 1 else 0)
            size += (2 * GUARD + self.cells_of(name, cap) * self.widths[name] + 1 + 63) & ~63
        self.size = size
        self.arena = ctx.to_device(np.full(size, SENT, np.uint8))

    def cells_of(self, name, n):
        return 1 if name == "rows_needed" else n

    def ptr(self, name):
        return self.arena.ptr + self.at[name] if name in self.at else None

    def kwargs(self):
        kw = dict(data=self.src.ptr + GUARD + 1, total_bytes=self.total, offsets=self.d_offs.ptr, lens=self.d_lens.ptr, index_width=self.iw, count=self.count, n=self.n)
        kw[self.out] = self.ptr(self.out)
        kw.update({name: self.ptr(name) for name in self.outputs})
        return kw

    def set_lens(self, lens):
        self.lens = list(lens)
        self.d_lens.upload(np.array(self.lens + [0], dtype=self.idt))

    def run(self):
        (self.ctx.code_hash_rows if self.kind == "rows" else self.ctx.code_hash_table)(**self.kwargs())
        self.ctx.sync()
        return self.arena.download(self.size, np.uint8)

    def split(self, image, written=True):
        """the bytes of every output; everything else in the arena still holds the sentinel"""
        mask = np.ones(self.size, bool)
        got = {}
        for name, at in self.at.items():
            size = self.cells_of(name, self.n) * self.widths[name] if written else 0
            mask[at:at + size] = False
            got[name] = image[at:at + size].copy()
        assert (image[mask] == SENT).all(), "a byte outside the cells of an output was written"
        return got

    def want(self):
        codes = effective(self.buf, self.offs, self.lens, self.total)
        if self.kind == "rows":
            w = ch.rows_numpy(codes, self.n)
            if self.n <= 1500:               # the line-by-line model where it is quick, the vectorised one (checked against it on the CPU) above
                line = ch.assign(codes, self.n)
                for name in ch.ROW_COLUMNS:
                    assert np.array_equal(w[name], ch.cells(name, line[name], ch.ROW_WIDTHS)), name
            return w
        w, needed = ch.table_numpy(codes, self.n)
        if self.n <= 1500:
            closed, _ = ch.table_closed(codes, self.n)
            loaded, _ = ch.dev_load(codes)
            assert needed == len(loaded)
            for name in ch.TABLE_COLUMNS:
                assert np.array_equal(w[name], ch.cells(name, closed[name], ch.TABLE_WIDTHS)), name
            for i, r in enumerate(loaded[:self.n]):
                assert (closed["input0"][i], closed["input1"][i], closed["control"][i], closed["heading_mark"][i]) == (r[0], r[1], r[2], r[4])
        w["rows_needed"] = np.array([needed], dtype="<u8").view(np.uint8)
        return w

    def compare(self, got, want, tag=None):
        for name, a in got.items():
            w = np.asarray(want[name]).view(np.uint8).reshape(-1)
            if not np.array_equal(a, w):
                width = self.widths[name]
                rows = np.argwhere((a != w).reshape(-1, width).any(axis=1))[:5].ravel().tolist()
                raise AssertionError((tag, name, "first differing rows", rows, [bytes(a[r * width:(r + 1) * width]).hex() for r in rows], [bytes(w[r * width:(r + 1) * width]).hex() for r in rows]))

    def check(self, tag=None):
        got = self.split(self.run())
        self.compare(got, self.want(), tag)
        assert np.array_equal(self.src.download(len(self.src_image), np.uint8), self.src_image), "the code bytes were written"
        return got

    def free(self):
        for b in (self.src, self.d_offs, self.d_lens, self.arena):
            b.free()


def checked(ctx, kind, codes, n=None, gap=3, **kw):
    rng = np.random.default_rng(sum(len(c) for c in codes) + len(codes))
    buf, offs, lens = ch.lay_out(codes, rng, gap)
    if n is None:
        n = sum(len(c) + 1 for c in codes) + 37 if kind == "rows" else sum(-(-len(c) // 62) for c in codes) + 5
    call = Call(ctx, kind, n, buf, offs, lens, **kw)
    try:
        return call.check()
    finally:
        call.free()

"""What the GPU tests of ZK_OP_EXP_ROWS share (not a test): one call's buffers on the device with sentinels in front of and behind
every one of them, and the closed forms of tests/exp_rows_cases.py as the bytes the op writes, computed once per scenario."""
import numpy as np

import exp_rows_cases as ex

GUARD = 64
SENT = 0xC3
OK, INVALID_ARG = 0, -1
OUT = "exponentiation_lo_hi"
OUTPUTS = tuple(name for name, _, _ in ex.OUTPUTS if name != OUT)      # the keyword outputs of Context.exp_rows, rows_needed aside
BYTES_PER_ROW = {name: width * planes for name, width, planes in ex.OUTPUTS}
SHIFT = {"is_last": 1, "mul_u16_64": 2, "mul_u16_128": 2, "parity_u16_64": 2, "parity_u16_128": 2}   # `odd`: as far off a dword as the cell allows
SCENARIOS = ex.scenarios()
_want = {}


def want_bytes(events, n, key=None):
    """{output: the n rows as bytes}; key: a name under which the result is kept for the tests that share the scenario"""
    if key is not None and key in _want:
        return _want[key]
    cols = ex.closed(events, n)
    out = {name: np.frombuffer(ex.output_bytes(cols, n, name), dtype=np.uint8) for name, _, _ in ex.OUTPUTS}
    if key is not None:
        _want[key] = out
    return out


def scenario_want(name):
    events, n = SCENARIOS[name]
    return want_bytes(events, n, key=name)


class Device:
    """the events on the device and one arena of sentinels that holds every output"""

    def __init__(self, ctx, events, n, outputs=OUTPUTS, odd=False, n_alloc=None, rows_needed=True):
        self.ctx, self.n, self.events, self.count = ctx, n, list(events), len(events)
        self.outputs = tuple(outputs)
        self.ev_image = np.concatenate([np.full(GUARD, SENT, np.uint8), ex.pack_events(self.events), np.full(GUARD, SENT, np.uint8)])
        self.ev = ctx.to_device(self.ev_image)
        cap = n if n_alloc is None else n_alloc
        self.at, size = {}, 0
        for name in (OUT,) + self.outputs + (("rows_needed",) if rows_needed else ()):
            self.at[name] = size + GUARD + (SHIFT.get(name, 0) if odd else 0)
            size += (2 * GUARD + cap * BYTES_PER_ROW.get(name, 0) + 8 + 63) & ~63
        self.size = size
        self.arena = ctx.to_device(np.full(size, SENT, np.uint8))

    def ptr(self, name):
        return self.arena.ptr + self.at[name] if name in self.at else None

    @property
    def d_events(self):
        return self.ev.ptr + GUARD if self.count else None

    def run(self):
        kw = {name: self.ptr(name) for name in self.outputs}
        if "rows_needed" in self.at:
            kw["rows_needed"] = self.ptr("rows_needed")
        self.ctx.exp_rows(self.d_events, self.count, self.n, self.ptr(OUT), **kw)
        self.ctx.sync()
        return self.image()

    def image(self):
        return self.arena.download(self.size, np.uint8)

    def clear(self):
        self.arena.upload(np.full(self.size, SENT, np.uint8))

    def check(self, image, want=None):
        """every output byte for byte, rows_needed exact, every other byte of the arena and the guards of the events still the sentinel"""
        want = want_bytes(self.events, self.n) if want is None else want
        mask = np.ones(self.size, bool)
        for name in (OUT,) + self.outputs:
            at, size = self.at[name], self.n * BYTES_PER_ROW[name]
            mask[at:at + size] = False
            got = image[at:at + size]
            if not np.array_equal(got, want[name]):
                bad = np.flatnonzero(got != want[name])
                width, planes = next((w, p) for o, w, p in ex.OUTPUTS if o == name)
                where = [(int(b) // (width * self.n), int(b) % (width * self.n) // width) for b in bad[:5]]
                raise AssertionError(f"{name}: {len(bad)} bytes differ, first (plane, row): {where}")
        if "rows_needed" in self.at and self.n:                          # n = 0 launches nothing: d_rows_needed keeps what it held
            at = self.at["rows_needed"]
            mask[at:at + 8] = False
            assert int(image[at:at + 8].view(np.uint64)[0]) == ex.rows_needed(self.events), "rows_needed"
        assert (image[mask] == SENT).all(), "a byte outside the n cells of an output was written"
        assert np.array_equal(self.ev.download(len(self.ev_image), np.uint8), self.ev_image), "the events were written"
        return image

    def free(self):
        self.ev.free()
        self.arena.free()

"""What the two GPU test files of the copy ops share (not a test): one call's buffers on the device with sentinels in front of and behind
every one of them, the model's columns as the arrays the ops write, and the scenarios both ops are run on."""
import numpy as np

import copy_rows_cases as cp

T = 1024                                     # CP_TILE of csrc/copy_rows.hip.hpp: the rows of a workgroup of ZK_OP_COPY_ROWS
STEP_BLOCK = 2048                            # SCAN_THREADS x SCAN_PER of csrc/affine.hip.hpp: the steps of a workgroup of ZK_OP_COPY_RLC (4096 rows)
SCAN_TILE = 2048                             # BC_SCAN_TILE: the entries of a workgroup of the scan of the row starts
GUARD = 64
SENT = 0xC3
OK, INVALID_ARG = 0, -1
SECOND_LEVEL_COUNT, SECOND_LEVEL_N = SCAN_TILE, 2 * STEP_BLOCK + 1
WINDOW_N = 2 * 256 * STEP_BLOCK + 1          # k_affine_b takes the block maps in windows of 256: one row more than 256 blocks of steps
R_WORD = 0x1234567890ABCDEF1234567890ABCDEF0123456789ABCDEF % cp.R
R_IN = cp.R - 0x0FEDCBA987654321
ROWS_OUTPUTS = ("is_first", "is_last", "tag", "tag_bits", "value", "value_prev", "mask", "front_mask", "word_index", "src_addr_end", "is_pad", "non_pad_non_mask",
                "real_bytes_left", "rw_counter", "rwc_inc_left", "types", "src_end_rows")
RLC_OUTPUTS = ("id", "id_other", "rlc_acc", "word_rlc", "word_rlc_prev")
WIDTH = {name: 1 for name in cp.BYTE_COLUMNS}
WIDTH.update({name: 8 for name in cp.WORD_COLUMNS})
WIDTH.update(cp.PLANE_COLUMNS)
WIDTH.update({name: 32 for name in cp.FR_COLUMNS})


def heap_of(size, seed=1):
    return bytes(np.random.default_rng(seed).integers(0, 256, size, dtype=np.uint8))


def want_arrays(events, heap, n, names=None):
    """the closed forms as the arrays the ops write: bytes (n,), planes (P, n), 8-byte cells (n,), Fr (n, 4) Montgomery limbs"""
    c = cp.closed(events, heap, n, R_WORD, R_IN)
    names = tuple(WIDTH) if names is None else names
    out = {}
    for name in names:
        if name in cp.PLANE_COLUMNS:
            out[name] = np.array([c[f"{name}{b}"] for b in range(cp.PLANE_COLUMNS[name])], dtype=np.uint8).reshape(cp.PLANE_COLUMNS[name], n)
        elif name in cp.FR_COLUMNS:
            out[name] = cp.fr_numpy(c[name]) if n else np.zeros((0, 4), np.uint64)
        else:
            out[name] = np.array(c[name], dtype=np.uint8 if WIDTH[name] == 1 else np.uint64)
    return out


def value_acc_only(events, heap, n, thread):
    """A_t(s) of the header comment for one thread, as a tight loop: the canonical integers of the thread's rows, in row order"""
    out, row = [], thread
    for e in cp.effective(events, len(heap)):
        L = e["length"]
        f, b = (e["dst_front"], e["dst_back"]) if thread else (e["src_front"], e["src_back"])
        if f + b >= L:
            f, b = L, 0
        off, acc = e["dst_off"] if thread else e["src_off"], 0
        for s in range(L):
            if row >= n:
                return out
            if f <= s < L - b:
                pad = thread == 0 and (e["src_addr"] + s - f) % cp.M64 >= e["src_addr_end"]
                acc = (acc * R_IN + (0 if pad else heap[off + s])) % cp.R
            out.append(acc)
            row += 2
    out += [0] * len(range(row, n, 2))
    return out


def join(parts):
    """want_arrays of consecutive row ranges, joined along the rows"""
    return {name: np.concatenate([p[name] for p in parts], axis=1 if name in cp.PLANE_COLUMNS else 0) for name in parts[0]}


class Device:
    """one set of inputs on the device and one arena of sentinels that holds every output of both ops"""

    def __init__(self, ctx, events, heap, n, odd=False, total=None, n_alloc=None, ids=True, rows_outputs=ROWS_OUTPUTS, rlc_outputs=RLC_OUTPUTS):
        self.ctx, self.n, self.events, self.heap = ctx, n, list(events), bytes(heap)
        self.total = len(heap) if total is None else total
        self.count = len(self.events)
        self.rows_outputs, self.rlc_outputs = tuple(rows_outputs), tuple(rlc_outputs)
        self.src_image = np.concatenate([np.full(GUARD + 1, SENT, np.uint8), np.frombuffer(self.heap, dtype=np.uint8), np.full(GUARD, SENT, np.uint8)])
        self.src = ctx.to_device(self.src_image)
        self.ev_image = np.concatenate([np.full(GUARD, SENT, np.uint8), cp.pack_events(self.events), np.full(GUARD, SENT, np.uint8)])
        self.ev = ctx.to_device(self.ev_image)
        self.ids = ctx.to_device(cp.pack_ids(self.events)) if ids and self.count else None
        cap = n if n_alloc is None else n_alloc
        self.at, size = {}, 0
        for name in ("addr",) + self.rows_outputs + ("value_acc",) + self.rlc_outputs:
            self.at[name] = size + GUARD + (1 if odd and name in cp.BYTE_COLUMNS + tuple(cp.PLANE_COLUMNS) else 0)
            size += (2 * GUARD + cap * WIDTH[name] + 1 + 63) & ~63
        self.size = size
        self.arena = ctx.to_device(np.full(size, SENT, np.uint8))
        self.written = set()

    def ptr(self, name):
        return self.arena.ptr + self.at[name] if name in self.at else None

    @property
    def d_events(self):
        return self.ev.ptr + GUARD

    @property
    def d_bytes(self):
        return self.src.ptr + GUARD + 1

    def upload_events(self, events):
        self.events = list(events)
        assert len(self.events) == self.count
        self.ev_image[GUARD:GUARD + 88 * self.count] = cp.pack_events(self.events)
        self.ev.upload(self.ev_image)

    def run_rows(self):
        self.ctx.copy_rows(self.d_events, self.count, self.d_bytes, self.total, self.n, self.ptr("addr"), **{name: self.ptr(name) for name in self.rows_outputs})
        self.ctx.sync()
        self.written |= {"addr", *self.rows_outputs}
        return self.image()

    def run_rlc(self):
        self.ctx.copy_rlc(self.d_events, self.count, self.d_bytes, self.total, self.n, self.ptr("value_acc"), cp.fr_numpy([R_WORD])[0], cp.fr_numpy([R_IN])[0],
                          ids=None if self.ids is None else self.ids.ptr, **{name: self.ptr(name) for name in self.rlc_outputs})
        self.ctx.sync()
        self.written |= {"value_acc", *self.rlc_outputs}
        return self.image()

    def image(self):
        return self.arena.download(self.size, np.uint8)

    def clear(self):
        self.arena.upload(np.full(self.size, SENT, np.uint8))
        self.written = set()

    def split(self, image):
        """the n cells of every output written so far; everything else in the arena still holds the sentinel"""
        mask = np.ones(self.size, bool)
        got, n = {}, self.n
        for name in self.written:
            at, width = self.at[name], WIDTH[name]
            mask[at:at + n * width] = False
            cells = image[at:at + n * width].copy()
            if name in cp.PLANE_COLUMNS:
                got[name] = cells.reshape(width, n)
            elif width == 32:
                got[name] = cells.view(np.uint64).reshape(n, 4)
            else:
                got[name] = cells.view(np.uint8 if width == 1 else np.uint64)
        assert (image[mask] == SENT).all(), "a byte outside the n cells of an output was written"
        return got

    def want(self, names=None):
        events = self.events if self.ids is not None else [dict(e, src_id=0, dst_id=0) for e in self.events]     # d_ids NULL: 0 on the rows of events
        return want_arrays(events, self.heap[:self.total], self.n, names=tuple(self.written) if names is None else names)

    def check(self, image, want=None):
        got = self.split(image)
        want = self.want() if want is None else want
        for name, a in got.items():
            w = want[name]
            diff = np.asarray(a != w)
            diff = diff.any(axis=0) if name in cp.PLANE_COLUMNS else diff.reshape(self.n, -1).any(axis=1) if self.n else np.zeros(0, bool)
            rows = np.argwhere(diff)[:5].ravel().tolist()
            assert not diff.any(), (name, "first differing rows", rows, [a[..., i].tolist() if name in cp.PLANE_COLUMNS else a[i].tolist() for i in rows],
                                    [w[..., i].tolist() if name in cp.PLANE_COLUMNS else w[i].tolist() for i in rows])
        assert np.array_equal(self.src.download(len(self.src_image), np.uint8), self.src_image), "the byte heap was written"
        assert np.array_equal(self.ev.download(len(self.ev_image), np.uint8), self.ev_image), "the events were written"
        return got

    def free(self):
        for b in (self.src, self.ev, self.ids, self.arena):
            if b is not None:
                b.free()


def sweep(ctx, firsts, tail, heap, run, names):
    """events [first, tail] for every first event of the list, on one arena: only the first record changes, on the device"""
    n = max(2 * f["length"] for f in firsts) + 2 * tail["length"] + 9
    d = Device(ctx, [firsts[0], tail], heap, n, rows_outputs=ROWS_OUTPUTS if run == "run_rows" else (), rlc_outputs=RLC_OUTPUTS if run == "run_rlc" else ())
    try:
        w_tail = want_arrays([tail], heap, 2 * tail["length"], names)
        for first in firsts:
            d.upload_events([first, tail])
            rows = 2 * first["length"] + 2 * tail["length"]
            want = join([want_arrays([first], heap, 2 * first["length"], names), w_tail, want_arrays([], heap, n - rows, names)])
            d.check(getattr(d, run)(), want)
        assert all(np.array_equal(v, want[k]) for k, v in want_arrays(d.events, heap, n, names).items()), "the joined parts are the model of the whole"
    finally:
        d.free()


def busy_event(length, heap_len, seed=0, **kw):
    """an event with everything switched on: aux bytes, previous bytes, masks that differ between the threads, a source that ends early"""
    rng = np.random.default_rng(seed + length)
    at = lambda: int(rng.integers(0, heap_len - length + 1))           # noqa: E731
    f = dict(src_tag=cp.MEMORY, dst_tag=cp.BYTECODE, src_addr=40, src_addr_end=40 + max(0, length - 9), dst_addr=7, rw_counter=1000, src_off=at(), dst_off=at(), prev_off=at(),
             src_front=min(3, length), src_back=min(2, max(0, length - 3)), dst_front=min(5, length), dst_back=0, src_id=11 + seed, dst_id=12 + seed)
    f.update(kw)
    return cp.event(length, **f)


def scenarios():
    """name -> (events, heap, n): every one at most 2^14 rows"""
    heap = heap_of(9000, 3)
    rng = np.random.default_rng(4)
    one_step = [cp.event(1, int(rng.integers(1, 6)), int(rng.integers(1, 6)), src_off=int(rng.integers(0, 8999)), dst_off=int(rng.integers(0, 8999)), src_addr=int(k),
                         src_addr_end=int(k) + int(rng.integers(0, 2)), rw_counter=int(k), src_front=int(rng.integers(0, 2)), dst_front=int(rng.integers(0, 2)),
                         src_id=int(k) + 1, dst_id=int(k) + 2) for k in range(4096)]
    mixed = cp.random_events(np.random.default_rng(5), 60, len(heap), max_len=300)
    second_levels = [busy_event(1, len(heap), seed=k) for k in range(SECOND_LEVEL_COUNT - 1)] + [busy_event(300, len(heap))]
    return {
        "one_event_fills_all_rows": ([busy_event(8192, len(heap))], heap, 16384),
        "4096_events_of_one_step": (one_step, heap, 8192 + 3),
        "mixed_random_events": (mixed, heap, sum(2 * e["length"] for e in mixed) + 11),
        "an_event_cut_at_n": ([busy_event(50, len(heap)), busy_event(700, len(heap), dst_tag=cp.RLC_ACC)], heap, 100 + 900),
        "n_odd_cuts_between_reader_and_writer": ([busy_event(50, len(heap)), busy_event(700, len(heap))], heap, 100 + 901),
        "n_odd_with_padding": ([busy_event(50, len(heap))], heap, 2 * T + 1),
        "no_events": ([], heap, T + 5),
        "n_smaller_than_the_first_event": ([busy_event(3000, len(heap)), busy_event(5, len(heap))], heap, 37),
        "one_row": ([busy_event(3, len(heap))], heap, 1),
        "overlapping_and_repeated_runs": ([busy_event(100, len(heap), src_off=10, dst_off=11, prev_off=12), busy_event(100, len(heap), src_off=10, dst_off=10, prev_off=10),
                                           busy_event(100, len(heap), src_off=10, dst_off=11, prev_off=12),
                                           cp.event(2000, cp.TX_CALLDATA, cp.TX_LOG, dst_addr_bias=cp.log_bias(2), src_off=0, src_addr_end=1990),
                                           cp.event(2000, cp.MEMORY, cp.MEMORY, flags=1, src_off=1, src_front=7, dst_front=1, src_id=9, dst_id=9)], heap, 2 * 4300 + 1),
        # SECOND_LEVEL_COUNT = 2048 events make 2049 scan entries, one more than a workgroup of the scan of the row starts takes;
        # SECOND_LEVEL_N = 4097 rows are 2049 steps, one more than a workgroup of the step maps of ZK_OP_COPY_RLC takes (the last event
        # is cut there); ZK_OP_COPY_ROWS has no hierarchy above its tiles
        "second_level_of_the_scan_and_of_the_step_maps": (second_levels, heap, SECOND_LEVEL_N),
    }

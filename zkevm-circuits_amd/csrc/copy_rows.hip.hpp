// Lane-free code of ZK_OP_COPY_ROWS and ZK_OP_COPY_RLC (csrc/copy_rows.hip holds the kernels and the host side): the event record, the
// rule that makes an event an empty one, what one row of the copy circuit holds as closed forms of (event, row), and the affine map of
// one step of value_acc.  Nothing here names a thread, a wave or LDS, so the host compiles it as it stands:
// tests/host_copy_rows_harness.hip drives whole small inputs serially through exactly these functions.
//
// Rows.  Event e of L_e steps owns the 2 L_e rows from start_e = sum_(c<e) 2 L_c (exclusive scan under bc_sat_add, saturating at n);
// row j of the event is step s = j >> 1 of thread t = j & 1 (0 the reader, 1 the writer).  The rows from start_count on are padding.
// Every column of the reference's serial loop (table.rs CopyTable::assignments) is a closed form of (event, s, t): a thread's masks
// are a masked prefix of f steps and a masked suffix of b steps, its address advances once per step behind the prefix, its bytes_left
// falls once per unmasked step, the rw counters move once per 32 steps.  A thread whose masks cover the whole event (f + b >= L) keeps
// front_mask = 1 on every row and never advances: (f, b) := (L, 0).
//
// value_acc in step space, per thread: A(s) = mask ? A(s - 1) : A(s - 1) r + (is_pad ? 0 : value), A(-1) = 0.  A masked step is the
// identity map, an unmasked one z -> r z + v, and step 0 of an event, which starts from 0, the constant map of its value: a scan over
// these maps needs no segment flags.  Padding steps are the constant 0.
#pragma once
#include "bytecode_rows.hip.hpp"

namespace zk {

constexpr uint32_t CP_LANES = 256, CP_PER_LANE = 4, CP_TILE = CP_LANES * CP_PER_LANE;
constexpr uint32_t CP_EVENT_BYTES = 88, CP_EVENT_WORDS = CP_EVENT_BYTES / 8;
constexpr uint32_t CP_TAG_MEMORY = 2, CP_TAG_BYTECODE = 1, CP_TAG_TXLOG = 4, CP_TAG_RLC = 5;

// a zk_copy_event out of its eleven little-endian 8-byte words
struct CpEvent {
    uint64_t src_addr, src_addr_end, dst_addr, bias, rw, src_off, dst_off, prev_off;
    uint32_t len, src_front, src_back, dst_front, dst_back;
    uint32_t src_tag, dst_tag, flags, reserved;
};
ZK_BC_HD CpEvent cp_event(const uint64_t (&w)[CP_EVENT_WORDS]) {
    CpEvent e;
    e.src_addr = w[0], e.src_addr_end = w[1], e.dst_addr = w[2], e.bias = w[3], e.rw = w[4];
    e.src_off = w[5], e.dst_off = w[6], e.prev_off = w[7];
    e.len = (uint32_t)w[8], e.src_front = (uint32_t)(w[8] >> 32);
    e.src_back = (uint32_t)w[9], e.dst_front = (uint32_t)(w[9] >> 32);
    e.dst_back = (uint32_t)w[10];
    e.src_tag = (uint32_t)(w[10] >> 32) & 0xffu, e.dst_tag = (uint32_t)(w[10] >> 40) & 0xffu;
    e.flags = (uint32_t)(w[10] >> 48) & 0xffu, e.reserved = (uint32_t)(w[10] >> 56) & 0xffu;
    return e;
}
// an event with a tag outside 1..5, a nonzero reserved byte, flag bits other than bit 0 or a byte run that does not lie inside the
// heap counts as an empty event; written so that nothing wraps
ZK_BC_HD bool cp_run_ok(uint64_t off, uint32_t len, uint64_t total) { return off <= total && len <= total - off; }
ZK_BC_HD bool cp_event_ok(const CpEvent& e, uint64_t total) {
    return e.src_tag - 1u < 5u && e.dst_tag - 1u < 5u && !e.reserved && !(e.flags & ~1u) && cp_run_ok(e.src_off, e.len, total) &&
           cp_run_ok(e.dst_off, e.len, total) && cp_run_ok(e.prev_off, e.len, total);
}
// the rows of an event, saturating at cap = n
ZK_BC_HD uint32_t cp_rows_of(uint32_t len, uint32_t cap) { return 2ull * len < cap ? 2u * len : cap; }

// the masks of thread t as (front, back) counts, a wholly masked thread as (L, 0)
ZK_BC_HD void cp_masks(const CpEvent& e, uint32_t t, uint32_t& f, uint32_t& b) {
    f = t ? e.dst_front : e.src_front, b = t ? e.dst_back : e.src_back;
    if ((uint64_t)f + b >= e.len) f = e.len, b = 0;
}
ZK_BC_HD bool cp_masked(uint32_t s, uint32_t len, uint32_t f, uint32_t b) { return s < f || s >= len - b; }
// the reader's address has reached src_addr_end at step s: the value counts as 0
ZK_BC_HD bool cp_is_pad(const CpEvent& e, uint32_t s, uint32_t f) { return e.src_addr + (s > f ? s - f : 0u) >= e.src_addr_end; }
ZK_BC_HD bool cp_has_rlc(const CpEvent& e) { return e.src_tag == CP_TAG_RLC || e.dst_tag == CP_TAG_RLC || e.dst_tag == CP_TAG_BYTECODE; }

// ---- one row ----------------------------------------------------------------------------------------------------------------------------
struct CpRow {
    uint64_t addr, src_addr_end, real_bytes_left, rw_counter, rwc_inc_left;
    uint8_t is_first, is_last, tag, value, value_prev, mask, front_mask, word_index, is_pad, non_pad_non_mask, memory_copy, src_end_row;
};
// the padding row i (copy_circuit.rs assign_padding_row)
ZK_BC_HD CpRow cp_padding_row(uint32_t i) {
    CpRow r{};
    r.is_last = (uint8_t)(i & 1u);
    r.src_addr_end = 1;
    r.mask = r.front_mask = r.src_end_row = 1;
    return r;
}
// row j of an event that counts (cp_event_ok); v, vp: the thread's byte of step j >> 1 and the byte written before (the reader: v)
ZK_BC_HD CpRow cp_row(const CpEvent& e, uint32_t j, uint32_t v, uint32_t vp) {
    CpRow r;
    const uint32_t s = j >> 1, t = j & 1u, L = e.len;
    uint32_t f, b;
    cp_masks(e, t, f, b);
    const uint32_t adv = s > f ? s - f : 0u, unmasked = L - f - b;
    const uint64_t cl = (uint64_t)e.src_front + e.src_back >= L ? 0u : L - e.src_front - e.src_back;
    r.is_first = (uint8_t)(j == 0);
    r.is_last = (uint8_t)(s == L - 1 && t == 1);
    r.tag = (uint8_t)(t ? e.dst_tag : e.src_tag);
    r.value = (uint8_t)v;
    r.value_prev = (uint8_t)(t ? vp : v);
    r.mask = (uint8_t)cp_masked(s, L, f, b);
    r.front_mask = (uint8_t)(s < f);
    r.word_index = (uint8_t)(s & 31u);
    r.addr = (t ? e.dst_addr + e.bias : e.src_addr) + adv;
    r.src_addr_end = t ? e.dst_addr + L : e.src_addr_end;
    r.is_pad = (uint8_t)(t == 0 && cp_is_pad(e, s, f));
    r.non_pad_non_mask = (uint8_t)(!r.is_pad && !r.mask);
    r.real_bytes_left = cl - (adv < unmasked ? adv : unmasked);
    const uint64_t R = e.src_tag == CP_TAG_MEMORY, W = e.dst_tag == CP_TAG_MEMORY || e.dst_tag == CP_TAG_TXLOG;
    const uint64_t delta = (R + W) * (L / 32), q = s / 32;
    r.memory_copy = (uint8_t)(e.flags & 1u);
    if (r.memory_copy) {
        r.rw_counter = e.rw + (t ? delta / 2 : 0u) + q;
        r.rwc_inc_left = (t ? delta - delta / 2 : delta) - q;
    } else {
        const uint64_t inc = q * (R + W) + (t == 1 && (s & 31u) == 31u ? R : 0u);
        r.rw_counter = e.rw + inc;
        r.rwc_inc_left = delta - inc;
    }
    r.src_end_row = (uint8_t)(t == 0);
    return r;
}

// ---- one step of value_acc ----------------------------------------------------------------------------------------------------------------
enum CpStep : uint32_t { CP_KEEP = 0, CP_CONST = 1, CP_STEP = 2 };   // z -> z;  z -> x;  z -> r z + x
// step s of thread t of an event that counts; v: the thread's byte.  x: the plain integer that is added
ZK_BC_HD uint32_t cp_acc_step(const CpEvent& e, uint32_t s, uint32_t t, uint32_t v, uint32_t& x) {
    uint32_t f, b;
    cp_masks(e, t, f, b);
    const bool masked = cp_masked(s, e.len, f, b);
    x = masked || (t == 0 && cp_is_pad(e, s, f)) ? 0u : v;
    return s == 0 ? CP_CONST : masked ? CP_KEEP : CP_STEP;
}

// the word RLCs at step s restart from the first byte of the word where nothing is carried into the step (a lane's first step, an
// event's first step) or the word begins: the first step to run through
ZK_BC_HD uint32_t cp_word_from(uint32_t s, bool fresh) { return fresh || (s & 31u) == 0 ? s & ~31u : s; }

}  // namespace zk

// Host-side helpers the descriptor ops of zk_field_vec_op share (row RLC, row inverse, scan RLC, Poseidon, Keccak, SHA-256, key sort,
// key order) and the typed-cell expansion: the plain constants 2^e mod r, the rules of a typed cell's width and alignment, and the rule
// "no output overlaps an input or another output".  Nothing here formats a message: the texts differ per op and stay with the caller.
#pragma once
#include <cstdint>

#include "ff.hip.hpp"

namespace zk {

// the integer 2^e mod r, e >= 256 (Fr::one() holds 2^256).  A loop of e - 256 doublings: callers keep the result in a function-local
// static where they are called more than once per context.
inline Fr fr_pow2(int e) {
    Fr c = Fr::one();
    for (int i = 256; i < e; ++i) c = dbl(c);
    return c;
}

// typed cells: little-endian unsigned integers of 1, 2, 4, 8 or 16 bytes at an address that is a multiple of their width, and, where
// the op takes them, 32-byte Montgomery elements at a multiple of 8 (the kernels read those as four 8-byte words)
inline bool typed_cell_width_ok(uint32_t width, bool allow32) {
    return width == 1 || width == 2 || width == 4 || width == 8 || width == 16 || (allow32 && width == 32);
}
inline uint32_t typed_cell_align(uint32_t width) { return width == 32 ? 8 : width; }

// A buffer an op reads or writes: [lo, hi) under the name the message gives it.
struct Span { uintptr_t lo, hi; const char* what; bool out; };
// The buffers of one call, in the order they were added.  overlap: the first pair in that order of which at least one is an output
// and whose ranges intersect.
template <int CAP>
struct SpanList {
    Span span[CAP];
    int count = 0;
    void add(const void* p, uint64_t bytes, const char* what, bool out) {      // NULL and empty buffers take no part
        if (p && bytes) span[count++] = {(uintptr_t)p, (uintptr_t)p + bytes, what, out};
    }
    bool overlap(const char** a, const char** b) const {
        for (int i = 0; i < count; ++i)
            for (int j = i + 1; j < count; ++j)
                if ((span[i].out || span[j].out) && span[i].lo < span[j].hi && span[j].lo < span[i].hi) { *a = span[i].what; *b = span[j].what; return true; }
        return false;
    }
};

}  // namespace zk

// Lane-free code of ZK_OP_BYTECODE_ROWS (csrc/bytecode_rows.hip holds the kernels and the host side): the geometry, what one row of
// the bytecode circuit holds, and every step of the parallel form of push_data_left.  Nothing here names a thread, a wave or LDS, so
// the host compiles it as it stands: tests/host_bytecode_rows_harness.hip drives whole small inputs serially, lanes as a loop, through
// exactly these functions.
//
// Rows.  Bytecode b of L_b bytes owns the L_b + 1 rows from start_b = sum_(c<b) (L_c + 1): a header row, then one row per byte; the
// rows behind the last bytecode are padding.  start is an exclusive scan of min(L_b + 1, n) under an addition that saturates at n
// (bc_sat_add: associative, so any scan tree gives the same sums), exact while it is <= n.
//
// push_data_left as a state s in 0..32 that ENTERS a row: a byte row holds s and hands s ? s - 1 : P(v) to the next row, a header or
// padding row (a "reset" row) holds 0 and hands 0 on, whatever entered.  A row that is entered with 0 is a LANDING row.  From a landing
// byte row the next landing row is fixed: next(i) = i + 1 + P(v_i), or the next reset row if that comes first and lies inside the
// tile (bc_next); from a reset row it is i + 1.
// So, inside a tile of BC_TILE rows, with h0 the first reset row of the tile (BC_TILE if none) and e the state that enters row 0:
//   the first landing row is c0 = min(e, h0) (e rows of push data, cut short by a reset row, which is itself a landing row);
//   the landing rows are next^t(c0);  the state that leaves the tile is next^t(c0) - BC_TILE for the first t that leaves it.
// next^(2^k) comes from k rounds of pointer doubling (bc_jump_twice); the tile's exit map is exit[e] = jump[min(e, h0)] - BC_TILE for
// the 33 states, a string of BC_STATES bytes.  Exit maps compose (bc_apply), and composition is associative: a node of the hierarchy
// composes BC_FAN children in order and keeps, per child, the map "state entering the node -> state entering the child", so the state
// that enters a tile is one lookup per level from the root, which is entered with 0.
#pragma once
#include "ff.hip.hpp"

namespace zk {

#define ZK_BC_HD __host__ __device__ __forceinline__

constexpr uint32_t BC_LANES = 256, BC_PER_LANE = 4, BC_TILE = BC_LANES * BC_PER_LANE, BC_TILE_LOG2 = 10;
constexpr uint32_t BC_STATES = 33, BC_MAP_STRIDE = 36;               // a map: 33 bytes in a slot of nine words
constexpr uint32_t BC_FAN = 64, BC_FAN_LOG2 = 6, BC_MAX_LEVELS = 4;   // 2^32 rows are 2^22 tiles: 2^16, 2^10, 2^4, 1 nodes above them
constexpr uint32_t BC_SCAN_ITEMS = 8, BC_SCAN_TILE = BC_LANES * BC_SCAN_ITEMS;
static_assert(BC_TILE == 1u << BC_TILE_LOG2 && BC_TILE >= BC_STATES && BC_FAN == 1u << BC_FAN_LOG2, "geometry");

enum BcKind : uint32_t { BC_PAD = 0, BC_HEADER = 1, BC_BYTE = 2 };

// push_data_size of a byte value: PUSH1 .. PUSH32 are 0x60 .. 0x7f
ZK_BC_HD uint32_t bc_push_size(uint32_t v) { return v - 0x60u < 0x20u ? v - 0x5fu : 0u; }
// an entry that does not lie inside the buffer counts as an empty bytecode; written so that nothing wraps
ZK_BC_HD bool bc_entry_ok(uint64_t off, uint64_t len, uint64_t total) { return off <= total && len <= total - off; }
// the rows of a bytecode, and their sums: both saturate at cap = n
ZK_BC_HD uint32_t bc_rows_of(uint64_t len, uint32_t cap) { return len < cap ? (uint32_t)len + 1u : cap; }
ZK_BC_HD uint32_t bc_sat_add(uint32_t a, uint32_t b, uint32_t cap) {
    const uint64_t s = (uint64_t)a + b;
    return s < cap ? (uint32_t)s : cap;
}
// the largest b in [lo, hi] with starts[b] <= row; starts is non-decreasing and starts[lo] <= row
ZK_BC_HD uint32_t bc_find(const uint32_t* starts, uint32_t lo, uint32_t hi, uint32_t row) {
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo + 1) / 2;
        if (starts[mid] <= row) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}
// the next landing row behind landing row i of a tile.  rows_left: the rows from this one up to the next reset row (L - p >= 1 for
// the byte at position p).  At most i + 33.  A reset row cuts the data short only where it lies inside the tile: behind the tile's
// end the rows up to it still hold their push_data_left, so what leaves the tile is the uncut i + 1 + P(v) - BC_TILE, and the
// next tile meets the reset row as its own h0.
ZK_BC_HD uint32_t bc_next(uint32_t i, uint32_t kind, uint32_t v, uint64_t rows_left) {
    if (kind != BC_BYTE) return i + 1;
    const uint32_t to = i + 1 + bc_push_size(v);
    const uint64_t reset_at = i + rows_left;
    return reset_at < BC_TILE && reset_at < to ? (uint32_t)reset_at : to;
}
// one round of pointer doubling: a value of BC_TILE or more has left the tile and stays
ZK_BC_HD uint32_t bc_jump_twice(const uint16_t* jump, uint32_t i) {
    const uint32_t j = jump[i];
    return j < BC_TILE ? jump[j] : j;
}
ZK_BC_HD uint32_t bc_first_landing(uint32_t entry, uint32_t h0) { return entry < h0 ? entry : h0; }
ZK_BC_HD uint32_t bc_exit_state(uint32_t left_at) { return left_at - BC_TILE; }                // left_at in [BC_TILE, BC_TILE + 32]
ZK_BC_HD uint32_t bc_apply(const uint8_t* map, uint32_t s) { return s < BC_STATES ? map[s] : 0u; }
// node of tile t at level l (level 0: the tiles), and the number of nodes of a level
ZK_BC_HD uint64_t bc_node(uint64_t tile, uint32_t level) { return tile >> (BC_FAN_LOG2 * level); }
ZK_BC_HD uint64_t bc_nodes(uint64_t tiles, uint32_t level) {
    for (uint32_t l = 0; l < level; ++l) tiles = (tiles + BC_FAN - 1) / BC_FAN;
    return tiles;
}

// ---- one row ----------------------------------------------------------------------------------------------------------------------------
struct BcRow {
    uint32_t index, value, length;
    uint8_t tag, is_code, push_data_left, push_data_size, acc_kind, rlc_kind;
};
// kind: BC_PAD, BC_HEADER or BC_BYTE; p: the position of the byte; len: L_b; v: the byte; s: the state that enters the row
ZK_BC_HD BcRow bc_row(uint32_t kind, uint64_t p, uint64_t len, uint32_t v, uint32_t s) {
    BcRow r;
    const bool byte = kind == BC_BYTE, last = p + 1 == len;
    const uint32_t size = byte ? bc_push_size(v) : 0u;
    s = byte ? s : 0u;
    r.tag = (uint8_t)byte;
    r.index = byte ? (uint32_t)p : 0u;
    r.value = byte ? v : kind == BC_HEADER ? (uint32_t)len : 0u;
    r.length = kind == BC_PAD ? 0u : (uint32_t)len;
    r.is_code = (uint8_t)(byte && s == 0);
    r.push_data_left = (uint8_t)s;
    r.push_data_size = (uint8_t)size;
    r.acc_kind = (uint8_t)(byte && s > 0);
    // push_rlc: a data row takes the accumulator where its instruction ends (1), else the value of the row below (2); the opcode
    // row of a push that has data rows below it copies too
    r.rlc_kind = !byte ? 0 : s > 0 ? ((s == 1 || last) ? 1 : 2) : (size > 0 && !last) ? 2 : 0;
    return r;
}

}  // namespace zk

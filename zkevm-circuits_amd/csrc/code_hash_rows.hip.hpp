// Lane-free code of ZK_OP_CODE_HASH_ROWS and ZK_OP_CODE_HASH_TABLE (csrc/code_hash_rows.hip holds the kernels and the host side): what
// one row of the bytecode circuit's Poseidon-hash extension holds (bytecode_circuit/circuit/to_poseidon_hash.rs assign_extended_row,
// set_header_row), what one row of the code-hash part of the PoseidonTable holds (table.rs PoseidonTable::dev_load over
// unroll_to_hash_input_default), and how up to 31 bytes become one field element.  Nothing here names a thread, a wave or LDS, so the
// host compiles it as it stands: tests/host_code_hash_rows_harness.hip drives whole small inputs serially through exactly these
// functions.  The geometry, the saturating sums and the search are those of bytecode_rows.hip.hpp.
//
// Both are closed forms of a row's position.  The reference carries row_input from row to row and clears it behind a field border
// and on a header row; so on byte row p of a bytecode, with m = p mod 31, field_input is the big-endian integer of the bytes
// B[p - m .. p], left-aligned in 31 bytes: sum_(t<=m) B[p - m + t] 256^(30 - t).  That is an integer below 2^248 < r: four 64-bit
// limbs straight from the bytes, and one Montgomery product with R^2 makes it an element.  Table row j of a bytecode holds the same
// integer for the whole fields [62 j, 62 j + 31) and [62 j + 31, 62 j + 62), cut at L: a border row's field_input.
#pragma once
#include "bytecode_rows.hip.hpp"

namespace zk {

constexpr uint32_t CH_F = 31, CH_W = 62;                            // HASHBLOCK_BYTES_IN_FIELD, and PoseidonTable::INPUT_WIDTH = 2 of them
static_assert(CH_W == 2 * CH_F && CH_F == 31, "the op is not generic in the field width: 31 bytes lie below the modulus, the tables hold 32 and 31 entries");
constexpr uint32_t CH_KIND_HEAD = 0, CH_KIND_CONT = 1, CH_KIND_OFF = 2;   // the kinds of ZK_OP_POSEIDON

// 256^k, k = 0 .. 31, and 1 / k, k = 1 .. 30 (entry 0: 0), as Montgomery Fr
ZK_BC_HD Fr ch_pow256(uint32_t k) {
    static constexpr uint32_t T[32][8] = {
        {0x4ffffffbu, 0xac96341cu, 0x9f60cd29u, 0x36fc7695u, 0x7879462eu, 0x666ea36fu, 0x9a07df2fu, 0x0e0a77c1u},
        {0x9ffffab6u, 0xf6e31f8cu, 0x31329faeu, 0x5d7570acu, 0x09e2a349u, 0x276f48b7u, 0xef86e357u, 0x0d791464u},
        {0x6ffab5b9u, 0x0f747098u, 0x703176adu, 0x4f0b4017u, 0xf7c3c787u, 0x5105616bu, 0x121feb95u, 0x0d42a313u},
        {0x5ab5b8bau, 0xe4a771fcu, 0xe8c1e556u, 0x0d0e939eu, 0x5a695dd6u, 0x9f6e5c10u, 0x8c59c9e8u, 0x07359fa8u},
        {0x15b8b9dau, 0x93e78865u, 0xb05ea154u, 0x16df2426u, 0x302ab839u, 0x1271b743u, 0xec6c226eu, 0x06bc037eu},
        {0xe8b9d9ddu, 0x9fa3d1dbu, 0xba46f0b7u, 0x600b64c7u, 0x7609245au, 0x3ebdbb3cu, 0xa259885eu, 0x1e4cc537u},
        {0xb9d9dc60u, 0x36985f72u, 0x330a5cd5u, 0xeaf39a6eu, 0x184d2026u, 0x8b8faa65u, 0x9a84442bu, 0x0e142fd5u},
        {0x79dc5fb6u, 0xf90e75f6u, 0xdac24b38u, 0x5499493fu, 0xddbc9bfdu, 0x48763e56u, 0x6bebdf7cu, 0x17312865u},
        {0x7c5fb586u, 0xb4c6edf9u, 0xbfeb93beu, 0x708c8d50u, 0x04f7e0efu, 0x9ffd1de4u, 0x9a392866u, 0x215b02acu},
        {0x5fb58550u, 0x1b9523c7u, 0x3c165ad6u, 0xe8dd9eecu, 0xeef42f64u, 0x45edf68bu, 0x670a49f1u, 0x160cbd9fu},
        {0xf5854f8cu, 0xd2c08056u, 0xee53d448u, 0xa619ab64u, 0x45935ab2u, 0x6996f53cu, 0xffcd5e5eu, 0x1f4a1358u},
        {0xd54f8b5bu, 0xffdd0e9bu, 0xdf4ebb31u, 0x3036ae37u, 0x1afcbe9bu, 0xcb384da4u, 0xa8622385u, 0x196cc8f4u},
        {0xaf8b5a7au, 0x54c81065u, 0x97aa45f6u, 0x2b82a1efu, 0x330a5a6du, 0xbe492693u, 0x8229aff4u, 0x1847e486u},
        {0x8b5a7980u, 0xd7159bb7u, 0xcd8dadb2u, 0x68adcb5au, 0x49ae3e97u, 0x2103b7f2u, 0x90dfdfe2u, 0x15bd4d11u},
        {0x8a797f8du, 0x971a6616u, 0xdf602195u, 0x9e7a023eu, 0x8123e58fu, 0x37a8a14du, 0xb694ef63u, 0x003dd3f5u},
        {0x897f8cffu, 0xd68420f6u, 0xe6682505u, 0x51ce5696u, 0xa2643741u, 0xf05107cau, 0xb3bdc30du, 0x0d6fa743u},
        {0xef8cfeb9u, 0xb075da81u, 0xa5b6cd8cu, 0xa7f12accu, 0x7957bf7bu, 0x32c47504u, 0x48ffa25eu, 0x03d581d7u},
        {0xccfeb8ecu, 0x28335260u, 0x3450c157u, 0xcd1ca6fcu, 0x39a49460u, 0x5e2f9237u, 0x67c1daf0u, 0x0dabb64fu},
        {0x7eb8ebb8u, 0x1bc54f31u, 0x1499ae4du, 0xce0da7d2u, 0x38338699u, 0x58fe9be5u, 0x6be5e4a2u, 0x0f803f18u},
        {0xd8ebb7aeu, 0x06ee881bu, 0x9c483e94u, 0x2d076addu, 0xb8184bf7u, 0xf4e590c2u, 0xc3ff54fbu, 0x001df79fu},
        {0xebb7ae00u, 0xee881bd8u, 0x483e9406u, 0x076add9cu, 0x184bf72du, 0xe590c2b8u, 0xff54fbf4u, 0x1df79fc3u},
        {0x97adff62u, 0xa2a6479du, 0x1e208d46u, 0x9ad43f8du, 0x5e22a388u, 0xcf37b174u, 0x585b1b25u, 0x19b75918u},
        {0x2dff6178u, 0x963d2700u, 0x76097976u, 0x78ac269du, 0x55ec971du, 0x4d0c6b69u, 0xb8be0fa5u, 0x020f6b50u},
        {0x9f6177f6u, 0x96536866u, 0x483b10e9u, 0x1a1f8aa1u, 0xdd89a9d5u, 0xd948b034u, 0xf21f63abu, 0x2b80403bu},
        {0xc177f51au, 0x5665c3b5u, 0xde75c713u, 0x00e7f02au, 0x2f747168u, 0xb09192e5u, 0xcccdc65du, 0x0621c0bbu},
        {0x77f519e0u, 0xe9850343u, 0x3e99012du, 0xe17321cfu, 0x44465c5bu, 0x878a2e5fu, 0xa7925879u, 0x1536ed70u},
        {0xf519df90u, 0xd227d2beu, 0x57dfee5bu, 0xdc6c2f89u, 0x9dc5b31fu, 0xe70fdf6bu, 0x0ca26746u, 0x0b0b1e65u},
        {0xb9df8fc6u, 0xc6a11b70u, 0x4beadae8u, 0x506ce8ecu, 0x6e651ac1u, 0x4dafa044u, 0x9d28fd73u, 0x14649f05u},
        {0x8f8fc595u, 0x41a9cbe4u, 0x0a58dc0fu, 0x9f36d601u, 0x440ad260u, 0xa6132126u, 0x093f81ddu, 0x2ab23b99u},
        {0x9fc5941fu, 0x00330d89u, 0x5ce01f95u, 0xe136d957u, 0x3823b6beu, 0x1493e0dcu, 0x52e418fbu, 0x2a12a611u},
        {0xa5941e22u, 0x551a9355u, 0x514ff707u, 0x59d5e883u, 0xd58c1e18u, 0xbe4467f3u, 0x9b1016e6u, 0x1baa09b3u},
        {0xb41e216eu, 0x63b54746u, 0xe434d47cu, 0xe84e09fbu, 0xb059b338u, 0x26a031bfu, 0xa1c98ef3u, 0x10d4f616u},
    };
    Fr r;
#pragma unroll
    for (int i = 0; i < 8; ++i) r.l[i] = T[k][i];
    return r;
}
ZK_BC_HD Fr ch_inv_small(uint32_t k) {
    static constexpr uint32_t T[31][8] = {
        {0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u},
        {0x4ffffffbu, 0xac96341cu, 0x9f60cd29u, 0x36fc7695u, 0x7879462eu, 0x666ea36fu, 0x9a07df2fu, 0x0e0a77c1u},
        {0x1ffffffeu, 0x783c14d8u, 0x0c8d1eddu, 0xaf982f6fu, 0xfcfd4f45u, 0x8f5f7492u, 0x3d9cbfacu, 0x1f37631au},
        {0x15555554u, 0xfad2b890u, 0x5db369e8u, 0x75101f9fu, 0x53538a2eu, 0xb4ea4db7u, 0xd3bdd51du, 0x14cf9766u},
        {0x0fffffffu, 0xbc1e0a6cu, 0x86468f6eu, 0xd7cc17b7u, 0x7e7ea7a2u, 0x47afba49u, 0x1ece5fd6u, 0x0f9bb18du},
        {0x09999999u, 0xd7453974u, 0x83c3efa8u, 0xb4ada7d4u, 0xe57f3161u, 0xc49ca2f8u, 0xac156cb3u, 0x162a3754u},
        {0x0aaaaaaau, 0x7d695c48u, 0xaed9b4f4u, 0x3a880fcfu, 0xa9a9c517u, 0xda7526dbu, 0x69deea8eu, 0x0a67cbb3u},
        {0x9db6db6du, 0xf4157528u, 0x847b8b05u, 0x07daec5eu, 0x7eecc0e2u, 0xea0fce34u, 0x83b7fb4fu, 0x02017ed2u},
        {0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x20000000u},
        {0x51c71c72u, 0x80dce13du, 0x1b0cc3aeu, 0xec7d5010u, 0xc77213a2u, 0x0c839db6u, 0x87605c7bu, 0x2732bc19u},
        {0xfccccccdu, 0x0d939783u, 0x7ebeb01du, 0x6e70c80eu, 0xb38044dfu, 0xbe767457u, 0xc6a3866eu, 0x234742e3u},
        {0x9e8ba2e9u, 0x9e265a3fu, 0xf2a6f027u, 0xf3b110cdu, 0x2351d247u, 0x1afe9ea6u, 0x6bf642f4u, 0x2478727cu},
        {0x05555555u, 0x3eb4ae24u, 0xd76cda7au, 0x9d4407e7u, 0xd4d4e28bu, 0x6d3a936du, 0xb4ef7547u, 0x0533e5d9u},
        {0xa13b13b1u, 0x7a2e512cu, 0xbc866fdeu, 0x80918f51u, 0x6bf5d7eau, 0xe9288d73u, 0xdfb97893u, 0x0886640cu},
        {0x46db6db7u, 0x9bfbb55eu, 0x7f1a7dcbu, 0x98076a53u, 0x80370c9fu, 0xd13009f5u, 0xb274cdbcu, 0x1932e6a2u},
        {0xfddddddeu, 0xb3b7ba57u, 0xa9d47568u, 0xf44b3009u, 0x77aad894u, 0xd44ef83au, 0x846d0449u, 0x1784d742u},
        {0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x10000000u},
        {0x45a5a5a6u, 0x9f7ced43u, 0xfdc8fa8du, 0x7799d982u, 0xa62da6b7u, 0xf5c1fa7cu, 0x5e89fc4au, 0x202366fbu},
        {0xa8e38e39u, 0x406e709eu, 0x0d8661d7u, 0x763ea808u, 0x63b909d1u, 0x8641cedbu, 0xc3b02e3du, 0x13995e0cu},
        {0x96bca1afu, 0x96f74503u, 0x80fdaadbu, 0xa8cf620fu, 0x64d0a134u, 0x84950277u, 0x55b4cbc3u, 0x05d536fbu},
        {0xf6666667u, 0x28bac68bu, 0x7c3c1057u, 0x4b52582bu, 0x1a80ce9eu, 0x3b635d07u, 0x53ea934cu, 0x29d5c8abu},
        {0xd9e79e7au, 0x12a7ce3eu, 0x54bc53ddu, 0x655a46e2u, 0x557a086au, 0xe0cab14eu, 0xcc4dde7du, 0x10cc99c1u},
        {0xc745d175u, 0x710427e9u, 0x3630305cu, 0x8df27c8bu, 0x52699552u, 0xe9a7722eu, 0xa693f18eu, 0x2a6e6077u},
        {0x6d37a6f5u, 0x61e5d21eu, 0xabb4038du, 0x696af1c6u, 0x3d69ea22u, 0x232bdc92u, 0x766aa596u, 0x117141e2u},
        {0xfaaaaaabu, 0xc14b51dbu, 0x28932585u, 0x62bbf818u, 0x2b2b1d74u, 0x92c56c92u, 0x4b108ab8u, 0x1acc1a26u},
        {0x5b851eb9u, 0x615c365au, 0x7bbb89fcu, 0xdde5db64u, 0x9580ea2au, 0x545f8b90u, 0x702bfc45u, 0x2b257d06u},
        {0x489d89d9u, 0xdf082360u, 0x1b1ff037u, 0xd462bbcdu, 0xf6bb9823u, 0xd0bc6994u, 0xe0758c5eu, 0x1c75593fu},
        {0x7097b426u, 0x2af44b14u, 0x0904413au, 0xf97f1ab0u, 0x427b5be0u, 0x59813492u, 0xd7cac97eu, 0x0d10e95du},
        {0x1b6db6dcu, 0x6feed579u, 0xfc69f72eu, 0x601da94du, 0x00dc327eu, 0x44c027d6u, 0xc9d336f3u, 0x24cb9a8au},
        {0xf8d3dcb1u, 0x2741fb53u, 0x8603ae0cu, 0x4fd0a5ebu, 0x42e1b4dau, 0x40f7d8a1u, 0x41a37cc3u, 0x1e853da6u},
        {0xfeeeeeefu, 0x59dbdd2bu, 0xd4ea3ab4u, 0x7a259804u, 0x3bd56c4au, 0xea277c1du, 0x42368224u, 0x0bc26ba1u},
    };
    Fr r;
#pragma unroll
    for (int i = 0; i < 8; ++i) r.l[i] = T[k][i];
    return r;
}

// ---- one row of the circuit ---------------------------------------------------------------------------------------------------------
struct ChRow {
    uint32_t control_length;            // mod 2^32, as the bytecode op's length
    uint32_t shift;                     // padding_shift = 256^shift
    uint32_t inv_of;                    // bytes_in_field_inv = 1 / inv_of, 0 where that is 0
    uint32_t m;                         // a byte row's position inside its field
    uint8_t bytes_in_field_index, is_field_border, field_index, field_index_inv;
};
// kind: BC_PAD, BC_HEADER or BC_BYTE; p: the position of the byte; len: L_b.  A padding row is a header row of length 0
// (set_header_row(region, 0, idx)), and a header row's field_index_inv is 0 although its field_index is 1: the reference's.
ZK_BC_HD ChRow ch_row(uint32_t kind, uint64_t p, uint64_t len) {
    ChRow r;
    if (kind != BC_BYTE) {
        r.control_length = kind == BC_HEADER ? (uint32_t)len : 0u;
        r.shift = CH_F, r.inv_of = 0, r.m = 0;
        r.bytes_in_field_index = 0, r.is_field_border = 0, r.field_index = 1, r.field_index_inv = 0;
        return r;
    }
    const uint32_t m = (uint32_t)(p % CH_F), second = (uint32_t)(p / CH_F & 1);
    r.control_length = (uint32_t)(len - CH_W * (p / CH_W));
    r.shift = CH_F - 1 - m, r.inv_of = CH_F - 1 - m, r.m = m;
    r.bytes_in_field_index = (uint8_t)(m + 1);
    r.is_field_border = (uint8_t)(m == CH_F - 1 || p + 1 == len);
    r.field_index = (uint8_t)(second + 1);
    r.field_index_inv = (uint8_t)(1 - second);                         // 1 / (2 - field_index), 0 where that is 0
    return r;
}

// ---- up to 31 bytes as one integer --------------------------------------------------------------------------------------------------
// The bytes bytes[at .. at + last], last <= 30, as sum_t bytes[at + t] 256^(30 - t): eight 32-bit limbs, not in Montgomery form.
// [lo, hi) is the bytecode the field lies in, lo <= at and at + last < hi: nothing outside it is read.  The bytes come as aligned
// dwords where a dword lies inside the bytecode, as single bytes at its two ends.
ZK_BC_HD Fr ch_field_int(const uint8_t* bytes, uint64_t lo, uint64_t hi, uint64_t at, uint32_t last) {
    const uintptr_t first = (uintptr_t)bytes + at, a0 = first & ~(uintptr_t)3, ok_lo = (uintptr_t)bytes + lo, ok_hi = (uintptr_t)bytes + hi;
    const uint32_t sh = (uint32_t)(first & 3), q_last = (sh + last) >> 2;           // at most (3 + 30) / 4 = 8
    uint32_t s[10];
#pragma unroll
    for (uint32_t q = 0; q < 9; ++q) {
        const uintptr_t a = a0 + 4 * q;
        uint32_t v = 0;
        if (q <= q_last) {
            if (a >= ok_lo && a + 4 <= ok_hi) v = *(const uint32_t*)a;
            else {
#pragma unroll
                for (uint32_t c = 0; c < 4; ++c)
                    if (a + c >= ok_lo && a + c < ok_hi) v |= (uint32_t)*(const uint8_t*)(a + c) << (8 * c);
            }
        }
        s[q] = v;
    }
    s[9] = 0;
    // y[7 - j]: the field's bytes 4 j .. 4 j + 3, big-endian, those behind `last` cleared (byte 31 is always behind it)
    uint32_t y[9];
#pragma unroll
    for (uint32_t j = 0; j < 8; ++j) {
        const uint32_t d = sh ? s[j] >> (8 * sh) | s[j + 1] << (32 - 8 * sh) : s[j];
        const uint32_t keep = last + 1 > 4 * j ? last + 1 - 4 * j : 0u;
        const uint32_t mask = keep >= 4 ? 0xffffffffu : (1u << (8 * keep)) - 1u;
        y[7 - j] = __builtin_bswap32(d & mask);
    }
    y[8] = 0;
    Fr r;                                                               // the 32-byte integer, a byte down
#pragma unroll
    for (uint32_t k = 0; k < 8; ++k) r.l[k] = y[k] >> 8 | y[k + 1] << 24;
    return r;
}

// field_input of byte row p (m = p mod 31) of the bytecode at [off, off + len)
ZK_BC_HD Fr ch_field_input(const uint8_t* bytes, uint64_t off, uint64_t len, uint64_t p, uint32_t m) {
    return to_mont(ch_field_int(bytes, off, off + len, off + p - m, m));
}

// ---- one row of the table -----------------------------------------------------------------------------------------------------------
// the table rows of a bytecode, and their sums: both saturate at cap = n.  An empty bytecode owns none.
ZK_BC_HD uint64_t ch_blocks_of(uint64_t len) { return len / CH_W + (len % CH_W ? 1u : 0u); }
ZK_BC_HD uint32_t ch_table_rows_of(uint64_t len, uint32_t cap) {
    const uint64_t k = ch_blocks_of(len);
    return k < cap ? (uint32_t)k : cap;
}
struct ChTableRow {
    uint64_t control_hi, cap;           // control = control_hi 2^64 (HASHABLE_DOMAIN_SPEC = 2^64): the low eight bytes of the cell are 0
    uint8_t heading_mark, kind;
};
// owned: the row belongs to a bytecode (of len bytes, as its block j); the rows behind the last bytecode are off
ZK_BC_HD ChTableRow ch_table_row(bool owned, uint64_t j, uint64_t len) {
    ChTableRow r;
    r.control_hi = owned ? len - CH_W * j : 0u;
    r.cap = owned ? len : 0u;
    r.heading_mark = (uint8_t)(owned && j == 0);
    r.kind = (uint8_t)(!owned ? CH_KIND_OFF : j ? CH_KIND_CONT : CH_KIND_HEAD);
    return r;
}
// input `which` (0 or 1) of block j: the field [62 j + 31 which, + 31), cut at len; zero where it begins at or behind len
ZK_BC_HD Fr ch_table_input(const uint8_t* bytes, uint64_t off, uint64_t len, uint64_t j, uint32_t which) {
    const uint64_t at = CH_W * j + CH_F * which;
    if (at >= len) return Fr::zero();
    const uint64_t left = len - at;
    return to_mont(ch_field_int(bytes, off, off + len, off + at, left < CH_F ? (uint32_t)left - 1 : CH_F - 1));
}

}  // namespace zk

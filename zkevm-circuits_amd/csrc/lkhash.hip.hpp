// The hash and the equality of the lookup hash join (csrc/lookup.hip: k_lk_insert, k_lk_count, the mock-verify probes) over the
// eight 32-bit limbs of a canonical Montgomery residue.  Host and device: tests/host_lkhash_harness.hip compiles this file for the
// host and tests/test_lkhash_host.py holds a pure-Python replica (tests/lookup_join_cases.py) to it, so that the test cases built
// with the replica -- values whose home slots collide, or wrap past the last slot -- are what they claim to be.
#pragma once
#include "ff.hip.hpp"

namespace zk {

__host__ __device__ __forceinline__ uint32_t fr_hash(const Fr& a) {
    uint32_t h = a.l[0];
#pragma unroll
    for (int i = 1; i < 8; ++i) h = (h ^ a.l[i]) * 0x9E3779B1u + (h >> 15);
    h ^= h >> 16; h *= 0x85EBCA6Bu; h ^= h >> 13; h *= 0xC2B2AE35u; h ^= h >> 16;   // murmur3 finaliser
    return h;
}
__host__ __device__ __forceinline__ bool fr_same(const Fr& a, const Fr& b) {
    uint32_t d = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) d |= a.l[i] ^ b.l[i];
    return d == 0;
}

}  // namespace zk

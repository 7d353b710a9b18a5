// xxh32.hpp -- XXH32, restated from the published specification (xxHash "XXH32 algorithm
// description": four-lane 16-B stripes for inputs of 16 B and more, the 4-B and 1-B tails,
// the avalanche), written once for the host and the device. The reference's partitioner is
// calculate_32(key) % partition_count with calculate_32 = XxHash32::oneshot(0, key)
// (core/common/src/utils/hash.rs:18-22).
//
// The input is read through a loader (u32(off): the little-endian word at byte `off`,
// u8(off): the byte), so the route kernel hashes keys at any byte address, or a key held
// in registers, and the host a plain pointer. No load passes the input's last byte.
// Pinned by tests/golden/xxh32_vectors.json (libxxhash 0.8.2).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define IGGY_XXH32_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define IGGY_XXH32_HD inline
#endif

namespace iggy {

constexpr uint32_t kX32P1 = 0x9E3779B1u, kX32P2 = 0x85EBCA77u, kX32P3 = 0xC2B2AE3Du, kX32P4 = 0x27D4EB2Fu,
                   kX32P5 = 0x165667B1u;

typedef uint32_t xxh32_u32_ua __attribute__((aligned(1), may_alias));

// bytes in memory, any alignment
struct Xxh32Mem {
    const uint8_t *p;
    IGGY_XXH32_HD uint32_t u32(uint64_t off) const { return *(const xxh32_u32_ua *)(p + off); }
    IGGY_XXH32_HD uint32_t u8(uint64_t off) const { return p[off]; }
};

// a 16-B little-endian value held in two registers (a message id: id_lo, id_hi)
struct Xxh32Reg128 {
    uint64_t lo, hi;
    IGGY_XXH32_HD uint32_t u32(uint64_t off) const { return (uint32_t)(((off & 8) ? hi : lo) >> (8 * (off & 4))); }
    IGGY_XXH32_HD uint32_t u8(uint64_t off) const { return (uint8_t)(((off & 8) ? hi : lo) >> (8 * (off & 7))); }
};

IGGY_XXH32_HD uint32_t xxh32_rotl(uint32_t x, uint32_t r) { return (x << r) | (x >> (32 - r)); }
IGGY_XXH32_HD uint32_t xxh32_round(uint32_t acc, uint32_t in) { return xxh32_rotl(acc + in * kX32P2, 13) * kX32P1; }

template <class Loader>
IGGY_XXH32_HD uint32_t xxh32(const Loader &in, uint64_t len, uint32_t seed) {
    uint64_t off = 0;
    uint32_t h;
    if (len >= 16) {
        uint32_t v1 = seed + kX32P1 + kX32P2, v2 = seed + kX32P2, v3 = seed, v4 = seed - kX32P1;
        for (; off + 16 <= len; off += 16) {
            v1 = xxh32_round(v1, in.u32(off));
            v2 = xxh32_round(v2, in.u32(off + 4));
            v3 = xxh32_round(v3, in.u32(off + 8));
            v4 = xxh32_round(v4, in.u32(off + 12));
        }
        h = xxh32_rotl(v1, 1) + xxh32_rotl(v2, 7) + xxh32_rotl(v3, 12) + xxh32_rotl(v4, 18);
    } else {
        h = seed + kX32P5;
    }
    h += (uint32_t)len;
    for (; off + 4 <= len; off += 4) h = xxh32_rotl(h + in.u32(off) * kX32P3, 17) * kX32P4;
    for (; off < len; ++off) h = xxh32_rotl(h + in.u8(off) * kX32P5, 11) * kX32P1;
    h ^= h >> 15;
    h *= kX32P2;
    h ^= h >> 13;
    h *= kX32P3;
    h ^= h >> 16;
    return h;
}

}  // namespace iggy

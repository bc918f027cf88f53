// crc_math.hpp -- the arithmetic of the pixel digests (include/llicti_hip.h, "PIXEL DIGESTS"): CRC-32 as zlib computes it, seen as polynomials
// over GF(2) modulo the reflected polynomial 0xEDB88320.  Plain C++17 with no HIP dependency, like host_types.hpp: the host compiles it for
// llicti_crc32_combine and for the tables a context uploads, the kernels of digest.hpp call the same functions.
//
// Representation: bit 31 of a word is the coefficient of x^0, bit 0 that of x^31 (zlib's), so x^0 = 0x80000000 and a multiplication by x is a
// right shift.  The RAW CRC of a message is its remainder with a zero initial register and no final complement.  For raw CRCs
//     raw(A || B) = raw(A) * x^(8 |B|)  xor  raw(B)
// and zero bytes IN FRONT of a message do not change it.  zlib's crc32 starts from an all-ones register and complements the result:
//     crc32(M) = raw(M)  xor  0xFFFFFFFF * x^(8 |M|)  xor  0xFFFFFFFF
// and crc32(A || B) = crc32(A) * x^(8 |B|) xor crc32(B) holds for the finished values too (the two complements' terms cancel): crc32_combine.
#pragma once
#include <stdint.h>

#include "host_types.hpp"

constexpr uint32_t kCrcPoly = 0xEDB88320u;
constexpr uint32_t kCrcOne = 0x80000000u;         // x^0

// The geometry of crc_planes_kernel (digest.hpp): a lane owns kCrcLanePixels consecutive pixels, a workgroup of kCrcThreads lanes
// kCrcGroupPixels; an image takes ceil(H W / kCrcGroupPixels) workgroups, at most kCrcMaxGroups (8160 x 8160).
constexpr int kCrcLanePixels = 32;
constexpr int kCrcThreads = 256;
constexpr int kCrcGroupPixels = kCrcLanePixels * kCrcThreads;
constexpr int kCrcMaxGroups = (8160 * 8160 + kCrcGroupPixels - 1) / kCrcGroupPixels;      // 8,129

// x * b
LLICTI_HD constexpr uint32_t gf2_mulx(uint32_t b) { return (b >> 1) ^ (kCrcPoly & (0u - (b & 1u))); }
// a * b mod P (branch-free: 32 steps whatever the operands)
LLICTI_HD constexpr uint32_t gf2_mul(uint32_t a, uint32_t b)
{
    uint32_t p = 0;
    for (int i = 31; i >= 0; --i) {
        p ^= b & (0u - ((a >> i) & 1u));
        b = gf2_mulx(b);
    }
    return p;
}
// the three colour planes' words times ONE factor: the factor's 32 shifts are shared
LLICTI_HD void gf2_mul3(uint32_t a[3], uint32_t b)
{
    uint32_t p0 = 0, p1 = 0, p2 = 0;
    for (int i = 31; i >= 0; --i) {
        p0 ^= b & (0u - ((a[0] >> i) & 1u));
        p1 ^= b & (0u - ((a[1] >> i) & 1u));
        p2 ^= b & (0u - ((a[2] >> i) & 1u));
        b = gf2_mulx(b);
    }
    a[0] = p0; a[1] = p1; a[2] = p2;
}
// x^(8 n) mod P: square and multiply over the bits of n (x has an order that divides 2^32 - 1, so any 64-bit n is fine)
LLICTI_HD constexpr uint32_t gf2_xpow8(uint64_t n)
{
    uint32_t p = kCrcOne, q = 0x00800000u;        // q = x^8
    while (n) {
        if (n & 1u) p = gf2_mul(p, q);
        q = gf2_mul(q, q);
        n >>= 1;
    }
    return p;
}
// crc32(A || B) from crc32(A), crc32(B) and |B| (zlib's crc32_combine); the same formula folds raw CRCs
LLICTI_HD constexpr uint32_t crc32_combine_pow(uint32_t crc_a, uint32_t crc_b, uint32_t xpow_b) { return gf2_mul(crc_a, xpow_b) ^ crc_b; }
LLICTI_HD constexpr uint32_t crc32_combine(uint32_t crc_a, uint32_t crc_b, uint64_t len_b) { return crc32_combine_pow(crc_a, crc_b, gf2_xpow8(len_b)); }
// zlib's crc32 of a message from its raw CRC and x^(8 |M|)
LLICTI_HD constexpr uint32_t crc32_finish(uint32_t raw, uint32_t xpow_len) { return raw ^ gf2_mul(0xFFFFFFFFu, xpow_len) ^ 0xFFFFFFFFu; }
// one byte into a raw or running CRC, bit by bit (the kernels build their 256-entry table from it: entry t = crc32_byte(0, t))
LLICTI_HD constexpr uint32_t crc32_byte(uint32_t crc, uint32_t byte)
{
    crc ^= byte & 0xFFu;
    for (int k = 0; k < 8; ++k) crc = gf2_mulx(crc);
    return crc;
}

// The shift constants of the equal-length runs: a lane's, a workgroup's
constexpr uint32_t kCrcXLane = gf2_xpow8(kCrcLanePixels);
constexpr uint32_t kCrcXGroup = gf2_xpow8(kCrcGroupPixels);
static_assert(crc32_finish(crc32_byte(0, 'a'), gf2_xpow8(1)) == 0xE8B7BE43u, "crc32(b\"a\")");
static_assert(crc32_combine(0xE8B7BE43u, 0x71BEEFF9u, 1) == 0x9E83486Du, "crc32(b\"ab\") from crc32(b\"a\"), crc32(b\"b\")");

// The tables of a context (one device buffer, filled by crc_fill_tables on the host):
//   [kCrcTabLane + m]   x^(8 kCrcLanePixels m), m < kCrcThreads: lane t of a workgroup multiplies its run's CRC by entry kCrcThreads - 1 - t
//   [kCrcTabPow + j]    x^(8 2^j), j < 32: the factors of x^(8 H W)
//   [kCrcTabGroup + m]  x^(8 kCrcGroupPixels m), m < kCrcMaxGroups: workgroup k of an image of n multiplies by entry n - 1 - k
constexpr int kCrcTabLane = 0, kCrcTabPow = kCrcThreads, kCrcTabGroup = kCrcThreads + 32, kCrcTabWords = kCrcTabGroup + kCrcMaxGroups;
static void crc_fill_tables(uint32_t *t)
{
    uint32_t v = kCrcOne;
    for (int m = 0; m < kCrcThreads; ++m) { t[kCrcTabLane + m] = v; v = gf2_mul(v, kCrcXLane); }
    v = 0x00800000u;
    for (int j = 0; j < 32; ++j) { t[kCrcTabPow + j] = v; v = gf2_mul(v, v); }
    v = kCrcOne;
    for (int m = 0; m < kCrcMaxGroups; ++m) { t[kCrcTabGroup + m] = v; v = gf2_mul(v, kCrcXGroup); }
}

// sanitize_digest_host.cpp -- the fold of llicti_amd/csrc/digest.hpp replayed on the host with crc_math.hpp (g++, no HIP; run under ASan + UBSan by
// tests/test_digest_cpu.py): lanes, groups and planes folded as the two kernels fold them, the ragged end in front, against a bytewise CRC-32.
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "../llicti_amd/csrc/crc_math.hpp"

static uint32_t ref_crc(const std::vector<uint8_t> &m)
{
    uint32_t c = 0xFFFFFFFFu;
    for (uint8_t b : m) c = crc32_byte(c, b);
    return c ^ 0xFFFFFFFFu;
}

int main()
{
    std::vector<uint32_t> tab(kCrcTabWords);
    crc_fill_tables(tab.data());
    const int L = kCrcLanePixels, G = kCrcGroupPixels, T = kCrcThreads;
    long sizes[] = { 1, 2, 3, 5, L - 1, L, L + 1, 2 * L + 1, G - 1, G, G + 1, 2 * G + L + 3, 67 * 93, 1024, 3 * G };
    int bad = 0;
    for (long plane : sizes) {
        std::vector<uint8_t> rgb(3 * plane);
        for (auto &v : rgb) v = (uint8_t)(rand() >> 7);
        const long groups = (plane + G - 1) / G, pad = groups * G - plane;
        uint32_t acc[3] = { 0, 0, 0 };
        for (long x = 0; x < groups; ++x) {
            uint32_t g[3] = { 0, 0, 0 };
            for (int t = 0; t < T; ++t) {
                uint32_t crc[3] = { 0, 0, 0 };
                for (int k = 0; k < L; ++k) {
                    const long v = x * G + (long)t * L + k;
                    if (v < pad) continue;
                    for (int c = 0; c < 3; ++c) crc[c] = crc32_byte(crc[c], rgb[c * plane + v - pad]);
                }
                gf2_mul3(crc, tab[kCrcTabLane + T - 1 - t]);
                for (int c = 0; c < 3; ++c) g[c] ^= crc[c];
            }
            gf2_mul3(g, tab[kCrcTabGroup + groups - 1 - x]);
            for (int c = 0; c < 3; ++c) acc[c] ^= g[c];
        }
        uint32_t xp = kCrcOne;
        for (int j = 0; j < 32; ++j) if ((plane >> j) & 1) xp = gf2_mul(xp, tab[kCrcTabPow + j]);
        const uint32_t xp2 = gf2_mul(xp, xp);
        const uint32_t raw = gf2_mul(acc[0], xp2) ^ gf2_mul(acc[1], xp) ^ acc[2];
        const uint32_t got = crc32_finish(raw, gf2_mul(xp2, xp)), want = ref_crc(rgb);
        if (got != want) { ++bad; printf("plane %ld: %08x != %08x\n", plane, got, want); }
    }
    // combine with a long len_b
    if (crc32_combine(0x12345678u, 0x9abcdef0u, (1ull << 32) + 5) != crc32_combine(crc32_combine(0x12345678u, 0, 1ull << 32), 0x9abcdef0u, 5)) { ++bad; printf("combine\n"); }
    printf(bad ? "FAIL\n" : "digest fold ok: %d sizes\n", (int)(sizeof sizes / sizeof sizes[0]));
    return bad;
}

// sanitize_progressive_host.cpp -- the table rules and the prefix arithmetic of progressive records (llicti_amd/csrc/progressive.hpp: the code
// the device check, the two copy kernels and llicti_progressive_prefix share) compiled by g++ alone.  What it holds:
//   - every record of the cases file (written by tests/test_progressive_cpu.py: the fixture's records, expected good with their prefix lengths,
//     and every malformed table, expected refused) gets its verdict from prog_check, from a heap block of EXACTLY the bytes given -- a read past
//     the table, or past a head cut short, is an AddressSanitizer report
//   - a good record's pieces (prog_piece), in dense order, tile the payload exactly once and add up to the prefix lengths
//   - random tables: valid ones pass with the prefix lengths a direct sum gives; with random words damaged, or cut short at any length, the
//     check returns a verdict without reading outside its block, and what it accepts tiles
// Under sanitizers:
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -o /tmp/sph tests/sanitize_progressive_host.cpp && /tmp/sph CASES
#include <stdio.h>
#include <stdlib.h>
#include <random>
#include <vector>

#include "../llicti_amd/csrc/progressive.hpp"

static long n_checks = 0;
#define REQUIRE(c)                                                                      \
    do {                                                                                \
        ++n_checks;                                                                     \
        if (!(c)) { fprintf(stderr, "FAILED %s (%s:%d)\n", #c, __FILE__, __LINE__); exit(1); } \
    } while (0)

// prog_check on an exact-size heap copy
static bool check_exact(const std::vector<uint8_t> &rec, int n_want, int L_want, long stride, ProgHead *h, int64_t *prefix)
{
    uint8_t *blk = (uint8_t *)malloc(rec.size() ? rec.size() : 1);
    memcpy(blk, rec.data(), rec.size());
    const bool ok = prog_check(blk, (long)rec.size(), n_want, L_want, stride, h, prefix);
    free(blk);
    return ok;
}

// the pieces of an accepted table tile [0, S) once, in an order whose running sums are the prefix lengths
static void pieces_tile(const std::vector<uint8_t> &rec, const ProgHead &h, const int64_t *prefix)
{
    long S = 0;
    for (int k = 0; k < h.n; ++k) { long v; REQUIRE(prog_seg(rec.data(), k, &v)); S += v; }
    REQUIRE(prefix[0] == h.T + S);
    std::vector<std::pair<long, long>> got;
    long dense = h.T;
    for (int r = h.L; r >= 0; --r) {
        const int i0 = r == h.L ? 0 : prog_piece_count(h, r + 1), i1 = prog_piece_count(h, r);
        for (int i = i0; i < i1; ++i) {
            long pay, len;
            prog_piece(rec.data(), h, S, i, &pay, &len);
            REQUIRE(len >= 0 && pay >= 0 && pay + len <= S);
            got.push_back({ pay, len });
            dense += len;
        }
        REQUIRE(dense == prefix[r]);
    }
    REQUIRE((int)got.size() <= kProgMaxPieces);
    std::sort(got.begin(), got.end());
    long at = 0;
    for (auto &p : got) { if (p.second == 0) continue; REQUIRE(p.first == at); at += p.second; }
    REQUIRE(at == S);
}

static void put32(std::vector<uint8_t> &v, size_t pos, uint32_t x) { for (int k = 0; k < 4; ++k) v[pos + k] = (uint8_t)(x >> (8 * k)); }

int main(int argc, char **argv)
{
    long n_good = 0, n_bad = 0;
    if (argc > 1) {
        FILE *f = fopen(argv[1], "rb");
        REQUIRE(f != nullptr);
        for (;;) {
            uint8_t expect;
            uint32_t len;
            int64_t want[LLICTI_NLEVELS + 1];
            if (fread(&expect, 1, 1, f) != 1) break;
            REQUIRE(fread(&len, 4, 1, f) == 1 && fread(want, sizeof want, 1, f) == 1);
            std::vector<uint8_t> rec(len);
            REQUIRE(len == 0 || fread(rec.data(), 1, len, f) == len);
            ProgHead h;
            int64_t prefix[LLICTI_NLEVELS + 1];
            const bool ok = check_exact(rec, 0, 0, -1, &h, prefix);
            REQUIRE(ok == (expect != 0));
            if (ok) {
                for (int r = 0; r <= LLICTI_NLEVELS; ++r) REQUIRE(prefix[r] == want[r]);
                pieces_tile(rec, h, prefix);
                std::vector<uint8_t> head(rec.begin(), rec.begin() + h.T);      // the table alone says the same
                int64_t p2[LLICTI_NLEVELS + 1];
                REQUIRE(check_exact(head, h.n, h.L, -1, &h, p2));
                for (int r = 0; r <= LLICTI_NLEVELS; ++r) REQUIRE(p2[r] == want[r]);
                REQUIRE(!check_exact(head, h.n == 49 ? 22 : 49, h.n == 49 ? 2 : 5, -1, &h, p2));      // the other model's context
                REQUIRE(!check_exact(head, 0, 0, prefix[0] - h.T - 1, &h, p2));                         // S above the stride
                ++n_good;
            } else ++n_bad;
        }
        fclose(f);
    }
    std::mt19937_64 rng(20240611);
    auto rnd = [&](long m) { return (long)(rng() % (uint64_t)m); };
    long n_rand = 0, n_damaged_ok = 0;
    for (int it = 0; it < 4000; ++it) {
        const bool A = rnd(2) == 0;
        const int n = A ? 49 : 22, L = A ? 5 : 2, M = 1 + (int)rnd(it % 7 == 0 ? 128 : 12);
        const long T = prog_table_bytes(n, L, M);
        std::vector<uint8_t> rec((size_t)T, 0);
        rec[0] = 'L'; rec[1] = 'L'; rec[2] = 'I'; rec[3] = 'P'; rec[4] = 1; rec[5] = (uint8_t)n; rec[6] = (uint8_t)L; rec[8] = (uint8_t)M; rec[9] = (uint8_t)(M >> 8);
        // streams with gaps between them; the payload's length spread over the segments
        long at = rnd(100), used = 0, lvl[LLICTI_NLEVELS] = { 0, 0, 0, 0, 0 };
        for (int m = 0; m < M; ++m) {
            const long len = rnd(3) == 0 ? 0 : rnd(it % 11 == 0 ? 40000000 : 5000);
            const size_t row = 12 + 4 * (size_t)n + 4 * (size_t)m * (L + 1);
            put32(rec, row, (uint32_t)at); put32(rec, row + 4, (uint32_t)len);
            std::vector<long> c(L + 1, 0);
            c[L] = len;
            for (int l = 1; l < L; ++l) c[l] = rnd(len + 1);
            std::sort(c.begin(), c.end());
            for (int l = 1; l < L; ++l) put32(rec, row + 4 + 4 * l, (uint32_t)c[l]);
            for (int l = 0; l < L; ++l) lvl[l] += c[l + 1] - c[l];
            used += len;
            at += len + (rnd(2) ? rnd(9) : 0);
        }
        long S = at + rnd(5), left = S;
        for (int k = 0; k < n; ++k) { const long v = k == n - 1 ? left : std::min(left, rnd(S / 3 + 2)); put32(rec, 12 + 4 * (size_t)k, (uint32_t)v); left -= v; }
        ProgHead h;
        int64_t prefix[LLICTI_NLEVELS + 1];
        REQUIRE(S < (1L << 31));
        REQUIRE(check_exact(rec, n, L, S, &h, prefix));
        long p = T + S - used;
        REQUIRE(prefix[L] == p);
        for (int r = L - 1; r >= 0; --r) { p += lvl[r]; REQUIRE(prefix[r] == p); }
        for (int r = L + 1; r <= LLICTI_NLEVELS; ++r) REQUIRE(prefix[r] == 0);
        pieces_tile(rec, h, prefix);
        ++n_rand;
        // damaged words, and every way of cutting the head short that changes a verdict
        for (int d = 0; d < 6; ++d) {
            std::vector<uint8_t> bad = rec;
            const int hits = 1 + (int)rnd(3);
            for (int k = 0; k < hits; ++k) {
                const size_t pos = (size_t)rnd(T);
                bad[pos] = rnd(3) == 0 ? (uint8_t)rnd(256) : (uint8_t)(bad[pos] ^ (1u << rnd(8)));
            }
            if (rnd(4) == 0) bad.resize((size_t)rnd(T + 1));
            if (check_exact(bad, 0, 0, -1, &h, prefix)) { pieces_tile(bad, h, prefix); ++n_damaged_ok; }
        }
    }
    printf("progressive tables ok: %ld good and %ld malformed records of the cases file, %ld random tables (%ld damaged ones still valid), %ld checks\n",
           n_good, n_bad, n_rand, n_damaged_ok, n_checks);
    return 0;
}

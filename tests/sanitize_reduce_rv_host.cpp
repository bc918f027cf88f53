// sanitize_reduce_rv_host.cpp -- the per-call schedule of the per-image-reduce decodes (llicti_amd/csrc/host_plan.hpp: admit_reduces,
// build_reduce_schedule, write_reduce_schedule) compiled by g++ alone and run under AddressSanitizer + UBSan by tests/test_reduce_per_image_cpu.py:
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -o /tmp/srv tests/sanitize_reduce_rv_host.cpp && /tmp/srv
// Over some thousands of seeded batches -- B 1 .. 40, sides 32 .. 700, one stream count for the call or one per image (what "auto" containers
// carry), both model depths, random reduces that include all-equal and none-zero -- it holds:
//   - every (level, band) tile list is exactly the tiles of the images with r_b <= lvl, once each, image-major (rows, then columns), and its
//     TileRun is choose_tile_form's over those images; levels below min(r) have no launch
//   - every level's stream list is exactly those images' streams, in the order of the plan's stream table
//   - the output table has reduced_dim(H_b, r_b) sizes (counted as numpy's [::2^r] counts them) and tight, disjoint offsets, or the caller's
//   - equal values r >= 1: the output table, max_rplane and pix_units are plan_add_reduced's (+ plan_add_pixels') at r, tight or placed
//   - every image active: build_tile_lists returns build_plan's lists and runs, and an all-zero schedule holds the same lists per (level, band)
//   - the tables fit the device block, apart and in bounds (the block is allocated to the byte: ASan sees a write past it)
//   - the refusals: a null array, a value out of range, differing values with a reference-format container -- each names the image
#include <stdio.h>
#include <stdlib.h>
#include <random>

#include "../llicti_amd/csrc/host_plan.hpp"

static long n_checks = 0;
#define REQUIRE(c)                                                                      \
    do {                                                                                \
        ++n_checks;                                                                     \
        if (!(c)) { fprintf(stderr, "FAILED %s (%s:%d)\n", #c, __FILE__, __LINE__); exit(1); } \
    } while (0)

static long n_batches = 0, n_equal = 0, n_nonzero = 0, n_scalar_twin = 0, n_tile_twin = 0;

static void drive(int B, const int *Hs, const int *Ws, int ME, const int *Ms, int nlev, bool ragged, const int *rv, bool placed, int n_cu, int tile_rows)
{
    ++n_batches;
    Plan p;
    build_plan(p, PlanSpec{ B, Hs, Ws, ME, Ms, nlev, ragged, nullptr, n_cu, tile_rows });
    REQUIRE(admit_reduces("test", B, rv, nlev, ME) == 0);
    std::vector<size_t> off(B);
    { size_t pos = 7; for (int b = 0; b < B; ++b) { off[b] = pos; pos += 3 * (size_t)reduced_dim(Hs[b], rv[b]) * reduced_dim(Ws[b], rv[b]) + 5; } }
    ReduceSchedule q;
    build_reduce_schedule(q, p, rv, placed ? off.data() : nullptr, n_cu, tile_rows);
    int rmin = nlev;
    for (int b = 0; b < B; ++b) rmin = std::min(rmin, rv[b]);
    if (reduces_equal(B, rv)) ++n_equal;
    if (rmin > 0) ++n_nonzero;
    REQUIRE(q.B == B && q.nlev == nlev && q.rmin == rmin && (int)q.r.size() == B && (int)q.red.size() == B);
    // the output table
    long pos = 0, max_rplane = 0;
    for (int b = 0; b < B; ++b) {
        REQUIRE(q.r[b] == rv[b]);
        int hr = 0, wr = 0;
        for (int i = 0; i < Hs[b]; i += 1 << rv[b]) ++hr;      // the rows / columns [::2^r] keeps
        for (int j = 0; j < Ws[b]; j += 1 << rv[b]) ++wr;
        REQUIRE(q.red[b].Hr == hr && q.red[b].Wr == wr);
        REQUIRE(((hr - 1) << rv[b]) < Hs[b] && ((wr - 1) << rv[b]) < Ws[b]);      // the last pixel read lies inside the plane
        REQUIRE(q.red[b].off == (placed ? (long)off[b] : pos));                   // tight: each block starts where the last one ended
        pos += 3L * hr * wr;
        max_rplane = std::max(max_rplane, (long)hr * wr);
    }
    REQUIRE(q.max_rplane == max_rplane);
    // equal values r >= 1: the table, max_rplane and pix_units are those of the scalar call's plan (plan_add_reduced + plan_add_pixels at r)
    if (reduces_equal(B, rv) && rv[0] >= 1) {
        ++n_scalar_twin;
        Plan ps;
        build_plan(ps, PlanSpec{ B, Hs, Ws, ME, Ms, nlev, ragged, nullptr, n_cu, tile_rows });
        plan_add_reduced(ps, rv[0], placed ? off.data() : nullptr);
        std::vector<int> Hw(B), Ww(B);
        for (int b = 0; b < B; ++b) { Hw[b] = reduced_dim(Hs[b], rv[0]); Ww[b] = reduced_dim(Ws[b], rv[0]); }
        std::vector<PixGeo> pix;
        REQUIRE(resolve_pixels("test", B, Hw.data(), Ww.data(), LLICTI_PIX_RGB8, nullptr, nullptr, pix) == 0);
        plan_add_pixels(ps, pix);
        REQUIRE((int)ps.red.size() == B && ps.max_rplane == q.max_rplane && ps.pix_units == q.pix_units);
        for (int b = 0; b < B; ++b) REQUIRE(ps.red[b].off == q.red[b].off && ps.red[b].Hr == q.red[b].Hr && ps.red[b].Wr == q.red[b].Wr);
    }
    // every image active: the shared tile-list builder returns build_plan's lists and runs exactly (a mixed-size plan has them)
    if (!p.uniform) {
        ++n_tile_twin;
        std::vector<TileRef> tiles;
        TileRun run[LLICTI_NLEVELS * 3];
        build_tile_lists(p.geo, B, 0, nlev, [](int, int) { return true; }, n_cu, tile_rows, tiles, run);
        REQUIRE(tiles.size() == p.tiles.size());
        for (size_t k = 0; k < tiles.size(); ++k) REQUIRE(tiles[k].img == p.tiles[k].img && tiles[k].yx == p.tiles[k].yx);
        for (int k = 0; k < LLICTI_NLEVELS * 3; ++k)
            REQUIRE(run[k].off == p.run[k].off && run[k].n_tiles == p.run[k].n_tiles && run[k].TH == p.run[k].TH && run[k].gx == p.run[k].gx);
        // ... and at all-zero reduces the schedule's lists are the plan's, level by level (the schedule walks the levels downwards)
        const std::vector<int> zero(B, 0);
        ReduceSchedule qz;
        build_reduce_schedule(qz, p, zero.data(), nullptr, n_cu, tile_rows);
        REQUIRE(qz.tiles.size() == p.tiles.size());
        for (int k = 0; k < nlev * 3; ++k) {
            REQUIRE(qz.run[k].n_tiles == p.run[k].n_tiles && qz.run[k].TH == p.run[k].TH && qz.run[k].gx == p.run[k].gx);
            for (int i = 0; i < p.run[k].n_tiles; ++i)
                REQUIRE(qz.tiles[qz.run[k].off + i].img == p.tiles[p.run[k].off + i].img && qz.tiles[qz.run[k].off + i].yx == p.tiles[p.run[k].off + i].yx);
        }
    }
    // streams and tiles, level by level
    size_t s_total = 0, t_total = 0;
    for (int lvl = 0; lvl < LLICTI_NLEVELS; ++lvl) {
        const bool runs = lvl < nlev && lvl >= rmin;
        std::vector<int> want;
        if (runs) for (int i = 0; i < p.nstreams; ++i) if (rv[p.sref[(size_t)i].b] <= lvl) want.push_back(i);
        REQUIRE(q.s_n[lvl] == (int)want.size());
        if (runs) {
            REQUIRE(!want.empty() || p.M == 0);
            REQUIRE(q.s_off[lvl] + want.size() <= q.streams.size());
            for (size_t k = 0; k < want.size(); ++k) REQUIRE(q.streams[q.s_off[lvl] + k] == want[k]);
        }
        s_total += want.size();
        for (int band = 0; band < 3; ++band) {
            const TileRun &r = q.run[lvl * 3 + band];
            if (!runs) { REQUIRE(r.n_tiles == 0); continue; }
            const Geom *gl = &p.geo[(size_t)lvl * B];
            auto count = [&](int th) -> long {
                long t = 0;
                for (int b = 0; b < B; ++b) if (rv[b] <= lvl) t += (long)((gl[b].w + kTileW - 1) / kTileW) * ((gl[b].h + th - 1) / th);
                return t;
            };
            const TileForm f = choose_tile_form(n_cu, tile_rows, band, count);
            REQUIRE(r.TH == f.TH && r.gx == f.gx && r.n_tiles == (int)f.n_tiles && r.n_tiles == (int)count(r.TH));
            REQUIRE(r.TH == kTileHMax || r.TH == kTileHMid || r.TH == kTileHSmall);
            REQUIRE(r.gx >= 1 && r.gx <= r.n_tiles && r.off + (size_t)r.n_tiles <= q.tiles.size());
            size_t k = r.off;
            for (int b = 0; b < B; ++b) {
                if (rv[b] > lvl) continue;
                const int tx_n = (gl[b].w + kTileW - 1) / kTileW, ty_n = (gl[b].h + r.TH - 1) / r.TH;
                for (int ty = 0; ty < ty_n; ++ty)
                    for (int tx = 0; tx < tx_n; ++tx, ++k) REQUIRE(q.tiles[k].img == b && q.tiles[k].yx == ((ty << 16) | tx));
            }
            REQUIRE(k == r.off + (size_t)r.n_tiles);
            t_total += (size_t)r.n_tiles;
        }
    }
    REQUIRE(q.streams.size() == s_total && q.tiles.size() == t_total);
    // the device block: the tables apart, in order, inside it
    REQUIRE(q.d_r % 256 == 0 && q.d_red % 256 == 0 && q.d_streams % 256 == 0 && q.d_tiles % 256 == 0 && q.d_pix % 256 == 0);
    REQUIRE(q.d_r + B * sizeof(int) <= q.d_red && q.d_red + B * sizeof(RedGeo) <= q.d_streams);
    REQUIRE(q.d_streams + q.streams.size() * sizeof(int) <= q.d_tiles && q.d_tiles + q.tiles.size() * sizeof(TileRef) <= q.d_pix);
    REQUIRE(q.d_pix + q.pix.size() * sizeof(PixGeo) <= q.d_total);
    std::vector<uint8_t> blk(q.d_total);
    write_reduce_schedule(q, blk.data());
    REQUIRE(memcmp(blk.data() + q.d_r, rv, B * sizeof(int)) == 0);
    if (!q.tiles.empty()) REQUIRE(memcmp(blk.data() + q.d_tiles, q.tiles.data(), q.tiles.size() * sizeof(TileRef)) == 0);
    // the pixel call's windows ride in the same block
    if (n_batches % 16 == 0) {
        std::vector<int> Hw(B), Ww(B);
        for (int b = 0; b < B; ++b) { Hw[b] = q.red[b].Hr; Ww[b] = q.red[b].Wr; }
        std::vector<PixGeo> pix;
        REQUIRE(resolve_pixels("test", B, Hw.data(), Ww.data(), LLICTI_PIX_BGRA8, nullptr, nullptr, pix) == 0);
        ReduceSchedule qp;
        build_reduce_schedule(qp, p, rv, nullptr, n_cu, tile_rows, &pix);
        long units = 0;
        for (int b = 0; b < B; ++b) units = std::max(units, (long)Hw[b] * ((Ww[b] + 3) / 4));
        REQUIRE((int)qp.pix.size() == B && qp.pix_units == units && qp.d_pix + B * sizeof(PixGeo) <= qp.d_total && qp.tiles.size() == q.tiles.size());
        std::vector<uint8_t> blk2(qp.d_total);
        write_reduce_schedule(qp, blk2.data());
    }
}

static bool last_error_names(int b)
{
    char want[32];
    snprintf(want, sizeof want, "image %d", b);
    return g_err.find(want) != std::string::npos;
}

static void refusals()
{
    const int rv[4] = { 0, 2, 5, 1 };
    REQUIRE(admit_reduces("t", 4, nullptr, 5, 8) == LLICTI_EINVAL);
    REQUIRE(admit_reduces("t", 4, rv, 5, 8) == 0);
    REQUIRE(admit_reduces("t", 4, rv, 5, 10 | 0x200) == 0);
    REQUIRE(admit_reduces("t", 4, rv, 2, 9 | 0x200) == LLICTI_EINVAL && last_error_names(2));       // 5 > config B's 2 levels
    REQUIRE(admit_reduces("t", 4, rv, 5, 0) == LLICTI_EINVAL && last_error_names(1));               // reference format, values differ
    const int eq[3] = { 3, 3, 3 };
    REQUIRE(admit_reduces("t", 3, eq, 5, 0) == 0 && reduces_equal(3, eq) && !reduces_equal(4, rv));  // ... all equal: the scalar call
    for (int bad : { -1, 6, 1 << 30, -(1 << 30) }) {
        for (int at = 0; at < 4; ++at) {
            int v[4] = { 1, 1, 1, 1 };
            v[at] = bad;
            REQUIRE(admit_reduces("t", 4, v, 5, 8) == LLICTI_EINVAL && last_error_names(at));
        }
    }
    const int one[1] = { 4 };
    REQUIRE(admit_reduces("t", 1, one, 5, 0) == 0 && reduces_equal(1, one));
}

int main()
{
    refusals();
    std::mt19937 rng(20261020u);
    auto rnd = [&](int lo, int hi) { return lo + (int)(rng() % (uint32_t)(hi - lo + 1)); };
    for (int it = 0; it < 2400; ++it) {
        const int nlev = (it % 4 == 3) ? kLevelsB : LLICTI_NLEVELS;
        const int B = (it % 7 == 0) ? rnd(1, 40) : rnd(1, 9);
        const int hi = (it % 5 == 0) ? 700 : 200;
        std::vector<int> Hs(B), Ws(B), Ms(B), rv(B);
        const bool equal_sizes = it % 6 == 1;
        for (int b = 0; b < B; ++b) { Hs[b] = (equal_sizes && b) ? Hs[0] : rnd(32, hi); Ws[b] = (equal_sizes && b) ? Ws[0] : rnd(32, hi); }
        // lane kind and counts: config B takes xwide streams only, at most 18 per image
        const int kind = nlev == kLevelsB ? 2 : rnd(0, 2);
        const int top = nlev == kLevelsB ? 18 : kind == 1 ? 14 : 32;
        const bool per_image = it % 3 == 0;
        for (int b = 0; b < B; ++b) Ms[b] = rnd(1, top);
        const int ME = Ms[0] | (kind << 8);
        // reduces: random, all equal, none zero, two values only
        const int pat = it % 8;
        const int base = rnd(0, nlev);
        for (int b = 0; b < B; ++b)
            rv[b] = pat == 0 ? base : pat == 1 ? rnd(1, nlev) : pat == 2 ? (rnd(0, 1) ? 0 : nlev) : rnd(0, nlev);
        const int n_cu = (it % 9 == 0) ? 32 : 256;
        const int tile_rows = (it % 11 == 0) ? 4 : (it % 13 == 0) ? 16 : 0;
        drive(B, Hs.data(), Ws.data(), ME, per_image ? Ms.data() : nullptr, nlev, !equal_sizes && it % 2 == 0, rv.data(), it % 10 == 0, n_cu, tile_rows);
    }
    REQUIRE(n_equal > 100 && n_nonzero > 100 && n_scalar_twin > 100 && n_tile_twin > 100);
    printf("per-image reduce schedules ok: %ld batches (%ld all equal, %ld without a level-0 image), %ld checks\n", n_batches, n_equal, n_nonzero, n_checks);
    return 0;
}

// sanitize_px_host.cpp -- the host plan of a call on interleaved, pitched pixels (llicti_amd/csrc/host_plan.hpp: resolve_pixels, pixel_key_tail,
// plan_add_pixels, pix_window_span) compiled by g++ alone, beside tests/sanitize_host.cpp and tests/sanitize_reduced_host.cpp.  What it holds:
//   - a pixel plan is the batch's tightly placed planar plan (with plan_add_reduced's table for a reduced decode) in every field the stages read:
//     only the key, the window table and the device block's size differ
//   - its key differs with the pitch, the offset, the format and the reduce of the call, and equals no planar or reduced key of the same batch
//   - the window table: default placement back to back, each window of its own span; a short pitch and an unknown format are refused
// tests/test_pixel_formats_cpu.py builds it plain; under sanitizers:
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -o /tmp/sph tests/sanitize_px_host.cpp && /tmp/sph
#include <stdio.h>
#include <stdlib.h>
#include <set>

#include "../llicti_amd/csrc/host_plan.hpp"

static long n_checks = 0;
#define REQUIRE(c)                                                                      \
    do {                                                                                \
        ++n_checks;                                                                     \
        if (!(c)) { fprintf(stderr, "FAILED %s (%s:%d)\n", #c, __FILE__, __LINE__); exit(1); } \
    } while (0)

static const int kFormats[] = { LLICTI_PIX_RGB8, LLICTI_PIX_BGR8, LLICTI_PIX_RGBA8, LLICTI_PIX_BGRA8 };

// the plan get_plan builds for a pixel call, and the key it looks it up with
static Plan pixel_plan(int B, const int *Hs, const int *Ws, int ME, int nlev, bool ragged, int reduce, int fmt, const size_t *off, const size_t *pitch,
                       std::vector<long> *lookup)
{
    std::vector<int> Hw(B), Ww(B);
    for (int b = 0; b < B; ++b) { Hw[b] = reduced_dim(Hs[b], reduce); Ww[b] = reduced_dim(Ws[b], reduce); }
    std::vector<PixGeo> pix;
    REQUIRE(resolve_pixels("test", B, Hw.data(), Ww.data(), fmt, off, pitch, pix) == 0);
    Plan p;
    build_plan(p, PlanSpec{ B, Hs, Ws, ME, nullptr, nlev, ragged });
    *lookup = p.key;
    if (reduce > 0) { plan_add_reduced(p, reduce, nullptr); reduced_key_tail(*lookup, B, Hs, Ws, reduce, nullptr); }
    plan_add_pixels(p, pix);
    pixel_key_tail(*lookup, pix);
    return p;
}

static void drive(int B, const int *Hs, const int *Ws, int ME, int nlev, bool ragged)
{
    Plan full;
    build_plan(full, PlanSpec{ B, Hs, Ws, ME, nullptr, nlev, ragged });
    std::set<std::vector<long>> keys = { full.key };
    for (int r = 1; r <= nlev; ++r) {
        Plan red;
        build_plan(red, PlanSpec{ B, Hs, Ws, ME, nullptr, nlev, ragged });
        plan_add_reduced(red, r, nullptr);
        REQUIRE(keys.insert(red.key).second);
    }
    for (int r = 0; r <= nlev; r += (r == 1 && nlev > 2) ? nlev - 1 : 1) {            // 0, 1, the model's maximum
        for (int fmt : kFormats) {
            const int bpp = pix_format_bytes(fmt);
            REQUIRE(bpp == (fmt >= LLICTI_PIX_RGBA8 ? 4 : 3));
            std::vector<size_t> tight(B), padded(B), off_a(B), off_b(B);
            size_t pos = 3;
            for (int b = 0; b < B; ++b) {
                const int Hw = reduced_dim(Hs[b], r), Ww = reduced_dim(Ws[b], r);
                tight[b] = (size_t)Ww * bpp;
                padded[b] = (tight[b] / 256 + 1) * 256 + (b & 1);         // (always longer than the row)
                off_a[b] = pos;
                off_b[b] = pos + 1;
                pos += (size_t)Hw * padded[b] + 5;
            }
            struct { const size_t *off, *pitch; } calls[] = { { nullptr, nullptr }, { nullptr, padded.data() }, { off_a.data(), padded.data() },
                                                             { off_b.data(), padded.data() }, { off_a.data(), tight.data() } };
            int n_call = 0;
            for (const auto &cl : calls) {
                std::vector<long> lookup;
                Plan p = pixel_plan(B, Hs, Ws, ME, nlev, ragged, r, fmt, cl.off, cl.pitch, &lookup);
                REQUIRE(p.key == lookup);                           // the key the cache looks up is the key the plan carries
                // different pitches, offsets, formats and reduces: different keys; none is a planar or a reduced key.  (The default placement with
                // explicit tight pitches is the one pair of calls that names the same windows -- not driven here.)
                REQUIRE(keys.insert(p.key).second);
                // every planar field is the planar plan's
                REQUIRE(p.uniform == full.uniform && p.vec_ok == full.vec_ok && p.rgb_bytes == full.rgb_bytes && p.max_plane == full.max_plane);
                REQUIRE(p.total == full.total && p.off_planes == full.off_planes && p.off_fplanes == full.off_fplanes && p.off_params == full.off_params);
                REQUIRE(p.off_slots == full.off_slots && p.off_status == full.off_status && p.nstreams == full.nstreams && p.M == full.M);
                REQUIRE(p.tiles.size() == full.tiles.size() && p.d_sref == full.d_sref && p.d_img == full.d_img && p.d_tiles == full.d_tiles);
                for (int b = 0; b < B; ++b) REQUIRE(p.img[b].rgb_off == full.img[b].rgb_off && p.img[b].pix_off == full.img[b].pix_off);
                // the window table, behind every other table
                REQUIRE((int)p.pix.size() == B && p.reduce == r);
                const size_t behind = r ? p.d_red + B * sizeof(RedGeo) : full.d_total;
                REQUIRE(p.d_pix >= behind && p.d_pix % 256 == 0 && p.d_total >= p.d_pix + B * sizeof(PixGeo) && p.d_total % 256 == 0);
                long next = 0, units = 0;
                for (int b = 0; b < B; ++b) {
                    const int Hw = reduced_dim(Hs[b], r), Ww = reduced_dim(Ws[b], r);
                    const PixGeo &pg = p.pix[b];
                    const size_t pt = cl.pitch ? cl.pitch[b] : tight[b];
                    REQUIRE(pg.fmt == fmt && pg.pitch == (int)pt && pg.pitch >= Ww * bpp);
                    REQUIRE(pg.off == (cl.off ? (long)cl.off[b] : next));
                    const size_t span = pix_window_span(fmt, Hw, Ww, pt);
                    REQUIRE(span == (size_t)(Hw - 1) * pt + (size_t)Ww * bpp);
                    next += (long)span;                              // (default placement: the next window starts where this one ends)
                    units = std::max(units, (long)Hw * ((Ww + 3) / 4));
                }
                REQUIRE(p.pix_units == units);
                ++n_call;
            }
            REQUIRE(n_call == 5);
            // refused: a pitch one byte short of a row (image 0, and the last image alone), an unknown format
            std::vector<PixGeo> pix;
            std::vector<int> Hw(B), Ww(B);
            for (int b = 0; b < B; ++b) { Hw[b] = reduced_dim(Hs[b], r); Ww[b] = reduced_dim(Ws[b], r); }
            std::vector<size_t> bad = tight;
            bad[0] -= 1;
            REQUIRE(resolve_pixels("test", B, Hw.data(), Ww.data(), fmt, nullptr, bad.data(), pix) == LLICTI_EINVAL);
            bad = tight;
            bad[B - 1] -= 1;
            REQUIRE(resolve_pixels("test", B, Hw.data(), Ww.data(), fmt, off_a.data(), bad.data(), pix) == LLICTI_EINVAL);
            bad[B - 1] = (size_t)1 << 31;
            REQUIRE(resolve_pixels("test", B, Hw.data(), Ww.data(), fmt, nullptr, bad.data(), pix) == LLICTI_EINVAL);
        }
        std::vector<PixGeo> pix;
        for (int fmt : { -1, 4, 255 }) REQUIRE(resolve_pixels("test", B, Hs, Ws, fmt, nullptr, nullptr, pix) == LLICTI_EINVAL && pix_format_bytes(fmt) == 0);
    }
    REQUIRE(full.pix.empty() && full.d_pix == 0);
}

int main()
{
    REQUIRE(pix_window_span(LLICTI_PIX_RGB8, 512, 768, 0) == 512u * 768u * 3u && pix_window_span(LLICTI_PIX_BGRA8, 2, 5, 32) == 32u + 20u);
    REQUIRE(pix_window_span(LLICTI_PIX_RGB8, 4, 5, 14) == 0 && pix_window_span(7, 4, 5, 0) == 0 && pix_window_span(LLICTI_PIX_RGB8, 0, 5, 0) == 0);
    const int modes[] = { 0, 8, 10 | 0x200 };
    const int sizes[][2] = { { 32, 32 }, { 33, 35 }, { 67, 93 }, { 64, 96 }, { 768, 512 }, { 8160, 8160 } };
    for (int ME : modes)
        for (const auto &hw : sizes)
            for (int B : { 1, 3 }) {
                if (hw[0] == 8160 && B > 1) continue;
                std::vector<int> Hs(B, hw[0]), Ws(B, hw[1]);
                drive(B, Hs.data(), Ws.data(), ME, LLICTI_NLEVELS, false);
                if (ME) drive(B, Hs.data(), Ws.data(), ME, LLICTI_NLEVELS, true);
            }
    for (int ME : { 0, 9 | 0x200 })                                // config B
        for (const auto &hw : sizes) {
            if (hw[0] > 1020 || hw[1] > 1020) continue;
            std::vector<int> Hs(2, hw[0]), Ws(2, hw[1]);
            drive(2, Hs.data(), Ws.data(), ME, kLevelsB, false);
        }
    {   // mixed sizes
        const int Hs[] = { 64, 33, 67, 512 }, Ws[] = { 96, 35, 93, 512 };
        drive(4, Hs, Ws, 6 | 0x200, LLICTI_NLEVELS, false);
        drive(4, Hs, Ws, 2, LLICTI_NLEVELS, false);
    }
    printf("pixel plans ok: %ld checks\n", n_checks);
    return 0;
}

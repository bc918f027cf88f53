// sanitize_reduced_host.cpp -- the host plan of a reduced-resolution decode (llicti_amd/csrc/host_plan.hpp: plan_add_reduced, reduced_key_tail)
// compiled by g++ alone, beside tests/sanitize_host.cpp (which drives the full-size plans).  What it holds:
//   - a reduced plan is the batch's full-size, tightly placed plan in every field the decode's stages read (workspace carving, uniform, vec_ok,
//     rgb_bytes, per-image tables): only the key, the output table and the device block's size differ
//   - its key equals no full-size key of the same batch (tight or explicit placement) and no reduced key of another r or placement
//   - the output table: sizes ceil(H / 2^r) x ceil(W / 2^r), blocks disjoint when tightly packed, inside the device block
// tests/test_reduced_cpu.py builds it plain; under sanitizers:
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -o /tmp/srh tests/sanitize_reduced_host.cpp && /tmp/srh
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

static void drive(int B, const int *Hs, const int *Ws, int ME, int nlev, bool ragged)
{
    Plan full;
    build_plan(full, PlanSpec{ B, Hs, Ws, ME, nullptr, nlev, ragged });
    std::vector<size_t> loose(B);                     // an explicit full-size placement: a different full-size key
    { size_t pos = 64; for (int b = 0; b < B; ++b) { loose[b] = pos; pos += 3 * (size_t)Hs[b] * Ws[b] + 64; } }
    Plan full_loose;
    build_plan(full_loose, PlanSpec{ B, Hs, Ws, ME, nullptr, nlev, ragged, loose.data() });
    std::set<std::vector<long>> keys = { full.key, full_loose.key };
    REQUIRE(keys.size() == 2);
    for (int r = 1; r <= nlev; ++r) {
        for (int placed = 0; placed < 2; ++placed) {
            std::vector<size_t> off(B);
            { size_t pos = 16; for (int b = 0; b < B; ++b) { off[b] = pos; pos += 3 * (size_t)reduced_dim(Hs[b], r) * reduced_dim(Ws[b], r) + 16; } }
            Plan p;
            build_plan(p, PlanSpec{ B, Hs, Ws, ME, nullptr, nlev, ragged });
            plan_add_reduced(p, r, placed ? off.data() : nullptr);
            // the same key as the one the cache looks up
            std::vector<long> key = full.key;
            reduced_key_tail(key, B, Hs, Ws, r, placed ? off.data() : nullptr);
            REQUIRE(p.key == key);
            REQUIRE(keys.insert(p.key).second);       // new among the full-size keys and every reduced key so far
            // every full-size field is the full plan's
            REQUIRE(p.uniform == full.uniform && p.vec_ok == full.vec_ok && p.rgb_bytes == full.rgb_bytes && p.max_plane == full.max_plane);
            REQUIRE(p.total == full.total && p.off_planes == full.off_planes && p.off_fplanes == full.off_fplanes && p.off_params == full.off_params);
            REQUIRE(p.off_slots == full.off_slots && p.off_status == full.off_status && p.nstreams == full.nstreams && p.M == full.M);
            REQUIRE(p.tiles.size() == full.tiles.size() && p.d_sref == full.d_sref && p.d_img == full.d_img);
            for (int b = 0; b < B; ++b) REQUIRE(p.img[b].rgb_off == full.img[b].rgb_off && p.img[b].pix_off == full.img[b].pix_off);
            // the output table
            REQUIRE(p.reduce == r && (int)p.red.size() == B);
            REQUIRE(p.d_red == full.d_total && p.d_total >= p.d_red + B * sizeof(RedGeo) && p.d_total % 256 == 0);
            long pos = 0;
            for (int b = 0; b < B; ++b) {
                const RedGeo &rg = p.red[b];
                int hr = 0, wr = 0;
                for (int i = 0; i < Hs[b]; i += 1 << r) ++hr;      // the rows / columns [::2^r] keeps
                for (int j = 0; j < Ws[b]; j += 1 << r) ++wr;
                REQUIRE(rg.Hr == hr && rg.Wr == wr);
                REQUIRE(((rg.Hr - 1) << r) < Hs[b] && ((rg.Wr - 1) << r) < Ws[b]);      // the last pixel read lies inside the plane
                REQUIRE(rg.off == (placed ? (long)off[b] : pos));
                pos += 3L * hr * wr;
            }
        }
    }
    REQUIRE(full.reduce == 0 && full.red.empty());
}

int main()
{
    const int modes[] = { 0, 8, 4 | 0x100, 10 | 0x200, 24 | 0x200 };
    const int sizes[][2] = { { 64, 48 }, { 67, 93 }, { 33, 64 }, { 577, 768 }, { 768, 512 }, { 32, 32 }, { 8160, 8160 } };
    for (int ME : modes)
        for (const auto &hw : sizes)
            for (int B : { 1, 3 }) {
                if (hw[0] == 8160 && B > 1) continue;
                std::vector<int> Hs(B, hw[0]), Ws(B, hw[1]);
                drive(B, Hs.data(), Ws.data(), ME, LLICTI_NLEVELS, false);
                if (ME) drive(B, Hs.data(), Ws.data(), ME, LLICTI_NLEVELS, true);
            }
    // config B: the reference format and xwide v4 streams
    for (int ME : { 0, 9 | 0x200 })
        for (const auto &hw : sizes) {
            if (hw[0] > 1020 || hw[1] > 1020) continue;
            std::vector<int> Hs(2, hw[0]), Ws(2, hw[1]);
            drive(2, Hs.data(), Ws.data(), ME, kLevelsB, false);
        }
    // mixed sizes
    {
        const int Hs[] = { 321, 481, 768, 67, 512 }, Ws[] = { 481, 321, 512, 93, 512 };
        drive(5, Hs, Ws, 6 | 0x200, LLICTI_NLEVELS, false);
        drive(5, Hs, Ws, 2, LLICTI_NLEVELS, false);
    }
    printf("reduced plans ok: %ld checks\n", n_checks);
    return 0;
}

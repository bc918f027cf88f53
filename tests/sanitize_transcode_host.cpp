// sanitize_transcode_host.cpp -- the host layout of llicti_transcode_images (llicti_amd/csrc/host_plan.hpp: transcode_layout,
// transcode_plans_agree, plan_transcode_workspace_bytes) compiled by g++ alone, beside tests/sanitize_host.cpp (which drives the plans
// themselves).  A transcode works on two plans of one batch -- the source containers' and the target containers' -- in one workspace,
// [source plan | target plan].  What it holds, over a few hundred random (sizes, source modes, target modes):
//   - the two regions do not overlap and every workspace offset of either plan lies inside the reported size
//   - llicti_transcode_workspace_bytes covers the layout of both plan forms (tight, and force_ragged's 64-element blocks) and is at least
//     what the source-only and the target-only call need
//   - wherever the target's kernels read what the decoder wrote through the TARGET plan's tables -- planes (ImgGeo / Geom / StageGeom offsets),
//     CNN outputs (par_off), the DC band's grid -- the two plans agree, field by field, and transcode_plans_agree says so
//   - the refused combinations give 0
// tests/test_transcode_cpu.py builds it plain; under sanitizers:
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -o /tmp/sth tests/sanitize_transcode_host.cpp && /tmp/sth
#include <stdio.h>
#include <stdlib.h>

#include "../llicti_amd/csrc/host_plan.hpp"

static long n_checks = 0;
#define REQUIRE(c)                                                                      \
    do {                                                                                \
        ++n_checks;                                                                     \
        if (!(c)) { fprintf(stderr, "FAILED %s (%s:%d)\n", #c, __FILE__, __LINE__); exit(1); } \
    } while (0)

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd(uint32_t n)      // xorshift64*: 0 .. n - 1
{
    rng_state ^= rng_state >> 12; rng_state ^= rng_state << 25; rng_state ^= rng_state >> 27;
    return (uint32_t)((rng_state * 0x2545F4914F6CDD1Dull) >> 33) % n;
}

// a mode of lane kind k (0: reference format, 1: 64 lanes, 2: wide, 3: xwide, 4: xwide "auto") for a model of nlev levels
static int random_mode(int kind, int nlev)
{
    const bool cfgB = nlev != LLICTI_NLEVELS;
    switch (kind) {
    case 0: return LLICTI_MODE_AC;
    case 1: return LLICTI_MODE_RANS(1 + (int)rnd(32));
    case 2: return LLICTI_MODE_RANS_WIDE(1 + (int)rnd(14));
    case 3: return LLICTI_MODE_RANS_X(1 + (int)rnd(cfgB ? 18 : 32));
    default: return LLICTI_MODE_RANS_X_AUTO(1 + (int)rnd(cfgB ? 13 : 24));
    }
}

// every workspace offset of a plan, with the bytes the region behind it needs at least
static void offsets_inside(const Plan &p, size_t base, size_t lo, size_t hi)
{
    const size_t offs[] = { p.off_status, p.off_minmax, p.off_lift_part, p.off_planes, p.off_fplanes, p.off_params, p.off_params2, p.off_pairs, p.off_slots,
                            p.off_rinfo, p.off_rstate, p.off_rpos, p.off_rtail, p.off_slot_len, p.off_tables, p.off_acstate };
    for (size_t o : offs) REQUIRE(base + o >= lo && base + o < hi);
    REQUIRE(base + p.total <= hi);
    long pix = 0;
    for (const ImgGeo &ig : p.img) pix = std::max(pix, ig.pix_off + 3 * ig.plane);
    REQUIRE(p.off_planes + (size_t)pix * sizeof(int16_t) <= p.off_fplanes);
    REQUIRE(p.off_fplanes + (size_t)pix * sizeof(float) <= p.total);
    REQUIRE(p.off_status + (kStatusHead + (size_t)p.B) * sizeof(int32_t) <= p.total);
    REQUIRE(p.off_rpos + (size_t)p.B * sizeof(unsigned long long) <= p.off_rtail);      // the "auto" pick's sums live in the cursor array
}

static void drive(int B, const int *Hs, const int *Ws, const std::vector<int> &src, const std::vector<int> &dst, int nlev)
{
    const size_t need = plan_transcode_workspace_bytes(B, Hs, Ws, src.data(), (int)src.size(), dst.data(), (int)dst.size(), nlev);
    REQUIRE(need > 0);
    REQUIRE(need >= plan_workspace_bytes_vm(B, Hs, Ws, src.data(), (int)src.size(), nlev));
    REQUIRE(need >= plan_workspace_bytes_vm(B, Hs, Ws, dst.data(), (int)dst.size(), nlev));
    int MEs = 0, MEd = 0;
    std::vector<int> Mss, Msd;
    REQUIRE(resolve_modes("source", src.data(), (int)src.size(), B, &MEs, Mss) == 0);
    REQUIRE(resolve_modes("target", dst.data(), (int)dst.size(), B, &MEd, Msd) == 0);
    for (int ragged = 0; ragged < 2; ++ragged) {
        Plan s, d;
        build_plan(s, PlanSpec{ B, Hs, Ws, MEs, modes_ptr(Mss), nlev, ragged != 0 });
        build_plan(d, PlanSpec{ B, Hs, Ws, MEd, modes_ptr(Msd), nlev, ragged != 0 });
        const TranscodeLayout lay = transcode_layout(s, d);
        REQUIRE(lay.total <= need);
        REQUIRE(lay.off_dst >= s.total && lay.off_dst % 256 == 0 && lay.total == lay.off_dst + d.total);      // [source | target], disjoint
        offsets_inside(s, 0, 0, lay.off_dst);
        offsets_inside(d, lay.off_dst, lay.off_dst, lay.total);
        // the placement the kernels assume, field by field
        REQUIRE(transcode_plans_agree(s, d));
        REQUIRE(s.uniform == d.uniform && s.max_plane == d.max_plane);
        for (int b = 0; b < B; ++b) {
            REQUIRE(s.img[b].pix_off == d.img[b].pix_off && s.img[b].plane == d.img[b].plane);                  // rans_encode_kernel's seed symbols, the header's DC band
            REQUIRE(s.img[b].h4 == d.img[b].h4 && s.img[b].w4 == d.img[b].w4 && s.img[b].dcs == d.img[b].dcs);
        }
        for (int lvl = 0; lvl < nlev; ++lvl) {
            REQUIRE(s.lev_floats[lvl] == d.lev_floats[lvl] && s.lev_maxpos[lvl] == d.lev_maxpos[lvl]);
            for (int band = 0; band < 3; ++band)
                for (int b = 0; b < B; ++b) {
                    const StageGeom &a = s.sg[(size_t)(lvl * 3 + band) * B + b], &t = d.sg[(size_t)(lvl * 3 + band) * B + b];
                    REQUIRE(a.img_off == t.img_off && a.par_off == t.par_off);                                  // cdf_pairs_kernel: planes and CNN outputs
                    REQUIRE(a.h == t.h && a.w == t.w && a.hc == t.hc && a.wc == t.wc && a.oi == t.oi && a.oj == t.oj && a.lvl == t.lvl);
                    REQUIRE(t.par_off + (long)LLICTI_PARAM_STRIDE * t.h * t.w <= (long)s.lev_floats[lvl]);      // ... inside the SOURCE plan's buffer
                    // the pairs the kernel writes lie inside the TARGET plan's pairs region
                    REQUIRE((size_t)(d.pair_base[lvl * 3 + band] + 2 * t.pair_cs + t.pair_off + (long)t.hc * t.wc) * sizeof(uint32_t) <= d.off_slots - d.off_pairs);
                }
        }
        REQUIRE(s.off_params + s.lev_floats[0] * sizeof(float) <= s.off_pairs);
    }
    // a plan pair that does NOT agree is told apart (another batch size)
    if (B > 1) {
        Plan s, d;
        build_plan(s, PlanSpec{ B, Hs, Ws, MEs, modes_ptr(Mss), nlev });
        build_plan(d, PlanSpec{ B - 1, Hs, Ws, MEd, nullptr, nlev });
        REQUIRE(!transcode_plans_agree(s, d));
    }
}

int main()
{
    int n_cases = 0;
    for (int it = 0; it < 360; ++it) {
        const int nlev = (it % 6 == 5) ? kLevelsB : LLICTI_NLEVELS;
        const int top = nlev == kLevelsB ? 700 : 900;
        const int B = 1 + (int)rnd(5);
        const bool mixed = rnd(2) != 0;
        std::vector<int> Hs(B), Ws(B);
        const int H0 = 32 + (int)rnd(top - 32), W0 = 32 + (int)rnd(top - 32);
        for (int b = 0; b < B; ++b) { Hs[b] = mixed ? 32 + (int)rnd(top - 32) : H0; Ws[b] = mixed ? 32 + (int)rnd(top - 32) : W0; }
        bool sizes_differ = false;
        for (int b = 1; b < B; ++b) sizes_differ = sizes_differ || Hs[b] != Hs[0] || Ws[b] != Ws[0];
        // lane kinds: config B codes the reference format and xwide streams; mixed sizes need rANS on both sides; "auto" is a target only
        auto pick_kind = [&](bool target) -> int {
            for (;;) {
                const int k = (int)rnd(target ? 5 : 4);
                if (k == 0 && sizes_differ) continue;
                if (nlev == kLevelsB && (k == 1 || k == 2)) continue;
                return k;
            }
        };
        const int ks = pick_kind(false), kd = pick_kind(true);
        auto side = [&](int kind) {
            std::vector<int> m;
            // one per image; fixed and "auto" counts mixed (the call's model check takes the first image's count as an "auto" one then, so the fixed
            // counts stay inside the "auto" range)
            if (rnd(2) && kind != 0)
                for (int b = 0; b < B; ++b) m.push_back(kind == 4 && rnd(3) == 0 ? LLICTI_MODE_RANS_X(random_mode(4, nlev) & 0xFF) : random_mode(kind, nlev));
            else m.push_back(random_mode(kind, nlev));
            return m;
        };
        drive(B, Hs.data(), Ws.data(), side(ks), side(kd), nlev);
        ++n_cases;
    }
    // the sizes the GPU tests use, every source x target kind
    {
        const int modes[] = { LLICTI_MODE_AC, LLICTI_MODE_RANS(8), LLICTI_MODE_RANS_WIDE(4), LLICTI_MODE_RANS_X(2), LLICTI_MODE_RANS_X(10) };
        const int sizes[][2] = { { 67, 93 }, { 96, 128 }, { 32, 32 }, { 192, 256 }, { 768, 512 } };
        for (const auto &hw : sizes)
            for (int ms : modes)
                for (int md : modes) {
                    const int Hs[2] = { hw[0], hw[0] }, Ws[2] = { hw[1], hw[1] };
                    drive(2, Hs, Ws, { ms }, { md }, LLICTI_NLEVELS);
                    ++n_cases;
                }
    }
    // refused combinations: 0
    {
        const int Hs[3] = { 192, 128, 321 }, Ws[3] = { 256, 192, 481 }, He[3] = { 96, 96, 96 }, We[3] = { 128, 128, 128 };
        const int ac = LLICTI_MODE_AC, x2 = LLICTI_MODE_RANS_X(2), r4 = LLICTI_MODE_RANS(4), au = LLICTI_MODE_RANS_X_AUTO(3), bad = 0x777;
        REQUIRE(plan_transcode_workspace_bytes(3, He, We, &x2, 1, &ac, 1) > 0);
        REQUIRE(plan_transcode_workspace_bytes(3, He, We, &au, 1, &ac, 1) == 0);                  // an auto mode as a source
        const int au_one[3] = { x2, au, x2 };
        REQUIRE(plan_transcode_workspace_bytes(3, He, We, au_one, 3, &ac, 1) == 0);               // ... of one image
        const int kinds[3] = { x2, r4, x2 };
        REQUIRE(plan_transcode_workspace_bytes(3, He, We, kinds, 3, &x2, 1) == 0);                // mixed lane kinds, source
        REQUIRE(plan_transcode_workspace_bytes(3, He, We, &x2, 1, kinds, 3) == 0);                // ... target
        const int ac_x[3] = { ac, x2, ac };
        REQUIRE(plan_transcode_workspace_bytes(3, He, We, ac_x, 3, &x2, 1) == 0);
        REQUIRE(plan_transcode_workspace_bytes(3, Hs, Ws, &ac, 1, &x2, 1) == 0);                  // the reference format with different sizes, source
        REQUIRE(plan_transcode_workspace_bytes(3, Hs, Ws, &x2, 1, &ac, 1) == 0);                  // ... target
        REQUIRE(plan_transcode_workspace_bytes(3, Hs, Ws, &x2, 1, &au, 1) > 0);
        REQUIRE(plan_transcode_workspace_bytes(3, He, We, &bad, 1, &x2, 1) == 0);
        REQUIRE(plan_transcode_workspace_bytes(3, He, We, &x2, 1, &bad, 1) == 0);
        REQUIRE(plan_transcode_workspace_bytes(3, He, We, nullptr, 1, &x2, 1) == 0);
        REQUIRE(plan_transcode_workspace_bytes(3, He, We, &x2, 2, &x2, 1) == 0);                  // neither one mode nor one per image
        const int small[3] = { 96, 31, 96 }, big[3] = { 96, 8161, 96 };
        REQUIRE(plan_transcode_workspace_bytes(3, small, We, &x2, 1, &x2, 1) == 0);
        REQUIRE(plan_transcode_workspace_bytes(3, He, big, &x2, 1, &x2, 1) == 0);
        REQUIRE(plan_transcode_workspace_bytes(0, He, We, &x2, 1, &x2, 1) == 0);
        // config B: its modes only, at most 1020 pixels per side
        const int x9 = LLICTI_MODE_RANS_X(9), x19 = LLICTI_MODE_RANS_X(19), Hb[1] = { 64 }, Wb[1] = { 48 }, Hl[1] = { 1056 };
        REQUIRE(plan_transcode_workspace_bytes(1, Hb, Wb, &ac, 1, &x9, 1, kLevelsB) > 0);
        REQUIRE(plan_transcode_workspace_bytes(1, Hb, Wb, &x9, 1, &ac, 1, kLevelsB) > 0);
        REQUIRE(plan_transcode_workspace_bytes(1, Hb, Wb, &r4, 1, &ac, 1, kLevelsB) == 0);
        REQUIRE(plan_transcode_workspace_bytes(1, Hb, Wb, &ac, 1, &x19, 1, kLevelsB) == 0);
        REQUIRE(plan_transcode_workspace_bytes(1, Hl, Wb, &ac, 1, &x9, 1, kLevelsB) == 0);
    }
    printf("transcode plans ok: %d cases, %ld checks\n", n_cases, n_checks);
    return 0;
}

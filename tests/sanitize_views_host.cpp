// sanitize_views_host.cpp -- the host side of llicti_decode_images_tensor_views (llicti_amd/csrc/host_plan.hpp: resolve_views; host_types.hpp:
// ViewSlice, kViewMax, kViewCountMax) compiled by g++ alone, beside tests/sanitize_resize_host.cpp.  What it holds:
//   - the views of a call are validated WITHOUT a plan and pack into three words per view that unpack, with the kernel's masks, to the view's
//     origin, flip, extent and image index -- image index 65,535 and a group of 1,048,576 views included
//   - every NULL default: image = view v is image v (n == B), y0 / x0 = 0, hs / ws = the whole decoded image of the VIEW'S image from the
//     origin, flip = none, mean / std = no normalisation
//   - every refusal, and that its message names the group and, where one is at fault, the view: G outside 1 .. LLICTI_VIEW_GROUPS_MAX, null
//     groups, a null d_out, n outside 1 .. 1,048,576, an image index outside 0 .. B - 1, image NULL with n != B, and resolve_resize's own
//     refusals against the view's image (box extents, a box one row or column too far, sizes, flag, scale above 4, dtype, mean / std)
//   - a one-group identity table packs the words resolve_resize packs for the same boxes
// tests/test_views_cpu.py builds it plain; under sanitizers:
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -o /tmp/svh tests/sanitize_views_host.cpp && /tmp/svh
#include <stdio.h>
#include <stdlib.h>
#include <limits>

#include "../llicti_amd/csrc/host_plan.hpp"

static long n_checks = 0;
#define REQUIRE(c)                                                                      \
    do {                                                                                \
        ++n_checks;                                                                     \
        if (!(c)) { fprintf(stderr, "FAILED %s (%s:%d) [%s]\n", #c, __FILE__, __LINE__, g_err.c_str()); exit(1); } \
    } while (0)

static const float kMean[3] = { 0.485f, 0.456f, 0.406f }, kStd[3] = { 0.229f, 0.224f, 0.225f };
static char g_dummy[16];      // (a non-null d_out: nothing here dereferences it)

static bool has(const char *word) { return g_err.find(word) != std::string::npos; }
static bool names(int g, int v)
{
    char want[64];
    snprintf(want, sizeof want, "group %d", g);
    if (!has(want)) return false;
    if (v < 0) return true;
    snprintf(want, sizeof want, "view %d ", v);
    return has(want);
}

static llicti_view_group group(int dtype, int Ho, int Wo, int aa, int n, const int *image, const int *y0, const int *x0, const int *hs, const int *ws,
                               const uint8_t *flip)
{
    llicti_view_group g;
    memset(&g, 0, sizeof g);
    g.d_out = g_dummy; g.dtype = dtype; g.Ho = Ho; g.Wo = Wo; g.antialias = aa; g.n = n;
    g.image = image; g.y0 = y0; g.x0 = x0; g.hs = hs; g.ws = ws; g.flip = flip;
    return g;
}

static int run(int B, const int *Hs, const int *Ws, int r, const llicti_view_group *gs, int G, std::vector<ViewGroupOut> &out, TensorNorm &nm,
               const float *mean = nullptr, const float *sd = nullptr)
{
    const ViewArgs a{ gs, G, mean, sd };
    return resolve_views("test", B, Hs, Ws, r, a, out, nm);
}

int main()
{
    REQUIRE(kViewMax == 128 && kViewCountMax == 1048576 && sizeof(ViewSlice) == 3 * 128 * 4 && LLICTI_VIEW_GROUPS_MAX == 16);
    const int Hs[] = { 33, 64, 96, 512 }, Ws[] = { 47, 96, 67, 768 };
    const int B = 4;
    std::vector<ViewGroupOut> out;
    TensorNorm nm;
    for (int r = 0; r <= 2; ++r) {
        int Hr[B], Wr[B];
        for (int b = 0; b < B; ++b) { Hr[b] = reduced_dim(Hs[b], r); Wr[b] = reduced_dim(Ws[b], r); }
        // two groups: seven views in no order with every array given, and the identity with every array NULL
        const int image[] = { 2, 0, 0, 3, 2, 1, 0 };
        const int n = 7;
        int y0[n], x0[n], hs[n], ws[n];
        uint8_t flip[n];
        for (int v = 0; v < n; ++v) {
            const int b = image[v];
            y0[v] = (Hr[b] - 1) / (v + 2); x0[v] = (Wr[b] - 1) / 3;
            hs[v] = std::min(Hr[b] - y0[v], 64); ws[v] = std::max(1, std::min((Wr[b] - x0[v]) / 2, 96));
            flip[v] = (uint8_t)((v & 1) * 5);
        }
        const llicti_view_group gs[2] = { group(LLICTI_T_F16, 16, 24, 1, n, image, y0, x0, hs, ws, flip),
                                          group(LLICTI_T_F32, 8160, 8160, 1, B, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) };
        REQUIRE(run(B, Hs, Ws, r, gs, 2, out, nm, kMean, kStd) == 0);
        REQUIRE(out.size() == 2 && nm.on == 1 && nm.mean[1] == kMean[1] && nm.std[2] == kStd[2]);
        REQUIRE(out[0].d_out == g_dummy && out[0].dtype == LLICTI_T_F16 && out[0].Ho == 16 && out[0].Wo == 24 && out[0].antialias == 1 && out[0].n == n);
        REQUIRE((int)out[0].words.size() == 3 * n && (int)out[1].words.size() == 3 * B);
        for (int v = 0; v < n; ++v) {                   // (the kernel's masks)
            const uint32_t w0 = out[0].words[3 * v], w1 = out[0].words[3 * v + 1], w2 = out[0].words[3 * v + 2];
            REQUIRE((int)(w0 & 0x1FFFu) == y0[v] && (int)((w0 >> 13) & 0x1FFFu) == x0[v] && ((w0 >> 26) & 1u) == (flip[v] ? 1u : 0u) && (w0 >> 27) == 0);
            REQUIRE((int)(w1 & 0x1FFFu) == hs[v] && (int)((w1 >> 13) & 0x1FFFu) == ws[v] && (w1 >> 26) == 0 && (int)w2 == image[v]);
            // the last plane pixel the view reads lies inside ITS image
            REQUIRE(((y0[v] + hs[v] - 1) << r) < Hs[image[v]] && ((x0[v] + ws[v] - 1) << r) < Ws[image[v]]);
        }
        for (int b = 0; b < B; ++b)
            REQUIRE(out[1].words[3 * b] == 0 && out[1].words[3 * b + 1] == resize_ext_pack(Hr[b], Wr[b]) && (int)out[1].words[3 * b + 2] == b);
        // without mean / std: no normalisation
        REQUIRE(run(B, Hs, Ws, r, gs, 2, out, nm) == 0 && nm.on == 0);
        // NULL extents are taken against the VIEW'S image: origins alone, on images in reverse order
        const int rev[] = { 3, 2, 1, 0 }, oy[] = { 5, 4, 3, 2 }, ox[] = { 1, 2, 3, 4 };
        const llicti_view_group rest = group(LLICTI_T_BF16, 8160, 8160, 0, B, rev, oy, ox, nullptr, nullptr, nullptr);
        REQUIRE(run(B, Hs, Ws, r, &rest, 1, out, nm) == 0);
        for (int v = 0; v < B; ++v)
            REQUIRE(out[0].words[3 * v] == tensor_win_pack(oy[v], ox[v], false) && out[0].words[3 * v + 1] == resize_ext_pack(Hr[rev[v]] - oy[v], Wr[rev[v]] - ox[v]) &&
                    (int)out[0].words[3 * v + 2] == rev[v]);
        // the identity group packs resolve_resize's words
        {
            int iy[B], ix[B], ih[B], iw[B];
            uint8_t fl[B];
            for (int b = 0; b < B; ++b) { iy[b] = b; ix[b] = 2 * b; ih[b] = std::min(Hr[b] - iy[b], 40); iw[b] = std::min(Wr[b] - ix[b], 50); fl[b] = (uint8_t)(b & 1); }
            const llicti_view_group id = group(LLICTI_T_F32, 10, 13, 1, B, nullptr, iy, ix, ih, iw, fl);
            const ResizeArgs t{ LLICTI_T_F32, 10, 13, iy, ix, ih, iw, fl, kMean, kStd, 1 };
            std::vector<uint32_t> bx;
            TensorNorm nm2;
            REQUIRE(run(B, Hs, Ws, r, &id, 1, out, nm, kMean, kStd) == 0 && resolve_resize("test", B, Hs, Ws, r, t, bx, nm2) == 0);
            REQUIRE(memcmp(&nm, &nm2, sizeof nm) == 0);
            for (int b = 0; b < B; ++b) REQUIRE(out[0].words[3 * b] == bx[2 * b] && out[0].words[3 * b + 1] == bx[2 * b + 1]);
        }
        // refusals per view of group 1 (group 0 valid in front of it), each naming group and view
        llicti_view_group two[2] = { gs[1], gs[0] };
        const int L = n - 1;
        REQUIRE(run(B, Hs, Ws, r, two, 2, out, nm) == 0);
        { const int keep = hs[L]; hs[L] = Hr[image[L]] - y0[L] + 1;                   // one row too far
          REQUIRE(run(B, Hs, Ws, r, two, 2, out, nm) == LLICTI_EINVAL && names(1, L) && has("leaves") && has("image 0")); hs[L] = keep; }
        { const int keep = ws[3]; ws[3] = Wr[image[3]] - x0[3] + 1;                   // one column too far
          two[1].antialias = 0;
          REQUIRE(run(B, Hs, Ws, r, two, 2, out, nm) == LLICTI_EINVAL && names(1, 3) && has("leaves") && has("image 3"));
          two[1].antialias = 1; ws[3] = keep; }
        for (int bad : { 0, -3 }) {
            { const int keep = ws[0]; ws[0] = bad; REQUIRE(run(B, Hs, Ws, r, two, 2, out, nm) == LLICTI_EINVAL && names(1, 0)); ws[0] = keep; }
            { const int keep = hs[L]; hs[L] = bad; REQUIRE(run(B, Hs, Ws, r, two, 2, out, nm) == LLICTI_EINVAL && names(1, L)); hs[L] = keep; }
        }
        { const int keep = y0[2]; y0[2] = -1; REQUIRE(run(B, Hs, Ws, r, two, 2, out, nm) == LLICTI_EINVAL && names(1, 2)); y0[2] = keep; }
        { const int keep = x0[4]; x0[4] = -1; REQUIRE(run(B, Hs, Ws, r, two, 2, out, nm) == LLICTI_EINVAL && names(1, 4)); x0[4] = keep; }
        // an origin outside the view's image with a NULL extent: refused, never a negative extent packed
        { int far[B] = { 0, 0, 0, 0 }; far[1] = Hr[rev[1]];
          const llicti_view_group g = group(LLICTI_T_F32, 4, 4, 0, B, rev, far, nullptr, nullptr, nullptr, nullptr);
          REQUIRE(run(B, Hs, Ws, r, &g, 1, out, nm) == LLICTI_EINVAL && names(0, 1)); }
        // the scale-4 edge on the rows of view 3 (image 3: the tall one): 4 Ho rows are taken, 4 Ho + 1 refused with the filter and taken without
        if (Hr[3] >= 65) {
            const int keep = hs[3], keep_y = y0[3];
            y0[3] = 0; hs[3] = 64;
            REQUIRE(run(B, Hs, Ws, r, two, 2, out, nm) == 0);
            hs[3] = 65;
            REQUIRE(run(B, Hs, Ws, r, two, 2, out, nm) == LLICTI_EINVAL && names(1, 3) && has("raise reduce"));
            two[1].antialias = 0;
            REQUIRE(run(B, Hs, Ws, r, two, 2, out, nm) == 0);
            two[1].antialias = 1; hs[3] = keep; y0[3] = keep_y;
        }
        // an image index outside the batch
        { int img2[n]; memcpy(img2, image, sizeof img2);
          two[1].image = img2;
          img2[5] = B; REQUIRE(run(B, Hs, Ws, r, two, 2, out, nm) == LLICTI_EINVAL && names(1, 5) && has("image 4"));
          img2[5] = -1; REQUIRE(run(B, Hs, Ws, r, two, 2, out, nm) == LLICTI_EINVAL && names(1, 5) && has("image -1"));
          img2[5] = std::numeric_limits<int>::max(); REQUIRE(run(B, Hs, Ws, r, two, 2, out, nm) == LLICTI_EINVAL && names(1, 5));
          two[1].image = image; }
        REQUIRE(run(B, Hs, Ws, r, two, 2, out, nm) == 0);
    }
    // per group: G, groups, d_out, n, image NULL with n != B, dtype, sizes, flag; per call: mean / std, reduce
    {
        const llicti_view_group ok = group(LLICTI_T_F32, 16, 24, 0, B, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
        llicti_view_group many[LLICTI_VIEW_GROUPS_MAX + 1];
        for (auto &g : many) g = ok;
        REQUIRE(run(B, Hs, Ws, 0, many, LLICTI_VIEW_GROUPS_MAX, out, nm) == 0 && (int)out.size() == LLICTI_VIEW_GROUPS_MAX);
        REQUIRE(run(B, Hs, Ws, 0, many, LLICTI_VIEW_GROUPS_MAX + 1, out, nm) == LLICTI_EINVAL && has("17 groups"));
        for (int bad : { 0, -1 }) REQUIRE(run(B, Hs, Ws, 0, many, bad, out, nm) == LLICTI_EINVAL && has("groups"));
        REQUIRE(run(B, Hs, Ws, 0, nullptr, 1, out, nm) == LLICTI_EINVAL && has("null groups"));
        auto one = [&](llicti_view_group g, const float *mean = nullptr, const float *sd = nullptr, int r = 0) {
            many[2] = g;
            const int rc = run(B, Hs, Ws, r, many, 4, out, nm, mean, sd);
            many[2] = ok;
            return rc;
        };
        { llicti_view_group g = ok; g.d_out = nullptr; REQUIRE(one(g) == LLICTI_EINVAL && names(2, -1) && has("d_out")); }
        for (int bad : { 0, -1, kViewCountMax + 1, std::numeric_limits<int>::max() }) {
            llicti_view_group g = ok; g.n = bad; REQUIRE(one(g) == LLICTI_EINVAL && names(2, -1) && has("views"));
        }
        for (int bad : { 1, B - 1, B + 1, kViewCountMax }) { llicti_view_group g = ok; g.n = bad; REQUIRE(one(g) == LLICTI_EINVAL && names(2, -1) && has("image = NULL")); }
        for (int bad : { -1, 3, 7 }) { llicti_view_group g = ok; g.dtype = bad; REQUIRE(one(g) == LLICTI_EINVAL && names(2, -1) && has("dtype")); }
        for (int bad : { 0, -2, 8161, 1 << 20 }) {
            llicti_view_group g = ok; g.Ho = bad; REQUIRE(one(g) == LLICTI_EINVAL && names(2, -1) && has("output size"));
            g = ok; g.Wo = bad; REQUIRE(one(g) == LLICTI_EINVAL && names(2, -1) && has("output size"));
        }
        for (int bad : { -1, 2, 255 }) { llicti_view_group g = ok; g.antialias = bad; REQUIRE(one(g) == LLICTI_EINVAL && names(2, -1) && has("antialias")); }
        { llicti_view_group g = ok; g.antialias = 1; g.Ho = 8; REQUIRE(one(g) == LLICTI_EINVAL && names(2, 0) && has("raise reduce")); }      // 33 rows to 8
        REQUIRE(one(ok, kMean, nullptr) == LLICTI_EINVAL && one(ok, nullptr, kStd) == LLICTI_EINVAL && one(ok, kMean, kStd) == 0);
        const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
        for (float v : { 0.0f, -0.0f, -1.0f, inf, -inf, nan })
            for (int k = 0; k < 3; ++k) {
                float sd[3] = { kStd[0], kStd[1], kStd[2] };
                sd[k] = v;
                REQUIRE(one(ok, kMean, sd) == LLICTI_EINVAL && has("std"));
            }
        for (int bad : { -1, LLICTI_NLEVELS + 1 }) REQUIRE(one(ok, nullptr, nullptr, bad) == LLICTI_EINVAL && has("reduce"));
    }
    // the width of the words: image index 65,535 of a batch of 65,536 images, and a group of 1,048,576 views whose last view names it
    {
        const int Bb = 65536, n = kViewCountMax;
        std::vector<int> Hb(Bb, 32), Wb(Bb, 32), image(n), y0(n), x0(n), hs(n), ws(n);
        std::vector<uint8_t> flip(n);
        Hb[Bb - 1] = 8160; Wb[Bb - 1] = 8160;
        for (int v = 0; v < n; ++v) { image[v] = (int)(((long)v * 40503L) % Bb); y0[v] = v & 7; x0[v] = (v >> 3) & 7; hs[v] = 1 + (v % 24); ws[v] = 1 + (v % 23); flip[v] = (uint8_t)(v & 1); }
        image[n - 1] = Bb - 1; y0[n - 1] = 8159; x0[n - 1] = 8158; hs[n - 1] = 1; ws[n - 1] = 2; flip[n - 1] = 1;
        image[0] = Bb - 1; y0[0] = 0; x0[0] = 0; hs[0] = 8160; ws[0] = 8160; flip[0] = 0;
        const llicti_view_group g = group(LLICTI_T_F16, 2040, 2040, 1, n, image.data(), y0.data(), x0.data(), hs.data(), ws.data(), flip.data());
        REQUIRE(run(Bb, Hb.data(), Wb.data(), 0, &g, 1, out, nm) == 0 && out[0].n == n && out[0].words.size() == 3 * (size_t)n);
        for (int v = 0; v < n; v += (v < 64 || v > n - 64) ? 1 : 4093) {
            const uint32_t w0 = out[0].words[3 * (size_t)v], w1 = out[0].words[3 * (size_t)v + 1], w2 = out[0].words[3 * (size_t)v + 2];
            REQUIRE((int)(w0 & 0x1FFFu) == y0[v] && (int)((w0 >> 13) & 0x1FFFu) == x0[v] && ((w0 >> 26) & 1u) == flip[v] && (w0 >> 27) == 0);
            REQUIRE((int)(w1 & 0x1FFFu) == hs[v] && (int)((w1 >> 13) & 0x1FFFu) == ws[v] && (w1 >> 26) == 0 && w2 == (uint32_t)image[v]);
        }
        REQUIRE(out[0].words[3 * (size_t)(n - 1) + 2] == 65535u && out[0].words[1] == resize_ext_pack(8160, 8160));
        // the launches' slices: every view is in exactly one, the last slice is full here (2^20 = 8192 x 128)
        long covered = 0;
        int launches = 0;
        for (int v0 = 0; v0 < n; v0 += kViewMax) { covered += std::min(kViewMax, n - v0); ++launches; }
        REQUIRE(covered == n && launches == 8192);
        image[n - 1] = Bb;
        REQUIRE(run(Bb, Hb.data(), Wb.data(), 0, &g, 1, out, nm) == LLICTI_EINVAL && names(0, n - 1) && has("image 65536"));
    }
    printf("view tables ok: %ld checks\n", n_checks);
    return 0;
}

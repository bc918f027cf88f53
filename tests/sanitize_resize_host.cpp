// sanitize_resize_host.cpp -- the host side of llicti_decode_images_tensor_resized (llicti_amd/csrc/host_plan.hpp: resolve_resize;
// host_types.hpp: resize_window_ok, resize_ext_pack, resize_axis) compiled by g++ alone, beside tests/sanitize_tensor_host.cpp.  What it holds:
//   - the boxes of a call are validated WITHOUT a plan (kernel arguments, no part of a plan or its key) and pack into two words per image that
//     unpack, with the kernel's masks, to the same origin, extent and flag, for sizes up to 8160 and every reduce
//   - every NULL default: y0 / x0 = 0, hs / ws = the whole decoded image from the origin, flip = none, mean / std = no normalisation
//   - every refusal, and that its message names the image: hs or ws < 1, a box one row or column too far, Ho or Wo outside 1 .. 8160, antialias
//     not 0 or 1, antialias = 1 at a scale above 4 (exactly 4 is taken; the message says to raise reduce), and resolve_tensor's own refusals
//   - resize_axis: the taps of every output index lie inside the box, are at most kResizeTapMax wherever the call is admitted, and sum to 1
// tests/test_resize_cpu.py builds it plain; under sanitizers:
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -o /tmp/srh tests/sanitize_resize_host.cpp && /tmp/srh
#include <math.h>
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

static bool names(int b)
{
    char want[32];
    snprintf(want, sizeof want, "image %d", b);
    return g_err.find(want) != std::string::npos;
}

static void drive(int B, const int *Hs, const int *Ws, int nlev)
{
    std::vector<uint32_t> bx;
    TensorNorm nm;
    for (int r = 0; r <= nlev; ++r) {
        std::vector<int> Hr(B), Wr(B), y0(B), x0(B), hs(B), ws(B);
        std::vector<uint8_t> flip(B);
        for (int b = 0; b < B; ++b) {
            Hr[b] = reduced_dim(Hs[b], r); Wr[b] = reduced_dim(Ws[b], r);
            y0[b] = (Hr[b] - 1) / (b + 2); x0[b] = (Wr[b] - 1) / 3;
            hs[b] = Hr[b] - y0[b]; ws[b] = std::max(1, (Wr[b] - x0[b]) / 2);      // ends at the bottom row; an interior column range
            flip[b] = (uint8_t)((b & 1) * 5);
        }
        // an output no box shrinks to by more than 4: taken with both flags
        int Ho = 1, Wo = 1;
        for (int b = 0; b < B; ++b) { Ho = std::max(Ho, (hs[b] + 3) / 4); Wo = std::max(Wo, (ws[b] + 3) / 4); }
        for (int aa = 0; aa < 2; ++aa)
            for (int dtype : { LLICTI_T_F32, LLICTI_T_F16, LLICTI_T_BF16 }) {
                const ResizeArgs t{ dtype, Ho, Wo, y0.data(), x0.data(), hs.data(), ws.data(), flip.data(), kMean, kStd, aa };
                REQUIRE(resolve_resize("test", B, Hs, Ws, r, t, bx, nm) == 0);
                REQUIRE((int)bx.size() == 2 * B && nm.on == 1 && nm.mean[1] == kMean[1] && nm.std[2] == kStd[2]);
                for (int b = 0; b < B; ++b) {                   // (the kernel's masks)
                    const uint32_t w0 = bx[2 * b], w1 = bx[2 * b + 1];
                    REQUIRE((int)(w0 & 0x1FFFu) == y0[b] && (int)((w0 >> 13) & 0x1FFFu) == x0[b] && ((w0 >> 26) & 1u) == (flip[b] ? 1u : 0u) && (w0 >> 27) == 0);
                    REQUIRE((int)(w1 & 0x1FFFu) == hs[b] && (int)((w1 >> 13) & 0x1FFFu) == ws[b] && (w1 >> 26) == 0);
                    // the last plane pixel the box reads lies inside the image
                    REQUIRE(((y0[b] + hs[b] - 1) << r) < Hs[b] && ((x0[b] + ws[b] - 1) << r) < Ws[b]);
                }
            }
        // NULL arrays: the whole decoded image from the corner, no flip, no normalisation
        const int Hall = 8160, Wall = 8160;      // (an output as large as it gets: magnification is always taken)
        const ResizeArgs plain{ LLICTI_T_F32, Hall, Wall, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 1 };
        REQUIRE(resolve_resize("test", B, Hs, Ws, r, plain, bx, nm) == 0 && nm.on == 0);
        for (int b = 0; b < B; ++b) REQUIRE(bx[2 * b] == 0 && bx[2 * b + 1] == resize_ext_pack(Hr[b], Wr[b]));
        // origins alone: the extents default to what is left of the image
        const ResizeArgs rest{ LLICTI_T_F32, Hall, Wall, y0.data(), x0.data(), nullptr, nullptr, nullptr, nullptr, nullptr, 0 };
        REQUIRE(resolve_resize("test", B, Hs, Ws, r, rest, bx, nm) == 0);
        for (int b = 0; b < B; ++b) REQUIRE(bx[2 * b] == tensor_win_pack(y0[b], x0[b], false) && bx[2 * b + 1] == resize_ext_pack(Hr[b] - y0[b], Wr[b] - x0[b]));
        // extents alone: from the corner
        const ResizeArgs ext{ LLICTI_T_F32, Hall, Wall, nullptr, nullptr, hs.data(), ws.data(), nullptr, nullptr, nullptr, 0 };
        REQUIRE(resolve_resize("test", B, Hs, Ws, r, ext, bx, nm) == 0);
        for (int b = 0; b < B; ++b) REQUIRE(bx[2 * b] == 0 && bx[2 * b + 1] == resize_ext_pack(hs[b], ws[b]));
        // an origin outside the image with a NULL extent: refused, never a negative extent packed
        { std::vector<int> far(y0); far[B - 1] = Hr[B - 1];
          const ResizeArgs t{ LLICTI_T_F32, Ho, Wo, far.data(), x0.data(), nullptr, nullptr, nullptr, nullptr, nullptr, 0 };
          REQUIRE(resolve_resize("test", B, Hs, Ws, r, t, bx, nm) == LLICTI_EINVAL && names(B - 1)); }
        // refusals on the last image alone (and image 0), each naming it
        const ResizeArgs ok{ LLICTI_T_F32, Ho, Wo, y0.data(), x0.data(), hs.data(), ws.data(), nullptr, nullptr, nullptr, 0 };
        const int L = B - 1;
        hs[L] += 1;                                              // one row too far (the box ended at the bottom row)
        REQUIRE(resolve_resize("test", B, Hs, Ws, r, ok, bx, nm) == LLICTI_EINVAL && names(L) && g_err.find("leaves") != std::string::npos);
        hs[L] -= 1;
        { const int keep = ws[0]; ws[0] = Wr[0] - x0[0] + 1;     // one column too far
          REQUIRE(resolve_resize("test", B, Hs, Ws, r, ok, bx, nm) == LLICTI_EINVAL && names(0));
          ws[0] = 0; REQUIRE(resolve_resize("test", B, Hs, Ws, r, ok, bx, nm) == LLICTI_EINVAL && names(0));
          ws[0] = -3; REQUIRE(resolve_resize("test", B, Hs, Ws, r, ok, bx, nm) == LLICTI_EINVAL && names(0));
          ws[0] = keep; }
        { const int keep = hs[L]; hs[L] = 0; REQUIRE(resolve_resize("test", B, Hs, Ws, r, ok, bx, nm) == LLICTI_EINVAL && names(L)); hs[L] = keep; }
        { const int keep = y0[L]; y0[L] = -1; REQUIRE(resolve_resize("test", B, Hs, Ws, r, ok, bx, nm) == LLICTI_EINVAL && names(L)); y0[L] = keep; }
        { const int keep = x0[L]; x0[L] = -1; REQUIRE(resolve_resize("test", B, Hs, Ws, r, ok, bx, nm) == LLICTI_EINVAL && names(L)); x0[L] = keep; }
        REQUIRE(resolve_resize("test", B, Hs, Ws, r, ok, bx, nm) == 0);
        // the scale-4 edge on the rows of the last image: hs = 4 Ho is taken, hs = 4 Ho + 1 refused with the filter on and taken without
        if (Hr[L] >= 5) {
            const int Hq = (Hr[L] - 1) / 4;
            std::vector<int> zy(B, 0), zx(B, 0), eh(B, Hq), ew(B, 1);      // (every image has at least Hq rows?  only the last one is stretched)
            for (int b = 0; b < B; ++b) eh[b] = std::min(Hq, Hr[b]);
            eh[L] = 4 * Hq;
            ResizeArgs t{ LLICTI_T_F32, Hq, 1, zy.data(), zx.data(), eh.data(), ew.data(), nullptr, nullptr, nullptr, 1 };
            REQUIRE(resolve_resize("test", B, Hs, Ws, r, t, bx, nm) == 0);
            eh[L] = 4 * Hq + 1;
            REQUIRE(resolve_resize("test", B, Hs, Ws, r, t, bx, nm) == LLICTI_EINVAL && names(L) && g_err.find("raise reduce") != std::string::npos);
            t.antialias = 0;
            REQUIRE(resolve_resize("test", B, Hs, Ws, r, t, bx, nm) == 0);
        }
    }
}

static void axis(int n, int m, int aa, bool admitted)
{
    float w[kResizeTapMax + 1];
    const int step = m > 600 ? 97 : 1;
    for (int i = 0; i < m; i = (i + step < m || i == m - 1) ? i + step : m - 1) {
        int lo = -1;
        const int cnt = resize_axis(n, m, aa, i, &lo, w, kResizeTapMax + 1);
        REQUIRE(cnt >= 1 && lo >= 0 && lo + cnt <= n);
        if (admitted) {
            REQUIRE(cnt <= kResizeTapMax && w[kResizeTapMax] == 0.0f);
            double sum = 0;
            for (int k = 0; k < kResizeTapMax; ++k) { REQUIRE(w[k] >= 0.0f && (k < cnt || w[k] == 0.0f)); sum += w[k]; }
            REQUIRE(fabs(sum - 1.0) <= 2.0 * 1.1920928955078125e-7);
        }
    }
}

int main()
{
    REQUIRE(resize_window_ok(8160, 8160, 0, 8159, 8159, 1, 1, 8160, 8160, 1) && !resize_window_ok(8160, 8160, 0, 8160, 0, 1, 1, 1, 1, 0));
    REQUIRE(resize_ext_pack(8160, 8160) == (8160u | (8160u << 13)));
    REQUIRE(!resize_window_ok(64, 64, 0, 2147483647, 0, 2, 2, 1, 1, 0) && !resize_window_ok(64, 64, 0, 0, 0, 2147483647, 2, 8160, 8160, 1));
    REQUIRE(!resize_window_ok(64, 64, 0, 0, 0, 2, 2147483647, 8160, 8160, 0));
    REQUIRE(!resize_window_ok(64, 64, 6, 0, 0, 1, 1, 1, 1, 0) && !resize_window_ok(64, 64, -1, 0, 0, 1, 1, 1, 1, 0) && resize_window_ok(64, 64, 5, 1, 1, 1, 1, 3, 3, 1));
    REQUIRE(!resize_window_ok(64, 64, 0, 0, 0, 8, 8, 8161, 8, 0) && !resize_window_ok(64, 64, 0, 0, 0, 8, 8, 8, 8161, 0) && !resize_window_ok(64, 64, 0, 0, 0, 8, 8, 0, 8, 0));
    REQUIRE(!resize_window_ok(64, 64, 0, 0, 0, 8, 8, 8, 8, 2) && !resize_window_ok(64, 64, 0, 0, 0, 8, 8, 8, 8, -1));
    REQUIRE(resize_window_ok(64, 64, 0, 0, 0, 64, 64, 16, 16, 1) && !resize_window_ok(64, 65, 0, 0, 0, 64, 65, 16, 16, 1) && resize_window_ok(64, 65, 0, 0, 0, 64, 65, 16, 16, 0));
    const int sizes[][2] = { { 32, 32 }, { 33, 35 }, { 67, 93 }, { 64, 96 }, { 768, 512 }, { 8160, 8160 } };
    for (const auto &hw : sizes)
        for (int B : { 1, 3 }) {
            std::vector<int> Hs(B, hw[0]), Ws(B, hw[1]);
            drive(B, Hs.data(), Ws.data(), LLICTI_NLEVELS);
            if (hw[0] <= 1020) drive(B, Hs.data(), Ws.data(), kLevelsB);
        }
    {   // mixed sizes
        const int Hs[] = { 67, 64, 33, 512 }, Ws[] = { 93, 96, 35, 512 };
        drive(4, Hs, Ws, LLICTI_NLEVELS);
        drive(3, Hs, Ws, kLevelsB);
    }
    // dtype, output size, flag, mean / std
    const int H1[] = { 64 }, W1[] = { 96 };
    std::vector<uint32_t> bx;
    TensorNorm nm;
    auto rc = [&](int dtype, int Ho, int Wo, int aa, const float *mean, const float *sd) {
        const ResizeArgs t{ dtype, Ho, Wo, nullptr, nullptr, nullptr, nullptr, nullptr, mean, sd, aa };
        return resolve_resize("test", 1, H1, W1, 0, t, bx, nm);
    };
    REQUIRE(rc(LLICTI_T_F16, 16, 24, 1, kMean, kStd) == 0 && rc(LLICTI_T_F16, 8160, 8160, 1, nullptr, nullptr) == 0 && rc(LLICTI_T_BF16, 1, 1, 0, nullptr, nullptr) == 0);
    REQUIRE(rc(LLICTI_T_F32, 1, 1, 1, nullptr, nullptr) == LLICTI_EINVAL && g_err.find("raise reduce") != std::string::npos);
    REQUIRE(rc(LLICTI_T_F32, 16, 23, 1, nullptr, nullptr) == LLICTI_EINVAL && rc(LLICTI_T_F32, 15, 24, 1, nullptr, nullptr) == LLICTI_EINVAL);
    for (int bad : { -1, 3, 7 }) REQUIRE(rc(bad, 16, 24, 1, nullptr, nullptr) == LLICTI_EINVAL);
    for (int bad : { 0, -2, 8161, 1 << 20 }) REQUIRE(rc(LLICTI_T_F32, bad, 24, 0, nullptr, nullptr) == LLICTI_EINVAL && rc(LLICTI_T_F32, 16, bad, 0, nullptr, nullptr) == LLICTI_EINVAL);
    for (int bad : { -1, 2, 255 }) REQUIRE(rc(LLICTI_T_F32, 16, 24, bad, nullptr, nullptr) == LLICTI_EINVAL);
    REQUIRE(rc(LLICTI_T_F32, 16, 24, 1, kMean, nullptr) == LLICTI_EINVAL && rc(LLICTI_T_F32, 16, 24, 1, nullptr, kStd) == LLICTI_EINVAL);
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    for (float v : { 0.0f, -0.0f, -1.0f, inf, -inf, nan })
        for (int k = 0; k < 3; ++k) {
            float sd[3] = { kStd[0], kStd[1], kStd[2] };
            sd[k] = v;
            REQUIRE(rc(LLICTI_T_F32, 16, 24, 1, kMean, sd) == LLICTI_EINVAL);
        }
    // the weight rule on the host: in bounds, at most kResizeTapMax taps where a call is admitted, weights that sum to 1
    for (int n : { 1, 2, 3, 31, 32, 33, 93, 224, 899, 8160 })
        for (int m : { 1, 2, 7, 23, 24, 224, 2040, 8160 })
            for (int aa = 0; aa < 2; ++aa) axis(n, m, aa, !aa || n <= 4 * m);
    printf("resize boxes ok: %ld checks\n", n_checks);
    return 0;
}

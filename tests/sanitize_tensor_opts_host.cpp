// sanitize_tensor_opts_host.cpp -- the host side of llicti_decode_images_tensor_o and kin (llicti_amd/csrc/host_plan.hpp: resolve_tensor_opts,
// resolve_tensor_padded; host_types.hpp: pad_index, tensor_window_pad_ok, pad_win_pack / pad_win_unpack) compiled by g++ alone, beside
// tests/sanitize_tensor_host.cpp.  What it holds, over a few thousand option / window combinations with the limits among them:
//   - pad_index never leaves 0 .. n - 1 (or -1, -2), and tensor_window_pad_ok is what a walk over EVERY coordinate of the window says
//   - every window the call takes packs into its two signed words and unpacks to the same origin and flag (the kernel's masks)
//   - every source pixel such a window reads lies inside the image's planes at the image's reduce
//   - the refusals and the image their message names: layout, pad mode, fill space, fill, size, origin, overhang; a pad mode without leave
// tests/test_tensor_layout_cpu.py builds it with -fsanitize=address,undefined -fno-sanitize-recover=all and runs it.
#include <stdio.h>
#include <stdlib.h>
#include <limits>

#include "../llicti_amd/csrc/host_plan.hpp"

static long n_checks = 0;
#define REQUIRE(c)                                                                      \
    do {                                                                                \
        ++n_checks;                                                                     \
        if (!(c)) { fprintf(stderr, "FAILED %s (%s:%d)\n", #c, __FILE__, __LINE__); exit(1); } \
    } while (0)

static const float kMean[3] = { 0.485f, 0.456f, 0.406f }, kStd[3] = { 0.229f, 0.224f, 0.225f };
static const int kModes[] = { LLICTI_PAD_NONE, LLICTI_PAD_CONSTANT, LLICTI_PAD_EDGE, LLICTI_PAD_REFLECT, LLICTI_PAD_SYMMETRIC };

// what the header's text says, coordinate by coordinate
static bool walk_ok(int n, int t0, int len, int mode)
{
    for (int k = 0; k < len; ++k) {
        const int s = pad_index(n, t0 + k, mode);
        REQUIRE(s >= -2 && s < n);
        if (s == -2) return false;
    }
    return true;
}

static void drive(int B, const int *Hs, const int *Ws, const int *rs)
{
    const Reduces rd = Reduces::each(rs);
    long taken = 0, refused = 0;
    for (int mode : kModes)
        for (int layout : { LLICTI_LAYOUT_NCHW, LLICTI_LAYOUT_NHWC })
            for (int space : { LLICTI_FILL_PIXEL, LLICTI_FILL_OUTPUT }) {
                int Hmin = 1 << 30, Wmin = 1 << 30;
                for (int b = 0; b < B; ++b) { Hmin = std::min(Hmin, reduced_dim(Hs[b], rs[b])); Wmin = std::min(Wmin, reduced_dim(Ws[b], rs[b])); }
                const int sizes[][2] = { { 1, 1 }, { Hmin, Wmin }, { Hmin + 3, Wmin + 5 }, { 2 * Hmin - 1, 2 * Wmin - 1 }, { 3 * Hmin, 3 * Wmin }, { 29, 32 } };
                for (const auto &hw : sizes) {
                    const int Ho = hw[0], Wo = hw[1];
                    // origins per image: inside, one pixel over each edge, at and one beyond the mirror limits, wholly outside
                    for (int pick = 0; pick < 9; ++pick) {
                        std::vector<int> y0(B), x0(B);
                        std::vector<uint8_t> flip(B);
                        for (int b = 0; b < B; ++b) {
                            const int Hr = reduced_dim(Hs[b], rs[b]), Wr = reduced_dim(Ws[b], rs[b]);
                            const int ys[] = { 0, -1, Hr - Ho + 1, -(Hr - 1), -Hr, -Hr - 1, Hr - Ho + Hr, Hr + 2, (Hr - Ho) / 2 };
                            const int xs[] = { 0, -1, Wr - Wo + 1, -(Wr - 1), -Wr, -Wr - 1, Wr - Wo + Wr, -Wo - 2, (Wr - Wo) / 2 };
                            y0[b] = ys[(pick + b) % 9]; x0[b] = xs[(pick + 2 * b) % 9]; flip[b] = (uint8_t)((b + pick) & 1);
                        }
                        const TensorArgs t{ LLICTI_T_F16, Ho, Wo, y0.data(), x0.data(), flip.data(), kMean, kStd };
                        const llicti_tensor_opts o{ layout, mode, space, { 124.0f, 116.0f, 104.0f } };
                        std::vector<uint32_t> wins;
                        TensorNorm nm;
                        TensorPad pad;
                        const int rc = resolve_tensor_padded("test", B, Hs, Ws, rd, t, o, wins, nm, pad);
                        int first_bad = -1;
                        for (int b = 0; b < B && first_bad < 0; ++b) {
                            const int Hr = reduced_dim(Hs[b], rs[b]), Wr = reduced_dim(Ws[b], rs[b]);
                            const bool in_limits = mode == LLICTI_PAD_NONE || (Ho <= 8160 && Wo <= 8160 && std::abs(y0[b]) <= 8160 && std::abs(x0[b]) <= 8160);
                            const bool ok = in_limits && walk_ok(Hr, y0[b], Ho, mode) && walk_ok(Wr, x0[b], Wo, mode);
                            REQUIRE(ok == tensor_window_pad_ok(Hs[b], Ws[b], rs[b], y0[b], x0[b], Ho, Wo, mode));
                            if (!ok) first_bad = b;
                        }
                        if (first_bad >= 0) {
                            char want[32];
                            snprintf(want, sizeof want, "image %d ", first_bad);
                            REQUIRE(rc == LLICTI_EINVAL && g_err.find(want) != std::string::npos);
                            ++refused;
                            continue;
                        }
                        ++taken;
                        REQUIRE(rc == 0 && (int)wins.size() == 2 * B && pad.layout == layout && pad.mode == mode && nm.on == 1);
                        if (mode != LLICTI_PAD_NONE) REQUIRE(pad.space == space && pad.fill[0] == 124.0f && pad.fill[2] == 104.0f);
                        for (int b = 0; b < B; ++b) {
                            int yy, xx;
                            bool ff;
                            pad_win_unpack(wins[2 * b], wins[2 * b + 1], yy, xx, ff);
                            REQUIRE(yy == y0[b] && xx == x0[b] && ff == (flip[b] != 0));
                            REQUIRE((wins[2 * b] >> 17) == 0 && (wins[2 * b + 1] >> 16) == 0);
                            const int Hr = reduced_dim(Hs[b], rs[b]), Wr = reduced_dim(Ws[b], rs[b]);
                            for (int t0 : { y0[b], y0[b] + Ho - 1 }) { const int s = pad_index(Hr, t0, mode); REQUIRE(s == -1 || (s >= 0 && (s << rs[b]) < Hs[b])); }
                            for (int t0 : { x0[b], x0[b] + Wo - 1 }) { const int s = pad_index(Wr, t0, mode); REQUIRE(s == -1 || (s >= 0 && (s << rs[b]) < Ws[b])); }
                        }
                    }
                }
            }
    REQUIRE(taken > 0 && refused > 0);
}

int main()
{
    // the index map by hand: n = 4
    const int want_reflect[] = { -2, 3, 2, 1, 0, 1, 2, 3, 2, 1, 0, -2 }, want_symm[] = { -2, 3, 2, 1, 0, 0, 1, 2, 3, 3, 2, 1, 0, -2 };
    for (int k = 0; k < 12; ++k) REQUIRE(pad_index(4, k - 4, LLICTI_PAD_REFLECT) == want_reflect[k]);
    for (int k = 0; k < 14; ++k) REQUIRE(pad_index(4, k - 5, LLICTI_PAD_SYMMETRIC) == want_symm[k]);
    REQUIRE(pad_index(4, -9, LLICTI_PAD_EDGE) == 0 && pad_index(4, 90, LLICTI_PAD_EDGE) == 3 && pad_index(4, -1, LLICTI_PAD_CONSTANT) == -1);
    REQUIRE(pad_index(4, 4, LLICTI_PAD_NONE) == -2 && pad_index(4, 3, LLICTI_PAD_NONE) == 3 && pad_index(4, -1, 9) == -2);
    REQUIRE(pad_index(1, 1, LLICTI_PAD_REFLECT) == -2 && pad_index(1, -1, LLICTI_PAD_REFLECT) == -2 && pad_index(1, 1, LLICTI_PAD_SYMMETRIC) == 0);
    REQUIRE(pad_index(0, 0, LLICTI_PAD_EDGE) == -2 && pad_index(8160, -8160, LLICTI_PAD_SYMMETRIC) == 8159 && pad_index(8160, 16319, LLICTI_PAD_SYMMETRIC) == 0);
    // the limits of the call
    REQUIRE(tensor_window_pad_ok(8160, 8160, 0, -8160, -8160, 8160, 8160, LLICTI_PAD_SYMMETRIC) && !tensor_window_pad_ok(8160, 8160, 0, -8161, 0, 8160, 8160, LLICTI_PAD_EDGE));
    REQUIRE(tensor_window_pad_ok(64, 64, 0, 8160, 8160, 8160, 8160, LLICTI_PAD_CONSTANT) && !tensor_window_pad_ok(64, 64, 0, 0, 8161, 4, 4, LLICTI_PAD_CONSTANT));
    REQUIRE(!tensor_window_pad_ok(64, 64, 0, 0, 0, 8161, 4, LLICTI_PAD_EDGE) && !tensor_window_pad_ok(64, 64, 0, 0, 0, 4, 0, LLICTI_PAD_EDGE));
    REQUIRE(!tensor_window_pad_ok(64, 64, 6, 0, 0, 4, 4, LLICTI_PAD_EDGE) && !tensor_window_pad_ok(64, 64, 0, 0, 0, 4, 4, 5) && !tensor_window_pad_ok(64, 64, 0, 0, 0, 4, 4, -1));
    REQUIRE(!tensor_window_pad_ok(64, 64, 0, 2147483647, 0, 2, 2, LLICTI_PAD_CONSTANT) && !tensor_window_pad_ok(64, 64, 0, 0, -2147483647 - 1, 2, 2, LLICTI_PAD_EDGE));
    REQUIRE(tensor_window_pad_ok(64, 64, 0, 60, 60, 4, 4, LLICTI_PAD_NONE) && !tensor_window_pad_ok(64, 64, 0, 61, 60, 4, 4, LLICTI_PAD_NONE));

    {
        const int Hs[] = { 67 }, Ws[] = { 93 }, r0[] = { 0 }, r2[] = { 2 };
        drive(1, Hs, Ws, r0);
        drive(1, Hs, Ws, r2);
    }
    {
        const int Hs[] = { 150, 96, 40 }, Ws[] = { 131, 160, 60 }, ra[] = { 0, 1, 0 }, rb[] = { 2, 0, 5 };
        drive(3, Hs, Ws, ra);
        drive(3, Hs, Ws, rb);
    }
    {
        const int Hs[] = { 8160, 32 }, Ws[] = { 32, 8160 }, ra[] = { 0, 0 };
        drive(2, Hs, Ws, ra);
    }

    // options by themselves
    TensorPad pad;
    auto opt = [&](int layout, int mode, int space, float f, bool pad_allowed) {
        const llicti_tensor_opts o{ layout, mode, space, { 0.0f, f, 0.0f } };
        return resolve_tensor_opts("test", o, pad_allowed, pad);
    };
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    REQUIRE(opt(LLICTI_LAYOUT_NHWC, LLICTI_PAD_NONE, 77, nan, true) == 0 && pad.layout == LLICTI_LAYOUT_NHWC && pad.mode == LLICTI_PAD_NONE);      // (no pad mode: space and fill are not read)
    REQUIRE(opt(LLICTI_LAYOUT_NHWC, LLICTI_PAD_NONE, 0, 0.0f, false) == 0);
    for (int bad : { -1, 2, 100 }) REQUIRE(opt(bad, LLICTI_PAD_NONE, 0, 0.0f, true) == LLICTI_EINVAL);
    for (int bad : { -1, 5, 100 }) REQUIRE(opt(LLICTI_LAYOUT_NCHW, bad, 0, 0.0f, true) == LLICTI_EINVAL);
    for (int bad : { -1, 2, 100 }) REQUIRE(opt(LLICTI_LAYOUT_NCHW, LLICTI_PAD_EDGE, bad, 0.0f, true) == LLICTI_EINVAL);
    for (float bad : { inf, -inf, nan }) REQUIRE(opt(LLICTI_LAYOUT_NCHW, LLICTI_PAD_CONSTANT, LLICTI_FILL_OUTPUT, bad, true) == LLICTI_EINVAL);
    for (int mode : { LLICTI_PAD_CONSTANT, LLICTI_PAD_EDGE, LLICTI_PAD_REFLECT, LLICTI_PAD_SYMMETRIC }) {
        REQUIRE(opt(LLICTI_LAYOUT_NHWC, mode, LLICTI_FILL_PIXEL, -3.5f, true) == 0 && pad.fill[1] == -3.5f);
        REQUIRE(opt(LLICTI_LAYOUT_NHWC, mode, LLICTI_FILL_PIXEL, 0.0f, false) == LLICTI_EINVAL);
    }
    REQUIRE(tensor_opts_plain(nullptr));
    const llicti_tensor_opts plain{ LLICTI_LAYOUT_NCHW, LLICTI_PAD_NONE, 9, { nan, nan, nan } }, nhwc{ LLICTI_LAYOUT_NHWC, LLICTI_PAD_NONE, 0, { 0, 0, 0 } };
    REQUIRE(tensor_opts_plain(&plain) && !tensor_opts_plain(&nhwc));

    // size, dtype, origin and normalisation of a padded call
    const int H1[] = { 64 }, W1[] = { 96 };
    std::vector<uint32_t> wins;
    TensorNorm nm;
    auto rc = [&](int dtype, int Ho, int Wo, int y, int x, int mode) {
        const TensorArgs t{ dtype, Ho, Wo, &y, &x, nullptr, nullptr, nullptr };
        const llicti_tensor_opts o{ LLICTI_LAYOUT_NHWC, mode, LLICTI_FILL_PIXEL, { 0, 0, 0 } };
        return resolve_tensor_padded("test", 1, H1, W1, 0, t, o, wins, nm, pad);
    };
    REQUIRE(rc(LLICTI_T_BF16, 8160, 8160, -8160, 8160, LLICTI_PAD_CONSTANT) == 0 && nm.on == 0);
    REQUIRE(rc(LLICTI_T_BF16, 8161, 4, 0, 0, LLICTI_PAD_CONSTANT) == LLICTI_EINVAL && rc(LLICTI_T_BF16, 4, 8161, 0, 0, LLICTI_PAD_EDGE) == LLICTI_EINVAL);
    REQUIRE(rc(LLICTI_T_BF16, 0, 4, 0, 0, LLICTI_PAD_EDGE) == LLICTI_EINVAL && rc(7, 4, 4, 0, 0, LLICTI_PAD_EDGE) == LLICTI_EINVAL);
    REQUIRE(rc(LLICTI_T_F32, 4, 4, -8161, 0, LLICTI_PAD_EDGE) == LLICTI_EINVAL && g_err.find("image 0 ") != std::string::npos);
    REQUIRE(rc(LLICTI_T_F32, 4, 4, 0, 8161, LLICTI_PAD_CONSTANT) == LLICTI_EINVAL && rc(LLICTI_T_F32, 4, 4, 2147483647, 0, LLICTI_PAD_CONSTANT) == LLICTI_EINVAL);
    REQUIRE(rc(LLICTI_T_F32, 64, 96, -63, -95, LLICTI_PAD_REFLECT) == 0 && rc(LLICTI_T_F32, 64, 96, -64, -95, LLICTI_PAD_REFLECT) == LLICTI_EINVAL);
    REQUIRE(rc(LLICTI_T_F32, 64, 96, 64, 96, LLICTI_PAD_SYMMETRIC) == 0 && rc(LLICTI_T_F32, 64, 96, 64, 97, LLICTI_PAD_SYMMETRIC) == LLICTI_EINVAL);
    REQUIRE(rc(LLICTI_T_F32, 64, 96, 0, 0, LLICTI_PAD_NONE) == 0 && rc(LLICTI_T_F32, 64, 96, 0, 1, LLICTI_PAD_NONE) == LLICTI_EINVAL && g_err.find("leaves image 0 ") != std::string::npos);
    printf("tensor options ok: %ld checks\n", n_checks);
    return 0;
}

// sanitize_tensor_host.cpp -- the host side of llicti_decode_images_tensor (llicti_amd/csrc/host_plan.hpp: resolve_tensor; host_types.hpp:
// tensor_window_ok, tensor_win_pack, tensor_elem_bytes) compiled by g++ alone, beside tests/sanitize_px_host.cpp.  What it holds:
//   - the windows of a call are validated WITHOUT a plan (resolve_tensor takes none: they are kernel arguments, no part of a plan or its key)
//   - every legal window packs into its word and unpacks to the same origin and flag (the kernel's masks), for sizes up to 8160 and every reduce
//   - the refusals: unknown dtype, Ho / Wo < 1, a window one row or column too far (the message names the image), one of mean / std alone,
//     a std that is zero, negative, infinite or NaN
// tests/test_tensor_cpu.py builds it plain; under sanitizers:
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -o /tmp/sth tests/sanitize_tensor_host.cpp && /tmp/sth
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

static void drive(int B, const int *Hs, const int *Ws, int nlev)
{
    for (int r = 0; r <= nlev; ++r) {
        int Hmin = 1 << 30, Wmin = 1 << 30;
        for (int b = 0; b < B; ++b) { Hmin = std::min(Hmin, reduced_dim(Hs[b], r)); Wmin = std::min(Wmin, reduced_dim(Ws[b], r)); }
        const int sizes[][2] = { { Hmin, Wmin }, { 1, 1 }, { std::max(1, Hmin - 1), std::max(1, Wmin / 2) } };
        for (const auto &hw : sizes) {
            const int Ho = hw[0], Wo = hw[1];
            std::vector<int> y0(B), x0(B);
            std::vector<uint8_t> flip(B);
            for (int b = 0; b < B; ++b) { y0[b] = reduced_dim(Hs[b], r) - Ho; x0[b] = (reduced_dim(Ws[b], r) - Wo) / (b + 1); flip[b] = (uint8_t)((b & 1) * 7); }
            std::vector<uint32_t> wins;
            TensorNorm nm;
            for (int dtype : { LLICTI_T_F32, LLICTI_T_F16, LLICTI_T_BF16 }) {
                const TensorArgs t{ dtype, Ho, Wo, y0.data(), x0.data(), flip.data(), kMean, kStd };
                REQUIRE(resolve_tensor("test", B, Hs, Ws, r, t, wins, nm) == 0);
                REQUIRE((int)wins.size() == B && nm.on == 1 && nm.mean[1] == kMean[1] && nm.std[2] == kStd[2]);
                for (int b = 0; b < B; ++b) {                   // (the kernel's masks)
                    REQUIRE((int)(wins[b] & 0x1FFFu) == y0[b] && (int)((wins[b] >> 13) & 0x1FFFu) == x0[b] && ((wins[b] >> 26) & 1u) == (flip[b] ? 1u : 0u));
                    REQUIRE((wins[b] >> 27) == 0);
                    // the last plane pixel the window reads lies inside the image
                    REQUIRE(((y0[b] + Ho - 1) << r) < Hs[b] && ((x0[b] + Wo - 1) << r) < Ws[b]);
                }
            }
            const TensorArgs plain{ LLICTI_T_F32, Ho, Wo, nullptr, nullptr, nullptr, nullptr, nullptr };      // NULL arrays: the corner, no flip, no normalisation
            REQUIRE(resolve_tensor("test", B, Hs, Ws, r, plain, wins, nm) == 0 && nm.on == 0);
            for (int b = 0; b < B; ++b) REQUIRE(wins[b] == 0);
            // one row / one column too far, on the last image alone: refused, and the message names it
            TensorArgs t{ LLICTI_T_F32, Ho, Wo, y0.data(), x0.data(), nullptr, nullptr, nullptr };
            y0[B - 1] += 1;
            REQUIRE(resolve_tensor("test", B, Hs, Ws, r, t, wins, nm) == LLICTI_EINVAL);
            char want[32];
            snprintf(want, sizeof want, "image %d ", B - 1);
            REQUIRE(g_err.find(want) != std::string::npos);
            y0[B - 1] -= 1;
            x0[0] = reduced_dim(Ws[0], r) - Wo + 1;
            REQUIRE(resolve_tensor("test", B, Hs, Ws, r, t, wins, nm) == LLICTI_EINVAL && g_err.find("image 0 ") != std::string::npos);
            x0[0] = -1;
            REQUIRE(resolve_tensor("test", B, Hs, Ws, r, t, wins, nm) == LLICTI_EINVAL);
            x0[0] = 0;
            REQUIRE(resolve_tensor("test", B, Hs, Ws, r, t, wins, nm) == 0);
        }
        // a window larger than the smallest image fits nowhere
        const TensorArgs big{ LLICTI_T_F32, Hmin + 1, Wmin, nullptr, nullptr, nullptr, nullptr, nullptr };
        std::vector<uint32_t> wins;
        TensorNorm nm;
        REQUIRE(resolve_tensor("test", B, Hs, Ws, r, big, wins, nm) == LLICTI_EINVAL);
    }
}

int main()
{
    REQUIRE(tensor_elem_bytes(LLICTI_T_F32) == 4 && tensor_elem_bytes(LLICTI_T_F16) == 2 && tensor_elem_bytes(LLICTI_T_BF16) == 2);
    for (int bad : { -1, 3, 7, 255 }) REQUIRE(tensor_elem_bytes(bad) == 0);
    REQUIRE(tensor_window_ok(8160, 8160, 0, 8159, 8159, 1, 1) && !tensor_window_ok(8160, 8160, 0, 8160, 0, 1, 1));
    REQUIRE(tensor_win_pack(8159, 8159, true) == (8159u | (8159u << 13) | (1u << 26)));
    REQUIRE(!tensor_window_ok(64, 64, 0, 2147483647, 0, 2, 2) && !tensor_window_ok(64, 64, 0, 0, 0, 2147483647, 2));
    REQUIRE(!tensor_window_ok(64, 64, 6, 0, 0, 1, 1) && !tensor_window_ok(64, 64, -1, 0, 0, 1, 1) && tensor_window_ok(64, 64, 5, 1, 1, 1, 1));
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
    // dtype, size, mean / std
    const int H1[] = { 64 }, W1[] = { 96 };
    std::vector<uint32_t> wins;
    TensorNorm nm;
    auto rc = [&](int dtype, int Ho, int Wo, const float *mean, const float *sd) {
        const TensorArgs t{ dtype, Ho, Wo, nullptr, nullptr, nullptr, mean, sd };
        return resolve_tensor("test", 1, H1, W1, 0, t, wins, nm);
    };
    REQUIRE(rc(LLICTI_T_F16, 64, 96, kMean, kStd) == 0);
    for (int bad : { -1, 3, 7 }) REQUIRE(rc(bad, 64, 96, nullptr, nullptr) == LLICTI_EINVAL);
    REQUIRE(rc(LLICTI_T_F32, 0, 96, nullptr, nullptr) == LLICTI_EINVAL && rc(LLICTI_T_F32, 64, 0, nullptr, nullptr) == LLICTI_EINVAL);
    REQUIRE(rc(LLICTI_T_F32, -2, -2, nullptr, nullptr) == LLICTI_EINVAL && rc(LLICTI_T_F32, 65, 96, nullptr, nullptr) == LLICTI_EINVAL);
    REQUIRE(rc(LLICTI_T_F32, 64, 96, kMean, nullptr) == LLICTI_EINVAL && rc(LLICTI_T_F32, 64, 96, nullptr, kStd) == LLICTI_EINVAL);
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    for (float v : { 0.0f, -0.0f, -1.0f, inf, -inf, nan })
        for (int k = 0; k < 3; ++k) {
            float sd[3] = { kStd[0], kStd[1], kStd[2] };
            sd[k] = v;
            REQUIRE(rc(LLICTI_T_F32, 64, 96, kMean, sd) == LLICTI_EINVAL);
        }
    const float tiny[3] = { std::numeric_limits<float>::denorm_min(), 1.0f, std::numeric_limits<float>::max() };      // finite and above zero: taken
    REQUIRE(rc(LLICTI_T_F32, 64, 96, kMean, tiny) == 0 && nm.std[0] == tiny[0]);
    printf("tensor windows ok: %ld checks\n", n_checks);
    return 0;
}

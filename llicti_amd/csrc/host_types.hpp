// host_types.hpp -- what the HOST side of the library and the kernels share: error reporting, geometry structs (one image, one level,
// one stage of a whole-batch call), stream descriptors and the constants of the container formats.  Plain C++17 with no HIP dependency:
// g++ compiles this file and host_plan.hpp under AddressSanitizer / UBSan (tests/sanitize_host.sh).  In the HIP build it is part of the
// single translation unit llicti_hip.hip (included through common.hpp).
#pragma once
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <algorithm>
#include <string>
#include <vector>

#include "../../include/llicti_hip.h"

#if defined(__HIPCC__)
#define LLICTI_HD __host__ __device__ __forceinline__
#else
#define LLICTI_HD inline
#endif

// ------------------------------------------------------------------------------------------------ errors
static thread_local std::string g_err;
static int fail(int code, const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}



// ------------------------------------------------------------------------------------------------ geometry
struct Geom {
    int B, H, W, lvl;
    int Hl, Wl, h, w, padH, padW;
    long plane;   // H*W
    // Whole-batch calls keep one Geom PER IMAGE in a device table (the images of a call may differ in size: llicti_encode_images_v); these two
    // fields are only meaningful there.  The kernel-level entry points pass one Geom by value and derive both from the image index.
    long pix_off; // first element of the image's [3][H][W] block in planes / fplanes
    long par_off; // first float of the image's [64][h * w] block in the CNN-output buffer of this level
};
// One image of a whole-batch call (device table, llicti_hip.hip: Plan).
struct ImgGeo {
    int H, W, h4, w4, padint, hdr_bytes;      // hdr_bytes = 17 + 3 h4 w4 (LLICTI_nets.py:347-350)
    int M, sbase;                             // rANS containers: the image's stream count (its header says so: images of one call may differ) and its first stream
    int byte0;                                // header byte 0 of its container (AC: the number of scales; rANS: the tag)
    int Mlo;                                  // "auto" xwide encodes (LLICTI_MODE_RANS_X_AUTO): the count the image's size gives; M is then the LARGEST the encoder may
                                              // pick -- it picks per image, on the device, from what the image's last stage costs (rans_auto_hi / rans_auto_min,
                                              // choose_streams_kernel) -- and the table holds M streams for it.  0: the count is M, fixed by the caller
    int dcs;                                  // pixel stride of the raw DC band (the last level's x00: 2 << (L - 1), 32 for config A)
    int nseg;                                 // container segments of the model: 4 + 9 L
    long plane;                               // H * W
    long pix_off;                             // first element of the image's [3][H][W] block in planes / fplanes (workspace)
    long rgb_off;                             // first byte of its [3][H][W] block in the caller's RGB buffer
};
// One image's OUTPUT of a reduced-resolution decode (llicti_decode_images_reduced; device table of the call's plan, behind the tables above):
// the pixels whose row and column are multiples of 2^r, planar uint8 [3][Hr][Wr] at byte `off` of the caller's buffer.
struct RedGeo {
    long off;
    int Hr, Wr;                               // ceil(H / 2^r), ceil(W / 2^r)
};
LLICTI_HD int reduced_dim(int n, int r) { return (n + (1 << r) - 1) >> r; }
// One image's window in the caller's INTERLEAVED pixel buffer (llicti_encode_images_px / llicti_decode_images_px; device table of the call's
// plan, behind the tables above): pixel (i, j) of the window is the bpp bytes at off + i * pitch + j * bpp.  fmt: LLICTI_PIX_* -- bit 0 says
// blue comes first, bit 1 that a fourth byte (alpha: ignored by the encoder, written as 255 by the decoder) follows the three colours.
struct PixGeo {
    long off;                                 // first byte of the window's first pixel
    int pitch;                                // bytes from one row of the window to the next (>= W * bpp)
    int fmt;
};
LLICTI_HD int pix_bpp(int fmt) { return 3 + (fmt >> 1); }            // of a VALID format (host: pix_format_bytes checks)
LLICTI_HD bool pix_bgr(int fmt) { return (fmt & 1) != 0; }
// Float tensor output (llicti_decode_images_tensor).  The windows of a call -- origin and flip flag of every image -- are PER CALL data: a
// training loop draws new ones for every batch, so they are no part of the plan (a plan per call would thrash the cache) but KERNEL ARGUMENTS
// of unlift_tensor_kernel: one packed word per image, kTensorWinMax images per launch (a larger batch takes several launches).
constexpr int kTensorWinMax = 256;
struct TensorWins { uint32_t w[kTensorWinMax]; };                    // y0 | x0 << 13 | flip << 26 (origins are below 8160 < 2^13)
struct TensorNorm { float mean[3], std[3]; int on; };                // on = 0: no normalisation
LLICTI_HD uint32_t tensor_win_pack(int y0, int x0, bool flip) { return (uint32_t)y0 | ((uint32_t)x0 << 13) | ((flip ? 1u : 0u) << 26); }
LLICTI_HD int tensor_elem_bytes(int dtype) { return dtype == LLICTI_T_F32 ? 4 : (dtype == LLICTI_T_F16 || dtype == LLICTI_T_BF16) ? 2 : 0; }
// an Ho x Wo window at (y0, x0) of an H x W image decoded at reduce r lies inside it
LLICTI_HD bool tensor_window_ok(int H, int W, int r, int y0, int x0, int Ho, int Wo)
{
    if (H < 1 || W < 1 || r < 0 || r > LLICTI_NLEVELS || Ho < 1 || Wo < 1 || y0 < 0 || x0 < 0) return false;
    return (long)y0 + Ho <= reduced_dim(H, r) && (long)x0 + Wo <= reduced_dim(W, r);
}
// Tensor options (llicti_decode_images_tensor_o and kin): the output's layout and, for windows, the padding past the image.  Per call data like
// the windows: `TensorPad` is a kernel argument of the sink_* kernels, and a padded window takes TWO words per image (PadWins) -- its origins
// are signed, -8160 .. 8160, and do not fit tensor_win_pack's 13 bits: [2 b] = (y0 + 8192) | flip << 16, [2 b + 1] = x0 + 8192.
constexpr int kPadWinMax = 128;                                      // images per launch of sink_window_kernel
constexpr int kPadOriginBias = 8192, kPadOriginMax = 8160;
struct PadWins { uint32_t w[2 * kPadWinMax]; };
struct TensorPad { int layout, mode, space; float fill[3]; };        // LLICTI_LAYOUT_*, LLICTI_PAD_*, LLICTI_FILL_*
LLICTI_HD void pad_win_pack(int y0, int x0, bool flip, uint32_t *words)
{
    words[0] = (uint32_t)(y0 + kPadOriginBias) | ((flip ? 1u : 0u) << 16);
    words[1] = (uint32_t)(x0 + kPadOriginBias);
}
LLICTI_HD void pad_win_unpack(uint32_t w0, uint32_t w1, int &y0, int &x0, bool &flip)
{
    y0 = (int)(w0 & 0xFFFFu) - kPadOriginBias; x0 = (int)(w1 & 0xFFFFu) - kPadOriginBias; flip = ((w0 >> 16) & 1u) != 0;
}
// The index map of one axis of a padded window (include/llicti_hip.h states it): coordinate t on an axis of n pixels -> the source index in
// 0 .. n - 1, -1 for "fill", -2 for refused.  ONE function for the kernel and llicti_pad_index (the host).  |t| <= 2^30.
LLICTI_HD int pad_index(int n, int t, int mode)
{
    if (n < 1) return -2;
    if (t >= 0 && t < n) return t;
    const int over = t < 0 ? -t : t - (n - 1);                       // pixels past the side, >= 1
    switch (mode) {
    case LLICTI_PAD_CONSTANT: return -1;
    case LLICTI_PAD_EDGE: return t < 0 ? 0 : n - 1;
    case LLICTI_PAD_REFLECT: return over > n - 1 ? -2 : t < 0 ? -t : 2 * (n - 1) - t;
    case LLICTI_PAD_SYMMETRIC: return over > n ? -2 : t < 0 ? -t - 1 : 2 * n - 1 - t;
    default: return -2;                                              // (LLICTI_PAD_NONE: the window leaves its image; an unknown mode)
    }
}
// llicti_decode_images_tensor_o takes an Ho x Wo window at (y0, x0) of an H x W image decoded at reduce r under pad mode `mode`: sizes 1 .. 8160,
// origins -8160 .. 8160, and both ends of either axis map somewhere (the overhang grows monotonically towards a window's ends)
LLICTI_HD bool tensor_window_pad_ok(int H, int W, int r, int y0, int x0, int Ho, int Wo, int mode)
{
    if (mode == LLICTI_PAD_NONE) return tensor_window_ok(H, W, r, y0, x0, Ho, Wo);
    if (mode < LLICTI_PAD_NONE || mode > LLICTI_PAD_SYMMETRIC) return false;
    if (H < 1 || W < 1 || r < 0 || r > LLICTI_NLEVELS || Ho < 1 || Wo < 1 || Ho > 8160 || Wo > 8160) return false;
    if (y0 < -kPadOriginMax || y0 > kPadOriginMax || x0 < -kPadOriginMax || x0 > kPadOriginMax) return false;
    const int Hr = reduced_dim(H, r), Wr = reduced_dim(W, r);
    return pad_index(Hr, y0, mode) != -2 && pad_index(Hr, y0 + Ho - 1, mode) != -2 && pad_index(Wr, x0, mode) != -2 && pad_index(Wr, x0 + Wo - 1, mode) != -2;
}
// Resized crops (llicti_decode_images_tensor_resized): image b's source BOX -- origin, extent, flip, in the coordinates of the decoded image --
// is resampled to Ho x Wo by unlift_resize_tensor_kernel.  Per call data like the windows above: two packed words per image (origins and
// extents are at most 8160 < 2^13), kResizeBoxMax images per launch.
constexpr int kResizeBoxMax = 128;
constexpr int kResizeTapMax = 9;                                     // taps of one output index along an axis, at a scale of at most 4 with the filter on
struct ResizeBoxes { uint32_t w[2 * kResizeBoxMax]; };               // [2 b]: y0 | x0 << 13 | flip << 26 (tensor_win_pack); [2 b + 1]: hs | ws << 13
LLICTI_HD uint32_t resize_ext_pack(int hs, int ws) { return (uint32_t)hs | ((uint32_t)ws << 13); }
// Views (llicti_decode_images_tensor_views): a view is such a box of the image it NAMES -- three words per view, kViewMax views per launch of
// unlift_views_tensor_kernel (a longer group takes several launches).  The image index has a word of its own: a batch has no upper bound.
constexpr int kViewMax = 128;
constexpr int kViewCountMax = 1 << 20;                               // views of one group
struct ViewSlice { uint32_t w[3 * kViewMax]; };                      // [3 v]: tensor_win_pack; [3 v + 1]: resize_ext_pack; [3 v + 2]: the image's index
// an hs x ws box at (y0, x0) of an H x W image decoded at reduce r lies inside it, and the resampling to Ho x Wo is one the kernel does: output
// sizes 1 .. 8160, the filter flag 0 or 1, and with the filter on a scale of at most 4 per axis (hs <= 4 Ho, ws <= 4 Wo: kResizeTapMax taps)
LLICTI_HD bool resize_window_ok(int H, int W, int r, int y0, int x0, int hs, int ws, int Ho, int Wo, int antialias)
{
    if (H < 1 || W < 1 || r < 0 || r > LLICTI_NLEVELS || hs < 1 || ws < 1 || y0 < 0 || x0 < 0) return false;
    if (Ho < 1 || Wo < 1 || Ho > 8160 || Wo > 8160 || (antialias != 0 && antialias != 1)) return false;
    if ((long)y0 + hs > reduced_dim(H, r) || (long)x0 + ws > reduced_dim(W, r)) return false;
    return !antialias || ((long)hs <= 4L * Ho && (long)ws <= 4L * Wo);
}
// The triangle filter of one axis (PIL's and torch's bilinear, align_corners = False): a box extent of n source pixels resampled to m, output
// index i -> the tap count; *lo: the first source index; w[0 .. cap - 1]: the weights of taps lo, lo + 1, ..., zeros behind the last tap.  The
// rule, every operation fp32 and rounded once (include/llicti_hip.h states it; no contraction: the build's -ffp-contract=off):
//   scale = n / m; support = (antialias && scale > 1) ? scale : 1; center = scale (i + 0.5); lo = max(0, (int)(center - support + 0.5));
//   hi = min(n, (int)(center + support + 0.5)); t_k = max(0, 1 - |(k - center + 0.5) / support|); w_k = t_k / (t_lo + ... + t_hi-1).
// ONE function for the kernel (w in LDS) and llicti_resize_axis (the host): the weights a test reads here are the kernel's.
LLICTI_HD float resize_tap(int k, float center, float inv)
{
    const float d = (((float)k - center) + 0.5f) * inv;
    const float t = 1.0f - (d < 0.0f ? -d : d);
    return t > 0.0f ? t : 0.0f;
}
LLICTI_HD int resize_axis(int n, int m, int antialias, int i, int *lo_out, float *w, int cap)
{
    const float scale = (float)n / (float)m;
    const float support = (antialias && scale > 1.0f) ? scale : 1.0f;
    const float inv = 1.0f / support;
    const float center = scale * ((float)i + 0.5f);
    int lo = (int)((center - support) + 0.5f), hi = (int)((center + support) + 0.5f);
    if (lo < 0) lo = 0;
    if (hi > n) hi = n;
    float total = 0.0f;
    for (int k = lo; k < hi; ++k) total = total + resize_tap(k, center, inv);
    for (int k = 0; k < cap; ++k) w[k] = (lo + k < hi) ? resize_tap(lo + k, center, inv) / total : 0.0f;
    *lo_out = lo;
    return hi - lo;
}
static Geom make_geom(int B, int H, int W, int lvl)
{
    Geom g;
    g.B = B; g.H = H; g.W = W; g.lvl = lvl;
    const int st = 1 << lvl;
    g.Hl = (H + st - 1) / st;
    g.Wl = (W + st - 1) / st;
    g.h = (g.Hl + 1) / 2;
    g.w = (g.Wl + 1) / 2;
    g.padH = g.Hl & 1;
    g.padW = g.Wl & 1;
    g.plane = (long)H * W;
    g.pix_off = 0; g.par_off = 0;
    return g;
}
static void coded_dims(const Geom &g, int band, int *hc, int *wc)
{
    *hc = (band == 0 || band == 2) ? g.h - g.padH : g.h;   // LLICTI_nets.py:396-397
    *wc = (band == 0 || band == 1) ? g.w - g.padW : g.w;
}
static int check_dims(int B, int H, int W)
{
    if (B < 1 || H < 32 || W < 32 || H > 8160 || W > 8160) return fail(LLICTI_EINVAL, "bad shape B=%d H=%d W=%d (need B>=1, 32<=H,W<=8160)", B, H, W);
    return 0;
}


// ------------------------------------------------------------------------------------------------ stages, streams, tiles
struct StageGeom {      // one (level, band): band grid, coded crop, full-res addressing
    int B, H, W, lvl, h, w, hc, wc, oi, oj;
    long plane;
    uint32_t wc_mul;    // n / wc for 0 <= n < 2^31 without a division: div_by_magic(n, wc_mul, wc_sh)
    int wc_sh;
    // Per-image placement (whole-batch calls keep one StageGeom per image in a device table -- the images of a call may differ in size; a
    // kernel-level entry point passes ONE by value and stage_at() derives these from the image index):
    long img_off;       // first element of the image's [3][H][W] block in planes / fplanes
    long par_off;       // first float of its [64][h * w] block in the CNN-output buffer of this (level, band)
    long pair_off;      // first pair of its Y stream in the (level, band)'s pairs [clr][image][n] ...
    long pair_cs;       // ... and the distance between two colour channels there (the images' coded positions together)
};
// exact unsigned division by an invariant divisor (Granlund / Montgomery, the 33-bit multiplier form), 1 <= d < 2^31,
// 0 <= n < 2^31: l = ceil(log2 d), mul = floor(2^32 (2^l - d) / d) + 1, t = mulhi(n, mul), q = (t + ((n - t) >> 1)) >> (l - 1).
// d == 1 has no 33-bit form with a non-negative shift: it is encoded as (mul, sh) = (0, -1) and div_by_magic() returns n.
static void div_magic(uint32_t d, uint32_t *mul, int *sh)
{
    int l = 0;
    while ((1ull << l) < d) ++l;                                   // l = ceil(log2 d)
    if (l == 0) { *mul = 0; *sh = -1; return; }                     // d == 1
    *mul = (uint32_t)(((1ull << 32) * ((1ull << l) - d)) / d + 1);
    *sh = l - 1;
}
LLICTI_HD uint32_t div_by_magic(uint32_t n, uint32_t mul, int sh)
{
    if (sh < 0) return n;
#if defined(__HIP_DEVICE_COMPILE__)
    const uint32_t t = __umulhi(n, mul);
#else
    const uint32_t t = (uint32_t)(((uint64_t)n * mul) >> 32);
#endif
    return (t + ((n - t) >> 1)) >> sh;
}
LLICTI_HD int div_wc(const StageGeom &s, int n) { return (int)div_by_magic((uint32_t)n, s.wc_mul, s.wc_sh); }
// host self-test (llicti_selftest): every divisor of the format's range against '/', at the values where a magic division breaks first
static int selftest_div_magic()
{
    for (uint32_t d = 1; d <= 8192; ++d) {
        uint32_t mul; int sh;
        div_magic(d, &mul, &sh);
        const uint32_t probes[] = { 0u, 1u, d - 1, d, d + 1, 2 * d - 1, 2 * d, 4080u * 4080u - 1, 4080u * 4080u, (1u << 24) - 1, (1u << 24) + d,
                                    0x7FFFFFFFu / d * d - 1, 0x7FFFFFFFu / d * d, 0x7FFFFFFFu };
        for (uint32_t n : probes) if ((n >> 31) == 0 && div_by_magic(n, mul, sh) != n / d) return (int)d;
        for (uint32_t k = 0; k < 4096; ++k) { const uint32_t n = k * 524287u + d; if ((n >> 31) == 0 && div_by_magic(n, mul, sh) != n / d) return (int)d; }
    }
    return 0;
}
static StageGeom make_stage(const Geom &g, int band)
{
    static const int OI[4] = { 0, 1, 0, 1 }, OJ[4] = { 0, 1, 1, 0 };
    StageGeom s;
    s.B = g.B; s.H = g.H; s.W = g.W; s.lvl = g.lvl; s.h = g.h; s.w = g.w; s.plane = g.plane;
    coded_dims(g, band, &s.hc, &s.wc);
    s.oi = OI[band + 1]; s.oj = OJ[band + 1];
    div_magic((uint32_t)s.wc, &s.wc_mul, &s.wc_sh);
    s.img_off = g.pix_off; s.par_off = g.par_off; s.pair_off = 0; s.pair_cs = 0;
    return s;
}

struct StreamDesc {     // one arithmetic-coded stream of the whole-batch encoder
    long pair_off;      // first (c_low, c_high) pair, in uint32 units
    long out_off;       // slot offset in bytes
    int n;              // symbols
    int cap;            // slot capacity in bytes
};


struct TileRef { int img, yx; };        // one tile of a mixed-size band-CNN launch: image, tile row << 16 | tile column
struct StreamRef { int b, m, M, sbase; };   // one rANS stream of a call: image, stream of the image, the image's stream count, the image's first stream

// ------------------------------------------------------------------------------------------------ container format constants
constexpr int kLiftMaxParts = 65536;        // entries of the partials scratch: B * gridDim.x <= this

constexpr int kAnchorRow = 208;

constexpr int kRansStateBits = 31;
constexpr int kRansTailMax = 2047;          // tail symbols of a 64- / 128-lane stream (the 11-bit T field)
constexpr int kRansTailBlock = 32;          // xwide v4: a tail is a multiple of 32 symbols (or the stream's whole share of the last stage): its field is T / 32 rounded up, 8 bits
constexpr int kRansTailMaxX = 255 * kRansTailBlock;      // 8,160: ... of an xwide stream
constexpr int kRansSpillMax = 512;          // xwide v4: bits by which the tail coder's output may exceed the payload (< 32 symbols x 16 bits); they lie at the bottom of the main bit region
// A stream has 64 Q lanes: Q = 1, Q = 2 ("wide" streams: two 64-symbol sub-chunks per step, decoded two lanes per symbol by
// rans_decode_stage_pair_kernel, at the price of a tail twice as long) or Q = 4 ("xwide": 256 lanes, decoded ONE lane per symbol by
// rans_decode_stage_lane_kernel, four wavefronts per stream).  Symbol n of a stage sits in chunk n / 64Q.
template <int Q> struct RansGeo {
    static constexpr int kLanes = 64 * Q;
    static constexpr int kPayBits = kLanes * kRansStateBits;      // 1984 / 3968 / 7936: what the initial states carry (the tail stream)
    static constexpr int kPayBytes = kPayBits / 8;                // 248 / 496 / 992
    static constexpr int kPayDw = (kPayBits + 31) / 32;           // 62 / 124 / 248
    static constexpr int kMinStream = 2 + kPayBytes;              // T | pad (xwide v4: the header field under its end marker -- ten bits of the bit region), states
};
constexpr int kRansPayBytesMax = RansGeo<4>::kPayBytes;
constexpr int kPhiLutN = 2048;                   // the lane decoder's hint table (llicti_ctx::d_phi_lut)
constexpr double kPhiLutZ = 6.0;
// xwide streams (Q = 4) only, "v4" since round 6 -- the older stream kinds keep their v3 bytes (spec: oracle/llicti_oracle.h, "tail, xwide v4").
//   arena    the tail coder's output is not cut to the payload: tail symbols are taken (j = 0: the stream's last) until, at a multiple of 32, the
//            output has reached the payload's 7,936 bits; what exceeds them (the "spill", < 512 bits) lies at the bottom of the main bit region,
//            where the main decoder -- reading down -- leaves it: its final cursor IS the spill's length;
//   chains   one or two (the encoder's integer rule on the stream's last 64 symbols; bit 8 of the header field = one).  Two: seeded as in v3 --
//            A = number of symbol values of the image's Cg channel, n = rans_seed_count(A), chain A starts from 2^31 | sum sym(i) A^i (i < n),
//            chain B from that of sym(n + i), symbol j >= 2 n on A if j is even -- states in the arena's lowest and highest 32 bits, fields
//            towards each other.  One: the chain starts from x = sym(0), raw, and emits nothing while its state is below the interval; fields
//            up from bit 32, one end-marker bit above the last -- the arena's highest set bit;
//   header   on top of the bit region: 8 bits ceil(T / 32), 1 bit "one chain", 1 end-marker bit, zeros to the byte boundary.
template <int Q> constexpr bool kSeeded = (Q == 4);
constexpr int kSeedMax = 31;
LLICTI_HD int rans_seed_count(int A, uint32_t &pw)      // n and A^n
{
    int n = 0;
    uint64_t p = 1;
    while (n < kSeedMax && p * (uint64_t)A <= (1ull << 31)) { p *= (uint64_t)A; ++n; }
    pw = (uint32_t)p;
    return n;
}

// symbols of stream m in a stage of nc symbols (chunks of L symbols m, m + M, ...; only the stage's last chunk can be partial)
LLICTI_HD int rans_stream_count(int nc, int m, int M, int L)
{
    const int nchunks = (nc + L - 1) / L;
    if (nchunks <= m) return 0;
    const int K = (nchunks - m + M - 1) / M;
    const int last = m + (K - 1) * M;
    return L * K - ((last == nchunks - 1 && (nc % L)) ? L - (nc % L) : 0);
}
// ... and its inverse: the position in the stage of stream m's q-th symbol, q < rans_stream_count(nc, m, M, L) -- over the streams every position
// below nc exactly once, rising with q (tests/sanitize_host.cpp holds the two against each other)
LLICTI_HD int rans_stream_pos(int q, int m, int M, int L) { return L * (m + (q / L) * M) + (q % L); }
// xwide v4: which of a stream's tail symbols sits where, counted from the stream's end (j = 0: its last symbol).  The first NS are the raw
// symbols in the chains' start states (chain c's digit d at j = c sn + d), the ncod behind them are coded, alternating between the chains.
// The encoder and the tail decoder both take it from here -- their agreement is what makes a stream decodable (tests/sanitize_host.cpp
// holds the counts and the indices against each other).
struct SeededTailShape {
    int nch, sn, NS, ncod;                      // chains; raw symbols in a chain's start state (n per chain of two, the stream's last symbol for one chain); seed symbols; coded symbols
    LLICTI_HD int chain_count(int c) const { return (ncod + nch - 1 - c) / nch; }      // coded symbols of chain c (chain 0 never has fewer than chain 1)
    LLICTI_HD int index(int c, int i) const { return nch * sn + c + nch * i; }         // j of chain c's i-th coded symbol, in coding order
    LLICTI_HD int seed_index(int c, int d) const { return c * sn + d; }                // j of digit d < sn of chain c's start state (a symbol of the stream if < NS)
};
// cnt: the stream's symbols of the last stage; tall: its tail symbols, or the encoder's candidates (tall <= cnt); ns = rans_seed_count(A).
// (seeded = false: a 64- / 128-lane stream's tail to the tail decoder -- one chain that starts from no symbol, all of the tail coded)
LLICTI_HD SeededTailShape seeded_tail_shape(int cnt, int tall, int nch, int ns, bool seeded = true)
{
    SeededTailShape s;
    s.nch = nch;
    s.sn = !seeded ? 0 : (nch == 2) ? ns : 1;
    const int held = nch * s.sn;
    s.NS = held < cnt ? held : cnt;
    const int rest = tall - s.NS;
    s.ncod = rest > 0 ? rest : 0;
    return s;
}


// M <= 32: stream m is segment 4 + m of the container.  M = 64 / 128 (latency modes for single / large images; the reference's list
// has 45 stream slots): G = M / 32 streams share segment 4 + m / G = G little-endian u32 stream lengths, then the G streams.
LLICTI_HD int rans_group(int M) { return M > 32 ? M / 32 : 1; }

// "auto" xwide encodes: the stream count of an image is chosen by the ENCODER, per image, from the image itself -- its size (Mlo, the caller's
// rule: llicti_amd.codec.image_streams, sized for natural-like content at ~4.7 bytes per stream) and what the symbols of its LAST stage cost,
// S = sum over its n symbols of (16 - floor(log2 freq)) (an integer; it overstates the ideal bits by about half a bit per symbol):
//   expensive symbols (S >= 11 n: uniform noise under the sigma-floor weights, ~12 bits each): an xwide v4 stream costs ~2.5 bytes there (two
//     seeded tail chains carry six raw symbols), so a third more streams fit the same byte budget: rans_auto_hi(Mlo);
//   cheap symbols (S < 4 n: the class of the reference's trained model on natural images, 1.7 bits each): a stream costs ~5.1 bytes and its
//     serial tail is ~5,000 symbols long: two thirds of the streams, rans_auto_cheap(Mlo);
//   and whatever the class, a count whose payloads of 7,936 bits the last stage cannot fill with a tenth to spare (2 S - n < 2 * 8,704 M)
//     falls to half the size rule's, rans_auto_min(Mlo) -- every unfilled payload bit is a wasted bit.
// A pure function of the image: the same image gets the same container whatever it is coded with, next to or after (oracle: orc_auto_streams).
LLICTI_HD int rans_auto_hi(int Mlo) { const int h = Mlo + (Mlo + 2) / 3; return h > 32 ? 32 : h; }
LLICTI_HD int rans_auto_cheap(int Mlo) { return (2 * Mlo + 2) / 3; }
LLICTI_HD int rans_auto_min(int Mlo) { return (Mlo + 1) / 2; }
LLICTI_HD int rans_auto_pick(int Mlo, long long S, long long n)
{
    if (n <= 0) return Mlo;
    int M = Mlo;
    if (S >= 11 * n) M = rans_auto_hi(Mlo);
    else if (S < 4 * n) M = rans_auto_cheap(Mlo);
    if (2 * S - n < 2LL * 8704 * M) M = (M > Mlo && 2 * S - n >= 2LL * 8704 * Mlo) ? Mlo : rans_auto_min(Mlo);
    return M;
}


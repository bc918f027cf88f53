// digest.hpp -- pixel digests: zlib's CRC-32 of every image's planar uint8 [3][H][W] bytes, computed from the int16 YCoCg-R planes a
// whole-batch call leaves in its workspace (include/llicti_hip.h, "PIXEL DIGESTS"; the arithmetic: crc_math.hpp).  Part of the single
// translation unit llicti_hip.hip.
//
// Two steps without atomics, like minmax_fold / minmax_reduce_kernel:
//   crc_planes_kernel  grid (groups, images).  A workgroup takes kCrcGroupPixels consecutive pixels of one image, inverts YCoCg-R and carries
//                      THREE raw CRCs, one per colour plane: pixel p is byte p of the R, of the G and of the B plane.  Its three partial
//                      words go to part[image][group][3].
//   crc_fold_kernel    one workgroup per image folds the groups in order, then the planes (R || G || B), and applies zlib's initial and
//                      final complement.
// THE RAGGED END IS IN FRONT.  An image of n pixels takes g = ceil(n / kCrcGroupPixels) groups; pixel p sits at position p + (g * kCrcGroupPixels
// - n) of them, so the positions in front of pixel 0 are empty and every lane behind them owns exactly kCrcLanePixels pixels.  Zero-length and
// short runs start from a zero register and a raw CRC does not see what is missing in front of it, so every run is folded with the
// constant of a FULL run: lane t's CRC times x^(8 L (T - 1 - t)), group k's times x^(8 G (g - 1 - k)) -- table entries, one multiplication per
// lane and per group, then plain xor reductions.  Only the planes' fold takes a true length, H W.
// HOW A LANE GETS ITS BYTES: the workgroup stages its pixels through LDS.  Global loads are coalesced (16-byte loads of 8 pixels per lane where
// the image's three plane bases are 16-byte aligned, element loads otherwise -- per image, wave-uniform); the inverse transform runs there, and
// a pixel's three bytes go to LDS as one word.  A lane then reads its own run, at a stride of kCrcLanePixels + 1 words between lanes
// (ds_read_b32 banks are the word index mod 32: conflict-free).
// HOW IT ADVANCES: one 256-entry table step per byte.  The table is built in LDS by the workgroup itself, 32 copies side by side -- entry e of
// copy c at word e * 32 + c, lane l reads copy l % 32 -- so the 32 lanes of a read group hit 32 different banks whatever bytes they hold.
#pragma once
#include "crc_math.hpp"

constexpr int kCrcPixStride = kCrcLanePixels + 1;
constexpr int kCrcLdsWords = 256 * 32 + kCrcThreads * kCrcPixStride;      // the table's copies, then the staged pixels
constexpr size_t kCrcLdsBytes = (size_t)kCrcLdsWords * sizeof(uint32_t);
constexpr int kCrcMaxParts = 65536;                                       // entries (of 3 words) of the context's partials scratch

struct alignas(16) Short8 { int16_t e[8]; };

// xor of v over the workgroup's 256 lanes, valid in lane 0 (red: 3 x 4 words of LDS)
__device__ __forceinline__ void crc_xor_reduce3(uint32_t v[3], uint32_t *red)
{
#pragma unroll
    for (int c = 0; c < 3; ++c)
        for (int o = 32; o > 0; o >>= 1) v[c] ^= __shfl_xor(v[c], o);
    const int wv = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { red[wv * 3 + 0] = v[0]; red[wv * 3 + 1] = v[1]; red[wv * 3 + 2] = v[2]; }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c] = red[c] ^ red[3 + c] ^ red[6 + c] ^ red[9 + c];
    }
}

// planes: the int16 planes; image b (= b0 + blockIdx.y) at iv[b].pix_off with iv[b].plane pixels per plane, or -- iv == nullptr -- contiguous
// at b * 3 * plane.  have: nullptr, or a flag per image: an image whose flag is 0 is not read.  tab: the context's tables (crc_math.hpp).
// part[(blockIdx.y * gridDim.x + group) * 3 + c]: the group's raw CRC of colour plane c.  Groups past the image's own count do nothing.
__global__ __launch_bounds__(kCrcThreads) void crc_planes_kernel(const int16_t *__restrict__ planes, long plane, const ImgGeo *__restrict__ iv,
                                                                 const int32_t *__restrict__ have, int b0, const uint32_t *__restrict__ tab,
                                                                 uint32_t *__restrict__ part)
{
    extern __shared__ uint32_t crc_lds[];
    uint32_t *ltab = crc_lds, *lpix = crc_lds + 256 * 32;
    __shared__ uint32_t red[12], ent[256];
    const int b = b0 + blockIdx.y, tid = threadIdx.x;
    if (have && have[b] == 0) return;
    long base = (long)b * 3 * plane;
    if (iv) { plane = iv[b].plane; base = iv[b].pix_off; }
    const long groups = (plane + kCrcGroupPixels - 1) / kCrcGroupPixels;
    const long x = blockIdx.x;
    if (x >= groups) return;
    const long pad = groups * kCrcGroupPixels - plane;                  // empty positions in front of pixel 0 (group 0 alone has any)
    const long v0 = x * kCrcGroupPixels;                                // the group's first position
    const long p0 = v0 > pad ? v0 - pad : 0, p1 = v0 + kCrcGroupPixels - pad;      // its pixels [p0, p1), p1 <= plane
    // the byte table: lane t computes entry t; the copies are then written a row of 256 consecutive words at a time (8 entries x 32 copies)
    ent[tid] = crc32_byte(0, (uint32_t)tid);
    __syncthreads();
    for (int r = 0; r < 32; ++r) ltab[r * kCrcThreads + tid] = ent[r * 8 + (tid >> 5)];
    const int16_t *src = planes + base;
    auto stage = [&](long p, int y, int co, int cg) {
        int R, G, Bl;
        ycocg_inv(y, co, cg, R, G, Bl);
        const int i = (int)(p + pad - v0);                              // position in the group
        lpix[(i / kCrcLanePixels) * kCrcPixStride + (i % kCrcLanePixels)] = (uint32_t)R | ((uint32_t)G << 8) | ((uint32_t)Bl << 16);
    };
    const bool vec = ((plane | base) & 7) == 0 && ((uintptr_t)planes & 15) == 0;
    if (vec) {
        for (long q = (p0 >> 3) + tid; q * 8 < p1; q += kCrcThreads) {  // (plane % 8 == 0 and p1 <= plane: a group of 8 never leaves its plane)
            const Short8 y = *reinterpret_cast<const Short8 *>(src + q * 8);
            const Short8 co = *reinterpret_cast<const Short8 *>(src + plane + q * 8);
            const Short8 cg = *reinterpret_cast<const Short8 *>(src + 2 * plane + q * 8);
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const long p = q * 8 + k;
                if (p >= p0 && p < p1) stage(p, y.e[k], co.e[k], cg.e[k]);
            }
        }
    } else {
        for (long p = p0 + tid; p < p1; p += kCrcThreads) stage(p, src[p], src[plane + p], src[2 * plane + p]);
    }
    __syncthreads();
    // the lane's run: positions v0 + tid L .. + L - 1, those in front of pixel 0 skipped
    const long lane_v = v0 + (long)tid * kCrcLanePixels;
    const int k0 = (int)(pad > lane_v ? (pad - lane_v < kCrcLanePixels ? pad - lane_v : kCrcLanePixels) : 0);
    const uint32_t *lt = ltab + (tid & 31);
    const uint32_t *lp = lpix + tid * kCrcPixStride;
    uint32_t crc[3] = { 0, 0, 0 };
    for (int k = k0; k < kCrcLanePixels; ++k) {
        const uint32_t px = lp[k];
#pragma unroll
        for (int c = 0; c < 3; ++c) crc[c] = lt[((crc[c] ^ (px >> (8 * c))) & 0xFFu) * 32] ^ (crc[c] >> 8);
    }
    gf2_mul3(crc, tab[kCrcTabLane + kCrcThreads - 1 - tid]);
    crc_xor_reduce3(crc, red);
    if (tid == 0) {
        uint32_t *q = part + ((long)blockIdx.y * gridDim.x + x) * 3;
        q[0] = crc[0]; q[1] = crc[1]; q[2] = crc[2];
    }
}

// One workgroup per image b = b0 + blockIdx.x: d_crc[b] = crc32 of its [3][H][W] bytes, d_have[b] = 1 (d_have may be nullptr); an image whose
// have flag is 0 gets d_crc[b] = 0, d_have[b] = 0.  gx: the groups per image part was written with.
__global__ __launch_bounds__(kCrcThreads) void crc_fold_kernel(const uint32_t *__restrict__ part, int gx, long plane, const ImgGeo *__restrict__ iv,
                                                               const int32_t *__restrict__ have, int b0, const uint32_t *__restrict__ tab,
                                                               uint32_t *__restrict__ d_crc, int32_t *__restrict__ d_have)
{
    __shared__ uint32_t red[12];
    const int b = b0 + blockIdx.x, tid = threadIdx.x;
    if (have && have[b] == 0) {
        if (tid == 0) { d_crc[b] = 0; if (d_have) d_have[b] = 0; }
        return;
    }
    if (iv) plane = iv[b].plane;
    const int groups = (int)((plane + kCrcGroupPixels - 1) / kCrcGroupPixels);
    uint32_t acc[3] = { 0, 0, 0 };
    for (int k = tid; k < groups; k += kCrcThreads) {
        const uint32_t *q = part + ((long)blockIdx.x * gx + k) * 3;
        uint32_t v[3] = { q[0], q[1], q[2] };
        gf2_mul3(v, tab[kCrcTabGroup + groups - 1 - k]);
        acc[0] ^= v[0]; acc[1] ^= v[1]; acc[2] ^= v[2];
    }
    crc_xor_reduce3(acc, red);
    if (tid >= 64) return;
    // x^(8 H W): the product of the table's x^(8 2^j) over the set bits of H W (< 2^27), a butterfly of five multiplications over 32 lanes
    uint32_t xp = (tid < 32 && ((plane >> tid) & 1)) ? tab[kCrcTabPow + tid] : kCrcOne;
    for (int o = 16; o > 0; o >>= 1) xp = gf2_mul(xp, __shfl_xor(xp, o));
    if (tid == 0) {
        const uint32_t xp2 = gf2_mul(xp, xp);
        const uint32_t raw = gf2_mul(acc[0], xp2) ^ gf2_mul(acc[1], xp) ^ acc[2];
        d_crc[b] = crc32_finish(raw, gf2_mul(xp2, xp));
        if (d_have) d_have[b] = 1;
    }
}

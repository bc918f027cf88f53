// lift.hpp -- integer YCoCg-R lift / unlift, per-image min/max, float planes (K1-K3, K13).
// Part of the single translation unit llicti_hip.hip (included in order; not a stand-alone header).
#pragma once

// ------------------------------------------------------------------------------------------------ the pixel end's parts, each ONCE
// Every kernel that turns pixels into planes or planes into pixels (here and in container.hpp) is made of these.

// forward YCoCg-R of one 8-bit pixel; Y comes out centred (- 127)
__device__ __forceinline__ void ycocg_fwd(int R, int G, int Bl, int &Y, int &Co, int &Cg)
{
    Co = R - Bl;
    const int t = Bl + (Co >> 1);        // floor division (torch >= 1.13 '//'; JVT YCoCg-R '>> 1')
    Cg = G - t;
    Y = t + (Cg >> 1) - 127;
}
// ... and back: the channels wrapped to 8 bits (what a corrupt container decodes to stays a byte)
__device__ __forceinline__ void ycocg_inv(int Y, int Co, int Cg, int &R, int &G, int &Bl)
{
    Y += 127;
    const int t = Y - (Cg >> 1);
    const int g = Cg + t, b = t - (Co >> 1), r = b + Co;
    R = (int)(uint8_t)r; G = (int)(uint8_t)g; Bl = (int)(uint8_t)b;
}

template <typename T> struct alignas(4 * sizeof(T)) Quad { T e[4]; };      // four elements moved by one access

// Per-image min / max of Co and Cg in two steps without atomics: every workgroup of a lift kernel leaves its four
// partial values in part[b][blockIdx.x][4], one small workgroup per image folds them.  (Thousands of atomicMin /
// atomicMax on the same 16 bytes of an image serialise at the memory side: 150 of the kernel's 180 us.)
struct MinMax {
    int mnCo = 32767, mnCg = 32767, mxCo = -32768, mxCg = -32768;
    __device__ __forceinline__ void add(int Co, int Cg) { mnCo = min(mnCo, Co); mxCo = max(mxCo, Co); mnCg = min(mnCg, Cg); mxCg = max(mxCg, Cg); }
};
// the workgroup's (256 threads) partial of image b: wave shuffle, four words per wave through LDS, one store per value
__device__ __forceinline__ void minmax_fold(int mnCo, int mnCg, int mxCo, int mxCg, int32_t *__restrict__ part, int b)
{
    for (int o = 32; o > 0; o >>= 1) {
        mnCo = min(mnCo, __shfl_xor(mnCo, o)); mxCo = max(mxCo, __shfl_xor(mxCo, o));
        mnCg = min(mnCg, __shfl_xor(mnCg, o)); mxCg = max(mxCg, __shfl_xor(mxCg, o));
    }
    __shared__ int red[4][4];
    if ((threadIdx.x & 63) == 0) {
        const int wv = threadIdx.x >> 6;
        red[wv][0] = mnCo; red[wv][1] = mnCg; red[wv][2] = mxCo; red[wv][3] = mxCg;
    }
    __syncthreads();
    if (threadIdx.x < 4) {
        const int k = threadIdx.x;
        int v = red[0][k];
        for (int wv = 1; wv < 4; ++wv) v = (k < 2) ? min(v, red[wv][k]) : max(v, red[wv][k]);
        part[((long)b * gridDim.x + blockIdx.x) * 4 + k] = v;
    }
}

__global__ __launch_bounds__(64) void minmax_reduce_kernel(const int32_t *__restrict__ part, int gx, int32_t *__restrict__ mm)
{
    const int b = blockIdx.x;
    MinMax m;
    for (int t = threadIdx.x; t < gx; t += 64) {
        const int32_t *q = part + ((long)b * gx + t) * 4;
        m.mnCo = min(m.mnCo, q[0]); m.mnCg = min(m.mnCg, q[1]); m.mxCo = max(m.mxCo, q[2]); m.mxCg = max(m.mxCg, q[3]);
    }
    for (int o = 32; o > 0; o >>= 1) {
        m.mnCo = min(m.mnCo, __shfl_xor(m.mnCo, o)); m.mxCo = max(m.mxCo, __shfl_xor(m.mxCo, o));
        m.mnCg = min(m.mnCg, __shfl_xor(m.mnCg, o)); m.mxCg = max(m.mxCg, __shfl_xor(m.mxCg, o));
    }
    if (threadIdx.x == 0) { mm[4 * b + 0] = m.mnCo; mm[4 * b + 1] = m.mnCg; mm[4 * b + 2] = m.mxCo; mm[4 * b + 3] = m.mxCg; }
}

// The first n (1 .. 4) of four consecutive pixels into the int16 planes and the float planes ((float)v / 255.0f) at dst / fdst: one short4 and
// one float4 per channel where `vec` (n == 4, both pointers aligned to four elements), element by element otherwise.  The twelve quotients are
// taken ONCE, in front of the branch: the divisions then overlap the loads of the next pixels in either arm.
__device__ __forceinline__ void store_planes4(int16_t *__restrict__ dst, float *__restrict__ fdst, long plane, const int (&y)[4], const int (&co)[4],
                                              const int (&cg)[4], int n, bool vec)
{
    float fy[4], fco[4], fcg[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) { fy[k] = (float)y[k] / 255.0f; fco[k] = (float)co[k] / 255.0f; fcg[k] = (float)cg[k] / 255.0f; }
    if (vec) {
        *reinterpret_cast<short4 *>(dst) = make_short4((short)y[0], (short)y[1], (short)y[2], (short)y[3]);
        *reinterpret_cast<short4 *>(dst + plane) = make_short4((short)co[0], (short)co[1], (short)co[2], (short)co[3]);
        *reinterpret_cast<short4 *>(dst + 2 * plane) = make_short4((short)cg[0], (short)cg[1], (short)cg[2], (short)cg[3]);
        *reinterpret_cast<float4 *>(fdst) = make_float4(fy[0], fy[1], fy[2], fy[3]);
        *reinterpret_cast<float4 *>(fdst + plane) = make_float4(fco[0], fco[1], fco[2], fco[3]);
        *reinterpret_cast<float4 *>(fdst + 2 * plane) = make_float4(fcg[0], fcg[1], fcg[2], fcg[3]);
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (k < n) {
                dst[k] = (int16_t)y[k]; dst[plane + k] = (int16_t)co[k]; dst[2 * plane + k] = (int16_t)cg[k];
                fdst[k] = fy[k]; fdst[plane + k] = fco[k]; fdst[2 * plane + k] = fcg[k];
            }
    }
}

// The first n of four consecutive DECODED pixels of row `row` from column `col` (leftwards where `flip`) out of planes of width W decoded at
// reduce r -- decoded pixel (i, j) is the plane pixel (i << r, j << r) --, zeros behind them: one short4 per channel where `vec` (r == 0, no
// flip, n == 4, the row piece aligned to four elements), a gather otherwise.
__device__ __forceinline__ void load_planes4(const int16_t *__restrict__ src, long plane, int W, int r, int row, int col, bool flip, int n, bool vec,
                                             int (&y)[4], int (&co)[4], int (&cg)[4])
{
    if (vec) {
        const long p = (long)row * W + col;
        const short4 a = *reinterpret_cast<const short4 *>(src + p);
        const short4 c = *reinterpret_cast<const short4 *>(src + plane + p);
        const short4 d = *reinterpret_cast<const short4 *>(src + 2 * plane + p);
        y[0] = a.x; y[1] = a.y; y[2] = a.z; y[3] = a.w;
        co[0] = c.x; co[1] = c.y; co[2] = c.z; co[3] = c.w;
        cg[0] = d.x; cg[1] = d.y; cg[2] = d.z; cg[3] = d.w;
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            y[k] = co[k] = cg[k] = 0;
            if (k < n) {
                const int16_t *s = src + ((long)(row << r) * W + ((long)(flip ? col - k : col + k) << r));
                y[k] = s[0]; co[k] = s[plane]; cg[k] = s[2 * plane];
            }
        }
    }
}

// The status words of a whole-batch call (the workspace's: [0] the call's, [head + b] image b's).  An encode's first kernel clears them before
// any kernel that can set them is launched; a decode's last kernel latches them into the context's -- every kernel that can set them has
// finished --, neither by a launch of its own.
__device__ __forceinline__ void clear_status(int32_t *__restrict__ zero, int n_zero)      // by ONE workgroup of the launch
{
    if (zero) for (int i = threadIdx.x; i < n_zero; i += blockDim.x) zero[i] = 0;
}
__device__ __forceinline__ void latch_call(const int32_t *__restrict__ status, int32_t *__restrict__ latched) { if (status[0] != 0) *latched = status[0]; }
__device__ __forceinline__ void latch_image(const int32_t *__restrict__ status, int head, int32_t *__restrict__ img_latched, int b)
{
    if (img_latched) img_latched[b] = status[head + b];
}
// by the kernels whose blockIdx.y walks the images: word 0 if set (image 0's first block), and image b's word by the image's first block
__device__ __forceinline__ void latch_status(const int32_t *__restrict__ status, int head, int32_t *__restrict__ latched,
                                             int32_t *__restrict__ img_latched, int b)
{
    if (status && blockIdx.x == 0 && threadIdx.x == 0) {
        if (b == 0) latch_call(status, latched);
        latch_image(status, head, img_latched, b);
    }
}
// by ONE workgroup, for all n images of the call
__device__ __forceinline__ void latch_status_all(const int32_t *__restrict__ status, int head, int32_t *__restrict__ latched,
                                                 int32_t *__restrict__ img_latched, int n)
{
    if (threadIdx.x == 0) latch_call(status, latched);
    for (int b = (int)threadIdx.x; b < n; b += (int)blockDim.x) latch_image(status, head, img_latched, b);
}

// ------------------------------------------------------------------------------------------------ lift
// the pixel value of a source sample.  A float sample (llicti_encode_images_f32: planar float32 in {k/255}, specified to the operation in
// include/llicti_hip.h so that the call is held EXACTLY against PyTorch on the CPU): round(x * 255) half to even -- one rounded product,
// -ffp-contract=off --, clamped to 0 .. 255; a NaN compares false and gives 0
__device__ __forceinline__ int f32_pixel(float x)
{
    const float t = rintf(__fmul_rn(x, 255.0f));
    return (t >= 0.0f) ? (int)fminf(t, 255.0f) : 0;
}
__device__ __forceinline__ int src_pixel(uint8_t v) { return v; }
__device__ __forceinline__ int src_pixel(float v) { return f32_pixel(v); }
// four consecutive samples by one access (aligned to four elements)
__device__ __forceinline__ void src_pixels4(const uint8_t *s, int (&v)[4]) { const uchar4 a = *reinterpret_cast<const uchar4 *>(s); v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; }
__device__ __forceinline__ void src_pixels4(const float *s, int (&v)[4])
{
    const float4 a = *reinterpret_cast<const float4 *>(s);
    v[0] = f32_pixel(a.x); v[1] = f32_pixel(a.y); v[2] = f32_pixel(a.z); v[3] = f32_pixel(a.w);
}

// Planar sources, SRC = uint8_t or float: 4 pixels per thread (VEC = 4) when the plane size allows aligned 4-element accesses.
// zero != nullptr (the whole-batch encode, whose first kernel this is): the call's n_zero status words are cleared here.
// iv != nullptr (whole-batch calls): image b's size and placement come from the call's table (the images may differ in size; rgb_off counts
// ELEMENTS of SRC); else B images of `plane` pixels each, tightly packed in all three arrays (llicti_lift_u8).
template <typename SRC, int VEC>
__global__ __launch_bounds__(256) void lift_kernel(const SRC *__restrict__ rgb, long plane, int16_t *__restrict__ planes,
                                                   float *__restrict__ fplanes, int32_t *__restrict__ part, int32_t *__restrict__ zero, int n_zero,
                                                   const ImgGeo *__restrict__ iv)
{
    const int b = blockIdx.y;
    if (blockIdx.x == 0 && b == 0) clear_status(zero, n_zero);
    long src_off = (long)b * 3 * plane, dst_off = src_off;
    if (iv) { plane = iv[b].plane; src_off = iv[b].rgb_off; dst_off = iv[b].pix_off; }
    const SRC *src = rgb + src_off;
    int16_t *dst = planes + dst_off;
    float *fdst = fplanes + dst_off;
    MinMax m;
    for (long p = ((long)blockIdx.x * blockDim.x + threadIdx.x) * VEC; p < plane; p += (long)gridDim.x * blockDim.x * VEC) {
        int ch[3][4];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            if constexpr (VEC == 4) src_pixels4(src + c * plane + p, ch[c]);
            else ch[c][0] = src_pixel(src[c * plane + p]);
        }
        int y[4] = {}, co[4] = {}, cg[4] = {};
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
            ycocg_fwd(ch[0][k], ch[1][k], ch[2][k], y[k], co[k], cg[k]);
            m.add(co[k], cg[k]);
        }
        store_planes4(dst + p, fdst + p, plane, y, co, cg, VEC, VEC == 4);
    }
    minmax_fold(m.mnCo, m.mnCg, m.mxCo, m.mxCg, part, b);
}

// status != nullptr (the whole-batch decode, whose last kernel this is): the call's status words are latched into the context's here.
__global__ __launch_bounds__(256) void unlift_kernel(const int16_t *__restrict__ planes, long plane, uint8_t *__restrict__ rgb,
                                                     const int32_t *__restrict__ status, int status_head, int32_t *__restrict__ latched,
                                                     int32_t *__restrict__ img_latched, const ImgGeo *__restrict__ iv)
{
    const int b = blockIdx.y;
    latch_status(status, status_head, latched, img_latched, b);
    long src_off = (long)b * 3 * plane, dst_off = src_off;
    if (iv) { plane = iv[b].plane; src_off = iv[b].pix_off; dst_off = iv[b].rgb_off; }      // (lift_kernel: the call's per-image table)
    const int16_t *src = planes + src_off;
    uint8_t *dst = rgb + dst_off;
    for (long p = (long)blockIdx.x * blockDim.x + threadIdx.x; p < plane; p += (long)gridDim.x * blockDim.x) {
        int R, G, Bl;
        ycocg_inv(src[p], src[plane + p], src[2 * plane + p], R, G, Bl);
        dst[p] = (uint8_t)R; dst[plane + p] = (uint8_t)G; dst[2 * plane + p] = (uint8_t)Bl;
    }
}

// The last kernel of a reduced-resolution decode (llicti_decode_images_reduced, r >= 1): output pixel (i, j) of image b is the plane pixel
// (i << r, j << r) -- final once level r has been decoded; the finer levels' pixels are never written and never read here -- through the same
// inverse YCoCg-R, written as compact planar uint8 [3][Hr][Wr] at rv[b].off.  One thread per output pixel; image b's sizes and offsets are
// scalar loads from the call's tables.  Latches the call's status words like unlift_kernel.
// rtab != nullptr (llicti_decode_images_reduced_rv): image b stops at ITS OWN level, r = rtab[b] (0: its full size) -- one more scalar load
// beside iv[b]'s; rv[b] holds the sizes that go with it.
__global__ __launch_bounds__(256) void unlift_reduced_kernel(const int16_t *__restrict__ planes, uint8_t *__restrict__ rgb, int r,
                                                             const int32_t *__restrict__ status, int status_head, int32_t *__restrict__ latched,
                                                             int32_t *__restrict__ img_latched, const ImgGeo *__restrict__ iv,
                                                             const RedGeo *__restrict__ rv, const int *__restrict__ rtab = nullptr)
{
    const int b = blockIdx.y;
    latch_status(status, status_head, latched, img_latched, b);
    if (rtab) r = rtab[b];
    const int W = iv[b].W, Hr = rv[b].Hr, Wr = rv[b].Wr;
    const long plane = iv[b].plane, rplane = (long)Hr * Wr;
    const long p = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= rplane) return;
    const int i = (int)((uint32_t)p / (uint32_t)Wr), j = (int)((uint32_t)p - (uint32_t)i * (uint32_t)Wr);      // (rplane <= 4080^2 < 2^32)
    const int16_t *src = planes + iv[b].pix_off + ((long)(i << r) * W + (j << r));
    uint8_t *dst = rgb + rv[b].off + p;
    int R, G, Bl;
    ycocg_inv(src[0], src[plane], src[2 * plane], R, G, Bl);
    dst[0] = (uint8_t)R; dst[rplane] = (uint8_t)G; dst[2 * rplane] = (uint8_t)Bl;
}

// ------------------------------------------------------------------------------------------------ interleaved, pitched pixels
// llicti_encode_images_px / llicti_decode_images_px: the caller's buffer holds interleaved 8-bit pixels (PixGeo: window offset, row pitch,
// format), the workspace the same planes as above.  ALPHA: the fourth byte of the 4-byte formats is ignored by the lift and written as 255
// by the unlift.  The kernels walk the window's ROWS (a pitch breaks the flat index): a lane owns 4 consecutive pixels of one row -- 12 or
// 16 contiguous bytes, so a wavefront covers 768 / 1024 contiguous bytes that are split into channels in registers.
//   pixel side   dword accesses (3 or 4 per lane) when the window's first byte and its pitch are multiples of 4, and the lane has 4 pixels;
//   plane side   short4 / float4 accesses when the image's W is a multiple of 4 (rows then start at multiples of 4 elements);
//   otherwise    byte by byte / element by element, the W % 4 pixels that end a row included.
// Both conditions are per IMAGE and come from its table entries (scalar loads, blockIdx.y): wave-uniform, and one call may hold an aligned
// frame next to a crop that starts at an odd byte.  The unlift stores only bytes of the window's rows: no store straddles a row's end, nothing
// of the canvas is read.

// channel ch (0 R, 1 G, 2 B) of pixel k out of the BPP dwords of 4 pixels
template <int BPP>
__device__ __forceinline__ int px_byte(const uint32_t *d, int k, int ch) { const int t = k * BPP + ch; return (int)((d[t >> 2] >> (8 * (t & 3))) & 0xFFu); }

template <int BPP>
__device__ __forceinline__ void lift_px_rows(const uint8_t *__restrict__ src, int pitch, bool bgr, int H, int W, long plane,
                                             int16_t *__restrict__ dst, float *__restrict__ fdst, MinMax &m)
{
    const uint32_t Wq = (uint32_t)(W + 3) >> 2, units = (uint32_t)H * Wq;        // (<= 8160 * 2040)
    const bool px_dw = (((uintptr_t)src | (uintptr_t)(uint32_t)pitch) & 3) == 0;
    const bool pl_vec = (W & 3) == 0 && (((uintptr_t)dst & 7) | ((uintptr_t)fdst & 15)) == 0;
    for (uint32_t u = blockIdx.x * blockDim.x + threadIdx.x; u < units; u += gridDim.x * blockDim.x) {
        const uint32_t i = u / Wq, j = (u - i * Wq) * 4;
        const int n = min(4, W - (int)j);
        const uint8_t *q = src + (long)i * pitch + (long)j * BPP;
        int ch[4][3];
        if (px_dw && n == 4) {
            uint32_t d[BPP];
#pragma unroll
            for (int k = 0; k < BPP; ++k) d[k] = reinterpret_cast<const uint32_t *>(q)[k];
#pragma unroll
            for (int k = 0; k < 4; ++k) { ch[k][0] = px_byte<BPP>(d, k, 0); ch[k][1] = px_byte<BPP>(d, k, 1); ch[k][2] = px_byte<BPP>(d, k, 2); }
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                ch[k][0] = ch[k][1] = ch[k][2] = 0;
                if (k < n) { ch[k][0] = q[k * BPP]; ch[k][1] = q[k * BPP + 1]; ch[k][2] = q[k * BPP + 2]; }
            }
        }
        int y[4], co[4], cg[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            ycocg_fwd(bgr ? ch[k][2] : ch[k][0], ch[k][1], bgr ? ch[k][0] : ch[k][2], y[k], co[k], cg[k]);
            if (k < n) m.add(co[k], cg[k]);
        }
        const long p = (long)i * W + j;
        store_planes4(dst + p, fdst + p, plane, y, co, cg, n, pl_vec);
    }
}

// lift_kernel on interleaved pixels: the same planes, min / max partials and clearing of the call's status words; image b's size and plane
// placement from iv[b], its window from pv[b].
__global__ __launch_bounds__(256) void lift_px_kernel(const uint8_t *__restrict__ pix, int16_t *__restrict__ planes, float *__restrict__ fplanes,
                                                      int32_t *__restrict__ part, int32_t *__restrict__ zero, int n_zero,
                                                      const ImgGeo *__restrict__ iv, const PixGeo *__restrict__ pv)
{
    const int b = blockIdx.y;
    if (blockIdx.x == 0 && b == 0) clear_status(zero, n_zero);
    const int H = iv[b].H, W = iv[b].W, pitch = pv[b].pitch, fmt = pv[b].fmt;
    const long plane = iv[b].plane;
    const uint8_t *src = pix + pv[b].off;
    int16_t *dst = planes + iv[b].pix_off;
    float *fdst = fplanes + iv[b].pix_off;
    MinMax m;
    if (pix_bpp(fmt) == 4) lift_px_rows<4>(src, pitch, pix_bgr(fmt), H, W, plane, dst, fdst, m);
    else lift_px_rows<3>(src, pitch, pix_bgr(fmt), H, W, plane, dst, fdst, m);
    minmax_fold(m.mnCo, m.mnCg, m.mxCo, m.mxCg, part, b);
}

// r: 0 = every pixel of the planes; r >= 1 = the pixels whose row and column are multiples of 2^r (unlift_reduced_kernel's gather) -- Ho x Wo
// is the window either way
template <int BPP>
__device__ __forceinline__ void unlift_px_rows(const int16_t *__restrict__ src, long plane, int W, int r, int Ho, int Wo,
                                               uint8_t *__restrict__ dst, int pitch, bool bgr)
{
    const uint32_t Wq = (uint32_t)(Wo + 3) >> 2, units = (uint32_t)Ho * Wq;
    const bool px_dw = (((uintptr_t)dst | (uintptr_t)(uint32_t)pitch) & 3) == 0;
    const bool pl_vec = r == 0 && (W & 3) == 0 && ((uintptr_t)src & 7) == 0;        // (Wo == W then: every lane has 4 pixels)
    for (uint32_t u = blockIdx.x * blockDim.x + threadIdx.x; u < units; u += gridDim.x * blockDim.x) {
        const uint32_t i = u / Wq, j = (u - i * Wq) * 4;
        const int n = min(4, Wo - (int)j);
        int y[4], co[4], cg[4];
        load_planes4(src, plane, W, r, (int)i, (int)j, false, n, pl_vec, y, co, cg);
        uint32_t c3[4][3];          // the pixel's bytes in the buffer's order
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            int R, G, Bl;
            ycocg_inv(y[k], co[k], cg[k], R, G, Bl);
            c3[k][0] = (uint32_t)(bgr ? Bl : R); c3[k][1] = (uint32_t)G; c3[k][2] = (uint32_t)(bgr ? R : Bl);
        }
        uint8_t *q = dst + (long)i * pitch + (long)j * BPP;
        if (px_dw && n == 4) {
            uint32_t d[BPP];
#pragma unroll
            for (int k = 0; k < BPP; ++k) d[k] = 0;
#pragma unroll
            for (int t = 0; t < 4 * BPP; ++t) {
                const int k = t / BPP, ch = t - k * BPP;
                d[t >> 2] |= (ch == 3 ? 255u : c3[k][ch == 3 ? 0 : ch]) << (8 * (t & 3));
            }
#pragma unroll
            for (int k = 0; k < BPP; ++k) reinterpret_cast<uint32_t *>(q)[k] = d[k];
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (k < n) {
                    q[k * BPP] = (uint8_t)c3[k][0]; q[k * BPP + 1] = (uint8_t)c3[k][1]; q[k * BPP + 2] = (uint8_t)c3[k][2];
                    if (BPP == 4) q[k * BPP + 3] = 255;
                }
        }
    }
}

// unlift_kernel (rv == nullptr, r = 0) and unlift_reduced_kernel (rv: the reduced sizes, r >= 1) into interleaved pixels: the last kernel of
// llicti_decode_images_px.  Latches the call's status words exactly as they do.
__global__ __launch_bounds__(256) void unlift_px_kernel(const int16_t *__restrict__ planes, uint8_t *__restrict__ pix, int r,
                                                        const int32_t *__restrict__ status, int status_head, int32_t *__restrict__ latched,
                                                        int32_t *__restrict__ img_latched, const ImgGeo *__restrict__ iv,
                                                        const RedGeo *__restrict__ rv, const PixGeo *__restrict__ pv,
                                                        const int *__restrict__ rtab = nullptr)
{
    const int b = blockIdx.y;
    latch_status(status, status_head, latched, img_latched, b);
    if (rtab) r = rtab[b];      // (the _rv call: the image's own level, wave-uniform; an image at 0 takes the full-size vector path below)
    const int W = iv[b].W, Ho = rv ? rv[b].Hr : iv[b].H, Wo = rv ? rv[b].Wr : W, pitch = pv[b].pitch, fmt = pv[b].fmt;
    const long plane = iv[b].plane;
    const int16_t *src = planes + iv[b].pix_off;
    uint8_t *dst = pix + pv[b].off;
    if (pix_bpp(fmt) == 4) unlift_px_rows<4>(src, plane, W, r, Ho, Wo, dst, pitch, pix_bgr(fmt));
    else unlift_px_rows<3>(src, plane, W, r, Ho, Wo, dst, pitch, pix_bgr(fmt));
}

// ------------------------------------------------------------------------------------------------ float tensors
// llicti_decode_images_tensor and its resampling kin: the dense [B][3][Ho][Wo] tensor a network is fed with.  The arithmetic is specified to
// the operation (include/llicti_hip.h) so that the output is held EXACTLY against PyTorch on the CPU: one IEEE division (and, normalised, one
// rounded subtraction and one correctly rounded division); -ffp-contract=off, no reciprocal anywhere.

// the element types of the output tensor: float, _Float16, and bfloat16 as its 16 bits
struct bf16_bits { uint16_t u; };
template <typename T> __device__ __forceinline__ T tensor_elem(float v);
template <> __device__ __forceinline__ float tensor_elem<float>(float v) { return v; }
template <> __device__ __forceinline__ _Float16 tensor_elem<_Float16>(float v) { return (_Float16)v; }      // round to nearest even, subnormals kept
template <> __device__ __forceinline__ bf16_bits tensor_elem<bf16_bits>(float v)
{
    const uint32_t u = __float_as_uint(v);
    if ((u & 0x7FFFFFFFu) > 0x7F800000u) return bf16_bits{ (uint16_t)0x7FC0 };                                // (a NaN, as torch writes it)
    return bf16_bits{ (uint16_t)((u + 0x7FFFu + ((u >> 16) & 1u)) >> 16) };                                   // round to nearest even
}
// channel c's element from its value v on the 0 .. 255 scale (a pixel value, or a filtered one).  __fdiv_rn and a plain '/' are the same
// correctly rounded IEEE division in this build (-ffp-contract=off, no fast-math): the float planes' (float)v / 255.0f is this quotient too.
template <typename T>
__device__ __forceinline__ T tensor_finish(float v, int c, const TensorNorm &nm)
{
    float f = __fdiv_rn(v, 255.0f);
    if (nm.on) f = __fdiv_rn(__fsub_rn(f, nm.mean[c]), nm.std[c]);
    return tensor_elem<T>(f);
}
// the first n of four consecutive output elements per channel at o: one 4-element store per channel where `vec`, element by element otherwise
template <typename T>
__device__ __forceinline__ void store_tensor_quads(T *__restrict__ o, long oplane, const Quad<T> (&q)[3], int n, bool vec)
{
    if (vec) {
#pragma unroll
        for (int c = 0; c < 3; ++c) *reinterpret_cast<Quad<T> *>(o + c * oplane) = q[c];
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (k < n) { o[k] = q[0].e[k]; o[oplane + k] = q[1].e[k]; o[2 * oplane + k] = q[2].e[k]; }
    }
}

// ... and the same four pixels INTERLEAVED (LLICTI_LAYOUT_NHWC): 12 consecutive elements at o, pixel k's channel c at o[3 k + c].  `vec`
// (n == 4 by Wo % 4 == 0, the tensor 16-byte aligned: o is then aligned to 48 bytes of float, to 8 of the 24 bytes of a 16-bit type): three
// 16-byte stores, or 16 + 8 bytes; element by element otherwise -- the same bytes either way.
template <typename T> struct alignas(8) Oct16 { T e[8]; };            // eight 16-bit elements moved by one access, aligned to half of it
template <typename T>
__device__ __forceinline__ void store_tensor_nhwc(T *__restrict__ o, const Quad<T> (&q)[3], int n, bool vec)
{
    if (vec) {
        T e[12];
#pragma unroll
        for (int k = 0; k < 4; ++k)
#pragma unroll
            for (int c = 0; c < 3; ++c) e[3 * k + c] = q[c].e[k];
        if constexpr (sizeof(T) == 4) {
#pragma unroll
            for (int s = 0; s < 3; ++s) *reinterpret_cast<Quad<T> *>(o + 4 * s) = Quad<T>{ { e[4 * s], e[4 * s + 1], e[4 * s + 2], e[4 * s + 3] } };
        } else {
            *reinterpret_cast<Oct16<T> *>(o) = Oct16<T>{ { e[0], e[1], e[2], e[3], e[4], e[5], e[6], e[7] } };
            *reinterpret_cast<Quad<T> *>(o + 8) = Quad<T>{ { e[8], e[9], e[10], e[11] } };
        }
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (k < n) { o[3 * k] = q[0].e[k]; o[3 * k + 1] = q[1].e[k]; o[3 * k + 2] = q[2].e[k]; }
    }
}
// Where a sink's four pixels go: pixel (i, j .. j + 3) of output slot `slot` of `out`, [slot][3][Ho][Wo] planes or [slot][Ho][Wo][3].  The
// condition of the wide stores is the same in both layouts: Wo % 4 == 0 and `out` aligned to 16 bytes (planar: to 4 elements, as ever).
struct PlanarStore {
    template <typename T>
    static __device__ __forceinline__ void put(T *__restrict__ out, long slot, int Ho, int Wo, int i, int j, const Quad<T> (&q)[3], int n)
    {
        const long oplane = (long)Ho * Wo;
        store_tensor_quads(out + slot * 3 * oplane + (long)i * Wo + j, oplane, q, n, (Wo & 3) == 0 && ((uintptr_t)out & (4 * sizeof(T) - 1)) == 0);
    }
};
struct NhwcStore {
    template <typename T>
    static __device__ __forceinline__ void put(T *__restrict__ out, long slot, int Ho, int Wo, int i, int j, const Quad<T> (&q)[3], int n)
    {
        store_tensor_nhwc(out + ((slot * Ho + i) * Wo + j) * 3, q, n, (Wo & 3) == 0 && ((uintptr_t)out & 15) == 0);
    }
};

// The last kernel of llicti_decode_images_tensor, in the place of unlift_kernel / unlift_reduced_kernel / unlift_px_kernel: image b's Ho x Wo
// window (origin and flip: word blockIdx.y of `wins`, the call's kernel arguments -- images b0 .. b0 + gridDim.y - 1 of the batch) through the
// inverse YCoCg-R into out[b][3][Ho][Wo].  Output pixel (i, j) is the plane pixel ((y0 + i) << r, (x0 + j') << r), j' = Wo - 1 - j where
// flipped.  A lane owns 4 consecutive output pixels of one row: one 4-element store per channel when Wo % 4 == 0 and `out` is aligned to
// 4 elements (every row then is), element by element otherwise; short4 plane loads when the window's rows are aligned in unflipped full-size
// planes.  Latches the call's status words exactly as the other unlift kernels do.
template <typename T>
__global__ __launch_bounds__(256) void unlift_tensor_kernel(const int16_t *__restrict__ planes, T *__restrict__ out, int r, int Ho, int Wo, int b0,
                                                            const TensorWins wins, const TensorNorm nm,
                                                            const int32_t *__restrict__ status, int status_head, int32_t *__restrict__ latched,
                                                            int32_t *__restrict__ img_latched, const ImgGeo *__restrict__ iv,
                                                            const int *__restrict__ rtab = nullptr)
{
    const int b = b0 + blockIdx.y;
    latch_status(status, status_head, latched, img_latched, b);
    if (rtab) r = rtab[b];      // (the _rv call: the image's own level, wave-uniform)
    const uint32_t wd = wins.w[blockIdx.y];
    const int y0 = (int)(wd & 0x1FFFu), x0 = (int)((wd >> 13) & 0x1FFFu);
    const bool flip = ((wd >> 26) & 1u) != 0;
    const int W = iv[b].W;
    const long plane = iv[b].plane, oplane = (long)Ho * Wo;
    const int16_t *src = planes + iv[b].pix_off;
    T *dst = out + (long)b * 3 * oplane;
    const uint32_t Wq = (uint32_t)(Wo + 3) >> 2, units = (uint32_t)Ho * Wq;
    const bool out_vec = (Wo & 3) == 0 && ((uintptr_t)out & (4 * sizeof(T) - 1)) == 0;
    const bool src_vec = r == 0 && !flip && ((W | x0) & 3) == 0 && ((uintptr_t)src & 7) == 0;
    for (uint32_t u = blockIdx.x * blockDim.x + threadIdx.x; u < units; u += gridDim.x * blockDim.x) {
        const uint32_t i = u / Wq, j = (u - i * Wq) * 4;
        const int n = min(4, Wo - (int)j);
        int y[4], co[4], cg[4];
        load_planes4(src, plane, W, r, y0 + (int)i, flip ? x0 + Wo - 1 - (int)j : x0 + (int)j, flip, n, src_vec && n == 4, y, co, cg);
        Quad<T> q[3];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            int v[3];
            ycocg_inv(y[k], co[k], cg[k], v[0], v[1], v[2]);
#pragma unroll
            for (int c = 0; c < 3; ++c) q[c].e[k] = tensor_finish<T>((float)v[c], c, nm);
        }
        store_tensor_quads(dst + (long)i * Wo + j, oplane, q, n, out_vec);
    }
}

// The last kernel of llicti_decode_images_tensor_o when its options ask for something unlift_tensor_kernel does not do: a window PADDED past its
// image, the NHWC layout, or both.  Image b's Ho x Wo window (two signed words of `wins`: pad_win_pack) is cut from its Hr x Wr decoded grid
// extended by pad.mode: row t = y0 + i and column x0 + j' (j' = Wo - 1 - j where flipped) go through pad_index, the map include/llicti_hip.h
// states -- a source index, or "fill".  A lane owns 4 consecutive output pixels of one row.  Where the row and all four columns lie INSIDE the
// grid it takes load_planes4 exactly as unlift_tensor_kernel does (its short4 path included); on the border it goes pixel by pixel: a mapped
// pixel is one gather through the same inverse and tensor_finish, a "fill" pixel the lane's three fill elements (tensor_finish of the fill, or
// the fill itself rounded to T).  Stores: PlanarStore / NhwcStore.  With LLICTI_PAD_NONE every lane is inside (the host saw to it): the values
// are unlift_tensor_kernel's.  Every source index is in 0 .. n - 1 by pad_index's construction, whatever the words hold: nothing is read
// outside the image's planes, nothing written outside the tensor.  Latches the call's status words exactly as unlift_tensor_kernel does.
template <typename T>
__global__ __launch_bounds__(256) void sink_window_kernel(const int16_t *__restrict__ planes, T *__restrict__ out, int r, int Ho, int Wo, int b0,
                                                          const PadWins wins, const TensorNorm nm, const TensorPad pad,
                                                          const int32_t *__restrict__ status, int status_head, int32_t *__restrict__ latched,
                                                          int32_t *__restrict__ img_latched, const ImgGeo *__restrict__ iv,
                                                          const int *__restrict__ rtab = nullptr)
{
    const int b = b0 + blockIdx.y;
    latch_status(status, status_head, latched, img_latched, b);
    if (rtab) r = rtab[b];      // (the _rv contract: the image's own level, wave-uniform)
    int y0, x0;
    bool flip;
    pad_win_unpack(wins.w[2 * blockIdx.y], wins.w[2 * blockIdx.y + 1], y0, x0, flip);
    const int W = iv[b].W, Hr = reduced_dim(iv[b].H, r), Wr = reduced_dim(W, r);
    const long plane = iv[b].plane;
    const int16_t *src = planes + iv[b].pix_off;
    T fill[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) fill[c] = pad.space == LLICTI_FILL_OUTPUT ? tensor_elem<T>(pad.fill[c]) : tensor_finish<T>(pad.fill[c], c, nm);
    const uint32_t Wq = (uint32_t)(Wo + 3) >> 2, units = (uint32_t)Ho * Wq;
    const bool src_vec = r == 0 && !flip && ((W | x0) & 3) == 0 && ((uintptr_t)src & 7) == 0;
    for (uint32_t u = blockIdx.x * blockDim.x + threadIdx.x; u < units; u += gridDim.x * blockDim.x) {
        const uint32_t i = u / Wq, j = (u - i * Wq) * 4;
        const int n = min(4, Wo - (int)j);
        const int row = y0 + (int)i, col = flip ? x0 + Wo - 1 - (int)j : x0 + (int)j;      // the window's coordinates of the lane's first pixel
        const int far = flip ? col - (n - 1) : col + (n - 1);                             // ... and of its last
        Quad<T> q[3];
        if (row >= 0 && row < Hr && min(col, far) >= 0 && max(col, far) < Wr) {
            int y[4], co[4], cg[4];
            load_planes4(src, plane, W, r, row, col, flip, n, src_vec && n == 4, y, co, cg);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                int v[3];
                ycocg_inv(y[k], co[k], cg[k], v[0], v[1], v[2]);
#pragma unroll
                for (int c = 0; c < 3; ++c) q[c].e[k] = tensor_finish<T>((float)v[c], c, nm);
            }
        } else {
            const int sy = pad_index(Hr, row, pad.mode);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int sx = pad_index(Wr, flip ? col - k : col + k, pad.mode);
#pragma unroll
                for (int c = 0; c < 3; ++c) q[c].e[k] = fill[c];
                if (k < n && sy >= 0 && sx >= 0) {
                    const int16_t *s = src + ((long)(sy << r) * W + ((long)sx << r));
                    int v[3];
                    ycocg_inv(s[0], s[plane], s[2 * plane], v[0], v[1], v[2]);
#pragma unroll
                    for (int c = 0; c < 3; ++c) q[c].e[k] = tensor_finish<T>((float)v[c], c, nm);
                }
            }
        }
        if (pad.layout == LLICTI_LAYOUT_NHWC) NhwcStore::put(out, (long)b, Ho, Wo, (int)i, (int)j, q, n);
        else PlanarStore::put(out, (long)b, Ho, Wo, (int)i, (int)j, q, n);
    }
}

// The resampling tile of llicti_decode_images_tensor_resized and llicti_decode_images_tensor_views: a source box (two words: origin, flip,
// extent -- decoded coordinates, plane pixel (y << r, x << r)) of image b's planes resampled to output slot `slot` of `out`, [slot][3][Ho][Wo],
// by the triangle filter of resize_axis, to the operation of include/llicti_hip.h: per row tap a the sum over the column taps of w^x_b * p, left
// to right from +0, then the sum over the row taps of w^y_a * h_a, then tensor_finish.
// A workgroup owns a 16 x 64 tile (blockIdx.x) of the output and computes the weights of its 64 columns and 16 rows ONCE into LDS (zeros behind
// the last tap: x + 0 * p == x, so the tap loops run to the tile's largest count, a wave-uniform bound, and no thread keeps a weight array); a
// flipped box's tile takes the weights of the mirrored columns.  A lane then owns 4 consecutive output pixels of one row: one 4-element store
// per channel when Wo % 4 == 0 and `out` is aligned to 4 elements, element by element otherwise.  Source indices are clamped into the box
// (only zero-weight taps ever are).
// Store: where the tile's pixels go -- PlanarStore (the default: the kernels below) or NhwcStore (sink_resize_nhwc_kernel, sink_views_nhwc_kernel).
constexpr int kResizeTileH = 16, kResizeTileW = 64;
template <typename T, typename Store = PlanarStore>
__device__ __forceinline__ void resize_tile(const int16_t *__restrict__ planes, T *__restrict__ out, long slot, int r, int Ho, int Wo, int tiles_x,
                                            int antialias, uint32_t w0, uint32_t w1, const TensorNorm &nm, const ImgGeo *__restrict__ iv, int b)
{
    __shared__ float wx[kResizeTileW][kResizeTapMax], wy[kResizeTileH][kResizeTapMax];
    __shared__ int xlo[kResizeTileW], ylo[kResizeTileH], ntap[2];
    const int y0 = (int)(w0 & 0x1FFFu), x0 = (int)((w0 >> 13) & 0x1FFFu);
    const bool flip = ((w0 >> 26) & 1u) != 0;
    const int hs = (int)(w1 & 0x1FFFu), ws = (int)((w1 >> 13) & 0x1FFFu);
    const int ty = (int)blockIdx.x / tiles_x, tx = (int)blockIdx.x - ty * tiles_x;
    const int i0 = ty * kResizeTileH, j0 = tx * kResizeTileW;
    const int tid = (int)threadIdx.x;
    if (tid < 2) ntap[tid] = 1;
    __syncthreads();
    if (tid < kResizeTileW) {
        const int j = min(j0 + tid, Wo - 1);                       // (columns behind the row's end: any valid one, never stored)
        const int n = resize_axis(ws, Wo, antialias, flip ? Wo - 1 - j : j, &xlo[tid], wx[tid], kResizeTapMax);
        atomicMax(&ntap[0], min(n, kResizeTapMax));
    } else if (tid < kResizeTileW + kResizeTileH) {
        const int k = tid - kResizeTileW;
        const int n = resize_axis(hs, Ho, antialias, min(i0 + k, Ho - 1), &ylo[k], wy[k], kResizeTapMax);
        atomicMax(&ntap[1], min(n, kResizeTapMax));
    }
    __syncthreads();
    const int li = tid >> 4, lj = (tid & 15) * 4;
    const int i = i0 + li, j = j0 + lj;
    if (i >= Ho || j >= Wo) return;
    const int nx = ntap[0], ny = ntap[1];
    const int n = min(4, Wo - j);
    const int W = iv[b].W;
    const long plane = iv[b].plane;
    const int16_t *src = planes + iv[b].pix_off;
    const int yl = ylo[li];
    float v[4][3];
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k][0] = v[k][1] = v[k][2] = 0.0f;
    for (int a = 0; a < ny; ++a) {
        const float wa = wy[li][a];
        const int16_t *row = src + (long)((y0 + min(yl + a, hs - 1)) << r) * W;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (k < n) {
                const int xl = xlo[lj + k];
                float h[3] = { 0.0f, 0.0f, 0.0f };
                for (int t = 0; t < nx; ++t) {
                    const float wb = wx[lj + k][t];
                    const int16_t *s = row + ((long)(x0 + min(xl + t, ws - 1)) << r);
                    int px[3];
                    ycocg_inv(s[0], s[plane], s[2 * plane], px[0], px[1], px[2]);
#pragma unroll
                    for (int c = 0; c < 3; ++c) h[c] = __fadd_rn(h[c], __fmul_rn(wb, (float)px[c]));
                }
#pragma unroll
                for (int c = 0; c < 3; ++c) v[k][c] = __fadd_rn(v[k][c], __fmul_rn(wa, h[c]));
            }
        }
    }
    Quad<T> q[3];
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int c = 0; c < 3; ++c) q[c].e[k] = tensor_finish<T>(v[k][c], c, nm);
    Store::put(out, slot, Ho, Wo, i, j, q, n);
}

// The last kernel of llicti_decode_images_tensor_resized, in the place of unlift_tensor_kernel: image b = b0 + blockIdx.y's box (two words of
// `boxes`, the call's kernel arguments) to out[b][3][Ho][Wo].  Latches the call's status words exactly as the other unlift kernels do.
template <typename T>
__global__ __launch_bounds__(256) void unlift_resize_tensor_kernel(const int16_t *__restrict__ planes, T *__restrict__ out, int r, int Ho, int Wo, int b0,
                                                                   int tiles_x, int antialias, const ResizeBoxes boxes, const TensorNorm nm,
                                                                   const int32_t *__restrict__ status, int status_head, int32_t *__restrict__ latched,
                                                                   int32_t *__restrict__ img_latched, const ImgGeo *__restrict__ iv,
                                                                   const int *__restrict__ rtab = nullptr)
{
    const int b = b0 + blockIdx.y;
    latch_status(status, status_head, latched, img_latched, b);
    if (rtab) r = rtab[b];      // (the _rv call: the image's own level, wave-uniform)
    resize_tile<T>(planes, out, (long)b, r, Ho, Wo, tiles_x, antialias, boxes.w[2 * blockIdx.y], boxes.w[2 * blockIdx.y + 1], nm, iv, b);
}

// The last kernel of llicti_decode_images_tensor_views: the same tile, of one VIEW's output.  View v0 + blockIdx.y of a group -- three words of
// `views`, the call's kernel arguments: origin and flip, extent, the index of the view's IMAGE -- is resampled from that image's planes to
// out[v0 + blockIdx.y][3][Ho][Wo]; views may name an image in any order, repeatedly or never.  The call's first launch (latch_n = B, every
// other one 0) latches the status words of ALL B images, those no view names included, as the other unlift kernels do for theirs.
template <typename T>
__global__ __launch_bounds__(256) void unlift_views_tensor_kernel(const int16_t *__restrict__ planes, T *__restrict__ out, int r, int Ho, int Wo, int v0,
                                                                  int tiles_x, int antialias, const ViewSlice views, const TensorNorm nm,
                                                                  const int32_t *__restrict__ status, int status_head, int32_t *__restrict__ latched,
                                                                  int32_t *__restrict__ img_latched, const ImgGeo *__restrict__ iv, int latch_n,
                                                                  const int *__restrict__ rtab = nullptr)
{
    if (blockIdx.x == 0 && blockIdx.y == 0 && latch_n > 0) latch_status_all(status, status_head, latched, img_latched, latch_n);
    const int b = (int)views.w[3 * blockIdx.y + 2];
    if (rtab) r = rtab[b];      // (the _rv call: the level of the view's IMAGE, wave-uniform)
    resize_tile<T>(planes, out, (long)v0 + blockIdx.y, r, Ho, Wo, tiles_x, antialias, views.w[3 * blockIdx.y], views.w[3 * blockIdx.y + 1], nm, iv, b);
}

// unlift_resize_tensor_kernel and unlift_views_tensor_kernel in the NHWC layout (the _o calls with LLICTI_LAYOUT_NHWC): the same tile, the same
// values, the same latches -- resize_tile with NhwcStore.
template <typename T>
__global__ __launch_bounds__(256) void sink_resize_nhwc_kernel(const int16_t *__restrict__ planes, T *__restrict__ out, int r, int Ho, int Wo, int b0,
                                                               int tiles_x, int antialias, const ResizeBoxes boxes, const TensorNorm nm,
                                                               const int32_t *__restrict__ status, int status_head, int32_t *__restrict__ latched,
                                                               int32_t *__restrict__ img_latched, const ImgGeo *__restrict__ iv,
                                                               const int *__restrict__ rtab = nullptr)
{
    const int b = b0 + blockIdx.y;
    latch_status(status, status_head, latched, img_latched, b);
    if (rtab) r = rtab[b];
    resize_tile<T, NhwcStore>(planes, out, (long)b, r, Ho, Wo, tiles_x, antialias, boxes.w[2 * blockIdx.y], boxes.w[2 * blockIdx.y + 1], nm, iv, b);
}

template <typename T>
__global__ __launch_bounds__(256) void sink_views_nhwc_kernel(const int16_t *__restrict__ planes, T *__restrict__ out, int r, int Ho, int Wo, int v0,
                                                              int tiles_x, int antialias, const ViewSlice views, const TensorNorm nm,
                                                              const int32_t *__restrict__ status, int status_head, int32_t *__restrict__ latched,
                                                              int32_t *__restrict__ img_latched, const ImgGeo *__restrict__ iv, int latch_n,
                                                              const int *__restrict__ rtab = nullptr)
{
    if (blockIdx.x == 0 && blockIdx.y == 0 && latch_n > 0) latch_status_all(status, status_head, latched, img_latched, latch_n);
    const int b = (int)views.w[3 * blockIdx.y + 2];
    if (rtab) r = rtab[b];
    resize_tile<T, NhwcStore>(planes, out, (long)v0 + blockIdx.y, r, Ho, Wo, tiles_x, antialias, views.w[3 * blockIdx.y], views.w[3 * blockIdx.y + 1], nm, iv, b);
}

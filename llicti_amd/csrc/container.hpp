// container.hpp -- container assembly kernels: header write / read, stream pack / unpack.
// Part of the single translation unit llicti_hip.hip (included in order; not a stand-alone header).
#pragma once

// ------------------------------------------------------------------------------------------------ container kernels
// The part of a header that does not depend on where the pixels come from, by ONE thread of the three header writers below: the 17 fixed bytes
// at o and the image's segment lengths sl[0 .. 3] (and zeros for the segments a model of fewer levels does not have); mm: the image's four
// min / max words.  Each writer adds the raw DC band behind it.
__device__ __forceinline__ void header_fixed(uint8_t *__restrict__ o, const ImgGeo &ig, const int32_t *__restrict__ mm, int32_t *__restrict__ sl)
{
    o[0] = (uint8_t)ig.byte0; o[1] = (uint8_t)ig.h4; o[2] = (uint8_t)ig.w4;    // LLICTI_nets.py:347 (AC: number of scales)
    const int16_t v[6] = { 0, (int16_t)mm[0], (int16_t)mm[1], 255, (int16_t)mm[2], (int16_t)mm[3] };   // :139, :348
    for (int k = 0; k < 6; ++k) { o[3 + 2 * k] = (uint8_t)(v[k] & 0xFF); o[4 + 2 * k] = (uint8_t)((v[k] >> 8) & 0xFF); }
    o[15] = (uint8_t)(ig.padint & 0xFF); o[16] = (uint8_t)((ig.padint >> 8) & 0xFF);                   // :349
    sl[0] = 3; sl[1] = 12; sl[2] = 2; sl[3] = 3 * ig.h4 * ig.w4;
    for (int k = ig.nseg; k < LLICTI_NSEG; ++k) sl[k] = 0;
}

// encode: header segments straight into the container; seg_len[b][0..3]
__global__ void header_write_kernel(const uint8_t *__restrict__ rgb, const int32_t *__restrict__ minmax, const ImgGeo *__restrict__ iv,
                                    uint8_t *__restrict__ out, long out_stride, int32_t *__restrict__ seg_len, unsigned long long *__restrict__ ssum)
{
    const int b = blockIdx.x;
    if (ssum && threadIdx.x == 0) ssum[b] = 0ull;       // "auto" encodes: the image's last-stage cost is summed into it later in the call (choose_streams_kernel)
    uint8_t *o = out + (long)b * out_stride;
    const ImgGeo ig = iv[b];
    const int W = ig.W, h4 = ig.h4, w4 = ig.w4;
    const long plane = ig.plane;
    if (threadIdx.x == 0) header_fixed(o, ig, minmax + 4 * b, seg_len + (long)b * LLICTI_NSEG);
    const int dcs = ig.dcs;                                                      // the last level's x00 (32 for 5 levels)
    for (int t = threadIdx.x; t < 3 * h4 * w4; t += blockDim.x) {                                        // :248-252, :350
        const int c = t / (h4 * w4), r = t - c * h4 * w4, i = r / w4, j = r - i * w4;
        o[17 + t] = rgb[ig.rgb_off + c * plane + (long)(dcs * i) * W + dcs * j];
    }
}

// header_write_kernel of llicti_encode_images_px: the raw DC band is read from the caller's interleaved pixels through image b's window
// (PixGeo), colour c of a pixel at byte c of it (2 - c where blue comes first)
__global__ void header_write_px_kernel(const uint8_t *__restrict__ pix, const PixGeo *__restrict__ pv, const int32_t *__restrict__ minmax,
                                       const ImgGeo *__restrict__ iv, uint8_t *__restrict__ out, long out_stride, int32_t *__restrict__ seg_len,
                                       unsigned long long *__restrict__ ssum)
{
    const int b = blockIdx.x;
    if (ssum && threadIdx.x == 0) ssum[b] = 0ull;
    uint8_t *o = out + (long)b * out_stride;
    const ImgGeo ig = iv[b];
    const PixGeo pg = pv[b];
    const int h4 = ig.h4, w4 = ig.w4;
    if (threadIdx.x == 0) header_fixed(o, ig, minmax + 4 * b, seg_len + (long)b * LLICTI_NSEG);
    const int dcs = ig.dcs, bpp = pix_bpp(pg.fmt);
    for (int t = threadIdx.x; t < 3 * h4 * w4; t += blockDim.x) {
        const int c = t / (h4 * w4), r = t - c * h4 * w4, i = r / w4, j = r - i * w4;
        o[17 + t] = pix[pg.off + (long)(dcs * i) * pg.pitch + (long)(dcs * j) * bpp + (pix_bgr(pg.fmt) ? 2 - c : c)];
    }
}

// header_write_kernel of llicti_transcode_images, which has no pixels: the header in the TARGET container's form (iv: the target plan's
// table); the min / max words are the ones the decoder read from the source header, and the raw DC band is the decoder's planes at the DC
// stride, taken back through the integer lift (a rejected source header left mid grey there).  The call's first kernel on the target side:
// it clears the target plan's n_zero status words (block 0; zero == nullptr: none, llicti_encode_images_f32 whose lift has cleared them).
__global__ void header_transcode_kernel(const int16_t *__restrict__ planes, const int32_t *__restrict__ minmax, const ImgGeo *__restrict__ iv,
                                        uint8_t *__restrict__ out, long out_stride, int32_t *__restrict__ seg_len, unsigned long long *__restrict__ ssum,
                                        int32_t *__restrict__ zero, int n_zero)
{
    const int b = blockIdx.x;
    if (b == 0) clear_status(zero, n_zero);
    if (ssum && threadIdx.x == 0) ssum[b] = 0ull;
    uint8_t *o = out + (long)b * out_stride;
    const ImgGeo ig = iv[b];
    const int W = ig.W, h4 = ig.h4, w4 = ig.w4;
    const long plane = ig.plane;
    if (threadIdx.x == 0) header_fixed(o, ig, minmax + 4 * b, seg_len + (long)b * LLICTI_NSEG);
    const int dcs = ig.dcs;
    for (int t = threadIdx.x; t < h4 * w4; t += blockDim.x) {
        const int i = t / w4, j = t - i * w4;
        const long off = ig.pix_off + (long)(dcs * i) * W + dcs * j;
        int R, G, Bl;
        ycocg_inv(planes[off], planes[off + plane], planes[off + 2 * plane], R, G, Bl);
        o[17 + t] = (uint8_t)R; o[17 + h4 * w4 + t] = (uint8_t)G; o[17 + 2 * h4 * w4 + t] = (uint8_t)Bl;
    }
}

// encode: copy the 45 slots of image b behind its header, tightly; seg_len[b][4..48].  st0: the model's first stage (host_plan.hpp: first_stage;
// 0 for 5 levels) -- stage st0 + x is segment 4 + x.
__global__ __launch_bounds__(256) void pack_kernel(const uint8_t *__restrict__ slots, const long *__restrict__ slot_off,
                                                   const int32_t *__restrict__ slot_len, int B, int hdr_bytes,
                                                   uint8_t *__restrict__ out, long out_stride, int32_t *__restrict__ seg_len,
                                                   int32_t *status, int st0)
{
    const int st = st0 + blockIdx.x, b = blockIdx.y;
    // slot index: streams are stored stage-major, image-minor (see build_plan)
    long dst = hdr_bytes;
    for (int k = st0; k < st; ++k) dst += slot_len[(long)k * B + b];
    const int n = slot_len[(long)st * B + b];
    if (dst + n > out_stride) { if (threadIdx.x == 0) atomicExch(&status[0], LLICTI_ENOSPACE); return; }
    const uint8_t *src = slots + slot_off[(long)st * B + b];
    uint8_t *o = out + (long)b * out_stride + dst;
    block_copy_bytes(o, src, n);
    if (threadIdx.x == 0) seg_len[(long)b * LLICTI_NSEG + 4 + st - st0] = n;
}

// decode: parse + validate header, min/max -> minmax[b][4], DC band -> planes at the DC stride (32 for 5 levels)
__global__ void header_read_kernel(const uint8_t *__restrict__ in, long in_stride, const int32_t *__restrict__ seg_len,
                                   const ImgGeo *__restrict__ iv, int16_t *__restrict__ planes,
                                   float *__restrict__ fplanes, int32_t *__restrict__ minmax, int32_t *status)
{
    const int b = blockIdx.x;
    const uint8_t *p = in + (long)b * in_stride;
    const int32_t *sl = seg_len + (long)b * LLICTI_NSEG;
    const ImgGeo ig = iv[b];
    const int byte0 = ig.byte0;
    const int W = ig.W, h4 = ig.h4, w4 = ig.w4, padint = ig.padint;
    const long plane = ig.plane;
    __shared__ int ok;
    __shared__ int sh_bad;
    __shared__ unsigned long long sh_tot;
    if (threadIdx.x == 0) { sh_bad = 0; sh_tot = 0ull; }
    __syncthreads();
    if ((int)threadIdx.x < ig.nseg) {              // the 49 lengths in parallel (one thread walking them was most of this kernel's 70 us; config B: its 22)
        const int v = sl[threadIdx.x];
        if (v < 0 || v > in_stride) atomicOr(&sh_bad, 1);
        atomicAdd(&sh_tot, (unsigned long long)((v < 0) ? 0 : v));
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        // every segment length is checked before a single container byte is read: a malformed seg_len must end in
        // LLICTI_EFORMAT, never in an access outside [in, in + in_stride)
        const long tot = (long)sh_tot;
        bool segs_ok = in_stride >= 17 + 3L * h4 * w4 && !sh_bad;
        if (tot > in_stride) segs_ok = false;
        ok = segs_ok && (sl[0] == 3 && sl[1] == 12 && sl[2] == 2 && sl[3] == 3 * h4 * w4);
        if (ok) {
            const int pad = (int)(uint16_t)(p[15] | (p[16] << 8));      // (xwide v4 containers carry their stream count in bits 10 .. 15: ig.padint has them)
            ok = (p[0] == byte0 && p[1] == h4 && p[2] == w4 && pad == padint);           // LLICTI_nets.py:423-428
        }
        if (!ok) flag_image(status, b, LLICTI_EFORMAT);
        int16_t v[6] = { 0, -255, -255, 255, 255, 255 };
        if (ok) for (int k = 0; k < 6; ++k) v[k] = (int16_t)(p[3 + 2 * k] | (p[4 + 2 * k] << 8));
        int32_t *mm = minmax + 4 * b;
        mm[0] = v[1]; mm[1] = v[2]; mm[2] = v[4]; mm[3] = v[5];
        if (v[1] > v[4] || v[2] > v[5] || v[1] < -255 || v[2] < -255 || v[4] > 255 || v[5] > 255) {
            flag_image(status, b, LLICTI_EFORMAT);
            mm[0] = mm[1] = -255; mm[2] = mm[3] = 255;
        }
    }
    __syncthreads();
    // a rejected header still gets a DC band (mid grey): the 45 stages run for every image of the batch, and what they write
    // must not depend on what an earlier call left in the shared workspace (the image is flagged: llicti_image_status)
    const uint8_t *dc = p + 17;
    const int dcs = ig.dcs;
    for (int t = threadIdx.x; t < h4 * w4; t += blockDim.x) {                              // :429-430, :443-444
        const int i = t / w4, j = t - i * w4;
        const int R = ok ? dc[t] : 128, G = ok ? dc[h4 * w4 + t] : 128, Bl = ok ? dc[2 * h4 * w4 + t] : 128;
        int Y, Co, Cg;
        ycocg_fwd(R, G, Bl, Y, Co, Cg);
        const long off = ig.pix_off + (long)(dcs * i) * W + dcs * j;
        planes[off] = (int16_t)Y; planes[off + plane] = (int16_t)Co; planes[off + 2 * plane] = (int16_t)Cg;
        fplanes[off] = (float)Y / 255.0f; fplanes[off + plane] = (float)Co / 255.0f; fplanes[off + 2 * plane] = (float)Cg / 255.0f;
    }
}

// decode: copy stream st of image b into its 4-byte aligned, zero padded slot (segment 4 + st - st0, see pack_kernel)
__global__ __launch_bounds__(256) void unpack_kernel(const uint8_t *__restrict__ in, long in_stride, const int32_t *__restrict__ seg_len,
                                                     int B, uint8_t *__restrict__ slots, const long *__restrict__ slot_off,
                                                     const int32_t *__restrict__ slot_cap, int32_t *__restrict__ slot_len, int32_t *status, int st0)
{
    const int st = st0 + blockIdx.x, b = blockIdx.y, seg = 4 + blockIdx.x;
    const int32_t *sl = seg_len + (long)b * LLICTI_NSEG;
    long src = 0;
    bool bad = false;
    for (int k = 0; k < seg; ++k) {          // a negative or oversized EARLIER entry must not move src outside the container
        const int v = sl[k];
        if (v < 0 || v > in_stride) bad = true;
        src += v;
        if (src < 0 || src > in_stride) { bad = true; src = 0; }
    }
    int n = sl[seg];
    const int cap = slot_cap[(long)st * B + b];
    if (bad || n < 0 || n + 16 > cap || src + n > in_stride) { if (threadIdx.x == 0) flag_image(status, b, LLICTI_EFORMAT); n = 0; src = 0; }
    const uint8_t *p = in + (long)b * in_stride + src;
    uint8_t *o = slots + slot_off[(long)st * B + b];
    block_copy_bytes(o, p, n);
    const int padded = min(cap, ((n + 3) & ~3) + 16);
    for (int t = n + threadIdx.x; t < padded; t += blockDim.x) o[t] = 0;
    if (threadIdx.x == 0) slot_len[(long)st * B + b] = n;       // the decoders read nothing past it
}

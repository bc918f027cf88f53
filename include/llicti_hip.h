/*
 * llicti_hip.h -- C-ABI of the MI355X-native LLICTI encode/decode hot path (libllicti_hip.so).
 *
 * The reference (kamisli-icpl/LLICTI) has no FFI: its seam for this path is Python-method level
 * (SURVEY.md section 8b).  Every entry point below names the reference call site it replaces; the
 * ctypes binding a maintainer would add on the reference side is shown in INTEGRATION.md.
 *
 * Conventions
 *   - plain C types only; device buffers are raw pointers obtained from the caller's allocator
 *     (e.g. torch.Tensor.data_ptr()); `stream` is a hipStream_t passed as void* (NULL = default stream)
 *   - every function returns 0 on success or a negative LLICTI_E* code; llicti_last_error() gives the
 *     message of the calling thread's last failure
 *   - nothing allocates device memory except llicti_create (status word, 1 MB of lift partials, streams and events
 *     of the AC decode pipeline), llicti_set_band_weights (weights) and a whole-batch call whose (mode, image sizes) the
 *     context has not seen lately (the plan's per-image tables, 0.1 - 0.3 MB of device + pinned host memory from a pool of
 *     blocks that are reused and never freed before llicti_destroy) -- all working memory comes from the caller-sized
 *     workspace (llicti_workspace_bytes / llicti_workspace_bytes_v)
 *   - launches are asynchronous on `stream`; functions that return host-visible results say so and
 *     synchronise the stream themselves
 *   - one context per GPU / host thread; a context is not thread-safe and its calls must not overlap on different
 *     streams (llicti_decode_images with the AC container fans out over two internal streams and joins back on `stream`;
 *     llicti_encode_images with the tuning switch "enc_side_levels" runs its coarse levels on one internal stream and joins back before
 *     the entropy coder)
 *   - a caller that takes a context from one stream to another orders the two itself (an event or hipStreamWaitEvent, so that the next call
 *     starts behind the previous one: calls of one context never overlap), as it orders its own buffers -- inputs, outputs and the workspace
 *     belong to a call until its stream has passed it.  The library orders everything of its own: a call waits on `stream` for a cached
 *     plan's tables that were uploaded or last used on another stream, forks its internal streams behind `stream` and joins them back onto it
 *     before it returns, hands a pooled table block to a new plan only once the block's last user has finished, and llicti_check_status /
 *     llicti_image_status wait for, read and clear on `stream` alone -- no kernel-level, whole-batch or status call uses the null stream unless it
 *     is given it (tests/test_hip_streams.py)
 *   - every call makes the context's device current for its own duration and restores the caller's current device
 *   - calls that BLOCK the host: llicti_create / llicti_destroy / llicti_set_band_weights (device-wide synchronise:
 *     work in flight may still read the old weights), llicti_check_status and llicti_last_timing (they return
 *     host-visible results).  A whole-batch call of a new (mode, image sizes) builds its plan on the host (tens of
 *     microseconds) and enqueues ONE asynchronous upload of its tables on the call's stream: it does not synchronise the
 *     device (the cache holds 32 plans, least recently used out first; a block that leaves it waits in the pool until its
 *     last user has finished -- the reference's own test set has 119 image sizes among 500 images, interleaved)
 *   - 32 <= H, W <= 8160 (the header stores h4, w4 as uint8, LLICTI_nets.py:347).  llicti_encode_images /
 *     llicti_decode_images take B images of ONE size; llicti_encode_images_v / llicti_decode_images_v take a size per
 *     image (the reference's test loader yields images of arbitrary sizes one at a time, dataloaders/image_dl.py:40-45):
 *     same kernels, same bytes per image as a call of its own -- an image's container never depends on its batch
 *
 * Data layout in HBM
 *   rgb     uint8  [B][3][H][W]   planar
 *   planes  int16  [B][3][H][W]   Y-127, Co, Cg (YCoCg-R); the polyphase bands of every level are
 *                                 strided views of these planes: band (oi,oj) of level l, pixel (i,j)
 *                                 is planes[.., (2i+oi)<<l, (2j+oj)<<l]  (lazyDWT, LLICTI_nets.py:218-225)
 *   fplanes float  [B][3][H][W]   planes / 255 (one IEEE division, LLICTI_nets.py:143-144)
 *   params  float  [B][64][h*w]   raw CNN outputs on the band grid of one (level, band), CHANNEL-PLANAR: 4 heads x 16 planes
 *                                 (15 used), reference channel o is plane (o/15)*16 + o%15; position (i, j) at i*w + j -- a
 *                                 decoder wavefront's consecutive symbols read consecutive floats of the planes it needs
 *   tables  uint16 [B][hc*wc][stride]  integer CDF rows of one stream (stride = Lp rounded up to 8)
 */
#ifndef LLICTI_HIP_H
#define LLICTI_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LLICTI_OK            0
#define LLICTI_EINVAL       -1   /* bad argument (shape, pointer, level/band index) */
#define LLICTI_EHIP         -2   /* a HIP runtime call failed */
#define LLICTI_ENOWEIGHTS   -3   /* llicti_set_band_weights has not been called for every band */
#define LLICTI_ENOSPACE     -4   /* workspace or output buffer too small */
#define LLICTI_EFORMAT      -5   /* malformed container (decode) */
#define LLICTI_ENODEVICE    -6   /* no usable gfx950 device */

#define LLICTI_NLEVELS   5
#define LLICTI_NSTREAMS 45      /* 5 levels x 3 bands x 3 colour channels per image */
#define LLICTI_NSEG     49      /* 4 header segments + 45 streams (the reference's bytestream_list) */
#define LLICTI_NPARAMS  60      /* mixture parameters per position: 15 sigma | 15 mu | 15 weight | 5 a | 5 b | 5 d */
#define LLICTI_PARAM_STRIDE 64  /* channel planes per (image, level, band) in HBM: 4 heads x 16 (15 used): reference channel o is plane (o/15)*16 + o%15 */

typedef struct llicti_ctx llicti_ctx;

const char *llicti_last_error(void);
const char *llicti_version(void);

/* Context on HIP device `device`.  Fails with LLICTI_ENODEVICE when no GPU is present: there is no
 * CPU fallback. */
int llicti_create(llicti_ctx **ctx, int device);
int llicti_destroy(llicti_ctx *ctx);

/* Model shape of the context: head = channels per head (chs[0]), nlevels = wavelet levels.  This build runs exactly the reference's two
 * configurations: (88, 5) = configs/llicti_A.json, the default of a new context, and (60, 2) = configs/llicti_B.json.  Anything else is
 * LLICTI_EINVAL.  Changing the shape drops the context's weights (llicti_set_band_weights again) and cached plans.  Under config B the container
 * has 4 + 9 x 2 = 22 segments (the DC band is level 1's x00), the level-indexed entry points take lvl 0 .. 1, and the whole-batch calls take
 * LLICTI_MODE_AC and LLICTI_MODE_RANS_X(1 .. 18) / LLICTI_MODE_RANS_X_AUTO(1 .. 13) (LLICTI_EINVAL otherwise) on images of at most 1020
 * pixels per side (the header stores level 1's grid in one byte each).  A context refuses the other model's containers (LLICTI_EFORMAT per
 * image): config B's reference-format header has byte 0 = 2 (its number of scales), its xwide v4 header byte 0 = 0xE9. */
int llicti_set_model(llicti_ctx *ctx, int head, int nlevels);

/* Upload one band network in canonical packed form (host pointers, float32), for the context's model (head h = 88 or 60):
 *   w0 [4h][K0] (K0 = 48 / 72 / 120), b0 [4h], w1 [4h][h], b1 [4h], w2 [60][h], b2 [60].
 * Replaces LLICTIEntropyModel4.__init__ / load_state_dict for the eval path
 * (LLICTI_nets.py:651-675, :695-712; agents/base.py:51-76). */
int llicti_set_band_weights(llicti_ctx *ctx, int band, int K0, const float *w0, const float *b0,
                            const float *w1, const float *b1, const float *w2, const float *b2);

/* Level geometry helper (host only): Hl = ceil(H/2^l), band grid h = ceil(Hl/2), pad flag = Hl odd;
 * coded (cropped) size of `band`'s streams in hc, wc (LLICTI_nets.py:226-230, :396-397). */
int llicti_level_geom(int H, int W, int lvl, int band, int *Hl, int *Wl, int *h, int *w,
                      int *padH, int *padW, int *hc, int *wc);

/* ---- kernel-level entry points ------------------------------------------------------------------ */

/* K1-K3: uint8 RGB -> YCoCg-R planes (+ float copy) and per-image min/max of Co, Cg.
 * d_minmax: int32 [B][4] = minCo, minCg, maxCo, maxCg.
 * Replaces get_YCoCg_R_from_RGB__intOps + min()/max().item() + x/255 (LLICTI_nets.py:62-74, :137-144). */
int llicti_lift_u8(llicti_ctx *ctx, const uint8_t *d_rgb, int B, int H, int W,
                   int16_t *d_planes, float *d_fplanes, int32_t *d_minmax, void *stream);

/* K13: planes -> uint8 RGB.  Replaces get_RGB_from_YCoCg_R__intOps (LLICTI_nets.py:76-88, :174-175). */
int llicti_unlift_u8(llicti_ctx *ctx, const int16_t *d_planes, int B, int H, int W, uint8_t *d_rgb, void *stream);

/* K4+K5: interpolator CNN of one (level, band) for every position of the h x w band grid of every
 * image -> d_params [B][64][h*w] (LLICTI_PARAM_STRIDE channel planes).  fp32 MFMA, k-ordered accumulation (bit-exact to the numerics spec).
 * Replaces LLICTIEntropyModel4.get_params (LLICTI_nets.py:721-753, :822-825). */
int llicti_band_params_f32(llicti_ctx *ctx, const float *d_fplanes, int B, int H, int W, int lvl, int band,
                           float *d_params, void *stream);

/* Training / validation likelihood path (adjacent to the codec, same CNN kernel).
 * llicti_lift_train_f32: uint8 RGB -> float planes [B][3][H][W] = (Y - 127/255, Co, Cg) of the FLOAT lift with
 * torch.round (half to even), bit-exact to the reference's elementwise fp32 ops.
 * Replaces get_YCoCg_R_from_RGB + "x[:,0] -= mean_y_ycocg" (LLICTI_nets.py:40-49, :108-110).
 * llicti_selfinfo_f32: -log2 of the mixture likelihood of every target pixel of (lvl, band):
 * d_bits [B][3 (Y, Co, Cg)][h][w]; d_params from llicti_band_params_f32 on the same planes.
 * Replaces LLICTIEntropyModel4.get_self_infos (LLICTI_nets.py:862-880, :933-935) and
 * GaussianConditionalLosslessGMM.forward / _likelihood_fk (entropy_layer_nets.py:117-139, :160-183). */
int llicti_lift_train_f32(llicti_ctx *ctx, const uint8_t *d_rgb, int B, int H, int W, float *d_fplanes, void *stream);
int llicti_selfinfo_f32(llicti_ctx *ctx, const float *d_fplanes, const float *d_params, int B, int H, int W,
                        int lvl, int band, float *d_bits, void *stream);

/* K6-K8 (full table): integer CDF rows of stream (lvl, band, clr) for every coded position:
 * d_tables [B][hc*wc][row_stride] uint16, row_stride >= Lp (entries beyond Lp are 0xFFFF).
 * Replaces the cross-channel mean update + LLICTIEntropyModel4.get_cdfs(int_cdf=True)
 * (LLICTI_nets.py:385-392, :938-983; entropy_layer_nets.py:185-204). */
int llicti_cdf_u16(llicti_ctx *ctx, const int16_t *d_planes, const float *d_params, const int32_t *d_minmax,
                   int B, int H, int W, int lvl, int band, int clr, uint16_t *d_tables, int row_stride, void *stream);

/* K6-K9 (encoder form): for every coded position of (lvl, band) and each colour channel, only the two
 * table entries the coder reads, packed (c_high & 0xFFFF) << 16 | c_low (c_high == 0x10000 is stored as 0),
 * written in stream order to d_pairs[clr][B][hc*wc]. */
int llicti_cdf_pairs_u32(llicti_ctx *ctx, const int16_t *d_planes, const float *d_params, const int32_t *d_minmax,
                         int B, int H, int W, int lvl, int band, uint32_t *d_pairs, void *stream);

/* K10: torchac-compatible arithmetic ENCODER on explicit tables -- the reference's third-party seam
 * torchac.encode_int16_normalized_cdf(cdf, sym) (LLICTI_nets.py:406-407).  n_streams independent
 * streams of N symbols; d_cdf [n_streams][N][row_stride] uint16 (Lp valid entries), d_sym [n_streams][N]
 * int16; bytes of stream s go to d_out + s*out_stride (4-byte aligned, out_stride a multiple of 4 and
 * >= 2N + 8), its length to d_len[s]. */
int llicti_ac_encode_u16cdf(llicti_ctx *ctx, const uint16_t *d_cdf, int Lp, int row_stride, const int16_t *d_sym,
                            int n_streams, long N, uint8_t *d_out, long out_stride, int32_t *d_len, void *stream);

/* K11: the matching DECODER, torchac.decode_int16_normalized_cdf (LLICTI_nets.py:492-493).
 * d_in + s*in_stride holds stream s (4-byte aligned, in_stride a multiple of 4, d_len[s] <= in_stride); bytes past
 * d_len[s] are never interpreted: like torchac's reader the decoder shifts in zero bits once the stream is exhausted. */
int llicti_ac_decode_u16cdf(llicti_ctx *ctx, const uint16_t *d_cdf, int Lp, int row_stride, const uint8_t *d_in,
                            long in_stride, const int32_t *d_len, int n_streams, long N, int16_t *d_sym, void *stream);

/* ---- whole-batch entry points (LLICTI.compress / LLICTI.decompres, LLICTI_nets.py:125-179) -------
 * Containers stay in HBM.  Image b's container is the reference's bytestream_list flattened: its 49
 * segments concatenated tightly at d_out + b*out_stride, lengths in d_seg_len[b][49]; segment order
 * [S,h4,w4 u8] | 6 x int16 min/max | int16 padHW | raw DC band u8 CHW | 45 streams, scale 4..0 x band
 * x (Y,Co,Cg)  (LLICTI_nets.py:347-354, :411).  Both calls are asynchronous on `stream` (except for the first
 * call of a new shape, see "calls that BLOCK" above); device-side failures (malformed header or segment lengths,
 * stream overflow) are latched in the context and reported by llicti_check_status.  A malformed container is a
 * reported error, never a memory fault: every segment length is validated against in_stride before any byte of the
 * container is read, and no read leaves [d_in + b*in_stride, d_in + (b+1)*in_stride). */

/* mode: LLICTI_MODE_AC = the reference's container (45 torchac-algorithm streams per image, bit-exact
 * to the oracle / reference format); LLICTI_MODE_RANS*(M) = the rANS containers, NEW formats of this
 * build (BASELINE.json north_star: "torchac replaced by a HIP rANS coder"): header byte 0 = bit 7 (rANS) | bit 3 (format v3 or later; the
 * retired v2 tag has it clear and is rejected with LLICTI_EFORMAT) | bit 6 (extended) | v in bits 5,4,2,1,0 with M = v + 1; extended:
 * v = 0 / 1 = 64 / 128 streams (latency modes), v = 2 .. 15 = v - 1 wide streams (LLICTI_MODE_RANS_WIDE), v = 16 (byte 0 = 0xE8) = xwide streams
 * in the v4 layout (LLICTI_MODE_RANS_X), their COUNT in bits 10 .. 15 of the header's int16 pad field (1 .. 32 as they are, 33 / 34 = 64 / 128
 * streams; zero in every other container).  v = 17 .. 31 were the xwide tags of the v3 layout (rounds 4-5): retired, LLICTI_EFORMAT; a reader of
 * the older formats refuses a v4 container because its pad field contradicts the image size.  Then M independent
 * L-way interleaved rANS streams per image (L = 64 lanes, 128 for wide, 256 for xwide streams; segments 4 .. 4+M-1, the other stream segments
 * empty), same CDFs and symbols, decodable L*M symbols at a time.  States live in [2^31, 2^32) and renormalise bit by bit (the coder loses
 * ~2^-16 of a symbol's length, like the range coder); the L INITIAL states of a stream carry the last T symbols of the stream's last stage,
 * coded by a single-state tail coder.  64 / 128 lanes (v3): stream = u16 (T | pad << 11) | bit region | L x 31-bit final states.  xwide (v4):
 * stream = bit region | 256 x 31-bit final states; the tail coder's output is not cut to the 7,936 payload bits -- T is a multiple of 32 and
 * what exceeds the payload lies at the bottom of the bit region --; the tail is one chain that starts from the stream's last symbol itself, or
 * two seeded chains where symbols are expensive; the header field (T / 32, the one-chain flag) sits on top of the bit region under an end marker.
 * Cost over the ideal code length: about 6 bytes per 64-lane stream that has symbols, 2.5 - 5 per xwide v4 stream (the reference format's 45
 * stream terminations cost about 25 bytes per image).  Format: oracle/llicti_oracle.h, DESIGN.md section 5. */
#define LLICTI_MODE_AC        0
#define LLICTI_MODE_RANS(M)  (0x100 | (M))      /* M in 1 .. 32: one stream per segment; {64, 128}: latency modes for single / large
                                                  images, M / 32 streams per segment behind a table of their u32 lengths (+6 bytes per stream) */
#define LLICTI_MODE_RANS_WIDE(M) (0x300 | (M))  /* M in 1 .. 14 WIDE streams: 128 lanes per stream (two 64-symbol chunks per coder step, 128 x
                                                  31-bit states, about twice the tail symbols), header byte 0 = bit 6 set with v = M + 1; two decoder lanes per symbol */
#define LLICTI_MODE_RANS_X(M) (0x500 | (M))     /* M in 1 .. 32, 64, 128 XWIDE streams (v4 layout): 256 lanes per stream, header byte 0 = 0xE8, the count in the pad field's
                                                  bits 10 .. 15 (64 / 128: two / four streams per segment); ONE decoder lane per symbol, four wavefronts per stream: the fewest
                                                  vector instructions per symbol of the three (15 per 768x512 image are inside +0.001 bpp of the reference format on natural-like content) */
#define LLICTI_MODE_RANS_X_AUTO(M) (0x10500 | (M))  /* ENCODE ONLY.  xwide v4 streams whose count the ENCODER picks per image, on the device, from the image itself: M (1 .. 32) is the
                                                  count the image's size gives (llicti_amd.codec.image_streams); an image whose last stage's symbols are expensive (sum of
                                                  16 - floor(log2 freq) >= 11 per symbol: an xwide stream costs ~2.5 bytes there) gets M + ceil(M / 3) streams (at most 32), one
                                                  whose symbols are cheap (< 4: ~5 bytes per stream, long serial tails) ceil(2 M / 3), every other M; and a count M' so chosen
                                                  whose payloads of 7,936 bits the last stage cannot fill with a tenth to spare -- 2 S - n < 2 * 8704 M', S the sum above over
                                                  the last stage's n symbols -- falls to M if M' > M and 2 S - n >= 2 * 8704 M, else to ceil(M / 2).  A pure function of the image: its
                                                  container does not depend on the batch, the device or anything coded before.  The container is an ordinary
                                                  LLICTI_MODE_RANS_X(count) container -- its header says which (llicti_header_mode) -- and is decoded as such. */

/* The bound on a stream's bits.  The rANS coders keep a stream's bit position in a signed 32-bit word, so a stream takes fewer than 2^28 bytes:
 * every whole-batch encode, decode and transcode (llicti_encode_images*, llicti_decode_images*, llicti_transcode_images) returns LLICTI_EINVAL for
 * a call in which one stream's worst case -- 2 bytes per symbol of its share of the image, chunks dealt round-robin, plus fixed terms -- is 2^28
 * bytes or more; the message names the image, its size, its stream count and the smallest count that fits; the size queries return 0.  An
 * LLICTI_MODE_RANS_X_AUTO(M) image is held to ceil(M / 2) streams, the fewest its encoder may pick.  Only ONE stream on an image of about 45 M
 * pixels or more meets it (8160 pixels wide: from 5,489 rows; xwide: 5,488): 8160x8160 takes any mode with two streams or more, and LLICTI_MODE_AC. */

/* Bytes of device workspace the calls below need for B images of H x W in `mode` (_v: of Hs[b] x Ws[b]).  0: a call the library refuses. */
size_t llicti_workspace_bytes(int B, int H, int W, int mode);
size_t llicti_workspace_bytes_v(int B, const int *Hs, const int *Ws, int mode);
size_t llicti_workspace_bytes_vm(int B, const int *Hs, const int *Ws, const int *modes);      /* one mode per image, see llicti_encode_images_vm */
/* Upper bound of the container size of ONE image: the minimum out_stride / in_stride. */
size_t llicti_max_container_bytes(int H, int W);
/* The same two sizes for the context's model (llicti_set_model; the functions above size config A): modes holds one mode (n_modes = 1) or
 * one per image (n_modes = B). */
size_t llicti_workspace_bytes_ctx(const llicti_ctx *ctx, int B, const int *Hs, const int *Ws, const int *modes, int n_modes);
size_t llicti_max_container_bytes_ctx(const llicti_ctx *ctx, int H, int W);

int llicti_encode_images(llicti_ctx *ctx, const uint8_t *d_rgb, int B, int H, int W, int mode,
                         void *d_workspace, size_t workspace_bytes,
                         uint8_t *d_out, size_t out_stride, int32_t *d_seg_len, void *stream);

/* H and W must be the size the headers describe (llicti_header_dims on a host copy of the first 17
 * bytes); every image of the call has that size. */
int llicti_decode_images(llicti_ctx *ctx, const uint8_t *d_in, size_t in_stride, const int32_t *d_seg_len,
                         int B, int H, int W, int mode, void *d_workspace, size_t workspace_bytes,
                         uint8_t *d_rgb, void *stream);

/* Batches of MIXED sizes (the reference's eval loop, agents/llicti_agent.py:122-164, meets a different H x W at almost every step;
 * what it does one image at a time these calls do for B images at once).  Hs, Ws: host arrays of B sizes.  rgb_off: host array of B byte
 * offsets into d_rgb, image b's uint8 [3][Hs[b]][Ws[b]] block at d_rgb + rgb_off[b]; NULL = the blocks tightly packed in call order.
 * Containers as above: image b's at d_out + b*out_stride (out_stride >= llicti_max_container_bytes of the largest image), its 49 segment
 * lengths in d_seg_len[b].  Image b's bytes equal those of llicti_encode_images(B = 1) on that image, whatever else is in the batch.
 * rANS containers only: the reference-format container (LLICTI_MODE_AC) codes equal sizes per call (LLICTI_EINVAL otherwise). */
int llicti_encode_images_v(llicti_ctx *ctx, const uint8_t *d_rgb, const size_t *rgb_off, int B, const int *Hs, const int *Ws, int mode,
                           void *d_workspace, size_t workspace_bytes,
                           uint8_t *d_out, size_t out_stride, int32_t *d_seg_len, void *stream);
/* ... with a container mode PER IMAGE (host array of B modes): rANS containers of one lane kind whose STREAM COUNTS may differ -- every image's header
 * carries its own count.  What it is for: a stage of the decoder takes as long as its longest stream, and in a batch of mixed sizes that is a
 * stream of the largest image; with each image's count given by its own size (llicti_amd.codec.auto_modes) the streams are about equally long,
 * and every image stays inside its own byte budget (a 768x768 image affords 20 xwide v4 streams, a 321x481 one 6).  Image b's bytes are those of
 * llicti_encode_images(B = 1) on it in modes[b]. */
int llicti_encode_images_vm(llicti_ctx *ctx, const uint8_t *d_rgb, const size_t *rgb_off, int B, const int *Hs, const int *Ws, const int *modes,
                            void *d_workspace, size_t workspace_bytes,
                            uint8_t *d_out, size_t out_stride, int32_t *d_seg_len, void *stream);
int llicti_decode_images_vm(llicti_ctx *ctx, const uint8_t *d_in, size_t in_stride, const int32_t *d_seg_len,
                            int B, const int *Hs, const int *Ws, const int *modes, void *d_workspace, size_t workspace_bytes,
                            uint8_t *d_rgb, const size_t *rgb_off, void *stream);
/* Hs[b] x Ws[b] must be the size container b's header describes (llicti_header_dims); a mismatch flags that image (llicti_image_status). */
int llicti_decode_images_v(llicti_ctx *ctx, const uint8_t *d_in, size_t in_stride, const int32_t *d_seg_len,
                           int B, const int *Hs, const int *Ws, int mode, void *d_workspace, size_t workspace_bytes,
                           uint8_t *d_rgb, const size_t *rgb_off, void *stream);

/* REDUCED-RESOLUTION decode: image b at 1 / 2^reduce of its size -- Hr = ceil(Hs[b] / 2^reduce), Wr = ceil(Ws[b] / 2^reduce)
 * (llicti_reduced_dims) -- EXACTLY the pixels full[:, ::2^reduce, ::2^reduce] of the full decode, which are the original image's (the codec is
 * lossless).  It is a DECIMATION, not a low-pass: the lazy wavelet has no smoothing filter, so fine texture aliases.  The decoder works coarse to
 * fine and a level never reads a finer one, so the call launches the stages of levels >= reduce only: 3 x (nlevels - reduce) band-CNN launches
 * (level 0 alone holds 3/4 of the symbols and CNN positions), none at reduce = nlevels, where the output is the header's raw DC band.
 * reduce = 0 is llicti_decode_images_vm / _v: same launches, bytes and status words.  0 <= reduce <= the model's levels (5 config A, 2 config B),
 * LLICTI_EINVAL otherwise; one value for the call (llicti_decode_images_reduced_rv below takes one per image).
 *   Hs, Ws   the FULL sizes the headers describe; modes: one mode (n_modes = 1) or one per image (n_modes = B), as for llicti_decode_images_vm;
 *            every container the full decoder reads (the reference format: equal sizes per call)
 *   d_rgb    image b's uint8 [3][Hr][Wr] at d_rgb + rgb_off[b]; rgb_off = NULL: the reduced images tightly packed in call order
 *   workspace  what llicti_workspace_bytes* gives for the full decode of the same batch (a reduced call uses the same layout)
 * INTEGRITY: a rANS container's end-of-stream check belongs to the tail coder of the LAST stage (level 0, band x10: it must end in its start
 * state), which a call with reduce >= 1 never launches.  Such a call reports what the kernels it did launch flag -- header, unpack, init and
 * the decoded stages (llicti_check_status, llicti_image_status) -- and nothing else: damage confined to the skipped levels goes unnoticed.
 * A valid container gives status 0 for every image.  (What a FULL decode returned can be held against a digest of the encoded pixels:
 * PIXEL DIGESTS below.) */
int llicti_reduced_dims(int H, int W, int reduce, int *Hr, int *Wr);
int llicti_decode_images_reduced(llicti_ctx *ctx, const uint8_t *d_in, size_t in_stride, const int32_t *d_seg_len,
                                 int B, const int *Hs, const int *Ws, const int *modes, int n_modes, int reduce,
                                 void *d_workspace, size_t workspace_bytes, uint8_t *d_rgb, const size_t *rgb_off, void *stream);

/* INTERLEAVED, PITCHED 8-bit pixels: the layout image sources deliver (decoded PNG / JPEG, video frames, screen captures, OpenCV and PIL arrays).
 * The calls above take planar uint8 [3][H][W]; these two read and write the caller's interleaved buffer directly -- the lift is the first kernel
 * of an encode, the unlift the last of a decode, so no separate conversion pass runs.  A container's bytes are a function of the pixel VALUES
 * alone: the same image gives the same container through either layout.
 *   format    LLICTI_PIX_*: three colour bytes per pixel in the named order, the 4-byte formats with a fourth byte behind them.  ALPHA IS NOT
 *             CODED: the encoder ignores the fourth byte, the decoder writes 255 there.
 *   px_off    host array of B byte offsets into d_pix: the first byte of the first pixel of image b's window.  Pixel (i, j) of the window is
 *             at px_off[b] + i * pitch[b] + j * bpp, so a window may be a crop of a larger frame (offset of its corner, the frame's pitch).
 *             NULL = the windows back to back in call order, each of llicti_pixel_span bytes
 *   pitch     host array of B row pitches in bytes, >= W * bpp (LLICTI_EINVAL otherwise; at most 2^31 - 1).  NULL = tight rows, W * bpp
 * No alignment is required.  Windows whose first byte (d_pix + px_off[b]) and pitch are multiples of 4 are read and written in dwords, the
 * others byte by byte; the choice is per image, so one call may mix them.  The decoder writes the W * bpp bytes of each of the window's rows and
 * nothing else: pitch padding and whatever surrounds a crop keep their bytes.  Windows of one decode must not overlap.
 * An unknown format, a short pitch or a null array the call needs is LLICTI_EINVAL before anything is launched. */
#define LLICTI_PIX_RGB8 0
#define LLICTI_PIX_BGR8 1
#define LLICTI_PIX_RGBA8 2
#define LLICTI_PIX_BGRA8 3
/* Host helpers (no device needed): bytes per pixel of a format (0: unknown format), and the bytes from the first pixel of an H x W window
 * to the end of its last one, (H - 1) * pitch + W * bpp (pitch = 0: tight rows; 0: unknown format, H or W < 1, or pitch < W * bpp). */
int llicti_pixel_bytes(int format);
size_t llicti_pixel_span(int format, int H, int W, size_t pitch);
/* llicti_encode_images_vm on interleaved pixels: modes holds B modes; every container and rule of that call (the reference format codes equal
 * sizes per call).  Image b's container and segment lengths are those of the planar call on the same pixel values. */
int llicti_encode_images_px(llicti_ctx *ctx, const uint8_t *d_pix, int format, const size_t *px_off, const size_t *pitch,
                            int B, const int *Hs, const int *Ws, const int *modes, void *d_workspace, size_t workspace_bytes,
                            uint8_t *d_out, size_t out_stride, int32_t *d_seg_len, void *stream);
/* llicti_decode_images_reduced into interleaved pixels (reduce = 0: the full decode): Hs, Ws are the FULL sizes the headers describe; with
 * reduce >= 1 image b's window has the reduced size (llicti_reduced_dims).  Same launches, status words and integrity rule as that call. */
int llicti_decode_images_px(llicti_ctx *ctx, const uint8_t *d_in, size_t in_stride, const int32_t *d_seg_len,
                            int B, const int *Hs, const int *Ws, const int *modes, int n_modes, int reduce,
                            void *d_workspace, size_t workspace_bytes,
                            uint8_t *d_pix, int format, const size_t *px_off, const size_t *pitch, void *stream);

/* FLOAT TENSORS: decode straight into the dense, normalised, cropped batch tensor a network is fed with, and encode from planar float32 in
 * {k/255} (the reference's compress() input) -- the unlift is the last kernel of a decode, the lift the first of an encode, so no conversion,
 * crop, flip, normalise or stack pass runs around the call and a batch of MIXED sizes comes out as one uniform tensor.
 *   d_out     ONE dense planar tensor [B][3][Ho][Wo] of `dtype` (LLICTI_T_*), channels R, G, B; nothing outside
 *             [d_out, d_out + B * 3 * Ho * Wo * llicti_tensor_elem_bytes(dtype)) is written.  Stores are 4 elements wide when Wo % 4 == 0 and d_out
 *             is aligned to 4 elements, element by element otherwise
 *   y0, x0    host arrays of B window origins in the coordinates of the decoded image -- the REDUCED one for reduce >= 1 (llicti_reduced_dims:
 *             Hr x Wr); NULL = 0.  Image b's window must lie inside it: 0 <= y0[b], y0[b] + Ho <= Hr, 0 <= x0[b], x0[b] + Wo <= Wr
 *             (llicti_tensor_window_ok).  No padding, no resampling (llicti_decode_images_tensor_resized resamples)
 *   flip      host array of B flags, NULL = none: a set flag mirrors the window, output column j is window column Wo - 1 - j
 *   mean, std host arrays of 3 floats (R, G, B); both NULL = no normalisation
 * ARITHMETIC, to the operation (torchvision's ToTensor + Normalize on the CPU, bit for bit): x = (float)v / 255.0f, one IEEE fp32 division; with
 * mean and std y = (x - mean[c]) / std[c], one rounded fp32 subtraction and one correctly rounded fp32 division (no reciprocal, no contraction);
 * LLICTI_T_F16 / LLICTI_T_BF16 round that fp32 value to nearest even.
 * THE WINDOWS ARE PER CALL, NOT PER PLAN: origins and flips travel as kernel arguments, so the plan of the call is the one
 * llicti_decode_images_reduced builds for the same sizes, modes and reduce with tight placement -- a loop that draws new crops and flips for
 * every batch hits that one cached plan and neither synchronises the device nor allocates.  Same launches, status words and integrity rule as
 * llicti_decode_images_reduced; the tensor is written by the call's last kernel.
 * LLICTI_EINVAL before anything is launched, naming the image: an unknown dtype, Ho or Wo < 1, a window that leaves its image, exactly one of
 * mean / std NULL, a std that is zero, negative or not finite, a null pointer the call needs, and whatever llicti_decode_images_reduced refuses. */
#define LLICTI_T_F32 0
#define LLICTI_T_F16 1
#define LLICTI_T_BF16 2
/* Host helpers (no device needed): bytes per element of a dtype (0: unknown dtype), and whether an Ho x Wo window at (y0, x0) lies inside an
 * H x W image decoded at `reduce` (1 / 0; 0 for H, W, Ho or Wo < 1 or a reduce outside 0 .. LLICTI_NLEVELS). */
int llicti_tensor_elem_bytes(int dtype);
int llicti_tensor_window_ok(int H, int W, int reduce, int y0, int x0, int Ho, int Wo);
int llicti_decode_images_tensor(llicti_ctx *ctx, const uint8_t *d_in, size_t in_stride, const int32_t *d_seg_len,
                                int B, const int *Hs, const int *Ws, const int *modes, int n_modes, int reduce,
                                void *d_workspace, size_t workspace_bytes,
                                void *d_out, int dtype, int Ho, int Wo, const int *y0, const int *x0, const uint8_t *flip,
                                const float *mean, const float *std, void *stream);
/* RESIZED CROPS: llicti_decode_images_tensor with a resampling step in the decode's last kernel -- image b's source BOX (origin y0, x0, extent
 * hs x ws, in the coordinates of the decoded image: the REDUCED one for reduce >= 1, source pixel (y, x) being plane pixel (y << reduce, x << reduce))
 * is resampled to Ho x Wo, flipped, normalised and written as out[b][3][Ho][Wo]: torchvision's RandomResizedCrop + flip + ToTensor + Normalize
 * on a batch of MIXED sizes in one call.  Containers, modes, reduce, workspace, d_out, dtype, flip, mean, std, status words and the integrity rule
 * are llicti_decode_images_tensor's; the plan is the one llicti_decode_images_reduced builds for the same sizes, modes and reduce with tight
 * placement.  Boxes, flips, output size and the filter flag are KERNEL ARGUMENTS of the last kernel (two packed words per image, 128 images per
 * launch), no part of the plan or its key: a loader that draws new boxes for every batch neither allocates device memory, synchronises nor
 * builds a plan.  A reduced decode is a DECIMATION (every 2^reduce-th pixel, no low-pass): it aliases; the filter below works on what is decoded.
 *   y0, x0    host arrays of B box origins, NULL = 0
 *   hs, ws    host arrays of B box extents, NULL = the whole decoded image from the origin (Hr - y0[b], Wr - x0[b]; llicti_reduced_dims)
 *   Ho, Wo    1 .. 8160
 *   antialias 1: the triangle filter is widened by the scale when the box shrinks (PIL, torch antialias=True); then hs <= 4 Ho and ws <= 4 Wo
 *             (at most 9 taps per axis) -- a larger scale is LLICTI_EINVAL: raise reduce.  0: two taps per axis at every scale (plain bilinear)
 * ARITHMETIC, to the operation: every value fp32, every operation rounded once, no contraction.  Per axis, n the box extent, m the output
 * extent, i an output index:
 *   scale   = (float)n / (float)m
 *   support = (antialias && scale > 1) ? scale : 1
 *   inv     = 1 / support
 *   center  = scale * ((float)i + 0.5f)
 *   lo      = max(0, (int)((center - support) + 0.5f))            (the conversion truncates)
 *   hi      = min(n, (int)((center + support) + 0.5f))
 *   t_k     = max(0, 1 - |(((float)k - center) + 0.5f) * inv|)    k = lo .. hi - 1
 *   total   = t_lo + t_lo+1 + ...                                 (left to right, from +0)
 *   w_k     = t_k / total
 * A channel of output pixel (i, j): p = the 8-bit value after the inverse YCoCg-R, as float; for every row tap a, h_a = sum over the column
 * taps b of w^x_b * p[a][b] (left to right from +0, product then sum); v = sum over a of w^y_a * h_a (the same way); x = v / 255.0f; then
 * (x - mean[c]) / std[c] and the rounding to dtype as llicti_decode_images_tensor.  A flipped image is the unflipped result mirrored: output
 * column j holds the value of column Wo - 1 - j.  This is F.interpolate(mode="bilinear", align_corners=False, antialias=...) up to fp32
 * rounding (tests/test_resize_cpu.py bounds it); at n == m the weights are 1 and 0, so a box of Ho x Wo gives the BYTES of
 * llicti_decode_images_tensor for the same window.
 * LLICTI_EINVAL before anything is launched, naming the image: a box with hs or ws < 1, a box that leaves the decoded image, Ho or Wo outside
 * 1 .. 8160, antialias not 0 or 1, antialias = 1 with hs > 4 Ho or ws > 4 Wo, and everything llicti_decode_images_tensor refuses.
 * Host helpers (no device needed): llicti_resize_window_ok -- 1 if the call takes that box of an H x W image at `reduce` for that output size and
 * flag, else 0; llicti_resize_axis -- the taps of output index i (0 .. m - 1) of an axis: returns their count, writes the first source index to
 * *lo and the weights of taps lo, lo + 1, ... to w[0 .. cap - 1] (zeros behind the last tap; a count above cap is cut, the weights stay those
 * of the full sum); 0 for n or m < 1 or i outside 0 .. m - 1.  It is compiled from the function the kernel calls. */
int llicti_resize_window_ok(int H, int W, int reduce, int y0, int x0, int hs, int ws, int Ho, int Wo, int antialias);
int llicti_resize_axis(int n, int m, int antialias, int i, int *lo, float *w, int cap);
int llicti_decode_images_tensor_resized(llicti_ctx *ctx, const uint8_t *d_in, size_t in_stride, const int32_t *d_seg_len,
                                        int B, const int *Hs, const int *Ws, const int *modes, int n_modes, int reduce,
                                        void *d_workspace, size_t workspace_bytes,
                                        void *d_out, int dtype, int Ho, int Wo, const int *y0, const int *x0, const int *hs, const int *ws,
                                        const uint8_t *flip, const float *mean, const float *std, int antialias, void *stream);
/* VIEWS: several resized crops per image from ONE decode.  The batch is decoded once -- exactly the launches of llicti_decode_images_reduced for the
 * same sizes, modes and reduce, with its plan and its key -- and the last kernel then runs once per view: view v of group g is what
 * llicti_decode_images_tensor_resized writes for image image[v] with that box, flip, size, dtype and flag, to the bit (the ARITHMETIC paragraph
 * above is the one specification).  A GROUP is a set of views of one output size, dtype and flag, written to ONE dense [n][3][Ho][Wo] tensor;
 * two crop sizes are two groups of one call (multi-crop: 2 x 224 and 6 x 96 views per image).  The view launches of group 0, then group 1, ...
 * follow the decode on the same stream.  A group with image == NULL and n == B gives llicti_decode_images_tensor_resized's bytes.
 * The image index, box and flip of a view are KERNEL ARGUMENTS of the view launches (three packed words per view, 128 views per launch), no
 * part of the plan or its key: no device allocation, no upload and no synchronisation per call.  Status words are latched for every one of the
 * B images, those no view names included: llicti_check_status and llicti_image_status report what the resized call reports for the same
 * containers; the integrity rule is llicti_decode_images_reduced's.  mean, std: one pair for the call, as above.
 * Nothing is written outside a group's [d_out, d_out + n * 3 * Ho * Wo * elem).  The outputs of different groups MUST NOT OVERLAP, and none may
 * overlap the workspace; this is NOT checked.
 * LLICTI_EINVAL before anything is launched, naming the group and the view: G outside 1 .. LLICTI_VIEW_GROUPS_MAX, null groups or d_out, n outside
 * 1 .. 1,048,576, an image index outside 0 .. B - 1, image == NULL with n != B, and per view, against the view's own image, everything
 * llicti_decode_images_tensor_resized refuses. */
#define LLICTI_VIEW_GROUPS_MAX 16
typedef struct llicti_view_group {
    void *d_out;                  /* ONE dense [n][3][Ho][Wo] tensor of dtype */
    int dtype, Ho, Wo, antialias;
    int n;                        /* views of this group, 1 .. 1,048,576 */
    const int *image;             /* n image indices in 0 .. B-1: any order, repeats allowed, images may be absent.  NULL: view v is image v, then n == B */
    const int *y0, *x0, *hs, *ws; /* n each; NULL defaults as in llicti_decode_images_tensor_resized, taken against the view's image */
    const uint8_t *flip;          /* n flags, NULL = none */
} llicti_view_group;
int llicti_decode_images_tensor_views(llicti_ctx *ctx, const uint8_t *d_in, size_t in_stride, const int32_t *d_seg_len,
                                      int B, const int *Hs, const int *Ws, const int *modes, int n_modes, int reduce,
                                      void *d_workspace, size_t workspace_bytes,
                                      const llicti_view_group *groups, int G, const float *mean, const float *std, void *stream);
/* PER-IMAGE REDUCE: the five decodes above with `int reduce` replaced by `const int *reduces`, a host array of B values, 0 <= reduces[b] <= the
 * model's levels.  Image b is decoded EXACTLY as the scalar call at reduce = reduces[b] decodes it: its output size is
 * llicti_reduced_dims(Hs[b], Ws[b], reduces[b]), its window / box / views are in the coordinates of ITS OWN decimated grid, its status word and
 * the integrity rule are that call's (the end-of-stream check runs for exactly the images with reduces[b] == 0), and nothing of it depends on
 * its neighbours' values.  So one tight crop no longer sends a whole batch through level 0 (three quarters of the CNN work).
 *   schedule   level l runs for the images with reduces[b] <= l alone: the band CNN over the tile list of those images, the stage decoders with
 *              one workgroup per stream of those images, the tail coder for the level-0 images; the loop ends at min(reduces)
 *   placement  rgb_off / px_off NULL: the images tightly packed in call order, each at its own reduced size
 *   views      a view is held against the reduce of the image it names; an image no view names is still decoded to its reduces[b] -- pass the
 *              model's level count for it (its DC band only)
 *   workspace  what the scalar sibling takes for the same batch and modes
 *   plan       the batch's full-size plan (llicti_decode_images_vm's with tight placement): it does not depend on the values.  What does -- the
 *              r table, the output table or windows, the levels' stream and tile lists -- is built per call on the host, uploaded with one
 *              asynchronous copy on `stream` from a pooled block and never cached: calls with fresh values neither build a plan, allocate nor
 *              synchronise once the pool is warm
 *   all equal  the call IS its scalar sibling at that value (it delegates): same launches, plan key, counters, bytes
 * LLICTI_EINVAL before anything is launched, naming the image: reduces NULL, a value out of range, differing values with a reference-format
 * container in the call (its pipeline codes equal sizes and one schedule per call), and whatever the sibling refuses at that image's reduce. */
int llicti_decode_images_reduced_rv(llicti_ctx *ctx, const uint8_t *d_in, size_t in_stride, const int32_t *d_seg_len,
                                    int B, const int *Hs, const int *Ws, const int *modes, int n_modes, const int *reduces,
                                    void *d_workspace, size_t workspace_bytes, uint8_t *d_rgb, const size_t *rgb_off, void *stream);
int llicti_decode_images_px_rv(llicti_ctx *ctx, const uint8_t *d_in, size_t in_stride, const int32_t *d_seg_len,
                               int B, const int *Hs, const int *Ws, const int *modes, int n_modes, const int *reduces,
                               void *d_workspace, size_t workspace_bytes,
                               uint8_t *d_pix, int format, const size_t *px_off, const size_t *pitch, void *stream);
int llicti_decode_images_tensor_rv(llicti_ctx *ctx, const uint8_t *d_in, size_t in_stride, const int32_t *d_seg_len,
                                   int B, const int *Hs, const int *Ws, const int *modes, int n_modes, const int *reduces,
                                   void *d_workspace, size_t workspace_bytes,
                                   void *d_out, int dtype, int Ho, int Wo, const int *y0, const int *x0, const uint8_t *flip,
                                   const float *mean, const float *std, void *stream);
int llicti_decode_images_tensor_resized_rv(llicti_ctx *ctx, const uint8_t *d_in, size_t in_stride, const int32_t *d_seg_len,
                                           int B, const int *Hs, const int *Ws, const int *modes, int n_modes, const int *reduces,
                                           void *d_workspace, size_t workspace_bytes,
                                           void *d_out, int dtype, int Ho, int Wo, const int *y0, const int *x0, const int *hs, const int *ws,
                                           const uint8_t *flip, const float *mean, const float *std, int antialias, void *stream);
int llicti_decode_images_tensor_views_rv(llicti_ctx *ctx, const uint8_t *d_in, size_t in_stride, const int32_t *d_seg_len,
                                         int B, const int *Hs, const int *Ws, const int *modes, int n_modes, const int *reduces,
                                         void *d_workspace, size_t workspace_bytes,
                                         const llicti_view_group *groups, int G, const float *mean, const float *std, void *stream);
/* TENSOR OPTIONS: the three tensor decodes with a trailing `opts` -- the memory LAYOUT of the output and, for llicti_decode_images_tensor_o
 * alone, windows PADDED past their image.  `reduces` is the _rv contract above (B values; all equal is the scalar call).  opts == NULL, or
 * { LLICTI_LAYOUT_NCHW, LLICTI_PAD_NONE }, IS the _rv sibling (it delegates): same launches, plan key, counters, bytes and status words.
 * Nothing cached depends on opts: layout, pad mode, fill, origins and flips are kernel arguments of the decode's last kernel, so calls with
 * fresh values hit the plan the reduced decode builds for the same sizes, modes and reduce, and neither allocate nor synchronise.
 *   layout     LLICTI_LAYOUT_NCHW: [B][3][Ho][Wo] planes.  LLICTI_LAYOUT_NHWC: element (b, i, j, c) at ((b * Ho + i) * Wo + j) * 3 + c -- the
 *              memory of a [B, 3, Ho, Wo] tensor in torch.channels_last, strides (3 Ho Wo, 1, 3 Wo, 3).  The VALUES are the planar call's.  A
 *              lane's 4 pixels x 3 channels are 12 consecutive elements: 16-byte stores (16 + 8 for the 16-bit types) when Wo % 4 == 0 and d_out
 *              is 16-byte aligned, element by element otherwise -- the same bytes either way.  In the views call it holds for every group.
 *   pad_mode   llicti_decode_images_tensor_o only; the other two refuse anything but LLICTI_PAD_NONE (a box that leaves its image stays refused).
 * A PADDED WINDOW, to the operation.  Image b's decoded grid is Hr x Wr (llicti_reduced_dims at that image's reduce), extended in both axes by
 * the pad mode.  The Ho x Wo window at origin (y0, x0) -- either may be NEGATIVE -- is cut from the extended plane; a set flip then mirrors the
 * window: output column j is window column Wo - 1 - j.  Per axis (n the grid's extent), coordinate t in y0 .. y0 + Ho - 1 (x0 .. x0 + Wo - 1)
 * maps to a source index in 0 .. n - 1 or to "fill" (llicti_pad_index):
 *   0 <= t < n              t, under every mode
 *   LLICTI_PAD_CONSTANT     fill
 *   LLICTI_PAD_EDGE         0 for t < 0, n - 1 for t >= n                      (numpy 'edge', torch 'replicate')
 *   LLICTI_PAD_REFLECT      -t for t < 0, 2 (n - 1) - t for t >= n             (numpy / torch 'reflect', period 2 n - 2: the edge pixel is not
 *                           repeated); an overhang of more than n - 1 on a side is refused, as torch refuses it -- n == 1 with any overhang is
 *   LLICTI_PAD_SYMMETRIC    -t - 1 for t < 0, 2 n - 1 - t for t >= n           (numpy 'symmetric', period 2 n: the edge pixel is repeated); an
 *                           overhang of more than n on a side is refused
 * An output pixel whose row AND column map to source indices (sy, sx) is the 8-bit value behind the inverse YCoCg-R of decoded pixel (sy, sx)
 * through the ARITHMETIC of llicti_decode_images_tensor, unchanged.  One whose row or column maps to "fill" holds, in channel c:
 *   LLICTI_FILL_PIXEL       fill[c] taken as a value on the 0 .. 255 scale through that same arithmetic: (fill[c] / 255.0f - mean[c]) / std[c],
 *                           rounded to dtype -- torchvision's Pad(fill) + ToTensor + Normalize bit for bit for integer fills
 *   LLICTI_FILL_OUTPUT      fill[c] itself, rounded to dtype and nothing else (the "pad with 0 after normalising" collate)
 * LLICTI_PAD_CONSTANT and LLICTI_PAD_EDGE do not need the window to overlap the image.  With LLICTI_PAD_NONE the window must lie inside it, as
 * in llicti_decode_images_tensor; a window inside its image gives that call's bytes under every pad mode.
 * Nothing outside [d_out, d_out + B * 3 * Ho * Wo * elem) is written in either layout.
 * LLICTI_EINVAL before anything is launched, naming the image: an unknown layout, pad mode or fill space; a fill that is not finite; with a pad
 * mode, Ho or Wo outside 1 .. 8160, an origin outside -8160 .. 8160, LLICTI_PAD_REFLECT overhanging a side by more than n - 1,
 * LLICTI_PAD_SYMMETRIC by more than n; a pad mode in the resized or views call; and everything the _rv sibling refuses.
 * Host helpers (no device needed), compiled from the function the kernel calls: llicti_pad_index -- the source index of coordinate t on an axis
 * of n pixels under `mode` (LLICTI_PAD_NONE: inside or refused), -1 for "fill", -2 for refused (n outside 1 .. 8160, |t| above 2^20 and an unknown mode too);
 * llicti_tensor_window_pad_ok -- 1 if llicti_decode_images_tensor_o takes that window of an H x W image at `reduce` under `mode`, else 0. */
#define LLICTI_LAYOUT_NCHW 0
#define LLICTI_LAYOUT_NHWC 1
#define LLICTI_PAD_NONE 0
#define LLICTI_PAD_CONSTANT 1
#define LLICTI_PAD_EDGE 2
#define LLICTI_PAD_REFLECT 3
#define LLICTI_PAD_SYMMETRIC 4
#define LLICTI_FILL_PIXEL 0
#define LLICTI_FILL_OUTPUT 1
typedef struct llicti_tensor_opts { int layout, pad_mode, fill_space; float fill[3]; } llicti_tensor_opts;
int llicti_pad_index(int n, int t, int mode);
int llicti_tensor_window_pad_ok(int H, int W, int reduce, int y0, int x0, int Ho, int Wo, int mode);
int llicti_decode_images_tensor_o(llicti_ctx *ctx, const uint8_t *d_in, size_t in_stride, const int32_t *d_seg_len,
                                  int B, const int *Hs, const int *Ws, const int *modes, int n_modes, const int *reduces,
                                  void *d_workspace, size_t workspace_bytes,
                                  void *d_out, int dtype, int Ho, int Wo, const int *y0, const int *x0, const uint8_t *flip,
                                  const float *mean, const float *std, void *stream, const llicti_tensor_opts *opts);
int llicti_decode_images_tensor_resized_o(llicti_ctx *ctx, const uint8_t *d_in, size_t in_stride, const int32_t *d_seg_len,
                                          int B, const int *Hs, const int *Ws, const int *modes, int n_modes, const int *reduces,
                                          void *d_workspace, size_t workspace_bytes,
                                          void *d_out, int dtype, int Ho, int Wo, const int *y0, const int *x0, const int *hs, const int *ws,
                                          const uint8_t *flip, const float *mean, const float *std, int antialias, void *stream,
                                          const llicti_tensor_opts *opts);
int llicti_decode_images_tensor_views_o(llicti_ctx *ctx, const uint8_t *d_in, size_t in_stride, const int32_t *d_seg_len,
                                        int B, const int *Hs, const int *Ws, const int *modes, int n_modes, const int *reduces,
                                        void *d_workspace, size_t workspace_bytes,
                                        const llicti_view_group *groups, int G, const float *mean, const float *std, void *stream,
                                        const llicti_tensor_opts *opts);
/* llicti_encode_images_vm on planar float32: image b's [3][Hs[b]][Ws[b]] block at ELEMENT offset x_off[b] of d_x (NULL = the blocks back to back
 * in call order).  A sample x becomes the pixel value v = (int)rintf(x * 255.0f) -- one rounded fp32 product, rounded half to even
 * (torch.round) --, clamped to 0 .. 255, a NaN gives 0; containers and segment lengths are byte for byte those of the uint8 call on v, under
 * every rule of that call.  Loads are 4 floats wide when d_x, the offsets and the plane sizes allow.  float32 is the only input type (bfloat16
 * cannot hold k/255). */
int llicti_encode_images_f32(llicti_ctx *ctx, const float *d_x, const size_t *x_off, int B, const int *Hs, const int *Ws, const int *modes,
                             void *d_workspace, size_t workspace_bytes,
                             uint8_t *d_out, size_t out_stride, int32_t *d_seg_len, void *stream);

/* TRANSCODE: containers of one kind into containers of another, on the device, at the cost of ONE decode.  Image b's output container and its 49
 * segment lengths are byte for byte what llicti_encode_images_vm (B = 1) writes, in dst_modes[b], for the pixels container b decodes to -- without
 * the pixels ever being made: behind each (level, band) stage of the decoder the stage's CNN outputs and symbols become the encoder's
 * (c_low, c_high) pairs (one cdf_pairs launch), and the target's entropy coder runs on them.  3 x levels band-CNN launches instead of the
 * 6 x levels of a decode followed by an encode, neither an unlift nor a lift.
 *   src_modes  one mode (n_src = 1) or one per image (n_src = B), under llicti_decode_images_vm's rules: every container the decoder reads
 *              (llicti_header_mode names it); LLICTI_MODE_RANS_X_AUTO is not a source
 *   dst_modes  one mode (n_dst = 1) or one per image (n_dst = B), under llicti_encode_images_vm's rules, LLICTI_MODE_RANS_X_AUTO included
 *   d_out      image b's container at d_out + b * out_stride (out_stride as for llicti_encode_images_v), its segment lengths in d_seg_len_out[b];
 *              must not overlap d_in
 *   workspace  llicti_transcode_workspace_bytes of the same arguments (ctx = NULL: config A): the source call's layout, then the target's
 * LLICTI_EINVAL before anything is launched: an auto mode as a source, mixed lane kinds on either side, the reference format on either side with
 * images of different sizes, a null pointer, a size outside 32 .. 8160, an in_stride below the header bytes, overlapping buffers;
 * LLICTI_ENOSPACE: a workspace or out_stride that is too small.  llicti_transcode_workspace_bytes gives 0 for a refused combination.
 * Asynchronous on `stream`, no device synchronisation or allocation on a warm context.  STATUS as after a decode: what the decoder's kernels flag
 * (header, unpack, init, every stage, the rANS end-of-stream check) and the coder's LLICTI_ENOSPACE are latched by the call's last kernel
 * (llicti_check_status, llicti_image_status).  A flagged image does not disturb the others; its own row of d_seg_len_out is 49 zeros. */
size_t llicti_transcode_workspace_bytes(const llicti_ctx *ctx, int B, const int *Hs, const int *Ws,
                                        const int *src_modes, int n_src, const int *dst_modes, int n_dst);
int llicti_transcode_images(llicti_ctx *ctx, const uint8_t *d_in, size_t in_stride, const int32_t *d_seg_len_in,
                            int B, const int *Hs, const int *Ws, const int *src_modes, int n_src,
                            const int *dst_modes, int n_dst, void *d_workspace, size_t workspace_bytes,
                            uint8_t *d_out, size_t out_stride, int32_t *d_seg_len_out, void *stream);

/* RECORDS: the strided device containers of a batch <-> ONE dense blob of .llic records, on the device -- what an archive file holds and what
 * one dense PCIe copy moves.  A record is exactly the bytes of one .llic file (llicti_amd/fileio.py: dumps_llic): b"LLIC", a version byte (1), a
 * byte n -- the model's segment count, 4 + 9 x levels: 49 for config A, 22 for config B --, n little-endian uint32 segment lengths, then the n
 * segments back to back.  A device container is already its segments back to back, so a record's payload is the sum(seg_len) bytes at
 * d_cont + b * stride.  Both calls are asynchronous on `stream`, neither synchronises nor allocates on a warm context (the first call with a
 * larger B than any whole-batch call before grows the per-image status words, as a decode does), and both report through the latched status:
 * llicti_check_status, and llicti_image_status for the call's B images (a later decode replaces those words with its own).
 * LLICTI_EINVAL before anything is launched: a null pointer, B < 1 or above 1,048,576, stride < 1, a blob_cap / blob_bytes above 2^62, and a blob
 * that overlaps the containers, the segment lengths or the offsets.
 *
 * llicti_record_bytes (host helper, no device): bytes of the record of one image from its n segment lengths, 6 + 4n + sum; 0 for a null
 * h_seg_len or a negative length.  n is the context's; ctx = NULL: config A's 49.
 *
 * llicti_pack_records: d_rec_off[b] = first byte of record b in d_blob, d_rec_off[B] = their total (a scan on the device); the records densely
 * from d_blob: the blob equals the concatenation of the images' .llic files byte for byte.  No byte at or past d_rec_off[B] is written.
 *   - an image whose seg_len row has a negative entry or sums to more than `stride` gets a ZERO-LENGTH record and LLICTI_EFORMAT in its status
 *     word; its neighbours are unaffected
 *   - a total above blob_cap latches LLICTI_ENOSPACE: d_rec_off is still filled completely -- d_rec_off[B] is the capacity the call needs --, the
 *     records that end at or before blob_cap are written, the others are not: nothing at or past blob_cap is written
 *   d_seg_len [B][49] as the encoders write it; only the first n entries of a row are read.
 *
 * llicti_unpack_records: the inverse, for records at d_blob + d_rec_off[b] .. d_rec_off[b + 1] (any offsets: the blob may hold more than the
 * call's records, in any order).  Every record is VALIDATED ON THE DEVICE BEFORE A PAYLOAD BYTE IS READ: 0 <= off[b] <= off[b+1] <= blob_bytes,
 * length >= 6 + 4n, magic, version, n equal to the context's, every length below 2^31, 6 + 4n + sum == off[b+1] - off[b], sum <= stride.
 *   - a good record gives its n lengths and zeros up to 49 in d_seg_len[b], its payload at d_cont + b * stride
 *   - a record that fails gets LLICTI_EFORMAT for that image and an all-zero d_seg_len row; no byte of its container is written.  Every decode
 *     call refuses a zero row with the same flag, so a caller may decode straight behind the unpack and read the status once
 *   - no read leaves [d_blob, d_blob + blob_bytes), no write leaves [d_cont + b * stride, + stride)
 *   stride: any value that holds the call's largest payload -- it need not be llicti_max_container_bytes, the decoders only require the header
 *   bytes of every image inside it -- so a loader can stage a batch tightly.
 *
 * THE COPY: a payload is cut into chunks of LLICTI_RECORD_CHUNK bytes, one workgroup each (a 4K image's tens of megabytes go over hundreds of
 * compute units); source and destination are misaligned against each other by any number of bytes, and every chunk moves as aligned 16-byte
 * loads, a byte realign in registers and aligned 16-byte stores, with up to 15 bytes at either end byte by byte.  All offsets are 64-bit. */
#define LLICTI_RECORD_CHUNK 32768
size_t llicti_record_bytes(const llicti_ctx *ctx, const int32_t *h_seg_len);
size_t llicti_record_bytes_n(int n, const int32_t *h_seg_len);      /* the same for a segment count given outright (49 or 22, else 0): needs no context */
/* All device buffers of a record call are PAIRWISE DISJOINT -- d_blob (blob_cap / blob_bytes), d_cont (B * stride), d_seg_len, d_rec_off --:
 * any two that overlap are LLICTI_EINVAL before anything is launched, and llicti_last_error names both. */
int llicti_pack_records(llicti_ctx *ctx, const uint8_t *d_cont, size_t stride, const int32_t *d_seg_len, int B,
                        uint8_t *d_blob, size_t blob_cap, int64_t *d_rec_off /* [B+1] */, void *stream);
int llicti_unpack_records(llicti_ctx *ctx, const uint8_t *d_blob, size_t blob_bytes, const int64_t *d_rec_off /* [B+1] */, int B,
                          uint8_t *d_cont, size_t stride, int32_t *d_seg_len /* [B][49] */, void *stream);

/* PROGRESSIVE RECORDS: a second record layout beside .llic, a permutation of the same bytes, of which a decode at reduce = r needs one
 * contiguous PREFIX.  A rANS stream's bit region is read downwards from its end, coarse stages first, so a decode that stops after level r has
 * touched only the bytes from the main coder's cursor upwards (and the states above the region).  The streams of an image are cut at the
 * level boundaries and the pieces stored level-major, the coarsest level first.  xwide v4 containers only (LLICTI_MODE_RANS_X, fixed or
 * "auto" counts, both models): a stream of 64 / 128 lanes keeps its T field at its bottom.  The containers themselves do not change by a bit.
 *
 * CUTS.  L = the model's levels (5 / 2).  For stream m of an image, cur[m][l] = the main coder's bit cursor behind the last stage of level l;
 * c[m][l] = cur[m][l] >> 3 for l = 1 .. L-1, c[m][0] = 0, c[m][L] = len_m (the stream's bytes).  The level-l PIECE of stream m is its bytes
 * [c[m][l], c[m][l+1]): the cursors only move down, so the pieces tile the stream.  The level L-1 piece holds the states, the end marker and
 * the 9-bit field; the level-0 piece the tail coder's spill.
 *
 * THE RECORD (little-endian).  P = the container's payload, its n segments back to back, S bytes; stream m occupies P[off_m : off_m + len_m]
 * (M > 32: behind its segment's length table, as the decoder locates it).  The payload's bytes outside every stream are the FRAME bytes: the
 * header segments first, then the length tables.
 *   0        b"LLIP", u8 version = 1, u8 n (49 / 22), u8 L (5 / 2), u8 0, u16 M (1 .. 128), u16 0
 *   12       u32 seg_len[n]                                   the plain record's
 *   12+4n    per stream m: u32 off_m, u32 len_m, u32 c[m][1] .. c[m][L-1]                 (L + 1 words a stream)
 *   T        the frame bytes, in payload order (F = S - sum len_m of them)                T = 12 + 4n + 4 M (L + 1)
 *   T+F      the level L-1 pieces of streams 0 .. M-1, then level L-2, ..., then level 0
 * Prefix lengths: P_r = T + F + sum over l >= r and m of (c[m][l+1] - c[m][l]); P_L = T + F (the header alone: the DC band), P_0 = T + S (the
 * whole record).  The first P_r bytes hold everything a decode at reduce >= r reads.  A progressive record is a function of the plain record.
 *
 * llicti_level_cuts: the arguments of llicti_decode_images_vm with d_cuts -- int32 [B][128][LLICTI_NLEVELS], entry [b][m][l] = c[m][l] of image
 * b -- in place of the output pixels (and of their placement).  Rows m >= the image's stream count and entry l = 0 are zero.  A full decode
 * that writes no pixels: behind each level >= 1 one small kernel stores every stream's cursor; the tail coder runs, so the container's
 * end-of-stream check does: llicti_image_status is a full decode's.  Asynchronous on `stream`; no synchronisation and no allocation on a
 * warm context.  Modes that are not xwide v4 (64- / 128-lane streams, the reference format): LLICTI_EINVAL before anything is launched.
 *
 * llicti_pack_progressive: llicti_pack_records' contract (a scan on the device, then the copy) for progressive records: d_rec_off[b] = first
 * byte of record b, d_rec_off[B] = the total; d_prefix int64 [B][LLICTI_NLEVELS + 1]: P_0 .. P_L of every image (entries above L: 0).
 *   - an image whose lengths (a negative entry, a sum above `stride` or of 2^31 or more -- the table's words have 32 bits, and the unpack
 *     refuses one of 2^31 or more --, header segments other than 3 / 12 / 2), header (not an xwide v4
 *     container of the context's model), length tables (M = 64 / 128) or cuts (a row that does not ascend within len_m) do not hold together
 *     gets a ZERO-LENGTH record, an all-zero prefix row and LLICTI_EFORMAT; its neighbours are unaffected
 *   - a total above blob_cap latches LLICTI_ENOSPACE as llicti_pack_records does; nothing at or past blob_cap is written
 *
 * llicti_unpack_progressive: record b is the bytes d_blob + d_rec_off[b] .. d_rec_off[b + 1]: the prefix P_{reduce[b]} alone or anything
 * longer (reduce: HOST array of B ints).  EVERYTHING IS VALIDATED ON THE DEVICE BEFORE A FRAME OR PIECE BYTE IS READ: offsets inside the blob;
 * magic, version, n and L equal to the context's; the zero bytes; 1 <= M <= 128; every length below 2^31 and S <= stride; the streams ascending
 * and disjoint inside [0, S); 0 <= c[m][1] <= ... <= c[m][L-1] <= len_m; 0 <= reduce[b] <= L; at least P_{reduce[b]} bytes present.
 *   - a good record gives its seg_len row (zeros up to 49), and the frame bytes and the pieces of the levels >= reduce[b] at their payload
 *     positions in d_cont + b * stride; EVERY OTHER BYTE OF THE CONTAINER IS LEFT AS IT WAS
 *   - a refused record gets LLICTI_EFORMAT for its image, an all-zero seg_len row and an untouched container; its neighbours unpack
 *   - no read leaves the blob, no write leaves [d_cont + b * stride, + stride)
 *   - whether off_m / len_m agree with the container's own length tables is the decoder's check, as it is for a plain record
 *   - a decode finer than reduce[b] reads stream bytes nobody delivered: garbage or LLICTI_EFORMAT, memory-safe as for any corrupt container.
 *     The decoders parse the TOP of every stream whatever the reduce (rans_init_kernel: end marker and states), so at reduce[b] = L -- no
 *     stream byte delivered -- an image is flagged where the container's old bytes leave a zero on top of a bit region
 * Both calls are asynchronous on `stream` and neither allocates nor synchronises warm; the reduces travel as kernel arguments.  They report
 * through the latched status as the record calls do.  LLICTI_EINVAL before anything is launched: as for the record calls, and a null or
 * overlapping d_cuts / d_prefix.
 *
 * THE COPY of both calls: the record's dense side behind its table is cut into ranges of LLICTI_RECORD_CHUNK bytes, one workgroup each, so a
 * record of a few huge pieces and one of 640 tiny ones load the chip alike; a workgroup finds the pieces its range overlaps from the record's
 * own table and moves each overlap with 16-byte stores.  All offsets are 64-bit.
 *
 * llicti_progressive_prefix (host helper, no device): from the first `bytes` bytes of a record -- at least its table, T bytes -- the prefix
 * lengths prefix[0 .. LLICTI_NLEVELS] (entries above the record's L: 0); LLICTI_EFORMAT for a head that breaks one of the rules above (the
 * same code checks them on the device), whichever of the two models it names. */
int llicti_level_cuts(llicti_ctx *ctx, const uint8_t *d_in, size_t in_stride, const int32_t *d_seg_len,
                      int B, const int *Hs, const int *Ws, const int *modes, void *d_workspace, size_t workspace_bytes,
                      int32_t *d_cuts /* [B][128][LLICTI_NLEVELS] */, void *stream);
/* All device buffers of these two calls are PAIRWISE DISJOINT, as for the record calls above: d_blob, d_cont, d_seg_len, d_rec_off and, for
 * llicti_pack_progressive, d_cuts and d_prefix (so d_cuts may not overlap d_rec_off, the containers or the segment lengths either). */
int llicti_pack_progressive(llicti_ctx *ctx, const uint8_t *d_cont, size_t stride, const int32_t *d_seg_len, int B, const int32_t *d_cuts,
                            uint8_t *d_blob, size_t blob_cap, int64_t *d_rec_off /* [B+1] */, int64_t *d_prefix /* [B][LLICTI_NLEVELS+1] */, void *stream);
int llicti_unpack_progressive(llicti_ctx *ctx, const uint8_t *d_blob, size_t blob_bytes, const int64_t *d_rec_off /* [B+1] */, int B,
                              const int *reduce /* host, [B] */, uint8_t *d_cont, size_t stride, int32_t *d_seg_len /* [B][49] */, void *stream);
int llicti_progressive_prefix(const uint8_t *head, size_t bytes, int64_t *prefix /* [LLICTI_NLEVELS+1] */);

/* PIXEL DIGESTS: a CRC-32 of every image's pixels, computed on the device, so that a decode can be checked without moving a pixel to the host
 * and without the original at hand.
 *
 * DEFINITION.  The digest of an H x W image is zlib's CRC-32 of its pixels as planar uint8 [3][H][W] bytes -- the R plane, then the G plane, then
 * the B plane, rows top to bottom: zlib.crc32(rgb_chw.tobytes()) in Python, crc32(0, p, 3 H W) in C.  Anyone recomputes it without this
 * library.  It depends on the pixel VALUES alone: not on the container kind, the batch, or the form a decode delivers them in.
 *
 * WHERE IT COMES FROM.  Every whole-batch encode and every full decode leaves the image's int16 YCoCg-R planes in the caller's workspace
 * (llicti_workspace_planes); the digest kernels read those planes once, invert the transform and write a word per image.  A decode into
 * interleaved pixels, a float crop, a resized box or views therefore yields the digest of the WHOLE image it decoded, although that image
 * never exists as bytes.  An image decoded at reduce >= 1 has no full-size planes: it has no digest (d_have = 0).
 *
 * THE FOLD.  CRCs concatenate: crc(A || B) = crc(A) * x^(8 |B|) xor crc(B) in GF(2)[x] modulo the reflected polynomial 0xEDB88320.  A lane
 * takes a run of llicti_crc32_geometry's lane_pixels pixels, a workgroup group_pixels, three CRCs at a time (pixel p is byte p of each
 * colour plane); lanes, then workgroups, then the three planes are folded in order with that rule.  The ragged end of an image lies in FRONT
 * of its first workgroup (a zero register does not see what is missing in front of a message), so a plane of n pixels has its seams at
 * n - k * lane_pixels and n - k * group_pixels.
 *
 * WHAT IT SHOWS.  Equal digests: the decode returned the pixels that were encoded, up to a 2^-32 chance per image -- through the entropy
 * decoder, the CNN's fp32 arithmetic on this device, driver and compiler, and the inverse transform.  It is a CHECK AGAINST ACCIDENTS, NOT A
 * MAC: whoever can alter a container can alter a stored digest, and CRC-32 collisions are easy to construct.
 *
 * llicti_crc32_combine (host, no context): crc32(A || B) from crc32(A), crc32(B) and len_b = |B| -- zlib's crc32_combine.
 * llicti_crc32_geometry (host, no context): the kernel's run per lane and per workgroup, in pixels (either pointer may be NULL).
 * llicti_crc32_planes: d_crc[b] = the digest of image b of d_planes, int16 [B][3][H][W] as llicti_lift_u8 writes them; 1 <= H, W <= 8160.
 *   Asynchronous on `stream`.
 * llicti_digest_images: the digests of the images of the PRECEDING whole-batch encode or decode of this batch, out of that call's workspace,
 *   which is read and never written.  B, Hs, Ws, modes / n_modes: that call's (an encode's "auto" modes as they were given).  reduce: NULL, or
 *   the B values the decode ran with (a scalar call: B copies).  d_have[b] = 1 and d_crc[b] = the digest where image b was coded in full --
 *   reduce NULL or reduce[b] == 0, and every encode --; d_have[b] = 0 and d_crc[b] = 0 otherwise, and no pixel of such an image is read.
 *   The call runs on the CACHED plan of that call -- the most recently used one of these sizes and modes -- and builds none: a batch no plan
 *   is cached for is LLICTI_EINVAL, and so is a workspace smaller than that plan's, a null pointer, a size outside 32 .. 8160 and a reduce
 *   outside 0 .. the model's levels.  Asynchronous on `stream`; no allocation and no synchronisation (the flags of a call with reduced
 *   images travel in a pooled table block, as the _rv decodes' tables do); neither the status words nor llicti_last_timing are touched.
 *   llicti_level_cuts is a full decode: its planes are digested like any other's.  A TRANSCODE's workspace is out of scope: its two plans
 *   share one workspace under a layout of their own. */
uint32_t llicti_crc32_combine(uint32_t crc_a, uint32_t crc_b, uint64_t len_b);
int llicti_crc32_geometry(int *lane_pixels, int *group_pixels);
int llicti_crc32_planes(llicti_ctx *ctx, const int16_t *d_planes, int B, int H, int W, uint32_t *d_crc, void *stream);
int llicti_digest_images(llicti_ctx *ctx, int B, const int *Hs, const int *Ws, const int *modes, int n_modes, const int *reduce /* NULL or [B] */,
                         const void *d_workspace, size_t workspace_bytes, uint32_t *d_crc, int32_t *d_have, void *stream);

/* Where llicti_encode_images / llicti_decode_images of B images of H x W in `mode` keep the YCoCg-R planes inside the caller's workspace
 * (byte offsets): int16 [B][3][H][W] (Y - 127, Co, Cg) and float32 [B][3][H][W] = planes / 255 -- the second is the `x_ycocg` the
 * reference's compress() returns beside the streams (LLICTI_nets.py:143-144, :159), so a caller that wants it reads it from the workspace
 * behind the encode instead of lifting the image a second time.  Valid until the next whole-batch call on that workspace. */
int llicti_workspace_planes(llicti_ctx *ctx, int B, int H, int W, int mode, size_t *off_planes, size_t *off_fplanes);
/* Where a whole-batch call on B images of Hs[b] x Ws[b] in modes[b] (llicti_encode_images_vm / llicti_decode_images_vm; the same placement as the
 * _v entry points with one mode) leaves the CNN outputs of its LAST launch -- level 0, band x10 -- of image `image`: byte offset of its
 * float32 [64][npos] block (channel planes, LLICTI_PARAM_STRIDE; position (i, j) of the h x w band grid at i * w + j) inside the caller's
 * workspace, and npos = h * w.  What it is for: holding the mixed-size form of the band CNN (tile lists, per-image geometry, the odd-edge
 * staging path) against the reference's own get_params outputs on a full-size odd shape (tests: ..._ragged_vs_reference).  Valid until the
 * next whole-batch call on that workspace. */
int llicti_workspace_params_v(llicti_ctx *ctx, int B, const int *Hs, const int *Ws, const int *modes, int image, size_t *off_params, long *npos);

/* Synchronises `stream` and returns the latched device-side status of the calls issued since the
 * last check (LLICTI_OK, LLICTI_EFORMAT, LLICTI_ENOSPACE). */
int llicti_check_status(llicti_ctx *ctx, void *stream);

/* Per-image status of the last llicti_decode_images call: h_status[b] = LLICTI_OK or LLICTI_EFORMAT for image b (a batch with one
 * malformed container decodes the others correctly; the bad image's pixels are deterministic garbage).  Synchronises `stream`.
 * The words are latched into the context at the end of the decode: the workspace may be freed or reused before this call. */
int llicti_image_status(llicti_ctx *ctx, int32_t *h_status, int n, void *stream);

/* Host-side self-test of arithmetic helpers that have no device dependency (the magic division of the stage geometry). */
int llicti_selftest(void);

/* Image size from a container's first 17 header bytes (host memory). */
int llicti_header_dims(const uint8_t *h_hdr17, int *H, int *W);
/* The mode a container's first 17 header bytes name -- LLICTI_MODE_AC or LLICTI_MODE_RANS*(count) -- i.e. what to hand to llicti_decode_images*
 * (LLICTI_EFORMAT for a header this build does not read: the retired v2 and xwide-v3 layouts). */
int llicti_header_mode(const uint8_t *h_hdr17, int *mode);

/* Device-resident timing of the last llicti_encode_images / llicti_decode_images call, measured with
 * HIP events on `stream`: ms[0] = whole call, ms[1] = sum of the band-CNN kernel launches,
 * n_launch = number of band-CNN launches.  Used by bench.py for the roofline figure. */
int llicti_last_timing(llicti_ctx *ctx, float ms[4], int *n_launch);
/* Where the last whole-batch call spent its device time (profiling on): summed event durations per kernel group --
 * cat_ms[LLICTI_PROF_CNN] band-CNN launches, [RANS_STAGE] rans_decode_stage_kernel, [RANS_TAIL] rans_tail_kernel,
 * [PAIRS] cdf_pairs_kernel, [RANS_ENC] rans_encode + pack, [AC] the range-coder / table kernels of the reference-format
 * container, [MISC] lift / unlift / header / unpack / init -- and the duration of every band-CNN launch in launch order
 * (scale 4..0 x band 0..2; up to cnn_cap entries, their number in *n_cnn).  Synchronises like llicti_last_timing. */
#define LLICTI_NPROF 7
#define LLICTI_PROF_CNN 0
#define LLICTI_PROF_RANS_STAGE 1
#define LLICTI_PROF_RANS_TAIL 2
#define LLICTI_PROF_PAIRS 3
#define LLICTI_PROF_RANS_ENC 4
#define LLICTI_PROF_AC 5
#define LLICTI_PROF_MISC 6
int llicti_last_timing_detail(llicti_ctx *ctx, float cat_ms[LLICTI_NPROF], float *cnn_launch_ms, int cnn_cap, int *n_cnn);
/* ... and the band-CNN time of that call per level (a level's launches may be split into sub-batches: their count is not fixed). */
int llicti_last_cnn_level_ms(llicti_ctx *ctx, float level_ms[LLICTI_NLEVELS]);
/* Tuning switches that never change a result.  "cnn_tile_rows" (0 = per launch, 16, 4): force the band CNN's 16-row throughput tiles
 * or its 4-row latency tiles (default: 4 rows whenever the 16-row tiles could not give every compute unit a workgroup).
 * "ac_anchor_min_batch" (default 96): from this many images per call on,
 * llicti_decode_images decodes the AC container over anchor rows (every 8th table entry from cdf_anchor_kernel, the 8
 * entries of the located bucket evaluated by the decoding wavefront) instead of full table rows; values above the
 * default are clamped to it (the workspace is sized for the default).  "force_ragged" (default 0; 1: a batch of equal sizes takes the
 * code path of a mixed-size batch too -- per-image tables, tile lists -- so that tests can run every case through both).
 * "enc_side_levels" (default 0; 1: llicti_encode_images runs levels 4..1 on an internal stream next to level 0's launches and joins it
 * before the entropy coder: -0.3 % of a step on MI355X, at the price of kernel traces whose side-queue durations include waiting). */
int llicti_set_tuning(llicti_ctx *ctx, const char *key, int value);
/* What the whole-batch calls have cost the host / device since llicti_create: "device_syncs" (hipDeviceSynchronize inside a whole-batch call),
 * "device_allocs" (hipMalloc inside one), "plan_builds" / "plan_hits" (calls whose (mode, sizes) were new / cached), "block_waits" (a new plan
 * had to wait for the last user of a pooled table block), "plans_cached", "blocks_pooled".  A warm context coding batch after batch of ever new
 * image sizes adds to plan_builds only (tests/test_hip_parity.py::test_many_sizes_no_device_sync_and_plan_reuse). */
int llicti_get_counter(llicti_ctx *ctx, const char *name, long *value);
/* enable / disable the per-kernel event timing above (off by default: it adds event records). */
int llicti_set_profiling(llicti_ctx *ctx, int enable);

#ifdef __cplusplus
}
#endif
#endif

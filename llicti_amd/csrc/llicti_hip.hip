// llicti_hip.hip -- gfx950 (MI355X / CDNA4) kernels and the C-ABI of include/llicti_hip.h.
// One translation unit: the kernels live in the *.hpp files included below (common, lift, likelihood, band_cnn,
// cdf, ac_coder, rans_coder, rans_tail, rans_encode, container); this file holds the context, the workspace plan and the entry points.
//
// Kernels (reference call sites in include/llicti_hip.h):
//   lift_kernel / unlift_kernel       integer YCoCg-R lift, min/max, float planes          (HBM bound)
//   lift_px_kernel / unlift_px_kernel the same on the caller's interleaved, pitched pixels (RGB8 / BGR8 / RGBA8 / BGRA8) (HBM bound)
//   lift_kernel<float> / unlift_tensor_kernel  planar float32 in, the dense float / half / bfloat16 batch tensor (crop, flip, normalise) out (HBM bound)
//   unlift_resize_tensor_kernel       the same tensor from a per-image source box RESAMPLED to the output size (triangle filter; a gather)
//   unlift_views_tensor_kernel        the same tile per VIEW: several boxes per image, each naming its image, from one decode
//   sink_window_kernel                unlift_tensor_kernel's window PADDED past its image (constant, edge, reflect, symmetric) and / or stored NHWC
//   sink_resize_nhwc_kernel, sink_views_nhwc_kernel   the two resampling kernels storing NHWC (torch.channels_last)
//   band_params_kernel<BAND>          interpolator CNN: 3 chained fp32-MFMA GEMMs per pixel tile,
//                                     weights of one 88-channel head resident in LDS        (MFMA bound)
//   cdf_pairs_kernel                  encoder: the two table entries per symbol (10 erfc)   (VALU)
//   cdf_table_kernel                  decoder: full Lp-entry uint16 rows                    (HBM / VALU bound)
//   ac_encode_*_kernel                torchac-algorithm range encoder, one lane per stream  (latency bound)
//   ac_decode_kernel                  matching decoder, one wavefront per stream            (latency bound)
//   rans_encode_kernel<Q>             rANS v3 encoder: 64 Q lanes per stream, one wavefront per 64 (latency bound)
//   rans_decode_stage_*_kernel        rANS v3 stage decoders, table-free: four / two / ONE lane per symbol for streams of 64 / 128 / 256
//                                     lanes (the timed mode: rans_decode_stage_lane_kernel<4>)    (VALU issue bound)
//   rans_tail_kernel<Q>               the serial tail coder behind the lanes' initial states: a coder wavefront and its preparing
//                                     wavefronts per chain (rans_tail.hpp)                        (latency bound)
//   header / pack / unpack kernels    container assembly in HBM
//   record_* kernels                  strided containers <-> one dense blob of .llic records: validation + a realigning 16-byte copy (HBM bound)
//   level_cuts / prog_* kernels       progressive records: the level cuts of a decode, validation + a piecewise copy in level-major order (HBM bound)
//   crc_planes_kernel / crc_fold_kernel   pixel digests: CRC-32 of every image's RGB bytes from the planes in the workspace (HBM / VALU bound)
//
// No CPU path exists in this library: every entry point needs a gfx950 device.
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <map>
#include <memory>
#include <optional>
#include <string>
#include <tuple>
#include <type_traits>
#include <utility>
#include <vector>

#include "../../include/llicti_hip.h"
#include "numerics.hpp"

using namespace llicti;

#include "common.hpp"
#include "lift.hpp"
#include "likelihood.hpp"
#include "band_cnn.hpp"
#include "cdf.hpp"
#include "ac_coder.hpp"
#include "rans_coder.hpp"
#include "rans_tail.hpp"
#include "rans_encode.hpp"
#include "container.hpp"
#include "records.hpp"
#include "records_progressive.hpp"
#include "digest.hpp"
#include "host_plan.hpp"

// ------------------------------------------------------------------------------------------------ context
constexpr int kMaxSub = 3;
constexpr int kMaxPlans = 32;         // plans the context keeps (least recently used goes first)
// Device + pinned host memory of one plan's tables.  Blocks are POOLED and never freed before llicti_destroy: a plan that leaves the cache
// hands its block back, the next new plan takes any block whose last user has finished (hipEventQuery on `done`, recorded behind every call
// that uses the block) -- so that a data set of many image sizes (the reference's own test set has 119 among 500 images) never makes the
// library synchronise the device or call hipFree (which does) once it is warm.
struct PlanBlock {
    uint8_t *dev = nullptr, *host = nullptr;
    size_t cap = 0;
    hipEvent_t done = nullptr;        // behind the last call that used the block
    hipEvent_t uploaded = nullptr;    // behind the table upload ...
    hipStream_t up_stream = nullptr;  // ... on this stream: a call on another stream waits for it
    bool used = false;                // `done` has been recorded at least once
    hipStream_t done_stream = nullptr;      // ... last on this stream: a call on ANOTHER stream waits for `done` before it re-records it, so that the one
                                            // event always lies behind every user of the block (a plan used on stream A, then on B, then evicted
                                            // was recycled as soon as B's record completed, while A's kernels could still be reading the tables)
};
struct PlanDev {
    Plan p;
    PlanBlock blk;
    uint64_t last_use = 0;
    template <class T> const T *dev(size_t off) const { return reinterpret_cast<const T *>(blk.dev + off); }
};

// profiling spans (llicti_set_profiling): what a pair of events brackets
enum ProfCat { PROF_CNN = 0, PROF_RANS_STAGE, PROF_RANS_TAIL, PROF_PAIRS, PROF_RANS_ENC, PROF_AC, PROF_MISC, PROF_NCAT };
static_assert(PROF_NCAT == LLICTI_NPROF, "include/llicti_hip.h: LLICTI_NPROF");

struct llicti_ctx {
    int device = 0;
    int head = kHead, nlev = LLICTI_NLEVELS;     // model shape (llicti_set_model): config A unless set
    float *d_pack[3] = { nullptr, nullptr, nullptr };
    size_t pack_floats_n[3] = { 0, 0, 0 };       // floats d_pack[band] holds
    bool have[3] = { false, false, false };
    std::map<std::vector<long>, struct PlanDev *> plans;   // Plan::key -> plan + its device tables (at most kMaxPlans, least recently used out first)
    std::vector<PlanBlock> pool;      // table blocks of plans that left the cache, for the next new plan
    uint64_t use_clock = 0;
    int force_ragged = 0;             // llicti_set_tuning("force_ragged"): equal-size batches take the mixed-size code path too (tests)
    // what the whole-batch calls did to the host / device since llicti_create (llicti_get_counter): a steady stream of calls over many image
    // sizes must add nothing to the first two
    long n_device_sync = 0, n_device_alloc = 0, n_plan_build = 0, n_plan_hit = 0, n_block_wait = 0;
    hipStream_t sub[kMaxSub] = { nullptr, nullptr, nullptr };    // internal streams of the AC decode pipeline ([0] unused: the caller's)
    hipEvent_t ev_ac[2][16] = {};      // AC decode pipeline: chunk c of Y / Co done
    hipEvent_t ev_ac_band = nullptr, ev_ac_end[2] = { nullptr, nullptr };
    int ac_anchor_min_batch = kAcAnchorBatch;
    int32_t *d_img_status = nullptr;  // per-image status words of the last llicti_decode_images call, latched from its workspace
    int img_status_cap = 0, img_status_n = 0;   // (context-owned: the caller may free or reuse the workspace before llicti_image_status)
    int32_t *d_status = nullptr;      // small persistent status word (for the kernel-level entry points)
    int32_t *d_lift_part = nullptr;   // min/max partials of llicti_lift_u8 (1 MB; calls on one context are not concurrent)
    uint32_t *d_crc_tab = nullptr;    // pixel digests: the shift constants (crc_math.hpp: crc_fill_tables) ...
    uint32_t *d_crc_part = nullptr;   // ... and the workgroups' partial CRCs, kCrcMaxParts x 3 words (digest.hpp)
    float2 *d_phi_lut = nullptr;      // normal CDF on [-6, 6] as (value, difference to the next) pairs: the lane decoder's hint table (rans_coder.hpp)
    int n_cu = 256;                   // compute units of the device (grid sizing of the persistent kernels)
    int cnn_tile_rows = 0;            // llicti_set_tuning("cnn_tile_rows"): 0 = choose per launch, 16 / 4 = force (tests, A/B)
    int enc_side_levels = 0;          // llicti_set_tuning("enc_side_levels"): 1 = encoder levels 4..1 on a side stream next to level 0, 0 = one queue (default)
    hipEvent_t ev_enc[2] = { nullptr, nullptr };
    bool profiling = false;
    std::vector<hipEvent_t> ev;       // event pool of the profiling spans
    struct Span { hipEvent_t e0, e1; int cat, tag; };
    std::vector<Span> spans;          // spans of the current call: (start, end) events, category, level of a PROF_CNN span (-1 otherwise)
    hipEvent_t last_ev = nullptr;     // the last event recorded by a span (or the call's opening event) ...
    hipStream_t last_ev_stream = nullptr;      // ... and the stream it was recorded on: a span that follows on the same stream starts from it
    float last_cnn_level_ms[LLICTI_NLEVELS] = {};
    int ev_used = 0;                  // events of the pool in use
    hipEvent_t ev_call[2] = { nullptr, nullptr };
    float last_ms[4] = { 0, 0, 0, 0 };
    float last_cat_ms[PROF_NCAT] = {};
    std::vector<float> last_cnn_ms;   // per band-CNN launch, launch order
    int last_launches = 0;
    bool timing_pending = false;
};

// One profiling span: events on `s` before and after the launches it brackets (no-op unless profiling is on).
// A failed event call only loses the measurement.
struct ProfSpan {
    // Spans on one stream are CHAINED: a span starts from the event that closed the previous one (one event per span, not two), so the
    // spans tile the call's time on that stream and a kernel's span holds its dispatch latency instead of a bubble made by the
    // measurement (start and end events around every launch read 5-7 % above rocprofv3's kernel durations; chained: ~1 %).
    llicti_ctx *c;
    hipStream_t s;
    hipEvent_t e1 = nullptr;
    static hipEvent_t pool_get(llicti_ctx *c)
    {
        if (c->ev_used == (int)c->ev.size()) {
            hipEvent_t e = nullptr;
            if (hipEventCreate(&e) != hipSuccess) return nullptr;
            c->ev.push_back(e);
        }
        return c->ev[c->ev_used++];
    }
    ProfSpan(llicti_ctx *c_, int cat, hipStream_t s_, int tag = -1) : c(c_), s(s_)
    {
        if (!c->profiling) return;
        hipEvent_t e0 = (c->last_ev && c->last_ev_stream == s) ? c->last_ev : nullptr;
        if (!e0) {
            e0 = pool_get(c);
            if (!e0 || hipEventRecord(e0, s) != hipSuccess) return;
        }
        hipEvent_t e = pool_get(c);
        if (!e) return;
        c->spans.push_back(llicti_ctx::Span{ e0, e, cat, tag });
        e1 = e;
    }
    ~ProfSpan()
    {
        if (!e1) return;
        if (hipEventRecord(e1, s) == hipSuccess) { c->last_ev = e1; c->last_ev_stream = s; }
        else c->spans.pop_back();
    }
    ProfSpan(const ProfSpan &) = delete;
    ProfSpan &operator=(const ProfSpan &) = delete;
};

// Every entry point that touches the device runs under this guard: the context's device becomes current for the
// call and the caller's current device is restored on return (a HipCodec on cuda:N used while the thread's current
// device is another one must not launch there, and must not leave the thread's device changed).
struct DeviceGuard {
    int prev = -1, dev = -1;
    explicit DeviceGuard(const llicti_ctx *c) {
        if (!c) return;
        dev = c->device;
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != dev) (void)hipSetDevice(dev);
    }
    ~DeviceGuard() { if (prev >= 0 && prev != dev) (void)hipSetDevice(prev); }
    DeviceGuard(const DeviceGuard &) = delete;
    DeviceGuard &operator=(const DeviceGuard &) = delete;
};

// what the context builds a batch's plan from (host_plan.hpp: PlanSpec)
static PlanSpec ctx_spec(const llicti_ctx *c, int B, const int *Hs, const int *Ws, const size_t *rgb_off, int ME, const int *Ms)
{
    return PlanSpec{ B, Hs, Ws, ME, Ms, c->nlev, c->force_ragged != 0, rgb_off, c->n_cu, c->cnn_tile_rows };
}

extern "C" size_t llicti_workspace_bytes_v(int B, const int *Hs, const int *Ws, int mode) { return plan_workspace_bytes_v(B, Hs, Ws, mode); }
extern "C" size_t llicti_workspace_bytes_vm(int B, const int *Hs, const int *Ws, const int *modes) { return plan_workspace_bytes_vm(B, Hs, Ws, modes, B); }
extern "C" size_t llicti_workspace_bytes(int B, int H, int W, int mode) { return plan_workspace_bytes(B, H, W, mode); }
extern "C" size_t llicti_max_container_bytes(int H, int W) { return plan_max_container_bytes(H, W); }
extern "C" size_t llicti_workspace_bytes_ctx(const llicti_ctx *c, int B, const int *Hs, const int *Ws, const int *modes, int n_modes)
{
    return c ? plan_workspace_bytes_vm(B, Hs, Ws, modes, n_modes, c->nlev) : 0;
}
extern "C" size_t llicti_max_container_bytes_ctx(const llicti_ctx *c, int H, int W) { return c ? plan_max_container_bytes(H, W, c->nlev) : 0; }
extern "C" int llicti_header_dims(const uint8_t *h, int *H, int *W) { return plan_header_dims(h, H, W); }
extern "C" int llicti_header_mode(const uint8_t *h, int *mode)
{
    if (!h || !mode) return fail(LLICTI_EINVAL, "header_mode: null pointer");
    int H = 0, W = 0;
    if (int rc = plan_header_dims(h, &H, &W)) return rc;          // (rejects what this build does not read, with the reason)
    if (h[0] == LLICTI_NLEVELS || h[0] == kLevelsB) { *mode = 0; return LLICTI_OK; }
    const int v = header_streams(h[0], (int)(uint16_t)(h[15] | (h[16] << 8)));
    *mode = ((v >> 8) == 2 ? 0x500 : (v >> 8) == 1 ? 0x300 : 0x100) | (v & 0xFF);
    return LLICTI_OK;
}

// The 18 forms of the band CNN -- 3 bands x tile rows 16 / 4 / 8 x equal / mixed sizes, in the order of launch_band_params' `form` index -- each as
// config A's kernel (88-wide heads) and config B's (60-wide heads): one signature, one grid, one tile list.
typedef void (*BandParamsFn)(const float *, Geom, const float *, float *, int, int, int, const Geom *, const TileRef *);
struct CnnForm { BandParamsFn fn[2]; int band, TH; };      // fn[0]: 88-wide, fn[1]: 60-wide
#define LLICTI_CNN_ROW(TH_, RAG) \
    { { band_params_kernel<0, TH_, RAG>, band_params_h60_kernel<0, TH_, RAG> }, 0, TH_ }, { { band_params_kernel<1, TH_, RAG>, band_params_h60_kernel<1, TH_, RAG> }, 1, TH_ }, \
    { { band_params_kernel<2, TH_, RAG>, band_params_h60_kernel<2, TH_, RAG> }, 2, TH_ }
static const CnnForm kCnnForms[18] = { LLICTI_CNN_ROW(kTileHMax, false), LLICTI_CNN_ROW(kTileHSmall, false), LLICTI_CNN_ROW(kTileHMid, false),
                                       LLICTI_CNN_ROW(kTileHMax, true),  LLICTI_CNN_ROW(kTileHSmall, true),  LLICTI_CNN_ROW(kTileHMid, true) };
#undef LLICTI_CNN_ROW

extern "C" int llicti_create(llicti_ctx **out, int device)
{
    if (!out) return fail(LLICTI_EINVAL, "create: null ctx pointer");
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return fail(LLICTI_ENODEVICE, "no HIP device: this library has no CPU path");
    if (device < 0 || device >= n) return fail(LLICTI_EINVAL, "create: device %d out of range (%d devices)", device, n);
    hipDeviceProp_t prop;
    HIPCHK(hipGetDeviceProperties(&prop, device));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) return fail(LLICTI_ENODEVICE, "device %d is %s; this library is built for gfx950 only", device, prop.gcnArchName);
    llicti_ctx *c = new llicti_ctx();
    c->device = device;
    c->n_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    DeviceGuard guard(c);
    HIPCHK(hipMalloc(&c->d_status, 64));
    HIPCHK(hipMalloc(&c->d_lift_part, (size_t)kLiftMaxParts * 4 * sizeof(int32_t)));
    HIPCHK(hipMemset(c->d_status, 0, 64));
    {
        std::vector<float2> lut(kPhiLutN);
        for (int j = 0; j < kPhiLutN; ++j) {
            const double z0 = -kPhiLutZ + j * (2.0 * kPhiLutZ / kPhiLutN), z1 = -kPhiLutZ + (j + 1) * (2.0 * kPhiLutZ / kPhiLutN);
            const double v0 = 0.5 * std::erfc(-z0 * 0.70710678118654752440), v1 = 0.5 * std::erfc(-z1 * 0.70710678118654752440);
            lut[j] = make_float2((float)v0, (float)(v1 - v0));
        }
        HIPCHK(hipMalloc(&c->d_phi_lut, sizeof(float2) * kPhiLutN));
        HIPCHK(hipMemcpy(c->d_phi_lut, lut.data(), sizeof(float2) * kPhiLutN, hipMemcpyHostToDevice));
    }
    {
        std::vector<uint32_t> tab(kCrcTabWords);
        crc_fill_tables(tab.data());
        HIPCHK(hipMalloc(&c->d_crc_tab, sizeof(uint32_t) * kCrcTabWords));
        HIPCHK(hipMemcpy(c->d_crc_tab, tab.data(), sizeof(uint32_t) * kCrcTabWords, hipMemcpyHostToDevice));
        HIPCHK(hipMalloc(&c->d_crc_part, (size_t)kCrcMaxParts * 3 * sizeof(uint32_t)));
        HIPCHK(hipFuncSetAttribute((const void *)crc_planes_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kCrcLdsBytes));
    }
    HIPCHK(hipEventCreate(&c->ev_call[0]));
    HIPCHK(hipEventCreate(&c->ev_call[1]));
    for (int k = 0; k < 2; ++k) {
        for (int i = 0; i < 16; ++i) HIPCHK(hipEventCreateWithFlags(&c->ev_ac[k][i], hipEventDisableTiming));
        HIPCHK(hipEventCreateWithFlags(&c->ev_ac_end[k], hipEventDisableTiming));
    }
    HIPCHK(hipEventCreateWithFlags(&c->ev_ac_band, hipEventDisableTiming));
    for (int k = 0; k < 2; ++k) HIPCHK(hipEventCreateWithFlags(&c->ev_enc[k], hipEventDisableTiming));
    for (int i = 1; i < kMaxSub; ++i) HIPCHK(hipStreamCreateWithFlags(&c->sub[i], hipStreamNonBlocking));
    // the band CNN stages a whole head (up to 86 KB) in LDS
    for (const CnnForm &f : kCnnForms) {
        HIPCHK(hipFuncSetAttribute((const void *)f.fn[0], hipFuncAttributeMaxDynamicSharedMemorySize, cnn_lds_bytes(f.band, f.TH)));
        HIPCHK(hipFuncSetAttribute((const void *)f.fn[1], hipFuncAttributeMaxDynamicSharedMemorySize, cnn_lds_bytes(f.band, f.TH, kHeadB)));
    }
    *out = c;
    return LLICTI_OK;
}

extern "C" int llicti_destroy(llicti_ctx *c)
{
    if (!c) return LLICTI_OK;
    {
    DeviceGuard guard(c);
    (void)hipDeviceSynchronize();
    for (int b = 0; b < 3; ++b) if (c->d_pack[b]) hipFree(c->d_pack[b]);
    for (auto &kv : c->plans) { c->pool.push_back(kv.second->blk); delete kv.second; }
    c->plans.clear();
    for (PlanBlock &bk : c->pool) {
        if (bk.dev) (void)hipFree(bk.dev);
        if (bk.host) (void)hipHostFree(bk.host);
        if (bk.done) (void)hipEventDestroy(bk.done);
        if (bk.uploaded) (void)hipEventDestroy(bk.uploaded);
    }
    c->pool.clear();
    for (int i = 0; i < kMaxSub; ++i) {
        if (c->sub[i]) hipStreamDestroy(c->sub[i]);
    }
    for (int k = 0; k < 2; ++k) {
        for (int i = 0; i < 16; ++i) if (c->ev_ac[k][i]) hipEventDestroy(c->ev_ac[k][i]);
        if (c->ev_ac_end[k]) hipEventDestroy(c->ev_ac_end[k]);
    }
    if (c->ev_ac_band) hipEventDestroy(c->ev_ac_band);
    for (int k = 0; k < 2; ++k) if (c->ev_enc[k]) hipEventDestroy(c->ev_enc[k]);
    if (c->d_status) hipFree(c->d_status);
    if (c->d_lift_part) hipFree(c->d_lift_part);
    if (c->d_phi_lut) hipFree(c->d_phi_lut);
    if (c->d_crc_tab) hipFree(c->d_crc_tab);
    if (c->d_crc_part) hipFree(c->d_crc_part);
    if (c->d_img_status) hipFree(c->d_img_status);
    for (auto e : c->ev) hipEventDestroy(e);
    for (int i = 0; i < 2; ++i) if (c->ev_call[i]) hipEventDestroy(c->ev_call[i]);
    }
    delete c;
    return LLICTI_OK;
}

extern "C" int llicti_set_band_weights(llicti_ctx *c, int band, int K0, const float *w0, const float *b0,
                                       const float *w1, const float *b1, const float *w2, const float *b2)
{
    if (!c || band < 0 || band > 2 || !w0 || !b0 || !w1 || !b1 || !w2 || !b2) return fail(LLICTI_EINVAL, "set_band_weights: bad argument");
    static const int K0s[3] = { 48, 72, 120 };
    if (K0 != K0s[band]) return fail(LLICTI_EINVAL, "set_band_weights: band %d needs K0=%d, got %d", band, K0s[band], K0);
    std::vector<float> pk;
    pack_band(K0, c->head, w0, b0, w1, b1, w2, b2, pk);          // (the arrays are the context's model's: llicti_set_model)
    DeviceGuard guard(c);
    // blocking by contract (include/llicti_hip.h): work in flight on any stream may still read the old weights
    HIPCHK(hipDeviceSynchronize());
    if (c->d_pack[band] && c->pack_floats_n[band] != pk.size()) { HIPCHK(hipFree(c->d_pack[band])); c->d_pack[band] = nullptr; }
    if (!c->d_pack[band]) HIPCHK(hipMalloc(&c->d_pack[band], pk.size() * sizeof(float)));
    c->pack_floats_n[band] = pk.size();
    HIPCHK(hipMemcpy(c->d_pack[band], pk.data(), pk.size() * sizeof(float), hipMemcpyHostToDevice));
    c->have[band] = true;
    return LLICTI_OK;
}

// every cached plan back to the block pool (no device work: the blocks wait there for their last users)
static void drop_plans(llicti_ctx *c)
{
    for (auto &kv : c->plans) { c->pool.push_back(kv.second->blk); delete kv.second; }
    c->plans.clear();
}

extern "C" int llicti_set_model(llicti_ctx *c, int head, int nlevels)
{
    if (!c) return fail(LLICTI_EINVAL, "set_model: null ctx");
    if (!((head == kHead && nlevels == LLICTI_NLEVELS) || (head == kHeadB && nlevels == kLevelsB)))
        return fail(LLICTI_EINVAL, "set_model: (head %d, %d levels) -- this build runs config A (88, 5) and config B (60, 2)", head, nlevels);
    if (head == c->head && nlevels == c->nlev) return LLICTI_OK;
    c->head = head;
    c->nlev = nlevels;
    for (int b = 0; b < 3; ++b) c->have[b] = false;      // the weights of the other shape no longer apply (the buffers are reused or replaced)
    drop_plans(c);                                       // (a plan is built for the model's levels)
    return LLICTI_OK;
}

extern "C" int llicti_set_tuning(llicti_ctx *c, const char *key, int value)
{
    if (!c || !key) return fail(LLICTI_EINVAL, "set_tuning: null argument");
    if (!strcmp(key, "ac_anchor_min_batch")) {
        if (value < 1) return fail(LLICTI_EINVAL, "set_tuning: ac_anchor_min_batch must be >= 1");
        c->ac_anchor_min_batch = value;
        return LLICTI_OK;
    }
    if (!strcmp(key, "cnn_tile_rows")) {
        if (value != 0 && value != kTileHMax && value != kTileHMid && value != kTileHSmall && value != -1)
            return fail(LLICTI_EINVAL, "set_tuning: cnn_tile_rows must be 0 (automatic), %d, %d or %d (-1: round 3's rule, 16 or 4)", kTileHMax, kTileHMid, kTileHSmall);
        if (c->cnn_tile_rows != value) drop_plans(c);       // (a mixed-size plan holds the tile lists of the forms chosen when it was built)
        c->cnn_tile_rows = value;
        return LLICTI_OK;
    }
    if (!strcmp(key, "enc_side_levels")) {
        if (value < 0 || value > 1) return fail(LLICTI_EINVAL, "set_tuning: enc_side_levels must be 0 or 1");
        c->enc_side_levels = value;
        return LLICTI_OK;
    }
    if (!strcmp(key, "force_ragged")) {
        if (value < 0 || value > 1) return fail(LLICTI_EINVAL, "set_tuning: force_ragged must be 0 or 1");
        c->force_ragged = value;
        return LLICTI_OK;
    }
    return fail(LLICTI_EINVAL, "set_tuning: unknown key '%s'", key);
}

extern "C" int llicti_workspace_planes(llicti_ctx *c, int B, int H, int W, int mode, size_t *off_planes, size_t *off_fplanes)
{
    if (!c || !off_planes || !off_fplanes) return fail(LLICTI_EINVAL, "workspace_planes: null argument");
    if (check_dims(B, H, W)) return LLICTI_EINVAL;
    const int ME = mode_streams(mode);
    if (ME < 0) return fail(LLICTI_EINVAL, "workspace_planes: unknown mode 0x%x", mode);
    std::vector<int> Hs(B, H), Ws(B, W);
    Plan p;
    build_plan(p, ctx_spec(c, B, Hs.data(), Ws.data(), nullptr, ME, nullptr));
    if (!p.uniform && B > 1) return fail(LLICTI_EINVAL, "workspace_planes: with the tuning switch force_ragged the images of a batch are not tightly packed");
    *off_planes = p.off_planes;
    *off_fplanes = p.off_fplanes;
    return LLICTI_OK;
}

extern "C" int llicti_get_counter(llicti_ctx *c, const char *name, long *value)
{
    if (!c || !name || !value) return fail(LLICTI_EINVAL, "get_counter: null argument");
    if (!strcmp(name, "device_syncs")) *value = c->n_device_sync;
    else if (!strcmp(name, "device_allocs")) *value = c->n_device_alloc;
    else if (!strcmp(name, "plan_builds")) *value = c->n_plan_build;
    else if (!strcmp(name, "plan_hits")) *value = c->n_plan_hit;
    else if (!strcmp(name, "block_waits")) *value = c->n_block_wait;
    else if (!strcmp(name, "plans_cached")) *value = (long)c->plans.size();
    else if (!strcmp(name, "blocks_pooled")) *value = (long)c->pool.size();
    else return fail(LLICTI_EINVAL, "get_counter: unknown counter '%s'", name);
    return LLICTI_OK;
}

extern "C" int llicti_set_profiling(llicti_ctx *c, int enable)
{
    if (!c) return fail(LLICTI_EINVAL, "null ctx");
    c->profiling = enable != 0;
    return LLICTI_OK;
}

// ------------------------------------------------------------------------------------------------ launches
// The grid of a lift launch over B images of at most `units` work items (pixels, or 4-pixel pieces): gx workgroups per image, so many that the
// B * gx partial min/max entries fit the scratch
static int lift_grid(long units, int B, int *gx)
{
    *gx = (int)std::max<long>(1, std::min<long>(std::min<long>((units + 255) / 256, std::max(8, 4096 / B)), kLiftMaxParts / B));
    if ((long)B * *gx > kLiftMaxParts) return fail(LLICTI_EINVAL, "lift: batch of %d images exceeds the partials scratch", B);
    return 0;
}

// where an encode's pixels come from: planar uint8, the caller's interleaved pixels (llicti_encode_images_px), planar float32 in {k/255}
// (llicti_encode_images_f32)
enum class PixelSrc { PlanarU8, Interleaved, PlanarF32 };

// One lift: the grid, the kernel of the source's kind, the fold of the partial min / max values, the check.
// part: scratch of kLiftMaxParts x 4 int32 (the workspace's for the whole-batch calls, the context's for llicti_lift_u8).
// units: H * W (with a table: of the batch's largest image -- it sizes the grid); Interleaved: the largest window in 4-pixel row pieces
// (Plan::pix_units), pv the windows.  vec_ok: every image's plane size and placement (in ELEMENTS of the source) allow 4-pixel accesses.
static int launch_lift(PixelSrc kind, const void *d_src, int B, long units, bool vec_ok, int16_t *planes, float *fplanes, int32_t *mm, int32_t *part,
                       hipStream_t s, int32_t *zero = nullptr, int n_zero = 0, const ImgGeo *iv = nullptr, const PixGeo *pv = nullptr)
{
    const bool vec = kind != PixelSrc::Interleaved && vec_ok && (units % 4 == 0) && (((uintptr_t)d_src | (uintptr_t)planes | (uintptr_t)fplanes) % 16 == 0);
    int gx;
    if (int rc = lift_grid(vec ? units / 4 : units, B, &gx)) return rc;
    const dim3 grid(gx, B);
    const uint8_t *u8 = (const uint8_t *)d_src;
    const float *f32 = (const float *)d_src;
    if (kind == PixelSrc::Interleaved) lift_px_kernel<<<grid, 256, 0, s>>>(u8, planes, fplanes, part, zero, n_zero, iv, pv);
    else if (kind == PixelSrc::PlanarF32 && vec) lift_kernel<float, 4><<<grid, 256, 0, s>>>(f32, units, planes, fplanes, part, zero, n_zero, iv);
    else if (kind == PixelSrc::PlanarF32) lift_kernel<float, 1><<<grid, 256, 0, s>>>(f32, units, planes, fplanes, part, zero, n_zero, iv);
    else if (vec) lift_kernel<uint8_t, 4><<<grid, 256, 0, s>>>(u8, units, planes, fplanes, part, zero, n_zero, iv);
    else lift_kernel<uint8_t, 1><<<grid, 256, 0, s>>>(u8, units, planes, fplanes, part, zero, n_zero, iv);
    minmax_reduce_kernel<<<B, 64, 0, s>>>(part, gx, mm);
    HIPCHK(hipGetLastError());
    return 0;
}

// One band-CNN launch.  Equal sizes (tiles == nullptr): B images of g's size, tile -> image by division; mixed sizes: the plan's tile list of
// this (level, band) and its per-image geometry table, form and grid chosen when the plan was built.
static int launch_band_params(llicti_ctx *c, const float *fplanes, const Geom &g, int band, float *params, hipStream_t s,
                              const Geom *gv = nullptr, const TileRef *tiles = nullptr, const TileRun *run = nullptr)
{
    if (!c->have[band]) return fail(LLICTI_ENOWEIGHTS, "band %d weights not set", band);
    const int tiles_x = (g.w + kTileW - 1) / kTileW;
    int TH, gx;
    long n_tiles_l;
    if (tiles) { TH = run->TH; gx = run->gx; n_tiles_l = run->n_tiles; }
    else {
        const TileForm f = choose_tile_form(c->n_cu, c->cnn_tile_rows, band, [&](int th) { return (long)g.B * tiles_x * ((g.h + th - 1) / th); });
        TH = f.TH; gx = f.gx; n_tiles_l = f.n_tiles;
    }
    const int tiles_y = (g.h + TH - 1) / TH;
    if (n_tiles_l > 0x7FFFFFFFL || n_tiles_l < 1) return fail(LLICTI_EINVAL, "band_params: bad tile count");
    const int n_tiles = (int)n_tiles_l;
    const int lds_bytes = cnn_lds_bytes(band, TH, c->head);
    const int form = band + (TH == kTileHSmall ? 3 : TH == kTileHMid ? 6 : 0) + (tiles ? 9 : 0);
    const CnnForm &f = kCnnForms[form];
    // (a row of the table that is not this launch's would run a kernel against another band's weight pack: refused here, on the host)
    if (f.band != band || f.TH != TH) return fail(LLICTI_EINVAL, "band_params: form %d of the table is band %d with %d tile rows, the launch band %d with %d", form, f.band, f.TH, band, TH);
    ProfSpan span(c, PROF_CNN, s, g.lvl);
    f.fn[c->head == kHeadB ? 1 : 0]<<<dim3((unsigned)gx, 4), 64 * TH, lds_bytes, s>>>(fplanes, g, c->d_pack[band], params, tiles_x, tiles_y, n_tiles, gv, tiles);
    HIPCHK(hipGetLastError());
    return 0;
}

extern "C" int llicti_lift_u8(llicti_ctx *c, const uint8_t *d_rgb, int B, int H, int W, int16_t *d_planes,
                              float *d_fplanes, int32_t *d_minmax, void *stream)
{
    if (!c || !d_rgb || !d_planes || !d_fplanes || !d_minmax) return fail(LLICTI_EINVAL, "lift: null pointer");
    DeviceGuard guard(c);
    if (check_dims(B, H, W)) return LLICTI_EINVAL;
    return launch_lift(PixelSrc::PlanarU8, d_rgb, B, (long)H * W, true, d_planes, d_fplanes, d_minmax, c->d_lift_part, (hipStream_t)stream);
}

extern "C" int llicti_unlift_u8(llicti_ctx *c, const int16_t *d_planes, int B, int H, int W, uint8_t *d_rgb, void *stream)
{
    if (!c || !d_planes || !d_rgb) return fail(LLICTI_EINVAL, "unlift: null pointer");
    DeviceGuard guard(c);
    if (check_dims(B, H, W)) return LLICTI_EINVAL;
    const long plane = (long)H * W;
    const int gx = (int)std::min<long>((plane + 255) / 256, 1024);
    unlift_kernel<<<dim3(gx, B), 256, 0, (hipStream_t)stream>>>(d_planes, plane, d_rgb, nullptr, 0, nullptr, nullptr, nullptr);
    HIPCHK(hipGetLastError());
    return LLICTI_OK;
}

extern "C" int llicti_band_params_f32(llicti_ctx *c, const float *d_fplanes, int B, int H, int W, int lvl, int band,
                                      float *d_params, void *stream)
{
    if (!c || !d_fplanes || !d_params) return fail(LLICTI_EINVAL, "band_params: null pointer");
    DeviceGuard guard(c);
    if (check_dims(B, H, W)) return LLICTI_EINVAL;
    if (lvl < 0 || lvl >= c->nlev || band < 0 || band > 2) return fail(LLICTI_EINVAL, "band_params: bad level/band (the model has %d levels)", c->nlev);
    Geom g = make_geom(B, H, W, lvl);
    return launch_band_params(c, d_fplanes, g, band, d_params, (hipStream_t)stream);
}

extern "C" int llicti_lift_train_f32(llicti_ctx *c, const uint8_t *d_rgb, int B, int H, int W, float *d_fplanes, void *stream)
{
    if (!c || !d_rgb || !d_fplanes) return fail(LLICTI_EINVAL, "lift_train: null pointer");
    DeviceGuard guard(c);
    if (check_dims(B, H, W)) return LLICTI_EINVAL;
    const long plane = (long)H * W;
    const int gx = (int)std::min<long>((plane + 255) / 256, 2048);
    lift_train_kernel<<<dim3(gx, B), 256, 0, (hipStream_t)stream>>>(d_rgb, plane, d_fplanes);
    HIPCHK(hipGetLastError());
    return LLICTI_OK;
}

extern "C" int llicti_selfinfo_f32(llicti_ctx *c, const float *d_fplanes, const float *d_params, int B, int H, int W,
                                   int lvl, int band, float *d_bits, void *stream)
{
    if (!c || !d_fplanes || !d_params || !d_bits) return fail(LLICTI_EINVAL, "selfinfo: null pointer");
    DeviceGuard guard(c);
    if (check_dims(B, H, W)) return LLICTI_EINVAL;
    if (lvl < 0 || lvl >= c->nlev || band < 0 || band > 2) return fail(LLICTI_EINVAL, "selfinfo: bad level/band (the model has %d levels)", c->nlev);
    Geom g = make_geom(B, H, W, lvl);
    StageGeom sg = make_stage(g, band);
    SelfGeom s;
    s.B = B; s.H = H; s.W = W; s.lvl = lvl; s.h = g.h; s.w = g.w; s.oi = sg.oi; s.oj = sg.oj; s.Hl = g.Hl; s.Wl = g.Wl; s.plane = g.plane;
    const long n = (long)g.h * g.w;
    selfinfo_kernel<<<dim3((unsigned)((n + 255) / 256), B), 256, 0, (hipStream_t)stream>>>(d_fplanes, d_params, s, d_bits);
    HIPCHK(hipGetLastError());
    return LLICTI_OK;
}

// kernel-level entry point: B images of one size, pairs [clr][B][n]
static int launch_cdf_pairs(const int16_t *planes, const float *params, const int32_t *mm, const Geom &g, int band,
                            uint32_t *pairs, hipStream_t s)
{
    StageGeom sg = make_stage(g, band);
    sg.pair_cs = (long)g.B * sg.hc * sg.wc;
    const long np = (long)sg.h * sg.w;                    // the kernel walks the band grid (rows of CNN outputs are contiguous there)
    cdf_pairs_kernel<<<dim3((unsigned)((np + kPairsThreads - 1) / kPairsThreads), g.B), kPairsThreads, 0, s>>>(planes, params, mm, sg, nullptr, pairs);
    HIPCHK(hipGetLastError());
    return 0;
}
static int launch_cdf_anchors(const int16_t *planes, const float *params, const int32_t *mm, const Geom &g, int band, int clr,
                              uint8_t *rows, long n0, long cnt, long cap_rows, hipStream_t s)
{
    StageGeom sg = make_stage(g, band);
    const long want = (cnt + kTabWaves - 1) / kTabWaves;
    const long cap = std::max<long>(1, (256L * 8 * 2) / std::max(1, g.B));
    cdf_anchor_kernel<<<dim3((unsigned)std::max<long>(1, std::min(want, cap)), g.B), 64 * kTabWaves, 0, s>>>(planes, params, mm, sg, clr, rows,
                                                                                                   (int)n0, (int)cnt, (int)cap_rows);
    HIPCHK(hipGetLastError());
    return 0;
}
static int launch_cdf_table(const int16_t *planes, const float *params, const int32_t *mm, const Geom &g, int band, int clr,
                            uint16_t *tables, int row_stride, long n0, long cnt, long cap_rows, hipStream_t s)
{
    StageGeom sg = make_stage(g, band);
    const long want = (cnt + kTabWaves - 1) / kTabWaves;                    // one row per wave ...
    const long cap = std::max<long>(1, (256L * 8 * 2) / std::max(1, g.B));   // ... up to ~16 waves per SIMD-quad in flight per image set
    cdf_table_kernel<<<dim3((unsigned)std::max<long>(1, std::min(want, cap)), g.B), 64 * kTabWaves, 0, s>>>(planes, params, mm, sg, clr, tables, row_stride,
                                                                                                  (int)n0, (int)cnt, (int)cap_rows);
    HIPCHK(hipGetLastError());
    return 0;
}

extern "C" int llicti_cdf_u16(llicti_ctx *c, const int16_t *d_planes, const float *d_params, const int32_t *d_minmax,
                              int B, int H, int W, int lvl, int band, int clr, uint16_t *d_tables, int row_stride, void *stream)
{
    if (!c || !d_planes || !d_params || !d_minmax || !d_tables) return fail(LLICTI_EINVAL, "cdf_u16: null pointer");
    DeviceGuard guard(c);
    if (check_dims(B, H, W)) return LLICTI_EINVAL;
    if (lvl < 0 || lvl >= c->nlev || band < 0 || band > 2 || clr < 0 || clr > 2) return fail(LLICTI_EINVAL, "cdf_u16: bad level/band/clr");
    if (row_stride < 8 || row_stride > 512 || (row_stride & 7)) return fail(LLICTI_EINVAL, "cdf_u16: row_stride must be a multiple of 8 in [8,512]");
    Geom g = make_geom(B, H, W, lvl);
    int hc, wc;
    coded_dims(g, band, &hc, &wc);
    const long nc = (long)hc * wc;
    return launch_cdf_table(d_planes, d_params, d_minmax, g, band, clr, d_tables, row_stride, 0, nc, nc, (hipStream_t)stream);
}

extern "C" int llicti_cdf_pairs_u32(llicti_ctx *c, const int16_t *d_planes, const float *d_params, const int32_t *d_minmax,
                                    int B, int H, int W, int lvl, int band, uint32_t *d_pairs, void *stream)
{
    if (!c || !d_planes || !d_params || !d_minmax || !d_pairs) return fail(LLICTI_EINVAL, "cdf_pairs: null pointer");
    DeviceGuard guard(c);
    if (check_dims(B, H, W)) return LLICTI_EINVAL;
    if (lvl < 0 || lvl >= c->nlev || band < 0 || band > 2) return fail(LLICTI_EINVAL, "cdf_pairs: bad level/band");
    Geom g = make_geom(B, H, W, lvl);
    return launch_cdf_pairs(d_planes, d_params, d_minmax, g, band, d_pairs, (hipStream_t)stream);
}

extern "C" int llicti_ac_encode_u16cdf(llicti_ctx *c, const uint16_t *d_cdf, int Lp, int row_stride, const int16_t *d_sym,
                                       int n_streams, long N, uint8_t *d_out, long out_stride, int32_t *d_len, void *stream)
{
    if (!c || !d_cdf || !d_sym || !d_out || !d_len) return fail(LLICTI_EINVAL, "ac_encode: null pointer");
    DeviceGuard guard(c);
    if (Lp < 2 || Lp > 65536 || row_stride < Lp || n_streams < 1 || N < 1 || out_stride < 8 || (out_stride & 3) || ((uintptr_t)d_out & 3))
        return fail(LLICTI_EINVAL, "ac_encode: bad argument (out_stride and d_out must be multiples of 4)");
    ac_encode_tables_kernel<<<(n_streams + 63) / 64, 64, 0, (hipStream_t)stream>>>(d_cdf, Lp, row_stride, d_sym, n_streams, N, d_out,
                                                                                  out_stride, d_len, c->d_status);
    HIPCHK(hipGetLastError());
    return LLICTI_OK;
}

extern "C" int llicti_ac_decode_u16cdf(llicti_ctx *c, const uint16_t *d_cdf, int Lp, int row_stride, const uint8_t *d_in,
                                       long in_stride, const int32_t *d_len, int n_streams, long N, int16_t *d_sym, void *stream)
{
    if (!c || !d_cdf || !d_in || !d_len || !d_sym) return fail(LLICTI_EINVAL, "ac_decode: null pointer");
    DeviceGuard guard(c);
    if (Lp < 2 || Lp > 512 || row_stride < Lp || row_stride > 512 || (row_stride & 7) || n_streams < 1 || N < 1 || (in_stride & 3) ||
        ((uintptr_t)d_in & 3) || ((uintptr_t)d_cdf & 15))
        return fail(LLICTI_EINVAL, "ac_decode: bad argument (Lp<=512, row_stride multiple of 8, 4-byte aligned streams, 16-byte aligned tables)");
    DecOut o;
    memset(&o, 0, sizeof o);
    o.sym = d_sym;
    o.len = d_len;          // bytes past d_len[s] read as zero bits (torchac's get()), whatever the buffer holds there
    AcChunk ck = { 0, (int)N, (int)N, (int)N, nullptr };
    ac_decode_kernel<<<n_streams, 64, 0, (hipStream_t)stream>>>(d_cdf, Lp, row_stride, d_in, in_stride, ck, o);
    HIPCHK(hipGetLastError());
    return LLICTI_OK;
}

// ------------------------------------------------------------------------------------------------ whole batch
// A block of >= need bytes for a new plan's tables: one from the pool whose last user has finished, else a new one.  Never hipFree
// (which synchronises the device) before llicti_destroy; the pool is bounded by kMaxPlans + the blocks in flight.
static int acquire_block(llicti_ctx *c, size_t need, PlanBlock *out)
{
    int pick = -1, busy_fit = -1;
    for (int i = 0; i < (int)c->pool.size(); ++i) {
        PlanBlock &bk = c->pool[i];
        if (bk.cap < need) continue;
        if (!bk.used || hipEventQuery(bk.done) == hipSuccess) { if (pick < 0 || bk.cap < c->pool[pick].cap) pick = i; }
        else if (busy_fit < 0) busy_fit = i;
    }
    if (pick < 0 && busy_fit >= 0 && c->pool.size() >= 16) {      // plenty of blocks, all still in flight: wait for the oldest one's user (a stream-level wait)
        ++c->n_block_wait;
        HIPCHK(hipEventSynchronize(c->pool[busy_fit].done));
        pick = busy_fit;
    }
    if (pick >= 0) {
        *out = c->pool[pick];
        c->pool.erase(c->pool.begin() + pick);
        out->used = false;
        return 0;
    }
    PlanBlock bk;
    size_t cap = 256 << 10;
    while (cap < need) cap *= 2;
    bk.cap = cap;
    ++c->n_device_alloc;
    if (hipMalloc(&bk.dev, cap) != hipSuccess) return fail(LLICTI_EHIP, "plan tables: hipMalloc(%zu) failed", cap);
    if (hipHostMalloc(&bk.host, cap, hipHostMallocDefault) != hipSuccess) { (void)hipFree(bk.dev); return fail(LLICTI_EHIP, "plan tables: hipHostMalloc(%zu) failed", cap); }
    if (hipEventCreateWithFlags(&bk.done, hipEventDisableTiming) != hipSuccess || hipEventCreateWithFlags(&bk.uploaded, hipEventDisableTiming) != hipSuccess) {
        (void)hipFree(bk.dev); (void)hipHostFree(bk.host);
        if (bk.done) (void)hipEventDestroy(bk.done);
        return fail(LLICTI_EHIP, "plan tables: hipEventCreate failed");
    }
    *out = bk;
    return 0;
}

// The plan of a batch: cached by (mode, sizes, placement).  A miss builds the tables on the host, copies them into a pinned block and
// enqueues ONE asynchronous upload on the call's stream -- no device synchronisation, no allocation once the pool is warm.
// reduce >= 1 (llicti_decode_images_reduced): rgb_off places the REDUCED outputs; the plan itself is the batch's full-size one with tight
// placement (the unused default of its full-size fields) plus the reduced output table, under a key of its own (host_plan.hpp: plan_add_reduced).
// pix (llicti_encode_images_px / llicti_decode_images_px): the call's windows in the caller's interleaved buffer; rgb_off is unused (the planar
// fields of the plan keep their tight default), the window table and its key tail go behind everything else (host_plan.hpp: plan_add_pixels).
static int get_plan(llicti_ctx *c, int B, const int *Hs, const int *Ws, const size_t *rgb_off, int ME, const int *Ms, hipStream_t s, PlanDev **out, int reduce = 0,
                    const std::vector<PixGeo> *pix = nullptr)
{
    if (pix) rgb_off = nullptr;
    const size_t *red_off = reduce > 0 ? rgb_off : nullptr;
    if (reduce > 0) rgb_off = nullptr;
    const PlanSpec sp = ctx_spec(c, B, Hs, Ws, rgb_off, ME, Ms);
    std::vector<long> key = plan_key(sp);
    if (reduce > 0) reduced_key_tail(key, B, Hs, Ws, reduce, red_off);
    if (pix) pixel_key_tail(key, *pix);
    auto it = c->plans.find(key);
    if (it != c->plans.end()) {
        PlanDev *pd = it->second;
        ++c->n_plan_hit;
        pd->last_use = ++c->use_clock;
        if (pd->blk.up_stream != s) HIPCHK(hipStreamWaitEvent(s, pd->blk.uploaded, 0));      // (uploaded on another stream: order behind it)
        if (pd->blk.used && pd->blk.done_stream != s) HIPCHK(hipStreamWaitEvent(s, pd->blk.done, 0));      // (last used on another stream: this call's `done` must lie behind that use too)
        *out = pd;
        return 0;
    }
    std::unique_ptr<PlanDev> pd(new PlanDev());
    Plan &p = pd->p;
    ++c->n_plan_build;
    build_plan(p, sp);
    if (reduce > 0) plan_add_reduced(p, reduce, red_off);
    if (pix) plan_add_pixels(p, *pix);
    if (p.rslot_off.size() != (size_t)p.nstreams || p.sref.size() != (size_t)p.nstreams)
        return fail(LLICTI_EINVAL, "plan: stream tables have %zu / %zu entries, expected %d", p.rslot_off.size(), p.sref.size(), p.nstreams);
    if (int rc = acquire_block(c, p.d_total, &pd->blk)) return rc;
    uint8_t *h = pd->blk.host;
    auto put = [&](size_t off, const void *src, size_t n) { if (n) memcpy(h + off, src, n); };
    put(p.d_img, p.img.data(), p.img.size() * sizeof(ImgGeo));
    put(p.d_geo, p.geo.data(), p.geo.size() * sizeof(Geom));
    put(p.d_sg, p.sg.data(), p.sg.size() * sizeof(StageGeom));
    put(p.d_desc, p.desc.data(), p.desc.size() * sizeof(StreamDesc));
    put(p.d_slot_off, p.slot_off.data(), p.slot_off.size() * sizeof(long));
    put(p.d_slot_cap, p.slot_cap.data(), p.slot_cap.size() * sizeof(int32_t));
    put(p.d_rslot_off, p.rslot_off.data(), p.rslot_off.size() * sizeof(long));
    put(p.d_tiles, p.tiles.data(), p.tiles.size() * sizeof(TileRef));
    put(p.d_sref, p.sref.data(), p.sref.size() * sizeof(StreamRef));
    put(p.d_red, p.red.data(), p.red.size() * sizeof(RedGeo));
    put(p.d_pix, p.pix.data(), p.pix.size() * sizeof(PixGeo));
    bool ok = hipMemcpyAsync(pd->blk.dev, h, p.d_total, hipMemcpyHostToDevice, s) == hipSuccess;
    ok = ok && hipEventRecord(pd->blk.uploaded, s) == hipSuccess;
    ok = ok && hipEventRecord(pd->blk.done, s) == hipSuccess;      // (so that the block is never recycled in front of its own upload)
    pd->blk.up_stream = s;
    pd->blk.done_stream = s;
    pd->blk.used = true;
    if (!ok) { c->pool.push_back(pd->blk); return fail(LLICTI_EHIP, "plan tables: upload failed"); }
    p.tiles.clear(); p.tiles.shrink_to_fit();                      // (the host copy of the largest table is not needed again)
    if ((int)c->plans.size() >= kMaxPlans) {                       // least recently used out; its block waits in the pool for its last user
        auto lru = c->plans.begin();
        for (auto jt = c->plans.begin(); jt != c->plans.end(); ++jt) if (jt->second->last_use < lru->second->last_use) lru = jt;
        c->pool.push_back(lru->second->blk);
        delete lru->second;
        c->plans.erase(lru);
    }
    pd->last_use = ++c->use_clock;
    *out = pd.get();
    c->plans[key] = pd.release();
    return 0;
}

// status[0] -> the context's latched word (llicti_check_status); decode: the B per-image words -> the context's copy (llicti_image_status)
// the call's status words are cleared by a kernel of the call's own queue: hipMemsetAsync goes through the runtime's blit path, which left the queue
// idle for ~17 us in front of every encode and decode (rocprofv3 trace, tools/trace_gaps.py)
__global__ void zero_words_kernel(int32_t *p, int n)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) p[i] = 0;
}
__global__ void latch_status_kernel(const int32_t *status, int32_t *latched, int32_t *img_latched, int B)
{
    latch_status_all(status, kStatusHead, latched, img_latched, B);
}

// The last kernel of llicti_transcode_images (which launches no unlift): the source plan's status words -- what the decoder's kernels flagged,
// per call and per image -- and the target plan's (LLICTI_ENOSPACE) merged into the context's, as latch_status_kernel / unlift_kernel do for
// an encode / a decode.  A flagged image's row of the output segment lengths becomes 49 zeros: what the coder made of its (deterministic)
// garbage pixels is no container.
__global__ void transcode_latch_kernel(const int32_t *src_status, const int32_t *dst_status, int32_t *latched, int32_t *img_latched, int B,
                                       int32_t *__restrict__ seg_len)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t == 0) {
        const int32_t st = src_status[0] != 0 ? src_status[0] : dst_status[0];
        if (st != 0) *latched = st;
    }
    if (t < B) img_latched[t] = src_status[kStatusHead + t];
    if (t < B * LLICTI_NSEG && src_status[kStatusHead + t / LLICTI_NSEG] != 0) seg_len[t] = 0;
}

// The profiled extent of one whole-batch call: the closing event is recorded on EVERY way out (an early error return
// included), so llicti_last_timing never waits on an event of a call that did not record it.
struct CallScope {
    llicti_ctx *c;
    hipStream_t s;
    bool on;
    CallScope(llicti_ctx *c_, hipStream_t s_) : c(c_), s(s_), on(c_->profiling)
    {
        c->ev_used = 0;
        c->spans.clear();
        c->last_ev = nullptr;
        c->timing_pending = false;
        if (on) on = hipEventRecord(c->ev_call[0], s) == hipSuccess;
        if (on) { c->last_ev = c->ev_call[0]; c->last_ev_stream = s; }
    }
    ~CallScope() { if (on && hipEventRecord(c->ev_call[1], s) == hipSuccess) c->timing_pending = true; }
    CallScope(const CallScope &) = delete;
    CallScope &operator=(const CallScope &) = delete;
};

// marks the plan's table block as in use behind everything the call enqueued (get_plan: blocks are recycled, never freed)
struct PlanUse {
    PlanDev *pd; hipStream_t s;
    ~PlanUse() { if (pd && hipEventRecord(pd->blk.done, s) == hipSuccess) { pd->blk.used = true; pd->blk.done_stream = s; } }
};

// The per-call tables of an _rv decode (host_plan.hpp: ReduceSchedule) in a block of the plans' pool: taken for the call, uploaded with ONE
// asynchronous copy on the call's stream, handed back to the pool behind the call's last kernel (`done`, as PlanUse records it) -- so a steady
// stream of calls with fresh reduces neither allocates nor synchronises, and nothing of it enters the plan cache or its LRU.
struct RvCall {
    llicti_ctx *c = nullptr;
    hipStream_t s = nullptr;
    ReduceSchedule q;
    PlanBlock blk;
    bool have = false;
    template <class T> const T *dev(size_t off) const { return reinterpret_cast<const T *>(blk.dev + off); }
    int upload()
    {
        if (int rc = acquire_block(c, q.d_total, &blk)) return rc;
        have = true;
        write_reduce_schedule(q, blk.host);
        if (hipMemcpyAsync(blk.dev, blk.host, q.d_total, hipMemcpyHostToDevice, s) != hipSuccess) return fail(LLICTI_EHIP, "per-image reduce tables: upload failed");
        return 0;
    }
    ~RvCall()
    {
        if (!have) return;
        if (hipEventRecord(blk.done, s) == hipSuccess) { blk.used = true; blk.done_stream = s; }
        c->pool.push_back(blk);
    }
    RvCall() = default;
    RvCall(const RvCall &) = delete;
    RvCall &operator=(const RvCall &) = delete;
};

// the pixel arguments of llicti_encode_images_px / llicti_decode_images_px as the caller gave them (host_plan.hpp: resolve_pixels)
struct PixArgs { int fmt; const size_t *off, *pitch; };

extern "C" int llicti_workspace_params_v(llicti_ctx *c, int B, const int *Hs, const int *Ws, const int *modes, int image, size_t *off_params, long *npos)
{
    if (!c || !off_params || !npos || !modes) return fail(LLICTI_EINVAL, "workspace_params_v: null argument");
    if (check_dims_v(B, Hs, Ws)) return LLICTI_EINVAL;
    if (image < 0 || image >= B) return fail(LLICTI_EINVAL, "workspace_params_v: image %d of %d", image, B);
    int ME = 0;
    std::vector<int> Ms;
    if (int rc = resolve_modes("workspace_params_v", modes, B, B, &ME, Ms)) return rc;
    Plan p;
    build_plan(p, ctx_spec(c, B, Hs, Ws, nullptr, ME, modes_ptr(Ms)));
    const Geom &g = p.geo[(size_t)0 * B + image];            // level 0: the last level both passes launch
    *off_params = p.off_params + (size_t)g.par_off * sizeof(float);
    *npos = (long)g.h * g.w;
    return LLICTI_OK;
}

// The entropy-coder back end of an encode, from the plan's pairs to the containers behind their headers: the range coder of the reference format,
// or the rANS coder (with the encoder's stream-count pick for "auto" images).  ws: the workspace part laid out by pd's plan (pairs, slots, status);
// planes, mm: the call's planes and min/max words (an encode's own; a transcode's decoder's, which sit in the source plan's part).
static int encode_back_end(llicti_ctx *c, PlanDev *pd, uint8_t *ws, const int16_t *planes, const int32_t *mm, uint8_t *d_out, size_t out_stride,
                           int32_t *d_seg_len, hipStream_t s)
{
    const Plan &p = pd->p;
    const int B = p.B, M = p.M, Q = p.Q;
    const bool autoM = (p.ME & 0x1000) != 0;
    int32_t *status = (int32_t *)(ws + p.off_status);
    uint32_t *pairs = (uint32_t *)(ws + p.off_pairs);
    uint8_t *slots = ws + p.off_slots;
    int32_t *slot_len = (int32_t *)(ws + p.off_slot_len);
    const ImgGeo *d_img = pd->dev<ImgGeo>(p.d_img);
    const StageGeom *d_sg = pd->dev<StageGeom>(p.d_sg);
    const StreamDesc *d_desc = pd->dev<StreamDesc>(p.d_desc);
    const long *d_rslot_off = pd->dev<long>(p.d_rslot_off);
    const StreamRef *d_sref = pd->dev<StreamRef>(p.d_sref);
    if (M == 0) {
        ProfSpan span(c, PROF_AC, s);
        const int st0 = first_stage(p.nlev), nst = LLICTI_NSTREAMS - st0;      // (the model's stages)
        const int n_streams = nst * B;
        ac_encode_pairs_kernel<<<n_streams, 64, 0, s>>>(pairs, d_desc + (size_t)st0 * B, n_streams, slots, slot_len + (size_t)st0 * B, status);
        pack_kernel<<<dim3(nst, B), 256, 0, s>>>(slots, pd->dev<long>(p.d_slot_off), slot_len, B, p.img[0].hdr_bytes, d_out, (long)out_stride, d_seg_len, status, st0);
    } else {
        ProfSpan span(c, PROF_RANS_ENC, s);
        int32_t *rinfo = (int32_t *)(ws + p.off_rinfo);
        const StageGeom *sglv = d_sg + (size_t)(0 * 3 + 2) * B;      // the last stage: an xwide stream's seed symbols are read from its pixels
        const int NS = p.nstreams;                                   // the streams of all images (an image's count is its own: ImgGeo::M)
        // LLICTI_MODE_RANS_X_AUTO: each image's stream count is picked here, on the device, from what its last stage costs (a pure function of
        // the image); the table holds the most it may get, the streams it does not get are empty segments
        unsigned long long *ssum = autoM ? (unsigned long long *)(ws + p.off_rpos) : nullptr;      // (the decoder's cursor array: unused by an encode; B x 8 bytes of its >= B x 128)
        if (autoM) choose_streams_kernel<<<dim3(kAutoSlices, B), 256, 0, s>>>(pairs, d_desc, B, ssum);
        if (Q == 4) rans_encode_kernel<4><<<NS, 256, 0, s>>>(pairs, d_desc, B, d_sref, slots, d_rslot_off, p.rslot_cap, rinfo, status, sglv, planes, mm, ssum, d_img);
        else if (Q == 2) rans_encode_kernel<2><<<NS, 128, 0, s>>>(pairs, d_desc, B, d_sref, slots, d_rslot_off, p.rslot_cap, rinfo, status, sglv, planes, mm, ssum, d_img);
        else rans_encode_kernel<1><<<NS, 64, 0, s>>>(pairs, d_desc, B, d_sref, slots, d_rslot_off, p.rslot_cap, rinfo, status, sglv, planes, mm, ssum, d_img);
        rans_pack_kernel<<<NS, 256, 0, s>>>(slots, d_rslot_off, rinfo, d_sref, d_img, d_out, (long)out_stride, d_seg_len, status, ssum, d_desc, B);
    }
    HIPCHK(hipGetLastError());
    return 0;
}

// The pixels of an encode: d of the kind's element type.  PlanarF32: rgb_off counts ELEMENTS -- the plan is the uint8 call's on the same numbers;
// Interleaved: px, the windows as the caller gave them (rgb_off is not read).
struct EncodeSrc { PixelSrc kind; const void *d; PixArgs px; };

static int encode_batch(llicti_ctx *c, const EncodeSrc &src, const size_t *rgb_off, int B, const int *Hs, const int *Ws, const int *modes, int n_modes,
                        void *d_workspace, size_t workspace_bytes, uint8_t *d_out, size_t out_stride, int32_t *d_seg_len, void *stream)
{
    if (!c || !src.d || !d_workspace || !d_out || !d_seg_len) return fail(LLICTI_EINVAL, "encode_images: null pointer");
    if (check_dims_v(B, Hs, Ws)) return LLICTI_EINVAL;
    const bool px = src.kind == PixelSrc::Interleaved;
    std::vector<PixGeo> pix;
    if (px) if (int rc = resolve_pixels("encode_images_px", B, Hs, Ws, src.px.fmt, src.px.off, src.px.pitch, pix)) return rc;
    int ME = 0;
    std::vector<int> Ms;
    if (int rc = resolve_modes("encode_images", modes, n_modes, B, &ME, Ms)) return rc;
    if (int rc = check_model(c->nlev, "encode_images", ME, Ms)) return rc;
    if (int rc = check_stream_bits("encode_images", c->nlev, B, Hs, Ws, ME, Ms)) return rc;
    if (int rc = check_header_grid("encode_images", c->nlev, B, Hs, Ws)) return rc;
    const bool autoM = (ME & 0x1000) != 0;
    for (int b = 0; b < 3; ++b) if (!c->have[b]) return fail(LLICTI_ENOWEIGHTS, "band %d weights not set", b);
    DeviceGuard guard(c);
    hipStream_t s = (hipStream_t)stream;
    PlanDev *pd = nullptr;
    if (int rc = get_plan(c, B, Hs, Ws, rgb_off, ME, modes_ptr(Ms), s, &pd, 0, px ? &pix : nullptr)) return rc;
    PlanUse use{ pd, s };
    const Plan &p = pd->p;
    const int M = p.M;
    if (!p.uniform && M == 0) return fail(LLICTI_EINVAL, "encode_images: a batch of mixed sizes needs a rANS container (the reference-format container codes equal sizes per call)");
    if (workspace_bytes < p.total) return fail(LLICTI_ENOSPACE, "encode_images: workspace %zu < %zu", workspace_bytes, p.total);
    if (out_stride < p.max_container) return fail(LLICTI_ENOSPACE, "encode_images: out_stride %zu < %zu", out_stride, p.max_container);
    uint8_t *ws = (uint8_t *)d_workspace;
    int16_t *planes = (int16_t *)(ws + p.off_planes);
    float *fplanes = (float *)(ws + p.off_fplanes);
    int32_t *mm = (int32_t *)(ws + p.off_minmax);
    int32_t *status = (int32_t *)(ws + p.off_status);
    uint32_t *pairs = (uint32_t *)(ws + p.off_pairs);
    const ImgGeo *d_img = pd->dev<ImgGeo>(p.d_img);
    const Geom *d_geo = pd->dev<Geom>(p.d_geo);
    const StageGeom *d_sg = pd->dev<StageGeom>(p.d_sg);
    const TileRef *d_tiles = p.uniform ? nullptr : pd->dev<TileRef>(p.d_tiles);

    CallScope call(c, s);
    {
        ProfSpan span(c, PROF_MISC, s);
        // (the lift is the call's first kernel and sets no status: it clears the call's status words on the way)
        unsigned long long *ssum0 = autoM ? (unsigned long long *)(ws + p.off_rpos) : nullptr;
        const PixGeo *d_pv = px ? pd->dev<PixGeo>(p.d_pix) : nullptr;
        const uint8_t *d_u8 = (const uint8_t *)src.d;
        if (int rc = launch_lift(src.kind, src.d, B, px ? p.pix_units : p.max_plane, p.vec_ok, planes, fplanes, mm, (int32_t *)(ws + p.off_lift_part), s, status,
                                 kStatusHead + B, d_img, d_pv)) return rc;
        if (px) header_write_px_kernel<<<B, 256, 0, s>>>(d_u8, d_pv, mm, d_img, d_out, (long)out_stride, d_seg_len, ssum0);
        // (float samples: the header's raw DC band is the planes just made, back through the integer lift -- the pixel values, without a second conversion)
        else if (src.kind == PixelSrc::PlanarF32) header_transcode_kernel<<<B, 256, 0, s>>>(planes, mm, d_img, d_out, (long)out_stride, d_seg_len, ssum0, nullptr, 0);
        else header_write_kernel<<<B, 256, 0, s>>>(d_u8, mm, d_img, d_out, (long)out_stride, d_seg_len, ssum0);
    }
    // The encoder has no dependency between stages: every (level, band) reads only original pixels.  With llicti_set_tuning("enc_side_levels", 1)
    // levels 4..1 (twelve CNN + twelve pairs launches, a quarter of the work) run on a side stream next to level 0's, with their own
    // quarter-size buffer for the CNN outputs.  Two CNN launches cannot share a compute unit (a workgroup holds 81-155 KB of its 160 KB LDS),
    // so this is no second queue of matrix work: what overlaps is the small stuff -- a pairs kernel under the other queue's CNN launch, a
    // launch's ramp-down under the other's ramp-up.  Measured (profiles/r4/ab_encoder_side_stream.json): -0.5 ... -4 % per encode, 10.75 ->
    // 10.68 ms at B = 24 -- 0.3 % of a step, for which every kernel trace of the run shows the side queue's launches with the time they
    // spend waiting for a compute unit inside their durations.  Off by default: the per-kernel evidence is worth more than 0.07 ms.
    const bool side = c->enc_side_levels != 0 && !c->profiling;      // (the profiling spans assume one queue)
    hipStream_t s2 = side ? c->sub[1] : s;
    if (side) {
        HIPCHK(hipEventRecord(c->ev_enc[0], s));      // lift and header are done
        HIPCHK(hipStreamWaitEvent(s2, c->ev_enc[0], 0));
    }
    for (int lvl = p.nlev - 1; lvl >= 0; --lvl) {
        const Geom &g = p.geo[(size_t)lvl * B];                         // image 0's (equal sizes: every image's)
        const Geom *gv = p.uniform ? nullptr : d_geo + (size_t)lvl * B;
        hipStream_t ls = (lvl >= 1) ? s2 : s;                           // the level's queue
        float *params = (lvl >= 1 && side) ? (float *)(ws + p.off_params2) : (float *)(ws + p.off_params);
        const unsigned pairs_gx = (unsigned)((p.lev_maxpos[lvl] + kPairsThreads - 1) / kPairsThreads);
        if (lvl >= 1 && !side) {
            // Levels 4..1: the three bands' CNN outputs side by side in the buffer (each a quarter of what level 0 needs of it, or less),
            // then ONE pairs launch for the three bands: 3 + 1 launches per level instead of 3 + 3.
            PairsBands pb;
            for (int band = 0; band < 3; ++band) {
                float *pband = params + band * p.lev_floats[lvl];
                if (int rc = launch_band_params(c, fplanes, g, band, pband, ls, gv, d_tiles ? d_tiles + p.run[lvl * 3 + band].off : nullptr, &p.run[lvl * 3 + band])) return rc;
                pb.sv[band] = d_sg + (size_t)(lvl * 3 + band) * B;
                pb.params[band] = pband;
                pb.pairs[band] = pairs + p.pair_base[lvl * 3 + band];
            }
            ProfSpan span(c, PROF_PAIRS, ls);
            cdf_pairs_bands_kernel<<<dim3(pairs_gx, B, 3), kPairsThreads, 0, ls>>>(planes, pb, mm);
            HIPCHK(hipGetLastError());
            continue;
        }
        for (int band = 0; band < 3; ++band) {
            // (a launch's CNN outputs are read once, by the pairs kernel right behind it; cutting level 0 into sub-batches whose outputs stay in
            // the memory-side cache was measured and bought nothing: profiles/r4/tried_encoder_subbatch.json)
            if (int rc = launch_band_params(c, fplanes, g, band, params, ls, gv, d_tiles ? d_tiles + p.run[lvl * 3 + band].off : nullptr, &p.run[lvl * 3 + band])) return rc;
            ProfSpan span(c, PROF_PAIRS, ls);
            const StageGeom *sv = d_sg + (size_t)(lvl * 3 + band) * B;
            cdf_pairs_kernel<<<dim3(pairs_gx, B), kPairsThreads, 0, ls>>>(planes, params, mm, p.sg[(size_t)(lvl * 3 + band) * B], sv, pairs + p.pair_base[lvl * 3 + band]);
            HIPCHK(hipGetLastError());
        }
    }
    if (side) {
        HIPCHK(hipEventRecord(c->ev_enc[1], s2));
        HIPCHK(hipStreamWaitEvent(s, c->ev_enc[1], 0));
    }
    if (int rc = encode_back_end(c, pd, ws, planes, mm, d_out, out_stride, d_seg_len, s)) return rc;
    latch_status_kernel<<<1, 64, 0, s>>>(status, c->d_status, nullptr, 0);
    HIPCHK(hipGetLastError());
    return LLICTI_OK;
}

extern "C" int llicti_encode_images_v(llicti_ctx *c, const uint8_t *d_rgb, const size_t *rgb_off, int B, const int *Hs, const int *Ws, int mode,
                                      void *d_workspace, size_t workspace_bytes,
                                      uint8_t *d_out, size_t out_stride, int32_t *d_seg_len, void *stream)
{
    return encode_batch(c, { PixelSrc::PlanarU8, d_rgb, {} }, rgb_off, B, Hs, Ws, &mode, 1, d_workspace, workspace_bytes, d_out, out_stride, d_seg_len, stream);
}

extern "C" int llicti_encode_images_vm(llicti_ctx *c, const uint8_t *d_rgb, const size_t *rgb_off, int B, const int *Hs, const int *Ws, const int *modes,
                                       void *d_workspace, size_t workspace_bytes,
                                       uint8_t *d_out, size_t out_stride, int32_t *d_seg_len, void *stream)
{
    return encode_batch(c, { PixelSrc::PlanarU8, d_rgb, {} }, rgb_off, B, Hs, Ws, modes, B, d_workspace, workspace_bytes, d_out, out_stride, d_seg_len, stream);
}

extern "C" int llicti_encode_images(llicti_ctx *c, const uint8_t *d_rgb, int B, int H, int W, int mode,
                                    void *d_workspace, size_t workspace_bytes,
                                    uint8_t *d_out, size_t out_stride, int32_t *d_seg_len, void *stream)
{
    if (check_dims(B, H, W)) return LLICTI_EINVAL;
    std::vector<int> Hs(B, H), Ws(B, W);
    return encode_batch(c, { PixelSrc::PlanarU8, d_rgb, {} }, nullptr, B, Hs.data(), Ws.data(), &mode, 1, d_workspace, workspace_bytes, d_out, out_stride, d_seg_len, stream);
}

// ------------------------------------------------------------------------------------------------ decode
// One whole-batch decode as its entry point received it: containers, images, container modes, workspace, where a Planar sink's images go
// (rgb_off; NULL: tight, and for every other kind), the caller's stream, and the level(s) the images stop at.
struct DecodeCall {
    const uint8_t *d_in; size_t in_stride; const int32_t *d_seg_len;
    int B; const int *Hs, *Ws, *modes; int n_modes;
    void *d_workspace; size_t workspace_bytes;
    const size_t *rgb_off;
    void *stream;
    Reduces rd;
};

// What a whole-batch decode ends in: ONE value of one kind.  An entry point fills in what its caller gave (one builder per kind, below);
// decode_batch validates that against the call's images (resolve_sink: the kind's payload, which is all launch_sink reads) -- reduced planar
// output is Planar at reduce > 0.
struct DecodeSink {
    enum Kind { Planar, Interleaved, Tensor, Resized, Views, Transcode, Cuts } kind = Planar;
    uint8_t *d_out = nullptr;               // the caller's buffer (Views: none, every group has its own)
    // as the caller gave them
    PixArgs px{};                           // Interleaved
    TensorArgs tensor{};                    // Tensor
    ResizeArgs resize{};                    // Resized
    ViewArgs views{};                       // Views
    // validated
    std::vector<PixGeo> pix;                // Interleaved: the windows (they enter the plan)
    std::vector<uint32_t> wins;             // Tensor: a packed window per image; Resized: two packed words per image
    std::vector<ViewGroupOut> groups;       // Views: three packed words per view
    TensorNorm nm{};                        // Tensor, Resized, Views
    // the _o calls: the caller's options (has_opts: they ask for something the unlift_* kernels do not do), validated into `pad`
    bool has_opts = false;
    llicti_tensor_opts opts{};
    TensorPad pad{};                        // Tensor, Resized, Views: layout; Tensor: pad mode, fill space, fill (wins then holds pad_win_pack's two words per image)
    // Transcode (llicti_transcode_images): the target plan of the call and its part of the workspace.  decode_stages launches cdf_pairs_kernel
    // behind every (level, band) stage -- the stage's CNN outputs and symbols are exactly what the encoder's pairs are made of -- and no unlift.
    PlanDev *target = nullptr;
    uint8_t *target_ws = nullptr;
    // Cuts (llicti_level_cuts): d_out is the call's int32 [B][128][LLICTI_NLEVELS] table.  decode_stages zeroes it and writes every stream's byte
    // cursor behind each level >= 1 (level_cuts_kernel); no pixels -- the sink latches the status words alone.
};
static DecodeSink planar_sink(uint8_t *d_rgb) { DecodeSink k; k.d_out = d_rgb; return k; }
static DecodeSink px_sink(uint8_t *d_pix, const PixArgs &px) { DecodeSink k; k.kind = DecodeSink::Interleaved; k.d_out = d_pix; k.px = px; return k; }
static DecodeSink tensor_sink(void *d_out, const TensorArgs &t) { DecodeSink k; k.kind = DecodeSink::Tensor; k.d_out = (uint8_t *)d_out; k.tensor = t; return k; }
static DecodeSink resized_sink(void *d_out, const ResizeArgs &t) { DecodeSink k; k.kind = DecodeSink::Resized; k.d_out = (uint8_t *)d_out; k.resize = t; return k; }
static DecodeSink views_sink(const ViewArgs &a) { DecodeSink k; k.kind = DecodeSink::Views; k.views = a; return k; }
// (opts NULL or plain: the sink is the _rv sibling's, to the last launch)
static DecodeSink with_opts(DecodeSink k, const llicti_tensor_opts *opts) { if (!tensor_opts_plain(opts)) { k.has_opts = true; k.opts = *opts; } return k; }
static DecodeSink cuts_sink(int32_t *d_cuts) { DecodeSink k; k.kind = DecodeSink::Cuts; k.d_out = (uint8_t *)d_cuts; return k; }

static int resolve_sink(DecodeSink &k, int B, const int *Hs, const int *Ws, const Reduces &rd)
{
    switch (k.kind) {
    case DecodeSink::Interleaved: {
        std::vector<int> Hw(B), Ww(B);      // the windows: the reduced sizes
        for (int b = 0; b < B; ++b) { Hw[b] = reduced_dim(Hs[b], rd.of(b)); Ww[b] = reduced_dim(Ws[b], rd.of(b)); }
        return resolve_pixels("decode_images_px", B, Hw.data(), Ww.data(), k.px.fmt, k.px.off, k.px.pitch, k.pix);
    }
    case DecodeSink::Tensor:
        if (k.has_opts) return resolve_tensor_padded("decode_images_tensor_o", B, Hs, Ws, rd, k.tensor, k.opts, k.wins, k.nm, k.pad);
        return resolve_tensor("decode_images_tensor", B, Hs, Ws, rd, k.tensor, k.wins, k.nm);
    case DecodeSink::Resized:
        if (k.has_opts) if (int rc = resolve_tensor_opts("decode_images_tensor_resized_o", k.opts, false, k.pad)) return rc;
        return resolve_resize("decode_images_tensor_resized", B, Hs, Ws, rd, k.resize, k.wins, k.nm);
    case DecodeSink::Views:
        if (k.has_opts) if (int rc = resolve_tensor_opts("decode_images_tensor_views_o", k.opts, false, k.pad)) return rc;
        return resolve_views("decode_images_tensor_views", B, Hs, Ws, rd, k.views, k.groups, k.nm);
    default:
        return 0;
    }
}

// What differs between a plan-driven decode and an _rv one, resolved ONCE per call (plan_run / rv_run) so that no launch asks which it is.
// A level: the streams that take part in it (act: their indices in the plan's stream table, nullptr = all NS of them), the band CNN's Geom table
// (nullptr: the division form of an equal-size plan), its three TileRuns and the tile table their offsets count in (nullptr: none).
struct LevelRun { int NS; const int *act; const Geom *gv; const TileRun *run; const TileRef *tiles; };
struct DecodeRun {
    int stop;                               // levels nlev - 1 .. stop run
    LevelRun lev[LLICTI_NLEVELS];
    // the sink: the reduce every image stops at, or rtab with each image's own (r is 0 then: the kernels read the table); the reduced output
    // table and the pixel windows (nullptr: none), and what sizes the grids of unlift_reduced_kernel / unlift_px_kernel
    int r; const int *rtab; const RedGeo *d_red; const PixGeo *d_pix; long max_rplane, pix_units;
};
static DecodeRun plan_run(PlanDev *pd, int reduce)
{
    const Plan &p = pd->p;
    DecodeRun r{ reduce, {}, reduce, nullptr, reduce > 0 ? pd->dev<RedGeo>(p.d_red) : nullptr, p.pix.empty() ? nullptr : pd->dev<PixGeo>(p.d_pix), p.max_rplane, p.pix_units };
    for (int lvl = 0; lvl < LLICTI_NLEVELS; ++lvl)
        r.lev[lvl] = { p.nstreams, nullptr, p.uniform ? nullptr : pd->dev<Geom>(p.d_geo) + (size_t)lvl * p.B, &p.run[lvl * 3], p.uniform ? nullptr : pd->dev<TileRef>(p.d_tiles) };
    return r;
}
// (rANS containers only: level lvl runs for the images with r_b <= lvl alone -- the band CNN in its tile-list form over the call's list of that
// level, on an equal-size plan too: its Geom table is on the device; the stage kernels and the tail with one workgroup per ACTIVE stream)
static DecodeRun rv_run(PlanDev *pd, const RvCall &rv)
{
    const Plan &p = pd->p;
    const ReduceSchedule &q = rv.q;
    DecodeRun r{ q.rmin, {}, 0, rv.dev<int>(q.d_r), rv.dev<RedGeo>(q.d_red), q.pix.empty() ? nullptr : rv.dev<PixGeo>(q.d_pix), q.max_rplane, q.pix_units };
    for (int lvl = 0; lvl < LLICTI_NLEVELS; ++lvl)
        r.lev[lvl] = { q.s_n[lvl], rv.dev<int>(q.d_streams) + q.s_off[lvl], pd->dev<Geom>(p.d_geo) + (size_t)lvl * p.B, &q.run[lvl * 3], rv.dev<TileRef>(q.d_tiles) };
    return r;
}

// calls f with a value of the element type an output tensor's (validated) dtype names
template <typename F> static void with_tensor_type(int dtype, F &&f)
{
    if (dtype == LLICTI_T_F32) f(float());
    else if (dtype == LLICTI_T_F16) f(_Float16());
    else f(bf16_bits());
}
// the by-value kernel argument S of one launch: entries first .. first + n - 1 of the call's table of k words per entry, zeros behind them
template <typename S> static S arg_slice(const std::vector<uint32_t> &words, int k, int first, int n)
{
    S a;
    memset(&a, 0, sizeof a);
    memcpy(a.w, words.data() + (size_t)k * first, (size_t)k * n * sizeof(uint32_t));
    return a;
}

// Where the kernels of a decode find their data: the workspace as pd's plan carves it, and the plan's device tables
struct DecodeBufs {
    int16_t *planes; float *fplanes; int32_t *mm, *status; float *params; uint8_t *slots, *tables; uint32_t *acstate; int32_t *slot_len;
    uint32_t *rstate, *rpos, *rtail;
    const ImgGeo *d_img; const StageGeom *d_sg; const long *d_rslot_off; const StreamRef *d_sref;
    DecodeBufs(const PlanDev *pd, uint8_t *ws)
    {
        const Plan &p = pd->p;
        planes = (int16_t *)(ws + p.off_planes); fplanes = (float *)(ws + p.off_fplanes); mm = (int32_t *)(ws + p.off_minmax);
        status = (int32_t *)(ws + p.off_status); params = (float *)(ws + p.off_params); slots = ws + p.off_slots; tables = ws + p.off_tables;
        acstate = (uint32_t *)(ws + p.off_acstate); slot_len = (int32_t *)(ws + p.off_slot_len);
        rstate = (uint32_t *)(ws + p.off_rstate); rpos = (uint32_t *)(ws + p.off_rpos); rtail = (uint32_t *)(ws + p.off_rtail);
        d_img = pd->dev<ImgGeo>(p.d_img); d_sg = pd->dev<StageGeom>(p.d_sg); d_rslot_off = pd->dev<long>(p.d_rslot_off); d_sref = pd->dev<StreamRef>(p.d_sref);
    }
};

// The last kernel(s) of a decode, one block per kind.  Each latches the call's status words into the context's (the workspace is the caller's:
// it may be gone or reused by the time the words are read); every side stream of the reference-format pipeline was joined back onto `s` at the
// end of its band, so nothing is pending here.
static int launch_sink(llicti_ctx *c, const Plan &p, const DecodeBufs &w, const DecodeSink &k, hipStream_t s, const DecodeRun &o)
{
    const int B = p.B;
    if (k.kind == DecodeSink::Transcode) return 0;      // (no pixels: the caller goes on with the target's header and coder, and latches the status words itself)
    ProfSpan span(c, PROF_MISC, s);
    switch (k.kind) {
    case DecodeSink::Cuts:
        level_cuts_latch_kernel<<<1, 256, 0, s>>>(w.status, kStatusHead, c->d_status, c->d_img_status, B);
        break;
    case DecodeSink::Tensor: {
        // full size or reduced: the windows are this call's kernel arguments, kTensorWinMax images per launch; every launch latches its own
        // images' status words, the first one the call's
        const TensorArgs &t = k.tensor;
        const int gx = (int)std::min<long>(((long)t.Ho * ((t.Wo + 3) / 4) + 255) / 256, 1024);
        if (k.has_opts) {      // (a padded window or the NHWC layout: two signed words per image, kPadWinMax images per launch, the same latches)
            for (int b0 = 0; b0 < B; b0 += kPadWinMax) {
                const int nb = std::min(kPadWinMax, B - b0);
                const PadWins pw = arg_slice<PadWins>(k.wins, 2, b0, nb);
                with_tensor_type(t.dtype, [&](auto e) {
                    using T = decltype(e);
                    sink_window_kernel<T><<<dim3(gx, nb), 256, 0, s>>>(w.planes, (T *)k.d_out, o.r, t.Ho, t.Wo, b0, pw, k.nm, k.pad, w.status, kStatusHead, c->d_status,
                                                                      c->d_img_status, w.d_img, o.rtab);
                });
            }
            break;
        }
        for (int b0 = 0; b0 < B; b0 += kTensorWinMax) {
            const int nb = std::min(kTensorWinMax, B - b0);
            const TensorWins tw = arg_slice<TensorWins>(k.wins, 1, b0, nb);
            with_tensor_type(t.dtype, [&](auto e) {
                using T = decltype(e);
                unlift_tensor_kernel<T><<<dim3(gx, nb), 256, 0, s>>>(w.planes, (T *)k.d_out, o.r, t.Ho, t.Wo, b0, tw, k.nm, w.status, kStatusHead, c->d_status,
                                                                    c->d_img_status, w.d_img, o.rtab);
            });
        }
        break;
    }
    case DecodeSink::Resized: {
        // boxes, flips, output size and filter flag are this call's kernel arguments, kResizeBoxMax images per launch; a workgroup per 16 x 64
        // tile of an image's output; the status words as above
        const ResizeArgs &t = k.resize;
        const int tiles_x = (t.Wo + kResizeTileW - 1) / kResizeTileW, tiles_y = (t.Ho + kResizeTileH - 1) / kResizeTileH;
        for (int b0 = 0; b0 < B; b0 += kResizeBoxMax) {
            const int nb = std::min(kResizeBoxMax, B - b0);
            const ResizeBoxes bx = arg_slice<ResizeBoxes>(k.wins, 2, b0, nb);
            with_tensor_type(t.dtype, [&](auto e) {
                using T = decltype(e);
                if (k.pad.layout == LLICTI_LAYOUT_NHWC)
                    sink_resize_nhwc_kernel<T><<<dim3(tiles_x * tiles_y, nb), 256, 0, s>>>(w.planes, (T *)k.d_out, o.r, t.Ho, t.Wo, b0, tiles_x, t.antialias, bx, k.nm,
                                                                                          w.status, kStatusHead, c->d_status, c->d_img_status, w.d_img, o.rtab);
                else
                unlift_resize_tensor_kernel<T><<<dim3(tiles_x * tiles_y, nb), 256, 0, s>>>(w.planes, (T *)k.d_out, o.r, t.Ho, t.Wo, b0, tiles_x, t.antialias, bx, k.nm,
                                                                                          w.status, kStatusHead, c->d_status, c->d_img_status, w.d_img, o.rtab);
            });
        }
        break;
    }
    case DecodeSink::Views: {
        // group after group, kViewMax views per launch, a workgroup per 16 x 64 tile of a view's output; boxes, flips, image indices, output size
        // and filter flag are kernel arguments.  The call's first launch latches the status words of all B images.
        int latch_n = B;
        for (const ViewGroupOut &g : k.groups) {
            const int tiles_x = (g.Wo + kResizeTileW - 1) / kResizeTileW, tiles_y = (g.Ho + kResizeTileH - 1) / kResizeTileH;
            for (int v0 = 0; v0 < g.n; v0 += kViewMax) {
                const int nv = std::min(kViewMax, g.n - v0);
                const ViewSlice vs = arg_slice<ViewSlice>(g.words, 3, v0, nv);
                with_tensor_type(g.dtype, [&](auto e) {
                    using T = decltype(e);
                    if (k.pad.layout == LLICTI_LAYOUT_NHWC)
                        sink_views_nhwc_kernel<T><<<dim3(tiles_x * tiles_y, nv), 256, 0, s>>>(w.planes, (T *)g.d_out, o.r, g.Ho, g.Wo, v0, tiles_x, g.antialias, vs, k.nm,
                                                                                             w.status, kStatusHead, c->d_status, c->d_img_status, w.d_img, latch_n, o.rtab);
                    else
                    unlift_views_tensor_kernel<T><<<dim3(tiles_x * tiles_y, nv), 256, 0, s>>>(w.planes, (T *)g.d_out, o.r, g.Ho, g.Wo, v0, tiles_x, g.antialias, vs, k.nm,
                                                                                             w.status, kStatusHead, c->d_status, c->d_img_status, w.d_img, latch_n, o.rtab);
                });
                latch_n = 0;
            }
        }
        break;
    }
    case DecodeSink::Interleaved: {
        // full size or reduced: one kernel, the window table behind the call's others
        const int gx = (int)std::min<long>((o.pix_units + 255) / 256, 1024);
        unlift_px_kernel<<<dim3(gx, B), 256, 0, s>>>(w.planes, k.d_out, o.r, w.status, kStatusHead, c->d_status, c->d_img_status, w.d_img, o.d_red, o.d_pix, o.rtab);
        break;
    }
    default:                                            // Planar (Transcode has returned above)
        if (o.d_red) {
            unlift_reduced_kernel<<<dim3((unsigned)((o.max_rplane + 255) / 256), B), 256, 0, s>>>(w.planes, k.d_out, o.r, w.status, kStatusHead, c->d_status,
                                                                                                  c->d_img_status, w.d_img, o.d_red, o.rtab);
        } else {
            const int gx = (int)std::min<long>((p.max_plane + 255) / 256, 1024);
            unlift_kernel<<<dim3(gx, B), 256, 0, s>>>(w.planes, p.max_plane, k.d_out, w.status, kStatusHead, c->d_status, c->d_img_status, w.d_img);
        }
    }
    HIPCHK(hipGetLastError());
    return 0;
}

// The front of a decode: the call's status words cleared, the headers read, the containers unpacked into the slots, the rANS states set up
static int decode_prologue(llicti_ctx *c, PlanDev *pd, const DecodeBufs &w, const DecodeCall &a, hipStream_t s)
{
    const Plan &p = pd->p;
    const int B = p.B, Q = p.Q, NS = p.nstreams;
    zero_words_kernel<<<(kStatusHead + B + 255) / 256, 256, 0, s>>>(w.status, kStatusHead + B);
    ProfSpan span(c, PROF_MISC, s);
    header_read_kernel<<<B, 256, 0, s>>>(a.d_in, (long)a.in_stride, a.d_seg_len, w.d_img, w.planes, w.fplanes, w.mm, w.status);
    if (p.M == 0) {
        const int st0 = first_stage(p.nlev);
        unpack_kernel<<<dim3(LLICTI_NSTREAMS - st0, B), 256, 0, s>>>(a.d_in, (long)a.in_stride, a.d_seg_len, B, w.slots, pd->dev<long>(p.d_slot_off), pd->dev<int32_t>(p.d_slot_cap), w.slot_len, w.status, st0);
    } else {
        const StageGeom *sglv = w.d_sg + (size_t)(0 * 3 + 2) * B;      // the last stage: an xwide v4 tail is at most the stream's share of it
        rans_unpack_kernel<<<NS, 256, 0, s>>>(a.d_in, (long)a.in_stride, a.d_seg_len, w.d_sref, 2 + Q * RansGeo<1>::kPayBytes,
                                              w.slots, w.d_rslot_off, p.rslot_cap, w.rpos, w.status, Q == 4 ? 4 : 2);
        if (Q == 4) rans_init_kernel<4><<<NS, 64, 0, s>>>(w.slots, w.d_rslot_off, w.d_sref, w.rstate, w.rpos, w.rtail, w.status, sglv);
        else if (Q == 2) rans_init_kernel<2><<<NS, 64, 0, s>>>(w.slots, w.d_rslot_off, w.d_sref, w.rstate, w.rpos, w.rtail, w.status, sglv);
        else rans_init_kernel<1><<<NS, 64, 0, s>>>(w.slots, w.d_rslot_off, w.d_sref, w.rstate, w.rpos, w.rtail, w.status, sglv);
    }
    return 0;
}

template <int Q> static void launch_tail(const DecodeBufs &w, const StageGeom *sgv, const LevelRun &lr, hipStream_t s)
{
    rans_tail_kernel<Q><<<lr.NS, tail_threads<Q>, 0, s>>>(w.params, sgv, w.d_sref, w.rstate, w.rpos, w.rtail, w.planes, w.fplanes, w.mm, w.status, w.slots, w.d_rslot_off, lr.act);
}

// One (level, band) of the rANS containers: the three colours' stage in one launch of a workgroup per stream of the level, and behind the last
// stage the tail coder
static void rans_stage(llicti_ctx *c, const Plan &p, const DecodeBufs &w, int lvl, int band, const LevelRun &lr, hipStream_t s)
{
    const int Q = p.Q, NS = lr.NS;
    const StageGeom *sgv = w.d_sg + (size_t)(lvl * 3 + band) * p.B;
    const int last = (lvl == 0 && band == 2) ? 1 : 0;      // the last stage's tail symbols are decoded by rans_tail_kernel
    {
        ProfSpan span(c, PROF_RANS_STAGE, s);
        if (Q == 4) {
            rans_decode_stage_lane_kernel<4><<<NS, 256, 0, s>>>(w.params, sgv, w.d_sref, w.slots, w.d_rslot_off, p.rslot_cap, w.rstate, w.rpos, w.rtail, w.planes, w.fplanes, w.mm, last, w.status, c->d_phi_lut, lr.act);
        } else if (Q == 2) {
            rans_decode_stage_pair_kernel<<<NS, 64 * kRansWaves, 0, s>>>(w.params, sgv, w.d_sref, c->d_phi_lut, w.slots, w.d_rslot_off, p.rslot_cap, w.rstate, w.rpos, w.rtail, w.planes, w.fplanes, w.mm, last, w.status, lr.act);
        } else {
            rans_decode_stage_kernel<<<NS, 64 * kRansWaves, 0, s>>>(w.params, sgv, w.d_sref, c->d_phi_lut, w.slots, w.d_rslot_off, p.rslot_cap, w.rstate, w.rpos, w.rtail, w.planes, w.fplanes, w.mm, last, w.status, lr.act);
        }
    }
    if (last) {
        ProfSpan span(c, PROF_RANS_TAIL, s);
        if (Q == 4) launch_tail<4>(w, sgv, lr, s);
        else if (Q == 2) launch_tail<2>(w, sgv, lr, s);
        else launch_tail<1>(w, sgv, lr, s);
    }
}

// One (level, band) of the reference-format container (equal sizes only; g: every image's geometry): Y, Co, Cg of this band as a pipeline over
// chunks of the stage: chunk c of Co needs only chunk c of Y (mean update from the SAME pixel, LLICTI_nets.py:474-477), chunk c of Cg only chunk
// c of Y and Co.  Three HIP streams; tables are built per chunk into one buffer per colour; the coder state of a stream travels between its
// chunk launches in `acstate`.  The colour queues are joined back onto `s` at the end.
static int ac_stage(llicti_ctx *c, const Plan &p, const DecodeBufs &w, const Geom &g, int lvl, int band, hipStream_t s)
{
    const int B = p.B;
    const StageGeom sg = make_stage(g, band);
    const long nc = (long)sg.hc * sg.wc;
    const int C = ac_chunks(nc);
    const long rows = ac_chunk_rows(nc);
    hipStream_t q[3] = { s, c->sub[1], c->sub[2] };
    if (C > 1) {
        HIPCHK(hipEventRecord(c->ev_ac_band, s));
        HIPCHK(hipStreamWaitEvent(q[1], c->ev_ac_band, 0));
        HIPCHK(hipStreamWaitEvent(q[2], c->ev_ac_band, 0));
    }
    for (int ch = 0; ch < C; ++ch) {
        const long n0 = (long)ch * rows, cnt = std::min(rows, nc - n0);
        for (int clr = 0; clr < 3; ++clr) {
            hipStream_t qs = (C > 1) ? q[clr] : s;
            if (C > 1 && clr > 0) HIPCHK(hipStreamWaitEvent(qs, c->ev_ac[clr - 1][ch], 0));
            ProfSpan span(c, PROF_AC, qs);
            const bool anchors = ac_use_anchors(B, c->ac_anchor_min_batch);
            const int row_stride = (clr == 0) ? 264 : 512;      // full rows: Y has Lp = 257, Co / Cg Lp <= 512
            uint8_t *tab = w.tables + (size_t)clr * B * p.ac_cap_rows * (anchors ? (size_t)kAnchorRow : (size_t)1024);
            if (anchors) { if (int rc = launch_cdf_anchors(w.planes, w.params, w.mm, g, band, clr, tab, n0, cnt, p.ac_cap_rows, qs)) return rc; }
            else if (int rc = launch_cdf_table(w.planes, w.params, w.mm, g, band, clr, (uint16_t *)tab, row_stride, n0, cnt, p.ac_cap_rows, qs)) return rc;
            const int st = stage_index(lvl, band, clr);
            DecOut o;
            memset(&o, 0, sizeof o);
            o.planes = w.planes; o.fplanes = w.fplanes; o.minmax = w.mm; o.sg = sg; o.clr = clr;
            o.len = w.slot_len + (size_t)st * B;
            // the B streams of one stage sit in consecutive slots of equal capacity
            const long in_stride_slots = p.slot_cap[(size_t)st * B];
            AcChunk ck = { (int)n0, (int)cnt, (int)nc, (int)p.ac_cap_rows, w.acstate + (size_t)clr * B * 8 };
            if (anchors) ac_decode_anchor_kernel<<<B, 64, 0, qs>>>(tab, w.slots + p.slot_off[(size_t)st * B], in_stride_slots, ck, o);
            else ac_decode_kernel<<<B, 64, 0, qs>>>((const uint16_t *)tab, 0, row_stride, w.slots + p.slot_off[(size_t)st * B], in_stride_slots, ck, o);
            if (C > 1 && clr < 2) HIPCHK(hipEventRecord(c->ev_ac[clr][ch], qs));
        }
    }
    if (C > 1) {
        for (int k = 1; k < 3; ++k) {
            HIPCHK(hipEventRecord(c->ev_ac_end[k - 1], q[k]));
            HIPCHK(hipStreamWaitEvent(s, c->ev_ac_end[k - 1], 0));
        }
    }
    return 0;
}

// A transcode's tap behind a (level, band): the target plan's pairs from the stage's CNN outputs and symbols (the next band's CNN launch, which
// overwrites `params`, follows on `s`)
static int transcode_tap(llicti_ctx *c, const DecodeBufs &w, const DecodeSink &sink, int B, int lvl, int band, hipStream_t s)
{
    const Plan &q = sink.target->p;
    const int k = lvl * 3 + band;
    ProfSpan span(c, PROF_PAIRS, s);
    cdf_pairs_kernel<<<dim3((unsigned)((q.lev_maxpos[lvl] + kPairsThreads - 1) / kPairsThreads), B), kPairsThreads, 0, s>>>(
        w.planes, w.params, w.mm, q.sg[(size_t)k * B], sink.target->dev<StageGeom>(q.d_sg) + (size_t)k * B,
        (uint32_t *)(sink.target_ws + q.off_pairs) + q.pair_base[k]);
    HIPCHK(hipGetLastError());
    return 0;
}

// 45 dependent stages (LLICTI_nets.py:440-498; 9 L for a model of L levels): CNN of band b needs bands < b of this level, Co needs Y, Cg needs Y, Co
// A reduced decode (run.stop = r >= 1) stops after level r: every pixel whose row and column are multiples of 2^r is final then, and nothing that
// ran reads a finer one.  The whole container has been unpacked by the prologue; the rANS bit region is read downwards from the stream's end and the
// coarse stages come first, so stopping is sound -- but the tail coder (the last stage's) never runs, and with it the end-of-stream check.
static int decode_stages(llicti_ctx *c, PlanDev *pd, const DecodeCall &a, uint8_t *ws, hipStream_t s, const DecodeRun &run, const DecodeSink &sink)
{
    const Plan &p = pd->p;
    const int B = p.B, M = p.M;
    const DecodeBufs w(pd, ws);
    if (int rc = decode_prologue(c, pd, w, a, s)) return rc;
    if (run.rtab && M == 0) return fail(LLICTI_EINVAL, "decode_images: per-image reduces need rANS containers");
    int32_t *cuts = sink.kind == DecodeSink::Cuts ? (int32_t *)sink.d_out : nullptr;
    if (cuts) HIPCHK(hipMemsetAsync(cuts, 0, (size_t)B * kProgMaxStreams * LLICTI_NLEVELS * sizeof(int32_t), s));
    for (int lvl = p.nlev - 1; lvl >= run.stop; --lvl) {
        const Geom &g = p.geo[(size_t)lvl * B];                         // image 0's (equal sizes: every image's)
        const LevelRun &lr = run.lev[lvl];
        if (lr.NS == 0 && M > 0) continue;                              // (no image takes part in the level)
        for (int band = 0; band < 3; ++band) {
            const TileRun *tr = &lr.run[band];
            if (int rc = launch_band_params(c, w.fplanes, g, band, w.params, s, lr.gv, lr.tiles ? lr.tiles + tr->off : nullptr, tr)) return rc;
            if (M > 0) rans_stage(c, p, w, lvl, band, lr, s);
            else if (int rc = ac_stage(c, p, w, g, lvl, band, s)) return rc;
            if (sink.kind == DecodeSink::Transcode) if (int rc = transcode_tap(c, w, sink, B, lvl, band, s)) return rc;
        }
        if (cuts && lvl >= 1) level_cuts_kernel<<<(lr.NS + 255) / 256, 256, 0, s>>>(w.rpos, w.d_sref, lr.NS, lvl, cuts);
    }
    return launch_sink(c, p, w, sink, s, run);
}

// Room for the per-image status words of a call on B images in the context's own copy (llicti_image_status); none are valid until the call has run
static int reserve_img_status(llicti_ctx *c, int B)
{
    c->img_status_n = 0;
    if (c->img_status_cap < B) {          // grows rarely (a larger batch than any before): blocking is fine here
        ++c->n_device_sync; ++c->n_device_alloc;
        HIPCHK(hipDeviceSynchronize());
        if (c->d_img_status) { (void)hipFree(c->d_img_status); c->d_img_status = nullptr; c->img_status_cap = 0; }
        const int cap = std::max(B, 64);
        HIPCHK(hipMalloc(&c->d_img_status, (size_t)cap * sizeof(int32_t)));
        c->img_status_cap = cap;
    }
    return 0;
}

static int decode_batch(llicti_ctx *c, const DecodeCall &a, DecodeSink sink)
{
    const int B = a.B, *Hs = a.Hs, *Ws = a.Ws;
    const Reduces &rd = a.rd;
    const bool own_out = sink.kind == DecodeSink::Views;      // (every group has its own output)
    if (!c || !a.d_in || !a.d_seg_len || !a.d_workspace || (!sink.d_out && !own_out)) return fail(LLICTI_EINVAL, "decode_images: null pointer");
    if (!rd.per_image() && (rd.r < 0 || rd.r > c->nlev)) return fail(LLICTI_EINVAL, "decode_images: reduce = %d (a %d-level model decodes at reduce 0 .. %d)", rd.r, c->nlev, c->nlev);
    if (check_dims_v(B, Hs, Ws)) return LLICTI_EINVAL;
    int ME = 0;
    std::vector<int> Ms;
    if (int rc = resolve_modes("decode_images", a.modes, a.n_modes, B, &ME, Ms)) return rc;
    if (int rc = check_model(c->nlev, "decode_images", ME, Ms)) return rc;
    if (int rc = check_stream_bits("decode_images", c->nlev, B, Hs, Ws, ME, Ms)) return rc;
    if (rd.per_image()) if (int rc = admit_reduces("decode_images", B, rd.rv, c->nlev, ME)) return rc;
    if (int rc = resolve_sink(sink, B, Hs, Ws, rd)) return rc;
    if (int rc = check_source_modes("decode_images", "container", ME)) return rc;
    if (sink.kind == DecodeSink::Cuts && ((ME & 0xFF) == 0 || ((ME >> 8) & 3) != 2))
        return fail(LLICTI_EINVAL, "level_cuts: progressive records hold xwide v4 streams (LLICTI_MODE_RANS_X): a stream of 64 / 128 lanes keeps its T field at its bottom, the reference format has no cursor");
    for (int b = 0; b < 3; ++b) if (!c->have[b]) return fail(LLICTI_ENOWEIGHTS, "band %d weights not set", b);
    DeviceGuard guard(c);
    hipStream_t s = (hipStream_t)a.stream;
    const std::vector<PixGeo> *pix = sink.kind == DecodeSink::Interleaved ? &sink.pix : nullptr;
    PlanDev *pd = nullptr;
    // (an _rv call: the batch's full-size plan with tight placement, whatever the values and the sink -- outputs and windows are per-call tables)
    if (rd.per_image()) { if (int rc = get_plan(c, B, Hs, Ws, nullptr, ME, modes_ptr(Ms), s, &pd)) return rc; }
    else if (int rc = get_plan(c, B, Hs, Ws, a.rgb_off, ME, modes_ptr(Ms), s, &pd, rd.r, pix)) return rc;
    PlanUse use{ pd, s };
    const Plan &p = pd->p;
    if (!p.uniform && p.M == 0) return fail(LLICTI_EINVAL, "decode_images: a batch of mixed sizes needs a rANS container (the reference-format container codes equal sizes per call)");
    if (int rc = check_in_stride("decode_images", p.nlev, B, Hs, Ws, a.in_stride)) return rc;
    if (a.workspace_bytes < p.total)
        return fail(LLICTI_ENOSPACE, "decode_images: workspace %zu < %zu", a.workspace_bytes, p.total);

    if (int rc = reserve_img_status(c, B)) return rc;
    RvCall rv;
    if (rd.per_image()) {      // rgb_off then places the images at their own reduced sizes
        rv.c = c; rv.s = s;
        build_reduce_schedule(rv.q, p, rd.rv, sink.kind == DecodeSink::Planar ? a.rgb_off : nullptr, c->n_cu, c->cnn_tile_rows, pix);
        if (int rc = rv.upload()) return rc;
    }
    CallScope call(c, s);
    if (int rc = decode_stages(c, pd, a, (uint8_t *)a.d_workspace, s, rd.per_image() ? rv_run(pd, rv) : plan_run(pd, rd.r), sink)) return rc;
    c->img_status_n = B;
    return LLICTI_OK;
}

extern "C" int llicti_decode_images_v(llicti_ctx *c, const uint8_t *d_in, size_t in_stride, const int32_t *d_seg_len,
                                      int B, const int *Hs, const int *Ws, int mode, void *d_workspace, size_t workspace_bytes,
                                      uint8_t *d_rgb, const size_t *rgb_off, void *stream)
{
    return decode_batch(c, { d_in, in_stride, d_seg_len, B, Hs, Ws, &mode, 1, d_workspace, workspace_bytes, rgb_off, stream, 0 }, planar_sink(d_rgb));
}

extern "C" int llicti_decode_images_vm(llicti_ctx *c, const uint8_t *d_in, size_t in_stride, const int32_t *d_seg_len,
                                       int B, const int *Hs, const int *Ws, const int *modes, void *d_workspace, size_t workspace_bytes,
                                       uint8_t *d_rgb, const size_t *rgb_off, void *stream)
{
    return decode_batch(c, { d_in, in_stride, d_seg_len, B, Hs, Ws, modes, B, d_workspace, workspace_bytes, rgb_off, stream, 0 }, planar_sink(d_rgb));
}

extern "C" int llicti_level_cuts(llicti_ctx *c, const uint8_t *d_in, size_t in_stride, const int32_t *d_seg_len,
                                 int B, const int *Hs, const int *Ws, const int *modes, void *d_workspace, size_t workspace_bytes,
                                 int32_t *d_cuts, void *stream)
{
    return decode_batch(c, { d_in, in_stride, d_seg_len, B, Hs, Ws, modes, B, d_workspace, workspace_bytes, nullptr, stream, 0 }, cuts_sink(d_cuts));
}

extern "C" int llicti_reduced_dims(int H, int W, int reduce, int *Hr, int *Wr)
{
    if (H < 1 || W < 1 || reduce < 0 || reduce > LLICTI_NLEVELS) return fail(LLICTI_EINVAL, "reduced_dims: H=%d W=%d reduce=%d (need H, W >= 1 and 0 <= reduce <= %d)", H, W, reduce, LLICTI_NLEVELS);
    if (Hr) *Hr = reduced_dim(H, reduce);
    if (Wr) *Wr = reduced_dim(W, reduce);
    return LLICTI_OK;
}

extern "C" int llicti_decode_images_reduced(llicti_ctx *c, const uint8_t *d_in, size_t in_stride, const int32_t *d_seg_len,
                                            int B, const int *Hs, const int *Ws, const int *modes, int n_modes, int reduce,
                                            void *d_workspace, size_t workspace_bytes, uint8_t *d_rgb, const size_t *rgb_off, void *stream)
{
    return decode_batch(c, { d_in, in_stride, d_seg_len, B, Hs, Ws, modes, n_modes, d_workspace, workspace_bytes, rgb_off, stream, reduce }, planar_sink(d_rgb));
}

extern "C" int llicti_pixel_bytes(int format) { return pix_format_bytes(format); }
extern "C" size_t llicti_pixel_span(int format, int H, int W, size_t pitch) { return pix_window_span(format, H, W, pitch); }

extern "C" int llicti_encode_images_px(llicti_ctx *c, const uint8_t *d_pix, int format, const size_t *px_off, const size_t *pitch,
                                       int B, const int *Hs, const int *Ws, const int *modes, void *d_workspace, size_t workspace_bytes,
                                       uint8_t *d_out, size_t out_stride, int32_t *d_seg_len, void *stream)
{
    return encode_batch(c, { PixelSrc::Interleaved, d_pix, { format, px_off, pitch } }, nullptr, B, Hs, Ws, modes, B, d_workspace, workspace_bytes, d_out, out_stride,
                        d_seg_len, stream);
}

extern "C" int llicti_decode_images_px(llicti_ctx *c, const uint8_t *d_in, size_t in_stride, const int32_t *d_seg_len,
                                       int B, const int *Hs, const int *Ws, const int *modes, int n_modes, int reduce,
                                       void *d_workspace, size_t workspace_bytes,
                                       uint8_t *d_pix, int format, const size_t *px_off, const size_t *pitch, void *stream)
{
    return decode_batch(c, { d_in, in_stride, d_seg_len, B, Hs, Ws, modes, n_modes, d_workspace, workspace_bytes, nullptr, stream, reduce },
                        px_sink(d_pix, { format, px_off, pitch }));
}

extern "C" int llicti_tensor_elem_bytes(int dtype) { return tensor_elem_bytes(dtype); }
extern "C" int llicti_tensor_window_ok(int H, int W, int reduce, int y0, int x0, int Ho, int Wo) { return tensor_window_ok(H, W, reduce, y0, x0, Ho, Wo) ? 1 : 0; }

// (the plan: rgb_off = nullptr -- llicti_decode_images_reduced's for the same sizes, modes and reduce with tight placement; the windows are
// kernel arguments, so calls that differ only in them share it)
extern "C" int llicti_decode_images_tensor(llicti_ctx *c, const uint8_t *d_in, size_t in_stride, const int32_t *d_seg_len,
                                           int B, const int *Hs, const int *Ws, const int *modes, int n_modes, int reduce,
                                           void *d_workspace, size_t workspace_bytes,
                                           void *d_out, int dtype, int Ho, int Wo, const int *y0, const int *x0, const uint8_t *flip,
                                           const float *mean, const float *std, void *stream)
{
    return decode_batch(c, { d_in, in_stride, d_seg_len, B, Hs, Ws, modes, n_modes, d_workspace, workspace_bytes, nullptr, stream, reduce },
                        tensor_sink(d_out, { dtype, Ho, Wo, y0, x0, flip, mean, std }));
}

extern "C" int llicti_resize_window_ok(int H, int W, int reduce, int y0, int x0, int hs, int ws, int Ho, int Wo, int antialias)
{
    return resize_window_ok(H, W, reduce, y0, x0, hs, ws, Ho, Wo, antialias) ? 1 : 0;
}
// (the host's compile of resize_axis: the function the resampling kernel calls)
extern "C" int llicti_resize_axis(int n, int m, int antialias, int i, int *lo, float *w, int cap)
{
    if (n < 1 || m < 1 || i < 0 || i >= m || !lo || cap < 0 || (cap > 0 && !w)) return 0;
    return resize_axis(n, m, antialias ? 1 : 0, i, lo, w, cap);
}

// (the plan: llicti_decode_images_tensor's -- boxes, flips, output size and filter flag are kernel arguments)
extern "C" int llicti_decode_images_tensor_resized(llicti_ctx *c, const uint8_t *d_in, size_t in_stride, const int32_t *d_seg_len,
                                                   int B, const int *Hs, const int *Ws, const int *modes, int n_modes, int reduce,
                                                   void *d_workspace, size_t workspace_bytes,
                                                   void *d_out, int dtype, int Ho, int Wo, const int *y0, const int *x0, const int *hs, const int *ws,
                                                   const uint8_t *flip, const float *mean, const float *std, int antialias, void *stream)
{
    return decode_batch(c, { d_in, in_stride, d_seg_len, B, Hs, Ws, modes, n_modes, d_workspace, workspace_bytes, nullptr, stream, reduce },
                        resized_sink(d_out, { dtype, Ho, Wo, y0, x0, hs, ws, flip, mean, std, antialias }));
}

// (the plan: the same one -- image indices, boxes and flips of every view are kernel arguments of the groups' launches)
extern "C" int llicti_decode_images_tensor_views(llicti_ctx *c, const uint8_t *d_in, size_t in_stride, const int32_t *d_seg_len,
                                                 int B, const int *Hs, const int *Ws, const int *modes, int n_modes, int reduce,
                                                 void *d_workspace, size_t workspace_bytes,
                                                 const llicti_view_group *groups, int G, const float *mean, const float *std, void *stream)
{
    return decode_batch(c, { d_in, in_stride, d_seg_len, B, Hs, Ws, modes, n_modes, d_workspace, workspace_bytes, nullptr, stream, reduce },
                        views_sink({ groups, G, mean, std }));
}

// ------------------------------------------------------------------------------------------------ per-image reduce
// The five _rv calls: the scalar sibling with `int reduce` replaced by B host values.  All equal: the call IS the sibling's (the scalar Reduces:
// same launches, plan key and counters).  Otherwise decode_batch runs the per-call schedule (host_plan.hpp: ReduceSchedule).
// -> 0 and *rd, or the refusal of a null array / a value out of range
static int rv_head(llicti_ctx *c, const char *who, int B, const int *reduces, Reduces *rd)
{
    if (!c) return fail(LLICTI_EINVAL, "%s: null ctx", who);
    if (B < 1) return fail(LLICTI_EINVAL, "%s: bad batch: B=%d", who, B);
    if (int rc = admit_reduces(who, B, reduces, c->nlev, 1)) return rc;      // (the container kind is held against the modes in decode_batch)
    *rd = reduces_equal(B, reduces) ? Reduces(reduces[0]) : Reduces::each(reduces);
    return 0;
}

extern "C" int llicti_decode_images_reduced_rv(llicti_ctx *c, const uint8_t *d_in, size_t in_stride, const int32_t *d_seg_len,
                                               int B, const int *Hs, const int *Ws, const int *modes, int n_modes, const int *reduces,
                                               void *d_workspace, size_t workspace_bytes, uint8_t *d_rgb, const size_t *rgb_off, void *stream)
{
    Reduces rd;
    if (int rc = rv_head(c, "decode_images_reduced_rv", B, reduces, &rd)) return rc;
    return decode_batch(c, { d_in, in_stride, d_seg_len, B, Hs, Ws, modes, n_modes, d_workspace, workspace_bytes, rgb_off, stream, rd }, planar_sink(d_rgb));
}

extern "C" int llicti_decode_images_px_rv(llicti_ctx *c, const uint8_t *d_in, size_t in_stride, const int32_t *d_seg_len,
                                          int B, const int *Hs, const int *Ws, const int *modes, int n_modes, const int *reduces,
                                          void *d_workspace, size_t workspace_bytes,
                                          uint8_t *d_pix, int format, const size_t *px_off, const size_t *pitch, void *stream)
{
    Reduces rd;
    if (int rc = rv_head(c, "decode_images_px_rv", B, reduces, &rd)) return rc;
    return decode_batch(c, { d_in, in_stride, d_seg_len, B, Hs, Ws, modes, n_modes, d_workspace, workspace_bytes, nullptr, stream, rd },
                        px_sink(d_pix, { format, px_off, pitch }));
}

extern "C" int llicti_decode_images_tensor_rv(llicti_ctx *c, const uint8_t *d_in, size_t in_stride, const int32_t *d_seg_len,
                                              int B, const int *Hs, const int *Ws, const int *modes, int n_modes, const int *reduces,
                                              void *d_workspace, size_t workspace_bytes,
                                              void *d_out, int dtype, int Ho, int Wo, const int *y0, const int *x0, const uint8_t *flip,
                                              const float *mean, const float *std, void *stream)
{
    Reduces rd;
    if (int rc = rv_head(c, "decode_images_tensor_rv", B, reduces, &rd)) return rc;
    return decode_batch(c, { d_in, in_stride, d_seg_len, B, Hs, Ws, modes, n_modes, d_workspace, workspace_bytes, nullptr, stream, rd },
                        tensor_sink(d_out, { dtype, Ho, Wo, y0, x0, flip, mean, std }));
}

extern "C" int llicti_decode_images_tensor_resized_rv(llicti_ctx *c, const uint8_t *d_in, size_t in_stride, const int32_t *d_seg_len,
                                                      int B, const int *Hs, const int *Ws, const int *modes, int n_modes, const int *reduces,
                                                      void *d_workspace, size_t workspace_bytes,
                                                      void *d_out, int dtype, int Ho, int Wo, const int *y0, const int *x0, const int *hs, const int *ws,
                                                      const uint8_t *flip, const float *mean, const float *std, int antialias, void *stream)
{
    Reduces rd;
    if (int rc = rv_head(c, "decode_images_tensor_resized_rv", B, reduces, &rd)) return rc;
    return decode_batch(c, { d_in, in_stride, d_seg_len, B, Hs, Ws, modes, n_modes, d_workspace, workspace_bytes, nullptr, stream, rd },
                        resized_sink(d_out, { dtype, Ho, Wo, y0, x0, hs, ws, flip, mean, std, antialias }));
}

extern "C" int llicti_decode_images_tensor_views_rv(llicti_ctx *c, const uint8_t *d_in, size_t in_stride, const int32_t *d_seg_len,
                                                    int B, const int *Hs, const int *Ws, const int *modes, int n_modes, const int *reduces,
                                                    void *d_workspace, size_t workspace_bytes,
                                                    const llicti_view_group *groups, int G, const float *mean, const float *std, void *stream)
{
    Reduces rd;
    if (int rc = rv_head(c, "decode_images_tensor_views_rv", B, reduces, &rd)) return rc;
    return decode_batch(c, { d_in, in_stride, d_seg_len, B, Hs, Ws, modes, n_modes, d_workspace, workspace_bytes, nullptr, stream, rd },
                        views_sink({ groups, G, mean, std }));
}

// ------------------------------------------------------------------------------------------------ tensor options
// The three _o calls: the _rv sibling with a trailing `opts`.  NULL or { NCHW, PAD_NONE }: the call IS the sibling's (with_opts leaves the sink
// as it is).  Otherwise the same decode with the sink_* kernels at its end -- the plan, its key and the per-call tables do not depend on opts.
extern "C" int llicti_pad_index(int n, int t, int mode)
{
    if (n < 1 || n > 8160 || t < -(1 << 20) || t > (1 << 20) || mode < LLICTI_PAD_NONE || mode > LLICTI_PAD_SYMMETRIC) return -2;
    return pad_index(n, t, mode);
}
extern "C" int llicti_tensor_window_pad_ok(int H, int W, int reduce, int y0, int x0, int Ho, int Wo, int mode)
{
    return tensor_window_pad_ok(H, W, reduce, y0, x0, Ho, Wo, mode) ? 1 : 0;
}

extern "C" int llicti_decode_images_tensor_o(llicti_ctx *c, const uint8_t *d_in, size_t in_stride, const int32_t *d_seg_len,
                                             int B, const int *Hs, const int *Ws, const int *modes, int n_modes, const int *reduces,
                                             void *d_workspace, size_t workspace_bytes,
                                             void *d_out, int dtype, int Ho, int Wo, const int *y0, const int *x0, const uint8_t *flip,
                                             const float *mean, const float *std, void *stream, const llicti_tensor_opts *opts)
{
    Reduces rd;
    if (int rc = rv_head(c, "decode_images_tensor_o", B, reduces, &rd)) return rc;
    return decode_batch(c, { d_in, in_stride, d_seg_len, B, Hs, Ws, modes, n_modes, d_workspace, workspace_bytes, nullptr, stream, rd },
                        with_opts(tensor_sink(d_out, { dtype, Ho, Wo, y0, x0, flip, mean, std }), opts));
}

extern "C" int llicti_decode_images_tensor_resized_o(llicti_ctx *c, const uint8_t *d_in, size_t in_stride, const int32_t *d_seg_len,
                                                     int B, const int *Hs, const int *Ws, const int *modes, int n_modes, const int *reduces,
                                                     void *d_workspace, size_t workspace_bytes,
                                                     void *d_out, int dtype, int Ho, int Wo, const int *y0, const int *x0, const int *hs, const int *ws,
                                                     const uint8_t *flip, const float *mean, const float *std, int antialias, void *stream,
                                                     const llicti_tensor_opts *opts)
{
    Reduces rd;
    if (int rc = rv_head(c, "decode_images_tensor_resized_o", B, reduces, &rd)) return rc;
    return decode_batch(c, { d_in, in_stride, d_seg_len, B, Hs, Ws, modes, n_modes, d_workspace, workspace_bytes, nullptr, stream, rd },
                        with_opts(resized_sink(d_out, { dtype, Ho, Wo, y0, x0, hs, ws, flip, mean, std, antialias }), opts));
}

extern "C" int llicti_decode_images_tensor_views_o(llicti_ctx *c, const uint8_t *d_in, size_t in_stride, const int32_t *d_seg_len,
                                                   int B, const int *Hs, const int *Ws, const int *modes, int n_modes, const int *reduces,
                                                   void *d_workspace, size_t workspace_bytes,
                                                   const llicti_view_group *groups, int G, const float *mean, const float *std, void *stream,
                                                   const llicti_tensor_opts *opts)
{
    Reduces rd;
    if (int rc = rv_head(c, "decode_images_tensor_views_o", B, reduces, &rd)) return rc;
    return decode_batch(c, { d_in, in_stride, d_seg_len, B, Hs, Ws, modes, n_modes, d_workspace, workspace_bytes, nullptr, stream, rd },
                        with_opts(views_sink({ groups, G, mean, std }), opts));
}

extern "C" int llicti_encode_images_f32(llicti_ctx *c, const float *d_x, const size_t *x_off, int B, const int *Hs, const int *Ws, const int *modes,
                                        void *d_workspace, size_t workspace_bytes,
                                        uint8_t *d_out, size_t out_stride, int32_t *d_seg_len, void *stream)
{
    return encode_batch(c, { PixelSrc::PlanarF32, d_x, {} }, x_off, B, Hs, Ws, modes, B, d_workspace, workspace_bytes, d_out, out_stride, d_seg_len, stream);
}

extern "C" int llicti_decode_images(llicti_ctx *c, const uint8_t *d_in, size_t in_stride, const int32_t *d_seg_len,
                                    int B, int H, int W, int mode, void *d_workspace, size_t workspace_bytes,
                                    uint8_t *d_rgb, void *stream)
{
    if (check_dims(B, H, W)) return LLICTI_EINVAL;
    std::vector<int> Hs(B, H), Ws(B, W);
    return decode_batch(c, { d_in, in_stride, d_seg_len, B, Hs.data(), Ws.data(), &mode, 1, d_workspace, workspace_bytes, nullptr, stream, 0 }, planar_sink(d_rgb));
}

// ------------------------------------------------------------------------------------------------ transcode
// total and max_container of the plan a call on (sizes, ME, Ms) would use: the cached plan's, or a host-only build -- so that a call can refuse
// a short workspace before it takes a plan (a new plan's tables are uploaded, and may allocate a block)
static void plan_need(llicti_ctx *c, int B, const int *Hs, const int *Ws, int ME, const int *Ms, size_t *total, size_t *max_container)
{
    const PlanSpec sp = ctx_spec(c, B, Hs, Ws, nullptr, ME, Ms);
    auto it = c->plans.find(plan_key(sp));
    if (it != c->plans.end()) { *total = it->second->p.total; *max_container = it->second->p.max_container; return; }
    Plan p;
    build_plan(p, sp);
    *total = p.total; *max_container = p.max_container;
}

extern "C" size_t llicti_transcode_workspace_bytes(const llicti_ctx *c, int B, const int *Hs, const int *Ws, const int *src_modes, int n_src,
                                                   const int *dst_modes, int n_dst)
{
    return plan_transcode_workspace_bytes(B, Hs, Ws, src_modes, n_src, dst_modes, n_dst, c ? c->nlev : LLICTI_NLEVELS);
}

extern "C" int llicti_transcode_images(llicti_ctx *c, const uint8_t *d_in, size_t in_stride, const int32_t *d_seg_len_in,
                                       int B, const int *Hs, const int *Ws, const int *src_modes, int n_src, const int *dst_modes, int n_dst,
                                       void *d_workspace, size_t workspace_bytes, uint8_t *d_out, size_t out_stride, int32_t *d_seg_len_out, void *stream)
{
    if (!c || !d_in || !d_seg_len_in || !d_workspace || !d_out || !d_seg_len_out) return fail(LLICTI_EINVAL, "transcode_images: null pointer");
    int MEs = 0, MEd = 0;
    std::vector<int> Mss, Msd;
    if (int rc = admit_transcode(c->nlev, c->force_ragged != 0, B, Hs, Ws, src_modes, n_src, dst_modes, n_dst, &MEs, Mss, &MEd, Msd)) return rc;
    if (int rc = check_in_stride("transcode_images", c->nlev, B, Hs, Ws, in_stride)) return rc;
    {
        const uintptr_t i0 = (uintptr_t)d_in, i1 = i0 + (size_t)B * in_stride, o0 = (uintptr_t)d_out, o1 = o0 + (size_t)B * out_stride;
        if (i0 < o1 && o0 < i1) return fail(LLICTI_EINVAL, "transcode_images: d_out overlaps d_in");
    }
    for (int b = 0; b < 3; ++b) if (!c->have[b]) return fail(LLICTI_ENOWEIGHTS, "band %d weights not set", b);
    DeviceGuard guard(c);
    hipStream_t s = (hipStream_t)stream;
    const int *ms_src = modes_ptr(Mss), *ms_dst = modes_ptr(Msd);
    {
        size_t tot_s = 0, tot_d = 0, mc_s = 0, mc_d = 0;
        plan_need(c, B, Hs, Ws, MEs, ms_src, &tot_s, &mc_s);
        plan_need(c, B, Hs, Ws, MEd, ms_dst, &tot_d, &mc_d);
        const size_t need = align_up(tot_s, 256) + tot_d;
        if (workspace_bytes < need) return fail(LLICTI_ENOSPACE, "transcode_images: workspace %zu < %zu", workspace_bytes, need);
        if (out_stride < mc_d) return fail(LLICTI_ENOSPACE, "transcode_images: out_stride %zu < %zu", out_stride, mc_d);
    }
    PlanDev *pds = nullptr, *pdd = nullptr;
    if (int rc = get_plan(c, B, Hs, Ws, nullptr, MEs, ms_src, s, &pds)) return rc;
    PlanUse use_src{ pds, s };
    if (int rc = get_plan(c, B, Hs, Ws, nullptr, MEd, ms_dst, s, &pdd)) return rc;      // (the source plan is the most recently used one: it stays cached)
    PlanUse use_dst{ pdd, s };
    const Plan &ps = pds->p, &pt = pdd->p;
    if (!transcode_plans_agree(ps, pt)) return fail(LLICTI_EINVAL, "transcode_images: the two plans place the planes differently");
    const TranscodeLayout lay = transcode_layout(ps, pt);
    if (workspace_bytes < lay.total) return fail(LLICTI_ENOSPACE, "transcode_images: workspace %zu < %zu", workspace_bytes, lay.total);
    uint8_t *ws = (uint8_t *)d_workspace;
    DecodeSink tc;
    tc.kind = DecodeSink::Transcode; tc.target = pdd; tc.target_ws = ws + lay.off_dst;
    const DecodeCall src{ d_in, in_stride, d_seg_len_in, B, Hs, Ws, src_modes, n_src, d_workspace, workspace_bytes, nullptr, stream, 0 };

    if (int rc = reserve_img_status(c, B)) return rc;
    CallScope call(c, s);
    if (int rc = decode_stages(c, pds, src, ws, s, plan_run(pds, 0), tc)) return rc;
    const int16_t *planes = (const int16_t *)(ws + ps.off_planes);
    const int32_t *mm = (const int32_t *)(ws + ps.off_minmax);
    int32_t *status_dst = (int32_t *)(tc.target_ws + pt.off_status);
    {
        ProfSpan span(c, PROF_MISC, s);
        unsigned long long *ssum0 = (pt.ME & 0x1000) ? (unsigned long long *)(tc.target_ws + pt.off_rpos) : nullptr;
        header_transcode_kernel<<<B, 256, 0, s>>>(planes, mm, pdd->dev<ImgGeo>(pt.d_img), d_out, (long)out_stride, d_seg_len_out, ssum0, status_dst, kStatusHead + B);
    }
    if (int rc = encode_back_end(c, pdd, tc.target_ws, planes, mm, d_out, out_stride, d_seg_len_out, s)) return rc;
    {
        ProfSpan span(c, PROF_MISC, s);
        transcode_latch_kernel<<<(B * LLICTI_NSEG + 255) / 256, 256, 0, s>>>((const int32_t *)(ws + ps.off_status), status_dst, c->d_status, c->d_img_status, B, d_seg_len_out);
    }
    HIPCHK(hipGetLastError());
    c->img_status_n = B;
    return LLICTI_OK;
}

// ------------------------------------------------------------------------------------------------ pixel digests
extern "C" uint32_t llicti_crc32_combine(uint32_t crc_a, uint32_t crc_b, uint64_t len_b) { return crc32_combine(crc_a, crc_b, len_b); }
extern "C" int llicti_crc32_geometry(int *lane_pixels, int *group_pixels)
{
    if (lane_pixels) *lane_pixels = kCrcLanePixels;
    if (group_pixels) *group_pixels = kCrcGroupPixels;
    return LLICTI_OK;
}

// The two digest kernels over B images: contiguous planes of `plane` pixels (iv == nullptr), or a call's table.  max_plane sizes the grid; the
// images go in slices whose partials fit the context's scratch (one slice unless B x groups exceeds kCrcMaxParts).
static int launch_crc(llicti_ctx *c, const int16_t *planes, long plane, const ImgGeo *iv, long max_plane, int B, const int32_t *d_flags,
                      uint32_t *d_crc, int32_t *d_have, hipStream_t s)
{
    const int gx = (int)((max_plane + kCrcGroupPixels - 1) / kCrcGroupPixels);
    const int slice = std::max(1, std::min(kCrcMaxParts / gx, 65535));
    for (int b0 = 0; b0 < B; b0 += slice) {
        const int nb = std::min(slice, B - b0);
        crc_planes_kernel<<<dim3(gx, nb), kCrcThreads, kCrcLdsBytes, s>>>(planes, plane, iv, d_flags, b0, c->d_crc_tab, c->d_crc_part);
        crc_fold_kernel<<<nb, kCrcThreads, 0, s>>>(c->d_crc_part, gx, plane, iv, d_flags, b0, c->d_crc_tab, d_crc, d_have);
    }
    HIPCHK(hipGetLastError());
    return 0;
}

extern "C" int llicti_crc32_planes(llicti_ctx *c, const int16_t *d_planes, int B, int H, int W, uint32_t *d_crc, void *stream)
{
    if (!c || !d_planes || !d_crc) return fail(LLICTI_EINVAL, "crc32_planes: null pointer");
    if (B < 1 || H < 1 || W < 1 || H > 8160 || W > 8160) return fail(LLICTI_EINVAL, "crc32_planes: bad shape B=%d H=%d W=%d (need B>=1, 1<=H,W<=8160)", B, H, W);
    DeviceGuard guard(c);
    return launch_crc(c, d_planes, (long)H * W, nullptr, (long)H * W, B, nullptr, d_crc, nullptr, (hipStream_t)stream);
}

// The plan the PRECEDING whole-batch call of this batch shape ran on: the most recently used cached plan of these sizes and modes, whatever its
// placement, reduce or pixel windows (their key tails follow the full-size key; the caller's RGB offsets are skipped) -- all of them carve the
// workspace's planes from the sizes alone.  nullptr: none is cached.
static PlanDev *find_batch_plan(llicti_ctx *c, const PlanSpec &sp)
{
    const std::vector<long> key = plan_key(sp);
    PlanDev *best = nullptr;
    for (auto &kv : c->plans) {
        const std::vector<long> &k = kv.first;
        if (k.size() < key.size()) continue;
        bool same = true;
        for (size_t i = 0; i < key.size() && same; ++i) same = (i >= 3 && (i - 3) % 4 == 2) || k[i] == key[i];
        if (same && (!best || kv.second->last_use > best->last_use)) best = kv.second;
    }
    return best;
}

extern "C" int llicti_digest_images(llicti_ctx *c, int B, const int *Hs, const int *Ws, const int *modes, int n_modes, const int *reduce,
                                    const void *d_workspace, size_t workspace_bytes, uint32_t *d_crc, int32_t *d_have, void *stream)
{
    if (!c || !d_workspace || !d_crc || !d_have) return fail(LLICTI_EINVAL, "digest_images: null pointer");
    if (check_dims_v(B, Hs, Ws)) return LLICTI_EINVAL;
    int ME = 0;
    std::vector<int> Ms;
    if (int rc = resolve_modes("digest_images", modes, n_modes, B, &ME, Ms)) return rc;
    bool any_reduced = false;
    for (int b = 0; reduce && b < B; ++b) {
        if (reduce[b] < 0 || reduce[b] > c->nlev) return fail(LLICTI_EINVAL, "digest_images: image %d: reduce = %d (a %d-level model decodes at reduce 0 .. %d)", b, reduce[b], c->nlev, c->nlev);
        any_reduced = any_reduced || reduce[b] != 0;
    }
    PlanDev *pd = find_batch_plan(c, ctx_spec(c, B, Hs, Ws, nullptr, ME, modes_ptr(Ms)));
    if (!pd) return fail(LLICTI_EINVAL, "digest_images: no plan is cached for this batch of %d images and these modes: the call follows a whole-batch encode or decode of the same batch", B);
    const Plan &p = pd->p;
    if (workspace_bytes < p.total) return fail(LLICTI_EINVAL, "digest_images: workspace %zu < %zu, the size of the call this one follows", workspace_bytes, p.total);
    DeviceGuard guard(c);
    hipStream_t s = (hipStream_t)stream;
    pd->last_use = ++c->use_clock;
    if (pd->blk.up_stream != s) HIPCHK(hipStreamWaitEvent(s, pd->blk.uploaded, 0));
    if (pd->blk.used && pd->blk.done_stream != s) HIPCHK(hipStreamWaitEvent(s, pd->blk.done, 0));
    PlanUse use{ pd, s };
    // the flags of a call with reduced images: a per-call table in a pooled block, as the _rv decodes upload theirs
    PlanBlock fb;
    const int32_t *d_flags = nullptr;
    if (any_reduced) {
        if (int rc = acquire_block(c, (size_t)B * sizeof(int32_t), &fb)) return rc;
        int32_t *h = (int32_t *)fb.host;
        for (int b = 0; b < B; ++b) h[b] = reduce[b] == 0 ? 1 : 0;
        if (hipMemcpyAsync(fb.dev, fb.host, (size_t)B * sizeof(int32_t), hipMemcpyHostToDevice, s) != hipSuccess) {
            c->pool.push_back(fb);
            return fail(LLICTI_EHIP, "digest_images: upload failed");
        }
        d_flags = (const int32_t *)fb.dev;
    }
    const int rc = launch_crc(c, (const int16_t *)((const uint8_t *)d_workspace + p.off_planes), 0, pd->dev<ImgGeo>(p.d_img), p.max_plane, B, d_flags, d_crc, d_have, s);
    if (any_reduced) {
        if (hipEventRecord(fb.done, s) == hipSuccess) { fb.used = true; fb.done_stream = s; }
        c->pool.push_back(fb);
    }
    return rc;
}

// ------------------------------------------------------------------------------------------------ records
extern "C" size_t llicti_record_bytes(const llicti_ctx *c, const int32_t *h_seg_len)
{
    return llicti_record_bytes_n(c ? 4 + 9 * c->nlev : LLICTI_NSEG, h_seg_len);      // (no context: config A, as the size queries)
}
extern "C" size_t llicti_record_bytes_n(int n, const int32_t *h_seg_len)
{
    if (!h_seg_len || (n != LLICTI_NSEG && n != 4 + 9 * kLevelsB)) return 0;
    size_t tot = (size_t)record_header_bytes(n);
    for (int k = 0; k < n; ++k) {
        if (h_seg_len[k] < 0) return 0;
        tot += (size_t)h_seg_len[k];
    }
    return tot;
}

constexpr int kRecMaxBatch = 1 << 20;
// One buffer of a record call; a record call's buffers are pairwise disjoint (include/llicti_hip.h)
struct RecordBuf { const void *p; size_t bytes; const char *name; };
// What the four record calls have in hand once record_call has admitted them: the model's segment count, the stream, the grid of the copy
// kernel (x walks the chunks of the longest dense run the call can hold, y the images), the context's device made current until the call returns
struct RecordCall { int n; hipStream_t s; dim3 grid; std::optional<DeviceGuard> guard; };

// Everything the four record calls do before their launches: refuse a null pointer, a batch, stride or blob out of range, any two buffers that
// overlap, more chunks than a grid holds (max_dense: the longest run of bytes one image can move); then make room for the B status words.
static int record_call(RecordCall &rc, const char *who, llicti_ctx *c, int B, size_t stride, size_t blob_bytes, size_t max_dense,
                       std::initializer_list<RecordBuf> bufs, void *stream)
{
    if (!c) return fail(LLICTI_EINVAL, "%s: null pointer", who);
    for (const RecordBuf &u : bufs) if (!u.p) return fail(LLICTI_EINVAL, "%s: null pointer", who);
    if (B < 1 || B > kRecMaxBatch) return fail(LLICTI_EINVAL, "%s: B=%d (need 1 <= B <= %d)", who, B, kRecMaxBatch);
    if (stride < 1 || stride > ((size_t)1 << 62) / (size_t)B) return fail(LLICTI_EINVAL, "%s: stride %zu", who, stride);
    if (blob_bytes > ((size_t)1 << 62)) return fail(LLICTI_EINVAL, "%s: a blob of %zu bytes", who, blob_bytes);
    for (const RecordBuf *u = bufs.begin(); u != bufs.end(); ++u)
        for (const RecordBuf *v = u + 1; v != bufs.end(); ++v) {
            const uintptr_t u0 = (uintptr_t)u->p, v0 = (uintptr_t)v->p;
            if (u0 < v0 + v->bytes && v0 < u0 + u->bytes) return fail(LLICTI_EINVAL, "%s: %s overlaps %s", who, u->name, v->name);
        }
    const size_t chunks = std::max<size_t>(1, (max_dense + kRecChunk - 1) / kRecChunk);
    if (chunks > 0x7FFFFFFFu) return fail(LLICTI_EINVAL, "%s: stride %zu", who, stride);
    rc.n = 4 + 9 * c->nlev;
    rc.s = (hipStream_t)stream;
    rc.grid = dim3((unsigned)chunks, (unsigned)std::min(B, 65535));
    rc.guard.emplace(c);
    return reserve_img_status(c, B);
}
// ... and behind them
static int record_call_end(llicti_ctx *c, int B)
{
    HIPCHK(hipGetLastError());
    c->img_status_n = B;
    return LLICTI_OK;
}
// the sizes of a call's per-image buffers
static size_t seg_len_bytes(int B) { return (size_t)B * LLICTI_NSEG * sizeof(int32_t); }
static size_t rec_off_bytes(int B) { return ((size_t)B + 1) * sizeof(int64_t); }

extern "C" int llicti_pack_records(llicti_ctx *c, const uint8_t *d_cont, size_t stride, const int32_t *d_seg_len, int B,
                                   uint8_t *d_blob, size_t blob_cap, int64_t *d_rec_off, void *stream)
{
    RecordCall rc;
    if (int e = record_call(rc, "pack_records", c, B, stride, blob_cap, stride, { { d_blob, blob_cap, "the blob" }, { d_cont, (size_t)B * stride, "the containers" },
                            { d_seg_len, seg_len_bytes(B), "the segment lengths" }, { d_rec_off, rec_off_bytes(B), "the record offsets" } }, stream)) return e;
    record_offsets_kernel<<<1, kRecThreads, 0, rc.s>>>(RecordSizeOfLengths{ d_seg_len, rc.n, (long)stride, c->d_img_status }, B, (long)blob_cap,
                                                       d_rec_off, c->d_status);
    record_pack_kernel<<<rc.grid, kRecThreads, 0, rc.s>>>(d_cont, (long)stride, d_seg_len, B, rc.n, d_blob, (long)blob_cap, d_rec_off);
    return record_call_end(c, B);
}

extern "C" int llicti_unpack_records(llicti_ctx *c, const uint8_t *d_blob, size_t blob_bytes, const int64_t *d_rec_off, int B,
                                     uint8_t *d_cont, size_t stride, int32_t *d_seg_len, void *stream)
{
    RecordCall rc;
    if (int e = record_call(rc, "unpack_records", c, B, stride, blob_bytes, std::min(stride, blob_bytes), { { d_blob, blob_bytes, "the blob" },
                            { d_cont, (size_t)B * stride, "the containers" }, { d_seg_len, seg_len_bytes(B), "the segment lengths" },
                            { d_rec_off, rec_off_bytes(B), "the record offsets" } }, stream)) return e;
    record_check_kernel<<<B, 64, 0, rc.s>>>(d_blob, (long)blob_bytes, d_rec_off, rc.n, (long)stride, d_seg_len, c->d_status, c->d_img_status);
    record_unpack_kernel<<<rc.grid, kRecThreads, 0, rc.s>>>(d_blob, (long)blob_bytes, d_rec_off, B, rc.n, d_cont, (long)stride, c->d_img_status);
    return record_call_end(c, B);
}

// ------------------------------------------------------------------------------------------------ progressive records
extern "C" int llicti_progressive_prefix(const uint8_t *head, size_t bytes, int64_t *prefix)
{
    if (!head || !prefix) return fail(LLICTI_EINVAL, "progressive_prefix: null pointer");
    ProgHead h;
    if (!prog_check(head, (long)std::min<size_t>(bytes, (size_t)1 << 62), 0, 0, -1, &h, prefix))
        return fail(LLICTI_EFORMAT, "progressive_prefix: not the head of a progressive record (magic, version, model, stream count, a length of 2^31 or more, "
                    "streams that overlap or leave the payload, cuts that do not ascend within their stream, or fewer bytes than the table)");
    return LLICTI_OK;
}

extern "C" int llicti_pack_progressive(llicti_ctx *c, const uint8_t *d_cont, size_t stride, const int32_t *d_seg_len, int B, const int32_t *d_cuts,
                                       uint8_t *d_blob, size_t blob_cap, int64_t *d_rec_off, int64_t *d_prefix, void *stream)
{
    RecordCall rc;
    if (int e = record_call(rc, "pack_progressive", c, B, stride, blob_cap, stride, { { d_blob, blob_cap, "the blob" }, { d_cont, (size_t)B * stride, "the containers" },
                            { d_seg_len, seg_len_bytes(B), "the segment lengths" }, { d_rec_off, rec_off_bytes(B), "the record offsets" },
                            { d_cuts, (size_t)B * kProgMaxStreams * LLICTI_NLEVELS * sizeof(int32_t), "the cuts" },
                            { d_prefix, (size_t)B * (LLICTI_NLEVELS + 1) * sizeof(int64_t), "the prefix table" } }, stream)) return e;
    prog_measure_kernel<<<B, kProgThreads, 0, rc.s>>>(d_cont, (long)stride, d_seg_len, rc.n, c->nlev, d_cuts, d_prefix, c->d_status, c->d_img_status);
    record_offsets_kernel<<<1, kRecThreads, 0, rc.s>>>(RecordSizeOfPrefix{ d_prefix }, B, (long)blob_cap, d_rec_off, c->d_status);
    prog_head_kernel<<<B, kProgThreads, 0, rc.s>>>(d_cont, (long)stride, d_seg_len, rc.n, c->nlev, d_cuts, d_blob, (long)blob_cap, d_rec_off);
    ProgReduces none;
    memset(&none, 0, sizeof none);
    prog_copy_kernel<true><<<rc.grid, kRecThreads, 0, rc.s>>>(d_blob, (long)blob_cap, d_rec_off, 0, B, none, const_cast<uint8_t *>(d_cont), (long)stride, c->d_img_status);
    return record_call_end(c, B);
}

extern "C" int llicti_unpack_progressive(llicti_ctx *c, const uint8_t *d_blob, size_t blob_bytes, const int64_t *d_rec_off, int B, const int *reduce,
                                         uint8_t *d_cont, size_t stride, int32_t *d_seg_len, void *stream)
{
    if (!reduce) return fail(LLICTI_EINVAL, "unpack_progressive: null pointer");
    RecordCall rc;
    if (int e = record_call(rc, "unpack_progressive", c, B, stride, blob_bytes, std::min(stride, blob_bytes), { { d_blob, blob_bytes, "the blob" },
                            { d_cont, (size_t)B * stride, "the containers" }, { d_seg_len, seg_len_bytes(B), "the segment lengths" },
                            { d_rec_off, rec_off_bytes(B), "the record offsets" } }, stream)) return e;
    // the reduces are kernel arguments, kProgReduceMax images a launch (a value outside 0 .. 15 travels as 15: the device check refuses it)
    for (int b0 = 0; b0 < B; b0 += kProgReduceMax) {
        const int nb = std::min(kProgReduceMax, B - b0);
        ProgReduces red;
        memset(&red, 0, sizeof red);
        for (int i = 0; i < nb; ++i) red.w[i >> 3] |= (uint32_t)((reduce[b0 + i] < 0 || reduce[b0 + i] > 15) ? 15 : reduce[b0 + i]) << (4 * (i & 7));
        prog_check_kernel<<<nb, kProgThreads, 0, rc.s>>>(d_blob, (long)blob_bytes, d_rec_off, b0, rc.n, c->nlev, red, (long)stride, d_seg_len, c->d_status, c->d_img_status);
        prog_copy_kernel<false><<<dim3(rc.grid.x, (unsigned)nb), kRecThreads, 0, rc.s>>>(const_cast<uint8_t *>(d_blob), (long)blob_bytes, d_rec_off, b0, b0 + nb, red,
                                                                                         d_cont, (long)stride, c->d_img_status);
    }
    return record_call_end(c, B);
}

extern "C" int llicti_check_status(llicti_ctx *c, void *stream)
{
    if (!c) return fail(LLICTI_EINVAL, "null ctx");
    DeviceGuard guard(c);
    // read and cleared ON `stream`: a synchronous hipMemcpy / hipMemset runs on the null stream and waits for whatever the caller has in flight
    // there (a caller that keeps the codec on a side stream next to a busy default stream; tests/test_hip_streams.py)
    hipStream_t s = (hipStream_t)stream;
    int32_t st = 0;
    HIPCHK(hipMemcpyAsync(&st, c->d_status, 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemsetAsync(c->d_status, 0, 4, s));
    HIPCHK(hipStreamSynchronize(s));
    if (st == LLICTI_EFORMAT) return fail(LLICTI_EFORMAT, "malformed container (header does not match the requested shape, or a stream is too long)");
    if (st == LLICTI_ENOSPACE) return fail(LLICTI_ENOSPACE, "output buffer too small for the encoded streams (or the blob for the packed records)");
    if (st != 0) return fail(st, "device-side status %d", st);
    return LLICTI_OK;
}

extern "C" int llicti_last_timing(llicti_ctx *c, float ms[4], int *n_launch)
{
    if (!c || !ms) return fail(LLICTI_EINVAL, "last_timing: null pointer");
    DeviceGuard guard(c);
    if (c->timing_pending) {
        HIPCHK(hipEventSynchronize(c->ev_call[1]));
        float t = 0;
        HIPCHK(hipEventElapsedTime(&t, c->ev_call[0], c->ev_call[1]));
        c->last_ms[0] = t;
        for (int k = 0; k < PROF_NCAT; ++k) c->last_cat_ms[k] = 0;
        c->last_cnn_ms.clear();
        for (int l = 0; l < LLICTI_NLEVELS; ++l) c->last_cnn_level_ms[l] = 0;
        for (const llicti_ctx::Span &sp : c->spans) {
            float k = 0;
            HIPCHK(hipEventSynchronize(sp.e1));       // spans of the AC decode pipeline sit on the internal streams
            HIPCHK(hipEventElapsedTime(&k, sp.e0, sp.e1));
            c->last_cat_ms[sp.cat] += k;
            if (sp.cat == PROF_CNN) { c->last_cnn_ms.push_back(k); if (sp.tag >= 0 && sp.tag < LLICTI_NLEVELS) c->last_cnn_level_ms[sp.tag] += k; }
        }
        c->last_ms[1] = c->last_cat_ms[PROF_CNN];
        c->last_launches = (int)c->last_cnn_ms.size();
        c->timing_pending = false;
    }
    for (int i = 0; i < 4; ++i) ms[i] = c->last_ms[i];
    if (n_launch) *n_launch = c->last_launches;
    return LLICTI_OK;
}

extern "C" int llicti_last_timing_detail(llicti_ctx *c, float cat_ms[LLICTI_NPROF], float *cnn_launch_ms, int cnn_cap, int *n_cnn)
{
    if (!c || !cat_ms) return fail(LLICTI_EINVAL, "last_timing_detail: null pointer");
    float ms[4];
    if (int rc = llicti_last_timing(c, ms, nullptr)) return rc;
    for (int k = 0; k < LLICTI_NPROF; ++k) cat_ms[k] = c->last_cat_ms[k];
    const int n = (int)c->last_cnn_ms.size();
    if (cnn_launch_ms) for (int i = 0; i < std::min(n, cnn_cap); ++i) cnn_launch_ms[i] = c->last_cnn_ms[i];
    if (n_cnn) *n_cnn = n;
    return LLICTI_OK;
}

extern "C" int llicti_last_cnn_level_ms(llicti_ctx *c, float level_ms[LLICTI_NLEVELS])
{
    if (!c || !level_ms) return fail(LLICTI_EINVAL, "last_cnn_level_ms: null pointer");
    float ms[4];
    if (int rc = llicti_last_timing(c, ms, nullptr)) return rc;
    for (int l = 0; l < LLICTI_NLEVELS; ++l) level_ms[l] = c->last_cnn_level_ms[l];
    return LLICTI_OK;
}

extern "C" int llicti_image_status(llicti_ctx *c, int32_t *h_status, int n, void *stream)
{
    if (!c || !h_status || n < 1) return fail(LLICTI_EINVAL, "image_status: bad argument");
    DeviceGuard guard(c);
    if (!c->d_img_status || n > c->img_status_n) return fail(LLICTI_EINVAL, "image_status: the last decode held %d images ", c->img_status_n);
    HIPCHK(hipMemcpyAsync(h_status, c->d_img_status, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, (hipStream_t)stream));      // (on `stream` alone, as llicti_check_status)
    HIPCHK(hipStreamSynchronize((hipStream_t)stream));
    return LLICTI_OK;
}

extern "C" int llicti_selftest(void)
{
    if (int d = selftest_div_magic()) return fail(LLICTI_EINVAL, "selftest: magic division by %d differs from '/'", d);
    return LLICTI_OK;
}

// host_plan.hpp -- the HOST logic of the whole-batch calls: container tags, the layout of a call (workspace carving, per-image geometry
// tables, stream descriptors, tile lists of the band CNN), size bounds, header parsing.  Plain C++17 with no HIP dependency -- g++
// compiles it, with host_types.hpp and cnn_pack.hpp, under AddressSanitizer / UBSan and drives it over every (B, sizes, mode) the tests
// use plus malformed input (tests/sanitize_host.sh, tests/sanitize_host.cpp).  In the HIP build it is part of llicti_hip.hip.
#pragma once
#include <algorithm>
#include <cmath>
#include <vector>

#include "cnn_pack.hpp"
#include "host_types.hpp"

// One whole-batch call's layout: the workspace carving and the per-image tables the kernels read.  The images of a call may differ in
// size (llicti_encode_images_v / llicti_decode_images_v); llicti_encode_images / llicti_decode_images are the same code with B equal sizes.
struct TileRun { size_t off = 0; int n_tiles = 0, TH = 0, gx = 0; };      // band-CNN launch of one (level, band) of a mixed-size plan: its tile list
struct Plan {
    int B = 0, ME = 0;
    int nlev = LLICTI_NLEVELS;          // wavelet levels of the model (5: config A, 2: config B; see kLevelsB)
    int M = 0;                          // rANS streams per image (0: AC container only); images of a call may differ: the largest count
    int nstreams = 0;                   // ... and the streams of all images together (sref)
    std::vector<StreamRef> sref;        // [nstreams]: stream -> (image, stream of the image, its count, its first stream)
    int Q = 1;                          // 64-lane sub-chunks per stream step (2: wide streams of 128 lanes; 4: xwide streams of 256 lanes)
    bool uniform = true;                // every image has the size of image 0: the band CNN runs its division form, the AC container is available
    bool vec_ok = true;                 // every image's plane size and placement allow the lift's 4-pixel accesses
    long lev_maxpos[LLICTI_NLEVELS];    // largest band grid (h * w) of a level
    std::vector<long> key;              // (ME, B, tile-form tuning, H, W, rgb offset per image): what the cache compares
    size_t off_lift_part, off_acstate;
    long ac_cap_rows = 0;               // rows per image of one colour's chunk table buffer (AC decode)
    size_t off_planes, off_fplanes, off_minmax, off_status, off_params, off_params2, off_pairs, off_slots, off_slot_len, off_tables;
    size_t total = 0;
    size_t rgb_bytes = 0;               // extent of the caller's RGB buffer
    long max_plane = 0;                 // largest H * W of the batch
    std::vector<ImgGeo> img;            // [B]
    std::vector<Geom> geo;              // [level][B]
    std::vector<StageGeom> sg;          // [level * 3 + band][B]
    size_t lev_floats[LLICTI_NLEVELS];  // CNN outputs of one (level, band): 64 floats per band-grid position of every image
    std::vector<StreamDesc> desc;       // stage-major, image-minor: index (stage * B + b)
    std::vector<long> slot_off;         // AC container (uniform plans)
    std::vector<int32_t> slot_cap;
    long pair_base[LLICTI_NLEVELS * 3]; // per (lvl, band): first pair of [clr][image][n]
    size_t max_container = 0;           // of the batch's largest image
    int rslot_cap = 0;
    std::vector<long> rslot_off;        // [B*M] byte offsets into the slots region
    size_t off_rinfo, off_rstate, off_rpos, off_rtail;
    std::vector<TileRef> tiles;            // mixed-size plans: the tile lists of the 15 band-CNN launches, back to back
    TileRun run[LLICTI_NLEVELS * 3];
    // device copies (one block, see PlanBlock)
    size_t d_img = 0, d_geo = 0, d_sg = 0, d_desc = 0, d_slot_off = 0, d_slot_cap = 0, d_rslot_off = 0, d_tiles = 0, d_sref = 0, d_total = 0;
    // reduced-resolution decodes (plan_add_reduced): the levels the call skips and where every image's reduced output goes
    int reduce = 0;
    std::vector<RedGeo> red;            // [B], empty for reduce = 0
    long max_rplane = 0;                // the largest Hr * Wr: sizes the grid of unlift_reduced_kernel
    size_t d_red = 0;
    // interleaved pixel buffers (plan_add_pixels): every image's window in the caller's buffer
    std::vector<PixGeo> pix;            // [B], empty for the planar calls
    size_t d_pix = 0;
    long pix_units = 0;                 // the largest window in 4-pixel row pieces, H * ceil(W / 4): sizes the grids of lift_px_kernel / unlift_px_kernel
};

// AC decode has two table forms.  Few images in flight (latency bound: every stream is one serial wave and the GPU is
// mostly idle): FULL rows from cdf_table_kernel, because the search over a ready-made row is the shortest instruction
// sequence on the serial wave (B = 24: 249 ms against 293 ms).  Many images (the SIMDs' issue slots are the bound): ANCHOR
// rows -- 1/8 of the erfc work and a fifth of the HBM traffic, the bucket's 8 entries evaluated by the decoding wave
// (B = 256: 475 ms against 641 ms).  The workspace is sized for full rows below kAcAnchorBatch images and for anchor rows
// from there on; llicti_set_tuning("ac_anchor_min_batch") can only LOWER the switch point (tests run both forms).
constexpr int kAcAnchorBatch = 96;
static bool ac_use_anchors(int B, int min_batch = kAcAnchorBatch) { return B >= std::min(min_batch, kAcAnchorBatch); }

constexpr int kRansMaxStreams = 128;   // rANS streams per image: <= 32 one per segment, 64 / 128 grouped (rans_group())
constexpr int kStatusHead = 16;       // status words in front of the per-image ones (common.hpp: image_status())
// AC decode: a stage of nc symbols per stream is cut into C chunks (multiples of 64 symbols) so that the Y, Co and Cg
// streams of a band run as a three-deep pipeline on three HIP streams (see decode_batch)
static int ac_chunks(long nc) { return nc >= 32768 ? 16 : nc >= 4096 ? 8 : nc >= 1024 ? 4 : nc >= 256 ? 2 : 1; }
static long ac_chunk_rows(long nc) { const int C = ac_chunks(nc); return ((nc + C - 1) / C + 63) / 64 * 64; }

static size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

static int stage_index(int lvl, int band, int clr) { return (LLICTI_NLEVELS - 1 - lvl) * 9 + band * 3 + clr; }   // scale 4..0

// Model shapes: config A codes 5 levels (88-wide heads), config B 2 (60-wide heads).  The stages keep config A's numbering for both: level l < L
// is stage_index(l, ..) whatever L is, so a 2-level model's plan has its first 27 stages EMPTY (n = 0, never launched) and every kernel that
// names "the last stage" (level 0, band x10: LLICTI_NSTREAMS - 1) or walks the stage table needs no change.  Its container has 4 + 9 L segments:
// the AC streams of stages first_stage(L) .. 44 are segments 4 .. 4 + 9 L - 1; rANS streams, at most 9 L per image, are segments 4 .. 4 + M - 1.
constexpr int kLevelsB = 2;
static int first_stage(int nlev) { return 9 * (LLICTI_NLEVELS - nlev); }
static int model_segments(int nlev) { return 4 + 9 * nlev; }

static int pad_int(int H, int W, int nlev = LLICTI_NLEVELS)
{
    int v = 0;
    for (int l = 0; l < nlev; ++l) {
        Geom g = make_geom(1, H, W, l);
        v = 4 * v + 2 * g.padH + g.padW;       // LLICTI_nets.py:230
    }
    return v;
}

// Bytes of a container's header: 17 + one raw byte per colour and position of the last level's grid (LLICTI_nets.py:347-350)
static int header_bytes(int H, int W, int nlev)
{
    const Geom g = make_geom(1, H, W, nlev - 1);
    return 17 + 3 * g.h * g.w;
}

// Tile height of a band-CNN launch (16, 8 or 4 rows; one wavefront per row, so 16 / 8 / 4 wavefronts per workgroup): the form whose launch is
// shortest under a two-parameter model of the persistent grid -- rounds = ceil(tiles / workgroups that fit the chip), a round = a fixed part
// (halo rows, staging the head's weights, barrier) + a part per tile row; the constants are the measured 46 / 25 / 15 us of a band-2
// tile of 16 / 8 / 4 rows.  Full launches come out at 16 rows; launches of one to three half-empty rounds (levels 3 and 4 of a batch
// of 24) at 8; launches that cannot give every compute unit a workgroup (coarse levels of a single image) at 4.  Every form computes
// each position with the same fmaf chains: the results do not depend on it (test_band_params_bitexact_and_golden runs all three).
// count(th) = tiles of the launch in tiles of th rows (all images).  tile_rows: llicti_set_tuning("cnn_tile_rows").
struct TileForm { int TH, gx; long n_tiles; };
template <class COUNT>
static TileForm choose_tile_form(int n_cu, int tile_rows, int band, COUNT &&count)
{
    auto plan_for = [&](int th, int *gx_out, long *tiles_out) -> double {
        const long tiles = count(th);
        const int per_cu = std::max(1, std::min(4, (160 * 1024) / cnn_lds_bytes(band, th)));
        const long gx = std::max<long>(1, std::min<long>(tiles, (long)n_cu * per_cu / 4));
        *gx_out = (int)gx; *tiles_out = tiles;
        return (double)((tiles + gx - 1) / gx) * (4.7 + 2.6 * th);
    };
    TileForm f{ kTileHMax, 1, 0 };
    if (tile_rows > 0) { f.TH = tile_rows; (void)plan_for(f.TH, &f.gx, &f.n_tiles); }
    else if (tile_rows < 0) {                              // round 3's rule (A/B): 4 rows iff the 16-row tiles cannot fill the chip
        f.TH = (4 * count(kTileHMax) < n_cu) ? kTileHSmall : kTileHMax;
        (void)plan_for(f.TH, &f.gx, &f.n_tiles);
    } else {
        // Launches of one or two rounds of 16-row tiles (coarse levels, single images) are priced from a table instead: a launch's first
        // round and its later ones per (band, form), measured on single-image launches (rocprofv3, tools/single_image_trace.py) -- the linear
        // model is off exactly there: a 4-row tile of band 2 takes 21-25 us, not 15 (one wavefront per SIMD cannot keep the matrix pipe busy and
        // 120 input channels are the longest layer 0), so three rounds of them lost to ONE round of 16-row tiles at level 1 of a lone image
        // (75 against 47 us).  Band 0 fits two workgroups per compute unit: its rounds are priced as shared.
        static const double kFirstUs[3][3] = { { 31.5, 18.1, 12.5 }, { 36.4, 20.8, 14.5 }, { 46.3, 26.2, 21.4 } };      // [band][16, 8, 4 rows]
        static const double kLaterUs[3][3] = { { 31.0, 17.0, 11.0 }, { 36.4, 19.0, 11.2 }, { 46.0, 23.9, 25.2 } };
        static const double kSharedUs[3] = { 61.3, 31.2, 16.7 };                                                            // band 0, two workgroups per CU
        int gx16; long nt16;
        (void)plan_for(kTileHMax, &gx16, &nt16);
        const bool small_launch = (nt16 + gx16 - 1) / gx16 <= 2;
        double best = 0;
        int fi = 0;
        for (int th : { kTileHMax, kTileHMid, kTileHSmall }) {
            int gx_t; long nt;
            double t = plan_for(th, &gx_t, &nt);
            if (small_launch) {
                const long rounds = (nt + gx_t - 1) / gx_t;
                const bool shared = 4L * gx_t > n_cu;                      // more workgroups (4 heads) than compute units
                t = shared ? 2.0 + rounds * kSharedUs[fi] : kFirstUs[band][fi] + (rounds - 1) * kLaterUs[band][fi];
            }
            if (th == kTileHMax || t < 0.995 * best) { best = t; f.TH = th; f.gx = gx_t; f.n_tiles = nt; }    // ties go to the larger form
            ++fi;
        }
    }
    return f;
}

// The band CNN's tile lists of levels lvl_first, lvl_first +- 1, ... up to but not including lvl_end, in that order, behind what `tiles` holds: one
// list per (level, band) over the images with active(b, lvl) -- image-major, rows, columns: the order the division form walks -- and its TileRun in
// run[lvl * 3 + band] (form chosen over those images; n_tiles clamped to 2^31 - 1).  No active image at a level: no list, its runs stay as they are.
// geo: a plan's [level][B] table.
template <class ACTIVE>
static void build_tile_lists(const std::vector<Geom> &geo, int B, int lvl_first, int lvl_end, ACTIVE &&active, int n_cu, int tile_rows,
                             std::vector<TileRef> &tiles, TileRun *run)
{
    for (int lvl = lvl_first; lvl != lvl_end; lvl += lvl_end > lvl_first ? 1 : -1) {
        const Geom *gl = &geo[(size_t)lvl * B];
        auto count = [&](int th) -> long {
            long t = 0;
            for (int b = 0; b < B; ++b) if (active(b, lvl)) t += (long)((gl[b].w + kTileW - 1) / kTileW) * ((gl[b].h + th - 1) / th);
            return t;
        };
        if (count(kTileHMax) == 0) continue;
        for (int band = 0; band < 3; ++band) {
            const TileForm f = choose_tile_form(n_cu, tile_rows, band, count);
            TileRun &r = run[lvl * 3 + band];
            r.off = tiles.size(); r.n_tiles = (int)std::min<long>(f.n_tiles, 0x7FFFFFFFL); r.TH = f.TH; r.gx = f.gx;
            for (int b = 0; b < B; ++b) {
                if (!active(b, lvl)) continue;
                const int tx_n = (gl[b].w + kTileW - 1) / kTileW, ty_n = (gl[b].h + f.TH - 1) / f.TH;
                for (int ty = 0; ty < ty_n; ++ty)
                    for (int tx = 0; tx < tx_n; ++tx) tiles.push_back(TileRef{ b, (ty << 16) | tx });
            }
        }
    }
}

static int rans_byte0(int M, int Q, int nlev = LLICTI_NLEVELS);
static int rans_pad_hi(int M, int Q);

// Bytes of the slot one rANS stream of an H x W image gets when the image has M streams of 64 Q lanes.  The worst case of one stream: every
// symbol emits 16 bits; chunks of 64 Q symbols are dealt round-robin, so a stream gets at most ceil(nchunks / M) chunks of every stage; + T, the
// 31-bit states, slack, zero pad (xwide v4: + the tail's spill and the header field).  build_plan sizes the slots with it, check_stream_bits bounds it.
static long rans_slot_bytes(int nlev, int H, int W, int M, int Q)
{
    const long L = 64 * Q;
    long syms = 0;
    for (int lvl = 0; lvl < nlev; ++lvl) {
        const Geom g = make_geom(1, H, W, lvl);
        for (int band = 0; band < 3; ++band) {
            int hc, wc;
            coded_dims(g, band, &hc, &wc);
            const long nchunks = ((long)hc * wc + L - 1) / L;
            syms += 3 * ((nchunks + M - 1) / M * L);      // (the three colours of a band code the same positions)
        }
    }
    return (long)align_up((size_t)(2 * syms + 4 + 8 + Q * RansGeo<1>::kPayBytes + 16 + 64 + (Q == 4 ? kRansSpillMax / 8 + 8 : 0)), 64);
}

// What a plan is built from, and nothing else: two calls with equal specs get equal plans.
struct PlanSpec {
    int B = 0;
    const int *Hs = nullptr, *Ws = nullptr;      // B sizes
    // ME: streams per image, | 0x100 for wide (128-lane) streams, | 0x200 for xwide (256-lane) streams -- what mode_streams() returns.
    // Ms: B stream counts (rANS containers: the images of a call may have different ones -- every header carries its own -- so that larger images
    // get more streams and a stage launch does not wait for its largest image), each | 0x1000 if that image is "auto" (ME then has 0x1000 if any
    // image is), or nullptr = ME's count and kind for every image.  Fixed and "auto" xwide images may share a call: a fixed one has Mlo = 0.
    int ME = 0;
    const int *Ms = nullptr;
    int nlev = LLICTI_NLEVELS;                   // the model's levels (LLICTI_NLEVELS: config A; kLevelsB: config B)
    bool force_ragged = false;                   // llicti_set_tuning("force_ragged"): image blocks at 64-element boundaries
    const size_t *rgb_off = nullptr;             // B byte offsets of the images in the caller's RGB buffer, or nullptr = tightly packed in call order
    int n_cu = 256, tile_rows = 0;               // the band CNN's tile forms of a mixed-size plan are chosen (and its tile lists written) in build_plan
};
static const int *modes_ptr(const std::vector<int> &Ms) { return Ms.empty() ? nullptr : Ms.data(); }      // resolve_modes' Ms as PlanSpec::Ms

// The cache key of a full-size planar plan, Plan::key: (ME, B, tile-form tuning, then H, W, rgb offset and stream count per image).  nlev and n_cu are
// the context's, whose cache it is (llicti_set_model drops the plans); reduced_key_tail and pixel_key_tail follow for the other plan kinds.
static std::vector<long> plan_key(const PlanSpec &sp)
{
    std::vector<long> key;
    key.reserve(3 + 4 * (size_t)sp.B);
    key.push_back(sp.ME); key.push_back(sp.B); key.push_back(sp.tile_rows * 2 + (sp.force_ragged ? 1 : 0));
    long pos = 0;
    for (int b = 0; b < sp.B; ++b) {
        key.push_back(sp.Hs[b]); key.push_back(sp.Ws[b]); key.push_back(sp.rgb_off ? (long)sp.rgb_off[b] : pos);
        key.push_back((sp.Ms && (sp.ME & 0xFF)) ? sp.Ms[b] : (sp.ME & 0xFF));
        pos += 3L * sp.Hs[b] * sp.Ws[b];
    }
    return key;
}

static void build_plan(Plan &p, const PlanSpec &sp)
{
    const int B = sp.B, ME = sp.ME, nlev = sp.nlev, n_cu = sp.n_cu, tile_rows = sp.tile_rows;
    const int *Hs = sp.Hs, *Ws = sp.Ws, *Ms = sp.Ms;
    const size_t *rgb_off = sp.rgb_off;
    const int Q = 1 << ((ME >> 8) & 3);
    const bool per_image = Ms && (ME & 0xFF) > 0;
    auto m_of = [&](int b) -> int { return per_image ? (Ms[b] & 0xFF) : (ME & 0xFF); };
    // LLICTI_MODE_RANS_X_AUTO: the count is the size rule's (Mlo); the encoder picks per image in [rans_auto_min, rans_auto_hi]
    auto auto_of = [&](int b) -> bool { return ((per_image ? Ms[b] : ME) & 0x1000) != 0; };
    int M = 0;
    for (int b = 0; b < B; ++b) M = std::max(M, auto_of(b) ? rans_auto_hi(m_of(b)) : m_of(b));
    p.B = B; p.ME = ME; p.M = M; p.Q = Q; p.nlev = nlev;
    p.uniform = !sp.force_ragged;
    for (int b = 1; b < B; ++b) if (Hs[b] != Hs[0] || Ws[b] != Ws[0]) p.uniform = false;
    {
        long pos = 0;
        for (int b = 0; b < B; ++b) { if (rgb_off && (long)rgb_off[b] != pos) p.uniform = false; pos += 3L * Hs[b] * Ws[b]; }      // (the division form of the kernels assumes tightly packed images)
    }
    p.vec_ok = true;
    p.rgb_bytes = 0;
    p.key = plan_key(sp);
    // images: sizes, header constants, placement (mixed sizes: planes / fplanes blocks start at multiples of 64 elements; equal sizes: tightly
    // packed, [B][3][H][W] -- what the division form of the band CNN and the AC container's kernels index)
    p.img.assign(B, ImgGeo{});
    long pix = 0, rgb_pos = 0;
    p.max_plane = 0;
    for (int b = 0; b < B; ++b) {
        ImgGeo &ig = p.img[b];
        ig.H = Hs[b]; ig.W = Ws[b];
        const Geom g4 = make_geom(1, ig.H, ig.W, nlev - 1);          // the last level's grid: the header's size bytes and the raw DC band
        ig.h4 = g4.h; ig.w4 = g4.w; ig.hdr_bytes = header_bytes(ig.H, ig.W, nlev);
        ig.dcs = 2 << (nlev - 1);
        ig.nseg = model_segments(nlev);
        ig.plane = (long)ig.H * ig.W;
        ig.pix_off = pix;
        pix += p.uniform ? 3 * ig.plane : (long)align_up((size_t)(3 * ig.plane), 64);
        ig.rgb_off = rgb_off ? (long)rgb_off[b] : rgb_pos;
        rgb_pos += 3 * ig.plane;
        if ((ig.plane & 3) || (ig.rgb_off & 3)) p.vec_ok = false;
        p.rgb_bytes = std::max(p.rgb_bytes, (size_t)(ig.rgb_off + 3 * ig.plane));
        p.max_plane = std::max(p.max_plane, ig.plane);
        ig.Mlo = auto_of(b) ? m_of(b) : 0;
        ig.M = auto_of(b) ? rans_auto_hi(ig.Mlo) : m_of(b);
        ig.byte0 = ig.M ? rans_byte0(ig.M, Q, nlev) : nlev;
        ig.padint = pad_int(ig.H, ig.W, nlev) | ((ig.M ? rans_pad_hi(ig.M, Q) : 0) << 10);      // the header's int16 pad field (xwide v4: its high bits carry the stream count; an "auto" encode writes the count it picked)
    }
    size_t o = 0;
    auto take = [&](size_t bytes) { size_t r = o; o = align_up(o + bytes, 256); return r; };
    p.off_status = take(kStatusHead * sizeof(int32_t) + (size_t)B * sizeof(int32_t));   // [0]: the call's status; [kStatusHead + b]: image b's
    p.off_minmax = take((size_t)B * 4 * sizeof(int32_t));
    p.off_lift_part = take((size_t)kLiftMaxParts * 4 * sizeof(int32_t));
    p.off_planes = take((size_t)pix * sizeof(int16_t));
    p.off_fplanes = take((size_t)pix * sizeof(float));
    // levels: geometry and the placement of every image's CNN outputs
    p.geo.assign((size_t)LLICTI_NLEVELS * B, Geom{});
    for (int lvl = 0; lvl < LLICTI_NLEVELS; ++lvl) {
        size_t fl = 0;
        p.lev_maxpos[lvl] = 0;
        for (int b = 0; b < B; ++b) {
            Geom g = make_geom(B, Hs[b], Ws[b], lvl);
            p.lev_maxpos[lvl] = std::max(p.lev_maxpos[lvl], (long)g.h * g.w);
            g.pix_off = p.img[b].pix_off;
            g.par_off = (long)fl;
            fl += (size_t)g.h * g.w * LLICTI_PARAM_STRIDE;
            p.geo[(size_t)lvl * B + b] = g;
        }
        p.lev_floats[lvl] = fl;
    }
    p.off_params = take(std::max(p.lev_floats[0], 3 * p.lev_floats[1]) * sizeof(float));
    // stages: pairs, streams, AC slots
    p.sg.assign((size_t)LLICTI_NLEVELS * 3 * B, StageGeom{});
    p.desc.assign((size_t)LLICTI_NSTREAMS * B, StreamDesc{});
    if (M == 0) { p.slot_off.assign((size_t)LLICTI_NSTREAMS * B, 0); p.slot_cap.assign((size_t)LLICTI_NSTREAMS * B, 0); }
    long pair_pos = 0, slot_pos = 0;
    std::vector<size_t> container(B);
    for (int b = 0; b < B; ++b) container[b] = (size_t)p.img[b].hdr_bytes;
    for (int lvl = nlev - 1; lvl >= 0; --lvl) {            // (the stages of levels >= nlev stay empty)
        for (int band = 0; band < 3; ++band) {
            StageGeom *sgr = &p.sg[(size_t)(lvl * 3 + band) * B];
            long cs = 0;
            for (int b = 0; b < B; ++b) {
                sgr[b] = make_stage(p.geo[(size_t)lvl * B + b], band);
                sgr[b].pair_off = cs;
                cs += (long)sgr[b].hc * sgr[b].wc;
            }
            for (int b = 0; b < B; ++b) sgr[b].pair_cs = cs;
            p.pair_base[lvl * 3 + band] = pair_pos;
            for (int clr = 0; clr < 3; ++clr) {
                const int st = stage_index(lvl, band, clr);
                for (int b = 0; b < B; ++b) {
                    const long nc = (long)sgr[b].hc * sgr[b].wc;
                    StreamDesc &d = p.desc[(size_t)st * B + b];
                    d.pair_off = pair_pos + (long)clr * cs + sgr[b].pair_off;
                    d.n = (int)nc;
                    if (M == 0) {
                        const int cap = (int)align_up((size_t)(2 * nc + 8 + 16), 16);   // <= 16 bits per symbol + termination + zero pad
                        d.out_off = slot_pos;
                        d.cap = cap - 16;
                        p.slot_off[(size_t)st * B + b] = slot_pos;
                        p.slot_cap[(size_t)st * B + b] = cap;
                        slot_pos += cap;
                    }
                    container[b] += (size_t)(2 * nc + 8);
                }
            }
            pair_pos += 3 * cs;
        }
    }
    p.max_container = 0;
    for (int b = 0; b < B; ++b) p.max_container = std::max(p.max_container, align_up(container[b] + 64 * 45, 16));
    p.off_pairs = take((size_t)pair_pos * sizeof(uint32_t));
    p.sref.clear();
    p.nstreams = 0;
    if (M > 0) {
        // one slot capacity for all streams: the largest any image's need (rans_slot_bytes)
        const int pay_bytes = Q * RansGeo<1>::kPayBytes;
        p.rslot_cap = 0;
        for (int b = 0; b < B; ++b) {
            const int Mb = p.img[b].M;
            const int Mfew = p.img[b].Mlo ? rans_auto_min(p.img[b].Mlo) : Mb;      // the fewest streams the image may end up with: the longest ones
            long all_syms = 0;
            for (int st = 0; st < LLICTI_NSTREAMS; ++st) all_syms += ((long)p.desc[(size_t)st * B + b].n + 63) / 64 * 64;
            p.rslot_cap = std::max(p.rslot_cap, (int)rans_slot_bytes(nlev, p.img[b].H, p.img[b].W, Mfew, Q));      // (below 2^28: check_stream_bits)
            // container bound: the streams together hold every symbol once (<= 16 bits each, whole chunks), plus per stream T | pad, the
            // 64 final states, a table entry (M > 32) and the byte the bit region rounds up to
            p.max_container = std::max(p.max_container, align_up((size_t)p.img[b].hdr_bytes + (size_t)(2 * all_syms) + (size_t)Mb * (2 + pay_bytes + 4 + 4 + (Q == 4 ? kRansSpillMax / 8 : 0)) + 64, 16));
            p.img[b].sbase = p.nstreams;
            for (int m = 0; m < Mb; ++m) p.sref.push_back(StreamRef{ b, m, Mb, p.nstreams });
            p.nstreams += Mb;
        }
        p.rslot_off.assign((size_t)p.nstreams, 0);
        for (long i = 0; i < (long)p.nstreams; ++i) p.rslot_off[i] = (long)i * p.rslot_cap;
        slot_pos = (long)p.nstreams * p.rslot_cap;
    }
    p.off_slots = take((size_t)slot_pos);
    const size_t ns = std::max((size_t)p.nstreams, (size_t)B * 32);
    p.off_rinfo = take(ns * 2 * sizeof(int32_t));
    p.off_rstate = take(ns * 64 * Q * sizeof(uint32_t));
    p.off_rpos = take(ns * sizeof(uint32_t));
    p.off_rtail = take(ns * sizeof(uint32_t));
    p.off_slot_len = take((size_t)LLICTI_NSTREAMS * B * sizeof(int32_t));
    // AC decode (equal sizes only): one chunk buffer per colour channel -- full rows (512 x uint16) or anchor rows (kAnchorRow bytes), see ac_use_anchors()
    size_t tables_bytes = 0;
    p.ac_cap_rows = 0;
    if (M == 0) {
        for (int st = 0; st < LLICTI_NSTREAMS; ++st) p.ac_cap_rows = std::max(p.ac_cap_rows, ac_chunk_rows((long)p.desc[(size_t)st * B].n));
        tables_bytes = (size_t)3 * B * p.ac_cap_rows * (ac_use_anchors(B) ? (size_t)kAnchorRow : (size_t)512 * sizeof(uint16_t));
    }
    {   // a second, quarter-size buffer for the CNN outputs of levels >= 1 (llicti_set_tuning("enc_side_levels"): the encoder's coarse levels
        // on a side stream).  Only the encoder uses it and only the AC DECODER uses the chunk tables, so the two share their bytes.
        tables_bytes = std::max(tables_bytes, p.lev_floats[1] * sizeof(float));
        p.off_tables = take(tables_bytes);
        p.off_params2 = p.off_tables;
    }
    static_assert(kAnchorRow <= 1024, "anchor rows must fit the full-row buffer");
    p.off_acstate = take((size_t)3 * B * 8 * sizeof(uint32_t));
    p.total = o;
    // mixed sizes: the band CNN's tile lists (image-major, rows, columns: the order the division form walks)
    p.tiles.clear();
    for (int k = 0; k < LLICTI_NLEVELS * 3; ++k) p.run[k] = TileRun{};
    if (!p.uniform) build_tile_lists(p.geo, B, 0, nlev, [](int, int) { return true; }, n_cu, tile_rows, p.tiles, p.run);
    // the device block: every table at a 256-byte boundary
    size_t d = 0;
    auto dtake = [&](size_t bytes) { size_t r = d; d = align_up(d + bytes, 256); return r; };
    p.d_img = dtake(p.img.size() * sizeof(ImgGeo));
    p.d_geo = dtake(p.geo.size() * sizeof(Geom));
    p.d_sg = dtake(p.sg.size() * sizeof(StageGeom));
    p.d_desc = dtake(p.desc.size() * sizeof(StreamDesc));
    p.d_slot_off = dtake(p.slot_off.size() * sizeof(long));
    p.d_slot_cap = dtake(p.slot_cap.size() * sizeof(int32_t));
    p.d_rslot_off = dtake(p.rslot_off.size() * sizeof(long));
    p.d_tiles = dtake(p.tiles.size() * sizeof(TileRef));
    p.d_sref = dtake(p.sref.size() * sizeof(StreamRef));
    p.d_total = d;
}

// The reduce of a decode: one level r for every image, or (the _rv calls) image b's own rv[b].
struct Reduces {
    int r = 0;
    const int *rv = nullptr;            // B values; r is not read then
    Reduces(int r_ = 0) : r(r_) {}
    static Reduces each(const int *rv) { Reduces d; d.rv = rv; return d; }
    bool per_image() const { return rv != nullptr; }
    int of(int b) const { return rv ? rv[b] : r; }
    int min(int B) const { int m = of(0); for (int b = 1; b < B; ++b) m = std::min(m, of(b)); return m; }
};
// Where a reduced decode's output goes: every image's size at its reduce and its byte offset (out_off, or nullptr = tightly packed in call order,
// each image at its own reduced size), the largest Hr * Wr (the grid of unlift_reduced_kernel) and the largest image in 4-pixel row pieces,
// Hr * ceil(Wr / 4) (the grid of unlift_px_kernel).  At reduce 0 the sizes are the full ones.
struct ReducedOut { std::vector<RedGeo> red; long max_rplane = 0, pix_units = 0; };
static ReducedOut reduced_out(int B, const int *Hs, const int *Ws, const Reduces &rd, const size_t *out_off)
{
    ReducedOut o;
    o.red.assign(B, RedGeo{});
    long pos = 0;
    for (int b = 0; b < B; ++b) {
        RedGeo &rg = o.red[b];
        rg.Hr = reduced_dim(Hs[b], rd.of(b)); rg.Wr = reduced_dim(Ws[b], rd.of(b));
        rg.off = out_off ? (long)out_off[b] : pos;
        pos += 3L * rg.Hr * rg.Wr;
        o.max_rplane = std::max(o.max_rplane, (long)rg.Hr * rg.Wr);
        o.pix_units = std::max(o.pix_units, (long)rg.Hr * ((rg.Wr + 3) / 4));
    }
    return o;
}
static ReducedOut reduced_out(const std::vector<ImgGeo> &img, const Reduces &rd, const size_t *out_off)      // (a plan's image table)
{
    std::vector<int> Hs, Ws;
    for (const ImgGeo &ig : img) { Hs.push_back(ig.H); Ws.push_back(ig.W); }
    return reduced_out((int)img.size(), Hs.data(), Ws.data(), rd, out_off);
}

// The extra words a reduced-resolution decode adds to the cache key of its batch's plan: a marker that no full-size key holds at that place
// (-reduce: sizes are >= 32), then the byte offset of every image's reduced output (reduced_out's).
// A full-size key has 3 + 4 B words, a reduced one 4 + 5 B: the two never compare equal, so a reduced call never finds, changes or
// replaces the full-size plan of the same batch.
static void reduced_key_tail(std::vector<long> &key, int reduce, const std::vector<RedGeo> &red)
{
    key.push_back(-(long)reduce);
    for (const RedGeo &rg : red) key.push_back(rg.off);
}
static void reduced_key_tail(std::vector<long> &key, int B, const int *Hs, const int *Ws, int reduce, const size_t *out_off)
{
    reduced_key_tail(key, reduce, reduced_out(B, Hs, Ws, reduce, out_off).red);
}
// Turns the plan build_plan made for a batch -- with FULL-size tight RGB placement: `uniform`, `vec_ok`, ImgGeo::rgb_off and rgb_bytes keep
// their full-size meaning and nothing of the decode's stages changes -- into the plan of a decode that stops after level `reduce`
// (1 .. nlev): the output table of unlift_reduced_kernel goes behind the other tables of the device block, the key gets its tail.
static void plan_add_reduced(Plan &p, int reduce, const size_t *out_off)
{
    ReducedOut o = reduced_out(p.img, reduce, out_off);
    p.reduce = reduce;
    p.red.swap(o.red);
    p.max_rplane = o.max_rplane;
    p.pix_units = o.pix_units;          // (of a pixel call: plan_add_pixels)
    reduced_key_tail(p.key, reduce, p.red);
    p.d_red = p.d_total;
    p.d_total = align_up(p.d_total + p.red.size() * sizeof(RedGeo), 256);
}

// Interleaved pixel buffers (llicti_encode_images_px / llicti_decode_images_px).  Bytes per pixel of a format, 0: not a format.
static int pix_format_bytes(int fmt) { return (fmt >= LLICTI_PIX_RGB8 && fmt <= LLICTI_PIX_BGRA8) ? pix_bpp(fmt) : 0; }
// Bytes from the first pixel of an H x W window to the end of its last one: (H - 1) pitch + W bpp.  pitch = 0: tight rows.  0: bad argument.
static size_t pix_window_span(int fmt, int H, int W, size_t pitch)
{
    const int bpp = pix_format_bytes(fmt);
    if (!bpp || H < 1 || W < 1) return 0;
    const size_t row = (size_t)W * bpp;
    if (pitch == 0) pitch = row;
    if (pitch < row || pitch > 0x7FFFFFFFu) return 0;
    return (size_t)(H - 1) * pitch + row;
}
// The windows of a call, validated: image b's is Hw[b] x Ww[b] (a reduced decode: the reduced size).  pitch = nullptr: tight rows;
// px_off = nullptr: the windows back to back in call order, each of its own span.
static int resolve_pixels(const char *who, int B, const int *Hw, const int *Ww, int fmt, const size_t *px_off, const size_t *pitch, std::vector<PixGeo> &out)
{
    const int bpp = pix_format_bytes(fmt);
    if (!bpp) return fail(LLICTI_EINVAL, "%s: unknown pixel format %d (LLICTI_PIX_RGB8, _BGR8, _RGBA8, _BGRA8)", who, fmt);
    out.assign(B, PixGeo{});
    size_t pos = 0;
    for (int b = 0; b < B; ++b) {
        const size_t row = (size_t)Ww[b] * bpp, pt = pitch ? pitch[b] : row;
        if (pt < row || pt > 0x7FFFFFFFu)
            return fail(LLICTI_EINVAL, "%s: pitch %zu of image %d (a row of its %d pixels has %zu bytes; at most 2^31 - 1)", who, pt, b, Ww[b], row);
        out[b].off = (long)(px_off ? px_off[b] : pos);
        out[b].pitch = (int)pt;
        out[b].fmt = fmt;
        pos += pix_window_span(fmt, Hw[b], Ww[b], pt);
    }
    return 0;
}
// The extra words a call on interleaved pixels adds to the cache key of its batch's plan, behind the reduced tail if there is one: a marker
// no other key holds at that place (sizes are >= 32, a reduced tail starts with -1 .. -5), then every window's offset and pitch.  With B in
// word 1, keys of 3 + 4 B (planar), 4 + 5 B (reduced), 4 + 6 B (pixels) and 5 + 7 B (both) words never compare equal.
static void pixel_key_tail(std::vector<long> &key, const std::vector<PixGeo> &pix)
{
    key.push_back(-(16 + (long)pix[0].fmt));
    for (const PixGeo &pg : pix) { key.push_back(pg.off); key.push_back(pg.pitch); }
}
// Turns the plan of a batch -- build_plan's, with plan_add_reduced's table for a reduced decode; tight PLANAR placement, whose fields
// (`uniform`, `vec_ok`, ImgGeo::rgb_off, rgb_bytes, the tile lists) keep their meaning and are not read by the pixel kernels -- into the plan
// of a call on interleaved pixels: the window table goes behind the other tables of the device block, the key gets its tail.
static void plan_add_pixels(Plan &p, const std::vector<PixGeo> &pix)
{
    p.pix = pix;
    if (!p.reduce) p.pix_units = reduced_out(p.img, 0, nullptr).pix_units;      // (a reduced plan has its own from plan_add_reduced)
    pixel_key_tail(p.key, pix);
    p.d_pix = p.d_total;
    p.d_total = align_up(p.d_total + p.pix.size() * sizeof(PixGeo), 256);
}

// The normalisation constants of a float tensor output, validated: both or neither, every std finite and above zero
static int resolve_norm(const char *who, const float *mean, const float *std, TensorNorm &nm)
{
    if ((mean == nullptr) != (std == nullptr)) return fail(LLICTI_EINVAL, "%s: mean and std go together (both, or both NULL)", who);
    memset(&nm, 0, sizeof nm);
    if (mean) {
        for (int k = 0; k < 3; ++k) {
            if (!(std[k] > 0.0f) || !std::isfinite(std[k])) return fail(LLICTI_EINVAL, "%s: std[%d] = %g (need a finite value above zero)", who, k, (double)std[k]);
            nm.mean[k] = mean[k]; nm.std[k] = std[k];
        }
        nm.on = 1;
    }
    return 0;
}

// Float tensor output (llicti_decode_images_tensor): the output description as the caller gave it ...
struct TensorArgs { int dtype, Ho, Wo; const int *y0, *x0; const uint8_t *flip; const float *mean, *std; };
// ... and validated against the call's images (FULL sizes Hs, Ws, image b decoded at rd.of(b)): every image's packed window word (tensor_win_pack)
// and the normalisation constants.  These are the call's kernel arguments -- nothing of them enters the plan or its key.
static int resolve_tensor(const char *who, int B, const int *Hs, const int *Ws, const Reduces &rd, const TensorArgs &t, std::vector<uint32_t> &wins, TensorNorm &nm)
{
    if (!tensor_elem_bytes(t.dtype)) return fail(LLICTI_EINVAL, "%s: unknown dtype %d (LLICTI_T_F32, _F16, _BF16)", who, t.dtype);
    if (t.Ho < 1 || t.Wo < 1) return fail(LLICTI_EINVAL, "%s: output size %dx%d (need Ho, Wo >= 1)", who, t.Wo, t.Ho);
    if (int rc = resolve_norm(who, t.mean, t.std, nm)) return rc;
    wins.assign(B, 0u);
    for (int b = 0; b < B; ++b) {
        const int y0 = t.y0 ? t.y0[b] : 0, x0 = t.x0 ? t.x0[b] : 0;
        const int reduce = rd.of(b);
        if (!tensor_window_ok(Hs[b], Ws[b], reduce, y0, x0, t.Ho, t.Wo))
            return fail(LLICTI_EINVAL, "%s: the %dx%d window at (y %d, x %d) leaves image %d (%dx%d at reduce %d)", who, t.Wo, t.Ho, y0, x0, b,
                        reduced_dim(Ws[b], reduce), reduced_dim(Hs[b], reduce), reduce);
        wins[b] = tensor_win_pack(y0, x0, t.flip && t.flip[b]);
    }
    return 0;
}

// Tensor options (the _o calls): what does not depend on the image -- layout, pad mode, fill space and fill -- validated into the kernel's
// TensorPad.  pad_allowed = false (the resized and views calls): anything but LLICTI_PAD_NONE is refused.
static bool tensor_opts_plain(const llicti_tensor_opts *o) { return !o || (o->layout == LLICTI_LAYOUT_NCHW && o->pad_mode == LLICTI_PAD_NONE); }
static int resolve_tensor_opts(const char *who, const llicti_tensor_opts &o, bool pad_allowed, TensorPad &pad)
{
    if (o.layout != LLICTI_LAYOUT_NCHW && o.layout != LLICTI_LAYOUT_NHWC) return fail(LLICTI_EINVAL, "%s: unknown layout %d (LLICTI_LAYOUT_NCHW, _NHWC)", who, o.layout);
    if (o.pad_mode < LLICTI_PAD_NONE || o.pad_mode > LLICTI_PAD_SYMMETRIC)
        return fail(LLICTI_EINVAL, "%s: unknown pad mode %d (LLICTI_PAD_NONE, _CONSTANT, _EDGE, _REFLECT, _SYMMETRIC)", who, o.pad_mode);
    if (!pad_allowed && o.pad_mode != LLICTI_PAD_NONE)
        return fail(LLICTI_EINVAL, "%s: pad mode %d: a box that leaves its image is refused, only llicti_decode_images_tensor_o pads (pass LLICTI_PAD_NONE)", who, o.pad_mode);
    memset(&pad, 0, sizeof pad);
    pad.layout = o.layout; pad.mode = o.pad_mode;
    if (o.pad_mode == LLICTI_PAD_NONE) return 0;                      // (fill space and fill are read with a pad mode alone)
    if (o.fill_space != LLICTI_FILL_PIXEL && o.fill_space != LLICTI_FILL_OUTPUT)
        return fail(LLICTI_EINVAL, "%s: unknown fill space %d (LLICTI_FILL_PIXEL, _OUTPUT)", who, o.fill_space);
    pad.space = o.fill_space;
    for (int k = 0; k < 3; ++k) {
        if (!std::isfinite(o.fill[k])) return fail(LLICTI_EINVAL, "%s: fill[%d] = %g (need a finite value)", who, k, (double)o.fill[k]);
        pad.fill[k] = o.fill[k];
    }
    return 0;
}
// resolve_tensor for a call with options: the same checks of dtype, size and normalisation; every image's window held to the pad mode
// (tensor_window_pad_ok; LLICTI_PAD_NONE: resolve_tensor's rule) and packed into its TWO signed words (pad_win_pack).  Kernel arguments all.
static int resolve_tensor_padded(const char *who, int B, const int *Hs, const int *Ws, const Reduces &rd, const TensorArgs &t, const llicti_tensor_opts &o,
                                 std::vector<uint32_t> &wins, TensorNorm &nm, TensorPad &pad)
{
    if (!tensor_elem_bytes(t.dtype)) return fail(LLICTI_EINVAL, "%s: unknown dtype %d (LLICTI_T_F32, _F16, _BF16)", who, t.dtype);
    if (int rc = resolve_tensor_opts(who, o, true, pad)) return rc;
    if (t.Ho < 1 || t.Wo < 1 || (pad.mode != LLICTI_PAD_NONE && (t.Ho > 8160 || t.Wo > 8160)))
        return fail(LLICTI_EINVAL, "%s: output size %dx%d (need Ho, Wo >= 1; with a pad mode at most 8160)", who, t.Wo, t.Ho);
    if (int rc = resolve_norm(who, t.mean, t.std, nm)) return rc;
    wins.assign(2 * (size_t)B, 0u);
    for (int b = 0; b < B; ++b) {
        const int y0 = t.y0 ? t.y0[b] : 0, x0 = t.x0 ? t.x0[b] : 0;
        const int reduce = rd.of(b), Hr = reduced_dim(Hs[b], reduce), Wr = reduced_dim(Ws[b], reduce);
        if (pad.mode != LLICTI_PAD_NONE && (y0 < -kPadOriginMax || y0 > kPadOriginMax || x0 < -kPadOriginMax || x0 > kPadOriginMax))
            return fail(LLICTI_EINVAL, "%s: the origin (y %d, x %d) of image %d (need -%d .. %d)", who, y0, x0, b, kPadOriginMax, kPadOriginMax);
        if (!tensor_window_pad_ok(Hs[b], Ws[b], reduce, y0, x0, t.Ho, t.Wo, pad.mode)) {
            if (pad.mode == LLICTI_PAD_NONE)
                return fail(LLICTI_EINVAL, "%s: the %dx%d window at (y %d, x %d) leaves image %d (%dx%d at reduce %d)", who, t.Wo, t.Ho, y0, x0, b, Wr, Hr, reduce);
            return fail(LLICTI_EINVAL, "%s: the %dx%d window at (y %d, x %d) overhangs image %d (%dx%d at reduce %d) by more than pad mode %d mirrors "
                        "(LLICTI_PAD_REFLECT: n - 1 pixels of an axis of n, LLICTI_PAD_SYMMETRIC: n)", who, t.Wo, t.Ho, y0, x0, b, Wr, Hr, reduce, pad.mode);
        }
        pad_win_pack(y0, x0, t.flip && t.flip[b], &wins[2 * (size_t)b]);
    }
    return 0;
}

// Resized crops (llicti_decode_images_tensor_resized): the output description as the caller gave it -- hs, ws NULL: the whole decoded image from
// the origin -- ...
struct ResizeArgs { int dtype, Ho, Wo; const int *y0, *x0, *hs, *ws; const uint8_t *flip; const float *mean, *std; int antialias; };
// ... and validated like resolve_tensor's: two packed words per image (ResizeBoxes) and the normalisation constants, kernel arguments all.
// (what does not depend on the image: dtype, output size, flag, a call-wide reduce -- per-image values are admit_reduces' to check -- mean and std)
static int resolve_resize_head(const char *who, const Reduces &rd, const ResizeArgs &t, TensorNorm &nm)
{
    if (!tensor_elem_bytes(t.dtype)) return fail(LLICTI_EINVAL, "%s: unknown dtype %d (LLICTI_T_F32, _F16, _BF16)", who, t.dtype);
    if (t.Ho < 1 || t.Wo < 1 || t.Ho > 8160 || t.Wo > 8160) return fail(LLICTI_EINVAL, "%s: output size %dx%d (need 1 <= Ho, Wo <= 8160)", who, t.Wo, t.Ho);
    if (t.antialias != 0 && t.antialias != 1) return fail(LLICTI_EINVAL, "%s: antialias = %d (0: two taps per axis, 1: the triangle filter widened by the scale)", who, t.antialias);
    if (!rd.per_image() && (rd.r < 0 || rd.r > LLICTI_NLEVELS)) return fail(LLICTI_EINVAL, "%s: reduce = %d", who, rd.r);
    if (int rc = resolve_norm(who, t.mean, t.std, nm)) return rc;
    return 0;
}
// (one box, entry k of the call's arrays, against its H x W image: `whose` is how a message names it; -> the two packed words)
static int resolve_resize_box(const char *who, const char *whose, int H, int W, int reduce, const ResizeArgs &t, int k, uint32_t *words)
{
    const int Hr = reduced_dim(H, reduce), Wr = reduced_dim(W, reduce);
    const int y0 = t.y0 ? t.y0[k] : 0, x0 = t.x0 ? t.x0[k] : 0;
    // (a NULL extent with an origin outside the image: the box is empty or negative, refused below)
    const int hs = t.hs ? t.hs[k] : (int)std::max<long>((long)Hr - y0, -1), ws = t.ws ? t.ws[k] : (int)std::max<long>((long)Wr - x0, -1);
    if (hs < 1 || ws < 1) return fail(LLICTI_EINVAL, "%s: the box of %s is %dx%d (need hs, ws >= 1)", who, whose, ws, hs);
    if (!resize_window_ok(H, W, reduce, y0, x0, hs, ws, t.Ho, t.Wo, 0))
        return fail(LLICTI_EINVAL, "%s: the %dx%d box at (y %d, x %d) leaves %s (%dx%d at reduce %d)", who, ws, hs, y0, x0, whose, Wr, Hr, reduce);
    if (!resize_window_ok(H, W, reduce, y0, x0, hs, ws, t.Ho, t.Wo, t.antialias))
        return fail(LLICTI_EINVAL, "%s: the %dx%d box of %s shrinks to %dx%d by more than 4 on an axis; the filter (antialias = 1) takes scales up to 4: "
                    "raise reduce (every step halves the box), or pass antialias = 0", who, ws, hs, whose, t.Wo, t.Ho);
    words[0] = tensor_win_pack(y0, x0, t.flip && t.flip[k]);
    words[1] = resize_ext_pack(hs, ws);
    return 0;
}
static int resolve_resize(const char *who, int B, const int *Hs, const int *Ws, const Reduces &rd, const ResizeArgs &t, std::vector<uint32_t> &boxes, TensorNorm &nm)
{
    if (int rc = resolve_resize_head(who, rd, t, nm)) return rc;
    boxes.assign(2 * (size_t)B, 0u);
    for (int b = 0; b < B; ++b) {
        char whose[32];
        snprintf(whose, sizeof whose, "image %d", b);
        if (int rc = resolve_resize_box(who, whose, Hs[b], Ws[b], rd.of(b), t, b, &boxes[2 * (size_t)b])) return rc;
    }
    return 0;
}

// Views (llicti_decode_images_tensor_views): the call's groups as the caller gave them ...
struct ViewArgs { const llicti_view_group *groups; int G; const float *mean, *std; };
// ... and one validated group: three packed words per view (ViewSlice), kernel arguments of the group's launches like the boxes above
struct ViewGroupOut { void *d_out; int dtype, Ho, Wo, antialias, n; std::vector<uint32_t> words; };
// Every view is held to resolve_resize's rules against the image it names (resolve_resize_head, resolve_resize_box: the same functions, the
// same words); a refusal names the group and the view.  A view is held against the reduce of the image it names.
static int resolve_views(const char *who, int B, const int *Hs, const int *Ws, const Reduces &rd, const ViewArgs &a, std::vector<ViewGroupOut> &out, TensorNorm &nm)
{
    if (a.G < 1 || a.G > LLICTI_VIEW_GROUPS_MAX) return fail(LLICTI_EINVAL, "%s: %d groups (need 1 .. %d)", who, a.G, LLICTI_VIEW_GROUPS_MAX);
    if (!a.groups) return fail(LLICTI_EINVAL, "%s: null groups", who);
    out.assign((size_t)a.G, ViewGroupOut());
    for (int g = 0; g < a.G; ++g) {
        const llicti_view_group &vg = a.groups[g];
        char whose[80];
        snprintf(whose, sizeof whose, "%s: group %d", who, g);
        if (!vg.d_out) return fail(LLICTI_EINVAL, "%s: null d_out", whose);
        if (vg.n < 1 || vg.n > kViewCountMax) return fail(LLICTI_EINVAL, "%s: n = %d views (need 1 .. %d)", whose, vg.n, kViewCountMax);
        if (!vg.image && vg.n != B) return fail(LLICTI_EINVAL, "%s: image = NULL means view v is image v: n = %d, the batch has %d images", whose, vg.n, B);
        const ResizeArgs t{ vg.dtype, vg.Ho, vg.Wo, vg.y0, vg.x0, vg.hs, vg.ws, vg.flip, a.mean, a.std, vg.antialias };
        if (int rc = resolve_resize_head(whose, rd, t, nm)) return rc;
        ViewGroupOut &o = out[(size_t)g];
        o.d_out = vg.d_out; o.dtype = vg.dtype; o.Ho = vg.Ho; o.Wo = vg.Wo; o.antialias = vg.antialias; o.n = vg.n;
        o.words.assign(3 * (size_t)vg.n, 0u);
        for (int v = 0; v < vg.n; ++v) {
            const int b = vg.image ? vg.image[v] : v;
            if (b < 0 || b >= B) return fail(LLICTI_EINVAL, "%s: view %d of group %d names image %d (the batch has images 0 .. %d)", who, v, g, b, B - 1);
            snprintf(whose, sizeof whose, "view %d of group %d (image %d)", v, g, b);
            if (int rc = resolve_resize_box(who, whose, Hs[b], Ws[b], rd.of(b), t, v, &o.words[3 * (size_t)v])) return rc;
            o.words[3 * (size_t)v + 2] = (uint32_t)b;
        }
    }
    return 0;
}

// mode: 0 = AC container (torchac-compatible, the reference's format); 0x100 | M = rANS container (v3) with M
// streams per image, M in 1 .. 32 (one per container segment) or {64, 128} (latency modes: 2 / 4 streams per segment)
static int mode_streams(int mode)      // -> M, | 0x100 for wide streams (LLICTI_MODE_RANS_WIDE), | 0x200 for xwide streams (LLICTI_MODE_RANS_X); 0: AC container; -1: unknown
{
    if (mode == 0) return 0;
    const int M = mode & 0xFF;
    if ((mode & ~0xFF) == 0x500) return ((M >= 1 && M <= 32) || M == 64 || M == 128) ? (M | 0x200) : -1;
    if ((mode & ~0xFF) == (0x500 | 0x10000)) return (M >= 1 && M <= 32) ? (M | 0x200 | 0x1000) : -1;      // LLICTI_MODE_RANS_X_AUTO(M): encode only
    if ((mode & ~0xFF) == 0x300) return (M >= 1 && M <= 14) ? (M | 0x100) : -1;
    if ((mode & ~0xFF) != 0x100) return -1;
    if (M < 1 || (M > 32 && M != 64 && M != 128)) return -1;
    return M;
}
static int ilog2(int v) { int l = 0; while ((1 << l) < v) ++l; return l; }
// Header byte 0 of a rANS container (the AC container stores the number of scales, 5, there): bit 7 = rANS, bit 3 = format v3 or later (the
// retired v2 had it clear), bit 6 = extended, bits 5,4,2,1,0 = a 5-bit value v:  M = v + 1 (1 .. 32 streams of 64 lanes, one per segment);
// extended: v = 0, 1: 64 / 128 streams of 64 lanes (M / 32 per segment); v = 2 .. 15: v - 1 wide streams (128 lanes); v = 16: xwide streams
// (256 lanes) in the v4 layout, whose COUNT is in bits 10 .. 15 of the int16 pad field (rans_pad_hi(); those bits are zero in every other
// container, so a reader of the older formats finds a pad field that contradicts the size and refuses).  v = 17 .. 31 were the xwide tags of
// the v3 layout (rounds 4-5): retired, refused.
// Config B (2 levels) writes xwide v4 only, with v = 17 (byte 0 = 0xE9): a tag no reader of config A's containers accepts, so that a container
// names the model that wrote it (config A's bytes are untouched).  Its pad field holds 4 pad bits and the count (bits 4 .. 9 zero).
static int rans_byte0(int M, int Q, int nlev)
{
    if (nlev == kLevelsB && Q == 4) return 0xE9;
    const int ext = (M > 32 || Q > 1) ? 1 : 0;
    const int v = Q == 4 ? 16 : Q == 2 ? M + 1 : M > 32 ? (M == 64 ? 0 : 1) : M - 1;
    return 0x88 | (ext << 6) | (((v >> 3) & 3) << 4) | (v & 7);
}
static int rans_pad_hi(int M, int Q) { return Q == 4 ? (M <= 32 ? M : M == 64 ? 33 : 34) : 0; }      // bits 10 .. 15 of the pad field
// -> M (| 0x100 for wide, | 0x200 for xwide streams) of a header's byte 0 and pad field; 0: not a rANS container this build reads
static int rans_streams_of_header(int b0, int padfield)
{
    if ((b0 & 0x88) != 0x88) return 0;
    const int v = (((b0 >> 4) & 3) << 3) | (b0 & 7), u = (padfield >> 10) & 0x3F;
    if (((b0 >> 6) & 1) && v >= 16) {
        if (v != 16 || u < 1 || u > 34) return 0;             // (v3's xwide tags, or no count)
        return (u <= 32 ? u : u == 33 ? 64 : 128) | 0x200;
    }
    if (u) return 0;
    if (!((b0 >> 6) & 1)) return v + 1;
    if (v <= 1) return 64 << v;
    return (v - 1) | 0x100;
}

// Levels of the model that wrote a header (5: config A, 2: config B), 0: not a container this build reads.  The AC container stores the number
// of scales in byte 0 (the reference: LLICTI_nets.py:347); config B's pad field has 4 bits, and its rANS containers the tag 0xE9 (rans_byte0).
static int header_levels(int b0, int padfield)
{
    if (b0 == LLICTI_NLEVELS) return LLICTI_NLEVELS;
    if (b0 == kLevelsB) return (padfield >> (2 * kLevelsB)) == 0 ? kLevelsB : 0;
    if (b0 == 0xE9) return ((padfield & 0x3F0) == 0 && rans_streams_of_header(0xE8, padfield) != 0) ? kLevelsB : 0;
    return rans_streams_of_header(b0, padfield) ? LLICTI_NLEVELS : 0;
}
// rans_streams_of_header of either model's tags
static int header_streams(int b0, int padfield) { return rans_streams_of_header(b0 == 0xE9 ? 0xE8 : b0, padfield); }
// the modes a model's whole-batch calls take: config A every one; config B the reference format and xwide v4 streams, at most 9 L = 18 per image
// (one per container segment; "auto" counts whose largest pick stays within that)
static bool model_takes(int nlev, int ME)
{
    if (nlev == LLICTI_NLEVELS || (ME & 0xFF) == 0) return true;
    const int M = ME & 0xFF;
    return ((ME >> 8) & 3) == 2 && ((ME & 0x1000) ? rans_auto_hi(M) : M) <= 9 * nlev;
}

static int check_dims_v(int B, const int *Hs, const int *Ws)
{
    if (B < 1 || !Hs || !Ws) return fail(LLICTI_EINVAL, "bad batch: B=%d (need B>=1 and the sizes of every image)", B);
    for (int b = 0; b < B; ++b)
        if (Hs[b] < 32 || Ws[b] < 32 || Hs[b] > 8160 || Ws[b] > 8160) return fail(LLICTI_EINVAL, "bad shape of image %d: H=%d W=%d (need 32<=H,W<=8160)", b, Hs[b], Ws[b]);
    return 0;
}
// ------------------------------------------------------------------------------------------------ admission
// What the whole-batch calls refuse before they take a plan, each rule stated once: the entry points (llicti_hip.hip) report the reason, the size
// queries below turn a refusal into 0 (the reason stays in llicti_last_error).  who: the caller's name, in front of every message.
//
// modes: one container mode for the call (n_modes = 1) or one per image (n_modes = B: rANS containers of ONE lane kind whose stream counts may differ,
// fixed and "auto" xwide counts mixed); -> ME of the call (the lane kind, with the first image's count, | 0x1000 if any image is "auto") and, for
// per-image modes that differ, Ms (count | 0x1000 for an "auto" image: PlanSpec)
static int resolve_modes(const char *who, const int *modes, int n_modes, int B, int *ME_out, std::vector<int> &Ms)
{
    Ms.clear();
    if (!modes || (n_modes != 1 && n_modes != B)) return fail(LLICTI_EINVAL, "%s: modes must hold one mode or one per image", who);
    const int ME0 = mode_streams(modes[0]);
    if (ME0 < 0) return fail(LLICTI_EINVAL, "%s: unknown mode 0x%x", who, modes[0]);
    *ME_out = ME0;
    if (n_modes == 1) return 0;
    bool differ = false, any_auto = false;
    for (int b = 0; b < B; ++b) {
        const int ME = mode_streams(modes[b]);
        if (ME < 0) return fail(LLICTI_EINVAL, "%s: unknown mode 0x%x of image %d", who, modes[b], b);
        if (((ME >> 8) & 3) != ((ME0 >> 8) & 3) || ((ME & 0xFF) == 0) != ((ME0 & 0xFF) == 0))
            return fail(LLICTI_EINVAL, "%s: the images of one call share a container kind (reference format, or rANS streams of one lane count); image %d differs", who, b);
        Ms.push_back(ME & 0x10FF);
        differ = differ || ME != ME0;
        any_auto = any_auto || (ME & 0x1000);
    }
    if (!differ) Ms.clear();
    else if (any_auto) *ME_out |= 0x1000;      // (the call runs the encoder's stream-count pick; images with Mlo = 0 keep their fixed count)
    return 0;
}
// the container modes a model of nlev levels takes (model_takes)
static int check_model(int nlev, const char *who, int ME, const std::vector<int> &Ms)
{
    bool ok = model_takes(nlev, ME);
    for (int m : Ms) ok = ok && model_takes(nlev, (ME & 0x300) | m);
    if (!ok)
        return fail(LLICTI_EINVAL, "%s: a %d-level model (config B) codes the reference-format container or xwide v4 streams, at most %d per image "
                    "(\"auto\": a size-rule count of at most 13)", who, nlev, 9 * nlev);
    return 0;
}
// a decoder's or a transcode source's modes name containers that exist: no "auto" (resolve_modes sets ME's 0x1000 if any image's mode has it)
static int check_source_modes(const char *who, const char *container, int ME)
{
    if (ME & 0x1000)
        return fail(LLICTI_EINVAL, "%s: LLICTI_MODE_RANS_X_AUTO is an encoder's mode -- a %s says how many streams it has (header: llicti_header_mode)", who, container);
    return 0;
}
// config B's header stores the last level's grid in one byte per side (config A's sizes, at most 8160, always fit)
static int check_header_grid(const char *who, int nlev, int B, const int *Hs, const int *Ws)
{
    if (nlev >= LLICTI_NLEVELS) return 0;
    for (int b = 0; b < B; ++b) {
        const Geom gl = make_geom(1, Hs[b], Ws[b], nlev - 1);
        if (gl.h > 255 || gl.w > 255)
            return fail(LLICTI_EINVAL, "%s: image %d is %dx%d; a %d-level model's header stores its level-%d grid (%dx%d) in one byte each "
                        "(at most %d pixels per side)", who, b, Ws[b], Hs[b], nlev, nlev - 1, gl.w, gl.h, 255 << nlev);
    }
    return 0;
}
// The rANS coders keep a stream's bit position in a signed 32-bit word (the encoder's cursor, rans_init_kernel's top and cur, the stage decoders'
// rpos): a stream's slot -- its worst case, rans_slot_bytes -- stays below 2^28 bytes = 2^31 bits.  An "auto" image is bounded at the fewest
// streams its encoder may pick.  Only one-stream calls on images of about 45 M pixels reach it (8,160 wide: from 5,488 rows); two streams hold 8160x8160.
constexpr long kRansSlotMax = 1L << 28;
static int check_stream_bits(const char *who, int nlev, int B, const int *Hs, const int *Ws, int ME, const std::vector<int> &Ms)
{
    if ((ME & 0xFF) == 0) return 0;
    const int Q = 1 << ((ME >> 8) & 3);
    for (int b = 0; b < B; ++b) {
        const int m = Ms.empty() ? (ME & 0x10FF) : Ms[b];
        const int M = m & 0xFF, Mfew = (m & 0x1000) ? rans_auto_min(M) : M;
        const long need = rans_slot_bytes(nlev, Hs[b], Ws[b], Mfew, Q);
        if (need < kRansSlotMax) continue;
        int fit = Mfew + 1;
        while (rans_slot_bytes(nlev, Hs[b], Ws[b], fit, Q) >= kRansSlotMax) ++fit;
        return fail(LLICTI_EINVAL, "%s: image %d is %dx%d; in %d stream%s%s one stream may take %ld bytes, and a stream's bit position is a signed 32-bit word "
                    "(fewer than 2^28 = %ld bytes per stream): the smallest count that fits is %d", who, b, Ws[b], Hs[b], Mfew, Mfew == 1 ? "" : "s",
                    (m & 0x1000) ? " (the fewest an \"auto\" encode may pick)" : "", need, kRansSlotMax, fit);
    }
    return 0;
}
// every container slot of a decode holds at least its image's header
static int check_in_stride(const char *who, int nlev, int B, const int *Hs, const int *Ws, size_t in_stride)
{
    for (int b = 0; b < B; ++b) {
        const int hdr = header_bytes(Hs[b], Ws[b], nlev);
        if (in_stride < (size_t)hdr)
            return fail(LLICTI_EINVAL, "%s: in_stride %zu is smaller than the %d header bytes of a %dx%d image", who, in_stride, hdr, Ws[b], Hs[b]);
    }
    return 0;
}
// a transcode of images that differ in size (ragged: or that llicti_set_tuning("force_ragged") places as if they did) has no reference-format side
static int check_transcode_sizes(const char *who, int B, const int *Hs, const int *Ws, int MEs, int MEd, bool ragged)
{
    bool mixed = ragged;
    for (int b = 1; b < B; ++b) mixed = mixed || Hs[b] != Hs[0] || Ws[b] != Ws[0];
    if (mixed && ((MEs & 0xFF) == 0 || (MEd & 0xFF) == 0))
        return fail(LLICTI_EINVAL, "%s: a batch of mixed sizes needs rANS containers on both sides (the reference-format container codes equal sizes per call)", who);
    return 0;
}
// Everything llicti_transcode_images refuses on sizes and modes alone -> (MEs, Mss) of the source side, (MEd, Msd) of the target side
static int admit_transcode(int nlev, bool ragged, int B, const int *Hs, const int *Ws, const int *src_modes, int n_src, const int *dst_modes, int n_dst,
                           int *MEs, std::vector<int> &Mss, int *MEd, std::vector<int> &Msd)
{
    if (check_dims_v(B, Hs, Ws)) return LLICTI_EINVAL;
    if (int rc = resolve_modes("transcode_images (source)", src_modes, n_src, B, MEs, Mss)) return rc;
    if (int rc = check_model(nlev, "transcode_images (source)", *MEs, Mss)) return rc;
    if (int rc = check_source_modes("transcode_images", "source container", *MEs)) return rc;
    if (int rc = check_stream_bits("transcode_images (source)", nlev, B, Hs, Ws, *MEs, Mss)) return rc;
    if (int rc = resolve_modes("transcode_images (target)", dst_modes, n_dst, B, MEd, Msd)) return rc;
    if (int rc = check_model(nlev, "transcode_images (target)", *MEd, Msd)) return rc;
    if (int rc = check_stream_bits("transcode_images (target)", nlev, B, Hs, Ws, *MEd, Msd)) return rc;
    if (int rc = check_transcode_sizes("transcode_images", B, Hs, Ws, *MEs, *MEd, ragged)) return rc;
    return check_header_grid("transcode_images", nlev, B, Hs, Ws);
}

// ------------------------------------------------------------------------------------------------ per-image reduce
// The _rv calls (llicti_decode_images_reduced_rv and its four kin): image b stops at its OWN level reduces[b].  The cached plan is the batch's
// full-size one with tight placement -- it does not depend on the values -- and everything that does is PER CALL data, built here: the r table,
// the reduced output table (or the pixel windows), for each level the streams of the images that take part in it (r_b <= lvl), and for each
// (level, band) the band CNN's tile list over those images with its TileRun (form chosen over the ACTIVE images: choose_tile_form).  The call
// copies the tables into one pooled block, uploads it with one asynchronous copy and hands the block back behind its last kernel; none of it
// enters the plan cache.
//
// What the calls refuse on the values alone: a null array, a value outside 0 .. nlev (naming the image), and differing values with a
// reference-format container (ME's count is 0), whose pipeline codes equal sizes and one schedule per call.
static int admit_reduces(const char *who, int B, const int *reduces, int nlev, int ME)
{
    if (!reduces) return fail(LLICTI_EINVAL, "%s: null reduces (one value per image)", who);
    for (int b = 0; b < B; ++b)
        if (reduces[b] < 0 || reduces[b] > nlev)
            return fail(LLICTI_EINVAL, "%s: reduces[%d] = %d of image %d (a %d-level model decodes at reduce 0 .. %d)", who, b, reduces[b], b, nlev, nlev);
    if ((ME & 0xFF) == 0)
        for (int b = 1; b < B; ++b)
            if (reduces[b] != reduces[0])
                return fail(LLICTI_EINVAL, "%s: image %d has reduce %d, image 0 reduce %d -- a reference-format container codes one schedule per call "
                            "(per-image reduces need rANS containers)", who, b, reduces[b], reduces[0]);
    return 0;
}
static bool reduces_equal(int B, const int *reduces) { return std::all_of(reduces, reduces + B, [&](int v) { return v == reduces[0]; }); }
struct ReduceSchedule {
    int B = 0, nlev = 0, rmin = 0;
    std::vector<int> r;                   // [B]
    std::vector<RedGeo> red;              // [B]: every image's reduced size (its full one at r = 0) and where its planar output goes
    long max_rplane = 0;                  // largest Hr * Wr
    std::vector<int> streams;             // the levels' lists of active streams (indices into the plan's stream table, ascending), back to back
    size_t s_off[LLICTI_NLEVELS] = {};
    int s_n[LLICTI_NLEVELS] = {};
    std::vector<TileRef> tiles;           // the (level, band) tile lists, back to back; image-major, rows, columns -- build_plan's order
    TileRun run[LLICTI_NLEVELS * 3];      // n_tiles = 0: no image takes part in the level, nothing is launched
    std::vector<PixGeo> pix;              // the pixel call's windows (empty otherwise)
    long pix_units = 0;
    // the device block
    size_t d_r = 0, d_red = 0, d_streams = 0, d_tiles = 0, d_pix = 0, d_total = 0;
};
// p: the batch's plan (build_plan; its host tile list may be gone).  out_off: the planar outputs' byte offsets (nullptr: tight in call order, each
// image at its own reduced size).  pix: the pixel call's validated windows (resolve_pixels on the reduced sizes), or nullptr.
static void build_reduce_schedule(ReduceSchedule &q, const Plan &p, const int *reduces, const size_t *out_off, int n_cu, int tile_rows,
                                  const std::vector<PixGeo> *pix = nullptr)
{
    const int B = p.B, nlev = p.nlev;
    q = ReduceSchedule{};
    q.B = B; q.nlev = nlev;
    q.r.assign(reduces, reduces + B);
    q.rmin = Reduces::each(reduces).min(B);
    ReducedOut o = reduced_out(p.img, Reduces::each(reduces), out_off);
    q.red.swap(o.red);
    q.max_rplane = o.max_rplane; q.pix_units = o.pix_units;
    if (pix) q.pix = *pix;
    for (int lvl = nlev - 1; lvl >= q.rmin; --lvl) {
        q.s_off[lvl] = q.streams.size();
        for (int i = 0; i < p.nstreams; ++i) if (q.r[p.sref[(size_t)i].b] <= lvl) q.streams.push_back(i);
        q.s_n[lvl] = (int)(q.streams.size() - q.s_off[lvl]);
    }
    build_tile_lists(p.geo, B, nlev - 1, q.rmin - 1, [&](int b, int lvl) { return q.r[b] <= lvl; }, n_cu, tile_rows, q.tiles, q.run);
    size_t d = 0;
    auto dtake = [&](size_t bytes) { size_t r = d; d = align_up(d + bytes, 256); return r; };
    q.d_r = dtake(q.r.size() * sizeof(int));
    q.d_red = dtake(q.red.size() * sizeof(RedGeo));
    q.d_streams = dtake(q.streams.size() * sizeof(int));
    q.d_tiles = dtake(q.tiles.size() * sizeof(TileRef));
    q.d_pix = dtake(q.pix.size() * sizeof(PixGeo));
    q.d_total = std::max<size_t>(d, 256);
}
// the tables into the block's host side, at their offsets
static void write_reduce_schedule(const ReduceSchedule &q, uint8_t *h)
{
    auto put = [&](size_t off, const void *src, size_t n) { if (n) memcpy(h + off, src, n); };
    put(q.d_r, q.r.data(), q.r.size() * sizeof(int));
    put(q.d_red, q.red.data(), q.red.size() * sizeof(RedGeo));
    put(q.d_streams, q.streams.data(), q.streams.size() * sizeof(int));
    put(q.d_tiles, q.tiles.data(), q.tiles.size() * sizeof(TileRef));
    put(q.d_pix, q.pix.data(), q.pix.size() * sizeof(PixGeo));
}

// ------------------------------------------------------------------------------------------------ size queries
// modes: one mode (n_modes = 1) or one per image (rANS containers of one lane kind, stream counts may differ)
static size_t plan_workspace_bytes_vm(int B, const int *Hs, const int *Ws, const int *modes, int n_modes, int nlev = LLICTI_NLEVELS)
{
    int ME = 0;
    std::vector<int> Ms;
    if (check_dims_v(B, Hs, Ws) || resolve_modes("workspace_bytes", modes, n_modes, B, &ME, Ms) || check_stream_bits("workspace_bytes", nlev, B, Hs, Ws, ME, Ms)) return 0;
    Plan p, q;
    build_plan(p, PlanSpec{ B, Hs, Ws, ME, modes_ptr(Ms), nlev, false });
    build_plan(q, PlanSpec{ B, Hs, Ws, ME, modes_ptr(Ms), nlev, true });      // (llicti_set_tuning("force_ragged"): image blocks at 64-element boundaries)
    return std::max(p.total, q.total);
}
static size_t plan_workspace_bytes_v(int B, const int *Hs, const int *Ws, int mode) { return plan_workspace_bytes_vm(B, Hs, Ws, &mode, 1); }
static size_t plan_workspace_bytes(int B, int H, int W, int mode)
{
    if (check_dims(B, H, W)) return 0;
    std::vector<int> Hs(B, H), Ws(B, W);
    return plan_workspace_bytes_v(B, Hs.data(), Ws.data(), mode);
}
static size_t plan_max_container_bytes(int H, int W, int nlev = LLICTI_NLEVELS)
{
    if (check_dims(1, H, W)) return 0;
    // the reference format; M <= 32; the many-stream latency modes (more per-stream slack); wide and xwide streams (larger state blocks)
    size_t most = 0;
    for (int ME : { 0, 32, kRansMaxStreams, 14 | 0x100, 128 | 0x200 }) {
        Plan p;
        build_plan(p, PlanSpec{ 1, &H, &W, ME, nullptr, nlev });
        most = std::max(most, p.max_container);
    }
    return most;
}

static int plan_header_dims(const uint8_t *h, int *H, int *W)
{
    if (!h || !H || !W) return fail(LLICTI_EINVAL, "header_dims: null pointer");
    if ((h[0] & 0x88) == 0x80)
        return fail(LLICTI_EFORMAT, "header: byte 0 = 0x%02x is the retired LLICTI-rANS v2 container; this build reads and writes v3 only", h[0]);
    const int nlev = header_levels(h[0], (int)(uint16_t)(h[15] | (h[16] << 8)));
    if (nlev == 0)
        return fail(LLICTI_EFORMAT, "header: byte 0 = 0x%02x (pad field 0x%04x) is neither %d / %d scales (AC container of config A / B) nor a rANS container tag of this build "
                    "(the xwide v3 layout of rounds 4-5 is retired)", h[0], (unsigned)(h[15] | (h[16] << 8)), LLICTI_NLEVELS, kLevelsB);
    int Hc = h[1], Wc = h[2];
    int pad = (int)(int16_t)(h[15] | (h[16] << 8));
    for (int l = nlev - 1; l >= 0; --l) {     // _get_padHW_lev_list, LLICTI_nets.py:533-542
        const int padW = pad & 1; pad >>= 1;
        const int padH = pad & 1; pad >>= 1;
        Hc = 2 * Hc - padH;
        Wc = 2 * Wc - padW;
    }
    *H = Hc; *W = Wc;
    return LLICTI_OK;
}

// ------------------------------------------------------------------------------------------------ transcode
// llicti_transcode_images runs the decoder of the source containers and the entropy-coder back end of the target ones in ONE call, on two
// plans of the same batch (sizes, tight placement) that differ in their container modes: the caller's workspace is [source plan | target plan],
// each part laid out as for a call of its own.  The decoder's planes, min/max words and CNN outputs stay where the source plan puts them; the
// target's kernels (cdf_pairs_kernel behind every stage, the rANS coder's seed symbols) address them through the TARGET plan's tables -- so
// the two plans must place every image's planes and CNN outputs identically, which they do because both are functions of the sizes and the
// `uniform` form alone (tests/sanitize_transcode_host.cpp checks it over random batches; the call checks it again, it costs nothing).
struct TranscodeLayout { size_t off_dst = 0, total = 0; };
static TranscodeLayout transcode_layout(const Plan &src, const Plan &dst)
{
    TranscodeLayout t;
    t.off_dst = align_up(src.total, 256);
    t.total = t.off_dst + dst.total;
    return t;
}
static bool transcode_plans_agree(const Plan &src, const Plan &dst)
{
    if (src.B != dst.B || src.nlev != dst.nlev || src.uniform != dst.uniform) return false;
    const int B = src.B;
    for (int b = 0; b < B; ++b) {
        const ImgGeo &a = src.img[b], &d = dst.img[b];
        if (a.H != d.H || a.W != d.W || a.plane != d.plane || a.pix_off != d.pix_off || a.h4 != d.h4 || a.w4 != d.w4 || a.dcs != d.dcs || a.hdr_bytes != d.hdr_bytes) return false;
    }
    for (int lvl = 0; lvl < src.nlev; ++lvl) {
        if (src.lev_maxpos[lvl] != dst.lev_maxpos[lvl]) return false;
        for (int b = 0; b < B; ++b) {
            const Geom &a = src.geo[(size_t)lvl * B + b], &d = dst.geo[(size_t)lvl * B + b];
            if (a.pix_off != d.pix_off || a.par_off != d.par_off || a.h != d.h || a.w != d.w) return false;
            for (int band = 0; band < 3; ++band) {
                const StageGeom &sa = src.sg[(size_t)(lvl * 3 + band) * B + b], &sd = dst.sg[(size_t)(lvl * 3 + band) * B + b];
                if (sa.img_off != sd.img_off || sa.par_off != sd.par_off || sa.hc != sd.hc || sa.wc != sd.wc || sa.plane != sd.plane) return false;
            }
        }
    }
    return true;
}
// Bytes of workspace llicti_transcode_images needs; 0: a combination it refuses (bad sizes or modes, an "auto" mode as the source, mixed lane
// kinds on a side, a mode the model does not take, the reference format on either side with images of different sizes).
static size_t plan_transcode_workspace_bytes(int B, const int *Hs, const int *Ws, const int *src_modes, int n_src, const int *dst_modes, int n_dst,
                                             int nlev = LLICTI_NLEVELS)
{
    int MEs = 0, MEd = 0;
    std::vector<int> Mss, Msd;
    if (admit_transcode(nlev, false, B, Hs, Ws, src_modes, n_src, dst_modes, n_dst, &MEs, Mss, &MEd, Msd)) return 0;
    size_t total = 0;
    for (int ragged = 0; ragged < 2; ++ragged) {      // (llicti_set_tuning("force_ragged"): image blocks at 64-element boundaries)
        Plan s, d;
        build_plan(s, PlanSpec{ B, Hs, Ws, MEs, modes_ptr(Mss), nlev, ragged != 0 });
        build_plan(d, PlanSpec{ B, Hs, Ws, MEd, modes_ptr(Msd), nlev, ragged != 0 });
        total = std::max(total, transcode_layout(s, d).total);
    }
    return total;
}

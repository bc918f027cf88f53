// rans_coder.hpp -- LLICTI-rANS v3 container: what the 64- or 128-way interleaved, bit-granular rANS encoder (rans_encode.hpp), the tail decoder
// (rans_tail.hpp) and the decoders here share, init, the table-free stage decoders, pack and unpack.  Part of the single translation unit llicti_hip.hip (included in order; not a stand-alone header).
#pragma once
#include <type_traits>

#include "prove_symbol.hpp"

// ------------------------------------------------------------------------------------------------ rANS container
// "LLICTI-rANS v3" (format of this build; BASELINE.json north_star: "torchac replaced by a HIP rANS coder"; spec and CPU
// restatement: oracle/llicti_oracle.h / .c).  Same CDFs and symbols as the AC container; each image has M independent
// streams, each an L-way interleaved rANS coder (L = 64 lanes, or 128 for wide streams) encoded by ONE wavefront: lane l of stream m
// codes symbol n = Lc + l of every chunk c = m (mod M) of every stage, so a whole stage decodes in ceil(nc / LM) steps.
// What v3 changes against v2 (16-bit words, states in [2^16, 2^32), ~60 bytes of start / flush overhead per stream):
//   * states live in [2^31, 2^32) and renormalise BIT by bit (0..16 bits per symbol): x / freq >= 2^15, so the coder loses
//     ~2^-16 of a symbol's length like the range coder does (v2 lost ~0.005 bpp on smooth content), and a final state is
//     31 bits flat -- no length field;
//   * a lane's INITIAL state carries payload instead of nothing: the last T symbols of the stream's last stage are coded by a
//     single-state "tail" coder whose output (<= 31 L bits) is cut into the L x 31 bits the lanes start from.  The decoder
//     is left with those states after the last stage, reassembles the tail stream and decodes its T symbols serially.
// Cost over the ideal code length: ~6 bytes per stream (v2: ~60) -- ten streams are within 0.001 bpp of the AC container.
// Stream bytes:  u16 (T | pad << 11) | bit region, read DOWN from its top minus pad unused bits | L x 31-bit final states.

__device__ __forceinline__ int lanes_below(uint64_t mask)
{
    return (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
}

// inclusive prefix sum over the 64 lanes (DPP: row_shr 1, 2, 4, 8 inside each row of 16, then row_bcast 15 / 31)
__device__ __forceinline__ int wave_incl_scan(int v)
{
    v += __builtin_amdgcn_update_dpp(0, v, 0x111, 0xF, 0xF, true);
    v += __builtin_amdgcn_update_dpp(0, v, 0x112, 0xF, 0xF, true);
    v += __builtin_amdgcn_update_dpp(0, v, 0x114, 0xF, 0xF, true);
    v += __builtin_amdgcn_update_dpp(0, v, 0x118, 0xF, 0xF, true);
    v += __builtin_amdgcn_update_dpp(0, v, 0x142, 0xA, 0xF, false);      // lane 15 of rows 0 / 2 -> rows 1 / 3
    v += __builtin_amdgcn_update_dpp(0, v, 0x143, 0xC, 0xF, false);      // lane 31 -> rows 2, 3
    return v;
}

// n bits (0 <= n <= 32) at bit position pos of a little-endian dword array in LDS
__device__ __forceinline__ uint32_t lds_get_bits(const uint32_t *buf, int pos, int n)
{
    const uint64_t w = (uint64_t)buf[pos >> 5] | ((uint64_t)buf[(pos >> 5) + 1] << 32);
    return (uint32_t)(w >> (pos & 31)) & (uint32_t)((1ull << n) - 1ull);
}
__device__ __forceinline__ void lds_or_bits(uint32_t *buf, int pos, int n, uint32_t v)     // v < 2^n
{
    if (n == 0) return;
    atomicOr(&buf[pos >> 5], v << (pos & 31));
    if ((pos & 31) + n > 32) atomicOr(&buf[(pos >> 5) + 1], v >> (32 - (pos & 31)));
}

// the image's stream count (the encoder and rans_pack_kernel ask): the table's (fixed by the caller), or -- "auto" -- what rans_auto_pick makes of
// the size rule's count and choose_streams_kernel's sum (rans_encode.hpp)
__device__ __forceinline__ int image_stream_count(const unsigned long long *ssum, const ImgGeo *iv, const StreamDesc *desc, int B, int b, int M_table)
{
    if (!ssum) return M_table;
    const int Mlo = iv[b].Mlo;
    return Mlo ? rans_auto_pick(Mlo, (long long)ssum[b], (long long)desc[(long)(LLICTI_NSTREAMS - 1) * B + b].n) : M_table;
}

// decode: parse a stream (copied by rans_unpack_kernel so that its bit region starts at slot + 4, dword aligned; its validated length is in rpos):
// T and the bit cursor, the 64 Q states.  64 / 128 lanes: u16 (T | pad << 11) | bit region | states.  xwide v4: bit region | states, the
// region's highest set bit its end marker, the 9 bits below it the header field (T / 32 rounded up -- T = min(32 field, the stream's share of
// the last stage) -- and the one-chain flag), the main coder's bits below that.
template <int Q>
__global__ __launch_bounds__(64) void rans_init_kernel(const uint8_t *__restrict__ slots, const long *__restrict__ rslot_off,
                                                       const StreamRef *__restrict__ sref, uint32_t *__restrict__ rstate, uint32_t *__restrict__ rpos,
                                                       uint32_t *__restrict__ rtail, int32_t *status, const StageGeom *__restrict__ sglv)
{
    using GEO = RansGeo<Q>;
    const int sidx = blockIdx.x, lane = threadIdx.x;
    const uint8_t *slot = slots + rslot_off[sidx];
    const int n = (int)rpos[sidx];                                 // >= GEO::kMinStream
    bool bad = false;
    int T = 0, single = 0, cur = 0, nbytes;
    if constexpr (kSeeded<Q>) {
        nbytes = n - GEO::kPayBytes;                               // >= 2
        const uint8_t *reg = slot + 4;
        const int lastb = reg[nbytes - 1];
        const int top = 8 * (nbytes - 1) + 31 - __clz(lastb | 1);      // the end marker
        if (lastb == 0 || top < 9) bad = true;
        else {
            const int p0 = top - 9;
            const uint32_t w = (uint32_t)reg[p0 >> 3] | ((uint32_t)reg[(p0 >> 3) + 1] << 8) | ((uint32_t)reg[min((p0 >> 3) + 2, nbytes - 1)] << 16);
            const uint32_t f9 = (w >> (p0 & 7)) & 0x1FFu;
            const StreamRef sr_ = sref[sidx];
            const StageGeom sgl = sglv[sr_.b];                     // the image's last stage: a tail is at most the stream's share of it
            T = min(kRansTailBlock * (int)(f9 & 0xFFu), rans_stream_count(sgl.hc * sgl.wc, sr_.m, sr_.M, GEO::kLanes));
            single = (int)(f9 >> 8);
            cur = p0;
        }
    } else {
        const int t16 = slot[2] | (slot[3] << 8);
        T = t16 & 0x7FF;
        nbytes = n - 2 - GEO::kPayBytes;
        const int pad = (t16 >> 11) & 7;
        if ((t16 >> 14) || nbytes < 0 || (nbytes == 0 && pad)) { bad = true; T = 0; nbytes = max(nbytes, 0); }
        else if (pad && (slot[4 + nbytes - 1] >> (8 - pad))) { bad = true; T = 0; }      // the unused bits on top of the region's last byte are zero
        cur = bad ? 0 : 8 * nbytes - pad;
    }
    const uint8_t *fs = slot + 4 + nbytes;
#pragma unroll
    for (int qq = 0; qq < Q; ++qq) {
        const int bpos = kRansStateBits * (64 * qq + lane);
        uint64_t w = 0;
#pragma unroll
        for (int k = 0; k < 5; ++k) w |= (uint64_t)fs[min((bpos >> 3) + k, GEO::kPayBytes - 1)] << (8 * k);
        rstate[((long)sidx * Q + qq) * 64 + lane] = (1u << 31) | ((uint32_t)(w >> (bpos & 7)) & 0x7FFFFFFFu);
    }
    if (lane == 0) { rpos[sidx] = (uint32_t)cur; rtail[sidx] = (uint32_t)T | ((uint32_t)single << 16); }
    if (bad && lane == 0) flag_image(status, sref[sidx].b, LLICTI_EFORMAT);
}

// One stage (level, band, colour channel) of all images.  One workgroup of 4 wavefronts per stream (one per
// SIMD: with the stage VALU-issue bound, the busiest SIMD sets the pace, so waves per workgroup is a multiple
// of 4).  Every wave keeps its own copy of the 64 rANS states (the update is cheap and identical in all of
// them), so a step needs ONE barrier.  A wave resolves 16 of the step's 64 symbols, 4 lanes per symbol: every lane of a
// group holds all five mixture components and probes its own table entry.  The symbol is first located with a CHEAP
// approximate CDF (Abramowitz-Stegun 7.1.26 erfc on v_rcp / v_exp, ~0.01 table counts of error) by 5-ary search, then
// PROVEN with the exact spec arithmetic: entry[s] <= slot < entry[s+1] is checked with cdf_entry()'s operations, and if
// the guess is off the exact search gallops away from it and bisects -- so the result is bit-identical to an exact
// search whatever the approximation does.  The 64 (c_low, c_high) pairs meet in a ping-pong LDS buffer, after which
// every wave updates its state copy and renormalises it bit-granularly: lane l needs clz(x) bits, a wave prefix sum
// places them in the stream (read DOWN: the encoder wrote upwards), pulled from a 128-dword register window.
// No table in HBM.
constexpr int kRansWaves = 4;

// (((tA0 + tA1) + tA2) + tA3) + tB3 of the 4-lane group starting at this lane (meaningful in the group's first lane)
__device__ __forceinline__ float dpp_sum5(float tA, float tB)
{
    float acc = tA + dpp_row_shl(tA, 1);
    acc = acc + dpp_row_shl(tA, 2);
    acc = acc + dpp_row_shl(tA, 3);
    acc = acc + dpp_row_shl(tB, 3);
    return acc;
}
__device__ __forceinline__ float quad_lane0(float v)    // broadcast lane (l & ~3) to its quad
{
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x00, 0xF, 0xF, true));   // quad_perm [0,0,0,0]
}

template <int J>
__device__ __forceinline__ float quad_bcast(float v)     // broadcast lane (l & ~3) + J to its quad
{
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), J * 0x55, 0xF, 0xF, true));   // quad_perm [J,J,J,J]
}

// exact table entry i (numerics spec); valid in the group's first lane.  erfc_spec_nobranch returns the same
// bits as erfc_spec (the saturation test selects the result instead of skipping the polynomial), which lets
// the two components' dependent chains interleave.
__device__ __forceinline__ uint32_t group_cdf_entry(const Comp &A, const Comp &B, const Grid &g, int i)
{
    const float pt = sample_pt(g, i);
    const float tA = mix_term(A.wn, A.mu, A.rsig, pt);
    const float tB = mix_term(B.wn, B.mu, B.rsig, pt);
    return entry_from_sum(dpp_sum5(tA, tB), g.scale, i);
}

// Approximate table entry i, 0 < i < Lp - 1 (search hint only -- never used as a result): Abramowitz-Stegun
// 7.1.26 erfc (|error| <= 1.5e-7) on v_rcp_f32 / v_exp_f32, with everything that does not depend on the sample
// point folded into per-component constants: x' = sqrt(log2 e) * x = c1 * pt + c0, exp(-x^2) = exp2(-x'^2),
// term = wh * erfc (wh = wn / 2).  15 vector operations per component and probe.
struct CompFast { float c1, c0, wh, wn; };
__device__ __forceinline__ CompFast comp_fast(const Comp &c)
{
    CompFast f;
    f.c1 = (kNegRsqrt2 * 1.2011224087864498f) * c.rsig;
    f.c0 = -c.mu * f.c1;
    f.wh = 0.5f * c.wn;
    f.wn = c.wn;
    return f;
}
__device__ __forceinline__ float term_fast(const CompFast &c, float pt)
{
    const float x = __builtin_fmaf(pt, c.c1, c.c0);
    const float a = __builtin_fabsf(x);
    const float u = __builtin_amdgcn_rcpf(__builtin_fmaf(0.3275911f / 1.2011224087864498f, a, 1.0f));
    float p = __builtin_fmaf(1.061405429f, u, -1.453152027f);
    p = __builtin_fmaf(p, u, 1.421413741f);
    p = __builtin_fmaf(p, u, -0.284496736f);
    p = __builtin_fmaf(p, u, 0.254829592f);
    const float E = ((p * u) * __builtin_amdgcn_exp2f(-(a * a))) * c.wh;
    return (x < 0.0f) ? c.wn - E : E;
}
// The same term read from a table of the normal CDF (llicti_ctx::d_phi_lut copied into LDS: Phi(z) on [-kPhiLutZ, kPhiLutZ] as (value,
// difference to the next) pairs, linear interpolation, error <= 1e-6): table coordinate by one fma with per-component constants, clamp,
// truncate, fract, one 8-byte LDS read, two fma -- 7 vector operations instead of 15 (two of them quarter-rate).  All three stage decoders'
// hints use it (rans_decode_stage_lane_kernel has the details and the measurements).
struct CompLut { float c1, c0, wn; };
__device__ __forceinline__ CompLut comp_lut(const Comp &c)
{
    constexpr float kS = kPhiLutN / (2.0f * (float)kPhiLutZ);
    CompLut f;
    f.c1 = c.rsig * kS;
    f.c0 = __builtin_fmaf(-c.mu, f.c1, (float)kPhiLutZ * kS);
    f.wn = c.wn;
    return f;
}
__device__ __forceinline__ float term_lut(const CompLut &c, float pt, const float2 *lut)
{
    // u in [0, kPhiLutN): v_med3_f32 returns one of its operands and v_cvt_u32_f32 turns a NaN into 0 -- the index stays inside the table
    const float u = __builtin_amdgcn_fmed3f(__builtin_fmaf(pt, c.c1, c.c0), 0.0f, (float)kPhiLutN - 0.0009765625f);
    const float2 e2 = lut[(uint32_t)u];
    return c.wn * __builtin_fmaf(e2.y, __builtin_amdgcn_fractf(u), e2.x);
}
__device__ __forceinline__ int group_cdf_entry_fast(const CompFast &A, const CompFast &B, float fbase, float scale, int i)
{
    const float pt = div255_exact(fbase + (float)i);     // the exact sample point: near a narrow component the CDF moves by counts per ulp of pt
    return (int)__builtin_rintf(dpp_sum5(term_fast(A, pt), term_fast(B, pt)) * scale) + i;
}

__global__ __launch_bounds__(64 * kRansWaves) void rans_decode_stage_kernel(const float *__restrict__ params, const StageGeom *__restrict__ sgv, const StreamRef *__restrict__ sref,
                                                               const float2 *__restrict__ phi_lut,
                                                               const uint8_t *__restrict__ slots, const long *__restrict__ rslot_off,
                                                               int rslot_cap, uint32_t *__restrict__ rstate, uint32_t *__restrict__ rpos,
                                                               const uint32_t *__restrict__ rtail,
                                                               int16_t *__restrict__ planes, float *__restrict__ fplanes,
                                                               const int32_t *__restrict__ minmax, int last_stage, int32_t *status,
                                                               const int *__restrict__ act = nullptr)
{
    __shared__ uint32_t sh_res[2][64][2];        // ping-pong by step parity: [0] = c_low, [1] = c_high
    __shared__ float2 sh_lut[kPhiLutN];          // the hint's normal CDF (term_lut)
    const int sidx = act ? act[blockIdx.x] : (int)blockIdx.x;      // (act: a per-image-reduce call's list of the level's streams, llicti_decode_images_*_rv)
    const StreamRef sr_ = sref[sidx];               // the stream's image, its index among the image's streams, the image's stream count (images of a call may differ)
    const int b = sr_.b, m = sr_.m, M = sr_.M;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const StageGeom sg = sgv[b];                 // the image's own stage geometry (the images of a call may differ in size)
    const int nc = sg.hc * sg.wc;
    const int nchunks = (nc + 63) >> 6;
    if (nchunks <= m) return;                    // whole workgroup
    for (int j = threadIdx.x; j < kPhiLutN; j += 64 * kRansWaves) sh_lut[j] = phi_lut[j];
    __syncthreads();
    const int K = (nchunks - m + M - 1) / M;
    uint32_t x = rstate[(long)sidx * 64 + lane];                       // every wave: its own copy
    int bcur = (int)rpos[sidx];                                          // bit cursor in the stream's bit region, moving DOWN
    const uint32_t *bitw = reinterpret_cast<const uint32_t *>(slots + rslot_off[sidx] + 4);
    const int max_dw = (rslot_cap - 4) >> 2;
    // Stream bits: register window of 128 dwords below wtop (a multiple of 64): lane l of winA holds dword wtop - 64 + l,
    // of winB dword wtop - 128 + l; bcur stays in (32 (wtop - 64), 32 wtop] and a step consumes at most 1024 bits, pulled
    // with ds_bpermute instead of a dependent global load.
    int wtop = max(64, (((bcur + 31) >> 5) + 63) & ~63);
    auto load_dw = [&](int d0) -> uint32_t { return bitw[min(max(d0 + lane, 0), max_dw - 1)]; };
    uint32_t winA = load_dw(wtop - 64), winB = load_dw(wtop - 128);
    int badx = 0;                                                        // a lane saw a state below 2^15 after its update (clz > 16): malformed stream
    // One pass per colour channel, Y -> Co -> Cg, in ONE launch per band (see rans_decode_stage_pair_kernel): a stream's chunk of Co
    // needs only the Y pixels of the same chunk, decoded by this very wavefront a pass earlier.
    auto pass = [&](auto tag) {
    constexpr int clr = decltype(tag)::value;    // compile-time: no branch (hence no register merge, hence no s_waitcnt vmcnt(0)) next to the prefetch loads
    // the stream's tail symbols (last stage only) are not in the main stream: sequence position 64 k + lane >= tail_from
    const int tail_from = (last_stage && clr == 2) ? rans_stream_count(nc, m, M, 64) - (int)(rtail[sidx] & 0xFFFFu) : 0x7FFFFFFF;
    int minv, maxv, shift;
    clr_range(minmax + 4 * b, clr, minv, maxv, shift);
    const Grid gr = make_grid(minv, maxv);
    const int max_symbol = gr.Lp - 2;
    const float fbase = (float)minv - 0.5f;
    const long img = sg.img_off;
    const int mA = lane & 3;                                            // component A of this lane; component B is 4 (read from lane 3 only)
    const int gsym = 16 * wave + (lane >> 2);                           // symbol (lane of the stream) this 4-lane group resolves
    const int gbit = lane & ~3;                                         // ballot bit of the group's first lane
    const bool head = (mA == 0);
    // Raw CNN outputs / prior-channel pixels of this group's symbol in step k: requested one step ahead, so the
    // memory round trip runs under the previous step's search instead of in front of this one's.
    struct Raw { float sgA, muA, wkA, a0A, a1A, sgB, muB, wkB, a0B, a1B, y, co; long off; bool on; };
    auto fetch = [&](int k) -> Raw {
        Raw r;
        const int n = min(64 * (m + k * M) + gsym, nc - 1);          // clamped: the loads are unconditional
        const int i = div_wc(sg, n), j = n - i * sg.wc;          // multiply-shift: a runtime division costs ~25 of the step's ~900 instructions
        const ParRow32 par = par_row32(params + sg.par_off, 0, (long)sg.h * sg.w, (long)i * sg.w + j);
        r.off = img + ((long)(2 * i + sg.oi) << sg.lvl) * sg.W + ((long)(2 * j + sg.oj) << sg.lvl);
        r.sgA = par[5 * clr + mA]; r.muA = par[16 + 5 * clr + mA]; r.wkA = par[32 + 5 * clr + mA];
        r.sgB = par[5 * clr + 4];  r.muB = par[16 + 5 * clr + 4];  r.wkB = par[32 + 5 * clr + 4];
        r.a0A = r.a1A = r.a0B = r.a1B = r.y = r.co = 0.0f;
        if constexpr (clr == 1) { r.a0A = par[48 + mA]; r.a0B = par[48 + 4]; r.y = fplanes[r.off]; }
        else if constexpr (clr == 2) {
            r.a0A = par[48 + 5 + mA]; r.a1A = par[48 + 10 + mA]; r.a0B = par[48 + 5 + 4]; r.a1B = par[48 + 10 + 4];
            r.y = fplanes[r.off]; r.co = fplanes[r.off + sg.plane];
        }
        r.on = (k < K) && (64 * (m + k * M) + gsym) < nc && (64 * k + gsym) < tail_from;
        return r;
    };
    Raw cur = fetch(0);
    for (int k = 0; k < K; ++k) {
        const int chunk0 = 64 * (m + k * M);
        Raw nxt = fetch(min(k + 1, K - 1));
        // slot of this group's symbol = low half of the state in lane gsym of this wave's copy
        const uint32_t slot = (uint32_t)__builtin_amdgcn_ds_bpermute(4 * gsym, (int)x) & 0xFFFFu;
        {
            if (cur.on) {                        // uniform within the group
                const long off = cur.off;
                float wA, wB;
                Comp A = mix_component<clr>(cur.sgA, cur.muA, cur.wkA, cur.a0A, cur.a1A, cur.y, cur.co, wA);
                Comp B = mix_component<clr>(cur.sgB, cur.muB, cur.wkB, cur.a0B, cur.a1B, cur.y, cur.co, wB);
                const float den = mix_weight_den(quad_lane0(dpp_sum5(wA, wB)));
                A.wn = wA / den;
                B.wn = wB / den;

                // 1. hint: 5-ary search on the approximate table.  Every lane of the group holds ALL five components in
                //    fast form (quad broadcasts) and evaluates the whole approximate mixture at its OWN probe point, so a
                //    round costs one 5-term evaluation (no cross-lane sum) and cuts the bracket to a fifth: 4 rounds for
                //    Lp = 512 instead of 9 bisection rounds.  The phase is instruction-issue bound (in-kernel stamps), and
                //    4 x ~85 instructions are fewer than 9 x 56.
                const CompLut Af = comp_lut(A), Bf = comp_lut(B);
                CompLut F0, F1, F2, F3;
                F0.c1 = quad_bcast<0>(Af.c1); F0.c0 = quad_bcast<0>(Af.c0); F0.wn = quad_bcast<0>(Af.wn);
                F1.c1 = quad_bcast<1>(Af.c1); F1.c0 = quad_bcast<1>(Af.c0); F1.wn = quad_bcast<1>(Af.wn);
                F2.c1 = quad_bcast<2>(Af.c1); F2.c0 = quad_bcast<2>(Af.c0); F2.wn = quad_bcast<2>(Af.wn);
                F3.c1 = quad_bcast<3>(Af.c1); F3.c0 = quad_bcast<3>(Af.c0); F3.wn = quad_bcast<3>(Af.wn);
                int glo = 0, ghi = max_symbol + 1;
                while (ghi - glo > 1) {
                    const int stp = (ghi - glo + 4) / 5;                   // >= 1; the last part is the (smaller) remainder
                    auto probe_at = [&](int j) { return min(glo + stp * (j + 1), ghi - 1); };
                    const int pi = probe_at(mA);
                    const float pt = div255_exact(fbase + (float)pi);     // the exact sample point: near a narrow component the CDF moves by counts per ulp of pt
                    float sum = term_lut(F0, pt, sh_lut);
                    sum += term_lut(F1, pt, sh_lut);
                    sum += term_lut(F2, pt, sh_lut);
                    sum += term_lut(F3, pt, sh_lut);
                    sum += term_lut(Bf, pt, sh_lut);
                    const int e = (int)__builtin_rintf(sum * gr.scale) + pi;
                    const uint64_t bal = ballot64(e <= (int)slot);
                    // the four probes are ordered, so the passes form a prefix of the quad's lanes (if the approximation
                    // ever breaks that, the hint is merely wrong: the proof below decides)
                    const int np = __builtin_popcount((uint32_t)(bal >> gbit) & 0xFu);
                    const int nlo = (np > 0) ? probe_at(np - 1) : glo;
                    const int nhi = (np < 4) ? probe_at(np) : ghi;
                    glo = nlo; ghi = nhi;
                }
                // 2. proof with the exact spec arithmetic: entries glo and glo + 1 in one round (independent chains);
                //    if the hint is off, gallop away from it and bisect -- prove_symbol()'s search, in place (profiles/README.md, decoder_parts)
                int lo = 0, hi = max_symbol + 1;
                uint32_t vlo = 0, vhi = 0x10000u;                    // meaningful in the group's first lane only
                bool have_lo = false, have_hi = false;
                {
                    const int s1 = glo, s2 = min(glo + 1, max_symbol);
                    // components 0..3 of both entries in their own lanes; component 4 of entry s1 in the group's
                    // lane 0 and of entry s2 in lane 1 (every lane holds component 4's parameters): three
                    // evaluations per lane instead of four
                    const float p1 = sample_pt(gr, s1), p2 = sample_pt(gr, s2);
                    const float pX = (mA == 1) ? p2 : p1;
                    const float t1 = mix_term(A.wn, A.mu, A.rsig, p1);
                    const float t2 = mix_term(A.wn, A.mu, A.rsig, p2);
                    const float tX = mix_term(B.wn, B.mu, B.rsig, pX);
                    float a1 = t1 + dpp_row_shl(t1, 1);              // (((t0 + t1) + t2) + t3) + t4, in the group's lane 0
                    a1 = a1 + dpp_row_shl(t1, 2);
                    a1 = a1 + dpp_row_shl(t1, 3);
                    a1 = a1 + tX;
                    float a2 = t2 + dpp_row_shl(t2, 1);
                    a2 = a2 + dpp_row_shl(t2, 2);
                    a2 = a2 + dpp_row_shl(t2, 3);
                    a2 = a2 + dpp_row_shl(tX, 1);
                    const uint32_t eA = entry_from_sum(a1, gr.scale, s1);
                    const uint32_t eB = entry_from_sum(a2, gr.scale, s2);
                    const bool bA = (ballot64(eA <= slot) >> gbit) & 1ull;
                    const bool bB = (ballot64(eB <= slot) >> gbit) & 1ull;
                    const bool leA = (s1 == 0) || bA;                // entry 0 is the floor of the search (torchac: left = 0)
                    const bool leB = (s1 + 1 <= max_symbol) && bB;   // past the top symbol: c_high = 0x10000 by definition
                    if (leA) {
                        lo = s1; vlo = eA; have_lo = true;
                        if (leB) { lo = s2; vlo = eB; }
                        else if (s1 + 1 <= max_symbol) { hi = s2; vhi = eB; have_hi = true; }
                    } else { hi = s1; vhi = eA; have_hi = true; }
                }
                int step = 2;
                while (hi - lo > 1) {
                    int probe;
                    if (have_lo && have_hi) probe = (lo + hi) >> 1;
                    else if (have_lo) { probe = min(lo + step, hi - 1); step <<= 1; }
                    else { probe = max(hi - step, lo + 1); step <<= 1; }
                    const uint32_t e = group_cdf_entry(A, B, gr, probe);
                    const uint64_t bal = ballot64(e <= slot);
                    if ((bal >> gbit) & 1ull) { lo = probe; vlo = e; have_lo = true; } else { hi = probe; vhi = e; have_hi = true; }
                }
                if (!have_lo) vlo = group_cdf_entry(A, B, gr, 0);
                if (head) {
                    sh_res[k & 1][gsym][0] = vlo;
                    sh_res[k & 1][gsym][1] = vhi;
                    const int v = lo - shift;
                    planes[off + (long)clr * sg.plane] = (int16_t)v;
                    fplanes[off + (long)clr * sg.plane] = div255_exact((float)v);
                }
            }
        }
        // (the next step's operands are pinned in their registers here, in front of this step's window reload: see rans_decode_stage_lane_kernel)
        asm volatile("" : "+v"(nxt.sgA), "+v"(nxt.muA), "+v"(nxt.wkA), "+v"(nxt.a0A), "+v"(nxt.a1A), "+v"(nxt.sgB), "+v"(nxt.muB), "+v"(nxt.wkB), "+v"(nxt.a0B), "+v"(nxt.a1B), "+v"(nxt.y), "+v"(nxt.co));
        lds_barrier();      // LDS words only cross here: global loads / stores in flight stay in flight (common.hpp)
        {
            const bool active = chunk0 + lane < nc && 64 * k + lane < tail_from;
            int nb = 0;
            if (active) {
                const uint32_t vlo = sh_res[k & 1][lane][0], vhi = sh_res[k & 1][lane][1];
                x = (vhi - vlo) * (x >> 16) + (x & 0xFFFFu) - vlo;            // in [freq << 15, freq << 16)
                const int lz = __clz((int)x);
                badx |= lz > 16;                                               // only a corrupt stream: the oracle rejects it right here, so flag the image (below)
                nb = min(lz, 16);
            }
            const int incl = wave_incl_scan(nb);
            const int bpos = bcur - incl;                                       // this lane's bits: [bpos, bpos + nb)
            const int d = bpos >> 5;                                           // wtop - 128 <= d < wtop on a well-formed stream
            const uint32_t a0 = (uint32_t)__builtin_amdgcn_ds_bpermute(4 * (d & 63), (int)winA);
            const uint32_t b0 = (uint32_t)__builtin_amdgcn_ds_bpermute(4 * (d & 63), (int)winB);
            const uint32_t a1 = (uint32_t)__builtin_amdgcn_ds_bpermute(4 * ((d + 1) & 63), (int)winA);
            const uint32_t b1 = (uint32_t)__builtin_amdgcn_ds_bpermute(4 * ((d + 1) & 63), (int)winB);
            const uint32_t w0 = (d >= wtop - 64) ? a0 : b0;
            const uint32_t w1 = (d + 1 >= wtop - 64) ? a1 : b1;
            const uint32_t bits = __builtin_amdgcn_alignbit(w1, w0, (uint32_t)(bpos & 31)) & ((1u << nb) - 1u);
            x = (x << nb) | bits;
            bcur -= __builtin_amdgcn_readlane(incl, 63);
            if (bcur <= 32 * (wtop - 64) && wtop > 64) { wtop -= 64; winA = winB; winB = load_dw(wtop - 128); }
        }
        cur = nxt;
    }
    };
    pass(std::integral_constant<int, 0>{});
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup"); __syncthreads();
    pass(std::integral_constant<int, 1>{});
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup"); __syncthreads();
    pass(std::integral_constant<int, 2>{});
    if (wave == 0) {
        rstate[(long)sidx * 64 + lane] = x;
        const bool anybad = ballot64(badx != 0) != 0;
        if (lane == 0) {
            rpos[sidx] = (uint32_t)max(bcur, 0);
            if (bcur < 0 || anybad) flag_image(status, b, LLICTI_EFORMAT);     // the stream ran out of bits, or a state fell out of [2^31, 2^32)
        }
    }
}

// Wide streams (Q = 2, 128 lanes): FOUR wavefronts per stream, TWO lanes per symbol.  The stage is bound by vector instructions per
// symbol (a CU's issue saturates at two wavefronts per SIMD), and four lanes per symbol spend them on overhead: four 5-ary rounds
// are 16 mixture evaluations per symbol where a pair's six ternary rounds are 12, and a wave's per-step fixed costs (fetch, the
// state update of all 128 lanes) are shared by 32 symbols instead of 16.  A pair's lanes each own three mixture components
// (0,1,2 / 2,3,4), prepare them (mix_component) and swap the results (quad_perm [1,0,3,2]); both then hold all five in
// canonical order.  Hint: ternary search on the approximate CDF, one probe per lane.  Proof: lane 0 evaluates the exact entry s,
// lane 1 entry s + 1, each all five terms in the spec's order -- no cross-lane sum.  Bit-identical to the four-lane kernel.
// One launch decodes a band's three stages (Y, Co, Cg passes).
__device__ __forceinline__ float pair_swap(float v)
{
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0xB1, 0xF, 0xF, true));     // quad_perm [1,0,3,2]
}
__device__ __forceinline__ uint32_t pair_swap_u(uint32_t v)
{
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xF, 0xF, true);
}

__global__ __launch_bounds__(64 * kRansWaves) void rans_decode_stage_pair_kernel(const float *__restrict__ params, const StageGeom *__restrict__ sgv, const StreamRef *__restrict__ sref,
                                                               const float2 *__restrict__ phi_lut,
                                                               const uint8_t *__restrict__ slots, const long *__restrict__ rslot_off,
                                                               int rslot_cap, uint32_t *__restrict__ rstate, uint32_t *__restrict__ rpos,
                                                               const uint32_t *__restrict__ rtail,
                                                               int16_t *__restrict__ planes, float *__restrict__ fplanes,
                                                               const int32_t *__restrict__ minmax, int last_stage, int32_t *status,
                                                               const int *__restrict__ act = nullptr)
{
    constexpr int Q = 2, L = 64 * Q;
    __shared__ uint32_t sh_res[2][L][2];         // ping-pong by step parity: [0] = c_low, [1] = c_high
    __shared__ float2 sh_lut[kPhiLutN];          // the hint's normal CDF (term_lut)
    const int sidx = act ? act[blockIdx.x] : (int)blockIdx.x;      // (act: a per-image-reduce call's list of the level's streams, llicti_decode_images_*_rv)
    const StreamRef sr_ = sref[sidx];               // the stream's image, its index among the image's streams, the image's stream count (images of a call may differ)
    const int b = sr_.b, m = sr_.m, M = sr_.M;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const StageGeom sg = sgv[b];                 // the image's own stage geometry (the images of a call may differ in size)
    const int nc = sg.hc * sg.wc;
    const int nchunks = (nc + L - 1) / L;
    if (nchunks <= m) return;                    // whole workgroup
    for (int j = threadIdx.x; j < kPhiLutN; j += 64 * kRansWaves) sh_lut[j] = phi_lut[j];
    __syncthreads();
    const int K = (nchunks - m + M - 1) / M;
    uint32_t x[Q];                                                      // every wave: its own copy of the stream's 128 states
#pragma unroll
    for (int qq = 0; qq < Q; ++qq) x[qq] = rstate[((long)sidx * Q + qq) * 64 + lane];
    int bcur = (int)rpos[sidx];                                          // bit cursor in the stream's bit region, moving DOWN
    const uint32_t *bitw = reinterpret_cast<const uint32_t *>(slots + rslot_off[sidx] + 4);
    const int max_dw = (rslot_cap - 4) >> 2;
    int wtop = max(64, (((bcur + 31) >> 5) + 63) & ~63);
    auto load_dw = [&](int d0) -> uint32_t { return bitw[min(max(d0 + lane, 0), max_dw - 1)]; };
    uint32_t winA = load_dw(wtop - 64), winB = load_dw(wtop - 128);
    int badx = 0;                                                        // a lane saw a state below 2^15 after its update (clz > 16): malformed stream
    // One pass per colour channel, Y -> Co -> Cg: a stream's chunk of Co needs only the Y pixels of the same chunk (the cross-channel
    // mean update reads the SAME position, LLICTI_nets.py:474-477), which this very wavefront decoded a pass earlier -- so the band's
    // three stages are one launch (15 per decode instead of 45: a launch's ramp-up and its wait for the slowest stream are paid once).
    // The channel is a compile-time constant of the pass: no branch next to the prefetch loads.
    auto pass = [&](auto tag) {
    constexpr int clr = decltype(tag)::value;
    const int tail_from = (last_stage && clr == 2) ? rans_stream_count(nc, m, M, L) - (int)(rtail[sidx] & 0xFFFFu) : 0x7FFFFFFF;
    int minv, maxv, shift;
    clr_range(minmax + 4 * b, clr, minv, maxv, shift);
    const Grid gr = make_grid(minv, maxv);
    const int max_symbol = gr.Lp - 2;
    const float fbase = (float)minv - 0.5f;
    const long img = sg.img_off;
    const int pl = lane & 1;                                            // lane of the pair
    const bool odd = pl != 0;
    const int gsym = 32 * wave + (lane >> 1);                           // stream lane (0 .. 127) this pair resolves
    const int gbit = lane & ~1;                                         // ballot bit of the pair's first lane
    const bool head = !odd;
    const int c0 = 2 * pl;                                              // the lane's own components: c0, c0 + 1, c0 + 2
    struct Raw { float sg[3], mu[3], wk[3], a0[3], a1[3], y, co; long off; bool on; };
    auto fetch = [&](int k) -> Raw {
        Raw r;
        const int n = min(L * (m + k * M) + gsym, nc - 1);           // clamped: the loads are unconditional
        const int i = div_wc(sg, n), j = n - i * sg.wc;
        const ParRow32 par = par_row32(params + sg.par_off, 0, (long)sg.h * sg.w, (long)i * sg.w + j);
        r.off = img + ((long)(2 * i + sg.oi) << sg.lvl) * sg.W + ((long)(2 * j + sg.oj) << sg.lvl);
        r.y = r.co = 0.0f;
#pragma unroll
        for (int t = 0; t < 3; ++t) {
            r.sg[t] = par[5 * clr + c0 + t]; r.mu[t] = par[16 + 5 * clr + c0 + t]; r.wk[t] = par[32 + 5 * clr + c0 + t];
            r.a0[t] = r.a1[t] = 0.0f;
            if constexpr (clr == 1) r.a0[t] = par[48 + c0 + t];
            else if constexpr (clr == 2) { r.a0[t] = par[48 + 5 + c0 + t]; r.a1[t] = par[48 + 10 + c0 + t]; }
        }
        if constexpr (clr == 1) r.y = fplanes[r.off];
        else if constexpr (clr == 2) { r.y = fplanes[r.off]; r.co = fplanes[r.off + sg.plane]; }
        r.on = (k < K) && (L * (m + k * M) + gsym) < nc && (L * k + gsym) < tail_from;
        return r;
    };
    // own[0..2] of the two lanes -> the five components in canonical order (component 2 is computed by both)
    auto canon = [&](const float own[3], float out[5]) {
        const float r0 = pair_swap(own[0]), r1 = pair_swap(own[1]), r2 = pair_swap(own[2]);
        out[0] = odd ? r0 : own[0];
        out[1] = odd ? r1 : own[1];
        out[2] = odd ? own[0] : own[2];
        out[3] = odd ? own[1] : r1;
        out[4] = odd ? own[2] : r2;
    };
    Raw cur = fetch(0);
    for (int k = 0; k < K; ++k) {
        const int chunk0 = L * (m + k * M);
        Raw nxt = fetch(min(k + 1, K - 1));
        const uint32_t xs = (wave < 2) ? x[0] : x[1];
        const uint32_t slot = (uint32_t)__builtin_amdgcn_ds_bpermute(4 * (gsym & 63), (int)xs) & 0xFFFFu;
        if (cur.on) {                            // uniform within the pair
            const long off = cur.off;
            float mu3[3], rs3[3], w3[3];             // the lane's three components
#pragma unroll
            for (int t = 0; t < 3; ++t) {
                const Comp c = mix_component<clr>(cur.sg[t], cur.mu[t], cur.wk[t], cur.a0[t], cur.a1[t], cur.y, cur.co, w3[t]);
                mu3[t] = c.mu; rs3[t] = c.rsig;
            }
            float w5[5];
            Mix mx;                                  // all five, in canonical order, in both lanes
            canon(w3, w5);
            const float den = mix_weight_den(w5[0], w5[1], w5[2], w5[3], w5[4]);
            float wn3[3];
#pragma unroll
            for (int t = 0; t < 3; ++t) wn3[t] = w3[t] / den;
            canon(mu3, mx.mu); canon(rs3, mx.rsig); canon(wn3, mx.wn);
            CompLut F[5];
#pragma unroll
            for (int c = 0; c < 5; ++c) { Comp cc; cc.mu = mx.mu[c]; cc.rsig = mx.rsig[c]; cc.wn = mx.wn[c]; F[c] = comp_lut(cc); }

            // 1. hint: ternary search on the approximate table, one probe per lane of the pair
            int glo = 0, ghi = max_symbol + 1;
            while (ghi - glo > 1) {
                const int stp = (ghi - glo + 2) / 3;                    // >= 1
                const int q1 = min(glo + stp, ghi - 1), q2 = min(glo + 2 * stp, ghi - 1);
                const int pi = odd ? q2 : q1;
                const float pt = div255_exact(fbase + (float)pi);
                float sum = term_lut(F[0], pt, sh_lut);
                sum += term_lut(F[1], pt, sh_lut);
                sum += term_lut(F[2], pt, sh_lut);
                sum += term_lut(F[3], pt, sh_lut);
                sum += term_lut(F[4], pt, sh_lut);
                const int e = (int)__builtin_rintf(sum * gr.scale) + pi;
                const uint64_t bal = ballot64(e <= (int)slot);
                const int np = __builtin_popcount((uint32_t)(bal >> gbit) & 0x3u);      // ordered probes: the passes form a prefix
                const int nlo = (np == 0) ? glo : (np == 1) ? q1 : q2;
                const int nhi = (np == 0) ? q1 : (np == 1) ? q2 : ghi;
                glo = nlo; ghi = nhi;
            }
            // exact table entry i in this lane: cdf_entry()'s operations, the terms formed before the first add (profiles/README.md, decoder_parts)
            auto entry_exact = [&](int i) __attribute__((always_inline)) -> uint32_t {
                const float pt = sample_pt(gr, i);
                float t[5];
#pragma unroll
                for (int c = 0; c < 5; ++c) t[c] = mix_term(mx.wn[c], mx.mu[c], mx.rsig[c], pt);
                return entry_from_sum((((t[0] + t[1]) + t[2]) + t[3]) + t[4], gr.scale, i);
            };
            // 2. proof: lane 0 evaluates entry glo, lane 1 entry glo + 1; if the hint is off, gallop away from it and bisect with the same
            //    probe in both lanes (uniform in the pair)
            const Proved pr = prove_symbol(glo, max_symbol, 2,
                [&](int s1, int s2, uint32_t &eA, uint32_t &eB) __attribute__((always_inline)) {
                    const uint32_t eM = entry_exact(odd ? s2 : s1);
                    const uint32_t eO = pair_swap_u(eM);
                    eA = odd ? eO : eM; eB = odd ? eM : eO;
                },
                entry_exact, [&](uint32_t e) __attribute__((always_inline)) { return e <= slot; });
            if (head) {
                sh_res[k & 1][gsym][0] = pr.vlo;
                sh_res[k & 1][gsym][1] = pr.vhi;
                const int v = pr.lo - shift;
                planes[off + (long)clr * sg.plane] = (int16_t)v;
                fplanes[off + (long)clr * sg.plane] = div255_exact((float)v);
            }
        }
        // (the next step's operands are pinned in their registers here, in front of this step's window reload: see rans_decode_stage_lane_kernel)
#pragma unroll
        for (int t = 0; t < 3; ++t) asm volatile("" : "+v"(nxt.sg[t]), "+v"(nxt.mu[t]), "+v"(nxt.wk[t]), "+v"(nxt.a0[t]), "+v"(nxt.a1[t]));
        asm volatile("" : "+v"(nxt.y), "+v"(nxt.co));
        lds_barrier();      // LDS words only cross here: global loads / stores in flight stay in flight (common.hpp)
        {
            int below = 0;                                                         // bits of the lower sub-chunk of this step
#pragma unroll
            for (int qq = 0; qq < Q; ++qq) {
                const int sl = 64 * qq + lane;                                     // stream lane
                const bool active = chunk0 + sl < nc && L * k + sl < tail_from;
                int nb = 0;
                if (active) {
                    const uint32_t vlo = sh_res[k & 1][sl][0], vhi = sh_res[k & 1][sl][1];
                    x[qq] = (vhi - vlo) * (x[qq] >> 16) + (x[qq] & 0xFFFFu) - vlo;  // in [freq << 15, freq << 16)
                    const int lz = __clz((int)x[qq]);
                    badx |= lz > 16;                                               // only a corrupt stream: the oracle rejects it right here, so flag the image (below)
                    nb = min(lz, 16);
                }
                const int incl = wave_incl_scan(nb);
                const int bpos = bcur - below - incl;                              // this lane's bits: [bpos, bpos + nb)
                const int d = bpos >> 5;                                           // wtop - 128 <= d < wtop on a well-formed stream
                const uint32_t a0 = (uint32_t)__builtin_amdgcn_ds_bpermute(4 * (d & 63), (int)winA);
                const uint32_t b0 = (uint32_t)__builtin_amdgcn_ds_bpermute(4 * (d & 63), (int)winB);
                const uint32_t a1 = (uint32_t)__builtin_amdgcn_ds_bpermute(4 * ((d + 1) & 63), (int)winA);
                const uint32_t b1 = (uint32_t)__builtin_amdgcn_ds_bpermute(4 * ((d + 1) & 63), (int)winB);
                const uint32_t w0 = (d >= wtop - 64) ? a0 : b0;
                const uint32_t w1 = (d + 1 >= wtop - 64) ? a1 : b1;
                const uint32_t bits = __builtin_amdgcn_alignbit(w1, w0, (uint32_t)(bpos & 31)) & ((1u << nb) - 1u);
                x[qq] = (x[qq] << nb) | bits;
                below += __builtin_amdgcn_readlane(incl, 63);
            }
            bcur -= below;
            if (bcur <= 32 * (wtop - 64) && wtop > 64) { wtop -= 64; winA = winB; winB = load_dw(wtop - 128); }
        }
        cur = nxt;
    }
    };
    // Between passes: the pixels a wavefront stored are loaded again by the SAME wavefront (same lanes, same positions), through the
    // same CU's L1 / the same XCD's L2 -- a workgroup-scope fence orders them (an agent-scope __threadfence() writes the L2 back: +0.45 ms
    // per decode); the barrier frees the ping-pong result buffers.
    pass(std::integral_constant<int, 0>{});
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup"); __syncthreads();
    pass(std::integral_constant<int, 1>{});
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup"); __syncthreads();
    pass(std::integral_constant<int, 2>{});
    if (wave == 0) {
#pragma unroll
        for (int qq = 0; qq < Q; ++qq) rstate[((long)sidx * Q + qq) * 64 + lane] = x[qq];
        const bool anybad = ballot64(badx != 0) != 0;
        if (lane == 0) {
            rpos[sidx] = (uint32_t)max(bcur, 0);
            if (bcur < 0 || anybad) flag_image(status, b, LLICTI_EFORMAT);     // the stream ran out of bits, or a state fell out of [2^31, 2^32)
        }
    }
}

// XWIDE streams (Q = 4, 256 lanes): ONE lane per symbol, one wavefront per 64 stream lanes -- four per workgroup, one per SIMD.
// The stage decoders are bound by vector instructions ISSUED per symbol (a lone wavefront per SIMD issues one every ~4 cycles whatever
// it does), and lanes that share a symbol spend them on each other: the pair kernel runs 12 approximate mixture evaluations (six ternary
// rounds x two lanes) and two preparations per symbol, this kernel 9 (binary search) and one; the two exact entries c_low, c_high are the
// same ten erfc either way.  ~26 instead of ~41 issued instructions per symbol.  What makes one lane per symbol possible without halving
// the wavefronts per workgroup is the lane count of the STREAM (bytes are per stream, 0.06 bit per lane), and what makes it cheap is the
// channel-planar `params` layout: a wavefront's 64 symbols are 64 consecutive positions, so every parameter load is one coalesced
// 256-byte access whose address is scalar base + lane position.
// Each wavefront owns the states of its 64 stream lanes (no copies): a step's symbols never leave their lane -- slot, search, c_low /
// c_high and the state update all happen in it -- and the only exchange is the four wavefronts' bit totals (LDS, one barrier per step),
// from which every lane knows where its bits start.  The stream's bits come from an LDS ring of 512 dwords (a step takes at most
// 128), refilled 128 dwords at a time: requested at the end of a step, stored at the end of the next, used after the barrier that follows.
template <int Q>
__global__ __launch_bounds__(64 * Q) void rans_decode_stage_lane_kernel(const float *__restrict__ params, const StageGeom *__restrict__ sgv, const StreamRef *__restrict__ sref,
                                                               const uint8_t *__restrict__ slots, const long *__restrict__ rslot_off,
                                                               int rslot_cap, uint32_t *__restrict__ rstate, uint32_t *__restrict__ rpos,
                                                               const uint32_t *__restrict__ rtail,
                                                               int16_t *__restrict__ planes, float *__restrict__ fplanes,
                                                               const int32_t *__restrict__ minmax, int last_stage, int32_t *status,
                                                               const float2 *__restrict__ phi_lut, const int *__restrict__ act = nullptr)
{
    constexpr int L = 64 * Q;
    constexpr int kRing = 512, kRefill = 128;    // dwords; a step consumes at most 16 L bits = L / 2 dwords
    static_assert(L / 2 <= kRefill && kRing >= 4 * kRefill && 64 * Q >= kRefill, "ring sizing");
    __shared__ uint32_t sh_ring[kRing];          // stream dword d at sh_ring[d & (kRing - 1)]
    __shared__ int sh_tot[2][Q];                 // a step's bit totals per wavefront (ping-pong by step parity)
    // The hint's mixture evaluations are 45 of the ~55 a symbol costs (nine probes x five components), and on the vector unit each is 15
    // operations, two of them quarter-rate (rcp, exp2).  The normal CDF of ONE variable is a table: Phi(z) on [-6, 6] in kPhiLutN steps as
    // (value, difference to the next) pairs (the context's, computed once on the host in double), 16 KB of LDS, read with linear
    // interpolation -- error <= h^2 / 8 max|Phi''| = 1e-6, a fifteenth of a count of the 16-bit table (the vector form's Abramowitz-Stegun
    // fit: 1.5e-7; either way the hint is proved or corrected by exact entries).  A term is then fma (table coordinate), clamp, floor,
    // convert, min, fract, one 8-byte LDS read, two fma: ~1,220 instead of ~1,510 vector instructions per symbol, stage launches -6 %.
    constexpr int kLutN = kPhiLutN;
    constexpr float kLutZ = (float)kPhiLutZ, kLutS = kLutN / (2.0f * kLutZ);
    __shared__ float2 sh_lut[kLutN];
    const int sidx = act ? act[blockIdx.x] : (int)blockIdx.x;      // (act: a per-image-reduce call's list of the level's streams, llicti_decode_images_*_rv)
    const StreamRef sr_ = sref[sidx];               // the stream's image, its index among the image's streams, the image's stream count (images of a call may differ)
    const int b = sr_.b, m = sr_.m, M = sr_.M;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;      // tid = lane of the stream
    const StageGeom sg = sgv[b];                 // the image's own stage geometry (the images of a call may differ in size)
    const int nc = sg.hc * sg.wc;
    const int nchunks = (nc + L - 1) / L;
    if (nchunks <= m) return;                    // whole workgroup
    for (int j = tid; j < kLutN; j += L) sh_lut[j] = phi_lut[j];
    const int K = (nchunks - m + M - 1) / M;
    uint32_t x = rstate[(long)sidx * L + tid];
    int bcur = (int)rpos[sidx];                  // bit cursor in the stream's bit region, moving DOWN
    const uint32_t *bitw = reinterpret_cast<const uint32_t *>(slots + rslot_off[sidx] + 4);
    const int max_dw = (rslot_cap - 4) >> 2;
    auto load_dw = [&](int d) -> uint32_t { return bitw[min(max(d, 0), max_dw - 1)]; };
    // ring window [wlo, wlo + kRing): everything a step can touch, dwords (bcur >> 5) - L / 2 .. (bcur >> 5) + 1, with two steps of slack below
    int wlo = ((((bcur >> 5) + 2) + kRefill - 1) & ~(kRefill - 1)) - kRing;
    for (int t = tid; t < kRing; t += L) sh_ring[(wlo + t) & (kRing - 1)] = load_dw(wlo + t);
    uint32_t pf = 0;                             // a refill in flight: dwords [wlo, wlo + kRefill) of the NEW wlo, lanes 0 .. kRefill - 1
    bool pend = false;
    int badx = 0;                                // a lane saw a state below 2^15 after its update (clz > 16): malformed stream
    int par = 0;                                 // step parity over the whole launch (sh_tot)
    __syncthreads();

    auto pass = [&](auto tag) {
    constexpr int clr = decltype(tag)::value;    // compile-time: no branch next to the prefetch loads
    const int tail_from = (last_stage && clr == 2) ? rans_stream_count(nc, m, M, L) - (int)(rtail[sidx] & 0xFFFFu) : 0x7FFFFFFF;
    int minv, maxv, shift;
    clr_range(minmax + 4 * b, clr, minv, maxv, shift);
    const Grid gr = make_grid(minv, maxv);
    const int max_symbol = gr.Lp - 2;
    const float fbase = (float)minv - 0.5f;
    const long img = sg.img_off;
    const long npos = (long)sg.h * sg.w;
    struct Raw { float sg[5], mu[5], wk[5], a0[5], a1[5], y, co; long off; bool on; };
    auto fetch = [&](int k) -> Raw {
        Raw r;
        const int n = min(L * (m + k * M) + tid, nc - 1);            // clamped: the loads are unconditional
        const int i = div_wc(sg, n), j = n - i * sg.wc;
        const ParRow32 prw = par_row32(params + sg.par_off, 0, npos, (long)i * sg.w + j);
        r.off = img + ((long)(2 * i + sg.oi) << sg.lvl) * sg.W + ((long)(2 * j + sg.oj) << sg.lvl);
        r.y = r.co = 0.0f;
#pragma unroll
        for (int t = 0; t < 5; ++t) {
            r.sg[t] = prw[5 * clr + t]; r.mu[t] = prw[16 + 5 * clr + t]; r.wk[t] = prw[32 + 5 * clr + t];
            r.a0[t] = r.a1[t] = 0.0f;
            if constexpr (clr == 1) r.a0[t] = prw[48 + t];
            else if constexpr (clr == 2) { r.a0[t] = prw[48 + 5 + t]; r.a1[t] = prw[48 + 10 + t]; }
        }
        if constexpr (clr == 1) r.y = fplanes[r.off];
        else if constexpr (clr == 2) { r.y = fplanes[r.off]; r.co = fplanes[r.off + sg.plane]; }
        r.on = (k < K) && (L * (m + k * M) + tid) < nc && (L * k + tid) < tail_from;
        return r;
    };
    Raw cur = fetch(0);
    for (int k = 0; k < K; ++k) {
        const uint32_t slot = x & 0xFFFFu;
        Proved pr{ 0, 0u, 0x10000u };
        // the five prepared components -- computed for every lane (a clamped position's values where the lane is off):
        // that makes the raw CNN outputs dead right here, so the NEXT step's are loaded into the same registers now and have the whole
        // search to arrive (no second register set, no copies)
        Mix mx;
        float w5[5];
#pragma unroll
        for (int t = 0; t < 5; ++t) {
            const Comp c = mix_component<clr>(cur.sg[t], cur.mu[t], cur.wk[t], cur.a0[t], cur.a1[t], cur.y, cur.co, w5[t]);
            mx.mu[t] = c.mu; mx.rsig[t] = c.rsig;
        }
        const long off_k = cur.off;
        const bool on_k = cur.on;
        cur = fetch(min(k + 1, K - 1));
        if (on_k) {
            const float den = mix_weight_den(w5[0], w5[1], w5[2], w5[3], w5[4]);
            float c1[5], c0[5];                  // table coordinate of component t at sample point pt: u = pt c1 + c0
#pragma unroll
            for (int t = 0; t < 5; ++t) { mx.wn[t] = w5[t] / den; c1[t] = mx.rsig[t] * kLutS; c0[t] = __builtin_fmaf(-mx.mu[t], c1[t], kLutZ * kLutS); }

            // 1. hint: binary search on the approximate table (probes 1 .. max_symbol: regular sample points only)
            int glo = 0, ghi = max_symbol + 1;
            while (ghi - glo > 1) {
                const int pi = (glo + ghi) >> 1;
                const float pt = div255_exact(fbase + (float)pi);
                float sum = 0.0f;
#pragma unroll
                for (int t = 0; t < 5; ++t) {
                    // u in [0, kLutN) -- v_med3_f32 returns one of its operands, so a NaN coordinate comes out as NaN, 0 or the bound, and v_cvt_u32_f32
                    // (which truncates) turns a NaN into 0: the index stays inside the table whatever the CNN produced; v_fract_f32 is what is left
                    const float u = __builtin_amdgcn_fmed3f(__builtin_fmaf(pt, c1[t], c0[t]), 0.0f, (float)kLutN - 0.0009765625f);
                    const float2 e2 = sh_lut[(uint32_t)u];
                    sum = __builtin_fmaf(mx.wn[t], __builtin_fmaf(e2.y, __builtin_amdgcn_fractf(u), e2.x), sum);
                }
                const int e = (int)__builtin_rintf(sum * gr.scale) + pi;
                const bool le = e <= (int)slot;
                glo = le ? pi : glo;
                ghi = le ? ghi : pi;
            }
            // exact table entry i in this lane: cdf_entry()'s operations, the terms formed before the first add (profiles/README.md, decoder_parts)
            auto entry_exact = [&](int i) __attribute__((always_inline)) -> uint32_t {
                const float pt = sample_pt(gr, i);
                float t[5];
#pragma unroll
                for (int c = 0; c < 5; ++c) t[c] = mix_term(mx.wn[c], mx.mu[c], mx.rsig[c], pt);
                return entry_from_sum((((t[0] + t[1]) + t[2]) + t[3]) + t[4], gr.scale, i);
            };
            // 2. the two entries the state update needs anyway, entry[s] and entry[s + 1], are also the proof of the hint; if it is off, gallop
            //    away from it and bisect with exact entries (a hint that is off is off by one: the first gallop probe is the neighbour)
            pr = prove_symbol(glo, max_symbol, 1,
                [&](int s1, int s2, uint32_t &eA, uint32_t &eB) __attribute__((always_inline)) { eA = entry_exact(s1); eB = entry_exact(s2); },
                entry_exact, [&](uint32_t e) __attribute__((always_inline)) { return e <= slot; });
            const int v = pr.lo - shift;
            planes[off_k + (long)clr * sg.plane] = (int16_t)v;
            fplanes[off_k + (long)clr * sg.plane] = div255_exact((float)v);
        }
        // The next step's CNN outputs were requested ~8,000 cycles ago and are pinned in their registers HERE, in front of the ring's refill
        // load: left alone, the compiler moves them into the loop-carried registers at the bottom of the loop, behind that load and the
        // pixel stores, and waits for them with s_waitcnt vmcnt(0) -- in-order counting makes that a wait for the refill load just issued
        // and for the stores (a memory round trip per step: most of the 22 % of wave cycles this kernel spent parked).
#pragma unroll
        for (int t = 0; t < 5; ++t) asm volatile("" : "+v"(cur.sg[t]), "+v"(cur.mu[t]), "+v"(cur.wk[t]), "+v"(cur.a0[t]), "+v"(cur.a1[t]));
        asm volatile("" : "+v"(cur.y), "+v"(cur.co));
        // state update of this lane, bit-granular renormalisation: lane l of the stream takes its clz(x) bits below those of lanes < l
        int nb = 0;
        if (on_k) {
            x = (pr.vhi - pr.vlo) * (x >> 16) + slot - pr.vlo;                 // in [freq << 15, freq << 16)
            const int lz = __clz((int)x);
            badx |= lz > 16;                                                   // only a corrupt stream: the oracle rejects it too
            nb = min(lz, 16);
        }
        const int incl = wave_incl_scan(nb);
        if (lane == 63) sh_tot[par][wave] = incl;
        lds_barrier();                  // (also: last step's ring refill is visible)  not __syncthreads(): the pixel stores above and the next step's parameter loads stay in flight
        int below = 0, step_total = 0;
#pragma unroll
        for (int q2 = 0; q2 < Q; ++q2) { const int t2 = sh_tot[par][q2]; step_total += t2; below += (q2 < wave) ? t2 : 0; }
        par ^= 1;
        {
            const int bpos = bcur - below - incl;                              // this lane's bits: [bpos, bpos + nb)
            const int d = bpos >> 5;
            const uint32_t w0 = sh_ring[d & (kRing - 1)], w1 = sh_ring[(d + 1) & (kRing - 1)];
            const uint32_t bits = __builtin_amdgcn_alignbit(w1, w0, (uint32_t)(bpos & 31)) & ((1u << nb) - 1u);
            x = (x << nb) | bits;
        }
        bcur -= step_total;
        // ring: store the refill requested a step ago (its slots held dwords >= wlo + kRing: above anything this step's readers touch),
        // then request the next one if fewer than two steps of dwords are left below the cursor
        if (pend) { if (tid < kRefill) sh_ring[(wlo + tid) & (kRing - 1)] = pf; pend = false; }
        if ((bcur >> 5) - 2 * kRefill < wlo) { wlo -= kRefill; if (tid < kRefill) pf = load_dw(wlo + tid); pend = true; }
    }
    };
    // Between passes: the pixels a lane stored are loaded again by the SAME lane (same position) -- a workgroup-scope fence orders them
    pass(std::integral_constant<int, 0>{});
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    pass(std::integral_constant<int, 1>{});
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    pass(std::integral_constant<int, 2>{});
    rstate[(long)sidx * L + tid] = x;
    const int anybad = __syncthreads_or(badx);
    if (tid == 0) {
        rpos[sidx] = (uint32_t)max(bcur, 0);
        if (bcur < 0 || anybad) flag_image(status, b, LLICTI_EFORMAT);     // the stream ran out of bits, or a state fell out of [2^31, 2^32)
    }
}

__global__ __launch_bounds__(256) void rans_pack_kernel(const uint8_t *__restrict__ slots, const long *__restrict__ rslot_off,
                                                        const int32_t *__restrict__ rinfo, const StreamRef *__restrict__ sref, const ImgGeo *__restrict__ iv,
                                                        uint8_t *__restrict__ out, long out_stride, int32_t *__restrict__ seg_len, int32_t *status,
                                                        const unsigned long long *__restrict__ ssum, const StreamDesc *__restrict__ desc, int B)
{
    const StreamRef sr_ = sref[blockIdx.x];
    const int b = sr_.b, m = sr_.m, M = image_stream_count(ssum, iv, desc, B, sr_.b, sr_.M), s0 = sr_.sbase;      // (s0 + k: stream k of this image)
    const int hdr_bytes = iv[b].hdr_bytes;
    if (ssum && iv[b].Mlo && m == 0 && threadIdx.x == 0) {
        // "auto": the header was written before the count was picked -- the pad field's bits 10 .. 15 say how many streams the image has
        // (an image of a fixed count in the same call, Mlo = 0, keeps the field header_write_kernel wrote: 64 / 128 streams have codes of their own there)
        uint8_t *oh = out + (long)b * out_stride;
        const int pf = (iv[b].padint & 0x3FF) | (M << 10);              // (auto counts are <= 32: the field holds them as they are)
        oh[15] = (uint8_t)(pf & 0xFF); oh[16] = (uint8_t)((pf >> 8) & 0xFF);
    }
    if (m >= M) {                                                       // a stream the image did not get: an empty segment
        if (threadIdx.x == 0) seg_len[(long)b * LLICTI_NSEG + 4 + m] = 0;
        return;
    }
    const int G = rans_group(M), sg = m / G;
    long dst = hdr_bytes + (G > 1 ? 4L * G * (sg + 1) : 0);
    for (int k = 0; k < m; ++k) dst += rinfo[2 * (s0 + k) + 1];
    const int n = rinfo[2 * (s0 + m) + 1];
    if (dst + n > out_stride) { if (threadIdx.x == 0) atomicExch(&status[0], LLICTI_ENOSPACE); return; }
    const uint8_t *src = slots + rslot_off[s0 + m] + rinfo[2 * (s0 + m)];
    uint8_t *o = out + (long)b * out_stride + dst;
    block_copy_bytes(o, src, n);
    if (threadIdx.x == 0) {
        if (G == 1) seg_len[(long)b * LLICTI_NSEG + 4 + m] = n;
        else if (m % G == 0) {                                  // the segment's length table and total
            uint8_t *tab = o - 4 * G;
            int tot = 4 * G;
            for (int k = 0; k < G; ++k) {
                const int len = rinfo[2 * (s0 + m + k) + 1];
                tab[4 * k] = (uint8_t)(len & 0xFF); tab[4 * k + 1] = (uint8_t)((len >> 8) & 0xFF);
                tab[4 * k + 2] = (uint8_t)((len >> 16) & 0xFF); tab[4 * k + 3] = (uint8_t)((len >> 24) & 0xFF);
                tot += len;
            }
            seg_len[(long)b * LLICTI_NSEG + 4 + sg] = tot;
        }
        if (m == 0) for (int k = 4 + M / G; k < LLICTI_NSEG; ++k) seg_len[(long)b * LLICTI_NSEG + k] = 0;
    }
}

__global__ __launch_bounds__(256) void rans_unpack_kernel(const uint8_t *__restrict__ in, long in_stride, const int32_t *__restrict__ seg_len,
                                                          const StreamRef *__restrict__ sref, int min_stream, uint8_t *__restrict__ slots, const long *__restrict__ rslot_off,
                                                          int rslot_cap, uint32_t *__restrict__ rpos, int32_t *status, int stream_off)
{
    const StreamRef sr_ = sref[blockIdx.x];
    const int b = sr_.b, m = sr_.m, M = sr_.M, s0 = sr_.sbase;
    const int G = rans_group(M), sg = m / G;
    const int32_t *sl = seg_len + (long)b * LLICTI_NSEG;
    long src = 0;
    bool bad = false;
    for (int k = 0; k < 4 + sg; ++k) {          // see unpack_kernel: every earlier entry is validated too
        const int v = sl[k];
        if (v < 0 || v > in_stride) bad = true;
        src += v;
        if (src < 0 || src > in_stride) { bad = true; src = 0; }
    }
    int n = sl[4 + sg];
    if (G > 1) {
        // the segment's table: G stream lengths, each a whole stream, together exactly the segment
        const int seg_n = n;
        if (bad || seg_n < 4 * G || src + seg_n > in_stride) { bad = true; n = 0; }
        else {
            const uint8_t *tab = in + (long)b * in_stride + src;
            long off = 4L * G, tot = 4L * G;
            for (int k = 0; k < G; ++k) {
                const long len = (long)tab[4 * k] | ((long)tab[4 * k + 1] << 8) | ((long)tab[4 * k + 2] << 16) | ((long)tab[4 * k + 3] << 24);
                if (len < min_stream || len > seg_n) bad = true;
                if (k < m % G) off += len;
                if (k == m % G) n = (int)min(len, (long)seg_n);
                tot += len;
            }
            if (tot != seg_n) bad = true;
            src += off;
        }
    }
    uint8_t *o = slots + rslot_off[s0 + m] + stream_off;         // the bit region lands dword aligned at slot + 4: stream offset 2 behind the u16 of a 64- / 128-lane stream, 0 in an xwide v4 stream
    if (bad || n < min_stream || n + 4 + 64 > rslot_cap || src + n > in_stride) {
        if (threadIdx.x == 0) flag_image(status, b, LLICTI_EFORMAT);
        n = min_stream;                                            // a harmless stream: T = 0, no bits, states 2^31
        for (int t = threadIdx.x; t < n; t += blockDim.x) o[t] = 0;
    } else {
        const uint8_t *p = in + (long)b * in_stride + src;
        block_copy_bytes(o, p, n);
    }
    const int padded = min(rslot_cap - stream_off, n + 64);
    for (int t = n + threadIdx.x; t < padded; t += blockDim.x) o[t] = 0;
    if (threadIdx.x == 0) rpos[s0 + m] = (uint32_t)n;            // the length rans_init_kernel parses
}

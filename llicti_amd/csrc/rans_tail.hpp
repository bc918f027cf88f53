// rans_tail.hpp -- LLICTI-rANS v3 / xwide v4 tail decoder: rans_tail_kernel<Q> in its two wavefront roles -- the preparing wavefronts
// (tail_prepare_role) and the chain's coder in its phases (tail_assemble, tail_start_state, tail_decode_rounds, tail_finish) -- on one
// context struct, RansTail<Q>.  The container is described in rans_coder.hpp, whose helpers (the LDS bit helpers, the mixture entry) this
// file uses; which tail symbol sits on which chain is SeededTailShape (host_types.hpp), shared with the encoder (rans_encode.hpp).
// Part of the single translation unit llicti_hip.hip (included in order; not a stand-alone header).
#pragma once

// After the last stage the 64 Q states of a stream ARE its tail stream (31 bits each, the tail coder's final state on top,
// its leading one the highest set bit).  The T tail symbols -- all of the last stage's Cg channel (level 0, band x10) -- come out
// of ONE coder state, serially; a lone wavefront issues one instruction every ~4 cycles whatever it does, so everything that does not
// depend on the coder state is done by other wavefronts of the workgroup:
//   * kTailAhead wavefronts per chain PREPARE symbols: the position's CNN outputs, the component's mean / 1 / sigma / normalised
//     weight with mix_component()'s operations, the approximate mixture at the 64 anchors 8 l (Lp <= 512) -- and, round 5, a
//     SPECULATED WINDOW: the twelve exact table entries around the mixture's median (where the approximate table crosses 2^15).
//     Round r + 1's symbols are prepared (into the other half of a ping-pong LDS buffer) while
//   * wavefront 0 DECODES round r's: if the slot lies inside the speculated window the symbol is proved by one compare, a ballot and
//     two v_readlane, and the state update runs on the scalar unit (the state is wave-uniform); otherwise the anchors pick a bucket,
//     12 x 5 lanes evaluate the 12 exact entries around it (lane = 5 e + mc: mixture component mc of window entry e) and a ballot
//     proves the symbol (an exact 13-ary search takes over when that hint is wrong too).  Either way the symbol is the one an exact
//     search of the whole row returns: the entries are the same bits wherever they are computed.  The renormalisation's bits come
//     from two payload dwords requested at the top of the symbol (they depend on the cursor only); the round's pixels are stored
//     together.
// What the window buys depends on the source: on uniform noise (12.8 bits per symbol, tails of ~620 symbols) it is not offered (the
// median's bucket holds a fiftieth of the mass) and nothing changes; on a source as cheap as the reference's trained model (1.7 bits
// per symbol: tails of ~4,700 symbols, all on one chain) the tail launch of 24 x 10 xwide streams goes from 2.70 to 1.29 ms, 64-lane
// streams 0.66 -> 0.34 (profiles/r5/tail_speculation.json: coder alone 1.2 ms, preparing wavefronts alone 1.2 ms).
// One barrier per round.  Checks: the main region was read to its last bit, the tail state ends at its start state (freq << 15 of
// the symbol the tail encoder began with; 2^31 when T = 0) with no bit left.  Xwide streams (two seeded chains, above): a second set of
// wavefronts runs chain B; the start states are seeds -- checked to be below A^n, with zero digits where the stream has no symbol -- the
// chains' cursors must not have crossed and the payload between them must be zero.  A ONE-chain xwide stream (cheap symbols: the second
// chain would cost its final state) leaves chain B's wavefronts idle: its preparing wavefronts join chain A's, a round is 2 kTailAhead symbols.
#ifndef TAIL_AHEAD
#define TAIL_AHEAD 4                            // (build switch for A/B runs: 2 / 3 / 4 / 5 measured, profiles/r5/tail_speculation.json)
#endif
constexpr int kTailAhead = TAIL_AHEAD;           // symbols per round = preparing wavefronts

template <int Q> constexpr int kTailChains = kSeeded<Q> ? 2 : 1;      // xwide: two chains, each with its own coder + preparing wavefronts
template <int Q> constexpr int tail_threads = 64 * (1 + kTailAhead) * kTailChains<Q>;      // the workgroup: per chain a coder and its preparing wavefronts

// The lane number is not in the context: every role and phase takes it (and mc, we) for itself.  Computed once in front of the role branch,
// the three stay live through the preparing wavefronts' code on their way to the coder's: 53 VGPRs instead of 50 (xwide: 51).
__device__ __forceinline__ int tail_lane() { return threadIdx.x & 63; }

// What both roles of rans_tail_kernel<Q> know: the call's arrays, the kernel's LDS, the stream and its tail's shape, the wavefront's place.
template <int Q> struct RansTail {
    using GEO = RansGeo<Q>;
    static constexpr int L = 64 * Q, NCH = kTailChains<Q>;
    static constexpr int kSpillDw = kSeeded<Q> ? kRansSpillMax / 32 + 1 : 0;      // xwide v4: the arena is the payload ++ the spill the main decoder left at the bottom of its region
    static constexpr int kArenaDw = GEO::kPayDw + kSpillDw;
    static constexpr int NSL = NCH * kTailAhead;        // prepared symbols per round and buffer: slot = chain kTailAhead + i
    const float *params; const uint32_t *rstate; int16_t *planes; float *fplanes; int32_t *status; const uint8_t *slots; const long *rslot_off;
    uint32_t *sh_pay;                                   // the arena (64 Q + 2 + kSpillDw dwords)
    float (*sh_cmp)[NSL][16];                           // [0..4] mu, [5..9] 1 / sigma, [10..14] normalised weight of the five components
    int (*sh_e1)[NSL][64];                              // approximate table entry at anchor 8 l
    long (*sh_off)[NSL];                                // the symbol's pixel
    int (*sh_spec)[NSL][16];                            // [0..11] the exact entries of the speculated window, [12] its first index (-1: none)
    int *sh_cur;                                        // xwide: where the two chains stopped reading
    int sidx, b, m, M;                                  // the stream, its image, its index among the image's streams, the image's stream count (images of a call may differ)
    StageGeom sg; int nc, cnt;                          // the image's own stage geometry (the images of a call may differ in size); the stage's symbols, the stream's
    Grid gr; int max_symbol, shift; uint32_t pw;        // the Cg channel's table grid; xwide: A^n of the seeds
    int alen;                                           // bits of the arena
    SeededTailShape shape;                              // chains, seeds, coded symbols (64 / 128 lanes: one chain, no seeds)
    int wave, role, chain;                              // (scalar: roles, chains and symbol counts are wave-uniform, their branches scalar)
    bool pool, live; int SA, T, R;                      // pooled wavefronts; the chain has symbols; symbols of a chain per round, this chain's symbols, rounds
    bool bad;
    struct Pos { int pi, pj; };
    __device__ __forceinline__ Pos pos(int j) const {   // (row, column) in the stage of the stream's j-th symbol from its end
        const int q = min(max(cnt - 1 - j, 0), max(cnt - 1, 0));
        const int n = min(rans_stream_pos(q, m, M, L), nc - 1);
        const int pi = div_wc(sg, n), pj = n - pi * sg.wc;
        return Pos{ pi, pj };
    }
    // position -> offset of its pixel in a plane; (offset, value) -> the Cg planes
    __device__ __forceinline__ long pixel_off(int pi, int pj) const { return sg.img_off + ((long)(2 * pi + sg.oi) << sg.lvl) * sg.W + ((long)(2 * pj + sg.oj) << sg.lvl); }
    __device__ __forceinline__ void store_pixel(long off, int v) const {
        planes[off + 2 * sg.plane] = (int16_t)v;
        fplanes[off + 2 * sg.plane] = div255_exact((float)v);      // (an integer in [-255, 255]: bit-identical to the division, numerics.hpp)
    }
};

// The stream, the tail's shape and the wavefront's place in it.
template <int Q> __device__ __forceinline__ void tail_open(RansTail<Q> &t, const StageGeom *sgv, const StreamRef *sref, const uint32_t *rpos,
                                                           const uint32_t *rtail, const int32_t *minmax, const int *act)
{
    using TL = RansTail<Q>;
    t.sidx = act ? act[blockIdx.x] : (int)blockIdx.x;      // (act: a per-image-reduce call's list of the level's streams, llicti_decode_images_*_rv)
    const StreamRef sr_ = sref[t.sidx];
    t.b = sr_.b; t.m = sr_.m; t.M = sr_.M;
    t.wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    // role 0: the chain's coder.  A workgroup's wavefronts go to the four SIMDs round robin: with two chains the coders are wavefronts 0 and 1 (their
    // own SIMD each, shared with one preparing wavefront), not 0 and 4 (the same SIMD, taking turns at its issue port)
    t.role = t.wave / TL::NCH;
    t.sg = sgv[t.b];
    t.nc = t.sg.hc * t.sg.wc;
    t.cnt = rans_stream_count(t.nc, t.m, t.M, TL::L);
    const int rt = (int)(rtail[t.sidx] & 0xFFFFu);
    const int nch = (kSeeded<Q> && !(rtail[t.sidx] >> 16)) ? 2 : 1;      // chains this stream's tail was coded with (xwide: its flag says one or two)
    // A one-chain xwide stream (well-predicted content: the second chain would cost its final state) has twice the symbols on its chain and a
    // second set of wavefronts with nothing to do: the idle chain's preparing wavefronts join chain 0's, and a round is 2 kTailAhead symbols.
    t.pool = TL::NCH == 2 && nch == 1;
    t.chain = (t.pool && t.role != 0) ? 0 : t.wave % TL::NCH;
    t.SA = t.pool ? TL::NSL : kTailAhead;
    // 64 / 128 lanes: the main region must have been read to its last bit.  xwide v4: what is left of it IS the tail coder's spill (its length the cursor)
    const int E = kSeeded<Q> ? (int)rpos[t.sidx] : 0;
    t.bad = (kSeeded<Q> ? E >= kRansSpillMax : rpos[t.sidx] != 0) || rt > t.cnt;
    t.alen = TL::GEO::kPayBits + (t.bad ? 0 : E);
    const int Tall = min(rt, t.cnt);                    // the stream's tail symbols: the coded ones, then (xwide) the seeds'
    int minv, maxv;
    clr_range(minmax + 4 * t.b, 2, minv, maxv, t.shift);
    t.gr = make_grid(minv, maxv);
    t.max_symbol = t.gr.Lp - 2;
    t.pw = 1;
    const int ns = kSeeded<Q> ? rans_seed_count(t.max_symbol + 1, t.pw) : 0;
    t.shape = seeded_tail_shape(t.cnt, Tall, nch, ns, kSeeded<Q>);
    t.bad = t.bad || Tall < t.shape.NS || (nch == 2 && t.cnt < 2 * ns);
    t.live = t.chain < nch;                             // (the second set of wavefronts idles through a one-chain stream's rounds)
    t.T = t.live ? t.shape.chain_count(t.chain) : 0;
    t.R = (t.shape.chain_count(0) + t.SA - 1) / t.SA;   // rounds (chain 0 has the most symbols)
}

// One exact table entry, idx (uniform in the lane's group of five: lane = 5 we + mc holds component mc), summed across the group left to
// right: valid in every lane of the group.  Both roles call it -- the entries are the same bits wherever they are computed.
__device__ __forceinline__ uint32_t tail_window_entry(const Grid &gr, int max_symbol, int we, float wn, float mu, float rsig, int idx)
{
    const float pt = sample_pt(gr, min(idx, gr.Lp - 1));
    const float term = mix_term(wn, mu, rsig, pt);
    const int g0 = 4 * 5 * min(we, 11);
    const float a0 = __int_as_float(__builtin_amdgcn_ds_bpermute(g0, __float_as_int(term)));
    const float a1 = __int_as_float(__builtin_amdgcn_ds_bpermute(g0 + 4, __float_as_int(term)));
    const float a2 = __int_as_float(__builtin_amdgcn_ds_bpermute(g0 + 8, __float_as_int(term)));
    const float a3 = __int_as_float(__builtin_amdgcn_ds_bpermute(g0 + 12, __float_as_int(term)));
    const float a4 = __int_as_float(__builtin_amdgcn_ds_bpermute(g0 + 16, __float_as_int(term)));
    const float acc = (((a0 + a1) + a2) + a3) + a4;
    return (idx <= max_symbol) ? entry_from_sum(acc, gr.scale, idx) : 0x10000u;      // past the top symbol: c_high = 2^16
}

// ---- role != 0, the preparing wavefronts: symbol k = SA r + i of round r (k counts the chain's symbols in decoding order), prepared into slot sl.
// Barriers A .. D pair with the coder's in rans_tail_kernel, one for one.
template <int Q> __device__ __forceinline__ void tail_prepare_role(const RansTail<Q> &t)
{
    using TL = RansTail<Q>;
    const int lane = tail_lane(), mc = lane % 5, we = lane / 5, max_symbol = t.max_symbol, SA = t.SA, T = t.T;      // lane = 5 we + mc: mixture component mc of window entry we
    const StageGeom &sg = t.sg;
    const Grid &gr = t.gr;
    const int i = t.pool ? t.wave - TL::NCH : t.role - 1;
    const int sl = t.chain * kTailAhead + i;
    struct Row { float sg, mu, wk, bb, dd, y, co; long off; };
    auto fetch = [&](int k) -> Row {
        Row r;
        const auto pp = t.pos(t.shape.index(t.chain, T - 1 - k));
        const int pi = pp.pi, pj = pp.pj;
        const ParRow src = par_row(t.params + sg.par_off, 0, (long)sg.h * sg.w, (long)pi * sg.w + pj);
        r.off = t.pixel_off(pi, pj);
        r.sg = src[10 + mc]; r.mu = src[16 + 10 + mc]; r.wk = src[32 + 10 + mc];      // the Cg channel's sigma, mu, weight ...
        r.bb = src[48 + 5 + mc]; r.dd = src[48 + 10 + mc];                                // ... and its cross-channel factors
        r.y = t.fplanes[r.off]; r.co = t.fplanes[r.off + sg.plane];
        return r;
    };
    auto prepare = [&](const Row &row, int buf) {
        // component mc: mix_component<2>'s operations, written out (profiles/README.md, section decoder_parts)
        const float t1 = row.bb * row.y;
        const float t2 = row.dd * row.co;
        const float tt = t1 + t2;
        const float mu = row.mu + tt;
        const float rsig = 1.0f / mix_sigma(row.sg);
        const float w = (row.wk > kWeightBound) ? row.wk : kWeightBound;
        float wk5[5], mu5[5], rs5[5];
#pragma unroll
        for (int k = 0; k < 5; ++k) wk5[k] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(w), k));
        const float wn = w / mix_weight_den(wk5[0], wk5[1], wk5[2], wk5[3], wk5[4]);
#pragma unroll
        for (int k = 0; k < 5; ++k) {
            mu5[k] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(mu), k));
            rs5[k] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(rsig), k));
            wk5[k] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(wn), k));
        }
        // the approximate mixture (all five components in every lane) at anchor 8 l
        const int i1 = min(8 * lane, max_symbol);
        const float pt1 = sample_pt(gr, i1);
        float sum = 0.0f;
#pragma unroll
        for (int k = 0; k < 5; ++k) { Comp ck; ck.mu = mu5[k]; ck.rsig = rs5[k]; ck.wn = wk5[k]; sum += term_fast(comp_fast(ck), pt1); }
        const int e1v = (int)__builtin_rintf(sum * gr.scale) + i1;
        t.sh_e1[buf][sl][lane] = e1v;
        if (lane < 5) { t.sh_cmp[buf][sl][lane] = mu; t.sh_cmp[buf][sl][5 + lane] = rsig; t.sh_cmp[buf][sl][10 + lane] = wn; }
        if (lane == 0) t.sh_off[buf][sl] = row.off;
        // The speculated window.  The coder's per-symbol chain is slot -> bucket -> 12 exact entries (an erfc and five cross-lane
        // moves) -> ballot -> state update, ~2,500 cycles of which the exact entries are most -- and they depend on the coder state
        // only through WHERE the window lies.  On a well-predicted source (the reference's trained model spends 1.7 bits per symbol of
        // this channel) that is nearly always around the mixture's median, which is known here: the anchor bucket in which the
        // approximate table crosses 2^15, refined linearly.  So the window's twelve entries are computed in THIS wavefront, by
        // tail_window_entry() like the coder's own, and the coder only has to look: slot inside [entry 0, entry 11) proves the symbol
        // exactly as its own window would (same entries, same ballot); outside, it falls back to its bucket search.  Not offered when
        // the median's bucket holds less than an eighth of the mass (noise: the window would miss nine times in ten).
        const int lst = __builtin_amdgcn_readfirstlane(__builtin_popcountll(ballot64(lane == 0 || (8 * lane <= max_symbol && e1v <= 0x8000))) - 1);
        const int eL = __builtin_amdgcn_readlane(e1v, lst);
        const int eH = (lst < 63 && 8 * (lst + 1) <= max_symbol) ? __builtin_amdgcn_readlane(e1v, min(lst + 1, 63)) : 0x10000;
        int wbs = -1;
        if (eH - eL >= 0x2000) {                          // (wave-uniform)
            const float fr = 8.0f * (float)(0x8000 - eL) * __builtin_amdgcn_rcpf((float)(eH - eL));
            wbs = max(8 * lst + (int)__builtin_amdgcn_fmed3f(fr, 0.0f, 8.0f) - 5, 0);
            const uint32_t ent = tail_window_entry(gr, max_symbol, we, wn, mu, rsig, wbs + min(we, 11));
            if (mc == 0 && we < 12) t.sh_spec[buf][sl][we] = (int)ent;
        }
        if (lane == 0) t.sh_spec[buf][sl][12] = wbs;
    };
    Row rowA = fetch(i);
    Row rowB = fetch(SA + i);
    prepare(rowA, 0);
    __syncthreads();                                      // A: the coder's A (the arena, assembled by wavefront 0; nothing of it is read here)
    __syncthreads();                                      // B: the coder's B -- round 0 is prepared
    for (int r = 0; r < t.R; ++r) {
        const Row rowC = fetch(SA * (r + 2) + i);            // two rounds ahead: the loads run under a whole round
        if (SA * (r + 1) + i < T) prepare(rowB, (r + 1) & 1);
        rowB = rowC;
        lds_barrier();      // C: the coder's C behind round r.  LDS words only cross here: global loads / stores in flight stay in flight (common.hpp)
    }
    if constexpr (kSeeded<Q>) lds_barrier();              // D: the coder's D (the coders exchange their cursors)
}

// ---- role 0, phase 1 (wavefront 0, for both chains): the arena from the lanes' states, then -- xwide v4 -- the spill the main decoder left
template <int Q> __device__ __forceinline__ void tail_assemble(const RansTail<Q> &t)
{
    using TL = RansTail<Q>;
    const int lane = tail_lane();
    uint32_t *const sh_pay = t.sh_pay;
#pragma unroll
    for (int qq = 0; qq < Q; ++qq) sh_pay[64 * qq + lane] = 0;
    if (lane < 2) sh_pay[64 * Q + lane] = 0;
    __builtin_amdgcn_wave_barrier();                      // same wavefront, in-order LDS
#pragma unroll
    for (int qq = 0; qq < Q; ++qq) {
        const uint32_t xl = t.rstate[((long)t.sidx * Q + qq) * 64 + lane] & 0x7FFFFFFFu;
        lds_or_bits(sh_pay, kRansStateBits * (64 * qq + lane), 16, xl & 0xFFFFu);
        lds_or_bits(sh_pay, kRansStateBits * (64 * qq + lane) + 16, kRansStateBits - 16, xl >> 16);
    }
    if constexpr (kSeeded<Q>) {
        // the spill: bits [0, E) of the stream's bit region (slot + 4), behind the payload's 248 dwords; what lies above it in the region is not the tail's
        if (lane < TL::kSpillDw) {
            const uint32_t w = reinterpret_cast<const uint32_t *>(t.slots + t.rslot_off[t.sidx] + 4)[lane];
            const int nb = min(max(t.alen - TL::GEO::kPayBits - 32 * lane, 0), 32);
            sh_pay[TL::GEO::kPayDw + lane] = nb >= 32 ? w : (w & ((1u << nb) - 1u));
        }
    }
}

// The coder's registers: the state (wave-uniform: kept scalar), the bit cursor -- plain chains and xwide chain B read DOWN to it, xwide
// chain A reads UP from it -- and, xwide with one chain, its end marker (the bits it may read end there).
struct TailCoder { uint32_t xt; int tc, a_end; };

// ---- role 0, phase 2: the chain's final state and where its bits begin, once per framing
template <int Q> __device__ __forceinline__ TailCoder tail_start_state(RansTail<Q> &t)
{
    using TL = RansTail<Q>;
    const int lane = tail_lane(), alen = t.alen;
    const uint32_t *const sh_pay = t.sh_pay;
    TailCoder c;
    c.a_end = alen;
    if constexpr (kSeeded<Q>) {
        // final states at fixed places: chain A's in bits [0, 32), chain B's in the arena's top 32 bits
        c.xt = !t.live ? (1u << 31) : (uint32_t)__builtin_amdgcn_readfirstlane((int)(t.chain ? lds_get_bits(sh_pay, alen - 32, 32) : sh_pay[0]));
        c.tc = t.chain ? alen - (t.live ? 32 : 0) : 32;
        if (t.shape.nch == 2) { if (!(c.xt >> 31)) { t.bad = true; c.xt |= 1u << 31; } }
        else {
            // one chain: the arena's highest set bit above the state is the chain's end marker (a spill ends with it)
            int top = -1;
            for (int d0 = 64 * ((TL::kArenaDw - 1) / 64); d0 >= 0 && top < 0; d0 -= 64) {
                const int d = d0 + lane;
                const uint32_t w = (d >= 1 && d < TL::kArenaDw) ? sh_pay[d] : 0u;
                const uint64_t nz = ballot64(w != 0);
                if (nz) {
                    const int hl = 63 - __clzll((long long)nz);
                    top = 32 * (d0 + hl) + 31 - __clz((int)__builtin_amdgcn_readlane((int)w, hl));
                }
            }
            if (top < 32 || (alen > TL::GEO::kPayBits && top != alen - 1)) { t.bad = true; top = 32; }
            c.a_end = top;
        }
    } else {
        int top = -1;                                                          // the payload's highest set bit
#pragma unroll
        for (int qq = Q - 1; qq >= 0; --qq) {
            const uint64_t nz = ballot64(sh_pay[64 * qq + lane] != 0);
            if (top < 0 && nz) {
                const int hd = 64 * qq + 63 - __clzll((long long)nz);
                top = 32 * hd + 31 - __clz((int)sh_pay[hd]);
            }
        }
        // a malformed stream still gets its T tail pixels written (from whatever state there is): the output of a flagged image
        // must not depend on what the workspace held
        if (top < 31) t.bad = true;
        c.xt = (top >= 31) ? (uint32_t)__builtin_amdgcn_readfirstlane((int)lds_get_bits(sh_pay, top - 31, 32)) : (1u << 31);
        c.tc = (top >= 31) ? top - 31 : 0;
    }
    return c;
}

// The renormalisation's bits.  The <= 16 bits a symbol takes lie in two arena dwords that depend on the cursor only: requested at the top of
// the symbol, next to the window, so that the LDS round trip runs under the search instead of behind the state update.
struct TailBits {
    uint32_t w0, w1; int base;                            // the dwords that hold bit `base` (a multiple of 32) and the 32 above
    __device__ __forceinline__ uint32_t bits(int pos, int n) const { return (uint32_t)((((uint64_t)w1 << 32) | w0) >> (pos - base)) & ((1u << n) - 1u); }      // [pos, pos + n), n <= 16, inside the two dwords
};
// A state needs nb bits of which the chain has `avail`: a sound stream has 0 <= nb <= 16 of them.  Corrupt: keep going on what is there.
__device__ __forceinline__ int tail_clamp_bits(int nb, int avail, bool &bad)
{
    if (nb > 16 || avail < nb) { bad = true; nb = max(min(nb, min(avail, 16)), 0); }
    return nb;
}
// nb bits into the state, reading DOWN to the cursor / UP from it
__device__ __forceinline__ void tail_take_down(TailCoder &c, const TailBits &w, int nb) { c.tc -= nb; c.xt = (c.xt << nb) | w.bits(c.tc, nb); }
__device__ __forceinline__ void tail_take_up(TailCoder &c, const TailBits &w, int nb) { c.xt = (c.xt << nb) | w.bits(c.tc, nb); c.tc += nb; }

// the state behind a symbol, back in [2^31, 2^32): each framing with its own `avail`.  first_coded: the encoder's first symbol, the chain's last
template <int Q> __device__ __forceinline__ void tail_renorm(RansTail<Q> &t, TailCoder &c, const TailBits &w, bool first_coded, uint32_t freq)
{
    if constexpr (kSeeded<Q>) {
        int nb = __clz((int)c.xt);
        if (t.shape.nch == 2) {
            // (never into the other chain's state; whether the chains crossed is checked at the end)
            nb = tail_clamp_bits(nb, t.chain ? c.tc - 32 : t.alen - 32 - c.tc, t.bad);
            if (t.chain) tail_take_down(c, w, nb); else tail_take_up(c, w, nb);
            c.xt |= 1u << 31;
        } else {
            // one chain: it started small and emitted nothing until its state had grown -- so once the bits below the end marker are used
            // up the decoder is in that silent start: it takes what is left (the encoder's first emission: < 16 bits) and then nothing.
            // Where bits were left, the encoder's state was in [2^31, 2^32): more than 16 is corrupt
            const int avail = c.a_end - c.tc;
            if (nb > avail) nb = max(avail, 0);
            tail_take_up(c, w, tail_clamp_bits(nb, 16, t.bad));
        }
    } else if (first_coded) t.bad = t.bad || c.xt != freq << 15;      // absorbing start, no bits
    else {
        tail_take_down(c, w, tail_clamp_bits(__clz((int)c.xt), c.tc, t.bad));
        c.xt |= 1u << 31;
    }
}

// ---- role 0, phase 3: the chain's symbols, SA per round, against what the preparing wavefronts left in buffer r & 1
template <int Q> __device__ __forceinline__ void tail_decode_rounds(RansTail<Q> &t, TailCoder &c)
{
    const int lane = tail_lane(), mc = lane % 5, we = lane / 5, max_symbol = t.max_symbol, SA = t.SA, T = t.T;      // lane = 5 we + mc: mixture component mc of window entry we
    for (int r = 0; r < t.R; ++r) {
        const int buf = r & 1;
        int vsym = 0;
        for (int i = 0; i < SA && SA * r + i < T; ++i) {
            const int sl = t.chain * kTailAhead + i;
            const uint32_t slot = c.xt & 0xFFFFu;
            // 0. the window the preparing wavefront speculated on (around the mixture's median), if it offered one: its twelve exact entries are there
            //    already -- lane k < 12 reads entry k, lane 12 the window's first index -- and the symbol is the last entry <= slot, proved when its
            //    successor is in the window too.  Everything from here to the next state is wave-uniform and meant for the scalar unit: ballot,
            //    count, two v_readlane, the state update.
            const int wv = t.sh_spec[buf][sl][min(lane, 12)];
            const bool up = kSeeded<Q> && t.chain == 0;          // xwide chain A reads UP from its cursor, everything else DOWN to it
            const int wpos = min(max(up ? c.tc : c.tc - 16, 0), t.alen);         // (a corrupt stream's cursor stays inside the arena's array)
            const TailBits bw{ (uint32_t)__builtin_amdgcn_readfirstlane((int)t.sh_pay[wpos >> 5]),
                               (uint32_t)__builtin_amdgcn_readfirstlane((int)t.sh_pay[(wpos >> 5) + 1]), wpos & ~31 };
            int wb = __builtin_amdgcn_readlane(wv, 12), np = 0;
            // (entries past the top symbol are 2^16, never <= slot; entry 0 is the floor of the search: counted whatever it holds)
            if (wb >= 0) np = __builtin_popcountll((ballot64((uint32_t)wv <= slot) & 0xFFFull) | (wb == 0 ? 1ull : 0ull));
            uint32_t vlo, vhi;
            if (np >= 1 && np <= 11) {
                vlo = (uint32_t)__builtin_amdgcn_readlane(wv, np - 1);
                vhi = (uint32_t)__builtin_amdgcn_readlane(wv, np);
            } else {
                const float mu = t.sh_cmp[buf][sl][mc], rsig = t.sh_cmp[buf][sl][5 + mc], wn = t.sh_cmp[buf][sl][10 + mc];
                const int e1 = t.sh_e1[buf][sl][lane];
                auto entry_at = [&](int idx) -> uint32_t { return tail_window_entry(t.gr, max_symbol, we, wn, mu, rsig, idx); };
                // 1. hint: the bucket of 8 entries the prepared anchors put the slot in
                const uint64_t p1 = ballot64(lane == 0 || (8 * lane <= max_symbol && e1 <= (int)slot));
                wb = max(8 * (__builtin_popcountll(p1) - 1) - 2, 0);
                // 2. proof: the 12 exact entries wb .. wb + 11; the symbol is the last one <= slot, its successor must be in the window too
                uint32_t ent = entry_at(wb + we);
                const uint64_t pw12 = ballot64(mc == 0 && we < 12 && wb + we <= max_symbol && (ent <= slot || wb + we == 0));
                np = __builtin_popcountll(pw12);
                if (np == 0 || np == 12) {
                    // the hint was wrong (only absurd mixtures get here): exact 13-ary search from scratch, then the window at the result
                    int lo = 0, hi = max_symbol + 1;
                    while (hi - lo > 1) {
                        const int stp = (hi - lo + 12) / 13;
                        const int pi = min(lo + stp * (min(we, 11) + 1), hi - 1);
                        const uint32_t e = entry_at(pi);
                        const uint64_t pb = ballot64(mc == 0 && we < 12 && e <= slot);
                        const int k = __builtin_popcountll(pb);                        // probes are ordered: the passes form a prefix
                        const int nlo = (k > 0) ? min(lo + stp * k, hi - 1) : lo;
                        const int nhi = (k < 12) ? min(lo + stp * (k + 1), hi - 1) : hi;
                        lo = nlo; hi = nhi;
                    }
                    wb = lo;
                    ent = entry_at(wb + we);
                    np = 1;
                }
                vlo = (uint32_t)__builtin_amdgcn_readlane((int)ent, 5 * (np - 1));
                vhi = (uint32_t)__builtin_amdgcn_readlane((int)ent, 5 * np);
            }
            vsym = (lane == i) ? wb + np - 1 - t.shift : vsym;      // the round's pixels are stored together, lane i symbol i (one vector store per round instead of a masked block per symbol)
            c.xt = (vhi - vlo) * (c.xt >> 16) + slot - vlo;
            tail_renorm(t, c, bw, SA * r + i == T - 1, vhi - vlo);
        }
        if (lane < SA && SA * r + lane < T) t.store_pixel(t.sh_off[buf][t.chain * kTailAhead + lane], vsym);
        lds_barrier();      // C: the preparing wavefronts' C behind round r.  LDS words only cross here: global loads / stores in flight stay in flight (common.hpp)
    }
}

// ---- role 0, phase 4: the chain is back at its start state -- the seeds' pixels and the end checks
template <int Q> __device__ __forceinline__ void tail_finish(RansTail<Q> &t, const TailCoder &c)
{
    using TL = RansTail<Q>;
    const int lane = tail_lane();
    bool bad = t.bad;
    if constexpr (kSeeded<Q>) {
        // Two chains: 2^31 | its n seed symbols in radix A (lane i: digit i = the stream's (chain n + i)-th symbol from the end).  One chain: the
        // stream's last symbol itself (zero if the stream has none), every bit below the end marker read.
        const int nch = t.shape.nch, sn = t.shape.sn;
        const uint32_t A = (uint32_t)(t.max_symbol + 1), v = (nch == 2) ? (c.xt & 0x7FFFFFFFu) : c.xt;
        bad = bad || (t.live && (nch == 2 ? v >= t.pw : (v >= A || c.tc != c.a_end)));
        uint32_t div = 1;
        for (int e = 0; e < min(lane, sn); ++e) div *= A;
        const int dg = (lane < sn) ? (int)((v / div) % A) : 0;
        const int j = t.shape.seed_index(t.chain, lane);
        if (t.live && lane < sn && j < t.shape.NS) {
            const auto pp = t.pos(j);
            t.store_pixel(t.pixel_off(pp.pi, pp.pj), dg - t.shift);
        }
        bad = bad || ballot64(t.live && lane < sn && j >= t.shape.NS && dg != 0) != 0;      // digits of symbols the stream does not have
        if (lane == 0) t.sh_cur[t.chain] = c.tc;
        lds_barrier();                                    // D: the preparing wavefronts' D -- the coders exchange their cursors
        if (t.chain == 0 && nch == 2) {
            // the chains must not have crossed, and what lies between them is zero
            const int ca = t.sh_cur[0], cb = t.sh_cur[1];
            uint32_t nz = 0;
            for (int d = lane; d < TL::kArenaDw; d += 64) {
                const int lo = max(ca, 32 * d), hi = min(cb, 32 * d + 32);
                if (lo < hi) nz |= t.sh_pay[d] & ((hi - lo == 32) ? 0xFFFFFFFFu : (((1u << (hi - lo)) - 1u) << (lo - 32 * d)));
            }
            bad = bad || ca > cb || ballot64(nz != 0) != 0;
        }
        if (bad && lane == 0) flag_image(t.status, t.b, LLICTI_EFORMAT);
    } else {
        if (t.T == 0) bad = bad || c.xt != (1u << 31);
        if ((bad || c.tc != 0) && lane == 0) flag_image(t.status, t.b, LLICTI_EFORMAT);
    }
}

// One workgroup per stream: per chain a coder wavefront and kTailAhead preparing ones.  The two roles meet at barriers A (the arena is
// assembled), B (round 0 is prepared), C (one per round, R of them) and -- xwide -- D (the coders' cursors): neither role returns early.
template <int Q>
__global__ __launch_bounds__(tail_threads<Q>) void rans_tail_kernel(const float *__restrict__ params, const StageGeom *__restrict__ sgv, const StreamRef *__restrict__ sref,
                                                       const uint32_t *__restrict__ rstate, const uint32_t *__restrict__ rpos,
                                                       const uint32_t *__restrict__ rtail,
                                                       int16_t *__restrict__ planes, float *__restrict__ fplanes,
                                                       const int32_t *__restrict__ minmax, int32_t *status,
                                                       const uint8_t *__restrict__ slots, const long *__restrict__ rslot_off,
                                                       const int *__restrict__ act = nullptr)
{
    using TL = RansTail<Q>;
    __shared__ uint32_t sh_pay[64 * Q + 2 + TL::kSpillDw];
    __shared__ float sh_cmp[2][TL::NSL][16];
    __shared__ int sh_e1[2][TL::NSL][64];
    __shared__ long sh_off[2][TL::NSL];
    __shared__ int sh_spec[2][TL::NSL][16];
    __shared__ int sh_cur[2];
    TL t{ params, rstate, planes, fplanes, status, slots, rslot_off, sh_pay, sh_cmp, sh_e1, sh_off, sh_spec, sh_cur };
    tail_open(t, sgv, sref, rpos, rtail, minmax, act);
    if (t.role != 0) tail_prepare_role(t);
    else {
        if (t.wave == 0) tail_assemble(t);                // (for both chains)
        __syncthreads();                                  // A: the preparing wavefronts' A -- the arena is assembled
        TailCoder c = tail_start_state(t);
        __syncthreads();                                  // B: the preparing wavefronts' B -- round 0 is prepared
        tail_decode_rounds(t, c);                         // C, once per round
        tail_finish(t, c);                                // D (xwide)
    }
}

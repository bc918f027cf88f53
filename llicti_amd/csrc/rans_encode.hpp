// rans_encode.hpp -- LLICTI-rANS v3 / xwide v4 encoder: the "auto" stream-count sum and rans_encode_kernel<Q> in its four phases (seeded or plain
// tail, main coder over the stages, finish).  The container is described in rans_coder.hpp, whose helpers (wave_incl_scan, the LDS bit helpers)
// this file uses.  Part of the single translation unit llicti_hip.hip (included in order; not a stand-alone header).
#pragma once

// encoder renormalisation: the smallest n with (x >> n) < freq << 16, x in [2^31, 2^32), 1 <= freq <= 2^16
__device__ __forceinline__ int rans_emit_bits(uint32_t x, uint32_t freq)
{
    if (freq >= 0x10000u) return 0;
    const int n0 = __clz((int)freq) - 16;                 // 32 - bit length of (freq << 16)
    return n0 + (((x >> n0) >= (freq << 16)) ? 1 : 0);
}
// the same for ANY state 0 <= x < 2^32 (the one-chain tail of an xwide v4 stream starts from a small state: nothing to emit until it has grown)
__device__ __forceinline__ int rans_emit_bits_any(uint32_t x, uint32_t freq)
{
    if (freq >= 0x10000u) return 0;
    const int n0 = max(__clz((int)freq) - 16 - __clz((int)x), 0);
    return n0 + (((x >> n0) >= (freq << 16)) ? 1 : 0);
}
// C(s, x) = (x / freq) << 16 + x % freq + lo for x < freq << 16: the quotient fits 16 bits, so a float reciprocal estimate
// is off by at most one and one signed remainder test repairs it (8 operations instead of a 32-bit division)
__device__ __forceinline__ uint32_t rans_push(uint32_t x, uint32_t lo, uint32_t freq)
{
    const uint32_t q = (uint32_t)((float)x * __builtin_amdgcn_rcpf((float)freq));
    const int32_t r = (int32_t)(x - q * freq);
    const bool neg = r < 0, big = r >= (int32_t)freq;                            // selects, not branches: the push is on the coder's dependency chain
    const uint32_t q2 = q + (big ? 1u : 0u) - (neg ? 1u : 0u);
    const int32_t r2 = r + (neg ? (int32_t)freq : 0) - (big ? (int32_t)freq : 0);
    return (q2 << 16) + (uint32_t)r2 + lo;
}
// "auto" xwide encodes (LLICTI_MODE_RANS_X_AUTO; host_types.hpp: rans_auto_pick): the weights 16 - floor(log2 freq) of the symbols of an image's
// LAST stage -- the pairs are all there before the coder runs -- are summed into ssum[b] (zeroed by header_write_kernel at the start of the call;
// kAutoSlices workgroups per image: one per image walked its 98,304 pairs of a 768x512 image in 384 dependent trips, 0.2 ms of a 0.3 ms coder), and
// every coder / pack workgroup works the image's stream count out of the sum itself.  A pure function of the image.
constexpr int kAutoSlices = 48;
__global__ __launch_bounds__(256) void choose_streams_kernel(const uint32_t *__restrict__ pairs, const StreamDesc *__restrict__ desc, int B,
                                                             unsigned long long *__restrict__ ssum)
{
    const int b = blockIdx.y;
    const StreamDesc dl = desc[(long)(LLICTI_NSTREAMS - 1) * B + b];
    const uint32_t *pl = pairs + dl.pair_off;
    long long s = 0;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < dl.n; i += 256 * kAutoSlices) s += pair_weight(CodedPair(pl[i]).freq);
    __shared__ long long sh[256];
    sh[threadIdx.x] = s;
    __syncthreads();
    for (int k = 128; k > 0; k >>= 1) { if ((int)threadIdx.x < k) sh[threadIdx.x] += sh[threadIdx.x + k]; __syncthreads(); }
    if (threadIdx.x == 0 && sh[0]) atomicAdd(&ssum[b], (unsigned long long)sh[0]);
}
// What every phase of rans_encode_kernel<Q> knows: the call's pairs, the workgroup's stream and slot, the thread's place, the kernel's LDS.
template <int Q> struct RansEnc {
    static constexpr int L = RansGeo<Q>::kLanes;
    // dwords: one flush = one dword per thread; a step adds at most kFlush / 2, a round of four steps 2 kFlush.  Ring of 8 flush units: when a
    // round's barrier opens, up to 3 kFlush dwords are waiting (a leftover below one unit + the previous round's), the round's own ORs reach
    // 2 kFlush + 1 further -- below wbase + 5 kFlush + 2 -- while slower wavefronts may still be reading / zeroing [wbase, wbase + 2 kFlush):
    // with 4 units (the size the one-step-per-round form needed) those ORs wrapped onto the units being flushed whenever the wavefronts
    // of a stream drifted apart -- never in a test that had the chip to itself, at once under a second context's kernels (bench.py's
    // overlapped_streams leg caught it; tests/test_hip_parity.py::test_two_contexts_concurrently_bitexact now does).
    static constexpr int kFlush = 64 * Q, kWin = 8 * kFlush, kPayLds = 64 * Q + kRansSpillMax / 32 + 8;
    const uint32_t *pairs; const StreamDesc *desc;
    int B, sidx, b, m, M;                           // images of the call; the stream, its image, its index among the image's streams, the image's stream count (images of a call may differ)
    int tid, lane, wq;                              // wavefront wq codes sub-chunk wq (stream lanes 64 wq .. 64 wq + 63); scalar: what depends on it alone branches on the scalar unit
    StreamDesc dl; int cnt;                         // the image's last stage and the stream's symbols of it
    uint8_t *slot; uint32_t *out32; int cap_dw;     // the stream's slot, its bit region, dwords the bit region may take
    uint32_t *sh_pay;                               // the tail coder's output (xwide v4: payload ++ spill) / the final states (62 Q dwords used, the rest slack)
    uint32_t *sh_win;                               // staging RING of the bit region: stream dword d at sh_win[d & (kWin - 1)], d in [wbase, wbase + kWin)
    int (*sh_tot)[Q][4];                            // a round's four bit totals per sub-chunk (ping-pong by round parity)
    int bad;                                        // 1: a malformed pair or seed symbol, 2: the slot is too small
    __device__ __forceinline__ uint32_t last_pair(int q) const { return pairs[dl.pair_off + rans_stream_pos(q, m, M, L)]; }      // the stream's q-th symbol of the last stage
};
// a field of at most 32 bits ORed at bit position pos into the ring, both dwords, unconditionally (a field of no bits ORs zeros)
template <int Q> __device__ __forceinline__ void ring_or(uint32_t *sh_win, int pos, uint32_t fld)
{
    const int sh = pos & 31;
    atomicOr(&sh_win[(pos >> 5) & (RansEnc<Q>::kWin - 1)], fld << sh);
    atomicOr(&sh_win[((pos >> 5) + 1) & (RansEnc<Q>::kWin - 1)], (uint32_t)(((uint64_t)fld << sh) >> 32));
}

// ---- tail, xwide v4 (seeded).  (host_types.hpp, oracle/llicti_oracle.h): ONE chain that starts from the stream's last symbol itself (raw)
// and emits nothing while its state is small, or TWO seeded chains where symbols are expensive -- chain c on wavefront c.  The chains are independent
// but for the stop rule, which looks at both: they run in blocks of 32 steps, record (field, bits) of every step in symbol order and their states of the
// last two blocks, and meet at a barrier after each block.  The output ("arena") is not cut to the payload: symbols are taken until, at a
// multiple of 32 counted from the stream's end, it has reached the payload's 7,936 bits -- so the recursion runs one block past the block that
// got there -- and what exceeds the payload (< 512 bits, the spill) is handed to the main coder as the bottom of its bit region.  Where
// exactly the rule stops -- T -- and where each field goes are prefix sums over the records, done by all 256 threads.
struct SeededTailLds {
    uint32_t *fld;                  // (field, bits) of every tail step, in symbol order: up to 8,160 of them (a tail of 2,047 symbols fills the 7,936-bit payload only at 3.9 bits per symbol; the trained model's last stage costs 1.7)
    uint32_t (*xs)[2][34];          // [block parity][chain]: the state at the block's start, then behind each of its steps
    int (*used)[2], (*scan)[4], *cut;
};
struct SeededTail { int T, tail_single, alen; };      // tail symbols; the tail has one chain, not two (bit 8 of the stream's header field); bits of the tail coder's output: what exceeds the payload starts the main bit region
template <int Q> __device__ __forceinline__ SeededTail encode_tail_seeded(RansEnc<Q> &e, const SeededTailLds &t, const StageGeom &sgl, const int16_t *__restrict__ planes,
                                                         const int32_t *__restrict__ minmax)
{
    using GEO = RansGeo<Q>;
    constexpr int L = GEO::kLanes, kFlush = RansEnc<Q>::kFlush, kWin = RansEnc<Q>::kWin;
    const int tid = e.tid, lane = e.lane, wq = e.wq, cnt = e.cnt;
    uint32_t *const sh_pay = e.sh_pay, *const sh_win = e.sh_win;
    int minv, maxv, shift;
    clr_range(minmax + 4 * e.b, 2, minv, maxv, shift);
    const int A = maxv - minv + 1;
    uint32_t pw;
    const int ns = rans_seed_count(A, pw);
    // one chain or two (the rule of oracle/llicti_oracle.c, rans_tail_encode_x: a second chain pays when symbols are expensive): on the
    // stream's last up to 64 symbols, two iff ns * mean(16 - floor(log2 freq)) >= 32 + ns / 2 -- every wavefront computes it for itself
    int nch = 1;
    if (cnt >= 2 * ns) {
        const int k64 = min(cnt, 64);
        const int wgt = (lane < k64) ? pair_weight(CodedPair(e.last_pair(cnt - 1 - lane)).freq) : 0;
        const int wsum = __builtin_amdgcn_readlane(wave_incl_scan(wgt), 63);
        if (2 * wsum * ns >= k64 * (64 + ns)) nch = 2;
    }
    const SeededTailShape shape = seeded_tail_shape(cnt, min(cnt, kRansTailMaxX), nch, ns);      // the seeds, and the candidates: coded up to where the rule stops
    const int fixed = (nch == 2) ? 64 : 33;                            // the final states; one chain: + its end marker
    const int NS = shape.NS, ncod = shape.ncod;
    const int n_own = (wq < nch) ? shape.chain_count(wq) : 0;
    const int nblk = (shape.chain_count(0) + 31) >> 5;                 // chain A's steps, in blocks
    uint32_t xc = (nch == 2) ? (1u << 31) : 0u;
    if (wq < nch) {
        const int j = shape.seed_index(wq, lane);
        int term = 0;
        if (lane < shape.sn && j < cnt) {
            const int n = rans_stream_pos(cnt - 1 - j, e.m, e.M, L);
            const int pi = div_wc(sgl, n), pj = n - pi * sgl.wc;
            int sv = (int)planes[sgl.img_off + 2 * sgl.plane + ((long)(2 * pi + sgl.oi) << sgl.lvl) * sgl.W + ((long)(2 * pj + sgl.oj) << sgl.lvl)] + shift;
            if (sv < 0 || sv >= A) { e.bad = 1; sv = 0; }
            uint32_t mul = 1;
            for (int k = 0; k < lane; ++k) mul *= (uint32_t)A;
            term = (int)((uint32_t)sv * mul);                         // the sum is below A^n <= 2^31
        }
        xc += (uint32_t)__builtin_amdgcn_readlane(wave_incl_scan(term), 63);
    }
    auto fetch_blk = [&](int blk) -> uint32_t {     // lane t < 32: step 32 blk + t of the wavefront's chain
        const int i = 32 * blk + (lane & 31);
        return (i < n_own) ? e.last_pair(cnt - 1 - shape.index(wq, i)) : 0u;
    };
    int used = 0, blk = 0, prev_tot = 0;
    uint32_t raw = fetch_blk(0);
    if (wq < 2 && lane == 0) { t.xs[0][wq][0] = xc; t.used[0][wq] = 0; }      // (a stream with nothing to code: the start states are the final ones)
    if (nblk > 0)
    for (;; ++blk) {                                // workgroup-uniform
        const uint32_t rawn = fetch_blk(blk + 1);
        if (wq < 2) {                               // (an idle chain B records no steps and reports 0 bits)
            const int nst = min(32, n_own - 32 * blk);
            if (lane == 0) t.xs[blk & 1][wq][0] = xc;
            uint32_t recv = 0, xsv = 0;             // lane t: step t's record and the state behind it -- written to LDS once per block, not once per step
            for (int s = 0; s < nst; ++s) {
                const CodedPair p((uint32_t)__builtin_amdgcn_readlane((int)raw, s));
                e.bad = p.wrong ? 1 : e.bad;
                const int nb = rans_emit_bits_any(xc, p.freq);
                recv = (lane == s) ? ((xc & ((1u << nb) - 1u)) | ((uint32_t)nb << 16)) : recv;
                used += nb;
                xc = rans_push(xc >> nb, p.lo, p.freq);
                xsv = (lane == s) ? xc : xsv;
            }
            if (lane < nst) { t.fld[nch * (32 * blk + lane) + wq] = recv; t.xs[blk & 1][wq][lane + 1] = xsv; }
            if (lane == 0) t.used[blk & 1][wq] = used;
        }
        __syncthreads();
        raw = rawn;
        const bool full_before = blk > 0 && prev_tot + fixed >= GEO::kPayBits;      // the payload was full a block ago: the stopping multiple of 32 lies in this block or the one before
        prev_tot = t.used[blk & 1][0] + t.used[blk & 1][1];
        if (full_before || blk + 1 >= nblk) break;
    }
    const int nrun = (nblk > 0) ? min(32 * nch * (blk + 1), ncod) : 0;     // records there are
    // Where the rule stops (tcod) and where each field goes are prefix sums over the records: thread tid takes records
    // 2048 q + 8 tid .. + 7 of quarter q (a long tail of a cheap source has up to four), the chains' bit counts before a quarter carried
    // over from the quarters in front of it.  One pass: every record of this thread goes to f as (index, on chain B, bits, field, the bits of
    // chain A / chain B in front of it); returns the chains' totals.  Two barriers per quarter.
    struct Bits { int a, b; };
    auto each_record = [&](auto &&f) -> Bits {
        Bits base{ 0, 0 };                          // bits of chain A / chain B in the quarters before the current one
        for (int q = 0; q < (nrun + 2047) >> 11; ++q) {
            int nbv[8], sa = 0, sb = 0;
            uint32_t fv[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const int idx = 2048 * q + 8 * tid + k;
                const uint32_t r = (idx < nrun) ? t.fld[idx] : 0u;
                nbv[k] = (int)(r >> 16); fv[k] = r & 0xFFFFu;
                if (nch == 2 && (k & 1)) sb += nbv[k]; else sa += nbv[k];      // record 2048 q + 8 tid + k belongs to chain B (2048 and 8 are even)
            }
            const int ia = wave_incl_scan(sa), ib = wave_incl_scan(sb);
            __syncthreads();                            // (the previous use of t.scan has been read)
            if (lane == 63) { t.scan[0][wq] = ia; t.scan[1][wq] = ib; }
            __syncthreads();
            int ca = base.a + ia - sa, cb = base.b + ib - sb;      // exclusive prefixes of this thread's records
            for (int w2 = 0; w2 < 4; ++w2) {
                if (w2 < wq) { ca += t.scan[0][w2]; cb += t.scan[1][w2]; }
                base.a += t.scan[0][w2]; base.b += t.scan[1][w2];
            }
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const bool onb = nch == 2 && (k & 1);
                f(2048 * q + 8 * tid + k, onb, nbv[k], fv[k], ca, cb);
                if (onb) cb += nbv[k]; else ca += nbv[k];
            }
        }
        return base;
    };
    if (tid == 0) t.cut[0] = nrun;
    __syncthreads();
    int first = 0x7FFFFFFF;                         // 1. the first record at a multiple of 32 symbols (from the stream's end) in front of which the arena has reached the payload
    each_record([&](int idx, bool, int, uint32_t, int ca, int cb) {
        if (((NS + idx) & (kRansTailBlock - 1)) == 0 && ca + cb + fixed >= GEO::kPayBits && idx < nrun && first == 0x7FFFFFFF) first = idx;
    });
    if (first != 0x7FFFFFFF) atomicMin(&t.cut[0], first);
    __syncthreads();
    const int tcod = t.cut[0];                      // coded symbols
    if (tid == 0 && tcod == nrun) { t.cut[1] = -1; t.cut[2] = -1; }
    const Bits all = each_record([&](int idx, bool, int, uint32_t, int ca, int cb) {      // 2. the chains' bits up to there
        if (idx == tcod) { t.cut[1] = ca; t.cut[2] = cb; }
    });
    __syncthreads();
    if (tid == 0 && (t.cut[1] < 0 || nrun == 0)) { t.cut[1] = all.a; t.cut[2] = all.b; }      // every record is coded: the totals
    __syncthreads();
    const int used_a = t.cut[1], used_b = t.cut[2];
    const int alen = max(GEO::kPayBits, fixed + used_a + used_b);     // the arena: payload ++ spill
    each_record([&](int idx, bool onb, int nb, uint32_t fld, int ca, int cb) {      // 3. the fields to their places: chain A's upwards from bit 32 in the decoder's reading order, chain B's below its state
        if (idx < tcod) lds_or_bits(sh_pay, onb ? alen - 32 - used_b + cb : 32 + used_a - ca - nb, nb, fld);
    });
    if (tid == 0) {
        // the chains' states behind their last coded step: s steps in, i.e. entry s - 32 b of block b = min(s / 32, the last block run)
        auto state_of = [&](int c, int steps) -> uint32_t { const int bb = min(steps >> 5, blk); return t.xs[bb & 1][c][steps - 32 * bb]; };
        sh_pay[0] = state_of(0, (tcod + nch - 1) / nch);
        if (nch == 2) {
            const uint32_t xb = state_of(1, tcod >> 1);
            lds_or_bits(sh_pay, alen - 32, 16, xb & 0xFFFFu);
            lds_or_bits(sh_pay, alen - 16, 16, xb >> 16);
        } else lds_or_bits(sh_pay, 32 + used_a, 1, 1u);      // one chain: the end marker behind its last field -- the arena's highest set bit
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < kWin; k += kFlush) sh_win[k + tid] = 0;
    __syncthreads();
    // the spill -- arena bits [7936, alen): whole dwords of sh_pay, the payload being 248 of them -- is the bottom of the main bit region
    if (tid < kRansSpillMax / 32 + 1) sh_win[tid] = sh_pay[GEO::kPayDw + tid];
    __syncthreads();
    return SeededTail{ NS + tcod, nch == 1, alen };
}

// ---- tail, 64 / 128 lanes: the stream's last T symbols of the last stage, last symbol first, single state; bits go UP from bit 0 of
//    the payload, the final state (32 bits, leading one = highest set bit of the payload) on top.  The recursion is serial and
//    wave-uniform (every wavefront runs it, on its scalar unit; thread 0 writes): what a symbol costs is its dependency chain, so
//    the chain holds nothing but the state update -- the pairs come out of a register by v_readlane (64 at a time, the next 64 in
//    flight), the emitted bits collect in a 64-bit accumulator and reach LDS a dword at a time.  (Round 3 read every pair from LDS
//    and ORed every bit field into LDS with an atomic: ~700 cycles a symbol; an xwide stream has ~620 tail symbols.)  Returns T.
template <int Q> __device__ __forceinline__ int encode_tail_plain(RansEnc<Q> &e)
{
    using GEO = RansGeo<Q>;
    const int tid = e.tid, lane = e.lane, cnt = e.cnt;
    uint32_t *const sh_pay = e.sh_pay;
    auto fetch_blk = [&](int q1) -> uint32_t {      // lane t: the t-th symbol from the end of the q1 symbols that are left
        const int q = q1 - 1 - lane;
        return (q >= 0) ? e.last_pair(q) : 0u;
    };
    int T = 0, tb = 0;
    uint32_t xt = 1u << 31;
    uint64_t acc = 0;                               // emitted bits not yet in LDS: the low accn (< 32) bits
    int accn = 0, wdw = 0;
    bool full = false;
    uint32_t raw = fetch_blk(cnt);
    for (int q1 = cnt; q1 > 0 && !full; q1 -= 64) {
        const uint32_t rawn = fetch_blk(q1 - 64);
        const int nblk = min(64, q1);
        for (int s = 0; s < nblk; ++s) {
            if (T >= kRansTailMax) { full = true; break; }
            const CodedPair p((uint32_t)__builtin_amdgcn_readlane((int)raw, s));
            e.bad = p.wrong ? 1 : e.bad;
            if (T == 0) xt = p.freq << 15;          // absorbing start: the first pushed symbol codes to 2^31 + c_low, no bits
            const int nb = (T == 0) ? 0 : rans_emit_bits(xt, p.freq);      // (the closed form needs x >= 2^31)
            if (tb + nb + 32 > GEO::kPayBits) { full = true; break; }
            acc |= (uint64_t)(xt & ((1u << nb) - 1u)) << accn;
            accn += nb;
            tb += nb;
            if (accn >= 32) {                        // wave-uniform
                if (tid == 0) sh_pay[wdw] = (uint32_t)acc;
                ++wdw; acc >>= 32; accn -= 32;
            }
            xt = rans_push(xt >> nb, p.lo, p.freq);
            ++T;
        }
        raw = rawn;
    }
    acc |= (uint64_t)xt << accn;                     // the final state on top: accn + 32 <= 63 bits
    if (tid == 0) { sh_pay[wdw] = (uint32_t)acc; if (accn > 0) sh_pay[wdw + 1] = (uint32_t)(acc >> 32); }
    __syncthreads();
    return T;
}

// ---- main coder: the lanes start from the payload; the main coder over the stages, last decoded symbol first; bits go UP from bit 0 of the bit
// region (xwide v4: from above the tail's spill, alen - payload).  Leaves the lanes' final states, the bit cursor and the ring's first dword.
struct MainCoded { uint32_t x; int bp, wbase; };
template <int Q> __device__ __forceinline__ MainCoded encode_stages(RansEnc<Q> &e, int T, int alen)
{
    using GEO = RansGeo<Q>;
    constexpr int L = GEO::kLanes, kFlush = RansEnc<Q>::kFlush, kWin = RansEnc<Q>::kWin;
    const int tid = e.tid, lane = e.lane, wq = e.wq, m = e.m, M = e.M;
    uint32_t *const sh_win = e.sh_win;
    uint32_t x = (1u << 31) | lds_get_bits(e.sh_pay, kRansStateBits * tid, kRansStateBits);      // (lane l of wavefront wq = stream lane 64 wq + l)
    const int tail_from = e.cnt - T;                // sequence position (L k + stream lane) of the first tail symbol
    int bp = alen - GEO::kPayBits, wbase = 0;       // bit cursor (xwide v4: above the tail's spill); first dword of the staging window (workgroup-uniform)
    int par = 0;                                    // parity of the coded steps (sh_tot)
    // A stage's steps of this stream: K of them (0: the stage has no chunk for stream m), its pairs, the first tail position
    struct Stg { const uint32_t *pp; int n, K, lim; };
    auto stage_of = [&](int st) -> Stg {
        if (st < 0) return Stg{ e.pairs, 1, 0, 0 };
        const StreamDesc d = e.desc[(long)st * e.B + e.b];
        const int nchunks = (d.n + L - 1) / L;
        return Stg{ e.pairs + d.pair_off, max(d.n, 1), (nchunks <= m) ? 0 : (nchunks - m + M - 1) / M,
                    (st == LLICTI_NSTREAMS - 1) ? tail_from : 0x7FFFFFFF };
    };
    // Pair loads are unconditional (clamped address); the raw value is masked only where it is consumed.
    auto fetch_of = [&](const Stg &g, int k) -> uint32_t { return g.pp[min(L * (m + max(k, 0) * M) + tid, g.n - 1)]; };
    // The pair loads do not depend on the coder state: two rounds (eight steps) are kept in flight in registers with FIXED roles (a
    // rotating ring makes the compiler copy the newest load, i.e. wait for it with s_waitcnt vmcnt(0) in every round) -- and a stage's
    // first eight are requested before the PREVIOUS stage's rounds run, so that the 45 stages do not each start with a memory round trip.
    Stg sg_cur = stage_of(LLICTI_NSTREAMS - 1);
    uint32_t a0 = fetch_of(sg_cur, sg_cur.K - 1), a1 = fetch_of(sg_cur, sg_cur.K - 2), a2 = fetch_of(sg_cur, sg_cur.K - 3), a3 = fetch_of(sg_cur, sg_cur.K - 4);
    uint32_t b0 = fetch_of(sg_cur, sg_cur.K - 5), b1 = fetch_of(sg_cur, sg_cur.K - 6), b2 = fetch_of(sg_cur, sg_cur.K - 7), b3 = fetch_of(sg_cur, sg_cur.K - 8);
    for (int st = LLICTI_NSTREAMS - 1; st >= 0; --st) {      // rANS is LIFO: last decoded symbol first
        const Stg d = sg_cur;
        const Stg sg_nxt = stage_of(st - 1);
        const uint32_t n0 = fetch_of(sg_nxt, sg_nxt.K - 1), n1 = fetch_of(sg_nxt, sg_nxt.K - 2), n2 = fetch_of(sg_nxt, sg_nxt.K - 3), n3 = fetch_of(sg_nxt, sg_nxt.K - 4);
        const uint32_t n4 = fetch_of(sg_nxt, sg_nxt.K - 5), n5 = fetch_of(sg_nxt, sg_nxt.K - 6), n6 = fetch_of(sg_nxt, sg_nxt.K - 7), n7 = fetch_of(sg_nxt, sg_nxt.K - 8);
        const int K = d.K, lim = d.lim;
        auto fetch = [&](int k) -> uint32_t { return fetch_of(d, k); };
        // FOUR steps per round.  The state recurrence of a lane -- x -> bits to emit -> push -> x -- does not depend on where the bits
        // go, and it is the only serial chain the coder has (~25 dependent operations a step); WHERE they go needs a prefix sum over
        // the stream's lanes, i.e. for a multi-wavefront stream an LDS exchange behind a barrier -- a ~350-cycle round trip that the
        // per-step form put on that chain (a step took ~2,000 cycles for ~90 instructions).  So a round first runs the recurrence
        // four steps ahead, keeping (bits, count) of each step in registers, then places the four steps' fields with ONE exchange:
        // four independent prefix sums, one 16-byte LDS write per wavefront, one barrier, four pairs of ORs.  No divergent branch: an
        // inactive lane (past the stage's end, a tail symbol, a step below 0) codes the neutral pair (freq 2^16: no bits, push discarded).
        auto round4 = [&](int k, uint32_t raw0, uint32_t raw1, uint32_t raw2, uint32_t raw3) {
            const uint32_t raws[4] = { raw0, raw1, raw2, raw3 };
            uint32_t fld[4];
            int nbs[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {                            // steps k, k - 1, k - 2, k - 3: the recurrence
                const int kk = k - j;
                const int n = L * (m + kk * M) + tid;
                const bool active = kk >= 0 && n < d.n && L * kk + tid < lim;      // (d.n >= 1: a clamped length of an empty stage, which has K = 0 and never gets here)
                const CodedPair p(active ? raws[j] : 0u);            // (lo, c_high) = (0, 2^16 stored as 0): freq 2^16, no bits
                e.bad = p.wrong ? 1 : e.bad;
                nbs[j] = rans_emit_bits(x, p.freq);
                fld[j] = x & ((1u << nbs[j]) - 1u);
                const uint32_t xn = rans_push(x >> nbs[j], p.lo, p.freq);
                x = active ? xn : x;
            }
            // placement: the decoder renormalises stream-lane-ascending reading DOWN -- the highest lane's bits lowest, i.e. sub-chunk
            // Q - 1 first -- and step k's bits below step k - 1's
            int incl[4], total[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) { incl[j] = wave_incl_scan(nbs[j]); total[j] = __builtin_amdgcn_readlane(incl[j], 63); }
            int below[4] = { 0, 0, 0, 0 }, step_total[4] = { total[0], total[1], total[2], total[3] };
            if constexpr (Q > 1) {
                if (lane == 0) *reinterpret_cast<int4 *>(&e.sh_tot[par][wq][0]) = make_int4(total[0], total[1], total[2], total[3]);
                lds_barrier();                                       // not __syncthreads(): the pair loads of the next rounds stay in flight
#pragma unroll
                for (int j = 0; j < 4; ++j) step_total[j] = 0;
#pragma unroll
                for (int q2 = 0; q2 < Q; ++q2) {
                    const int4 t4 = *reinterpret_cast<const int4 *>(&e.sh_tot[par][q2][0]);
                    const int t[4] = { t4.x, t4.y, t4.z, t4.w };
#pragma unroll
                    for (int j = 0; j < 4; ++j) { step_total[j] += t[j]; below[j] += (q2 > wq) ? t[j] : 0; }
                }
                par ^= 1;
            }
            // The ring's lowest kFlush dwords are complete once the cursor has passed them -- and every wavefront's ORs of the PREVIOUS
            // round are done once this round's barrier (above; Q = 1: same wavefront, program order) has been passed: they are written
            // out and zeroed here, one dword per thread, with no barrier of their own (this round's ORs start at bp, beyond them, and end
            // below wbase + 5 kFlush + 2: inside the ring of 8 units; a round adds at most 2 kFlush dwords).
            while (bp - 32 * wbase >= 32 * kFlush) {                 // workgroup-uniform; at most twice
                const int slot_i = (wbase + tid) & (kWin - 1);
                if (wbase + kFlush <= e.cap_dw) e.out32[wbase + tid] = sh_win[slot_i]; else e.bad = 2;
                sh_win[slot_i] = 0;
                wbase += kFlush;
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                ring_or<Q>(sh_win, bp + below[j] + (total[j] - incl[j]), fld[j]);        // nb = 0: ORs zeros
                bp += step_total[j];
            }
        };
        for (int k = K - 1; k >= 0; k -= 8) {                 // steps k .. k - 7 (those below 0 are no-ops)
            round4(k, a0, a1, a2, a3);
            a0 = fetch(k - 8); a1 = fetch(k - 9); a2 = fetch(k - 10); a3 = fetch(k - 11);
            if (k - 4 >= 0) round4(k - 4, b0, b1, b2, b3);         // workgroup-uniform
            b0 = fetch(k - 12); b1 = fetch(k - 13); b2 = fetch(k - 14); b3 = fetch(k - 15);
        }
        a0 = n0; a1 = n1; a2 = n2; a3 = n3; b0 = n4; b1 = n5; b2 = n6; b3 = n7;
        sg_cur = sg_nxt;
    }
    return MainCoded{ x, bp, wbase };
}

// ---- finish: the rest of the ring, the 64 Q final states (31 bits each), T | pad (xwide v4: the header field on top of the bit region instead), rinfo
template <int Q> __device__ __forceinline__ void encode_finish(RansEnc<Q> &e, const MainCoded &c, int T, int tail_single, int32_t *__restrict__ rinfo)
{
    using GEO = RansGeo<Q>;
    constexpr int kWin = RansEnc<Q>::kWin;
    const int tid = e.tid, wbase = c.wbase;
    uint32_t *const sh_pay = e.sh_pay, *const sh_win = e.sh_win;
    int bp = c.bp;
    __syncthreads();
    if constexpr (kSeeded<Q>) {
        // 8 bits T / 32 rounded up, 1 bit "one chain", 1 end-marker bit -- ORed into the ring above the main coder's last bit (every wavefront's
        // ORs of the last round are behind the barrier; the ring holds at least 3 flush units beyond the cursor)
        if (tid == 0) ring_or<Q>(sh_win, bp, (uint32_t)((T + kRansTailBlock - 1) / kRansTailBlock) | ((uint32_t)tail_single << 8) | (1u << 9));
        bp += 10;
        __syncthreads();
    }
    const int nbytes = (bp + 7) >> 3;
    sh_pay[tid] = 0;
    __syncthreads();
    lds_or_bits(sh_pay, kRansStateBits * tid, 16, c.x & 0xFFFFu);
    lds_or_bits(sh_pay, kRansStateBits * tid + 16, kRansStateBits - 16, (c.x >> 16) & 0x7FFFu);
    __syncthreads();
    const int ndw = (nbytes >> 2) - wbase;                    // whole ring dwords still to write (< 2 kFlush); then 0..3 bytes
    const bool over = (nbytes >> 2) + 1 > e.cap_dw;
    if (over) e.bad = 2;
    else {
        for (int k = tid; k < ndw; k += 64 * Q) e.out32[wbase + k] = sh_win[(wbase + k) & (kWin - 1)];
        if (tid < (nbytes & 3)) e.slot[4 + (nbytes & ~3) + tid] = (uint8_t)(sh_win[(wbase + ndw) & (kWin - 1)] >> (8 * tid));
        uint8_t *fs = e.slot + 4 + nbytes;
        for (int k = tid; k < GEO::kPayBytes; k += 64 * Q) fs[k] = (uint8_t)(sh_pay[k >> 2] >> (8 * (k & 3)));
    }
    if (tid == 0) {
        if constexpr (kSeeded<Q>) {
            // the stream is bit region | states: it starts at the region (slot + 4)
            rinfo[2 * e.sidx] = 4; rinfo[2 * e.sidx + 1] = (e.bad == 2) ? 0 : nbytes + GEO::kPayBytes;
        } else {
            const int t16 = (T & 0x7FF) | ((8 * nbytes - bp) << 11);      // pad: unused (zero) bits on top of the region's last byte
            e.slot[2] = (uint8_t)(t16 & 0xFF); e.slot[3] = (uint8_t)(t16 >> 8);
            rinfo[2 * e.sidx] = 2; rinfo[2 * e.sidx + 1] = (e.bad == 2) ? 0 : 2 + nbytes + GEO::kPayBytes;      // overflowed slot (never with the plan's sizing): nothing to pack, ENOSPACE is latched
        }
    }
}

// One wavefront per 64 lanes of a stream (a wide stream: two, one per sub-chunk; their bit fields interleave, so the step's bit
// totals meet in LDS behind one barrier).  Slot layout (rslot_off is 64-byte aligned): [0,2) unused | [2,4) T | [4, 4 + nbytes) bit region
// (dword aligned) | 248 Q bytes of final states; rinfo = (2, 2 + nbytes + 248 Q) for rans_pack_kernel.
template <int Q>
__global__ __launch_bounds__(64 * Q) void rans_encode_kernel(const uint32_t *__restrict__ pairs, const StreamDesc *__restrict__ desc,
                                                         int B, const StreamRef *__restrict__ sref, uint8_t *__restrict__ slots, const long *__restrict__ rslot_off,
                                                         int rslot_cap, int32_t *__restrict__ rinfo, int32_t *status,
                                                         const StageGeom *__restrict__ sglv, const int16_t *__restrict__ planes, const int32_t *__restrict__ minmax,
                                                         const unsigned long long *__restrict__ ssum, const ImgGeo *__restrict__ iv)
{
    using E = RansEnc<Q>;
    const int M_img = image_stream_count(ssum, iv, desc, B, sref[blockIdx.x].b, sref[blockIdx.x].M);
    if (sref[blockIdx.x].m >= M_img) {                                   // "auto": the image got fewer streams than the table holds for it -- this one does not exist
        if (threadIdx.x == 0) { rinfo[2 * blockIdx.x] = 4; rinfo[2 * blockIdx.x + 1] = 0; }
        return;                                                          // (whole workgroup, in front of every barrier)
    }
    __shared__ uint32_t sh_pay[E::kPayLds];
    __shared__ uint32_t sh_win[E::kWin];
    __shared__ __attribute__((aligned(16))) int sh_tot[2][Q][4];
    const int sidx = blockIdx.x, tid = threadIdx.x;
    const StreamRef sr_ = sref[sidx];
    uint8_t *slot = slots + rslot_off[sidx];
    const StreamDesc dl = desc[(long)(LLICTI_NSTREAMS - 1) * B + sr_.b];
    E e{ pairs, desc, B, sidx, sr_.b, sr_.m, M_img, tid, tid & 63, __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)),
         dl, rans_stream_count(dl.n, sr_.m, M_img, E::L), slot, reinterpret_cast<uint32_t *>(slot + 4), (rslot_cap - 4 - RansGeo<Q>::kPayBytes - 8) >> 2,
         sh_pay, sh_win, sh_tot, 0 };
    sh_pay[tid] = 0;
    if (tid < kRansSpillMax / 32 + 8) sh_pay[64 * Q + tid] = 0;
#pragma unroll
    for (int t = 0; t < E::kWin; t += E::kFlush) sh_win[t + tid] = 0;
    __syncthreads();
    SeededTail tail{ 0, 0, RansGeo<Q>::kPayBits };
    if constexpr (kSeeded<Q>) {
        __shared__ uint32_t sh_fld[kRansTailMaxX + 1];
        __shared__ uint32_t sh_xs[2][2][34];
        __shared__ int sh_used[2][2], sh_scan[2][4], sh_cut[3];
        tail = encode_tail_seeded(e, SeededTailLds{ sh_fld, sh_xs, sh_used, sh_scan, sh_cut }, sglv[sr_.b], planes, minmax);      // the image's last stage (level 0, band x10): an xwide stream's seed symbols are read from its pixels
    } else tail.T = encode_tail_plain(e);
    const MainCoded c = encode_stages(e, tail.T, tail.alen);
    encode_finish(e, c, tail.T, tail.tail_single, rinfo);
    if (e.bad) atomicExch(&status[0], e.bad == 1 ? LLICTI_EFORMAT : LLICTI_ENOSPACE);
}

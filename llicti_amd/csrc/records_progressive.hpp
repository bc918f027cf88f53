// records_progressive.hpp -- progressive records on the device (llicti_level_cuts / llicti_pack_progressive / llicti_unpack_progressive): the
// level cuts of a decode, and strided containers <-> one dense blob of "LLIP" records.  The format, the table's rules and the prefix arithmetic
// are progressive.hpp's; the kernels here run those functions with a thread per segment and per stream.
// Part of the single translation unit llicti_hip.hip (included in order; not a stand-alone header).
#pragma once
#include "progressive.hpp"

constexpr int kProgThreads = 128;                   // the check / measure / head kernels: a thread per stream (and per segment)
constexpr int kProgPer = 4;                         // pieces a thread of the copy kernel lists: 256 x 4 >= kProgMaxPieces
static_assert(kRecThreads * kProgPer >= kProgMaxPieces, "the copy kernel's piece list");
constexpr int kProgReduceMax = 1024;                // images per launch of the unpack kernels: their reduces are kernel arguments
struct ProgReduces { uint32_t w[kProgReduceMax / 8]; };      // four bits an image
__host__ __device__ __forceinline__ int prog_reduce_of(const ProgReduces &q, int i) { return (int)((q.w[i >> 3] >> (4 * (i & 7))) & 15u); }

// level_cuts: behind the three bands of level lvl >= 1, the main coder's cursor of every stream of the call as a byte offset into the stream
// (rpos holds the bit cursor between stage launches) -> cuts[b][m][lvl]
__global__ __launch_bounds__(256) void level_cuts_kernel(const uint32_t *__restrict__ rpos, const StreamRef *__restrict__ sref, int NS, int lvl,
                                                         int32_t *__restrict__ cuts)
{
    const int sidx = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (sidx >= NS) return;
    const StreamRef sr = sref[sidx];
    if (sr.m < kProgMaxStreams) cuts[((long)sr.b * kProgMaxStreams + sr.m) * LLICTI_NLEVELS + lvl] = (int32_t)(rpos[sidx] >> 3);
}
// ... and the call's last kernel: the status words into the context's (the sink of a decode that writes no pixels)
__global__ __launch_bounds__(256) void level_cuts_latch_kernel(const int32_t *__restrict__ status, int head, int32_t *__restrict__ latched,
                                                               int32_t *__restrict__ img_latched, int B)
{
    latch_status_all(status, head, latched, img_latched, B);
}

// The stream count an xwide v4 container's header names (byte 0: 0xE8 config A, 0xE9 config B; bits 10 .. 15 of the pad field), 0: none
__device__ __forceinline__ int prog_header_streams(const uint8_t *cont, int L)
{
    if (cont[0] != (L == LLICTI_NLEVELS ? 0xE8 : 0xE9)) return 0;
    const int u = (((int)cont[15] | ((int)cont[16] << 8)) >> 10) & 0x3F;
    return (u >= 1 && u <= 32) ? u : u == 33 ? 64 : u == 34 ? 128 : 0;
}
// Stream m of a container of M streams whose n segment lengths sl are non-negative and sum to S <= stride: where it lies in the payload, as
// rans_unpack_kernel finds it (M <= 32: segment 4 + m; M = 64 / 128: behind its segment's table of M / 32 lengths, which must add up)
__device__ __forceinline__ bool prog_locate(const uint8_t *cont, const int32_t *sl, int n, int M, int m, long *off, long *len)
{
    const int G = rans_group(M), sg = m / G;
    if (4 + sg >= n) return false;
    long src = 0;
    for (int k = 0; k < 4 + sg; ++k) src += sl[k];
    if (G == 1) { *off = src; *len = sl[4 + sg]; return true; }
    const long seg_n = sl[4 + sg];
    if (seg_n < 4L * G) return false;
    const uint8_t *tab = cont + src;
    long o = 4L * G, tot = 4L * G;
    bool ok = true;
    for (int k = 0; k < G; ++k) {
        const uint32_t v = prog_u32(tab + 4 * k);
        if (v >> 31) ok = false;
        if (k < m % G) o += v;
        if (k == m % G) *len = (long)v;
        tot += v;
    }
    *off = src + o;
    return ok && tot == seg_n;
}

// One image of a pack, by a workgroup of kProgThreads: -> its stream count, payload bytes and (thread m < M) stream m's place and cuts; false
// (uniform) for an image whose lengths, header, length tables or cuts do not hold together.  sh: 8 + LLICTI_NLEVELS words of LDS.
struct ProgImage { int M; long S, off, len, piece[LLICTI_NLEVELS]; };
__device__ __forceinline__ bool prog_measure(const uint8_t *cont, long stride, const int32_t *sl, int n, int L, const int32_t *cuts, ProgImage *im,
                                             unsigned long long *sh)
{
    const int tid = (int)threadIdx.x;
    if (tid < 8 + LLICTI_NLEVELS) sh[tid] = 0ull;
    __syncthreads();
    if (tid < n) {
        const int v = sl[tid];
        if (v < 0) atomicOr(&sh[0], 1ull); else atomicAdd(&sh[1], (unsigned long long)v);
    }
    __syncthreads();
    const long S = (long)sh[1];
    // (S below 2^31: the record stores every offset and length in 32 bits, and the unpack refuses a word of 2^31 or more)
    bool ok = sh[0] == 0 && S <= stride && S < (1L << 31) && sl[0] == 3 && sl[1] == 12 && sl[2] == 2;
    const int M = ok ? prog_header_streams(cont, L) : 0;      // (17 header bytes: inside S)
    ok = ok && M >= 1 && M / rans_group(M) <= n - 4;
    im->M = M; im->S = S;
    __syncthreads();
    if (ok && tid < M) {
        bool good = prog_locate(cont, sl, n, M, tid, &im->off, &im->len);
        good = good && im->off + im->len <= S;
        long c = 0;
        const int32_t *row = cuts + (long)tid * LLICTI_NLEVELS;
#pragma unroll
        for (int l = 0; l < LLICTI_NLEVELS; ++l) {              // (constant trip count and indices: the pieces stay in registers)
            long next = im->len;
            if (l + 1 < L) {
                next = row[l + 1 < LLICTI_NLEVELS ? l + 1 : 0];
                if (next < c || next > im->len) good = false;
            }
            im->piece[l] = l < L ? next - c : 0;
            c = next;
        }
        if (good) {
            atomicAdd(&sh[2], (unsigned long long)im->len);
#pragma unroll
            for (int l = 0; l < LLICTI_NLEVELS; ++l) if (l < L) atomicAdd(&sh[8 + l], (unsigned long long)im->piece[l]);
        } else atomicOr(&sh[0], 1ull);
    }
    __syncthreads();
    return ok && sh[0] == 0;
}

// pack, step 1: a workgroup per image -- the image's prefix row P_0 .. P_L (zeros for a refused image: a zero-length record, LLICTI_EFORMAT)
__global__ __launch_bounds__(kProgThreads) void prog_measure_kernel(const uint8_t *__restrict__ cont, long stride, const int32_t *__restrict__ seg_len,
                                                                    int n, int L, const int32_t *__restrict__ cuts, int64_t *__restrict__ prefix,
                                                                    int32_t *latched, int32_t *__restrict__ img_latched)
{
    __shared__ unsigned long long sh[8 + LLICTI_NLEVELS];
    const int b = (int)blockIdx.x;
    ProgImage im;
    const bool ok = prog_measure(cont + (long)b * stride, stride, seg_len + (long)b * LLICTI_NSEG, n, L,
                                 cuts + (long)b * kProgMaxStreams * LLICTI_NLEVELS, &im, sh);
    if (threadIdx.x == 0) {
        int64_t *row = prefix + (long)b * (LLICTI_NLEVELS + 1);
        if (ok) {
            const ProgHead h = { n, L, im.M, prog_table_bytes(n, L, im.M) };
            long lvl[LLICTI_NLEVELS];
#pragma unroll
            for (int l = 0; l < LLICTI_NLEVELS; ++l) lvl[l] = (long)sh[8 + l];
            prog_prefixes(h, im.S, (long)sh[2], lvl, row);
        } else {
            for (int r = 0; r <= LLICTI_NLEVELS; ++r) row[r] = 0;
            atomicExch(latched, LLICTI_EFORMAT);
        }
        img_latched[b] = ok ? 0 : LLICTI_EFORMAT;
    }
}

// pack, step 2: record_offsets_kernel over the record sizes P_0 of the prefix rows step 1 wrote (its verdicts stand)
struct RecordSizeOfPrefix {
    const int64_t *prefix;
    __device__ __forceinline__ long long operator()(int b, int32_t *) const { return prefix[(long)b * (LLICTI_NLEVELS + 1)]; }
};

// pack, step 3: a workgroup per image writes the record's fixed bytes, lengths and table (a record that would end past blob_cap is not written)
__global__ __launch_bounds__(kProgThreads) void prog_head_kernel(const uint8_t *__restrict__ cont, long stride, const int32_t *__restrict__ seg_len,
                                                                 int n, int L, const int32_t *__restrict__ cuts, uint8_t *__restrict__ blob, long blob_cap,
                                                                 const int64_t *__restrict__ rec_off)
{
    __shared__ unsigned long long sh[8 + LLICTI_NLEVELS];
    const int b = (int)blockIdx.x, tid = (int)threadIdx.x;
    const long o0 = rec_off[b], o1 = rec_off[b + 1];
    if (o1 == o0 || o1 > blob_cap) return;
    const int32_t *sl = seg_len + (long)b * LLICTI_NSEG;
    ProgImage im;
    if (!prog_measure(cont + (long)b * stride, stride, sl, n, L, cuts + (long)b * kProgMaxStreams * LLICTI_NLEVELS, &im, sh)) return;
    uint8_t *rec = blob + o0;
    auto put32 = [](uint8_t *p, uint32_t v) { p[0] = (uint8_t)v; p[1] = (uint8_t)(v >> 8); p[2] = (uint8_t)(v >> 16); p[3] = (uint8_t)(v >> 24); };
    if (tid == 0) {
        rec[0] = 'L'; rec[1] = 'L'; rec[2] = 'I'; rec[3] = 'P'; rec[4] = kProgVersion; rec[5] = (uint8_t)n; rec[6] = (uint8_t)L; rec[7] = 0;
        rec[8] = (uint8_t)(im.M & 0xFF); rec[9] = (uint8_t)(im.M >> 8); rec[10] = 0; rec[11] = 0;
    }
    if (tid < n) put32(rec + kProgFixed + 4 * tid, (uint32_t)sl[tid]);
    if (tid < im.M) {
        uint8_t *row = rec + kProgFixed + 4L * n + 4L * tid * (L + 1);
        put32(row, (uint32_t)im.off);
        put32(row + 4, (uint32_t)im.len);
        long c = 0;
#pragma unroll
        for (int l = 1; l < LLICTI_NLEVELS; ++l) { c += im.piece[l - 1]; if (l < L) put32(row + 4 + 4 * l, (uint32_t)c); }
    }
}

// unpack, step 1: a workgroup per record.  EVERYTHING about a record is decided here, from rec_off and the record's own table, before a frame
// or piece byte is read (progressive.hpp states the rules): offsets inside the blob, the fixed bytes against the context's model, every length
// below 2^31, S <= stride, the streams ascending and disjoint inside [0, S), the cuts ascending within their stream, 0 <= r <= L and at least
// P_r bytes present.  A good record: its n lengths and zeros up to 49 in seg_len[b], status 0.  A refused one: an all-zero row,
// LLICTI_EFORMAT, and prog_copy_kernel skips it.
__global__ __launch_bounds__(kProgThreads) void prog_check_kernel(const uint8_t *__restrict__ blob, long blob_bytes, const int64_t *__restrict__ rec_off,
                                                                  int b0, int n, int L, ProgReduces red, long stride, int32_t *__restrict__ seg_len,
                                                                  int32_t *latched, int32_t *__restrict__ img_latched)
{
    __shared__ unsigned long long sh[8 + LLICTI_NLEVELS];
    const int b = b0 + (int)blockIdx.x, tid = (int)threadIdx.x, r = prog_reduce_of(red, (int)blockIdx.x);
    const long o0 = rec_off[b], o1 = rec_off[b + 1];
    if (tid < 8 + LLICTI_NLEVELS) sh[tid] = 0ull;
    __syncthreads();
    bool ok = o0 >= 0 && o0 <= o1 && o1 <= blob_bytes && r <= L;      // (uniform)
    const uint8_t *rec = blob + o0;
    ProgHead h = { 0, 0, 0, 0 };
    ok = ok && prog_head(rec, o1 - o0, n, L, &h);
    long v = 0;
    if (ok && tid < n) {
        if (prog_seg(rec, tid, &v)) atomicAdd(&sh[1], (unsigned long long)v); else atomicOr(&sh[0], 1ull);
    }
    __syncthreads();
    const long S = (long)sh[1];
    ok = ok && sh[0] == 0 && S <= stride;
    if (ok && tid < h.M) {
        long off, len, piece[LLICTI_NLEVELS];
        if (prog_stream(rec, h, tid, S, &off, &len, piece)) {
            atomicAdd(&sh[2], (unsigned long long)len);
#pragma unroll
            for (int l = 0; l < LLICTI_NLEVELS; ++l) if (l < L) atomicAdd(&sh[8 + l], (unsigned long long)piece[l]);
        } else atomicOr(&sh[0], 1ull);
    }
    __syncthreads();
    ok = ok && sh[0] == 0;
    if (ok) {
        int64_t prefix[LLICTI_NLEVELS + 1];
        long lvl[LLICTI_NLEVELS];
#pragma unroll
        for (int l = 0; l < LLICTI_NLEVELS; ++l) lvl[l] = (long)sh[8 + l];
        prog_prefixes(h, S, (long)sh[2], lvl, prefix);
        ok = o1 - o0 >= prog_prefix_at(prefix, r);
    }
    record_verdict(b, tid, n, ok, (int32_t)v, seg_len, latched, img_latched);
}

// The copy of both directions: grid (chunks, images).  A record's dense side behind its table -- the frame bytes, then the pieces level by
// level -- is cut into ranges of kRecChunk bytes; workgroup (x, b) lists the record's pieces from the record's own table (kProgPer a thread, a
// scan over the workgroup), finds the ones its range overlaps and moves each overlap with block_copy_bytes.  PACK: container -> blob, every
// level, for the records prog_head_kernel wrote; else blob -> container, the levels >= the image's reduce, for the records prog_check_kernel
// accepted: no other byte of the container is written.
template <bool PACK>
__global__ __launch_bounds__(kRecThreads) void prog_copy_kernel(uint8_t *__restrict__ blob, long blob_cap, const int64_t *__restrict__ rec_off, int b0, int b1,
                                                                ProgReduces red, uint8_t *__restrict__ cont, long stride,
                                                                const int32_t *__restrict__ img_latched)
{
    __shared__ long sh_dense[kRecThreads * kProgPer + 1], sh_pay[kRecThreads * kProgPer];
    __shared__ long long sh_scan[kRecThreads];
    __shared__ unsigned long long sh_S;
    const int tid = (int)threadIdx.x;
    for (int b = b0 + (int)blockIdx.y; b < b1; b += (int)gridDim.y) {
        if (img_latched[b] != 0) continue;
        const long o0 = rec_off[b], o1 = rec_off[b + 1];
        if (PACK && (o1 == o0 || o1 > blob_cap)) continue;
        const uint8_t *rec = blob + o0;
        ProgHead h;
        if (!prog_head(rec, o1 - o0, 0, 0, &h)) continue;             // (never: the record is the one the step before wrote / accepted)
        // The grid is sized by the longest payload the call can hold; the dense side of THIS record ends at P_r - T <= the bytes present - T
        // (a loader hands over exactly P_r, a pack P_0): a workgroup whose range starts behind that has nothing to list.  At reduce 2 or 3
        // that is fifteen of an image's sixteen.
        const long c0 = (long)blockIdx.x * kRecChunk;
        if (c0 >= o1 - o0 - h.T) continue;
        __syncthreads();                                             // (the lists of the image before are done with)
        if (tid == 0) sh_S = 0ull;
        __syncthreads();
        if (tid < h.n) { long v; prog_seg(rec, tid, &v); atomicAdd(&sh_S, (unsigned long long)v); }
        __syncthreads();
        const long S = (long)sh_S;
        const int np = prog_piece_count(h, PACK ? 0 : prog_reduce_of(red, b - b0));
        long pay[kProgPer], len[kProgPer], mine = 0;
#pragma unroll
        for (int k = 0; k < kProgPer; ++k) {
            const int i = tid * kProgPer + k;
            pay[k] = 0; len[k] = 0;
            if (i < np) prog_piece(rec, h, S, i, &pay[k], &len[k]);
            mine += len[k];
        }
        long at = (long)block_exclusive_scan(mine, sh_scan);
#pragma unroll
        for (int k = 0; k < kProgPer; ++k) { sh_dense[tid * kProgPer + k] = at; sh_pay[tid * kProgPer + k] = pay[k]; at += len[k]; }
        if (tid == kRecThreads - 1) sh_dense[kRecThreads * kProgPer] = at;
        __syncthreads();
        const long total = sh_dense[kRecThreads * kProgPer];          // P_r - T
        const long c1 = min(c0 + kRecChunk, total);
        if (c0 >= total) continue;
        int lo = 0, hi = np - 1;                                      // the first piece that ends behind c0
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (sh_dense[mid + 1] > c0) hi = mid; else lo = mid + 1;
        }
        uint8_t *img = cont + (long)b * stride;
        for (int i = lo; i < np && sh_dense[i] < c1; ++i) {
            const long d0 = max(c0, sh_dense[i]), d1 = min(c1, sh_dense[i + 1]);
            if (d1 <= d0) continue;
            uint8_t *dense = blob + o0 + h.T + d0, *sparse = img + sh_pay[i] + (d0 - sh_dense[i]);
            if (PACK) block_copy_bytes(dense, sparse, (int)(d1 - d0)); else block_copy_bytes(sparse, dense, (int)(d1 - d0));
        }
    }
}

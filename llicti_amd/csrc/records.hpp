// records.hpp -- .llic records on the device: strided containers <-> one dense blob of records (llicti_pack_records / llicti_unpack_records).
// Part of the single translation unit llicti_hip.hip (included in order; not a stand-alone header).
//
// A record is what fileio.dumps_llic writes for one image: b"LLIC", version 1, n, n little-endian u32 segment lengths, the n segments back
// to back.  A device container IS its segments back to back, so a record's payload is one run of sum(seg_len) bytes: packing and unpacking are
// a validation pass over the lengths (one small kernel) and one copy whose two sides are misaligned against each other by an arbitrary number
// of bytes (the 6 + 4n header bytes, records at any byte offset, callers' views at any byte offset).
#pragma once

constexpr int kRecChunk = LLICTI_RECORD_CHUNK;      // payload bytes one workgroup copies: a 4K image's tens of megabytes go over hundreds of them
constexpr int kRecThreads = 256;
constexpr int kRecVersion = 1;

__host__ __device__ __forceinline__ int record_header_bytes(int n) { return 6 + 4 * n; }

// bytes mis .. mis + 15 of the 32 bytes (a, b), mis = 4 DS + bs: v_alignbyte_b32 shifts a pair of dwords right by bs bytes
template <int DS>
__device__ __forceinline__ uint4 realign16(const uint4 a, const uint4 b, uint32_t bs)
{
    const uint32_t w[8] = { a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w };
    return make_uint4(__builtin_amdgcn_alignbyte(w[DS + 1], w[DS], bs), __builtin_amdgcn_alignbyte(w[DS + 2], w[DS + 1], bs),
                      __builtin_amdgcn_alignbyte(w[DS + 3], w[DS + 2], bs), __builtin_amdgcn_alignbyte(w[DS + 4], w[DS + 3], bs));
}

template <int DS>
__device__ __forceinline__ void record_copy_body(uint4 *__restrict__ d4, const uint4 *__restrict__ s4, int i0, int i1, uint32_t bs)
{
#pragma unroll 4
    for (int i = i0 + (int)threadIdx.x; i < i1; i += kRecThreads) {
        const uint4 a = s4[i], b = s4[i + 1];
        d4[i] = realign16<DS>(a, b, bs);
    }
}

// By ONE workgroup of kRecThreads: n (<= kRecChunk) bytes from src to dst, both at any byte address.  Up to 15 head bytes bring dst to a 16-byte
// boundary; the body is aligned 16-byte stores, each made from the two aligned 16-byte loads that cover its source bytes, realigned in
// registers (one load where both sides happen to agree); the tail is bytes.  No load leaves [lo, hi) (src >= lo, src + n <= hi): an aligned
// load may reach up to 15 bytes outside the chunk on either side, which is inside the caller's buffer everywhere but at the buffer's own two
// ends -- the (at most three) body vectors whose loads would cross lo or hi are copied byte by byte instead.
__device__ __forceinline__ void record_copy_chunk(uint8_t *__restrict__ dst, const uint8_t *__restrict__ src, int n,
                                                  const uint8_t *lo, const uint8_t *hi)
{
    const int tid = (int)threadIdx.x;
    const int head = min(n, (int)((16u - ((uint32_t)(uintptr_t)dst & 15u)) & 15u));
    if (tid < head) dst[tid] = src[tid];
    const int nvec = (n - head) >> 4;
    const uint8_t *s = src + head;
    uint8_t *d = dst + head;
    const uint32_t mis = (uint32_t)(uintptr_t)s & 15u;
    const uint8_t *sa = s - mis;                                        // (sa > lo - 16)
    const int i_lo = (nvec > 0 && sa < lo) ? 1 : 0;
    const long room = (long)(hi - sa) - (mis ? 32 : 16);                // vector i loads [sa + 16 i, + 16 or 32)
    int i_hi = room < 0 ? 0 : (int)min((long)nvec, room / 16 + 1);
    i_hi = max(i_hi, i_lo);
    const int n_edge = i_lo + (nvec - i_hi);                            // <= 3
    if (tid < 16 * n_edge) {
        const int k = tid >> 4, i = k < i_lo ? k : i_hi + (k - i_lo);
        d[16 * i + (tid & 15)] = s[16 * i + (tid & 15)];
    }
    uint4 *d4 = reinterpret_cast<uint4 *>(d);
    const uint4 *s4 = reinterpret_cast<const uint4 *>(sa);
    if (mis == 0) {
#pragma unroll 4
        for (int i = i_lo + tid; i < i_hi; i += kRecThreads) d4[i] = s4[i];
    } else {
        switch (mis >> 2) {
        case 0: record_copy_body<0>(d4, s4, i_lo, i_hi, mis & 3u); break;
        case 1: record_copy_body<1>(d4, s4, i_lo, i_hi, mis & 3u); break;
        case 2: record_copy_body<2>(d4, s4, i_lo, i_hi, mis & 3u); break;
        default: record_copy_body<3>(d4, s4, i_lo, i_hi, mis & 3u); break;
        }
    }
    for (int t = head + (nvec << 4) + tid; t < n; t += kRecThreads) dst[t] = src[t];
}

// By EVERY thread of a workgroup of kRecThreads: the sum of v over the threads below this one (Hillis-Steele over sh[kRecThreads]); behind it
// sh[kRecThreads - 1] is the workgroup's total.  A caller that reads sh puts a __syncthreads() between that and its next call.
__device__ __forceinline__ long long block_exclusive_scan(long long v, long long *sh)
{
    const int tid = (int)threadIdx.x;
    sh[tid] = v;
    __syncthreads();
    for (int d = 1; d < kRecThreads; d <<= 1) {
        const long long t = tid >= d ? sh[tid - d] : 0;
        __syncthreads();
        sh[tid] += t;
        __syncthreads();
    }
    return sh[tid] - v;
}

// The verdict on image b of a record call, by the threads tid of one workgroup (at least LLICTI_NSEG of them): its seg_len row -- the n
// lengths (v: thread tid's) of a good record, zeros up to 49 behind them and throughout a refused one --, img_latched[b], and the call's status.
__device__ __forceinline__ void record_verdict(int b, int tid, int n, bool ok, int32_t v, int32_t *__restrict__ seg_len, int32_t *latched,
                                               int32_t *__restrict__ img_latched)
{
    if (tid < LLICTI_NSEG) seg_len[(long)b * LLICTI_NSEG + tid] = (ok && tid < n) ? v : 0;
    if (tid == 0) {
        img_latched[b] = ok ? 0 : LLICTI_EFORMAT;
        if (!ok) atomicExch(latched, LLICTI_EFORMAT);
    }
}

// How a thread of record_offsets_kernel obtains image b's record size.  Here: from the image's n segment lengths -- 6 + 4n + sum, or 0 for a
// row with a negative entry or a sum above `stride`, which is also the image's verdict (LLICTI_EFORMAT).  (The other: RecordSizeOfPrefix.)
struct RecordSizeOfLengths {
    const int32_t *seg_len; int n; long stride; int32_t *img_latched;
    __device__ __forceinline__ long long operator()(int b, int32_t *latched) const
    {
        const int32_t *sl = seg_len + (long)b * LLICTI_NSEG;
        bool bad = false;
        long long sum = 0;
        for (int k = 0; k < n; ++k) {
            const int v = sl[k];
            if (v < 0) bad = true; else sum += v;
        }
        if (sum > stride) bad = true;
        img_latched[b] = bad ? LLICTI_EFORMAT : 0;
        if (bad) atomicExch(latched, LLICTI_EFORMAT);
        return bad ? 0 : record_header_bytes(n) + sum;
    }
};

// pack (one workgroup): the exclusive scan of the B record sizes into rec_off[0 .. B] (rec_off[B]: the total), kRecThreads images a round, and
// LLICTI_ENOSPACE where the total exceeds blob_cap.  Status goes straight into the context's latched words: the call has no workspace.
template <class SizeOf>
__global__ __launch_bounds__(kRecThreads) void record_offsets_kernel(const SizeOf size_of, int B, long blob_cap, int64_t *__restrict__ rec_off, int32_t *latched)
{
    __shared__ long long sh[kRecThreads];
    long long carry = 0;                                                // (the same in every thread)
    for (int base = 0; base < B; base += kRecThreads) {
        const int b = base + (int)threadIdx.x;
        const long long before = block_exclusive_scan(b < B ? size_of(b, latched) : 0, sh);
        if (b < B) rec_off[b] = carry + before;
        carry += sh[kRecThreads - 1];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        rec_off[B] = carry;
        if (carry > blob_cap) atomicExch(latched, LLICTI_ENOSPACE);
    }
}

// pack, step 2: grid (chunks, images).  Workgroup (x, b) writes chunk x of record b's payload; x == 0 also writes the record's 6 + 4n header
// bytes.  A record that would end past blob_cap is not written at all (the scan has latched LLICTI_ENOSPACE).
__global__ __launch_bounds__(kRecThreads) void record_pack_kernel(const uint8_t *__restrict__ cont, long stride, const int32_t *__restrict__ seg_len,
                                                                  int B, int n, uint8_t *__restrict__ blob, long blob_cap,
                                                                  const int64_t *__restrict__ rec_off)
{
    const int hdr = record_header_bytes(n), tid = (int)threadIdx.x;
    for (int b = (int)blockIdx.y; b < B; b += (int)gridDim.y) {
        const long o0 = rec_off[b], o1 = rec_off[b + 1];
        if (o1 == o0 || o1 > blob_cap) continue;
        const long pay = o1 - o0 - hdr, c0 = (long)blockIdx.x * kRecChunk;
        if (blockIdx.x == 0 && tid < hdr) {
            int v;
            if (tid < 4) v = "LLIC"[tid];
            else if (tid == 4) v = kRecVersion;
            else if (tid == 5) v = n;
            else v = ((uint32_t)seg_len[(long)b * LLICTI_NSEG + ((tid - 6) >> 2)] >> (8 * ((tid - 6) & 3))) & 0xFF;
            blob[o0 + tid] = (uint8_t)v;
        }
        if (c0 >= pay) continue;
        const uint8_t *src = cont + (long)b * stride;
        record_copy_chunk(blob + o0 + hdr + c0, src + c0, (int)min((long)kRecChunk, pay - c0), src, src + stride);
    }
}

// unpack, step 1: one wavefront per record.  EVERYTHING about a record is decided here, from rec_off and the record's own 6 + 4n header bytes,
// before a payload byte is read: 0 <= off[b] <= off[b+1] <= blob_bytes (nothing of the record is read unless this holds and the record has room
// for its header), length >= 6 + 4n, magic, version, n == the model's, every length below 2^31, 6 + 4n + sum == the record's length, sum <= stride.
// A good record: its n lengths and zeros up to 49 in seg_len[b], status 0.  A refused one: an all-zero row (which every decode call refuses in
// turn: header_read_kernel wants seg_len[0] == 3), LLICTI_EFORMAT, and record_unpack_kernel skips it.
__global__ __launch_bounds__(64) void record_check_kernel(const uint8_t *__restrict__ blob, long blob_bytes, const int64_t *__restrict__ rec_off,
                                                          int n, long stride, int32_t *__restrict__ seg_len, int32_t *latched,
                                                          int32_t *__restrict__ img_latched)
{
    const int b = (int)blockIdx.x, tid = (int)threadIdx.x, hdr = record_header_bytes(n);
    const long o0 = rec_off[b], o1 = rec_off[b + 1];
    bool ok = o0 >= 0 && o0 <= o1 && o1 <= blob_bytes && o1 - o0 >= hdr;       // (uniform: every lane reads the same words)
    uint32_t v = 0;
    if (ok) {
        const uint8_t *p = blob + o0;
        ok = p[0] == 'L' && p[1] == 'L' && p[2] == 'I' && p[3] == 'C' && p[4] == kRecVersion && p[5] == n;
        if (tid < n) {
            const uint8_t *q = p + 6 + 4 * tid;
            v = (uint32_t)q[0] | ((uint32_t)q[1] << 8) | ((uint32_t)q[2] << 16) | ((uint32_t)q[3] << 24);
        }
    }
    if (__any((int)(v >> 31))) ok = false;
    unsigned long long sum = v;
    for (int d = 32; d >= 1; d >>= 1) sum += __shfl_xor(sum, d, 64);
    ok = ok && (long)sum <= stride && hdr + (long)sum == o1 - o0;
    record_verdict(b, tid, n, ok, (int32_t)v, seg_len, latched, img_latched);
}

// unpack, step 2: grid (chunks, images); workgroup (x, b) copies chunk x of record b's payload to d_cont + b * stride.  The lengths are the ones
// record_check_kernel accepted (payload <= stride, the record inside the blob); a refused record's container is not touched.
__global__ __launch_bounds__(kRecThreads) void record_unpack_kernel(const uint8_t *__restrict__ blob, long blob_bytes, const int64_t *__restrict__ rec_off,
                                                                    int B, int n, uint8_t *__restrict__ cont, long stride,
                                                                    const int32_t *__restrict__ img_latched)
{
    const int hdr = record_header_bytes(n);
    for (int b = (int)blockIdx.y; b < B; b += (int)gridDim.y) {
        if (img_latched[b] != 0) continue;
        const long o0 = rec_off[b], pay = rec_off[b + 1] - o0 - hdr, c0 = (long)blockIdx.x * kRecChunk;
        if (c0 >= pay) continue;
        record_copy_chunk(cont + (long)b * stride + c0, blob + o0 + hdr + c0, (int)min((long)kRecChunk, pay - c0), blob, blob + blob_bytes);
    }
}

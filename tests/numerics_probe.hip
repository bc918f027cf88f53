// numerics_probe.hip -- the device side of the exhaustive sweep of the numerics spec's scalar functions.
// TEST INFRASTRUCTURE: a stand-alone program that includes the product's header itself (not a copy) and is built with the library's
// own flags (llicti_amd/_lib.py: build_probe).  tests/test_hip_numerics.py runs it once and holds what it prints against
// tests/golden/numerics_sums.npz (the CPU oracle's side: tests/numerics_sums_host.c, which also says what a chunk, S1 and S2 are).
//
//   numerics_probe --out FILE        sweeps, one JSON object on stdout; FILE gets S1[4096] then S2[4096] of erfc_spec (uint64)
//   numerics_probe --dump C FILE     erfc_spec's 2^20 output words over chunk C (uint32) to FILE, nothing else
//
// One workgroup per chunk; erfc_spec and erfc_spec_nobranch are called through separate non-inlined functions, so that the compiler
// cannot merge the two bodies it is asked to compare.
#include "../llicti_amd/csrc/numerics.hpp"

#include <chrono>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

#define HIP_CHECK(e)                                                                                          \
    do {                                                                                                      \
        hipError_t err_ = (e);                                                                                \
        if (err_ != hipSuccess) {                                                                             \
            fprintf(stderr, "%s:%d: %s: %s\n", __FILE__, __LINE__, #e, hipGetErrorString(err_));              \
            exit(1);                                                                                          \
        }                                                                                                     \
    } while (0)

constexpr int kChunkBits = 20;
constexpr uint32_t kChunk = 1u << kChunkBits;
constexpr int kChunks = 4096;
constexpr int kThreads = 256;
constexpr uint32_t kRecipLo = 0x40000000u, kRecipHi = 0x41100000u;      // 2.0f, 9.0f
constexpr int kRecipChunk0 = (int)(kRecipLo >> kChunkBits);
constexpr int kRecipChunks = (int)(kRecipHi >> kChunkBits) - kRecipChunk0 + 1;
constexpr uint32_t kNone = 0xFFFFFFFFu;

struct ChunkOut { uint64_t s1, s2; uint32_t bad, first; };       // first: the smallest k of the chunk whose two results differ

__device__ __noinline__ float call_erfc_spec(float x) { return llicti::erfc_spec(x); }
__device__ __noinline__ float call_erfc_nobranch(float x) { return llicti::erfc_spec_nobranch(x); }

__device__ __forceinline__ void reduce_chunk(uint64_t s1, uint64_t s2, uint32_t bad, uint32_t first, ChunkOut *out)
{
    __shared__ uint64_t l1[kThreads], l2[kThreads];
    __shared__ uint32_t lb[kThreads], lf[kThreads];
    const int t = threadIdx.x;
    l1[t] = s1; l2[t] = s2; lb[t] = bad; lf[t] = first;
    __syncthreads();
    for (int d = kThreads / 2; d > 0; d >>= 1) {
        if (t < d) {
            l1[t] += l1[t + d]; l2[t] += l2[t + d]; lb[t] += lb[t + d];
            lf[t] = min(lf[t], lf[t + d]);
        }
        __syncthreads();
    }
    if (t == 0) *out = ChunkOut{ l1[0], l2[0], lb[0], lf[0] };
}

// chunk = chunk0 + blockIdx.x; sums of erfc_spec, mismatches against erfc_spec_nobranch
__global__ __launch_bounds__(kThreads) void erfc_sweep(int chunk0, ChunkOut *__restrict__ out)
{
    const uint32_t base = (uint32_t)(chunk0 + blockIdx.x) << kChunkBits;
    uint64_t s1 = 0, s2 = 0;
    uint32_t bad = 0, first = kNone;
    for (uint32_t k = threadIdx.x; k < kChunk; k += kThreads) {
        const float x = __uint_as_float(base + k);
        const uint32_t a = __float_as_uint(call_erfc_spec(x)), b = __float_as_uint(call_erfc_nobranch(x));
        s1 += a;
        s2 += (uint64_t)(2 * k + 1) * a;
        if (a != b) { ++bad; first = min(first, k); }
    }
    reduce_chunk(s1, s2, bad, first, out + blockIdx.x);
}

// sums of 1.0f / d over the floats of [2, 9] in chunk kRecipChunk0 + blockIdx.x, mismatches of recip_2_9 against it
__global__ __launch_bounds__(kThreads) void recip_sweep(ChunkOut *__restrict__ out)
{
    const uint32_t base = (uint32_t)(kRecipChunk0 + blockIdx.x) << kChunkBits;
    uint64_t s1 = 0, s2 = 0;
    uint32_t bad = 0, first = kNone;
    for (uint32_t k = threadIdx.x; k < kChunk; k += kThreads) {
        const uint32_t u = base + k;
        if (u < kRecipLo || u > kRecipHi) continue;
        const float d = __uint_as_float(u);
        const uint32_t a = __float_as_uint(1.0f / d), b = __float_as_uint(llicti::recip_2_9(d));
        s1 += a;
        s2 += (uint64_t)(2 * k + 1) * a;
        if (a != b) { ++bad; first = min(first, k); }
    }
    reduce_chunk(s1, s2, bad, first, out + blockIdx.x);
}

__global__ void div255_probe(const float *__restrict__ x, int n, uint32_t *__restrict__ exact, uint32_t *__restrict__ div)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    exact[i] = __float_as_uint(llicti::div255_exact(x[i]));
    div[i] = __float_as_uint(x[i] / 255.0f);
}

__global__ __launch_bounds__(kThreads) void erfc_dump(int chunk, uint32_t *__restrict__ words)
{
    const uint32_t k = blockIdx.x * kThreads + threadIdx.x;          // grid: kChunk / kThreads workgroups
    if (k < kChunk) words[k] = __float_as_uint(call_erfc_spec(__uint_as_float(((uint32_t)chunk << kChunkBits) + k)));
}

static int write_file(const char *path, const void *p, size_t bytes)
{
    FILE *f = fopen(path, "wb");
    if (!f || fwrite(p, 1, bytes, f) != bytes || fclose(f)) { perror(path); return 1; }
    return 0;
}

static void print_u32s(const char *name, const std::vector<uint32_t> &v)
{
    printf("\"%s\": [", name);
    for (size_t i = 0; i < v.size(); ++i) printf("%s%u", i ? ", " : "", v[i]);
    printf("]");
}

int main(int argc, char **argv)
{
    const char *out_path = nullptr, *dump_path = nullptr;
    int dump_chunk = -1;
    for (int a = 1; a < argc; ++a) {
        if (!strcmp(argv[a], "--out") && a + 1 < argc) out_path = argv[++a];
        else if (!strcmp(argv[a], "--dump") && a + 2 < argc) { dump_chunk = atoi(argv[a + 1]); dump_path = argv[a + 2]; a += 2; }
        else { fprintf(stderr, "usage: %s --out FILE | --dump C FILE\n", argv[0]); return 2; }
    }
    if ((!out_path && !dump_path) || (dump_path && (dump_chunk < 0 || dump_chunk >= kChunks))) {
        fprintf(stderr, "usage: %s --out FILE | --dump C FILE   (C in 0 .. %d)\n", argv[0], kChunks - 1);
        return 2;
    }
    int ndev = 0;
    HIP_CHECK(hipGetDeviceCount(&ndev));
    if (ndev < 1) { fprintf(stderr, "no HIP device\n"); return 1; }

    if (dump_path) {
        uint32_t *d_words;
        std::vector<uint32_t> words(kChunk);
        HIP_CHECK(hipMalloc(&d_words, sizeof(uint32_t) * kChunk));
        erfc_dump<<<kChunk / kThreads, kThreads>>>(dump_chunk, d_words);
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipMemcpy(words.data(), d_words, sizeof(uint32_t) * kChunk, hipMemcpyDeviceToHost));
        HIP_CHECK(hipFree(d_words));
        return write_file(dump_path, words.data(), sizeof(uint32_t) * kChunk);
    }

    const auto t0 = std::chrono::steady_clock::now();
    ChunkOut *d_out;
    HIP_CHECK(hipMalloc(&d_out, sizeof(ChunkOut) * (kChunks + kRecipChunks)));
    HIP_CHECK(hipDeviceSynchronize());
    const auto t1 = std::chrono::steady_clock::now();
    erfc_sweep<<<kChunks, kThreads>>>(0, d_out);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipDeviceSynchronize());
    const auto t2 = std::chrono::steady_clock::now();
    recip_sweep<<<kRecipChunks, kThreads>>>(d_out + kChunks);
    HIP_CHECK(hipGetLastError());
    std::vector<ChunkOut> res(kChunks + kRecipChunks);
    HIP_CHECK(hipMemcpy(res.data(), d_out, sizeof(ChunkOut) * res.size(), hipMemcpyDeviceToHost));
    HIP_CHECK(hipFree(d_out));

    // every half-integer |x| <= 350 (every regular sample point of any table), then every integer |v| <= 255 (every plane value)
    std::vector<float> x;
    for (int k = -700; k <= 700; ++k) x.push_back(0.5f * (float)k);
    for (int v = -255; v <= 255; ++v) x.push_back((float)v);
    const int n = (int)x.size();
    float *d_x;
    uint32_t *d_w;
    HIP_CHECK(hipMalloc(&d_x, sizeof(float) * n));
    HIP_CHECK(hipMalloc(&d_w, sizeof(uint32_t) * 2 * n));
    HIP_CHECK(hipMemcpy(d_x, x.data(), sizeof(float) * n, hipMemcpyHostToDevice));
    div255_probe<<<(n + kThreads - 1) / kThreads, kThreads>>>(d_x, n, d_w, d_w + n);
    HIP_CHECK(hipGetLastError());
    std::vector<uint32_t> xb(n), ex(n), dv(n);
    HIP_CHECK(hipMemcpy(ex.data(), d_w, sizeof(uint32_t) * n, hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(dv.data(), d_w + n, sizeof(uint32_t) * n, hipMemcpyDeviceToHost));
    HIP_CHECK(hipFree(d_x));
    HIP_CHECK(hipFree(d_w));
    memcpy(xb.data(), x.data(), sizeof(float) * n);
    const auto t3 = std::chrono::steady_clock::now();

    std::vector<uint64_t> sums(2 * kChunks);
    unsigned long long nb_bad = 0, rc_bad = 0;
    uint32_t nb_first = 0, rc_first = 0;
    bool nb_seen = false, rc_seen = false;
    for (int c = 0; c < kChunks; ++c) {
        sums[c] = res[c].s1;
        sums[kChunks + c] = res[c].s2;
        nb_bad += res[c].bad;
        if (res[c].bad && !nb_seen) { nb_seen = true; nb_first = ((uint32_t)c << kChunkBits) + res[c].first; }
    }
    if (write_file(out_path, sums.data(), sizeof(uint64_t) * sums.size())) return 1;
    for (int c = 0; c < kRecipChunks; ++c) {
        const ChunkOut &r = res[kChunks + c];
        rc_bad += r.bad;
        if (r.bad && !rc_seen) { rc_seen = true; rc_first = ((uint32_t)(kRecipChunk0 + c) << kChunkBits) + r.first; }
    }
    auto ms = [](auto a, auto b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
    printf("{\"chunks\": %d, \"chunk_bits\": %d, \"sums_file\": \"%s\", ", kChunks, kChunkBits, out_path);
    printf("\"nobranch_mismatches\": %llu, \"nobranch_first\": %s%u, ", nb_bad, "", nb_seen ? nb_first : 0u);
    printf("\"nobranch_first_valid\": %s, ", nb_seen ? "true" : "false");
    printf("\"recip_checked\": %u, \"recip_mismatches\": %llu, \"recip_first\": %u, \"recip_first_valid\": %s, ", kRecipHi - kRecipLo + 1, rc_bad,
           rc_seen ? rc_first : 0u, rc_seen ? "true" : "false");
    printf("\"recip_chunk0\": %d, \"recip_s1\": [", kRecipChunk0);
    for (int c = 0; c < kRecipChunks; ++c) printf("%s\"%016llx\"", c ? ", " : "", (unsigned long long)res[kChunks + c].s1);
    printf("], \"recip_s2\": [");
    for (int c = 0; c < kRecipChunks; ++c) printf("%s\"%016llx\"", c ? ", " : "", (unsigned long long)res[kChunks + c].s2);
    printf("], ");
    print_u32s("div255_x", xb);
    printf(", ");
    print_u32s("div255_exact", ex);
    printf(", ");
    print_u32s("div255_div", dv);
    printf(", \"erfc_sweep_ms\": %.3f, \"wall_ms\": %.3f}\n", ms(t1, t2), ms(t0, t3));
    return 0;
}

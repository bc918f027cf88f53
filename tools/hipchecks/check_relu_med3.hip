// The band CNN's one-instruction ReLU (band_cnn.hpp: relu4) against its definition, relu(x) = x > 0 ? x : +0, bit for bit (run on the GPU box).
// v_med3_f32(x, 0, +inf) with the +inf opaque to the compiler.  Values: both zeros, denormals, the normal range's ends, both infinities, quiet
// NaNs of both signs, MFMA results (an accumulator is what the kernel applies it to) and 2^20 random bit patterns that are no signalling NaN
// (an MFMA never returns one; the two forms differ there: reported, not counted).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <vector>
typedef float f32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ float relu_med3(float x)
{
    int inf_bits = 0x7f800000;
    asm volatile("" : "+s"(inf_bits));
    return __builtin_amdgcn_fmed3f(x, 0.0f, __int_as_float(inf_bits));
}
__global__ void k(const float *x, float *y, float *ym, int n)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;                                   // (n is a multiple of 64: whole wavefronts)
    y[i] = relu_med3(x[i]);
    // the same value as an MFMA result: D = 1 * 0 + C leaves C as it is, except that -0 + +0 is +0
    f32x4 acc = { x[i], x[i], x[i], x[i] };
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(1.0f, 0.0f, acc, 0, 0, 0);
    ym[i] = relu_med3(acc[i & 3]);
}
static uint32_t bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
static float fl(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }
int main()
{
    std::vector<float> h;
    const uint32_t special[] = { 0x00000000u, 0x80000000u, 0x00000001u, 0x80000001u, 0x007fffffu, 0x807fffffu, 0x00800000u, 0x80800000u, 0x3f800000u,
                                 0xbf800000u, 0x7f7fffffu, 0xff7fffffu, 0x7f800000u, 0xff800000u, 0x7fc00000u, 0xffc00000u, 0x7fc12345u, 0xffc12345u,
                                 0x7fffffffu, 0xffffffffu };
    for (uint32_t s : special) h.push_back(fl(s));
    uint64_t r = 0x9E3779B97F4A7C15ull;
    while (h.size() < (1u << 20)) {
        r = r * 6364136223846793005ull + 1442695040888963407ull;
        const uint32_t u = (uint32_t)(r >> 32);
        if ((u & 0x7f800000u) == 0x7f800000u && (u & 0x007fffffu) && !(u & 0x00400000u)) continue;      // signalling NaN
        h.push_back(fl(u));
    }
    const int n = (int)h.size();
    float *x, *y, *ym;
    hipMalloc(&x, n * 4); hipMalloc(&y, n * 4); hipMalloc(&ym, n * 4);
    hipMemcpy(x, h.data(), n * 4, hipMemcpyHostToDevice);
    k<<<n / 256, 256>>>(x, y, ym, n);
    std::vector<float> hy(n), hm(n);
    hipMemcpy(hy.data(), y, n * 4, hipMemcpyDeviceToHost);
    hipMemcpy(hm.data(), ym, n * 4, hipMemcpyDeviceToHost);
    int bad = 0;
    for (int i = 0; i < n; ++i) {
        const float want = (h[i] > 0.0f) ? h[i] : 0.0f;
        if (bits(hy[i]) != bits(want) || bits(hm[i]) != bits(want)) {
            if (bad < 8) printf("x %08x: want %08x, med3 %08x, med3 of the MFMA result %08x\n", bits(h[i]), bits(want), bits(hy[i]), bits(hm[i]));
            ++bad;
        }
    }
    float hs[64], *xs = x, *ys = y;
    for (int i = 0; i < 64; ++i) hs[i] = fl(i & 1 ? 0xffa00000u : 0x7fa00000u);
    hipMemcpy(xs, hs, 256, hipMemcpyHostToDevice);
    k<<<1, 64>>>(xs, ys, ym, 64);
    hipMemcpy(hs, ys, 8, hipMemcpyDeviceToHost);
    printf("(signalling NaNs 7fa00000 / ffa00000 -> %08x / %08x; the select gives 00000000)\n", bits(hs[0]), bits(hs[1]));
    printf("relu as v_med3_f32(x, 0, +inf): %d mismatches against x > 0 ? x : +0 over %d values\n", bad, n);
    return bad != 0;
}

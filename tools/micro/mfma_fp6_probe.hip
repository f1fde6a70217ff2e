// What v_mfma_scale_f32_32x32x64_f8f6f4 / _16x16x128_ with FP6 (e2m3) operands gives the int4 halo convolution:
//   1. the A / B lane map and the 6-bit packing (exact integer data, asymmetric B): lane l of 32x32x64 supplies row (col)
//      l & 31 and k = 32 (l >> 5) + e in field e (bits 6e .. 6e + 5 of its six registers); 16x16x128: row l & 15,
//      k = 32 (l >> 4) + e.  Prints the mismatches against that assumed map;
//   2. exactness of the int4 codes as e2m3 (activation u = c + 8 in [0, 15] = u / 8, weight w in [-8, 7] = sign-magnitude
//      w / 8, both E8M0 scales 2^3, so every product is the integer u w): 9 chained instructions = 576 taps, random codes
//      and the extreme sums (u = 15 against w = -8 / 7), C seeded at 0 and at 1.5 * 2^23 (the fold's magic constant);
//   3. cycles per instruction back to back (4 independent accumulators, one wave per SIMD, every CU busy) for FP6 x FP6,
//      FP8 (e4m3) x FP6 and v_mfma_i32_32x32x32_i8, with the clock held (s_memtime ticks / s_memrealtime at 100 MHz).
//   hipcc --offload-arch=gfx950 -O3 tools/micro/mfma_fp6_probe.hip -o /tmp/mfma_fp6_probe && /tmp/mfma_fp6_probe
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <math.h>
typedef int v4i __attribute__((ext_vector_type(4)));
typedef int v8i __attribute__((ext_vector_type(8)));
typedef int v16i __attribute__((ext_vector_type(16)));
typedef float v4f __attribute__((ext_vector_type(4)));
typedef float v16f __attribute__((ext_vector_type(16)));

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP error %s at %d\n", hipGetErrorString(e_), __LINE__); exit(1); } } while (0)

static uint32_t e2m3_act(int u) { return (uint32_t)u; }                                        // u in [0, 15] -> u / 8
static uint32_t e2m3_w(int w) { return w < 0 ? (0x20u | (uint32_t)(-w)) : (uint32_t)w; }      // w in [-8, 7] -> w / 8

// 32 six-bit fields -> 6 dwords (field e at bits 6e .. 6e + 5)
static void pack32(const uint32_t* f, uint32_t* out) {
    for (int i = 0; i < 8; ++i) out[i] = 0;
    for (int e = 0; e < 32; ++e)
        for (int b = 0; b < 6; ++b)
            if ((f[e] >> b) & 1) out[(6 * e + b) >> 5] |= 1u << ((6 * e + b) & 31);
}

// BIG: 32x32x64 (else 16x16x128); `steps` chained instructions with operand set s, C seeded with `seed`
template <bool BIG>
__global__ void k_map(const v8i* a, const v8i* b, float seed, int steps, float* c) {
    const int l = threadIdx.x;
    if constexpr (BIG) {
        v16f acc;
        for (int j = 0; j < 16; ++j) acc[j] = seed;
        for (int s = 0; s < steps; ++s)
            acc = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a[s * 64 + l], b[s * 64 + l], acc, 2, 2, 0, 130, 0, 130);
        for (int j = 0; j < 16; ++j) c[l * 16 + j] = acc[j];
    } else {
        v4f acc;
        for (int j = 0; j < 4; ++j) acc[j] = seed;
        for (int s = 0; s < steps; ++s)
            acc = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a[s * 64 + l], b[s * 64 + l], acc, 2, 2, 0, 130, 0, 130);
        for (int j = 0; j < 4; ++j) c[l * 4 + j] = acc[j];
    }
}

// A[row][k] (u), B[k][col] (w) over `steps` K-blocks -> lane images, device run, compare with the exact integer sum
template <bool BIG>
static long run_map(const int* A, const int* B, int steps, float seed, double* maxabs) {
    const int M = BIG ? 32 : 16, K = BIG ? 64 : 128, G = BIG ? 32 : 16;        // G: lanes per k-group
    const int KT = K * steps;
    v8i *ha = (v8i*)calloc(64 * steps, sizeof(v8i)), *hb = (v8i*)calloc(64 * steps, sizeof(v8i));
    for (int s = 0; s < steps; ++s)
        for (int l = 0; l < 64; ++l) {
            uint32_t fa[32], fb[32], pa[8], pb[8];
            const int r = l % G, kg = l / G;
            for (int e = 0; e < 32; ++e) {
                const int k = s * K + 32 * kg + e;
                fa[e] = e2m3_act(A[r * KT + k]);
                fb[e] = e2m3_w(B[k * M + r]);
            }
            pack32(fa, pa); pack32(fb, pb);
            for (int i = 0; i < 8; ++i) { ha[s * 64 + l][i] = (int)pa[i]; hb[s * 64 + l][i] = (int)pb[i]; }
        }
    v8i *da, *db; float* dc;
    CK(hipMalloc(&da, 64 * steps * sizeof(v8i))); CK(hipMalloc(&db, 64 * steps * sizeof(v8i))); CK(hipMalloc(&dc, 64 * 16 * 4));
    CK(hipMemcpy(da, ha, 64 * steps * sizeof(v8i), hipMemcpyHostToDevice));
    CK(hipMemcpy(db, hb, 64 * steps * sizeof(v8i), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_map<BIG>, dim3(1), dim3(64), 0, 0, da, db, seed, steps, dc);
    CK(hipDeviceSynchronize());
    float hc[64 * 16];
    CK(hipMemcpy(hc, dc, sizeof(hc), hipMemcpyDeviceToHost));
    long bad = 0;
    *maxabs = 0;
    for (int l = 0; l < 64; ++l)
        for (int j = 0; j < (BIG ? 16 : 4); ++j) {
            // C/D: 32x32: col l & 31, row (j & 3) + 8 (j >> 2) + 4 (l >> 5); 16x16: col l & 15, row 4 (l >> 4) + j
            const int col = l % M, row = BIG ? (j & 3) + 8 * (j >> 2) + 4 * (l >> 5) : 4 * (l >> 4) + j;
            long ref = 0;
            for (int k = 0; k < KT; ++k) ref += (long)A[row * KT + k] * B[k * M + col];
            const double want = (double)seed + (double)ref;
            const double got = hc[l * (BIG ? 16 : 4) + j];
            if (got != (double)(float)want) ++bad;
            if (fabs((double)ref) > *maxabs) *maxabs = fabs((double)ref);
        }
    CK(hipFree(da)); CK(hipFree(db)); CK(hipFree(dc));
    free(ha); free(hb);
    return bad;
}

template <bool BIG>
static void map_suite() {
    const int M = BIG ? 32 : 16, K = BIG ? 64 : 128, steps = BIG ? 9 : 5;    // 576 / 640 taps
    const int KT = K * steps;
    int* A = (int*)malloc(sizeof(int) * M * KT);
    int* B = (int*)malloc(sizeof(int) * KT * M);
    const char* nm = BIG ? "32x32x64" : "16x16x128";
    const float seeds[2] = {0.0f, 12582912.0f};
    for (int si = 0; si < 2; ++si) {
        double mx;
        // single K-block, asymmetric data: the lane map
        for (int r = 0; r < M; ++r) for (int k = 0; k < KT; ++k) A[r * KT + k] = (r * 7 + k * 3 + (k >> 4)) & 15;
        for (int k = 0; k < KT; ++k) for (int c = 0; c < M; ++c) B[k * M + c] = ((k * 5 + c * 11 + (c >> 2)) & 15) - 8;
        long bad = run_map<BIG>(A, B, 1, seeds[si], &mx);
        printf("%-10s seed %-9.0f map (one instruction, asymmetric)         : %ld / %d wrong\n", nm, seeds[si], bad, M * M);
        // every (u, w) pair on a diagonal sweep, chained over all taps
        for (int r = 0; r < M; ++r) for (int k = 0; k < KT; ++k) A[r * KT + k] = (k + r) & 15;
        for (int k = 0; k < KT; ++k) for (int c = 0; c < M; ++c) B[k * M + c] = ((k >> 4) + 3 * c) % 16 - 8;
        bad = run_map<BIG>(A, B, steps, seeds[si], &mx);
        printf("%-10s seed %-9.0f all 16x16 (u, w) pairs, %d taps              : %ld wrong, max |sum| %.0f\n", nm, seeds[si], KT, bad, mx);
        srand(12345 + si);
        for (int i = 0; i < M * KT; ++i) { A[i] = rand() & 15; B[i] = (rand() & 15) - 8; }
        bad = run_map<BIG>(A, B, steps, seeds[si], &mx);
        printf("%-10s seed %-9.0f random codes, %d taps                      : %ld wrong, max |sum| %.0f\n", nm, seeds[si], KT, bad, mx);
        for (int wv = 0; wv < 2; ++wv) {
            for (int i = 0; i < M * KT; ++i) { A[i] = 15; B[i] = wv ? 7 : -8; }
            bad = run_map<BIG>(A, B, steps, seeds[si], &mx);
            printf("%-10s seed %-9.0f extreme u = 15, w = %2d, %d taps            : %ld wrong, |sum| %.0f\n", nm, seeds[si],
                   wv ? 7 : -8, KT, bad, mx);
        }
    }
    free(A); free(B);
}

// ---- rate: 4 independent accumulators, operands in registers ----
template <int MODE>   // 0 FP6 x FP6, 1 FP8 x FP6, 2 i8
__global__ __launch_bounds__(256, 1) void k_rate(const uint32_t* rnd, int iters, float* out, unsigned long long* st) {
    const int l = threadIdx.x & 63;
    v8i a, b;
    for (int i = 0; i < 8; ++i) { a[i] = (int)rnd[(l * 8 + i) & 1023]; b[i] = (int)rnd[(l * 8 + i + 512) & 1023]; }
    if (MODE == 0) for (int i = 0; i < 8; ++i) { a[i] &= 0x3DF7DF7D; b[i] &= 0x3DF7DF7D; }     // finite, small e2m3 codes
    const unsigned long long t0 = __builtin_amdgcn_s_memtime(), r0 = __builtin_amdgcn_s_memrealtime();
    float sum = 0.0f;
    if constexpr (MODE == 2) {
        const v4i a4 = {a[0], a[1], a[2], a[3]}, b4 = {b[0], b[1], b[2], b[3]};
        v16i acc[4] = {};
        for (int it = 0; it < iters; ++it)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[j] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a4, b4, acc[j], 0, 0, 0);
        for (int j = 0; j < 4; ++j) sum += (float)acc[j][0];
    } else {
        v16f acc[4] = {};
        for (int it = 0; it < iters; ++it)
#pragma unroll
            for (int j = 0; j < 4; ++j)
                acc[j] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a, b, acc[j], MODE == 0 ? 2 : 0, 2, 0, 127, 0, 127);
        for (int j = 0; j < 4; ++j) sum += acc[j][0];
    }
    const unsigned long long t1 = __builtin_amdgcn_s_memtime(), r1 = __builtin_amdgcn_s_memrealtime();
    out[blockIdx.x * 256 + threadIdx.x] = sum;
    if (threadIdx.x == 0) { st[blockIdx.x * 2] = t1 - t0; st[blockIdx.x * 2 + 1] = r1 - r0; }
}

template <int MODE>
static void rate(const char* nm, const uint32_t* drnd, int ncu) {
    const int iters = 20000;
    float* dout; unsigned long long* dst;
    CK(hipMalloc(&dout, (size_t)ncu * 256 * 4)); CK(hipMalloc(&dst, (size_t)ncu * 16));
    hipLaunchKernelGGL(k_rate<MODE>, dim3(ncu), dim3(256), 0, 0, drnd, 100, dout, dst);     // warm-up
    CK(hipDeviceSynchronize());
    hipLaunchKernelGGL(k_rate<MODE>, dim3(ncu), dim3(256), 0, 0, drnd, iters, dout, dst);
    CK(hipDeviceSynchronize());
    unsigned long long* h = (unsigned long long*)malloc((size_t)ncu * 16);
    CK(hipMemcpy(h, dst, (size_t)ncu * 16, hipMemcpyDeviceToHost));
    double cyc = 0, ns = 0;
    for (int i = 0; i < ncu; ++i) { cyc += (double)h[2 * i]; ns += (double)h[2 * i + 1] * 10.0; }
    cyc /= ncu; ns /= ncu;
    const double n = 4.0 * iters;
    printf("%-22s %.2f cycles per instruction, %.2f ns (clock held %.2f GHz)\n", nm, cyc / n, ns / n, cyc / ns);
    free(h); CK(hipFree(dout)); CK(hipFree(dst));
}

int main() {
    int ncu = 0;
    CK(hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, 0));
    map_suite<true>();
    map_suite<false>();
    uint32_t hr[1024];
    srand(7);
    for (int i = 0; i < 1024; ++i) hr[i] = ((uint32_t)rand() << 16) ^ (uint32_t)rand();
    uint32_t* dr;
    CK(hipMalloc(&dr, sizeof(hr)));
    CK(hipMemcpy(dr, hr, sizeof(hr), hipMemcpyHostToDevice));
    rate<0>("fp6 x fp6 32x32x64", dr, ncu);
    rate<1>("fp8 x fp6 32x32x64", dr, ncu);
    rate<2>("i8 32x32x32", dr, ncu);
    CK(hipFree(dr));
    return 0;
}

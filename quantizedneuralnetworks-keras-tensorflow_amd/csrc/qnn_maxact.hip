// quantized_maxrelu / quantized_leakymaxrelu (layers/quantized_ops.py:125-171; include/qnn_abi_maxact.h): the quantised
// activations whose scale is the smallest power of two >= the maximum of the whole batch tensor.
//
// Two HBM-bound passes over the tensor, as ternary_tanh has them (qnn_elementwise.hip): the maximum into a device word
// (4 bytes per value read), then the clip with the scales derived from that word (8 bytes per value).  Between the two a
// batch sharded over processes all-reduces the word.  Nothing is read back to the host.
#include "qnn_common.h"

namespace {

constexpr int kBlock = 256;
constexpr int kMaxBlocks = 1 << 22;      // of the apply pass: one 16-byte item per thread, as k_act_f32
constexpr int kReduceBlocks = 1024;      // of the reduction: one atomic per block, so at most 1024 per call (as k_tern_sum)
constexpr int kReduceUnroll = 4;         // independent 16-byte loads in flight per lane: 1024 blocks alone leave HBM idle

typedef float v4f __attribute__((ext_vector_type(4)));

inline int blocks_for(size_t items, int cap) {
    size_t b = (items + kBlock - 1) / kBlock;
    if (b < 1) b = 1;
    if (b > (size_t)cap) b = cap;
    return (int)b;
}

// Pass 1: M = max over the tensor of max(x, 0).  Non-negative floats order like their bit patterns, so the blocks merge
// with one unsigned atomicMax each on a word that starts at 0 = +0.0f.  fmaxf drops a NaN operand; a -0 that fmaxf may
// hand back for max(+0, -0) has its sign cleared before the atomic (as an unsigned it would beat every real maximum).
__global__ __launch_bounds__(kBlock) void k_maxact_reduce(const float* __restrict__ x, size_t n, uint32_t* __restrict__ word) {
    constexpr int U = kReduceUnroll;
    const size_t n4 = n / 4;
    const v4f* x4 = reinterpret_cast<const v4f*>(x);
    const size_t stride = (size_t)gridDim.x * kBlock;
    size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x;
    float mx = 0.0f;
    auto take = [&](v4f v) { mx = fmaxf(fmaxf(fmaxf(mx, v.x), fmaxf(v.y, v.z)), v.w); };
    for (; i + (U - 1) * stride < n4; i += U * stride) {
        v4f v[U];
#pragma unroll
        for (int u = 0; u < U; ++u) v[u] = __builtin_nontemporal_load(&x4[i + u * stride]);
#pragma unroll
        for (int u = 0; u < U; ++u) take(v[u]);
    }
    for (; i < n4; i += stride) take(__builtin_nontemporal_load(&x4[i]));
    // tail (n % 4 elements)
    const size_t t = n4 * 4 + (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (t < n) mx = fmaxf(mx, x[t]);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) mx = fmaxf(mx, __shfl_down(mx, off, 64));
    __shared__ float part[kBlock / 64];
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = mx;
    __syncthreads();
    if (threadIdx.x == 0) {
        float b = part[0];
#pragma unroll
        for (int w = 1; w < kBlock / 64; ++w) b = fmaxf(b, part[w]);
        atomicMax(word, __float_as_uint(b) & 0x7FFFFFFFu);
    }
}

// Pass 2: every block reads the word and derives the scales itself (integer exponent arithmetic, qnn_common.h), then
// streams like k_act_f32.  A word outside the exact range (0 = no positive value) turns every output into quiet NaN.
template <int FN>
__global__ __launch_bounds__(kBlock) void k_maxact_apply(const float* __restrict__ x, float* __restrict__ y, size_t n, int nb,
                                                         const uint32_t* __restrict__ word) {
    float s_in = 0.0f, s_out = 0.0f;
    const bool ok = qnn_maxact_scales(*word, nb, &s_in, &s_out);
    const float m = __uint_as_float((uint32_t)(127 + nb - 1) << 23);
    const float qnan = __uint_as_float(0x7FC00000u);
    auto f1 = [&](float v) { return ok ? qnn_maxact(FN, v, m, s_in, s_out) : qnan; };
    const size_t n4 = n / 4;
    const v4f* x4 = reinterpret_cast<const v4f*>(x);
    v4f* y4 = reinterpret_cast<v4f*>(y);
    const size_t stride = (size_t)gridDim.x * kBlock;
    for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < n4; i += stride) {
        const v4f v = __builtin_nontemporal_load(&x4[i]);
        __builtin_nontemporal_store((v4f){f1(v.x), f1(v.y), f1(v.z), f1(v.w)}, &y4[i]);
    }
    // tail (n % 4 elements)
    const size_t t = n4 * 4 + (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (t < n) y[t] = f1(x[t]);
}

}  // namespace

extern "C" int qnn_maxact_max_f32(const float* x, size_t n, void* workspace16, void* stream) {
    QNN_REQUIRE(workspace16 && (x || n == 0), QNN_EINVAL, "qnn_maxact_max_f32: null pointer");
    hipStream_t s = (hipStream_t)stream;
    // a memset node, not a copy from host memory: this call is captured into hipGraphs
    QNN_HIP(hipMemsetAsync(workspace16, 0, 16, s));
    if (n == 0) return QNN_OK;
    hipLaunchKernelGGL(k_maxact_reduce, dim3(blocks_for(n / 4, kReduceBlocks)), dim3(kBlock), 0, s, x, n,
                       (uint32_t*)workspace16);
    QNN_HIP(hipGetLastError());
    return QNN_OK;
}

extern "C" int qnn_maxact_apply_f32(const float* x, float* y, size_t n, int fn, int nb, const void* workspace16,
                                    void* stream) {
    QNN_REQUIRE(qnn_is_maxact(fn), QNN_EINVAL,
                "qnn_maxact_apply_f32: fn=%d is neither QNN_FN_QUANTIZED_MAXRELU nor QNN_FN_QUANTIZED_LEAKYMAXRELU", fn);
    QNN_REQUIRE(nb >= 2 && nb <= 24, QNN_EINVAL, "qnn_maxact_apply_f32: nb=%d out of range (2 .. 24)", nb);
    if (n == 0) return QNN_OK;
    QNN_REQUIRE(x && y && workspace16, QNN_EINVAL, "qnn_maxact_apply_f32: null pointer");
    const dim3 grid(blocks_for((n + 3) / 4, kMaxBlocks)), block(kBlock);
    if (fn == QNN_FN_QUANTIZED_MAXRELU)
        hipLaunchKernelGGL(k_maxact_apply<QNN_FN_QUANTIZED_MAXRELU>, grid, block, 0, (hipStream_t)stream, x, y, n, nb,
                           (const uint32_t*)workspace16);
    else
        hipLaunchKernelGGL(k_maxact_apply<QNN_FN_QUANTIZED_LEAKYMAXRELU>, grid, block, 0, (hipStream_t)stream, x, y, n, nb,
                           (const uint32_t*)workspace16);
    QNN_HIP(hipGetLastError());
    return QNN_OK;
}

extern "C" int qnn_quantized_maxact_f32(const float* x, float* y, size_t n, int fn, int nb, void* workspace16, void* stream) {
    QNN_REQUIRE(qnn_is_maxact(fn), QNN_EINVAL,
                "qnn_quantized_maxact_f32: fn=%d is neither QNN_FN_QUANTIZED_MAXRELU nor QNN_FN_QUANTIZED_LEAKYMAXRELU", fn);
    QNN_REQUIRE(nb >= 2 && nb <= 24, QNN_EINVAL, "qnn_quantized_maxact_f32: nb=%d out of range (2 .. 24)", nb);
    if (n == 0) return QNN_OK;
    QNN_REQUIRE(x && y && workspace16, QNN_EINVAL, "qnn_quantized_maxact_f32: null pointer");
    const int rc = qnn_maxact_max_f32(x, n, workspace16, stream);
    if (rc != QNN_OK) return rc;
    return qnn_maxact_apply_f32(x, y, n, fn, nb, workspace16, stream);
}

// Float32-activation convolution on v_mfma_f32_16x16x4_f32: the 3x3 (stride 1 / 2) and 1x1 stride-2 layers with 16, 32
// or 64 input channels of the networks whose activations stay float32 (LeakyReLU families of models/model_factory.py:
// bnn, tnn, qnn, float), and the Keras layers on such inputs.  Dispatch: qnn_conv2d_forward (qnn_conv.hip), after the
// other float-input routes and before k_conv_generic.
//
// Same arithmetic as k_conv_generic: per output value one float32 FMA chain over k = (dy, dx, c) in ascending order.
// The f32-input MFMA computes exactly that chain (one rounding per product, accumulator carried between K-steps).  No
// split-K, no reordering within a tap.  Out-of-image taps enter as zeros where k_conv_generic skips them, and
// fma(w, 0, acc) = acc except in two cases, where the two kernels may differ in border pixels:
//   - a non-finite weight (Inf * 0 = NaN).  No quantizer produces one; only a float ("Conv2D") kernel can hold it.
//   - acc = -0.  acc starts at +0, and an exact cancellation rounds to +0, so this needs a partial sum that underflows
//     from below to -0 (magnitude under 2^-150), i.e. products of activations and weights far below any real value.
// Then bias / BN (qnn_epi_value), the float32 or packed shortcut with post_scale (qnn_epi_residual), fn, and the 2x2
// max-pool in k_conv_generic's window order.
//
// Structure: filters are the A operand (rows = output channels), 16 output pixels the B operand (columns), so a lane ends
// up with four consecutive channels of one pixel = one 16-byte store.  K-step s of tap t feeds lane (kq, r) channel
// 4*(s mod CIN/4) + kq of pixel r: one dword load per lane and step (the four kq lanes of a pixel read 16 contiguous
// bytes).  A block stages the k-step-major filters of NT 16-filter tiles in LDS once (qnn_f32act_prepare packs them at
// qnn_prepack_weights time, 36 KiB for every CIN) and its four waves walk tasks of NP 16-pixel groups; a wave keeps
// NT x NP independent accumulators (>= 4: the dependent latency is 40 cycles against a 32-cycle issue interval).
// Pixels are enumerated over the flattened (n, oy, ox) of the whole batch -- with pool = 2 as (pooled pixel, window
// position) quadruples of adjacent lanes -- so any H / W and any batch fills the 16 columns.
#include "qnn_mfma_common.h"

typedef float v4f __attribute__((ext_vector_type(4)));

namespace {

constexpr int kF32ActLds = 36864;   // bytes of staged filters per block: NT * KS * 64 lanes * 4 B

__device__ __forceinline__ float f32act_fn(float v, const EpiArgs& e) {
    if (e.fn == QNN_FN_LEAKY_RELU) return qnn_leaky_relu(v);
    if (e.fn == QNN_FN_BINARY_TANH) return qnn_binary_tanh(v);
    if (e.fn == QNN_FN_QUANTIZED_TANH) return qnn_quantized_tanh(v, e.act_m);
    return v;
}

// wpk[ft][s][lane] = wq[16 ft + (lane & 15)][4 s + (lane >> 4)]: one 256-byte row per 16-filter tile and K-step
__global__ __launch_bounds__(256) void k_f32act_pack(const float* __restrict__ wq, float* __restrict__ wpk, int K,
                                                     int total) {
    for (int i = blockIdx.x * 256 + threadIdx.x; i < total; i += gridDim.x * 256) {
        const int lane = i & 63, row = i >> 6;
        const int KS = K / 4;
        const int s = row % KS, ft = row / KS;
        wpk[i] = wq[(size_t)(16 * ft + (lane & 15)) * K + 4 * s + (lane >> 4)];
    }
}

template <int CIN, int KH, int NT, int NP>
__global__ __launch_bounds__(256) void k_conv_f32act(ConvGeom g, EpiArgs e, const float* __restrict__ x,
                                                     const float* __restrict__ wpk, float* __restrict__ y, int ntasks,
                                                     int ptotal) {
    constexpr int CG = CIN / 4;               // K-steps per tap
    constexpr int KS = KH * KH * CG;
    static_assert(NT * KS * 64 * 4 <= kF32ActLds, "staged filters exceed the LDS budget");
    __shared__ v4f lw4[NT * KS * 16];
    const float* lw = (const float*)lw4;
    const int lane = threadIdx.x & 63;
    const int r = lane & 15, kq = lane >> 4;
    const int fg = blockIdx.y;
    {
        const v4f* src = (const v4f*)(wpk + (size_t)fg * NT * KS * 64);
        for (int i = threadIdx.x; i < NT * KS * 16; i += 256) lw4[i] = src[i];
    }
    __syncthreads();
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const bool pool2 = g.pool == 2;
    const uint32_t cw = pool2 ? (uint32_t)g.Wp : (uint32_t)g.Wo, ch = pool2 ? (uint32_t)g.Hp : (uint32_t)g.Ho;

    for (int task = blockIdx.x * 4 + wave; task < ntasks; task += gridDim.x * 4) {
        int pn[NP], poy[NP], pox[NP], pq[NP];
        bool pv[NP];
#pragma unroll
        for (int j = 0; j < NP; ++j) {
            const int P = (task * NP + j) * 16 + r;
            pv[j] = P < ptotal;
            const uint32_t Pc = pv[j] ? (uint32_t)P : 0u;
            const uint32_t q = pool2 ? Pc >> 2 : Pc;
            const uint32_t qx = q % cw, t = q / cw;
            const uint32_t qy = t % ch;
            pn[j] = (int)(t / ch);
            pq[j] = (int)q;
            poy[j] = pool2 ? 2 * (int)qy + (int)((Pc >> 1) & 1u) : (int)qy;
            pox[j] = pool2 ? 2 * (int)qx + (int)(Pc & 1u) : (int)qx;
        }
        v4f acc[NT][NP];
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int j = 0; j < NP; ++j) acc[t][j] = v4f{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll 1
        for (int tap = 0; tap < KH * KH; ++tap) {
            const int dy = tap / KH, dx = tap - dy * KH;
            const float* bp[NP];
            bool bv[NP];
#pragma unroll
            for (int j = 0; j < NP; ++j) {
                const int iy = poy[j] * g.stride + dy - g.pt, ix = pox[j] * g.stride + dx - g.pl;
                bv[j] = pv[j] && (unsigned)iy < (unsigned)g.H && (unsigned)ix < (unsigned)g.W;
                const size_t off = bv[j] ? (((size_t)pn[j] * g.H + iy) * g.W + ix) * CIN + kq : 0;
                bp[j] = x + off;
            }
            const float* la = lw + tap * CG * 64 + lane;
            float b[CG][NP];
#pragma unroll
            for (int c = 0; c < CG; ++c)
#pragma unroll
                for (int j = 0; j < NP; ++j) b[c][j] = bv[j] ? bp[j][4 * c] : 0.0f;
#pragma unroll
            for (int c = 0; c < CG; ++c) {
                float a[NT];
#pragma unroll
                for (int t = 0; t < NT; ++t) a[t] = la[(t * KS + c) * 64];
#pragma unroll
                for (int t = 0; t < NT; ++t)
#pragma unroll
                    for (int j = 0; j < NP; ++j)
                        acc[t][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[t], b[c][j], acc[t][j], 0, 0, 0);
            }
        }
        // epilogue: lane (kq, r) holds channels 16 ft + 4 kq + i of pixel r of group j
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const int c0 = (fg * NT + t) * 16 + 4 * kq;
#pragma unroll
            for (int j = 0; j < NP; ++j) {
                v4f v;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    float u = qnn_epi_value(acc[t][j][i], c0 + i, e);
                    if (!pool2 && pv[j]) u = qnn_epi_residual(u, (long)pq[j], c0 + i, e);
                    v[i] = f32act_fn(u, e);
                }
                if (pool2) {
                    // k_conv_generic's order: best = max(max(max(v(0,0), v(0,1)), v(1,0)), v(1,1)); lanes r = 4 p + w
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const float v1 = __shfl_xor(v[i], 1), v2 = __shfl_xor(v[i], 2), v3 = __shfl_xor(v[i], 3);
                        v[i] = fmaxf(fmaxf(fmaxf(v[i], v1), v2), v3);
                    }
                    if (pv[j] && (r & 3) == 0) *(v4f*)(y + (size_t)pq[j] * g.cout + c0) = v;
                } else if (pv[j]) {
                    *(v4f*)(y + (size_t)pq[j] * g.cout + c0) = v;
                }
            }
        }
    }
}

template <int CIN, int KH, int NT, int NP>
void launch_f32act(const ConvGeom& g, const EpiArgs& e, const float* x, const float* wpk, float* y, hipStream_t s,
                   int ptotal) {
    const int ntasks = (ptotal + 16 * NP - 1) / (16 * NP);
    const int nfg = g.cout / (16 * NT);
    int bx = (ntasks + 3) / 4;
    const int cap = 1024 / nfg > 0 ? 1024 / nfg : 1;     // ~4 resident blocks per CU over 256 CUs
    if (bx > cap) bx = cap;
    hipLaunchKernelGGL((k_conv_f32act<CIN, KH, NT, NP>), dim3((unsigned)bx, (unsigned)nfg), dim3(256), 0, s, g, e, x,
                       wpk, y, ntasks, ptotal);
}

// shapes the kernel serves (the prepared filter image exists exactly for these)
bool f32act_shape(int kh, int kw, int stride, int same_pad, int cin, int cout) {
    if (!(cin == 16 || cin == 32 || cin == 64) || cout % 16 != 0 || cout > 256 || !same_pad || kh != kw) return false;
    return (kh == 3 && (stride == 1 || stride == 2)) || (kh == 1 && stride == 2);
}

// filter tiles per block: as many as divide cout / 16 within the LDS budget (36 KiB at 3x3)
int f32act_nt(int cin, int cout) {
    const int tiles = cout / 16, ntmax = 64 / cin;
    for (int nt = 4; nt > 1; nt >>= 1)
        if (nt <= ntmax && tiles % nt == 0) return nt;
    return 1;
}

}  // namespace

// the k-step-major filter image next to d_wq (freed by qnn_free_weights)
int qnn_f32act_prepare(qnn_weights* w, hipStream_t s) {
    // only handles prepacked for float32 inputs reach this kernel (packed stores take the integer routes)
    if (w->store != QNN_STORE_F32 || !w->d_wq || !f32act_shape(w->kh, w->kw, w->stride, w->same_pad, w->cin, w->cout))
        return QNN_OK;
    const int K = w->kh * w->kw * w->cin;
    const size_t n = (size_t)w->cout * K;
    QNN_HIP(hipMalloc(&w->d_f32act, n * sizeof(float)));
    int grid = (int)((n + 255) / 256);
    if (grid > 4096) grid = 4096;
    hipLaunchKernelGGL(k_f32act_pack, dim3(grid), dim3(256), 0, s, w->d_wq, w->d_f32act, K, (int)n);
    QNN_HIP(hipGetLastError());
    return QNN_OK;
}

// 0 = launched.  Eligibility: float32 input of any values, 16 / 32 / 64 channels, cout a multiple of 16 up to 256,
// 3x3 SAME stride 1 / 2 or 1x1 stride 2, float32 output, pool 1 / 2, no identity trick, fold or in-launch projection.
int qnn_try_launch_f32act(const ConvGeom& g, const EpiArgs& e, const void* x, const qnn_weights* w, void* y,
                          hipStream_t s, char* name, size_t name_len) {
    if (!w->d_f32act || e.out_store != QNN_STORE_F32 || e.trick_s != 0.0f || e.fold_a || e.proj_x) return 1;
    if (e.fn != QNN_FN_NONE && e.fn != QNN_FN_LEAKY_RELU && e.fn != QNN_FN_BINARY_TANH &&
        e.fn != QNN_FN_QUANTIZED_TANH)
        return 1;
    if (e.first_mode != 0 || (g.pool != 1 && g.pool != 2) || (e.res && g.pool != 1)) return 1;
    if (g.cin != w->cin || g.cout != w->cout || e.ocw != g.cout) return 1;
    if (((uintptr_t)y & 15) != 0 || ((uintptr_t)x & 3) != 0) return 1;
    const double pt = (double)g.N * g.Hp * g.Wp * g.pool * g.pool;
    if (pt >= 2.0e9) return 1;
    const int ptotal = (int)pt;
    const int nt = f32act_nt(g.cin, g.cout);
    const float* xf = (const float*)x;
    float* yf = (float*)y;
    snprintf(name, name_len, "mfma_f32_act_c%d%s", g.cin, g.kh == 1 ? "_pw" : g.stride == 2 ? "_s2" : "");
#define F32ACT_CASE(CIN_, KH_, NT_, NP_)                                                                               \
    if (g.cin == CIN_ && g.kh == KH_ && nt == NT_) {                                                                   \
        launch_f32act<CIN_, KH_, NT_, NP_>(g, e, xf, w->d_f32act, yf, s, ptotal);                                      \
        return 0;                                                                                                      \
    }
    F32ACT_CASE(16, 3, 4, 2) F32ACT_CASE(16, 3, 2, 2) F32ACT_CASE(16, 3, 1, 4)
    F32ACT_CASE(32, 3, 2, 2) F32ACT_CASE(32, 3, 1, 4)
    F32ACT_CASE(64, 3, 1, 4)
    F32ACT_CASE(16, 1, 4, 2) F32ACT_CASE(16, 1, 2, 2) F32ACT_CASE(16, 1, 1, 4)
    F32ACT_CASE(32, 1, 2, 2) F32ACT_CASE(32, 1, 1, 4)
    F32ACT_CASE(64, 1, 1, 4)
#undef F32ACT_CASE
    return 1;
}

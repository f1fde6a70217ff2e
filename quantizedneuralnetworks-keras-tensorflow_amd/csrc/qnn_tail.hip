// The classifier tail of every ResNet (models/resnet.py:134-140) in ONE launch:
//     y = softmax(dense(flatten(avgpool_size(x))))        x: packed NHWC codes (QNN_STORE_BIN / _I4 / _I8)
// instead of k_avgpool_packed / k_avgpool_i4_wave -> k_dense_f32in -> k_softmax_rows with two float32 round trips
// through HBM.  Bit-identical to those three launches; what that takes, per phase:
//
//   average  integer window sums of the codes (any order: integers), then ONE rounding chain
//            __fdiv_rn(__fmul_rn((float)acc, inv_m), area) -- k_avgpool_packed, qnn_elementwise.hip:288.  The Ho*Wo*C
//            averages of an image stay in LDS as float32 in flatten order (oy, ox, c).
//   dense    the summation order of k_dense_f32in (qnn_conv.hip:322-354), the kernel qnn_dense_forward reaches for a
//            float32 input and a QNN_STORE_F32 handle (route_dense, qnn_conv.hip:1301-1310): every float32 product exact
//            in float64; K % 4 == 0: lane l takes k = 4l + 256i, acc0 += p[k], acc1 += p[k+1], acc0 += p[k+2],
//            acc1 += p[k+3]; else lane l takes k = l + 64i into acc0; sum = acc0 + acc1, __shfl_xor butterfly over the
//            offsets 32..1, one rounding to float32.  No fma anywhere (products and sums are separate float64
//            operations; the library is built with -ffp-contract=off).  Then qnn_epi_value: + bias, * bn_inv + bn_shift.
//            A dot product whose non-zero lanes fit an aligned group of `seg` < 64 lanes is reduced inside that group
//            only: the skipped butterfly steps would add +0.0 (a sum formed as 0.0 + ... is never -0.0), so the bits
//            are the same and 64 / seg dot products share a wave.
//   softmax  the arithmetic of k_softmax_rows (qnn_elementwise.hip:332-353): maximum and sum in float64, thread t of a
//            256-thread workgroup takes the columns t + 256j, butterfly 32..1 within each of its four waves, then
//            fmax(fmax(r0, r1), fmax(r2, r3)) and (r0 + r1) + (r2 + r3); y = (float)(exp(x - mx) / sum).  Here ONE wave
//            plays the four waves one after the other (the same operations on the same values in the same tree); with
//            cols <= 64 only wave 0 holds terms, the other three are the identities -inf and 0.0 and are not computed;
//            with cols <= 32 a row is reduced inside an aligned lane group, as above.
//
// Work mapping (chosen by the host from the shapes): a workgroup takes G images.  Pooling: a task = (image, output pixel,
// packed word) is summed by S lanes (S a power of two, 8 where the window has that many pixels: lane (task, slot) reads
// the window's pixels slot, slot + S, ..., so the lanes of a wave read whole consecutive pixels, as k_avgpool_i4_wave
// does), then log2(S) shuffle steps.  CIFAR (8x8x64 -> 64 -> 10, thousands of images): G = 4 images per 256-thread
// workgroup, one pass each for pooling and softmax.  ImageNet (56x56x64 -> 3136 -> 10, tens of images): one
// 1024-thread workgroup per image.
//
// LDS: G * (Ho*Wo*C + classes) float32 (averages + logits), dynamic.  CAP: 64 KiB per workgroup (16384 floats; the
// ImageNet-224 ResNet needs 12.6 KB); a larger tail is declined with QNN_EUNSUPPORTED and runs as three launches.
// Only vector stores; no allocation, no host synchronisation, no host memory: capturable into a hipGraph.
#include "qnn_common.h"

namespace {

constexpr int kTailLdsCap = 64 * 1024;      // bytes per workgroup
constexpr int kTailMaxImages = 8;           // images per workgroup

struct TailArgs {
    const uint32_t* x;       // packed codes, N x H x W x cw words
    const float* wq;         // [classes][K] quantized dense kernel as float32 (qnn_weights.d_wq)
    const float* bias;       // [classes] or nullptr
    const float* bn_inv;     // [classes] or nullptr
    const float* bn_shift;
    float* logits;           // (N, classes) or nullptr
    float* y;                // (N, classes): softmax, or the logits when softmax == 0
    int N, H, W, C, cw, size, Ho, Wo;
    int K, classes;
    int G;                   // images per workgroup
    int lgS;                 // log2 of the lanes that share one pooling task
    int dseg;                // lanes of one dot product's reduction group (power of two <= 64)
    int sseg;                // lanes of one softmax row's reduction group
    int softmax;
    float inv_m;             // 2^-(bits-1); BIN: 1
};

template <int STORE>
__global__ __launch_bounds__(1024) void k_tail_avg_dense_softmax(TailArgs a) {
    constexpr int PW = (STORE == QNN_STORE_BIN) ? 32 : (STORE == QNN_STORE_I4) ? 8 : 4;
    constexpr int BITS = 32 / PW;
    extern __shared__ __align__(16) float lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nwaves = blockDim.x >> 6;
    const int n0 = blockIdx.x * a.G;
    const int G = min(a.G, a.N - n0);                   // images of this workgroup
    float* avg = lds;                                   // [a.G][K]
    float* lg = lds + (size_t)a.G * a.K;                // [a.G][classes]

    // ---- window averages into LDS ----
    {
        const int S = 1 << a.lgS, slot = tid & (S - 1);
        const int per_image = a.Ho * a.Wo * a.cw, tasks = G * per_image, stride = blockDim.x >> a.lgS;
        const int area = a.size * a.size;
        const float farea = (float)area;
        for (int base = 0; base < tasks; base += stride) {          // same trip count for every lane (shuffles below)
            const int task = base + (tid >> a.lgS);
            const bool live = task < tasks;
            int acc[PW];
#pragma unroll
            for (int i = 0; i < PW; ++i) acc[i] = 0;
            int g = 0, o = 0, j = 0;
            if (live) {
                g = task / per_image;
                const int r = task - g * per_image;
                o = r / a.cw;
                j = r - o * a.cw;
                const int oy = o / a.Wo, ox = o - oy * a.Wo;
                const uint32_t* win = a.x + (((size_t)(n0 + g) * a.H + (size_t)oy * a.size) * a.W + (size_t)ox * a.size) * a.cw + j;
                for (int k = slot; k < area; k += S) {
                    const int dy = k / a.size, dx = k - dy * a.size;
                    const uint32_t word = win[((size_t)dy * a.W + dx) * a.cw];
#pragma unroll
                    for (int i = 0; i < PW; ++i) {
                        if constexpr (STORE == QNN_STORE_BIN) acc[i] += ((word >> i) & 1u) ? 1 : -1;
                        else acc[i] += (int)(word << (32 - BITS - BITS * i)) >> (32 - BITS);
                    }
                }
            }
            for (int off = S >> 1; off >= 1; off >>= 1) {
#pragma unroll
                for (int i = 0; i < PW; ++i) acc[i] += __shfl_xor(acc[i], off);
            }
            if (live && slot == 0) {
                float* dst = avg + (size_t)g * a.K + (size_t)o * a.C + j * PW;
#pragma unroll
                for (int i = 0; i < PW; ++i)
                    if (j * PW + i < a.C) dst[i] = __fdiv_rn(__fmul_rn((float)acc[i], a.inv_m), farea);
            }
        }
    }
    __syncthreads();

    // ---- dense: one dot product per group of `dseg` lanes ----
    {
        const int seg = a.dseg, sl = lane & (seg - 1), per_wave = 64 / seg;
        const int dots = G * a.classes, stride = nwaves * per_wave;
        const bool vec = (a.K & 3) == 0;
        for (int base = 0; base < dots; base += stride) {
            const int d = base + wave * per_wave + lane / seg;
            const bool live = d < dots;
            const int g = live ? d / a.classes : 0, c = live ? d - g * a.classes : 0;
            const float* xa = avg + (size_t)g * a.K;
            const float* w = a.wq + (size_t)c * a.K;
            double acc0 = 0.0, acc1 = 0.0;
            if (live) {
                if (vec) {
                    for (int k = 4 * sl; k < a.K; k += 256) {
                        const float4 av = *reinterpret_cast<const float4*>(xa + k);
                        const float4 wv = *reinterpret_cast<const float4*>(w + k);
                        acc0 += (double)av.x * (double)wv.x;
                        acc1 += (double)av.y * (double)wv.y;
                        acc0 += (double)av.z * (double)wv.z;
                        acc1 += (double)av.w * (double)wv.w;
                    }
                } else {
                    for (int k = sl; k < a.K; k += 64) acc0 += (double)xa[k] * (double)w[k];
                }
            }
            double sum = acc0 + acc1;
#pragma unroll
            for (int off = 32; off > 0; off >>= 1)
                if (off < seg) sum += __shfl_xor(sum, off, 64);
            if (live && sl == 0) {
                float v = (float)sum;
                if (a.bias) v = __fadd_rn(v, a.bias[c]);
                if (a.bn_inv) v = __fadd_rn(__fmul_rn(v, a.bn_inv[c]), a.bn_shift[c]);
                lg[g * a.classes + c] = v;
                const size_t at = (size_t)(n0 + g) * a.classes + c;
                if (a.logits) a.logits[at] = v;
                if (!a.softmax) a.y[at] = v;
            }
        }
    }
    if (!a.softmax) return;
    __syncthreads();

    // ---- softmax: one row per group of `sseg` lanes, the group's wave playing k_softmax_rows' four waves ----
    {
        const int seg = a.sseg, sl = lane & (seg - 1), per_wave = 64 / seg, cols = a.classes;
        const int nv = cols <= 64 ? 1 : 4;              // waves of k_softmax_rows that hold terms
        for (int base = 0; base < G; base += nwaves * per_wave) {
            const int g = base + wave * per_wave + lane / seg;
            const bool live = g < G;
            const float* xr = lg + (live ? g : 0) * cols;
            double red[4];
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                double mx = -__builtin_huge_val();
                if (v < nv) {
                    if (live)
                        for (int c = 64 * v + sl; c < cols; c += 256) mx = fmax(mx, (double)xr[c]);
#pragma unroll
                    for (int off = 32; off >= 1; off >>= 1)
                        if (off < seg) mx = fmax(mx, __shfl_xor(mx, off));
                }
                red[v] = mx;
            }
            const double mx = fmax(fmax(red[0], red[1]), fmax(red[2], red[3]));
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                double sum = 0.0;
                if (v < nv) {
                    if (live)
                        for (int c = 64 * v + sl; c < cols; c += 256) sum += exp((double)xr[c] - mx);
#pragma unroll
                    for (int off = 32; off >= 1; off >>= 1)
                        if (off < seg) sum += __shfl_xor(sum, off);
                }
                red[v] = sum;
            }
            const double sum = (red[0] + red[1]) + (red[2] + red[3]);
            if (live) {
                float* yr = a.y + (size_t)(n0 + g) * cols;
                for (int v = 0; v < nv; ++v)
                    for (int c = 64 * v + sl; c < cols; c += 256) yr[c] = (float)(exp((double)xr[c] - mx) / sum);
            }
        }
    }
}

int pow2_at_least(int v) {
    int p = 1;
    while (p < v) p <<= 1;
    return p;
}

}  // namespace

extern "C" int qnn_avgpool_dense_softmax_forward(const qnn_weights_t* wd, const void* x, int x_store, int x_bits,
                                                 int N, int H, int W, int C, int size, const qnn_epilogue_t* epi_dense,
                                                 int softmax, float* logits_or_null, float* y, void* stream) {
    // an empty batch has no addresses: the pointers of empty tensors are null
    QNN_REQUIRE(wd && epi_dense && ((x && y) || N == 0), QNN_EINVAL, "qnn_avgpool_dense_softmax_forward: null pointer");
    QNN_REQUIRE(N >= 0 && H > 0 && W > 0 && C > 0 && size > 0 && size <= H && size <= W, QNN_EINVAL,
                "qnn_avgpool_dense_softmax_forward: shape (%d,%d,%d,%d) size %d", N, H, W, C, size);
    if (x_store == QNN_STORE_T2) {
        qnn_set_error("qnn_avgpool_dense_softmax_forward: no fused kernel for QNN_STORE_T2 input");
        return QNN_EUNSUPPORTED;
    }
    QNN_REQUIRE(x_store == QNN_STORE_BIN || ((x_store == QNN_STORE_I4 || x_store == QNN_STORE_I8) && x_bits >= 1 && x_bits <= x_store),
                QNN_EINVAL, "qnn_avgpool_dense_softmax_forward: x_store=%d x_bits=%d", x_store, x_bits);
    const int Ho = H / size, Wo = W / size;
    QNN_REQUIRE(wd->kh == 1 && wd->kw == 1, QNN_EINVAL,
                "qnn_avgpool_dense_softmax_forward: weights were prepacked as a %dx%d conv", wd->kh, wd->kw);
    QNN_REQUIRE(wd->dil_h == 1 && wd->dil_w == 1, QNN_EUNSUPPORTED,
                "qnn_avgpool_dense_softmax_forward: a dense layer has no dilation (handle prepacked with %d x %d)", wd->dil_h, wd->dil_w);
    QNN_REQUIRE((long)Ho * Wo * C == (long)wd->cin, QNN_EINVAL,
                "qnn_avgpool_dense_softmax_forward: the dense layer takes %d inputs, the pooled tensor has %d x %d x %d",
                wd->cin, Ho, Wo, C);
    QNN_REQUIRE((epi_dense->bn_inv == nullptr) == (epi_dense->bn_shift == nullptr), QNN_EINVAL,
                "qnn_avgpool_dense_softmax_forward: bn_inv and bn_shift must both be set or both be NULL");
    if (wd->store != QNN_STORE_F32 || !wd->d_wq) {
        qnn_set_error("qnn_avgpool_dense_softmax_forward: the dense handle must be prepacked for QNN_STORE_F32 (store=%d)",
                      wd->store);
        return QNN_EUNSUPPORTED;
    }
    QNN_REFUSE_MAXACT(epi_dense->fn, "qnn_avgpool_dense_softmax_forward");
    if (epi_dense->fn != QNN_FN_NONE || epi_dense->pool != 1 || epi_dense->res || epi_dense->proj || epi_dense->trick_s != 0.0f ||
        epi_dense->out_store != QNN_STORE_F32) {
        qnn_set_error("qnn_avgpool_dense_softmax_forward: no fused kernel for a dense epilogue with an activation, pooling, a "
                      "residual, the identity trick or a packed output");
        return QNN_EUNSUPPORTED;
    }
    const int K = wd->cin, classes = wd->cout;
    const long per_image_bytes = ((long)K + classes) * 4;
    if (per_image_bytes > kTailLdsCap) {
        qnn_set_error("qnn_avgpool_dense_softmax_forward: %d averages + %d logits per image exceed the %d-byte LDS cap", K,
                      classes, kTailLdsCap);
        return QNN_EUNSUPPORTED;
    }
    if (N == 0) return QNN_OK;

    TailArgs a;
    a.x = (const uint32_t*)x; a.wq = wd->d_wq; a.bias = wd->d_bias;
    a.bn_inv = epi_dense->bn_inv; a.bn_shift = epi_dense->bn_shift;
    a.logits = logits_or_null; a.y = y;
    a.N = N; a.H = H; a.W = W; a.C = C; a.cw = qnn_words(x_store, C); a.size = size; a.Ho = Ho; a.Wo = Wo;
    a.K = K; a.classes = classes; a.softmax = softmax ? 1 : 0;
    a.inv_m = x_store == QNN_STORE_BIN ? 1.0f : 1.0f / (float)(1u << (x_bits - 1));
    // lanes per pooling task: 8 (whole pixels per load, three shuffle steps), fewer for a smaller window, more while
    // the images of a workgroup leave lanes of its 256 threads without a task
    const long area = (long)size * size, tasks = (long)Ho * Wo * a.cw;
    int S = 1;
    while (S < 8 && 2 * S <= area) S <<= 1;
    while (S < 64 && 2 * S <= area && tasks * 2 * S * (N < kTailMaxImages ? N : kTailMaxImages) <= 256) S <<= 1;
    a.lgS = 0;
    while ((1 << a.lgS) < S) ++a.lgS;
    const int threads = tasks * S >= 1024 ? 1024 : 256;
    long G = threads / (tasks * S);
    if (G < 1) G = 1;
    if (G > kTailMaxImages) G = kTailMaxImages;
    if (G > kTailLdsCap / per_image_bytes) G = kTailLdsCap / per_image_bytes;
    if (G > N) G = N;
    a.G = (int)G;
    // lanes that hold non-zero terms of a dot product / a softmax row, rounded up to a power of two
    const int dlanes = (K & 3) == 0 ? (K + 3) / 4 : K;
    a.dseg = dlanes >= 64 ? 64 : pow2_at_least(dlanes);
    a.sseg = classes >= 64 ? 64 : pow2_at_least(classes);
    const size_t lds = (size_t)a.G * per_image_bytes;
    const unsigned blocks = (unsigned)((N + a.G - 1) / a.G);
    hipStream_t s = (hipStream_t)stream;
    if (x_store == QNN_STORE_BIN)
        hipLaunchKernelGGL(k_tail_avg_dense_softmax<QNN_STORE_BIN>, dim3(blocks), dim3(threads), lds, s, a);
    else if (x_store == QNN_STORE_I4)
        hipLaunchKernelGGL(k_tail_avg_dense_softmax<QNN_STORE_I4>, dim3(blocks), dim3(threads), lds, s, a);
    else
        hipLaunchKernelGGL(k_tail_avg_dense_softmax<QNN_STORE_I8>, dim3(blocks), dim3(threads), lds, s, a);
    QNN_HIP(hipGetLastError());
    qnn_set_kernel_name(a.softmax ? "tail_avg_dense_softmax" : "tail_avg_dense");
    return QNN_OK;
}

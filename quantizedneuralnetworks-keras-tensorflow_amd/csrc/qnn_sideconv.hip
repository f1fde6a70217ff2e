// Host side of qnn_sideconv.h: the weight quantiser's two kernels behind their launchers, the common part of the
// depthwise / transposed / grouped convolution handles, and the checks their forward entries share.
#include <stdio.h>

#include "qnn_sideconv.h"

namespace {

constexpr int kBlock = 256;

// ternary_ops.py:15-30: cutoff = 0.7 * mean(|W / H|) over the WHOLE kernel.  One block,
// fixed reduction order (deterministic), double accumulation.
__global__ __launch_bounds__(1024) void k_tern_cutoff(const float* __restrict__ kernel, int n, float H,
                                                      float* __restrict__ cutoff) {
    __shared__ double part[1024];
    double s = 0.0;
    for (int i = threadIdx.x; i < n; i += 1024) s += (double)fabsf(__fdiv_rn(kernel[i], H));
    part[threadIdx.x] = s;
    __syncthreads();
    for (int off = 512; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) part[threadIdx.x] += part[threadIdx.x + off];
        __syncthreads();
    }
    if (threadIdx.x == 0) cutoff[0] = __fmul_rn(0.7f, (float)(part[0] / (double)n));
}

// the quantiser elementwise, in the kernel's own order; the codes are value * 2^wshift (binary / ternary on a packed
// store have H = 1: the value itself)
__global__ __launch_bounds__(kBlock) void k_quantize(const float* __restrict__ kernel, float* __restrict__ wq,
                                                     int32_t* __restrict__ wcode, int n, int wkind, float H, float m,
                                                     const float* __restrict__ cutoff_p) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const float q = qnn_quantize_weight(kernel[i], wkind, H, m, wkind == QNN_W_TERNARY ? cutoff_p[0] : 0.0f);
    wq[i] = q;
    if (wcode) wcode[i] = (int)__fmul_rn(q, m);
}

}  // namespace

void qnn_launch_tern_cutoff(const float* kernel, int n, float H, float* cutoff, hipStream_t s) {
    hipLaunchKernelGGL(k_tern_cutoff, dim3(1), dim3(1024), 0, s, kernel, n, H, cutoff);
}

int qnn_side_hip(hipError_t err, const char* what) {
    if (err == hipSuccess) return QNN_OK;
    qnn_set_error("%s failed: %s", what, hipGetErrorString(err));
    return err == hipErrorOutOfMemory ? QNN_ENOMEM : QNN_EHIP;
}

int qnn_side_weights_check(const char* who, int wkind, int wbits, float H, int store, SideWeights* w) {
    QNN_REQUIRE(wkind == QNN_W_FLOAT || wkind == QNN_W_BINARY || wkind == QNN_W_QUANT || wkind == QNN_W_TERNARY,
                QNN_EINVAL, "%s: wkind=%d not supported", who, wkind);
    QNN_REQUIRE(H > 0.0f, QNN_EINVAL, "%s: H=%g", who, (double)H);
    if (wkind == QNN_W_QUANT) QNN_REQUIRE(wbits >= 2 && wbits <= 24, QNN_EINVAL, "%s: wbits=%d", who, wbits);
    switch (store) {
        case QNN_STORE_F32:
            break;
        case QNN_STORE_BIN:
            QNN_REQUIRE(wkind == QNN_W_BINARY && H == 1.0f, QNN_EINVAL, "%s: BIN storage needs binary weights with H=1", who);
            break;
        case QNN_STORE_I4:
        case QNN_STORE_I8:
            QNN_REQUIRE(((wkind == QNN_W_BINARY || wkind == QNN_W_TERNARY) && H == 1.0f) ||
                            (wkind == QNN_W_QUANT && wbits <= store),
                        QNN_EINVAL, "%s: wkind=%d wbits=%d does not fit %d-bit storage", who, wkind, wbits, store);
            break;
        case QNN_STORE_T2:
            QNN_REQUIRE((wkind == QNN_W_BINARY || wkind == QNN_W_TERNARY) && H == 1.0f, QNN_EINVAL,
                        "%s: sign / mask storage needs ternary (or binary) weights with H=1", who);
            break;
        default:
            qnn_set_error("%s: store=%d", who, store);
            return QNN_EINVAL;
    }
    w->wkind = wkind; w->wbits = wbits; w->H = H;
    w->store = store;
    w->wshift = wkind == QNN_W_QUANT ? wbits - 1 : 0;
    return QNN_OK;
}

int qnn_side_quantize(SideWeights* w, const float* kernel, int n, const float* bias, int cout, hipStream_t s) {
    QNN_SIDE_HIP(hipMalloc(&w->d_wq, (size_t)n * sizeof(float)));
    if (w->store != QNN_STORE_F32) QNN_SIDE_HIP(hipMalloc(&w->d_wcode, (size_t)n * sizeof(int32_t)));
    if (w->wkind == QNN_W_TERNARY) {
        QNN_SIDE_HIP(hipMalloc(&w->d_aux, 16));
        qnn_launch_tern_cutoff(kernel, n, w->H, w->d_aux, s);
    }
    hipLaunchKernelGGL(k_quantize, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, s, kernel, w->d_wq, w->d_wcode, n,
                       w->wkind, w->H, (float)(1u << w->wshift), (const float*)w->d_aux);
    if (bias) {
        QNN_SIDE_HIP(hipMalloc(&w->d_bias, (size_t)cout * sizeof(float)));
        QNN_SIDE_HIP(hipMemcpyAsync(w->d_bias, bias, (size_t)cout * sizeof(float), hipMemcpyDeviceToDevice, s));
    }
    return QNN_OK;
}

void qnn_side_free(SideWeights* w) {
    if (w->d_wq) (void)hipFree(w->d_wq);
    if (w->d_wcode) (void)hipFree(w->d_wcode);
    if (w->d_bias) (void)hipFree(w->d_bias);
    if (w->d_aux) (void)hipFree(w->d_aux);
}

int qnn_side_forward_check(const char* who, const SideWeights* w, int cout, int x_store, int x_bits, const qnn_epilogue_t* epi,
                           const char* layer, int* xshift, EpiArgs* e) {
    QNN_REQUIRE(x_store != QNN_STORE_U8 && x_store != QNN_STORE_F32_IMAGE && x_store != QNN_STORE_F32_UNIT,
                QNN_EUNSUPPORTED, "%s: x_store=%d (QNN_STORE_U8 and the typed float32 stores are first-layer inputs of "
                "qnn_conv2d_forward)", who, x_store);
    const bool packed = x_store != QNN_STORE_F32;
    *xshift = 0;
    if (packed) {
        QNN_REQUIRE(x_store == QNN_STORE_BIN || x_store == QNN_STORE_T2 || x_store == QNN_STORE_I4 || x_store == QNN_STORE_I8,
                    QNN_EINVAL, "%s: x_store=%d", who, x_store);
        QNN_REQUIRE(x_store == w->store, QNN_EINVAL, "%s: x_store=%d but the weights were prepacked for store=%d", who,
                    x_store, w->store);
        if (x_store == QNN_STORE_I4 || x_store == QNN_STORE_I8) {
            QNN_REQUIRE(x_bits >= 1 && x_bits <= x_store, QNN_EINVAL, "%s: x_bits=%d does not fit %d-bit storage", who,
                        x_bits, x_store);
            *xshift = x_bits - 1;
        }
    }
    // ---- the epilogue subset ----
    QNN_REQUIRE(epi->pool == 1, QNN_EUNSUPPORTED, "%s: epilogue field pool=%d (no pooling behind %s)", who, epi->pool, layer);
    QNN_REQUIRE(!epi->res, QNN_EUNSUPPORTED, "%s: epilogue field res (no residual input)", who);
    QNN_REQUIRE(!epi->fold, QNN_EUNSUPPORTED, "%s: epilogue field fold (no folded epilogue)", who);
    QNN_REQUIRE(!epi->proj, QNN_EUNSUPPORTED, "%s: epilogue field proj (no in-launch projection)", who);
    QNN_REQUIRE(epi->trick_s == 0.0f, QNN_EUNSUPPORTED, "%s: epilogue field trick_s=%g (no identity trick)", who,
                (double)epi->trick_s);
    QNN_REQUIRE(epi->flags == 0u, QNN_EUNSUPPORTED, "%s: epilogue field flags=%u (no kernel-selection bits)", who, epi->flags);
    QNN_REQUIRE((epi->bn_inv == nullptr) == (epi->bn_shift == nullptr), QNN_EINVAL,
                "%s: bn_inv and bn_shift must both be set or both be NULL", who);
    QNN_REFUSE_MAXACT(epi->fn, who);
    const int fn = epi->fn, os = epi->out_store;
    QNN_REQUIRE(fn == QNN_FN_NONE || fn == QNN_FN_BINARY_TANH || qnn_is_qact(fn) || fn == QNN_FN_LEAKY_RELU, QNN_EINVAL,
                "%s: fn=%d cannot be fused", who, fn);
    QNN_REQUIRE(fn != QNN_FN_LEAKY_RELU || os == QNN_STORE_F32, QNN_EINVAL, "%s: leaky_relu needs a float32 output", who);
    if (qnn_is_qact(fn)) QNN_REQUIRE(epi->act_bits >= 2 && epi->act_bits <= 24, QNN_EINVAL, "%s: act_bits=%d", who, epi->act_bits);
    QNN_REQUIRE(os == QNN_STORE_F32 || os == QNN_STORE_BIN || os == QNN_STORE_I4 || os == QNN_STORE_I8, QNN_EINVAL,
                "%s: out_store=%d", who, os);
    QNN_REQUIRE(os != QNN_STORE_BIN || fn == QNN_FN_BINARY_TANH, QNN_EINVAL, "%s: BIN output needs fn=binary_tanh", who);
    QNN_REQUIRE(!(os == QNN_STORE_I4 || os == QNN_STORE_I8) || fn == QNN_FN_BINARY_TANH ||
                    (qnn_is_qact(fn) && epi->act_bits <= os),
                QNN_EINVAL, "%s: fn=%d act_bits=%d does not fit %d-bit output", who, fn, epi->act_bits, os);

    *e = EpiArgs{};
    e->bias = w->d_bias;
    e->bn_inv = epi->bn_inv;
    e->bn_shift = epi->bn_shift;
    e->scale = packed ? ldexpf(1.0f, -(w->wshift + *xshift)) : 1.0f;
    e->act_m = qnn_is_qact(fn) ? (float)(1u << (epi->act_bits - 1)) : 1.0f;
    e->fn = fn;
    e->out_store = os;
    e->ocw = os == QNN_STORE_F32 ? cout : qnn_words(os, cout);
    e->post_scale = 1.0f;
    return QNN_OK;
}

int qnn_side_io_check(const char* who, int N, size_t owords, const void* x, size_t xbytes, const void* y, bool* run) {
    *run = false;
    QNN_REQUIRE(owords < ((size_t)1 << 31), QNN_EUNSUPPORTED, "%s: %zu output words (2^31 or more)", who, owords);
    if (N == 0) return QNN_OK;
    QNN_REQUIRE(x && y, QNN_EINVAL, "%s: null pointer", who);
    const uintptr_t xa = (uintptr_t)x, ya = (uintptr_t)y;
    QNN_REQUIRE(xa + xbytes <= ya || ya + owords * 4 <= xa, QNN_EINVAL, "%s: x and y overlap", who);
    *run = true;
    return QNN_OK;
}

const char* store_name(int store) {
    return store == QNN_STORE_BIN  ? "bin"
           : store == QNN_STORE_I4 ? "i4"
           : store == QNN_STORE_I8 ? "i8"
           : store == QNN_STORE_T2 ? "t2"
                                   : "f32";
}

void qnn_side_kernel_name(const char* op, int x_store, const char* route) {
    char name[40];
    const bool two_forms = x_store == QNN_STORE_I4 || x_store == QNN_STORE_I8;
    snprintf(name, sizeof(name), "%s_%s%s", op, store_name(x_store), two_forms ? route : "");
    qnn_set_kernel_name(name);
}

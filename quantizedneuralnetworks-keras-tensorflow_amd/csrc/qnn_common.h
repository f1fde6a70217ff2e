// Shared host/device helpers of the gfx950 low-bit forward engine.
// Written for CDNA4 only (wave64); no portability layer.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string>

#include "qnn_abi.h"
#include "qnn_abi_dilation.h"
#include "qnn_abi_qact.h"
#include "qnn_abi_maxact.h"
#include "qnn_abi_scaled.h"

#define QNN_WAVE 64

// ---- error plumbing --------------------------------------------------------
void qnn_set_error(const char* fmt, ...);
void qnn_set_kernel_name(const char* name);

#define QNN_HIP(expr)                                                          \
    do {                                                                       \
        hipError_t _e = (expr);                                                \
        if (_e != hipSuccess) {                                                \
            qnn_set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), \
                          __FILE__, __LINE__);                                 \
            return QNN_EHIP;                                                   \
        }                                                                      \
    } while (0)

#define QNN_REQUIRE(cond, code, ...)                                           \
    do {                                                                       \
        if (!(cond)) {                                                         \
            qnn_set_error(__VA_ARGS__);                                        \
            return (code);                                                     \
        }                                                                      \
    } while (0)

// ---- no measurement scaffolding ---------------------------------------------------
// The sources carry no run-time switch: nothing here reads the environment, and there is no ablation code.  Kernel
// selection is qnn_set_conv_impl() and the per-call QNN_EPI_* flags; A/B work compares against the parent commit, or
// rebuilds one file with a -D tuning constant (QNN_*_WPS, QNN_*_DEPTH, QNN_DMA_NBUF, ...) through tools/build_variant.py.

// ---- opaque weights handle --------------------------------------------------
struct qnn_weights {
    int wkind, wbits;
    float H;
    int kh, kw, cin, cout;
    int stride, same_pad;
    int dil_h, dil_w; // dilation_rate (qnn_prepack_weights_dilated); 1, 1 from qnn_prepack_weights
    int store;        // QNN_STORE_F32 (float path only) | BIN | I4 | I8
    int cw;           // packed words per tap (ceil(cin / per_word))
    int kwords;       // kh*kw*cw
    int wshift;       // quantized value = code * 2^-wshift
    uint32_t* d_packed;   // [cout][kh*kw][cw]   packed codes (store != F32)
    float* d_wq;          // [cout][kh*kw][cin]  quantized values as float32
    float* d_bias;        // [cout] or nullptr
    int32_t* d_corr;      // BIN + same_pad: [64][cout] zero-padding corrections
    uint8_t* d_mfma;      // int8 image [cout][kh*kw][cin] for the MFMA kernel (may alias d_packed)
    void* d_mfma_own;     // owned allocation behind d_mfma (I4 store), or nullptr
    void* d_aux;          // ternary: the 0.7*mean|W| cutoff (1 float), else nullptr
    uint32_t* d_head;     // dense 1024 -> <= 16 int4 heads: the per-lane table of the fused conv + classifier kernel
    uint32_t* h_flag;     // domain flag (pinned, device-visible host word; qnn_weights_check) or nullptr
    uint32_t* d_flag;     // the same word through the device's address space
    float* d_f32act;      // float32-activation kernel (qnn_f32act.hip): filters k-step major [cout/16][K/4][64 lanes], or nullptr
    uint8_t* d_fp6;       // I4 3x3, cin 64: the FP6 (e2m3) filter image of k_conv_mfma_halo, per 64-filter slice the 27 648
                          // bytes of the kernel's two LDS planes in LDS order (k_fp6_weights), or nullptr
    int32_t* d_fp6_wsum;  // [cout] sum of the channel's 576 weight codes (inside the d_fp6 allocation)
};

struct ConvGeom;
struct EpiArgs;
int qnn_mfma_prepare_weights(qnn_weights* w, hipStream_t s);
int qnn_conv_impl_pref();
int qnn_head_prepare(qnn_weights* w, hipStream_t s);
int qnn_try_launch_stem(const ConvGeom& g, const EpiArgs& e, const void* x, const float* wq, void* y, hipStream_t s);
int qnn_try_launch_first_fixed(const ConvGeom& g, const EpiArgs& e, const void* x, const qnn_weights* w, void* y,
                               hipStream_t s);
int qnn_f32act_prepare(qnn_weights* w, hipStream_t s);
int qnn_try_launch_f32act(const ConvGeom& g, const EpiArgs& e, const void* x, const qnn_weights* w, void* y,
                          hipStream_t s, char* name, size_t name_len);
int qnn_try_launch_first_u8(const ConvGeom& g, const EpiArgs& e, const void* x, const qnn_weights* w, void* y,
                            hipStream_t s, bool f32in);

// ---- division by a launch-constant via multiply-high (dividends < 2^31) ----------
struct FastDiv {
    uint32_t d, m;
    int s;
};
static inline FastDiv qnn_fastdiv(uint32_t d) {
    FastDiv f;
    f.d = d; f.m = 0; f.s = 0;
    if (d > 1) {
        int s = 0;
        while ((1ull << s) < d) ++s;
        f.s = s;
        f.m = (uint32_t)(((1ull << (31 + s)) + d - 1) / d);
    }
    return f;
}
#ifdef __HIPCC__
__device__ __forceinline__ uint32_t qnn_div(uint32_t q, const FastDiv& f) {
    return f.d == 1 ? q : (__umulhi(q, f.m) >> (f.s - 1));
}
#endif

// ---- geometry shared by every conv kernel ------------------------------------
struct ConvGeom {
    int N, H, W, Ho, Wo;       // Ho/Wo: conv output (before pooling)
    int cin, cout, kh, kw, stride;
    int pt, pl;                // SAME padding before (top/left)
    int dil_h, dil_w;          // rows / columns between neighbouring taps (1 = an ordinary window)
    int cw, kwords;
    int pool;                  // 1 or 2
    int Hp, Wp;                // stored output size (Ho/pool, Wo/pool)
    FastDiv fd_wp, fd_hp;      // q -> (n, py, px) without integer division
};

struct EpiArgs {
    const float* bias;         // or nullptr
    const float* bn_inv;       // or nullptr
    const float* bn_shift;
    float scale;               // 2^-(wshift+xshift); QNN_STORE_U8 input: the divisor 255 * 2^wshift
    float act_m;               // 2^(act_bits-1) for quantized_tanh
    int fn;
    int out_store;
    int ocw;                   // words per stored output pixel (packed) or cout (f32)
    const void* res;           // residual tensor (same pixels x cout) or nullptr
    int res_store;
    int res_cw;                // words (packed) or floats (f32) per residual pixel
    float res_scale;           // 2^-(res_bits-1)
    float post_scale;
    float trick_c, trick_s;    // output-side identity trick of the reference ("faithful" mode); trick_s == 0: off
    const float* fold_a;       // qnn_fold_t of this layer + epilogue (qnn_fold.h): per-channel slope, or nullptr = evaluate
    const int32_t* fold_b;     // the float32 chain; per-channel accumulator offset in units of acc / 256
    uint32_t flags;            // QNN_EPI_* kernel-selection bits of this call (qnn_epilogue_t.flags)
    int first_mode;            // domain declared for this call's float32 input: 0 none, 1 image bytes / 255, 2 [0, 1]
    uint32_t* dom_flag;        // the caller's domain-flag word for this call (qnn_epilogue_t.domain_flag) or nullptr = the handle's
    const float* fold_c;       // "bits" form of the fold (fold_b carries 0x4B400000, u = fma(as_float(acc), a, c)), or nullptr
    // projection shortcut computed inside the launch (qnn_projection_t, qnn_abi.h), or proj_x == nullptr
    const uint8_t* proj_x;     // block input: N x proj_H x proj_W x proj_cin int4 codes
    const uint8_t* proj_w;     // [cout][proj_cin] bytes code * 16 (the 1x1 kernel's d_mfma image)
    const float* proj_bias;    // or nullptr
    float proj_scale;          // 2^-(wshift + x_bits - 1) of the projection
    int proj_cin, proj_H, proj_W;
    // byte first layer with a mode-3 fold: the handle's operand table (qnn_fold.h, qnn_first_u8_entry) or nullptr = the
    // in-kernel preamble (QNN_EPI_NO_FIRST_TAB); first_tab_bits: the table carries the bits form of the fold
    const void* first_tab;
    int first_tab_bits;
    // k_conv_mfma_halo with a mode-2 fold: the handle's per-lane epilogue table (qnn_fold.h, qnn_halo_epi_entry) or nullptr =
    // the in-kernel preamble (QNN_EPI_NO_HALO_TAB, or a layer the halo kernel does not take)
    const void* halo_tab;
};

// One conv call as every route of the dispatch sees it: validated, geometry and epilogue filled in once
// (conv_describe, qnn_conv.hip).
struct ConvCall {
    ConvGeom g;
    EpiArgs e;
    const qnn_weights* w;
    const void* x;
    int x_store;               // QNN_STORE_F32 also for the typed float32 stores: their domain is e.first_mode
    void* y;
    hipStream_t s;
    bool dense;
    // qnn_abi_scaled.h: the 16-byte workspace word of the batch-scaled activation that left the packed codes in x, or nullptr
    // = an ordinary call.  Host side only: it reaches a kernel as a trailing argument of the routes that list CAP_XSCALE, so
    // no kernel's EpiArgs block (and no ordinary call's code) changes.
    const uint32_t* x_scale;
};
// the matrix-pipe routes: 0 = launched (and `name` set), 1 = declined.  qnn_route_first_f32 and qnn_route_gemm are in
// qnn_mfma.hip, qnn_route_strip is in qnn_route_strip.hip.
int qnn_route_first_f32(const ConvCall& c, char* name, size_t name_len);
int qnn_route_strip(const ConvCall& c, char* name, size_t name_len);
int qnn_route_gemm(const ConvCall& c, char* name, size_t name_len);
// the one route for dilated calls besides k_conv_generic (qnn_mfma_strip_dil.hip)
int qnn_route_strip_dil(const ConvCall& c, char* name, size_t name_len);

#ifdef __HIPCC__
#define QNN_HD __host__ __device__
#else
#define QNN_HD
#endif

QNN_HD static inline int qnn_per_word(int store) {
    return store == QNN_STORE_BIN ? 32 : store == QNN_STORE_I4 ? 8 : store == QNN_STORE_I8 ? 4 : 1;
}
QNN_HD static inline int qnn_words(int store, int channels) {
    if (store == QNN_STORE_T2) return 2 * ((channels + 31) / 32);     // (mask, sign) word pairs
    int pw = qnn_per_word(store);
    return (channels + pw - 1) / pw;
}

// qnn_same_pad: output size and leading padding of one axis (TF 'SAME' / 'VALID'), plain C++
#include "qnn_conv_geom.h"

#ifdef __HIPCC__
// ---- float32 activation clips, replayed op by op ------------------------------
// All arithmetic uses the explicitly rounded intrinsics so that no FMA
// contraction can change a rounding the reference performs.

// binary_ops.py:16-24,8-13,37-51: 2*round_through(clip(0.5x+0.5,0,1)) - 1
__device__ __forceinline__ float qnn_binary_tanh(float x) {
    float h = __fadd_rn(__fmul_rn(0.5f, x), 0.5f);
    h = fminf(fmaxf(h, 0.0f), 1.0f);
    float r = rintf(h);                          // tf.round: half to even
    float rt = __fadd_rn(h, __fsub_rn(r, h));    // x + stop_gradient(round(x) - x)
    return __fsub_rn(__fmul_rn(2.0f, rt), 1.0f);
}
// the one bit of information in binary_tanh(x): 1 <=> +1
__device__ __forceinline__ uint32_t qnn_binary_bit(float x) {
    return qnn_binary_tanh(x) > 0.0f ? 1u : 0u;
}
// quantized_ops.py:49-66,87-100 in code units: clip(round_through(x*m), -m, m-1)
__device__ __forceinline__ float qnn_quant_code_f(float x, float m) {
    float t = __fmul_rn(x, m);
    float r = rintf(t);
    float rt = __fadd_rn(t, __fsub_rn(r, t));
    return fminf(fmaxf(rt, -m), __fsub_rn(m, 1.0f));
}
// m is always 2^(bits-1): dividing by it equals multiplying by its exact reciprocal (one integer
// subtraction on the exponent field) -- an IEEE divide costs ~10 instructions per value, which made
// every float32-output epilogue with a fused clip VALU-bound
__device__ __forceinline__ float qnn_quantized_tanh(float x, float m) {
    const float inv_m = __uint_as_float(0x7F000000u - __float_as_uint(m));
    return __fmul_rn(qnn_quant_code_f(x, m), inv_m);
}

// The quantised activations that share quantized_tanh's grid (QNN_FN_QUANTIZED_TANH / _RELU / _LEAKYRELU, qnn_abi.h), as
// the one pair every kernel calls: the code as a float, and the value code / m.  `fn` is a constant at most call sites.
//   quantized_relu, quantized_ops.py:69-84: clip(2 round(clip((x+1)/2, 0, 1) 2^nb) / 2^nb - 1, 0, 1 - 1/m).  Only x + 1
//     rounds (every later step is a power-of-two scaling, an integer difference or a clip), so the code is
//     clamp(rint((x + 1) m) - m, 0, m - 1); +-inf clamp like the reference's inner clip.
//   quantized_leakyrelu, quantized_ops.py:102-123, alpha = float32(0.1): relu(x) - alpha relu(-x) is x for x >= 0 and
//     -(alpha * -x) = alpha * x (round-to-nearest is sign-symmetric) for x < 0, then quantized_tanh's clip.
QNN_HD static inline bool qnn_is_qact(int fn) {
    return fn == QNN_FN_QUANTIZED_TANH || fn == QNN_FN_QUANTIZED_RELU || fn == QNN_FN_QUANTIZED_LEAKYRELU;
}
__device__ __forceinline__ float qnn_qact_code_f(int fn, float x, float m) {
    if (fn == QNN_FN_QUANTIZED_RELU) {
        const float r = __fsub_rn(rintf(__fmul_rn(__fadd_rn(x, 1.0f), m)), m);
        return fminf(fmaxf(r, 0.0f), __fsub_rn(m, 1.0f));
    }
    if (fn == QNN_FN_QUANTIZED_LEAKYRELU) x = x >= 0.0f ? x : __fmul_rn(0.1f, x);
    return qnn_quant_code_f(x, m);
}
__device__ __forceinline__ float qnn_qact(int fn, float x, float m) {
    const float inv_m = __uint_as_float(0x7F000000u - __float_as_uint(m));
    return __fmul_rn(qnn_qact_code_f(fn, x, m), inv_m);
}

// quantized_maxrelu / quantized_leakymaxrelu (QNN_FN_QUANTIZED_MAXRELU / _LEAKYMAXRELU, qnn_abi_maxact.h): the scale is
// P = the smallest power of two >= M, M = the maximum of the whole batch tensor, so they are NOT among qnn_is_qact's
// per-value functions: every entry but the elementwise one refuses them (QNN_REFUSE_MAXACT).
QNN_HD static inline bool qnn_is_maxact(int fn) {
    return fn == QNN_FN_QUANTIZED_MAXRELU || fn == QNN_FN_QUANTIZED_LEAKYMAXRELU;
}
#define QNN_REFUSE_MAXACT(fn, who)                                                                                      \
    QNN_REQUIRE(!qnn_is_maxact(fn), QNN_EUNSUPPORTED,                                                                   \
                "%s: fn=%d (quantized_maxrelu / quantized_leakymaxrelu) scales by the maximum of the whole batch tensor " \
                "and is no per-value function: run qnn_quantized_maxact_f32 on the float32 tensor (qnn_abi_maxact.h)",  \
                who, (int)(fn))
// The two scales from the bits of M, by integer exponent arithmetic: P = 2^e, e = M's exponent plus one when its mantissa
// is not zero; s_in = m / P = 2^(nb-1-e), s_out = P / m.  False unless -64 <= e <= 64, i.e. outside 2^-65 < M <= 2^64 (zero, subnormal, inf and NaN
// patterns included): the caller writes NaN.
__device__ __forceinline__ bool qnn_maxact_scales(uint32_t mbits, int nb, float* s_in, float* s_out) {
    const int e = (int)(mbits >> 23) - 127 + ((mbits & 0x7FFFFFu) != 0u ? 1 : 0);
    if (mbits == 0u || mbits >= 0x7F800000u || e < -64 || e > 64) return false;
    *s_in = __uint_as_float((uint32_t)(127 + (nb - 1) - e) << 23);
    *s_out = __uint_as_float((uint32_t)(127 + e - (nb - 1)) << 23);
    return true;
}
// The per-value arithmetic: clip(rint(x s_in), lo, m - 1) s_out, on L(x) = (x >= 0 ? x : 0.1f x) with lo = -m for the
// leaky form, lo = 0 otherwise.  Both multiplications are exponent shifts; `+ 0` turns a -0 code into the +0 of the
// reference's round_through.
__device__ __forceinline__ float qnn_maxact_code_f(int fn, float x, float m, float s_in) {
    if (fn == QNN_FN_QUANTIZED_LEAKYMAXRELU) x = x >= 0.0f ? x : __fmul_rn(0.1f, x);
    const float lo = fn == QNN_FN_QUANTIZED_LEAKYMAXRELU ? -m : 0.0f;
    const float code = fminf(fmaxf(rintf(__fmul_rn(x, s_in)), lo), __fsub_rn(m, 1.0f));
    return __fadd_rn(code, 0.0f);
}
__device__ __forceinline__ float qnn_maxact(int fn, float x, float m, float s_in, float s_out) {
    return __fmul_rn(qnn_maxact_code_f(fn, x, m, s_in), s_out);
}
// Output scale of a scaled consumer (qnn_abi_scaled.h): scale * P with P = 2^e from the same word and the same helper as
// the activation itself (qnn_maxact_scales at nb = 1: s_out = P), one uniform load and integer exponent arithmetic.  Both
// factors are powers of two, so the product is exact; a word outside the exact range gives quiet NaN.
__device__ __forceinline__ float qnn_scaled_scale(float scale, const uint32_t* __restrict__ word) {
    float s_in = 0.0f, p = 0.0f;
    return qnn_maxact_scales(*word, 1, &s_in, &p) ? __fmul_rn(scale, p) : __uint_as_float(0x7FC00000u);
}

// Keras LeakyReLU() at its default alpha = float32(0.3): one rounding, as torch.where(v >= 0, v, v * 0.3) computes it
__device__ __forceinline__ float qnn_leaky_relu(float v) {
    return v >= 0.0f ? v : __fmul_rn(v, 0.3f);
}

// ---- dot products on packed words ----------------------------------------------
// popcount(a ^ w): number of channels whose signs differ.
__device__ __forceinline__ int qnn_dot_bin(uint32_t a, uint32_t w, int acc) {
    return acc + __popc(a ^ w);
}
// Same, with the accumulate form of v_bcnt_u32_b32 (D = popcount(S0) + S1) pinned: for
// callers that keep several independent chains themselves (the compiler otherwise emits
// bcnt(x, 0) plus a tree of v_add3, ~22 % more VALU instructions).
__device__ __forceinline__ int qnn_dot_bin_chain(uint32_t a, uint32_t w, int acc) {
    const uint32_t x = a ^ w;
    int r;
    asm("v_bcnt_u32_b32 %0, %1, %2" : "=v"(r) : "v"(x), "v"(acc));
    return r;
}
// 8 x (int4 * int4) + acc  -> v_dot8_i32_i4
__device__ __forceinline__ int qnn_dot_i4(uint32_t a, uint32_t w, int acc) {
    return __builtin_amdgcn_sdot8((int)a, (int)w, acc, false);
}
// 4 x (int8 * int8) + acc  -> v_dot4_i32_i8
__device__ __forceinline__ int qnn_dot_i8(uint32_t a, uint32_t w, int acc) {
    return __builtin_amdgcn_sdot4((int)a, (int)w, acc, false);
}

// ternary x ternary on (mask, sign) word pairs: popc(m) - 2 popc(m & (sa ^ sw)),  m = ma & mw
__device__ __forceinline__ int qnn_dot_t2(uint32_t ma, uint32_t sa, uint32_t mw, uint32_t sw, int acc) {
    const uint32_t m = ma & mw;
    return acc + __popc(m) - 2 * __popc(m & (sa ^ sw));
}

template <int STORE>
__device__ __forceinline__ int qnn_dot(uint32_t a, uint32_t w, int acc) {
    if constexpr (STORE == QNN_STORE_BIN) return qnn_dot_bin(a, w, acc);
    else if constexpr (STORE == QNN_STORE_I4) return qnn_dot_i4(a, w, acc);
    else return qnn_dot_i8(a, w, acc);
}

// ---- epilogue: acc -> float value in the reference's op order -------------------
__device__ __forceinline__ float qnn_epi_value(float v, int c, const EpiArgs& e) {
    // binary_layers.py:175-176: (o - (1 - 1/klm) * o) * klm, three float32 roundings ("faithful" mode only)
    if (e.trick_s != 0.0f) v = __fmul_rn(__fsub_rn(v, __fmul_rn(e.trick_c, v)), e.trick_s);
    if (e.bias) v = __fadd_rn(v, e.bias[c]);
    if (e.bn_inv) v = __fadd_rn(__fmul_rn(v, e.bn_inv[c]), e.bn_shift[c]);
    return v;
}
// residual merge of models/resnet.py:127-128: (x + y) * post_scale, float32, two roundings
__device__ __forceinline__ float qnn_epi_residual(float v, long q, int c, const EpiArgs& e) {
    if (!e.res) return v;
    float r;
    if (e.res_store == QNN_STORE_F32) {
        r = ((const float*)e.res)[q * e.res_cw + c];
    } else if (e.res_store == QNN_STORE_BIN) {
        const uint32_t w = ((const uint32_t*)e.res)[q * e.res_cw + (c >> 5)];
        r = ((w >> (c & 31)) & 1u) ? 1.0f : -1.0f;
    } else if (e.res_store == QNN_STORE_I4) {
        const uint32_t w = ((const uint32_t*)e.res)[q * e.res_cw + (c >> 3)];
        const int code = (int)(w << (28 - 4 * (c & 7))) >> 28;
        r = __fmul_rn((float)code, e.res_scale);
    } else {
        const uint32_t w = ((const uint32_t*)e.res)[q * e.res_cw + (c >> 2)];
        const int code = (int)(w << (24 - 8 * (c & 3))) >> 24;
        r = __fmul_rn((float)code, e.res_scale);
    }
    return __fmul_rn(__fadd_rn(r, v), e.post_scale);
}
// ---- QNN_STORE_U8 input: the affine map behind the exact integer sum (qnn_abi.h, qnn_conv2d_forward) ----
struct U8Affine {
    float A, B;
};
__device__ __forceinline__ U8Affine qnn_u8_affine(const EpiArgs& e, int c) {
    const double inv = e.bn_inv ? (double)e.bn_inv[c] : 1.0, shift = e.bn_inv ? (double)e.bn_shift[c] : 0.0;
    const double bias = e.bias ? (double)e.bias[c] : 0.0;
    const double m = e.fn == QNN_FN_QUANTIZED_TANH ? (double)e.act_m : 1.0;
    U8Affine a;
    a.A = (float)(inv * m / (double)e.scale);
    a.B = (float)((bias * inv + shift) * m);
    return a;
}
// t = fma(S, A, B) -> what is pooled: the integer code (quantized_tanh), +-1 (binary_tanh), or t itself
__device__ __forceinline__ float qnn_u8_value(float t, const EpiArgs& e) {
    if (e.fn == QNN_FN_BINARY_TANH) return t > 0x1p-24f ? 1.0f : -1.0f;
    if (e.fn == QNN_FN_QUANTIZED_TANH) return fminf(fmaxf(rintf(t), -e.act_m), e.act_m - 1.0f);
    return t;
}
// value -> stored code (BIN: 0/1; I4/I8: signed code) or float bits
__device__ __forceinline__ int qnn_epi_code(float v, const EpiArgs& e) {
    if (e.fn == QNN_FN_BINARY_TANH) {
        const int b = (int)qnn_binary_bit(v);
        return e.out_store == QNN_STORE_BIN ? b : 2 * b - 1;   // +-1 as a signed code
    }
    return (int)qnn_qact_code_f(e.fn, v, e.act_m);
}
#endif  // __HIPCC__

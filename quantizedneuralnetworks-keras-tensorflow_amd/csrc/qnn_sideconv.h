// What the depthwise, transposed and grouped convolutions (qnn_depthwise.hip, qnn_tconv.hip, qnn_gconv.hip) share: the weight
// quantiser, the common part of their handles with its prepack and free, the checks of their forward entries, and the
// device helpers of the streaming lane map (qnn_pool.hip and qnn_concat.hip take those from here too).  The host functions
// and the two weight kernels are in qnn_sideconv.hip; what differs between the entries -- geometry, limits, the int32
// bound, the operand images of the fast forms -- stays in their files.
#pragma once
#include <type_traits>

#include "qnn_common.h"

// ---- weights: binarize (binary_ops.py:54-64), quantize (quantized_ops.py:49-66), ternarize ---------------------------------
__device__ __forceinline__ float qnn_quantize_weight(float w, int wkind, float H, float m, float cutoff) {
    if (wkind == QNN_W_BINARY) return __fmul_rn(H, qnn_binary_tanh(__fdiv_rn(w, H)));
    if (wkind == QNN_W_QUANT) return qnn_quantized_tanh(w, m);
    if (wkind == QNN_W_TERNARY) {
        // ternary_ops.py:21-27: W/H > cutoff -> 1, W/H <= -cutoff -> -1, else 0; times H.
        // ("exact" mode: the straight-through W + (Wt - W) of ternary_ops.py:41 is taken as Wt.)
        const float u = __fdiv_rn(w, H);
        const float t = u > cutoff ? 1.0f : (u <= -cutoff ? -1.0f : 0.0f);
        return __fmul_rn(t, H);
    }
    return w;
}
// cutoff[0] = 0.7 * mean(|kernel / H|) over the n values (ternary_ops.py:15-30); one block, fixed order
void qnn_launch_tern_cutoff(const float* kernel, int n, float H, float* cutoff, hipStream_t s);

// ---- the common part of a handle --------------------------------------------------------------------------------------------
struct SideWeights {
    int wkind, wbits;
    float H;
    int store;
    int wshift;              // quantized value = code * 2^-wshift
    int xcw;                 // words per input pixel on the handle's packed store (F32: 0)
    float* d_wq;             // the kernel in Keras' own order, quantized values
    int32_t* d_wcode;        // the same order, integer codes value * 2^wshift (packed stores) or nullptr
    float* d_bias;           // [cout] or nullptr
    float* d_aux;            // ternary: the cutoff (1 float), else nullptr
};

// a HIP call of a prepack: QNN_OK, or the error text set and QNN_ENOMEM / QNN_EHIP.  The entry frees its handle once, where
// it sees the code.
int qnn_side_hip(hipError_t err, const char* what);
#define QNN_SIDE_HIP(expr)                                                     \
    do {                                                                       \
        const int _rc = qnn_side_hip((expr), #expr);                           \
        if (_rc != QNN_OK) return _rc;                                         \
    } while (0)

// validates (wkind, wbits, H, store) and writes them, with wshift, to *w
int qnn_side_weights_check(const char* who, int wkind, int wbits, float H, int store, SideWeights* w);
// d_wq, d_wcode (packed stores) and d_aux (ternary) allocated and filled from the n values of `kernel`, d_bias copied:
// cutoff, quantiser, bias copy, in this order on s
int qnn_side_quantize(SideWeights* w, const float* kernel, int n, const float* bias, int cout, hipStream_t s);
void qnn_side_free(SideWeights* w);

// ---- the forward entries ----------------------------------------------------------------------------------------------------
// The input's store against the handle's and the epilogue subset of these entries (no pooling, residual, fold, projection,
// identity trick or flags; `layer` names the entry in the pool message).  Writes xshift and the whole of *e.
int qnn_side_forward_check(const char* who, const SideWeights* w, int cout, int x_store, int x_bits, const qnn_epilogue_t* epi,
                           const char* layer, int* xshift, EpiArgs* e);
// The output-word bound, then N == 0 (*run = false with QNN_OK: no pointer is looked at), then null pointers and overlap.
int qnn_side_io_check(const char* who, int N, size_t owords, const void* x, size_t xbytes, const void* y, bool* run);
// "<op>_<store>" + route, the route only on the stores that have two forms (I4, I8)
void qnn_side_kernel_name(const char* op, int x_store, const char* route);

const char* store_name(int store);

// the store dispatch of a plain form: f(std::integral_constant<int, XS>()) with XS the input's store
template <class F>
void qnn_side_for_store(int x_store, F&& f) {
    if (x_store == QNN_STORE_F32) f(std::integral_constant<int, QNN_STORE_F32>());
    else if (x_store == QNN_STORE_BIN) f(std::integral_constant<int, QNN_STORE_BIN>());
    else if (x_store == QNN_STORE_T2) f(std::integral_constant<int, QNN_STORE_T2>());
    else if (x_store == QNN_STORE_I4) f(std::integral_constant<int, QNN_STORE_I4>());
    else f(std::integral_constant<int, QNN_STORE_I8>());
}

// the channel (0 .. 15 of the lane's 16) that byte j of an MFMA B operand carries: in order for int8; for int4 the order
// strip_widen leaves (even nibbles of a word, then odd ones)
__host__ __device__ inline int qnn_operand_channel(int store, int j) {
    if (store == QNN_STORE_I8) return j;
    const int wd = j >> 2, b = j & 3;
    return (wd >> 1) * 8 + 2 * b + (wd & 1);
}

// ---- V consecutive words of a lane ------------------------------------------------------------------------------------------
template <int V> struct Words;
template <> struct Words<1> { typedef uint32_t type; };
template <> struct Words<4> { typedef uint4 type; };

template <int V>
__device__ __forceinline__ void load_words(const uint32_t* p, uint32_t (&w)[V]) {
    const typename Words<V>::type v = *reinterpret_cast<const typename Words<V>::type*>(p);
    __builtin_memcpy(w, &v, sizeof(v));
}
template <int V>
__device__ __forceinline__ void store_words(uint32_t* p, const uint32_t (&w)[V]) {
    typename Words<V>::type v;
    __builtin_memcpy(&v, w, sizeof(v));
    *reinterpret_cast<typename Words<V>::type*>(p) = v;
}

// value behind the chain -> what a float32 output stores (k_conv_generic's order)
__device__ __forceinline__ float act_value(float v, const EpiArgs& e) {
    if (e.fn == QNN_FN_BINARY_TANH) return qnn_binary_tanh(v);
    if (qnn_is_qact(e.fn)) return qnn_qact(e.fn, v, e.act_m);
    if (e.fn == QNN_FN_LEAKY_RELU) return qnn_leaky_relu(v);
    return v;
}

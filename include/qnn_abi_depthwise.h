/*
 * qnn_abi_depthwise.h -- extension of the C ABI (qnn_abi.h, version 4): keras.layers.DepthwiseConv2D with float, binary,
 * quantized or ternary weights, on NHWC float32 tensors and on packed codes.  A handle type of its own and five entry
 * points; conventions, status codes, the QNN_STORE_* layouts and qnn_epilogue_t are those of qnn_abi.h.  An extension of
 * ABI 4 in a header of its own: qnn_abi.h, its symbol list, qnn_version(), qnn_weights_t and every existing struct are
 * what they were.
 *
 * Semantics.  The kernel is Keras' depthwise_kernel (kh, kw, C, M), M = depth_multiplier.  Output channel c * M + m reads
 * input channel c only: there is no reduction over channels.  Neighbouring taps are dil_h rows / dil_w columns apart;
 * output size and 'same' padding follow TensorFlow's rule on the effective window dil * (k - 1) + 1 (csrc/qnn_conv_geom.h).
 * A tap outside the image contributes 0 on every store, QNN_STORE_BIN included: the sum runs over the in-bounds taps.
 *   packed input   acc = the exact integer sum over the in-bounds taps of input code x weight code (BIN: +-1; T2: -1, 0,
 *                  +1),  v = (float)acc * 2^-(wshift + x_bits - 1)  (wshift = wbits - 1 for quantized weights, else 0;
 *                  x_bits - 1 = 0 for BIN / T2), exact: |acc| < 2^24;
 *   float32 input  a float64 accumulator starts at 0 and adds (double)x * (double)w per in-bounds tap in (ky, kx)
 *                  row-major order (every product is exact); it is rounded once to float32;
 * then the float32 chain of qnn_epilogue_t in the reference's order: + bias[c], * bn_inv[c] + bn_shift[c] (two roundings),
 * fn, store.
 */
#ifndef QNN_ABI_DEPTHWISE_H
#define QNN_ABI_DEPTHWISE_H

#include "qnn_abi.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct qnn_dw_weights qnn_dw_weights_t;   /* opaque prepacked depthwise kernel */

#define QNN_DW_MAX_WINDOW 7   /* kh, kw <= 7: QNN_EUNSUPPORTED beyond */

/*
 * Quantize + pack a depthwise kernel once.  wkind / wbits / H / store mean what they mean for qnn_prepack_weights, with
 * the same store rules (BIN: binary weights, H = 1; I4 / I8: quantized weights of wbits <= store, or binary / ternary
 * with H = 1; T2: ternary or binary with H = 1; F32: float32 inputs only).  The quantiser is applied elementwise to the
 * (kh, kw, C, M) kernel; the ternary cutoff 0.7 * mean|W / H| is taken over this whole kernel.  The mean is a float64
 * sum in a fixed TREE order (1024 strided partial sums, then halving), as qnn_prepack_weights forms it -- not the
 * sequential order of a numpy restatement: on arbitrary weights the float32 cutoff can differ from such a restatement in
 * its last bit, and a weight exactly at the cutoff can then ternarise differently.  The tests use kernels whose values are
 * multiples of 1/64, where every order gives the same sum.
 *   kernel : DEVICE, float32, Keras layout (kh, kw, C, M);  bias : DEVICE [C * M] or NULL.
 *   stride : 1 or 2 (square);  same_pad : 1 'same', 0 'valid';  dil_h, dil_w : 1 .. QNN_MAX_DILATION.
 * QNN_EINVAL: null kernel / out, sizes < 1, stride < 1, dilation < 1, an unknown wkind / store, weights that do not fit
 * the store, H <= 0.  QNN_EUNSUPPORTED: stride > 2, a window beyond QNN_DW_MAX_WINDOW, a dilation above QNN_MAX_DILATION,
 * dilation != 1 together with stride != 1.  Allocates device memory and launches on `stream`; a set-up call.
 */
int qnn_depthwise_prepack(int wkind, int wbits, float H, const float* kernel, int kh, int kw, int C,
                          int depth_multiplier, const float* bias, int stride, int same_pad, int dil_h, int dil_w,
                          int store, void* stream, qnn_dw_weights_t** out);
int qnn_depthwise_free(qnn_dw_weights_t* w);
/* the quantized kernel as float32 (kh, kw, C, M) into a DEVICE buffer (tests) */
int qnn_depthwise_dequant(const qnn_dw_weights_t* w, float* kernel_khkwCM, void* stream);
/* Output size on an H x W image; QNN_EINVAL for a null pointer or H, W < 1.  An empty output reports 0. */
int qnn_depthwise_out_hw(const qnn_dw_weights_t* w, int H, int W, int* Ho, int* Wo);
/*
 * y = epilogue(depthwise_conv(x)) for an N x H x W x C tensor x; y is N x Ho x Wo x (C * M).
 *   x_store  QNN_STORE_F32 (any handle), or the handle's packed store (BIN / I4 / I8 / T2 in the layouts of qnn_pack_f32);
 *            I4 / I8: 1 <= x_bits <= x_store.
 *   epi      bn_inv / bn_shift, and fn in {NONE, BINARY_TANH, QUANTIZED_TANH, QUANTIZED_RELU, QUANTIZED_LEAKYRELU};
 *            LEAKY_RELU with a float32 output only; out_store F32 / BIN / I4 / I8 under the act_bits <= out_store rules of
 *            qnn_abi.h.  The bias is the handle's.
 *   output   the bits of a packed pixel's last word beyond channel C * M - 1 are zero, whatever x holds in its spare bits.
 * Answers, all before the first HIP call.  QNN_EINVAL: a null pointer with N > 0, N < 0, H or W < 1, an x_store / x_bits
 * that does not fit the handle, an fn / out_store pair outside the rules, an empty output, y overlapping x.
 * QNN_EUNSUPPORTED (the message names the field): pool != 1, res, fold, proj, trick_s != 0, flags != 0, QNN_STORE_U8 /
 * _F32_IMAGE / _F32_UNIT as x_store, quantized_maxrelu / quantized_leakymaxrelu, 2^31 output words (float32: values) or
 * more.  N == 0 is QNN_OK without a launch (the pointers may then be null).
 * No allocation, no host read, no synchronisation: the call may be captured into a hipGraph.  qnn_last_kernel() names
 * depthwise_f32, depthwise_bin, depthwise_t2, depthwise_i4, depthwise_i8 (the 16-bit-lane form) or depthwise_i4_plain,
 * depthwise_i8_plain.  The 16-bit-lane form multiplies two channels per instruction in 16-bit lanes and runs where
 * depth_multiplier is 1, the window 3x3 at stride 1 without dilation, the store I4 / I8, out_store == x_store and
 *     kh * kw * 2^(x_bits - 1) * 2^wshift < 2^15,
 * which bounds every partial sum of the taps (|input code| <= 2^(x_bits-1), |weight code| <= 2^wshift); every other call
 * takes the plain form with 32-bit sums.  Results are bit-identical between the two.
 */
int qnn_depthwise_forward(const qnn_dw_weights_t* w, const void* x, int x_store, int x_bits,
                          int N, int H, int W, const qnn_epilogue_t* epi, void* y, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* QNN_ABI_DEPTHWISE_H */

/*
 * qnn_abi_tconv.h -- extension of the C ABI (qnn_abi.h, version 4): keras.layers.Conv2DTranspose with float, binary,
 * quantized or ternary weights, on NHWC float32 tensors and on packed codes.  A handle type of its own and five entry
 * points; conventions, status codes, the QNN_STORE_* layouts and qnn_epilogue_t are those of qnn_abi.h.  An extension of
 * ABI 4 in a header of its own: qnn_abi.h, its symbol list, qnn_version(), qnn_weights_t and every existing struct are
 * what they were.
 *
 * Semantics.  The kernel is Keras' kernel (kh, kw, Cout, Cin): filters come BEFORE input channels, unlike HWIO.  x is
 * N x H x W x Cin, y is N x Ho x Wo x Cout, strides are square, s >= 1.  y is the scatter
 *     full[n, iy * s + ky, ix * s + kx, f] += x[n, iy, ix, c] * w[ky, kx, f, c]
 * (no kernel flip: tf.nn.conv2d_transpose), where `full` has (H - 1) * s + kh rows, cut or zero-extended to TensorFlow's
 * output size.  Per axis (csrc/qnn_conv_geom.h, qnn_tconv_out_pad):
 *   'valid'  Ho = H * s + max(k - s, 0): rows [0, Ho) of `full`; rows beyond `full` (k < s) are sums over no tap;
 *   'same'   Ho = H * s; pad_total = max(k - s, 0), pad_before = pad_total / 2 (integer division): rows
 *            [pad_before, pad_before + Ho) of `full`, zero-extended where `full` is short.
 * So output row oy is reached by the taps ky == (oy + pad_before) mod s with iy = (oy + pad_before - ky) / s inside the
 * image.  An output pixel that no tap reaches has sum 0 on every store, QNN_STORE_BIN included, and still goes through
 * the epilogue.
 *   packed input   acc = the exact integer sum of input code x weight code (BIN: +-1; T2: -1, 0, +1) over the
 *                  contributing (tap, channel) pairs, in int32;  v = (float)acc * 2^-(wshift + x_bits - 1): the int32 sum
 *                  is converted to float32 (round to nearest even) and multiplied by the power of two in one float32
 *                  multiplication, as k_conv_generic does (wshift = wbits - 1 for quantized weights, else 0; x_bits - 1
 *                  = 0 for BIN / T2).  A call where int32 could overflow,
 *                      ceil(kh / s) * ceil(kw / s) * Cin * 2^(x_bits - 1) * 2^wshift >= 2^31,
 *                  is refused with QNN_EUNSUPPORTED before any HIP call;
 *   float32 input  a float64 accumulator starts at 0 and adds (double)x * (double)w over the contributing taps in
 *                  (ky, kx, c) row-major order; it is rounded once to float32;
 * then the float32 chain of qnn_epilogue_t in the reference's order (qnn_epi_value / qnn_epi_code): + bias[f],
 * * bn_inv[f] + bn_shift[f] (two roundings), fn, store.
 */
#ifndef QNN_ABI_TCONV_H
#define QNN_ABI_TCONV_H

#include "qnn_abi.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct qnn_tconv_weights qnn_tconv_weights_t;   /* opaque prepacked transposed-convolution kernel */

#define QNN_TC_MAX_WINDOW 8   /* kh, kw <= 8: QNN_EUNSUPPORTED beyond */
#define QNN_TC_MAX_STRIDE 4   /* stride 1 .. 4: QNN_EUNSUPPORTED beyond */

/*
 * Quantize + pack a transposed-convolution kernel once.  wkind / wbits / H / store mean what they mean for
 * qnn_prepack_weights, with the same store rules (BIN: binary weights, H = 1; I4 / I8: quantized weights of wbits <=
 * store, or binary / ternary with H = 1; T2: ternary or binary with H = 1; F32: float32 inputs only).  The quantiser is
 * applied elementwise to the (kh, kw, Cout, Cin) kernel; the ternary cutoff 0.7 * mean|W / H| is taken over this whole
 * kernel.  The mean is a float64 sum in a fixed TREE order (1024 strided partial sums, then halving), as
 * qnn_prepack_weights forms it -- not the sequential order of a numpy restatement: on arbitrary weights the float32
 * cutoff can differ from such a restatement in its last bit, and a weight exactly at the cutoff can then ternarise
 * differently.  The tests use kernels whose values are multiples of 1/64, where every order gives the same sum.
 *   kernel : DEVICE, float32, Keras layout (kh, kw, Cout, Cin);  bias : DEVICE [Cout] or NULL.
 *   stride : 1 .. QNN_TC_MAX_STRIDE (square);  same_pad : 1 'same', 0 'valid'.
 * QNN_EINVAL: null kernel / out, sizes < 1, stride < 1, an unknown wkind / store, weights that do not fit the store,
 * H <= 0.  QNN_EUNSUPPORTED (the message names the field): stride above QNN_TC_MAX_STRIDE, kh or kw above
 * QNN_TC_MAX_WINDOW.  Allocates device memory and launches on `stream`; a set-up call.  For the shapes of the
 * matrix-pipe form (below) the filters are also laid out per sub-pixel phase and tap in MFMA operand order here.
 */
int qnn_tconv_prepack(int wkind, int wbits, float H, const float* kernel, int kh, int kw, int Cout, int Cin,
                      const float* bias, int stride, int same_pad, int store, void* stream, qnn_tconv_weights_t** out);
int qnn_tconv_free(qnn_tconv_weights_t* w);
/* the quantized kernel as float32 (kh, kw, Cout, Cin) into a DEVICE buffer (tests) */
int qnn_tconv_dequant(const qnn_tconv_weights_t* w, float* kernel_khkwFC, void* stream);
/* Output size on an H x W image; QNN_EINVAL for a null pointer or H, W < 1.  No device call. */
int qnn_tconv_out_hw(const qnn_tconv_weights_t* w, int H, int W, int* Ho, int* Wo);
/*
 * y = epilogue(conv2d_transpose(x)) for an N x H x W x Cin tensor x; y is N x Ho x Wo x Cout.
 *   x_store  QNN_STORE_F32 (any handle), or the handle's packed store (BIN / I4 / I8 / T2 in the layouts of qnn_pack_f32);
 *            I4 / I8: 1 <= x_bits <= x_store.
 *   epi      bn_inv / bn_shift, and fn in {NONE, BINARY_TANH, QUANTIZED_TANH, QUANTIZED_RELU, QUANTIZED_LEAKYRELU};
 *            LEAKY_RELU with a float32 output only; out_store F32 / BIN / I4 / I8 under the act_bits <= out_store rules of
 *            qnn_abi.h.  The bias is the handle's.
 *   output   the bits of a packed pixel's last word beyond channel Cout - 1 are zero, whatever x holds in its spare bits.
 * Answers, all before the first HIP call.  QNN_EINVAL: a null pointer with N > 0, N < 0, H or W < 1, an x_store / x_bits
 * that does not fit the handle, an fn / out_store pair outside the rules, y overlapping x.  QNN_EUNSUPPORTED (the message
 * names the field): pool != 1, res, fold, proj, trick_s != 0, flags != 0, QNN_STORE_U8 / _F32_IMAGE / _F32_UNIT as
 * x_store, quantized_maxrelu / quantized_leakymaxrelu, 2^31 output words (float32: values) or more, the int32 bound
 * above.  N == 0 is QNN_OK without a launch (the pointers may then be null).
 * No allocation, no host read, no synchronisation: the call may be captured into a hipGraph.  qnn_last_kernel() names
 * tconv_f32, tconv_bin, tconv_t2, tconv_i4_plain, tconv_i8_plain (the plain form: a gather, one lane per group of output
 * words) or tconv_i4_mfma, tconv_i8_mfma (the matrix-pipe form on v_mfma_i32_16x16x64_i8).  The matrix-pipe form runs
 * where ALL of
 *     stride 2, kh == kw in {2, 3, 4} (either padding), x_store I4 or I8 and out_store == x_store,
 *     Cin a multiple of 64 and at most 16384, Cout a multiple of 16,
 *     both pointers 16-byte aligned, one input image (H * W * Cin codes as stored) below 2^31 bytes
 * hold; every other call takes the plain form.  Results are bit-identical between the two.
 */
int qnn_tconv_forward(const qnn_tconv_weights_t* w, const void* x, int x_store, int x_bits, int N, int H, int W,
                      const qnn_epilogue_t* epi, void* y, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* QNN_ABI_TCONV_H */

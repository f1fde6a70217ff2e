/*
 * qnn_abi_gconv.h -- extension of the C ABI (qnn_abi.h, version 4): the grouped convolution keras.layers.Conv2D(...,
 * groups=g) with float, binary, quantized or ternary weights, on NHWC float32 tensors and on packed codes.  A handle type
 * of its own and five entry points; conventions, status codes, the QNN_STORE_* layouts and qnn_epilogue_t are those of
 * qnn_abi.h.  An extension of ABI 4 in a header of its own: qnn_abi.h, its symbol list, qnn_version(), qnn_weights_t and
 * every existing struct are what they were.
 *
 * Semantics.  The kernel is Keras' kernel (kh, kw, Cin / g, Cout).  With Cg = Cin / g and Fg = Cout / g, filter f belongs
 * to group grp = f / Fg and reads the input channels [grp * Cg, (grp + 1) * Cg) only; kernel[ky, kx, c, f] meets input
 * channel grp * Cg + c.  x is N x H x W x Cin, y is N x Ho x Wo x Cout.  g = 1 is the ordinary convolution, g = Cin the
 * depthwise one with the (kh, kw, 1, C * M) <-> (kh, kw, C, M) reshape.  Neighbouring taps are dil_h rows / dil_w columns
 * apart; output size and 'same' padding follow TensorFlow's rule on the effective window dil * (k - 1) + 1
 * (csrc/qnn_conv_geom.h).  A tap outside the image contributes 0 on every store, QNN_STORE_BIN included: the sum runs
 * over the in-bounds taps.
 *   packed input   acc = the exact int32 sum of input code x weight code (BIN: +-1; T2: -1, 0, +1) over the in-bounds taps
 *                  and the group's Cg channels;  v = (float)acc * 2^-(wshift + x_bits - 1): the int32 sum is converted to
 *                  float32 (round to nearest even) and multiplied by the power of two in one float32 multiplication, as
 *                  k_conv_generic and qnn_tconv_forward do (wshift = wbits - 1 for quantized weights, else 0; x_bits - 1
 *                  = 0 for BIN / T2).  A call where int32 could overflow,
 *                      kh * kw * Cg * 2^(x_bits - 1) * 2^wshift >= 2^31,
 *                  is refused with QNN_EUNSUPPORTED before any HIP call;
 *   float32 input  a float64 accumulator starts at 0 and adds (double)x * (double)w over the in-bounds taps and the
 *                  group's channels in (ky, kx, c) row-major order; it is rounded once to float32;
 * then the float32 chain of qnn_epilogue_t in the reference's order (qnn_epi_value / qnn_epi_code): + bias[f],
 * * bn_inv[f] + bn_shift[f] (two roundings), fn, store.
 */
#ifndef QNN_ABI_GCONV_H
#define QNN_ABI_GCONV_H

#include "qnn_abi.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct qnn_gconv_weights qnn_gconv_weights_t;   /* opaque prepacked grouped-convolution kernel */

#define QNN_GC_MAX_WINDOW 7   /* kh, kw <= 7: QNN_EUNSUPPORTED beyond */

/*
 * Quantize + pack a grouped kernel once.  wkind / wbits / H / store mean what they mean for qnn_prepack_weights, with
 * the same store rules as qnn_depthwise_prepack (BIN: binary weights, H = 1; I4 / I8: quantized weights of wbits <=
 * store, or binary / ternary with H = 1; T2: ternary or binary with H = 1; F32: float32 inputs only).  The quantiser is
 * applied elementwise to the (kh, kw, Cin / g, Cout) kernel; the ternary cutoff 0.7 * mean|W / H| is taken over this
 * whole kernel (NOT over a block-diagonal expansion, whose structural zeros would lower the mean).  The mean is a float64
 * sum in a fixed TREE order (1024 strided partial sums, then halving), as qnn_prepack_weights forms it -- not the
 * sequential order of a numpy restatement: on arbitrary weights the float32 cutoff can differ from such a restatement in
 * its last bit, and a weight exactly at the cutoff can then ternarise differently.  The tests use kernels whose values are
 * multiples of 1/64, where every order gives the same sum.
 *   kernel : DEVICE, float32, Keras layout (kh, kw, Cin / groups, Cout);  bias : DEVICE [Cout] or NULL.
 *   groups : 1 .. Cin, dividing Cin and Cout.
 *   stride : 1 or 2 (square);  same_pad : 1 'same', 0 'valid';  dil_h, dil_w : 1 .. QNN_MAX_DILATION, with stride 1 only.
 * QNN_EINVAL: null kernel / out, sizes < 1 (kh, kw, Cin, Cout, groups), stride < 1, dilation < 1, Cin % groups != 0 or
 * Cout % groups != 0, an unknown wkind / store, weights that do not fit the store, H <= 0.  QNN_EUNSUPPORTED (the message
 * names the field): stride > 2, kh or kw above QNN_GC_MAX_WINDOW, a dilation above QNN_MAX_DILATION, dilation != 1
 * together with stride != 1, a kernel of kh * kw * (Cin / groups) * Cout >= 2^30 values, packed filter rows (kh * kw * Cout
 * rows of as many words as one group's channels span in an input pixel) of 2^31 words or more.  Allocates device memory
 * and launches on `stream`; a set-up call.  For the shapes of the matrix-pipe form (below) the filters are also laid out
 * in MFMA operand order per (filter tile, K-step) here.
 */
int qnn_gconv_prepack(int wkind, int wbits, float H, const float* kernel, int kh, int kw, int Cin, int Cout, int groups,
                      const float* bias, int stride, int same_pad, int dil_h, int dil_w, int store, void* stream,
                      qnn_gconv_weights_t** out);
int qnn_gconv_free(qnn_gconv_weights_t* w);
/* the quantized kernel as float32 (kh, kw, Cin / groups, Cout) into a DEVICE buffer (tests) */
int qnn_gconv_dequant(const qnn_gconv_weights_t* w, float* kernel_khkwCF, void* stream);
/* Output size on an H x W image; QNN_EINVAL for a null pointer or H, W < 1.  An empty output reports 0.  No device call. */
int qnn_gconv_out_hw(const qnn_gconv_weights_t* w, int H, int W, int* Ho, int* Wo);
/*
 * y = epilogue(grouped_conv(x)) for an N x H x W x Cin tensor x; y is N x Ho x Wo x Cout.
 *   x_store  QNN_STORE_F32 (any handle), or the handle's packed store (BIN / I4 / I8 / T2 in the layouts of qnn_pack_f32);
 *            I4 / I8: 1 <= x_bits <= x_store.
 *   epi      bn_inv / bn_shift, and fn in {NONE, BINARY_TANH, QUANTIZED_TANH, QUANTIZED_RELU, QUANTIZED_LEAKYRELU};
 *            LEAKY_RELU with a float32 output only; out_store F32 / BIN / I4 / I8 under the act_bits <= out_store rules of
 *            qnn_abi.h.  The bias is the handle's.
 *   output   the bits of a packed pixel's last word beyond channel Cout - 1 are zero, whatever x holds in its spare bits.
 * Answers, all before the first HIP call.  QNN_EINVAL: a null pointer with N > 0, N < 0, H or W < 1, an x_store / x_bits
 * that does not fit the handle, an fn / out_store pair outside the rules, an empty output, y overlapping x.
 * QNN_EUNSUPPORTED (the message names the field): pool != 1, res, fold, proj, trick_s != 0, flags != 0, QNN_STORE_U8 /
 * _F32_IMAGE / _F32_UNIT as x_store, quantized_maxrelu / quantized_leakymaxrelu, 2^31 output words (float32: values) or
 * more, the int32 bound above.  N == 0 is QNN_OK without a launch (the pointers may then be null).
 * No allocation, no host read, no synchronisation: the call may be captured into a hipGraph.  qnn_last_kernel() names
 * gconv_f32, gconv_bin, gconv_t2, gconv_i4_plain, gconv_i8_plain (the plain form: a gather, one lane per group of output
 * words; group boundaries need not fall on word boundaries) or gconv_i4_mfma, gconv_i8_mfma (the matrix-pipe form on
 * v_mfma_i32_16x16x64_i8).  With Cg = Cin / g, Fg = Cout / g, t = 1 where Fg % 16 == 0 and t = 16 / Fg otherwise, and
 * R = t * Cg (the run of input channels that 16 consecutive filters read; csrc/qnn_gconv_plan.h), the matrix-pipe form
 * runs where ALL of
 *     store I4 or I8, x_store == store and out_store == x_store,
 *     Cout % 16 == 0,  Fg % 16 == 0 or 16 % Fg == 0,  R % 16 == 0,  R <= 16384,
 *     both pointers 16-byte aligned, one input image (H * W * Cin codes as stored) below 2^31 bytes
 *     (and the prepacked operand image, (Cout / 16) * ceil(kh * kw * R / 64) KiB, below 2^31 bytes)
 * hold, for every window, stride, dilation and padding the entry accepts; every other call takes the plain form.  Results
 * are bit-identical between the two.
 */
int qnn_gconv_forward(const qnn_gconv_weights_t* w, const void* x, int x_store, int x_bits, int N, int H, int W,
                      const qnn_epilogue_t* epi, void* y, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* QNN_ABI_GCONV_H */

/*
 * qnn_abi_scaled.h -- extension of the C ABI (qnn_abi.h, version 4): the activations of qnn_abi_maxact.h carried as packed
 * codes plus a device-resident scale.  Three entry points; conventions and status codes are those of qnn_abi.h.  An
 * extension of ABI 4 in a header of its own: qnn_abi.h, its symbol list, qnn_version() and qnn_epilogue_t are what they were.
 *
 * Why.  quantized_maxrelu / quantized_leakymaxrelu give y = code * P / m with m = 2^(nb-1) and P = the smallest power of two
 * >= M, the maximum of the whole batch tensor (qnn_abi_maxact.h).  P is known on the device only, so the values are not on
 * the fixed grid k / m the packed stores assume.  But the whole tensor shares ONE P, and P is a power of two: it commutes
 * with every float32 rounding, so conv(P k / m, W) = P conv(k / m, W) exactly.  A consumer therefore needs the codes and
 * its ordinary output scale 2^-(wshift + x_bits - 1) multiplied by P, read on the device from the 16-byte workspace word
 * qnn_maxact_max_f32 left there.  Nothing is read back to the host.
 *
 * Contract of the scaled consumers.  The packed input's value is code * P / 2^(x_bits-1).  The entries take a layer only if
 * K * 2^(x_bits-1) * 2^(wbits-1) <= 2^24 (QNN_EUNSUPPORTED beyond, as the QNN_STORE_U8 entry refuses sums past 2^24).  The
 * result is then the EXACT integer sum of code x weight-code products, as a float32 without rounding, times scale * P (both
 * powers of two: the product is exact), then the epilogue of qnn_conv2d_forward as it is: identity trick, bias, BN, float32
 * residual with post_scale, per-value fn.  For a word outside the exact range of qnn_abi_maxact.h (no positive value, M <=
 * 2^-65, M > 2^64, inf) the effective scale is quiet NaN, hence so is every pre-activation value: what the float32 route
 * computes from the all-NaN activation qnn_maxact_apply_f32 writes in that case.
 *
 * Exactness against the float32 route.  qnn_conv2d_forward on the float32 tensor y (QNN_STORE_F32 input) sums with a
 * float32 fmaf chain; every product and partial sum is then an integer times P / (m 2^wshift), so the chain is exact -- and
 * equal to this header's result bit for bit -- whenever every partial sum fits 24 bits:
 *     K * 2^(x_bits-1) * 2^(wbits-1) <= 2^24,   K = kh * kw * cin (a dense layer: its input width), wbits = 1 for binary
 *     and ternary weights.
 * Beyond that bound the chain may round and the int32 -> float32 conversion of the sum could too, so the scaled entries
 * refuse the layer: it stays on the float32 route.
 *
 * Kernels.  The scaled entries dispatch through the route list of qnn_conv2d_forward with one more requirement
 * (CAP_XSCALE); the routes that list it are route_dense (k_dense_packed / k_dense_packed_split), qnn_route_gemm (int4 or int8
 * codes, input channels a multiple of 64, filters a multiple of 128, no residual: k_conv_mfma16_scaled, the 256 x 128 and
 * 256 x 256 tiles on the matrix pipe) and route_generic
 * (k_conv_generic).  Every other route is skipped for a scaled call; the strip kernels store packed codes only and have no
 * float32 output form (DESIGN.md 3.4 has the reason per kernel).  Calls of the unscaled entries run the kernels they ran.
 */
#ifndef QNN_ABI_SCALED_H
#define QNN_ABI_SCALED_H

#include "qnn_abi.h"
#include "qnn_abi_maxact.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * Pass 2 of qnn_abi_maxact.h as a pack: with M read on the device from workspace16 (as written by qnn_maxact_max_f32 and,
 * under batch sharding, all-reduced by the caller), code = clip(rint(L(x) * m / P), lo, m - 1) by the rule of
 * qnn_abi_maxact.h, written in the layout of qnn_pack_f32: `pixels` rows of ceil(channels / per_word) 32-bit words,
 * store = QNN_STORE_I4 (8 codes per word) or QNN_STORE_I8 (4), codes sign-extended into their field, the spare fields of a
 * pixel's last word zero.  nb in 2 .. 8 and nb <= the store's field width (a 4-bit activation may go into QNN_STORE_I8 to
 * meet 8-bit weights).  fn = QNN_FN_QUANTIZED_MAXRELU or QNN_FN_QUANTIZED_LEAKYMAXRELU, anything else is QNN_EINVAL.
 * y_or_null != NULL: the same pass also writes the float32 result code * P / m to y, bit for bit what
 * qnn_maxact_apply_f32 writes (for consumers that need float32: a shortcut add, a float-weight layer); y == x allowed.
 * M outside the exact range: every code is 0 and y (if given) is quiet NaN everywhere.
 * pixels == 0 launches nothing.  pixels * words >= 2^31 is QNN_EUNSUPPORTED.  No host read, no synchronisation; the call
 * may be captured into a hipGraph.
 */
int qnn_maxact_pack_f32(const float* x, void* packed, float* y_or_null, size_t pixels, int channels, int fn, int nb,
                        int store, const void* workspace16, void* stream);

/*
 * qnn_conv2d_forward / qnn_dense_forward on packed codes whose value is code * P / 2^(x_bits-1), P from the word in
 * x_scale16 (the workspace16 of qnn_maxact_pack_f32, unchanged since).  Required: x_store = QNN_STORE_I4 or QNN_STORE_I8
 * (QNN_EUNSUPPORTED otherwise), epi->out_store == QNN_STORE_F32, epi->fold == NULL, epi->proj == NULL, epi->pool == 1
 * (QNN_EUNSUPPORTED), x_scale16 != NULL (QNN_EINVAL); every message names the entry.  The output is float32: the next
 * activation of such a network is batch-scaled again and needs this output's maximum.
 */
int qnn_conv2d_forward_scaled(const qnn_weights_t* w, const void* x, int x_store, int x_bits, int N, int H, int W,
                              const qnn_epilogue_t* epi, const void* x_scale16, void* y, void* stream);
int qnn_dense_forward_scaled(const qnn_weights_t* w, const void* x, int x_store, int x_bits, int N,
                             const qnn_epilogue_t* epi, const void* x_scale16, void* y, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* QNN_ABI_SCALED_H */

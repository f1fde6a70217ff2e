/*
 * qnn_abi_maxact.h -- extension of the C ABI (qnn_abi.h, version 4): quantized_maxrelu and quantized_leakymaxrelu
 * (layers/quantized_ops.py:125-171), the two quantised activations whose scale is the maximum of the whole batch tensor.
 * Two QNN_FN_* codes and three entry points; conventions and status codes are those of qnn_abi.h.  An extension of ABI 4
 * in a header of its own: qnn_abi.h, its symbol list and qnn_version() are what they were.
 *
 * Contract, all float32.  r(x) = max(x, 0);  L(x) = x for x >= 0, float32(0.1) * x (one rounding) for x < 0 -- the
 * reference's relu(x) - 0.1 relu(-x), as QNN_FN_QUANTIZED_LEAKYRELU computes it;  m = 2^(nb-1), nb in 2 .. 24.
 *   M = the maximum of r(x) over the tensor (for leakymaxrelu max L(x) = max r(x) whenever a value is positive); under
 *       batch sharding the maximum over all shards' valid rows (the caller all-reduces the workspace word, below).
 *   P = the smallest power of two >= M, read from M's exponent and mantissa bits: 2^e with e = exponent(M), plus one when
 *       the mantissa is not zero.  No logarithm is taken.
 *   QNN_FN_QUANTIZED_MAXRELU:       code = clip(rint(x    * (m / P)), 0,  m - 1),  y = code * (P / m)
 *   QNN_FN_QUANTIZED_LEAKYMAXRELU:  code = clip(rint(L(x) * (m / P)), -m, m - 1),  y = code * (P / m)
 *   rint rounds half to even; m / P and P / m are powers of two, so rint is the only rounding after L.  A zero result
 *   is +0.
 *
 * Range of M.  Exact whenever P = 2^e has -64 <= e <= 64, that is for 2^-65 < M <= 2^64 (2^-64 <= M <= 2^64 included).
 * For every other M -- no positive value at all (M <= 0: the reference takes the logarithm of zero or of a negative
 * number), M <= 2^-65, M > 2^64, +inf -- the apply entry writes quiet NaN (0x7FC00000) to EVERY output element; it does
 * not read the word on the host, synchronise or fail.  Non-finite inputs are outside the contract (a NaN is ignored by
 * the maximum and comes out as the lower clip edge); they cannot fault.
 *
 * Documented deviation from the reference.  The reference computes the exponent as ceil(log(M) / log(2)) in float32.
 * Where M is an exact power of two, or lies within 16 ulp above one, that quotient may land on either side of the
 * integer, depending on the platform's float32 log: its scale is then 2x or 1/2x the one above (with numpy's float32 log,
 * 23 of the 254 normal powers of two, e.g. log(2^13) / log(2) = 13.000001, and up to 12 ulp above a power of two).
 * Everywhere else the two agree.  This library always takes the exact e.
 *
 * Every other entry that takes a QNN_FN_* code -- the conv, dense, pack and fold entries of qnn_abi.h and
 * qnn_quantized_act_f32 -- answers QNN_EUNSUPPORTED for these two codes: without the batch-wide maximum they are no
 * per-value function, and the values P k / m are not on the fixed grid k / m the packed stores assume.
 */
#ifndef QNN_ABI_MAXACT_H
#define QNN_ABI_MAXACT_H

#include "qnn_abi.h"

#ifdef __cplusplus
extern "C" {
#endif

#define QNN_FN_QUANTIZED_MAXRELU       8   /* quantized_ops.py:125-143 */
#define QNN_FN_QUANTIZED_LEAKYMAXRELU  9   /* quantized_ops.py:145-171 at alpha = float32(0.1) */

/*
 * Pass 1: leaves the bit pattern of M (a non-negative float32; bit order = value order) in the first 32-bit word of
 * the 16-byte device buffer `workspace16`; the other 12 bytes are zeroed.  The buffer is cleared by a memset node, so the
 * call may be captured into a hipGraph.  n == 0 clears the word and launches no kernel (an empty shard).
 * For a batch sharded over processes: all-reduce the word with MAX (as uint32 or as float32) before pass 2.
 */
int qnn_maxact_max_f32(const float* x, size_t n, void* workspace16, void* stream);

/*
 * Pass 2: y = fn(x) on n values at nb bits with the M found in workspace16 (read on the device).
 * fn = QNN_FN_QUANTIZED_MAXRELU or QNN_FN_QUANTIZED_LEAKYMAXRELU, anything else is QNN_EINVAL; nb in 2 .. 24.
 * x == y allowed.  n == 0 launches nothing.
 */
int qnn_maxact_apply_f32(const float* x, float* y, size_t n, int fn, int nb, const void* workspace16, void* stream);

/* The two passes in sequence on the same n values.  n == 0 returns QNN_OK and launches nothing.  x == y allowed. */
int qnn_quantized_maxact_f32(const float* x, float* y, size_t n, int fn, int nb, void* workspace16, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* QNN_ABI_MAXACT_H */

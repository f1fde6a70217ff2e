/*
 * qnn_abi_merge.h -- extension of the C ABI (qnn_abi.h, version 4): Keras' element-wise merge layers Add, Subtract,
 * Multiply, Average, Maximum and Minimum (keras/layers/merge.py) on float32 tensors and on packed codes.  One descriptor
 * and two entry points; conventions, status codes and the QNN_STORE_* layouts are those of qnn_abi.h.  An extension of
 * ABI 4 in a header of its own: qnn_abi.h, its symbol list, qnn_version() and qnn_epilogue_t are what they were.
 *
 * Semantics.  The n inputs share one store, one code width and one shape: `pixels` rows of `channels` values in the
 * layout qnn_pack_f32 writes (float32: rows of `channels` values).  n is 2 .. QNN_MERGE_MAX, exactly 2 for _SUB.
 *
 * float32 in, float32 out -- Keras' own chain: out = x[0]; out = out o x[i], left to right, one float32 rounding per
 * step.  _AVG is the sum chain followed by ONE correctly rounded division by (float)n (not a multiplication by a
 * reciprocal).  _MAX / _MIN give NaN where either operand is NaN (tf.maximum, np.maximum; the first NaN of the chain is
 * handed on); of two zeros of opposite sign either may be returned.
 *
 * Packed in, packed out (same store, same bits) -- no arithmetic on values, only on codes:
 *   _MAX / _MIN   BIN       OR / AND of the words
 *   _MAX / _MIN   I4, I8    signed maximum / minimum per field
 *   _MAX / _MIN   T2        maximum / minimum of the values -1, 0, +1 as logic on the (mask, sign) pair; a sign bit under a
 *                           clear mask bit never reaches the result
 *   _MUL          BIN       XNOR of the words
 *   _MUL          T2        mask = AND of the masks; the product is positive where the signs agree: the sign plane holds
 *                           "the value is +1" (qnn_pack_f32), so sign = NOT (XOR of the signs) under that mask
 * The bits of a row's last word (T2: last word pair) beyond `channels` are zero in y, whatever the inputs hold there.
 *
 * Packed in, float32 out -- _ADD, _SUB, _AVG on BIN / I4 / I8 / T2 and _MUL on I4 / I8: every code is decoded in
 * registers (code / 2^(x_bits - 1); BIN: +-1; T2: the value) and the values are combined by the float32 chain above.
 * They are small dyadic numbers, so every step before _AVG's division is exact and the result is bit-identical to
 * qnn_unpack_f32 followed by the float32 form.
 */
#ifndef QNN_ABI_MERGE_H
#define QNN_ABI_MERGE_H

#include "qnn_abi.h"

#ifdef __cplusplus
extern "C" {
#endif

#define QNN_MERGE_MAX 8


/* The ops.  Maximum / Minimum are spelled out: QNN_MERGE_MAX is the input count above. */
enum {
    QNN_MERGE_ADD = 0,
    QNN_MERGE_SUB = 1,
    QNN_MERGE_MUL = 2,
    QNN_MERGE_AVG = 3,
    QNN_MERGE_MAXIMUM = 4,
    QNN_MERGE_MINIMUM = 5
};

typedef struct qnn_merge {
    int32_t n;                           /* inputs: 2 .. QNN_MERGE_MAX (QNN_MERGE_SUB: exactly 2) */
    int32_t op;                          /* QNN_MERGE_*                                            */
    const void* x[QNN_MERGE_MAX];        /* device pointers of the n inputs, ignored beyond        */
} qnn_merge_t;

/*
 * The store y gets for `op` on inputs of `store` (the table above): `store` itself for the packed-out forms and for
 * float32, QNN_STORE_F32 for the float32-out forms; QNN_EINVAL for an op outside the enum or a store other than
 * QNN_STORE_F32 / _BIN / _T2 / _I4 / _I8.  No device call.
 */
int qnn_merge_out_store(int op, int store);

/*
 * y = merge(x[0], ..., x[n-1]).
 *   store, x_bits   of every input; for _I4 / _I8 the codes are signed x_bits-bit values, 1 <= x_bits <= store (checked);
 *                   x_bits is ignored for the other stores.
 *   out_store       must be qnn_merge_out_store(op, store).  y is then `pixels` rows of qnn_pack_f32's words for `channels`
 *                   channels at x_bits, or of `channels` float32 values.
 * Answers, all before the first HIP call.  QNN_EINVAL: a null descriptor, n or op out of range, _SUB with n != 2, another
 * store, x_bits that does not fit, channels < 1, an out_store that differs from the table, a null pointer (pixels > 0), y
 * overlapping an input.  QNN_EUNSUPPORTED: pixels x (words of an input row, or values of a float32 row of x or y) >= 2^31.
 * pixels == 0 is QNN_OK without a launch (the pointers may then be null).  The descriptor is read during the call only
 * and reaches the kernel by value: no allocation, no host read, no synchronisation, so the call may be captured into a
 * hipGraph.  qnn_last_kernel() names merge_f32; merge_bin, merge_i4, merge_i8, merge_t2 (codes out); merge_bin_f32,
 * merge_i4_f32, merge_i8_f32, merge_t2_f32 (float32 out).
 */
int qnn_merge_forward(const qnn_merge_t* m, int store, int x_bits, size_t pixels, int channels, int out_store, void* y,
                      void* stream);

#ifdef __cplusplus
}
#endif
#endif /* QNN_ABI_MERGE_H */

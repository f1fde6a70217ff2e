/*
 * qnn_abi_pool.h -- extension of the C ABI (qnn_abi.h, version 4): Keras' MaxPooling2D / AveragePooling2D with
 * pool_size, strides and padding, and through them GlobalMaxPooling2D / GlobalAveragePooling2D, on float32 tensors and
 * on packed codes.  One descriptor and two entry points; conventions, status codes and the QNN_STORE_* layouts are those
 * of qnn_abi.h.  An extension of ABI 4 in a header of its own: qnn_abi.h, its symbol list and qnn_version() are what
 * they were.  qnn_avgpool_packed_f32 (the size-only average of qnn_abi.h) is untouched.
 *
 * Semantics (Keras 2.1.3 on TensorFlow, NHWC).  Window (ph, pw), strides (sh, sw), padding 'valid' (same_pad = 0) or
 * 'same' (1).  Per axis, with k the window, s the stride and h the image size:
 *   output size   'same': ceil(h / s);  'valid': (h - k) / s + 1, which needs k <= h -- the convolution's rule at
 *                 dilation 1 (csrc/qnn_conv_geom.h);
 *   padding       pad_total = max((out - 1) s + k - h, 0), pad_before = pad_total / 2, the odd cell goes behind; output
 *                 cell o covers the input cells o s - pad_before .. o s - pad_before + k - 1 that lie inside the image;
 *   max           the maximum over the in-bounds cells of the window: padding never takes part (no value stands in for it);
 *   avg           the sum over the in-bounds cells divided by the NUMBER OF IN-BOUNDS CELLS (tf.nn.avg_pool does not
 *                 count padding).  Packed input: the exact integer sum of the codes, then
 *                 fdiv_rn(fmul_rn((float)sum, 2^-(x_bits-1)), (float)count) -- the rounding of qnn_avgpool_packed_f32
 *                 (QNN_STORE_BIN: codes +-1, no scaling).  float32 input: the window summed in float64 in row order (rows
 *                 outer, columns inner), rounded once to float32, divided in float32 by (float)count;
 *   global        the window is the whole image under 'valid': an N x 1 x 1 x C result.
 * Under these rules every window holds at least one in-bounds cell.
 */
#ifndef QNN_ABI_POOL_H
#define QNN_ABI_POOL_H

#include "qnn_abi.h"

#ifdef __cplusplus
extern "C" {
#endif

#define QNN_POOL_MAX 0
#define QNN_POOL_AVG 1

typedef struct qnn_pool2d {
    int32_t mode;            /* QNN_POOL_MAX | QNN_POOL_AVG */
    int32_t ph, pw;          /* window rows, columns: >= 1  */
    int32_t sh, sw;          /* strides: >= 1               */
    int32_t same_pad;        /* 0 'valid', 1 'same'         */
} qnn_pool2d_t;

/*
 * Output size of qnn_pool2d_forward on an H x W image.  QNN_EINVAL where that call would answer QNN_EINVAL for the
 * geometry: a null pointer, H or W < 1, a window or stride < 1, a mode or same_pad outside the values above, 'valid' with
 * a window larger than the image.  Touches no device.
 */
int qnn_pool2d_out_hw(int H, int W, const qnn_pool2d_t* p, int* Ho, int* Wo);

/*
 * y = pool(x) for an N x H x W x C tensor x.
 *   x_store  QNN_STORE_F32, or QNN_STORE_BIN / _I4 / _I8 in the layout qnn_pack_f32 writes; for _I4 / _I8 the codes are
 *            signed x_bits-bit values, 1 <= x_bits <= x_store (x_bits is ignored for the other two).
 *            QNN_STORE_T2 answers QNN_EUNSUPPORTED (unpack, pool, pack); every other store is QNN_EINVAL.
 *   max      y_store == x_store: codes go to codes at the same x_bits (the maximum of grid codes is a grid code), in the
 *            layout qnn_pack_f32 writes -- the bits of a pixel's last word beyond channel C - 1 are zero, whatever the
 *            input holds there -- so y can be handed to every entry that takes a packed tensor.  float32 goes to float32.
 *   avg      y_store == QNN_STORE_F32 only: averages leave the grid.
 * x and y must not overlap.  Everything is checked before the first HIP call; N == 0 is QNN_OK without a launch (the
 * pointers may then be null).  N x Ho x Wo x (words, or channels for float32, per pixel) must stay below 2^31:
 * QNN_EUNSUPPORTED beyond.  No allocation, no synchronisation: the call may be captured into a hipGraph.
 * qnn_last_kernel() names the kernel that ran: pool_max_bin / _i4 / _i8 / _f32, pool_avg_bin / _i4 / _i8 / _f32.
 */
int qnn_pool2d_forward(const void* x, int x_store, int x_bits, int N, int H, int W, int C,
                       const qnn_pool2d_t* p, void* y, int y_store, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* QNN_ABI_POOL_H */

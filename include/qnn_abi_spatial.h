/*
 * qnn_abi_spatial.h -- extension of the C ABI (qnn_abi.h, version 4): keras.layers.Cropping2D, UpSampling2D (nearest
 * neighbour) and ZeroPadding2D on NHWC float32 tensors and on packed codes.  One descriptor and two entry points;
 * conventions, status codes and the QNN_STORE_* layouts are those of qnn_abi.h.  An extension of ABI 4 in a header of its
 * own: qnn_abi.h, its symbol list, qnn_version() and every existing struct are what they were.
 *
 * Semantics.  The three steps apply in the order crop, then repeat, then pad; a Keras layer sets only its own fields
 * (crop and pad 0, up 1 elsewhere).  With Hc = H - crop_t - crop_b and Wc = W - crop_l - crop_r:
 *   output size   Ho = Hc * up_y + pad_t + pad_b,  Wo = Wc * up_x + pad_l + pad_r;
 *   output pixel  (n, oy, ox) is zero where oy < pad_t, oy >= pad_t + Hc * up_y, ox < pad_l or ox >= pad_l + Wc * up_x;
 *                 otherwise it is input pixel (n, crop_t + (oy - pad_t) / up_y, crop_l + (ox - pad_l) / up_x);
 *   zero          float 0.0, code 0 for QNN_STORE_I4 / _I8, mask 0 / sign 0 for QNN_STORE_T2.  A QNN_STORE_BIN code is
 *                 +-1 and has no zero: a pad on that store is refused (crop and repeat are fine).
 * Every output pixel is a copy of one input pixel or zero: codes are copied, never re-quantised, there is no arithmetic.
 * On the packed stores a pixel is a whole number of words, so the entry moves words.
 */
#ifndef QNN_ABI_SPATIAL_H
#define QNN_ABI_SPATIAL_H

#include "qnn_abi.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct qnn_spatial2d {
    int32_t crop[4];   /* top, bottom, left, right rows / columns removed: >= 0            */
    int32_t up[2];     /* nearest-neighbour repeat of rows, columns: >= 1                  */
    int32_t pad[4];    /* top, bottom, left, right rows / columns of zeros added: >= 0     */
} qnn_spatial2d_t;

/*
 * Output size of qnn_spatial2d_forward on an H x W image.  QNN_EINVAL where that call would answer QNN_EINVAL for the
 * geometry: a null pointer, H or W < 1, a negative crop or pad, up < 1, a crop that leaves no row or no column.
 * QNN_EUNSUPPORTED where a size does not fit an int.  Touches no device.
 */
int qnn_spatial2d_out_hw(int H, int W, const qnn_spatial2d_t* s, int* Ho, int* Wo);

/*
 * y = pad(repeat(crop(x))) for an N x H x W x C tensor x; y is N x Ho x Wo x C.
 *   store    QNN_STORE_F32, or QNN_STORE_BIN / _I4 / _I8 / _T2 in the layout qnn_pack_f32 writes; the store and x_bits
 *            of y are those of x.  The bits of a pixel's last word (T2: last word pair) beyond channel C - 1 are zero in
 *            y, whatever x holds there (as qnn_pool2d_forward and qnn_concat_forward), so y can be handed to every entry
 *            that takes a packed tensor.
 *   x_bits   for _I4 / _I8 the codes are signed x_bits-bit values, 1 <= x_bits <= store (checked; the fields are copied
 *            whole); ignored for the other stores.
 * Answers.  QNN_EINVAL: a null descriptor, a null pointer with N > 0, H, W or C < 1, N < 0, a negative crop or pad,
 * up < 1, a crop that leaves no row or no column, another store (QNN_STORE_U8 included), x_bits that does not fit, y
 * overlapping x.  QNN_EUNSUPPORTED: QNN_STORE_BIN with any pad > 0 (the message says: unpack, pad in float32); N x Ho x Wo
 * x (words per pixel; float32: channels) >= 2^31.  N == 0 is QNN_OK without a launch (the pointers may then be null).
 * Everything is checked before the first HIP call.  No allocation, no host read, no synchronisation, and the descriptor
 * reaches the kernel by value: the call may be captured into a hipGraph.  qnn_last_kernel() names spatial_f32,
 * spatial_bin, spatial_i4, spatial_i8 or spatial_t2.
 */
int qnn_spatial2d_forward(const void* x, int store, int x_bits, int N, int H, int W, int C,
                          const qnn_spatial2d_t* s, void* y, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* QNN_ABI_SPATIAL_H */

/*
 * qnn_abi_concat.h -- extension of the C ABI (qnn_abi.h, version 4): keras.layers.Concatenate(axis=-1) on NHWC float32
 * tensors and on packed codes.  One descriptor and one entry point; conventions, status codes and the QNN_STORE_* layouts
 * are those of qnn_abi.h.  An extension of ABI 4 in a header of its own: qnn_abi.h, its symbol list, qnn_version() and
 * qnn_epilogue_t are what they were.
 *
 * Semantics.  Output pixel p holds the channels of x[0] at pixel p, then those of x[1] at p, and so on: channels[0] +
 * ... + channels[n-1] channels.  Between two low-bit layers the activations are packed codes, and the channel counts of
 * the branches that meet (growth rates such as 12 or 24, a 3-channel image) rarely fill whole words, so on the packed
 * stores the entry moves bit fields, not words.  Codes are copied, never re-quantised: there is no arithmetic.
 */
#ifndef QNN_ABI_CONCAT_H
#define QNN_ABI_CONCAT_H

#include "qnn_abi.h"

#ifdef __cplusplus
extern "C" {
#endif

#define QNN_CONCAT_MAX 8

typedef struct qnn_concat {
    int32_t n;                            /* inputs: 1 .. QNN_CONCAT_MAX (1: a copy with the spare bits cleared) */
    int32_t channels[QNN_CONCAT_MAX];     /* channels of input i: >= 1 for i < n, ignored beyond                  */
    const void* x[QNN_CONCAT_MAX];        /* device pointers of the n inputs                                      */
} qnn_concat_t;

/*
 * y = concatenate(x[0], ..., x[n-1]) along the channels, for `pixels` pixels (N * H * W of an NHWC tensor, N of an (N, K) one).
 *   store    QNN_STORE_F32, or QNN_STORE_BIN / _I4 / _I8 / _T2, shared by every input and by y; every other store is
 *            QNN_EINVAL.  Input i is in the layout qnn_pack_f32 writes for channels[i] channels: `pixels` rows of
 *            ceil(channels[i] / per_word) words (QNN_STORE_T2: ceil(channels[i] / 32) (mask, sign) word pairs); float32: rows
 *            of channels[i] values.  y is in that layout for the sum of the channels.  The bits of a pixel's last word
 *            (T2: last word pair) beyond the last channel are zero, whatever the inputs hold in their own spare bits, so y can
 *            be handed to every entry that takes a packed tensor.
 *   x_bits   as in qnn_pool2d_forward: for _I4 / _I8 the codes are signed x_bits-bit values, 1 <= x_bits <= store
 *            (checked; the fields are copied whole); ignored for the other stores.
 * Answers.  QNN_EINVAL: a null descriptor, n outside 1 .. QNN_CONCAT_MAX, a channels[i] < 1, another store, x_bits that
 * does not fit, a null pointer (pixels > 0), y overlapping an input.  QNN_EUNSUPPORTED: pixels x (words of an output
 * pixel; float32: channels) >= 2^31, or an output pixel of 2^26 words or more.  pixels == 0 is QNN_OK without a launch
 * (the pointers may then be null).  Everything is checked before the first HIP call.  The descriptor is read during the
 * call only and reaches the kernel by value: no allocation, no host read, no synchronisation, so the call may be captured
 * into a hipGraph.  qnn_last_kernel() names concat_f32, concat_bin, concat_i4, concat_i8 or concat_t2.
 */
int qnn_concat_forward(const qnn_concat_t* c, int store, int x_bits, size_t pixels, void* y, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* QNN_ABI_CONCAT_H */

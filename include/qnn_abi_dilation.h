/*
 * qnn_abi_dilation.h -- extension of the C ABI (qnn_abi.h, version 4): conv layers with a dilation_rate.
 * One entry point; conventions, status codes and handles are those of qnn_abi.h.
 */
#ifndef QNN_ABI_DILATION_H
#define QNN_ABI_DILATION_H

#include "qnn_abi.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * qnn_prepack_weights with a dilated window: `dilation_rate` of the reference's conv layers, which hand it to K.conv2d
 * (layers/quantized_layers.py:171-177, binary_layers.py:167-173, ternary_layers.py).  Neighbouring taps are dil_h rows /
 * dil_w columns apart, so a kh x kw kernel covers the EFFECTIVE window ke = dil * (k - 1) + 1 per axis, and output size
 * and 'same' padding follow TensorFlow's rule on ke: same -> out = in, total padding ke - 1, the odd cell after;
 * valid -> out = in - ke + 1, and 0 (an empty output, refused by the forward calls) for in < ke.
 * qnn_prepack_weights(...) is this entry with dil_h = dil_w = 1.  The two axes are independent.
 *   dil_h, dil_w : 1 .. QNN_MAX_DILATION; < 1 is QNN_EINVAL, larger QNN_EUNSUPPORTED.  kh, kw stay <= 3.
 * QNN_EUNSUPPORTED, each with its reason in qnn_last_error():
 *   - dilation != 1 together with stride != 1 (here; Keras refuses the pair as well);
 *   - a dilated handle in qnn_dense_forward, qnn_conv2d_dense_forward or qnn_fold_prepare;
 *   - a dilated handle with epi->proj or epi->fold.
 * Kernels: 3x3 'same' int4 -> int4 layers of 16 / 32 / 64 input channels with a square dilation of 2 or 3 run on the
 * matrix pipe (qnn_last_kernel() "strip_i4_c<cin>_dil"; QNN_EPI_NO_STRIP keeps them off it); every other dilated call
 * runs on the generic kernel, all stores and epilogues included.  Results are bit-identical between the two.
 * An extension of ABI 4 in a header of its own: qnn_abi.h, its symbol list and qnn_version() are what they were, and a
 * caller that never includes this file sees no change.
 */
#define QNN_MAX_DILATION 64
int qnn_prepack_weights_dilated(int wkind, int wbits, float H, const float* kernel,
                                int kh, int kw, int cin, int cout, const float* bias,
                                int stride, int same_pad, int dil_h, int dil_w, int store, void* stream,
                                qnn_weights_t** out);

#ifdef __cplusplus
}
#endif
#endif /* QNN_ABI_DILATION_H */

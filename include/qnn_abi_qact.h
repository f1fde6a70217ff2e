/*
 * qnn_abi_qact.h -- extension of the C ABI (qnn_abi.h, version 4): the quantised activations as an elementwise op.
 * One entry point; conventions, status codes and the QNN_FN_* codes are those of qnn_abi.h.
 */
#ifndef QNN_ABI_QACT_H
#define QNN_ABI_QACT_H

#include "qnn_abi.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * y = fn(x) on n float32 values, the result on the grid k / 2^(nb-1) as float32:
 *   fn = QNN_FN_QUANTIZED_RELU       quantized_ops.quantized_relu, layers/quantized_ops.py:69-84
 *   fn = QNN_FN_QUANTIZED_LEAKYRELU  quantized_ops.quantized_leakyrelu at alpha = float32(0.1), quantized_ops.py:102-123
 *   fn = QNN_FN_QUANTIZED_TANH       the same as qnn_quantized_tanh_f32
 * (the arithmetic is stated beside the codes in qnn_abi.h).  nb in 1 .. 24; any other fn is QNN_EINVAL.  x == y allowed.
 * An extension of ABI 4 in a header of its own: qnn_abi.h, its symbol list and qnn_version() are what they were.
 */
int qnn_quantized_act_f32(const float* x, float* y, size_t n, int fn, int nb, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* QNN_ABI_QACT_H */

// Output size and leading padding of one axis of a convolution, TensorFlow semantics.  Plain C++ without HIP, so that
// the rule is compiled and tested on its own (tests/test_conv_geom.py); qnn_common.h includes it for every launcher.
#pragma once

// SAME:  out = ceil(in / s), total padding = max((out - 1) * s + k - in, 0), `before` = total / 2 (the odd cell goes
//        after) -- oracle: same_padding().
// VALID: out = number of window starts 0, s, 2s, ... whose k cells lie inside the image = (in - k) / s + 1 for
//        in >= k and 0 for in < k.  The quotient alone is not enough: C division truncates toward zero, so
//        (in - k) / s + 1 is 1, not 0, for 0 < k - in < s.
static inline void qnn_same_pad(int in, int k, int s, int same, int* out, int* before) {
    if (same) {
        *out = (in + s - 1) / s;
        int total = (*out - 1) * s + k - in;
        if (total < 0) total = 0;
        *before = total / 2;
    } else {
        *out = in < k ? 0 : (in - k) / s + 1;
        *before = 0;
    }
}

// The same rule for a dilated window: taps d cells apart cover the effective window ke = d * (k - 1) + 1, and SAME / VALID
// are TensorFlow's rule on ke (tf.nn.conv2d with dilations).  d = 1 is qnn_same_pad itself.  VALID is 0 for in < ke.
static inline void qnn_same_pad_dilated(int in, int k, int s, int d, int same, int* out, int* before) {
    qnn_same_pad(in, d * (k - 1) + 1, s, same, out, before);
}

// The transposed convolution (tf.nn.conv2d_transpose, include/qnn_abi_tconv.h): the scatter of `in` cells at stride s
// through a window of k fills `full` = (in - 1) * s + k cells; the output is cells [before, before + out) of it, read as
// zero beyond `full`.
// VALID: out = in * s + max(k - s, 0), before = 0 (k < s: the last s - k cells lie beyond `full`).
// SAME:  out = in * s, before = max(k - s, 0) / 2 (the odd cell is cut after) -- the padding of the forward SAME
//        convolution that maps `out` cells back to `in`.
static inline void qnn_tconv_out_pad(int in, int k, int s, int same, int* out, int* before) {
    const int extra = k > s ? k - s : 0;
    *out = same ? in * s : in * s + extra;
    *before = same ? extra / 2 : 0;
}

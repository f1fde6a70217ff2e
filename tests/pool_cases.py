"""Cases and the numpy reference of the pooling tests (test_pool_cpu.py, test_gpu_pool.py): Keras 2.1.3's
MaxPooling2D / AveragePooling2D on TensorFlow, NHWC, as include/qnn_abi_pool.h states them.

The reference is written without the package: its output size and its padding offsets are TensorFlow's rule spelt out
here, so that the tests can hold _abi.out_hw and the library against it."""
import functools
import zlib

import numpy as np

F32 = np.float32


def pair(v):
    return (int(v), int(v)) if np.isscalar(v) else (int(v[0]), int(v[1]))


def axis(h, k, s, same):
    """(output size, padding before) of one axis: 'same' = ceil(h / s) with pad_total = max((out - 1) s + k - h, 0), the
    odd cell behind; 'valid' = the window starts 0, s, 2s, ... whose window lies inside the image."""
    if same:
        out = -(-h // s)
        return out, max((out - 1) * s + k - h, 0) // 2
    if k > h:
        raise ValueError("'valid' window %d is larger than the image %d" % (k, h))
    return (h - k) // s + 1, 0


def pool2d_ref(x, mode, size, strides=None, padding="valid"):
    """x: NHWC float32 or float64.  mode "max": the maximum over the in-bounds cells of every window, in x's dtype.
    mode "avg": the in-bounds cells summed in float64 in row order (rows outer, columns inner), rounded once to float32
    and divided in float32 by float32(number of in-bounds cells): float32.  For grid values k / 2^(bits-1) the float64
    sum is the exact integer sum of the codes times 2^-(bits-1) and fits float32, so this is also the rounding of the
    packed kernels: fdiv_rn(fmul_rn((float)sum, 2^-(bits-1)), (float)count)."""
    assert mode in ("max", "avg") and padding in ("valid", "same")
    ph, pw = pair(size)
    sh, sw = (ph, pw) if strides is None else pair(strides)
    N, H, W, C = x.shape
    same = padding == "same"
    Ho, pt = axis(H, ph, sh, same)
    Wo, pl = axis(W, pw, sw, same)
    out = np.empty((N, Ho, Wo, C), x.dtype if mode == "max" else F32)
    for oy in range(Ho):
        ya, yb = max(oy * sh - pt, 0), min(oy * sh - pt + ph, H)
        for ox in range(Wo):
            xa, xb = max(ox * sw - pl, 0), min(ox * sw - pl + pw, W)
            assert yb > ya and xb > xa                  # a window without an in-bounds cell cannot occur
            if mode == "max":
                out[:, oy, ox, :] = x[:, ya:yb, xa:xb, :].max(axis=(1, 2))
            else:
                acc = np.zeros((N, C), np.float64)
                for yy in range(ya, yb):
                    for xx in range(xa, xb):
                        acc += x[:, yy, xx, :].astype(np.float64)
                out[:, oy, ox, :] = acc.astype(F32) / F32((yb - ya) * (xb - xa))
    return out


def global_ref(x, mode):
    N, H, W, C = x.shape
    return pool2d_ref(x, mode, (H, W)).reshape(N, C)


# (N, H, W, window or "whole", strides or None = the window, padding)
GEOMS = [
    (1, 1, 1, (1, 1), None, "valid"),
    (1, 1, 1, (1, 1), None, "same"),
    (3, 2, 5, (2, 2), None, "valid"),
    (1, 2, 5, (2, 3), (1, 1), "same"),
    (1, 5, 2, (3, 2), (2, 1), "same"),
    (3, 5, 2, (2, 2), (1, 1), "valid"),
    (1, 7, 7, (3, 3), (2, 2), "same"),        # pad_total 2: 1 before, 1 behind
    (3, 8, 8, (3, 3), (2, 2), "same"),        # pad_total 1: 0 before, 1 behind
    (1, 8, 8, (2, 2), None, "same"),          # 'same' pads nothing
    (1, 8, 8, (2, 2), None, "valid"),         # the geometry of the old size-only form
    (1, 8, 8, (2, 2), (3, 3), "valid"),       # strides above the window: cells no window reads
    (1, 8, 8, (2, 2), (3, 3), "same"),
    (1, 8, 8, (3, 3), (3, 3), "same"),
    (3, 9, 6, (3, 2), None, "valid"),
    (1, 9, 6, (2, 3), (2, 1), "same"),
    (1, 9, 6, (3, 3), (1, 1), "same"),
    (1, 7, 7, (3, 3), (1, 1), "valid"),
    (1, 7, 7, (2, 2), (2, 2), "valid"),       # the last row and column are read by no window
    (1, 9, 6, "whole", None, "valid"),        # the global ops
    (3, 7, 7, "whole", None, "valid"),
    (1, 2, 5, "whole", (1, 1), "same"),       # the whole image as a sliding window: every output cuts it differently
]

# channels across the word edges; BIN 128 / I4 64 / I8 64 / F32 64: words per pixel divisible by 4 (16 bytes per lane)
CHANNELS = {"bin": (1, 31, 32, 33, 70, 128), "i4": (1, 7, 8, 9, 64, 72), "i8": (1, 3, 4, 5, 64), "f32": (1, 5, 64)}
# (channels, bits): the store's own width everywhere, narrower codes where a word is split and where it is whole
BITS = {"bin": [(c, 1) for c in CHANNELS["bin"]],
        "i4": [(c, 4) for c in CHANNELS["i4"]] + [(9, 2), (64, 2), (9, 3), (64, 3)],
        "i8": [(c, 8) for c in CHANNELS["i8"]] + [(5, 5), (64, 5)],
        "f32": [(c, 0) for c in CHANNELS["f32"]]}
VALUE_SETS = ("random", "min", "const")


def geom(g):
    """(N, H, W, size, strides, padding) with "whole" resolved."""
    N, H, W, size, strides, padding = g
    return N, H, W, ((H, W) if size == "whole" else size), strides, padding


@functools.lru_cache(maxsize=None)
def values(gi, kind, C, bits, vset):
    """The input of one case, float32 NHWC, read-only.  Packed kinds: grid values code * 2^-(bits-1) (bin: +-1) --
    "random" codes, "min" the smallest code everywhere (a padded cell replaced by zero would win the maximum), "const" one
    code everywhere (a 'same' average must return it exactly: a division by the window area would not).  f32: random
    multiples of 2^-10 in [-8, 8], whose sums are exact in float64 in any order; "min" -8 everywhere, "const" 0.625."""
    N, H, W, _, _, _ = geom(GEOMS[gi])
    rng = np.random.default_rng(zlib.crc32(repr((gi, kind, C, bits, vset)).encode()))
    shape = (N, H, W, C)
    if kind == "f32":
        x = {"random": rng.integers(-8192, 8193, shape) / 1024.0, "min": np.full(shape, -8.0),
             "const": np.full(shape, 0.625)}[vset]
    elif kind == "bin":
        x = {"random": rng.integers(0, 2, shape) * 2.0 - 1.0, "min": np.full(shape, -1.0), "const": np.full(shape, 1.0)}[vset]
    else:
        m = 2 ** (bits - 1)
        x = {"random": rng.integers(-m, m, shape), "min": np.full(shape, -m), "const": np.full(shape, m - 1 if bits > 1 else -1)}[vset] / float(m)
    x = np.ascontiguousarray(x, dtype=F32)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def expected(gi, kind, C, bits, vset, mode):
    """pool2d_ref of values(...), computed once and shared, read-only."""
    _, _, _, size, strides, padding = geom(GEOMS[gi])
    y = pool2d_ref(values(gi, kind, C, bits, vset), mode, size, strides, padding)
    y.setflags(write=False)
    return y

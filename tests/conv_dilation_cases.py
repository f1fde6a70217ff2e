"""The dilated convolutions the test files share: tests/test_conv_dilation_cpu.py proves the expected values (the plain
convolution with the ZERO-STUFFED kernel) against torch in float64 on every case; tests/test_gpu_conv_dilation.py runs
the cases on the GPU.

A dilated k-tap axis with rate d covers the effective window ke = d (k - 1) + 1; the zero-stuffed kernel is ke x ke with
the original taps at multiples of d and zeros between them, so oracle.conv2d -- which takes any window and applies
TensorFlow's SAME / VALID rule to it -- needs no change.  The kernel values handed to stuff() are already quantized
(0 is not a binary weight: a stuffed kernel never goes through binarize)."""
import numpy as np

from conv_geometry_cases import codes                    # integer codes in [lo, hi]  # noqa: F401

WINDOWS = ((3, 3), (1, 3), (3, 1), (2, 2), (2, 3))
DILATIONS = ((2, 2), (1, 2), (3, 1), (2, 3), (5, 5))
PADDINGS = ("same", "valid")
IMAGES = ((7, 9), (2, 3), (1, 1))                        # the last two are smaller than most effective windows
N = 2

# the generic kernel's layers: input store -> (Cin, Cout), the channel counts of GROUP1 in test_gpu_conv_geometry.py
GENERIC = {"f32": (5, 10), "u8": (5, 4), "bin": (24, 10), "t2": (3, 4), "i4": (24, 10), "i8": (5, 4)}

# the strip kernel (csrc/qnn_mfma_strip_dil.hip): the dilations its route claims, one it does not, and the images
STRIP_CLAIMED = (2, 3)
STRIP_UNCLAIMED = 4
STRIP_CIN = (16, 32, 64)
STRIP_IMAGES = ((3, 5, 16), (2, 1, 1), (3, 2, 3), (2, 13, 20), (2, 9, 33), (1, 3, 47), (1, 40, 16))      # (N, H, W)
TALL = (1, 40, 16)                                       # several row chunks (test_strip_plan_cuts_the_tall_image)


def effective(k, d):
    return d * (k - 1) + 1


def out_size(size, k, d, padding):
    """TensorFlow's rule on the effective window, stride 1; VALID is 0 where the image is smaller."""
    if padding == "same":
        return size
    ke = effective(k, d)
    return size - ke + 1 if size >= ke else 0


def same_before(size, k, d):
    """Leading SAME padding at stride 1: the total is ke - 1, the odd cell goes after."""
    return (effective(k, d) - 1) // 2


def stuff(kernel, dh, dw):
    """HWIO kernel -> the zero-stuffed (ke_h, ke_w, I, O) kernel of the same convolution without dilation."""
    kh, kw, ci, co = kernel.shape
    out = np.zeros((effective(kh, dh), effective(kw, dw), ci, co), kernel.dtype)
    out[::dh, ::dw] = kernel
    return out


def geometries():
    """Every (window, dilation, padding, image) of the list, as dicts."""
    return [dict(kh=kh, kw=kw, dh=dh, dw=dw, padding=p, H=H, W=W)
            for kh, kw in WINDOWS for dh, dw in DILATIONS for p in PADDINGS for H, W in IMAGES]


def geom_id(g):
    return "%dx%d_d%dx%d_%s_%dx%d" % (g["kh"], g["kw"], g["dh"], g["dw"], g["padding"], g["H"], g["W"])


def out_hw(g):
    return out_size(g["H"], g["kh"], g["dh"], g["padding"]), out_size(g["W"], g["kw"], g["dw"], g["padding"])


def seed_of(g, salt=0):
    return ((((g["kh"] * 4 + g["kw"]) * 8 + g["dh"]) * 8 + g["dw"]) * 2 + (g["padding"] == "same")) * 4096 + \
        g["H"] * 64 + g["W"] + 1000003 * salt


def layer_values(kind, g, cin, cout, n=N, salt=0):
    """(x, quantized kernel, bias) of one layer, dyadic: values of input store `kind` and weights of the matching width."""
    rng = np.random.default_rng(seed_of(g, salt) + 17 * cin + cout)
    sx, sw = (n, g["H"], g["W"], cin), (g["kh"], g["kw"], cin, cout)
    bias = (codes(rng, (cout,), -8, 8) / 16.0).astype(np.float32)
    if kind == "bin":
        return (2 * codes(rng, sx, 0, 1) - 1).astype(np.float32), (2 * codes(rng, sw, 0, 1) - 1).astype(np.float32), bias
    if kind == "t2":
        return codes(rng, sx, -1, 1).astype(np.float32), codes(rng, sw, -1, 1).astype(np.float32), bias
    if kind == "i8":
        return (codes(rng, sx, -128, 127) / 128.0).astype(np.float32), \
            (codes(rng, sw, -128, 127) / 128.0).astype(np.float32), bias
    if kind == "u8":
        return codes(rng, sx, 0, 255).astype(np.uint8), (codes(rng, sw, -8, 7) / 8.0).astype(np.float32), bias
    return (codes(rng, sx, -8, 7) / 8.0).astype(np.float32), (codes(rng, sw, -8, 7) / 8.0).astype(np.float32), bias


WKIND = {"bin": "binary", "t2": "ternary", "i8": "quantized", "u8": "quantized", "f32": "quantized", "i4": "quantized"}
WBITS = {"i8": 8, "u8": 4, "f32": 4, "i4": 4}


def conv_op(kind, g, kernel, bias):
    """The conv op of a net spec (what engine._prepack reads) for already quantized `kernel` values."""
    op = {"op": "conv", "kind": WKIND[kind], "kernel": kernel, "bias": bias, "strides": (1, 1), "padding": g["padding"],
          "dilation_rate": (g["dh"], g["dw"])}
    if kind in WBITS:
        op["nb"] = WBITS[kind]
    return op

"""Cases and the numpy reference of the spatial-op tests (test_spatial_cpu.py, test_gpu_spatial.py): Cropping2D,
UpSampling2D (nearest) and ZeroPadding2D on NHWC float32 tensors and on packed codes, as include/qnn_abi_spatial.h
states them: crop, then repeat, then pad.

  DESCS, CHANNELS, BITS   the descriptors of the kernel grid with their image sizes, the channel counts per store (a ragged
                          last word, a whole word, the 16-byte form), the code widths
  out_hw / spatial_ref    the reference: decode words to codes (concat_cases.encode / decode), a[:, ct:H-cb, cl:W-cr],
                          np.repeat on both axes, np.pad, encode.  No arithmetic: every comparison is bit for bit
  form                    which kernel form the library's rule picks (restated from the issue's words)
  Net / reference / guard whole specs with crop / upsample / pair-form zeropad (and concat) on top of concat_cases.py
  SPECS, CHAINS           the encoder-decoder and the crop / pad network per activation, and their concat-free
                          counterparts that LayerModel runs too

Plain numpy: neither torch nor the package is imported here."""
import numpy as np

import concat_cases as C
import spec_graph_cases as S

F32 = np.float32
STORE, PER_WORD, words, encode, decode, spare, codes, f32_values = \
    C.STORE, C.PER_WORD, C.words, C.encode, C.decode, C.spare, C.codes, C.f32_values

IDENTITY = {"crop": ((0, 0), (0, 0)), "up": (1, 1), "pad": ((0, 0), (0, 0))}


def desc(crop=((0, 0), (0, 0)), up=(1, 1), pad=((0, 0), (0, 0))):
    return {"crop": crop, "up": up, "pad": pad}


# (name, (H, W), descriptor): four distinct numbers per step, non-square images
DESCS = [
    ("pad", (3, 5), desc(pad=((1, 2), (0, 3)))),
    ("crop", (4, 6), desc(crop=((1, 0), (2, 1)))),
    ("up23", (3, 5), desc(up=(2, 3))),
    ("up11", (3, 5), desc(up=(1, 1))),
    ("all", (4, 6), desc(crop=((1, 0), (2, 1)), up=(2, 3), pad=((1, 2), (0, 3)))),
]
N_GRID = 2
RAGGED_IMAGE = (7, 20)                   # 2 x 7 x 20 pixels: a ragged last workgroup
# per store: a ragged last word, a whole word (None: no such count below the 16-byte one), the 16-byte form
CHANNELS = {"bin": (33, 64, 128), "t2": (33, None, 64), "i4": (9, 8, 32), "i8": (5, 4, 16), "f32": (3, None, 4)}
BITS = {"bin": (1,), "t2": (1,), "i4": (4, 3), "i8": (8, 7), "f32": (0,)}       # the store's width and one below it


def padded(d):
    return any(v > 0 for side in d["pad"] for v in side)


def out_hw(H, W, d):
    (ct, cb), (cl, cr) = d["crop"]
    (pt, pb), (pl, pr) = d["pad"]
    return (H - ct - cb) * d["up"][0] + pt + pb, (W - cl - cr) * d["up"][1] + pl + pr


def spatial_array(a, d):
    """crop -> repeat -> pad of an (N, H, W, C) array."""
    (ct, cb), (cl, cr) = d["crop"]
    H, W = a.shape[1:3]
    a = a[:, ct:H - cb, cl:W - cr]
    a = np.repeat(np.repeat(a, d["up"][0], axis=1), d["up"][1], axis=2)
    return np.pad(a, ((0, 0), tuple(d["pad"][0]), tuple(d["pad"][1]), (0, 0)))


def spatial_ref(w, kind, shape, d):
    """The reference on stored tensors: words (N * H * W, words) -> words (N * Ho * Wo, words); float32: values, moved
    as their bits."""
    N, H, W, Cn = shape
    if kind == "f32":
        bits = np.ascontiguousarray(w, dtype=F32).view(np.uint32).reshape(N, H, W, Cn)
        return spatial_array(bits, d).view(F32)
    assert not (kind == "bin" and padded(d)), "a +-1 code has no zero"
    k = decode(np.asarray(w).reshape(N * H * W, -1), kind, Cn).reshape(N, H, W, Cn)
    out = spatial_array(k, d)
    if kind == "bin":
        assert np.all(out != 0)
    return encode(out.reshape(-1, Cn), kind)


def form(kind, Cn, aligned16=True):
    """"v4" (16 bytes per lane) where a pixel's word count divides by 4 and both pointers are 16-byte aligned, else "v1"."""
    return "v4" if aligned16 and words(kind, Cn) % 4 == 0 else "v1"


# ---- whole specs ------------------------------------------------------------------------------------------------------
class Net(C.Net):
    """concat_cases.Net with the three spatial ops."""

    def _spatial(self, op, d, src, dst):
        h, w, c = self.shape[self.cur if src is None else src]
        ho, wo = out_hw(h, w, d)
        assert ho > 0 and wo > 0
        return self._put(op, src, (ho, wo, c), dst)

    def zeropad2(self, pad, src=None, dst=None):
        return self._spatial({"op": "zeropad", "pad": pad}, desc(pad=pad), src, dst)

    def crop(self, crop, src=None, dst=None):
        return self._spatial({"op": "crop", "crop": crop}, desc(crop=crop), src, dst)

    def upsample(self, size, src=None, dst=None):
        return self._spatial({"op": "upsample", "size": size}, desc(up=size), src, dst)

    def images(self):                    # batch 2
        return S.Net.images(self)[:2]


def op_desc(op):
    """The descriptor of a new-form spatial spec op, or None."""
    return S.spatial_desc(op)


def reference(spec, x, return_all=False):
    """spec_graph_cases.reference: the shared op-by-op float32 reference knows the spatial ops (spatial_array)."""
    return S.reference(spec, x, return_all)


def guard(spec, x):
    """spec_graph_cases.guard: None, or the reason the case is not exact by construction."""
    return S.guard(spec, x)


# activation name -> (fn, abits, weight kind, weight bits, the spatial kernel GraphModel logs)
ACTS = {"q4": ("quantized_tanh", 4, "quantized", 4, "i4"), "q8": ("quantized_tanh", 8, "quantized", 8, "i8"),
        "tern": ("ternary_tanh", 1, "ternary", 1, "t2"), "bin": ("binary_tanh", 1, "binary", 1, "bin")}


def encoder_decoder(seed, act, skip=True):
    """conv -> clip -> max-pool -> conv -> clip -> upsample (2, 2) -> [concat with the skip ->] conv, 8 x 8 images."""
    fn, abits, wk, wnb, _ = ACTS[act]
    net = Net(seed, hw=(8, 8))
    a0 = net.group(8, wk, wnb, fn, abits, dst="a0")
    net.pool("maxpool", 2, src=a0, dst="p")
    net.group(12, wk, wnb, fn, abits, dst="a1")
    up = net.upsample((2, 2), dst="up")
    if skip:
        net.concat([up, a0], dst="cat")
    net.group(8, wk, wnb, fn, abits)
    net.classifier(wk, wnb)
    return net


def crop_and_pad(seed, act, skip=True):
    """A crop ((0, 1), (1, 0)) in front of a concat (the other branch: a VALID 2 x 2 conv of the same size), then a
    pair-form zeropad in front of a VALID conv."""
    fn, abits, wk, wnb, _ = ACTS[act]
    net = Net(seed, hw=(8, 8))
    a0 = net.group(8, wk, wnb, fn, abits, dst="a0")
    cr = net.crop(((0, 1), (1, 0)), src=a0, dst="cr")                        # 7 x 7
    if skip:
        a1 = net.group(12, wk, wnb, fn, abits, k=2, pad="valid", src=a0, dst="a1")      # 7 x 7
        net.concat([cr, a1], dst="cat")
    net.zeropad2(((1, 2), (0, 3)), dst="zp")                                 # 10 x 10
    net.group(8, wk, wnb, fn, abits, pad="valid")                            # 8 x 8
    net.classifier(wk, wnb)
    return net


def _log(kinds, act):
    s = ACTS[act][4]
    return [("spatial_" if k == "s" else "concat_") + s for k in kinds]


# name -> (net, GraphModel's kernel_log): the issue's two specs per activation: everything between the clip and the next
# low-bit layer runs on the codes
SPECS = {}
# the same networks without the concat: the one form LayerModel (one tensor per op) expresses, run on both engines
CHAINS = {}
for _i, _a in enumerate(("q4", "q8", "tern")):
    SPECS["encdec_" + _a] = (encoder_decoder(40 + _i, _a), _log("sc", _a))
    SPECS["croppad_" + _a] = (crop_and_pad(50 + _i, _a), _log("scs", _a))
    CHAINS["encdec_" + _a] = (encoder_decoder(60 + _i, _a, skip=False), _log("s", _a))
    CHAINS["croppad_" + _a] = (crop_and_pad(70 + _i, _a, skip=False), _log("ss", _a))


def binary_pad(seed=81):
    """A pair-form zeropad behind a 1-bit clip: a +-1 code has no zero, the pad runs in float32."""
    net = Net(seed, hw=(8, 8))
    net.group(8, "binary", 1, "binary_tanh", 1)
    net.zeropad2(((1, 2), (0, 3)))
    net.group(8, "binary", 1, "binary_tanh", 1, pad="valid")
    net.classifier("binary", 1)
    return net


def binary_upsample(seed=82):
    net = Net(seed, hw=(4, 4))
    net.group(8, "binary", 1, "binary_tanh", 1)
    net.upsample((2, 2))
    net.group(8, "binary", 1, "binary_tanh", 1)
    net.classifier("binary", 1)
    return net

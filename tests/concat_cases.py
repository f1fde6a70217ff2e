"""Cases and the numpy reference of the channel-concatenation tests (test_concat_cpu.py, test_gpu_concat.py):
keras.layers.Concatenate(axis=-1) on NHWC float32 tensors and on packed codes, as include/qnn_abi_concat.h states it.

  LISTS, PIXELS, BITS   the channel lists per store, the pixel counts and the code widths
  codes / encode / decode / concat_ref
                        the reference on packed words: decode each input's words to codes, np.concatenate(axis=-1),
                        encode in the layout qnn_pack_f32 writes.  encode / decode are written channel by channel here;
                        test_concat_cpu.py holds them against tail_cases.pack_words, the suite's restatement of that layout
  form                  which kernel form the library's rule picks for a list (restated from the header's words)
  Net / reference / guard
                        whole specs with a `concat` op on top of spec_graph_cases.py: its builder with one more method, its
                        op-by-op float32 reference with one more op, its exactness guard over the contractions
  SPECS                 the small networks the GPU file runs on GraphModel

Plain numpy: neither torch nor the package is imported here."""
import functools
import zlib

import numpy as np

import spec_graph_cases as S

F32 = np.float32
STORE = {"f32": 0, "bin": 1, "t2": 2, "i4": 4, "i8": 8}                  # include/qnn_abi.h
PER_WORD = {"bin": 32, "t2": 32, "i4": 8, "i8": 4}
MAX_INPUTS = 8                                                          # QNN_CONCAT_MAX

LISTS = {
    "bin": [[3, 5], [32, 32], [31, 1, 33], [3] * 8, [128, 256], [64, 32]],
    "i4": [[3, 5], [8, 8], [7, 9, 16], [12, 24, 36], [32, 64]],
    "i8": [[1, 2, 5], [4, 4], [3, 64], [16, 48]],
    "t2": [[3, 5], [32, 31]],
    "f32": [[3, 5], [4, 4], [1] * 8],
}
PIXELS = (1, 7, 280)                     # 280 = 2 x 7 x 20: a ragged last workgroup
BITS = {"bin": (1,), "t2": (1,), "i4": (4, 2), "i8": (8, 5), "f32": (0,)}       # the store's own width, and one below it
# what the issue calls the aligned (16 bytes per lane) and the whole-word lists; every other packed list is a funnel
ALIGNED = {"bin": [[128, 256]], "i4": [[32, 64]], "i8": [[16, 48]], "f32": [[4, 4]]}
WORD = {"bin": [[32, 32], [64, 32]], "i4": [[8, 8]], "i8": [[4, 4]], "f32": [[3, 5], [1] * 8]}


def words(kind, C):
    """Words of one pixel: ceil(C / per_word); T2: a (mask, sign) word pair per 32 channels; float32: C."""
    if kind == "f32":
        return C
    n = -(-C // PER_WORD[kind])
    return 2 * n if kind == "t2" else n


def form(kind, channels, aligned16=True):
    """The kernel form of include/qnn_abi_concat.h / csrc/qnn_concat.hip for one call: "words4" where every input is a whole
    number of words per pixel, that number divides by 4 and every pointer is 16-byte aligned; "words1" where they are whole
    words only; "funnel" otherwise."""
    if kind == "f32":
        whole, cw = True, list(channels)
    elif kind == "t2":
        whole, cw = all(c % 32 == 0 for c in channels), [2 * (c // 32) for c in channels]
    else:
        field = 32 // PER_WORD[kind]
        whole, cw = all(c * field % 32 == 0 for c in channels), [c * field // 32 for c in channels]
    if not whole:
        return "funnel"
    return "words4" if aligned16 and all(w % 4 == 0 for w in cw) else "words1"


@functools.lru_cache(maxsize=None)
def codes(kind, bits, pixels, C, seed):
    """Integer codes (pixels, C), read-only: bin +-1, t2 {-1, 0, 1}, i4 / i8 the signed `bits`-bit range with both ends
    present in the first pixel where there is room."""
    rng = np.random.default_rng(zlib.crc32(repr((kind, bits, pixels, C, seed)).encode()))
    if kind == "bin":
        k = rng.integers(0, 2, (pixels, C)) * 2 - 1
    elif kind == "t2":
        k = rng.integers(-1, 2, (pixels, C))
    else:
        m = 1 << (bits - 1)
        k = rng.integers(-m, m, (pixels, C))
        k[0, 0] = -m
        k[0, -1] = m - 1 if C > 1 else -m
    k = np.ascontiguousarray(k, dtype=np.int64)
    k.setflags(write=False)
    return k


def encode(k, kind):
    """Codes (pixels, C) -> uint32 words (pixels, words(kind, C)) in the layout qnn_pack_f32 writes: channel c in word
    c // per_word at bit (c % per_word) * field, two's complement in the field; bin: bit = 1 <=> +1; t2: the mask word
    (code != 0) then the sign word (code > 0) of each 32 channels.  Spare bits zero."""
    k = np.asarray(k, dtype=np.int64)
    P, C = k.shape
    pw = PER_WORD[kind]
    field = 32 // pw
    out = np.zeros((P, words(kind, C)), dtype=np.uint64)
    for c in range(C):
        w, sh = c // pw, (c % pw) * field
        if kind == "bin":
            out[:, w] |= (k[:, c] > 0).astype(np.uint64) << np.uint64(sh)
        elif kind == "t2":
            out[:, 2 * w] |= (k[:, c] != 0).astype(np.uint64) << np.uint64(sh)
            out[:, 2 * w + 1] |= (k[:, c] > 0).astype(np.uint64) << np.uint64(sh)
        else:
            out[:, w] |= (k[:, c] & ((1 << field) - 1)).astype(np.uint64) << np.uint64(sh)
    return out.astype(np.uint32)


def decode(w, kind, C):
    """The inverse of encode on the C channels of every pixel; the spare bits are not read."""
    w = np.asarray(w).astype(np.uint32).astype(np.int64)
    pw = PER_WORD[kind]
    field = 32 // pw
    k = np.zeros((w.shape[0], C), dtype=np.int64)
    for c in range(C):
        i, sh = c // pw, (c % pw) * field
        if kind == "bin":
            k[:, c] = ((w[:, i] >> sh) & 1) * 2 - 1
        elif kind == "t2":
            k[:, c] = ((w[:, 2 * i] >> sh) & 1) * (((w[:, 2 * i + 1] >> sh) & 1) * 2 - 1)
        else:
            f = (w[:, i] >> sh) & ((1 << field) - 1)
            k[:, c] = f - ((f >> (field - 1)) << field)
    return k


def spare(kind, C):
    """uint32 (words(kind, C),): the bits of a pixel's words that belong to no channel."""
    # bin / t2 code +1 (t2: in the mask and in the sign word), two's-complement -1: every bit of every channel is set
    return ~encode(np.full((1, C), 1 if kind in ("bin", "t2") else -1, dtype=np.int64), kind)[0]


def concat_ref(ws, channels, kind):
    """The reference: words of the inputs -> words of their channel concatenation (float32: the values themselves)."""
    if kind == "f32":
        return np.concatenate([np.asarray(w).reshape(-1, c) for w, c in zip(ws, channels)], axis=-1)
    return encode(np.concatenate([decode(w, kind, c) for w, c in zip(ws, channels)], axis=-1), kind)


@functools.lru_cache(maxsize=None)
def f32_values(pixels, C, seed):
    """float32 (pixels, C), read-only; the first values are the ones a copy through arithmetic would change: -0.0, the
    infinities, a NaN with a payload, the smallest subnormal.  Compared on their bits."""
    rng = np.random.default_rng(zlib.crc32(repr(("f32", pixels, C, seed)).encode()))
    v = rng.standard_normal((pixels, C)).astype(F32)
    special = np.array([0x80000000, 0x7F800000, 0xFF800000, 0x7FC12345, 0x00000001], dtype=np.uint32).view(F32)
    flat = v.reshape(-1)
    n = min(len(special), flat.size)
    flat[:n] = special[:n]
    v.setflags(write=False)
    return v


# ---- whole specs with a concat op --------------------------------------------------------------------------------------
class Net(S.Net):
    """spec_graph_cases.Net with the concat op; `dst` of a group names its activation."""

    def group(self, cout, kind="quantized", nb=4, fn="quantized_tanh", abits=4, dst=None, **kw):
        self.conv(cout, kind, nb, **kw)
        self.bn()
        return self.act(fn, abits, dst=dst)

    def concat(self, srcs, dst=None):
        shapes = [self.shape[s] for s in srcs]
        assert len({s[:-1] for s in shapes}) == 1, shapes
        op = {"op": "concat", "srcs": list(srcs)}
        if dst is not None:
            op["dst"] = dst
        self.spec.append(op)
        name = S.names_of(self.spec)[-1]
        assert name not in self.shape, name
        self.shape[name] = shapes[0][:-1] + (sum(s[-1] for s in shapes),)
        self.cur = name
        return name


def sources(spec):
    return S.sources(spec)


def reference(spec, x, return_all=False):
    """spec_graph_cases.reference: the shared op-by-op float32 reference knows the concat op."""
    return S.reference(spec, x, return_all)


def guard(spec, x):
    """spec_graph_cases.guard: None, or the reason the case is not exact by construction."""
    return S.guard(spec, x)


def _packed_branches(seed, fn, abits, wkind, wnb, c):
    """Two new-form max-pools of one activation meet: both hand packed codes, the concat joins codes."""
    net = Net(seed, hw=(8, 8))
    a0 = net.group(c, wkind, wnb, fn, abits, dst="a0")
    p1 = net.pool("maxpool", (2, 2), (2, 2), "valid", src=a0, dst="p1")
    p2 = net.pool("maxpool", (3, 3), (2, 2), "same", src=a0, dst="p2")
    net.concat([p1, p2], dst="cat")
    net.group(16, wkind, wnb, fn, abits)
    net.classifier(wkind, wnb)
    return net


def _virtual_branches(seed):
    """Two clips of one function and width meet: the concat joins their pre-activations."""
    net = Net(seed, hw=(8, 8))
    a0 = net.group(8, dst="a0")
    a1 = net.group(12, src=a0, dst="a1")
    a2 = net.group(24, k=1, src=a0, dst="a2")
    net.concat([a1, a2], dst="cat")
    net.group(16)
    net.classifier()
    return net


def _mixed_branches(seed):
    """A max-pool branch (packed codes) beside a strided convolution (a clip): joined in float32."""
    net = Net(seed, hw=(8, 8))
    a0 = net.group(8, dst="a0")
    p = net.pool("maxpool", (3, 3), (2, 2), "same", src=a0, dst="p")
    a1 = net.group(12, s=2, src=a0, dst="a1")
    net.concat([p, a1], dst="cat")
    net.group(16)
    net.classifier()
    return net


def densenet(seed=5, growth=12, blocks=3, stem=24):
    """A DenseNet-style 4-bit network at 8 x 8: every block's 3 x 3 conv -> BN -> clip adds `growth` channels to the
    concatenation of everything before it (24 -> 36 -> 48 -> 60), then the classifier tail."""
    net = Net(seed, hw=(8, 8))
    cur = net.group(stem, dst="stem")
    for b in range(blocks):
        new = net.group(growth, src=cur, dst="grow%d" % b)
        cur = net.concat([cur, new], dst="dense%d" % b)
    net.pool("avgpool", 8)
    net.flatten()
    net.dense(10)
    return net


# name -> (net, GraphModel's kernel_log: its new-form pools and its concats, in order)
SPECS = {
    "packed_i4": (_packed_branches(31, "quantized_tanh", 4, "quantized", 4, 12), ["pool_max_i4", "pool_max_i4", "concat_i4"]),
    "packed_bin": (_packed_branches(32, "binary_tanh", 1, "binary", 1, 12), ["pool_max_bin", "pool_max_bin", "concat_bin"]),
    "packed_i8": (_packed_branches(33, "quantized_tanh", 8, "quantized", 8, 6), ["pool_max_i8", "pool_max_i8", "concat_i8"]),
    "virtual": (_virtual_branches(34), ["concat_f32"]),
    "mixed": (_mixed_branches(35), ["pool_max_i4", "concat_f32"]),
    "densenet": (densenet(), ["concat_f32"] * 3),
}

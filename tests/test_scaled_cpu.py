"""scaled_cases.py proven on the CPU: the integer codes times P / m have the bits of maxrelu_cases.maxact; for every conv /
dense case the GPU tests run, the integer reference equals the oracle's float32 convolution of the float32 activation bit for
bit (in float64 accumulation and in the kernels' fma order), which shows the exactness rule's bound holds for them; a case
just beyond the bound exists in which the two differ; and the Python surface of include/qnn_abi_scaled.h."""
import ctypes
import os
import re

import numpy as np
import pytest

import maxrelu_cases as C
import scaled_cases as S

F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- codes -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nb", C.NBS)
@pytest.mark.parametrize("fn", C.FNS)
def test_codes_times_the_scale_have_the_bits_of_maxact(fn, nb):
    m = 2 ** (nb - 1)
    seen = set()
    for i, M in enumerate(C.MAXIMA + C.AMBIGUOUS):
        for x in (C.edge_inputs(nb, M), np.concatenate([[M], C.uniform_inputs(M, i, 300)]).astype(F32)):
            k = S.codes(x, nb, fn, M)
            lo = 0 if fn == "quantized_maxrelu" else -m
            assert k.min() >= lo and k.max() <= m - 1
            assert C.same_bits(S.values(k, nb, M), C.maxact(x, nb, fn, M=M)), (float(M), nb)
            seen.update(k.tolist())
    assert m - 1 in seen and 0 in seen and (fn == "quantized_maxrelu" or -m in seen)      # both clip edges were reached
    # outside the exact range: codes zero, values NaN -- as maxact
    for M in (F32(0), F32(2.0 ** 64 * 1.0001), F32(2.0 ** -65), F32(np.inf)):
        x = np.array([1.0, -1.0, 0.0], F32)
        assert not S.codes(x, nb, fn, M).any() and np.isnan(S.values(S.codes(x, nb, fn, M), nb, M)).all()
        assert np.isnan(C.maxact(x, nb, fn, M=M)).all()


def test_word_layout():
    k = np.array([[1, -1, 7, -8, 0, 3, -2, 5, 2, -3, 1, 0]])          # 12 channels: a full I4 word and a ragged one
    w4 = S.pack_words(k, S.STORE_I4)
    assert w4.shape == (1, 2) and w4.dtype == np.uint32
    assert w4.tolist() == [[0x5E3087F1, 0x000001D2]]                 # field j = code j: (2, -3 = 0xD, 1, 0) -> 0x01D2
    assert S.spare_mask(12, S.STORE_I4) == 0xFFFF0000 and not (w4[0, 1] & S.spare_mask(12, S.STORE_I4))
    w8 = S.pack_words(k[:, :5], S.STORE_I8)
    assert w8.tolist() == [[0xF807FF01, 0x00000000]]
    assert S.spare_mask(5, S.STORE_I8) == 0xFFFFFF00 and S.spare_mask(8, S.STORE_I4) == 0 and S.spare_mask(16, S.STORE_I8) == 0
    # a 4-bit code in the wide store is sign-extended to the byte
    assert S.pack_words(np.array([[-8, 7, -1, 0]]), S.STORE_I8).tolist() == [[0x00FF07F8]]


# ---- the rule and the cases ------------------------------------------------------------------------------------------
def test_the_exactness_rule():
    assert S.route_is_exact(9 * 512, 4, 4) and S.route_is_exact(4608 * 4, 4, 4)          # 4/4 networks: everywhere they go
    assert S.route_is_exact(1024, 8, 8) and not S.route_is_exact(1025, 8, 8) and not S.route_is_exact(1152, 8, 8)
    assert S.route_is_exact(2 ** 17, 8, 1) and not S.route_is_exact(2 ** 17 + 1, 8, 1)  # binary / ternary weights
    for name, (op, shape, nb, store, kernel, pieces) in S.CONSUMERS.items():
        assert S.route_is_exact(S.contraction_depth(op), nb, S.weight_bits(op)), name


@pytest.mark.parametrize("name", sorted(S.CONSUMERS))
def test_integer_reference_equals_the_float_route(name):
    op, shape, nb, store, kernel, pieces = S.CONSUMERS[name]
    fn = "quantized_leakymaxrelu"
    for P in S.SCALES + (2.0 ** -64, 2.0 ** 64):
        x, M = S.consumer_input(name, P, fn)
        assert C.batch_max(x) == M and 2.0 ** C.scale_exponent(M) == P
        k = S.codes(x, nb, fn, M)
        assert k.min() == -2 ** (nb - 1) and k.max() == 2 ** (nb - 1) - 1          # both clip edges
        y = C.maxact(x, nb, fn)
        bare = S.scaled_reference(k, nb, M, op)
        for which in S.epilogue_sets(pieces) if P in S.SCALES else [()]:
            epi = S.epilogue_args(name, which, bare.shape, P)
            want = S.scaled_reference(k, nb, M, op, **epi)
            assert np.isfinite(want).all() and want.any()
            for order in ("ideal", "device"):
                assert C.same_bits(want, S.float_reference(y, op, order, **epi)), (name, P, which, order)
    # an out-of-range maximum: NaN in front of the epilogue on both routes
    x, M = S.consumer_input(name, 1.0, fn)
    assert np.isnan(S.scaled_reference(S.codes(x, nb, fn, F32(0)), nb, F32(0), op)).all()


def test_beyond_the_bound_the_routes_differ():
    k, op, nb, M = S.beyond_the_bound()
    K = k.shape[1]
    assert not S.route_is_exact(K, nb, 8) and S.route_is_exact(1024, nb, 8)
    y = S.values(k, nb, M)
    wc, wshift = S.O.weight_codes(op)
    assert int(wc.min()) == int(wc.max()) == 127 and int(k.min()) == 127       # all-maximal codes and weights
    exact = int(k.astype(np.int64).dot(wc.reshape(K, 1))[0, 0])
    assert exact == 1041 * 127 * 127 > 2 ** 24 and exact % 2                   # 25 bits and odd: no float32 holds it
    chain = S.float_reference(y, op, "device")
    truth = exact * 2.0 ** -(wshift + nb - 1)
    assert float(chain[0, 0]) != truth                                         # the fma chain has rounded: the guard is needed
    # one step inside the bound the same construction is exact
    k2 = k[:, :1024]
    op2 = dict(op, kernel=op["kernel"][:1024])
    assert C.same_bits(S.scaled_reference(k2, nb, M, op2), S.float_reference(S.values(k2, nb, M), op2, "device"))


# ---- the Python surface --------------------------------------------------------------------------------------------------
def test_the_extension_header_and_its_symbols():
    from qnn_amd import _abi, engine
    hdr = open(os.path.join(ROOT, "include", "qnn_abi_scaled.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert sorted(set(re.findall(r"\b(qnn_[a-z0-9_]+)\s*\(", code))) == sorted(_abi.EXPORTS_SCALED)
    assert sorted(_abi.EXPORTS_SCALED) == ["qnn_conv2d_forward_scaled", "qnn_dense_forward_scaled", "qnn_maxact_pack_f32"]
    others = _abi.EXPORTS + _abi.EXPORTS_QACT + _abi.EXPORTS_DILATION + _abi.EXPORTS_MAXACT + _abi.EXPORTS_POOL
    assert not set(_abi.EXPORTS_SCALED) & set(others) and len(_abi.EXPORTS) == 29
    lib = _abi.load()
    assert lib.qnn_version() == 4
    buf = ctypes.cast(ctypes.create_string_buffer(256), ctypes.c_void_p)
    # argument checks come before any device call
    for fn in _abi.MAXACT_FNS:
        assert lib.qnn_maxact_pack_f32(buf, buf, None, 0, 8, fn, 4, _abi.STORE_I4, buf, None) == 0      # no pixels: nothing launched
        for nb, store in ((1, 4), (5, 4), (9, 8), (4, _abi.STORE_BIN), (4, _abi.STORE_F32)):
            assert lib.qnn_maxact_pack_f32(buf, buf, None, 1, 8, fn, nb, store, buf, None) == -1, (nb, store)
        assert lib.qnn_maxact_pack_f32(buf, buf, None, 1, 0, fn, 4, _abi.STORE_I4, buf, None) == -1
        assert lib.qnn_maxact_pack_f32(buf, buf, None, 1, 8, fn, 4, _abi.STORE_I4, None, None) == -1
        assert lib.qnn_maxact_pack_f32(buf, buf, None, 2 ** 31, 1, fn, 4, _abi.STORE_I4, buf, None) == _abi.QNN_EUNSUPPORTED
        assert b"qnn_maxact_pack_f32" in lib.qnn_last_error()
    for fn in (_abi.FN_QUANTIZED_TANH, _abi.FN_QUANTIZED_RELU, _abi.FN_NONE):
        assert lib.qnn_maxact_pack_f32(buf, buf, None, 1, 8, fn, 4, _abi.STORE_I4, buf, None) == -1
    assert engine.scaled_route_exact(1024, 8, 8) and not engine.scaled_route_exact(1152, 8, 8)
    for K, nb, wb in ((9 * 512, 4, 4), (1024, 8, 8), (1025, 8, 8), (2 ** 17 + 1, 8, 1), (27, 2, 1)):
        assert engine.scaled_route_exact(K, nb, wb) == S.route_is_exact(K, nb, wb)

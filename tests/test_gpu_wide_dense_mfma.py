"""The register-fed dense GEMM (k_dense_mfma, csrc/qnn_dense_mfma.hip) against the oracle's dense call followed by the
float32 BN and the activation, bit for bit, and against the same call on the VALU kernels.

Every case keeps K * 2^(x_bits-1) * 2^(w_bits-1) <= 2^24 (the rule of scaled_cases.py), so the float32 oracle is exact.
Shapes: K = 64 / 192 / 1024 (one K-step; three, ragged over two or four waves; sixteen), N = 1 / 17 / 65 (a ragged image
tile, more than one workgroup), units = 16 / 48 / 272 (one tile; NT does not divide; past route_dense's 256, 17 tiles).
At these sizes the plan keeps NT = 1; PLAN_SHAPES are the smallest layers past one round of workgroups, where it picks
NT = 2 / ks = 4, NT = 4 / ks = 2, NT = 4 / ks = 4 and NT = 4 / ks = 1.

The file is named to be collected behind every other GPU file, so that the 5000 GPU ids the suite had before it keep
their places in a run."""
import ctypes

import numpy as np
import pytest
import torch

import qnn_amd
from qnn_amd import _abi, engine
from oracle import qnn_oracle as O
import qrelu_cases as Q

pytestmark = pytest.mark.gpu
F32 = np.float32
I4, I8, BIN, SF32 = _abi.STORE_I4, _abi.STORE_I8, _abi.STORE_BIN, _abi.STORE_F32
BITS = {I4: 4, I8: 8, BIN: 1}
FN = {"none": _abi.FN_NONE, "binary_tanh": _abi.FN_BINARY_TANH, "quantized_tanh": _abi.FN_QUANTIZED_TANH,
      "quantized_relu": _abi.FN_QUANTIZED_RELU}
SHAPES = [(N, K, U) for K in (64, 192, 1024) for N in (1, 17, 65) for U in (16, 48, 272)]
PLAN_SHAPES = [(1040, 1024, 272), (1025, 1024, 1040), (513, 1024, 1040), (4096, 64, 1024)]
# (operand store, output store, fn, act_bits); a float32 output reaches the route above 256 units only, and from BIN operands
# above 64 images only: the BIN forms stand at j = 1 and 4, where (i + j) % 3 below pairs them with N = 65
F32_FORMS = [(I4, SF32, "none", 0), (BIN, SF32, "binary_tanh", 0), (I8, SF32, "none", 0), (I8, SF32, "quantized_tanh", 8),
             (BIN, SF32, "none", 0), (I4, SF32, "quantized_relu", 4)]
PACKED_FORMS = [(I4, I4, "quantized_tanh", 2), (I4, I4, "quantized_tanh", 4), (I4, I4, "binary_tanh", 0),
                (I4, I4, "quantized_relu", 4), (I8, I8, "quantized_tanh", 8), (I8, I8, "quantized_relu", 8),
                (BIN, I4, "binary_tanh", 0), (BIN, I4, "quantized_tanh", 4)]
CASES = [s + f for i, s in enumerate(SHAPES) for j, f in enumerate(PACKED_FORMS) if (i + j) % 9 == 0] + \
        [s + f for i, s in enumerate(s for s in SHAPES if s[2] == 272) for j, f in enumerate(F32_FORMS) if (i + j) % 3 == 0] + \
        [s + f for s, f in zip(PLAN_SHAPES, (PACKED_FORMS[1], F32_FORMS[3], PACKED_FORMS[6], F32_FORMS[0]))]


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def host(t):
    torch.cuda.synchronize()
    return t.detach().cpu().numpy()


def layer(N, K, U, store, seed):
    """Grid-valued inputs, the dense op, a BN with both signs of inv, and the oracle's pre-activation."""
    bits = BITS[store]
    assert K * 2 ** (bits - 1) * 2 ** (bits - 1) <= 2 ** 24
    rng = np.random.default_rng(seed)
    x = Q.grid_values((N, K), bits, seed)
    op = {"op": "dense", "kind": "binary" if store == BIN else "quantized", "nb": bits,
          "kernel": rng.uniform(-1, 1, (K, U)).astype(F32), "bias": (rng.standard_normal(U) * 0.05).astype(F32)}
    inv, shift = engine.bn_constants(Q.bn_for(U, seed + 1))
    assert (inv > 0).any() and (inv < 0).any()
    v = O.binary_dense_call(x, op["kernel"], op["bias"]) if store == BIN else O.quantized_dense_call(x, op["kernel"], op["bias"], bits)
    pre = ((v * inv).astype(F32) + shift).astype(F32)
    xp = _abi.pack(dev(x), K, _abi.FN_BINARY_TANH if store == BIN else _abi.FN_GRID, bits, store)
    return xp, engine._prepack(op, store, "cuda"), dev(inv), dev(shift), pre


def run(w, xp, store, N, inv, shift, fn, act_bits, out_store, **res):
    """One qnn_dense_forward -> (kernel name, float32 values: a packed output decoded with qnn_unpack_f32)."""
    U = w.shape[3]
    packed = out_store != SF32
    y = torch.empty((N, _abi.words(out_store, U) if packed else U), dtype=torch.int32 if packed else torch.float32, device="cuda")
    epi = _abi.make_epilogue(inv, shift, FN[fn], act_bits, 1, out_store, **res)
    _abi.check(_abi.load().qnn_dense_forward(w.handle, _abi.ptr(xp), store, BITS[store], N, ctypes.byref(epi), _abi.ptr(y),
                                             _abi.stream_ptr()), "qnn_dense_forward")
    kernel = _abi.last_kernel()
    return kernel, host(_abi.unpack(y, N, U, out_store, act_bits or 1) if packed else y)


def both(*a, **kw):
    """The call under the default preference and on its VALU twin."""
    try:
        got = run(*a, **kw)
        _abi.set_conv_impl(_abi.IMPL_VALU)
        return got, run(*a, **kw)
    finally:
        _abi.set_conv_impl(_abi.IMPL_AUTO)


def activation(fn, pre, act_bits):
    return pre if fn == "none" else O.binary_tanh(pre) if fn == "binary_tanh" else Q.ACT[fn](pre, act_bits)


@pytest.mark.parametrize("N,K,U,store,out_store,fn,act_bits", CASES)
def test_dense_mfma_has_the_oracle_bits_and_the_valu_bits(N, K, U, store, out_store, fn, act_bits):
    xp, w, inv, shift, pre = layer(N, K, U, store, 1000 * K + 10 * U + N)
    (kernel, got), (twin_kernel, twin) = both(w, xp, store, N, inv, shift, fn, act_bits, out_store)
    assert kernel == "dense_mfma_" + {I4: "i4", I8: "i8", BIN: "bin"}[store], kernel
    assert not twin_kernel.startswith("dense_mfma"), twin_kernel
    want = activation(fn, pre, act_bits)
    assert Q.same_bits(got, want) if out_store == SF32 else np.array_equal(got, want), np.count_nonzero(got != want)
    assert Q.same_bits(got, twin), (twin_kernel, np.count_nonzero(got != twin))


@pytest.mark.parametrize("what,N,K,U,store,out_store,fn", [
    ("units = 24", 17, 64, 24, I4, I4, "quantized_tanh"), ("cin = 96", 17, 96, 16, I4, I4, "quantized_tanh"),
    ("residual", 17, 64, 272, I4, SF32, "none"), ("BIN output", 17, 64, 32, BIN, BIN, "binary_tanh"),
    ("BIN to float32 at 64 images", 64, 192, 272, BIN, SF32, "none")])
def test_calls_just_outside_the_route_keep_their_kernel_and_bits(what, N, K, U, store, out_store, fn):
    xp, w, inv, shift, pre = layer(N, K, U, store, 7)
    res = {}
    if what == "residual":
        r = np.random.default_rng(8).standard_normal((N, U)).astype(F32)
        res = dict(res=dev(r), res_store=SF32, post_scale=0.5)
        pre = ((r + pre).astype(F32) * F32(0.5)).astype(F32)
    (kernel, got), (twin_kernel, twin) = both(w, xp, store, N, inv, shift, fn, 4 if fn == "quantized_tanh" else 0, out_store, **res)
    assert kernel == twin_kernel and not kernel.startswith("dense_"), (what, kernel, twin_kernel)
    assert np.array_equal(got, activation(fn, pre, 4)) and Q.same_bits(got, twin), what


def test_quantized_dense_layer_of_272_units_runs_on_the_route():
    N, K, U = 17, 192, 272
    rng = np.random.default_rng(5)
    x = Q.grid_values((N, K), 4, 5)
    dense = qnn_amd.QuantizedDense(U, nb=4, input_domain=("quantized", 4))
    dense.build((None, K))
    dense.set_weights([rng.uniform(-1, 1, (K, U)).astype(F32), (rng.standard_normal(U) * 0.05).astype(F32)])
    got = host(dense(dev(x)))
    assert _abi.last_kernel() == "dense_mfma_i4", _abi.last_kernel()
    assert Q.same_bits(got, O.quantized_dense_call(x, *dense.get_weights(), nb=4))

"""k_dense_mfma (csrc/qnn_dense_mfma.hip) on the cases of dense_mfma_cases.py: its own copy of the chain epilogue on exact
ties, zeros and clip edges (group A), every tile width and K split on every (operand store, output store) pair (B),
saturated operands up to the route's cin limit (C) and narrow operands of every weight kind (D).  Each case runs under the
default preference and on its VALU twin; packed outputs are pre-filled with PACKED_FILL; the comparison with the integer /
float64 reference and with the twin is bit for bit, the sign of zero included.

The kernel name says dense_mfma_i4 / _i8 / _bin, not which instantiation or split ran: this file cannot see NT or ks.  That a
case's shape makes the host plan choose them is proven without a GPU: test_dense_plan.py holds dense_mfma_cases.plan() to
the C++ header the route calls, and test_dense_mfma_cases_cpu.py holds the table to plan() -- all 24 (XS, OUT, NT)
instantiations, all nine (NT, ks) and the K shares.

The file is named to be collected behind test_gpu_wide_dense_mfma.py, so that earlier GPU ids keep their places in a run."""
import ctypes

import numpy as np
import pytest
import torch

from qnn_amd import _abi, engine
import dense_mfma_cases as M
import qrelu_cases as Q
import tail_cases as T

pytestmark = pytest.mark.gpu
FN = {"none": _abi.FN_NONE, M.BT: _abi.FN_BINARY_TANH, M.QT: _abi.FN_QUANTIZED_TANH, M.RELU: _abi.FN_QUANTIZED_RELU,
      M.LEAKY: _abi.FN_QUANTIZED_LEAKYRELU}
WKIND = {"binary": _abi.W_BINARY, "ternary": _abi.W_TERNARY, "quantized": _abi.W_QUANT}
KERNEL = {M.I4: "dense_mfma_i4", M.I8: "dense_mfma_i8", M.BIN: "dense_mfma_bin"}
CASES = M.cases()


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def host(t):
    torch.cuda.synchronize()
    return t.detach().cpu().numpy()


class Call:
    """A case's handle, epilogue constants and packed input on the device (built as test_gpu_tail.py builds them)."""

    def __init__(self, c):
        d = M.layer(c)[0]
        self.c = c
        self.w = _abi.Weights(WKIND[c["wkind"]], int(c["wbits"]) if c["wkind"] == "quantized" else 1, 1.0, dev(d["kernel"]),
                              dev(d["bias"]) if d["bias"] is not None else None, 1, True, c["x_store"])
        self.inv = self.shift = None
        if d["bn"] is not None:
            self.inv, self.shift = (dev(a) for a in engine.bn_constants(d["bn"]))
        self.x = dev(T.pack_words(d["codes"], c["x_store"]).view(np.int32))

    def run(self, fn, nb):
        """(kernel name, float32 (N, units)); a packed output is decoded with qnn_unpack_f32."""
        c = self.c
        N, U, out = c["N"], c["units"], c["out_store"]
        packed = out != M.SF32
        if packed:
            y = torch.full((N, T.words(out, U)), T.PACKED_FILL, dtype=torch.int32, device="cuda")
        else:
            y = torch.full((N, U), float("nan"), dtype=torch.float32, device="cuda")
        epi = _abi.make_epilogue(self.inv, self.shift, FN[fn], nb, 1, out)
        _abi.check(_abi.load().qnn_dense_forward(self.w.handle, _abi.ptr(self.x), c["x_store"], c["x_bits"], N, ctypes.byref(epi),
                                                 _abi.ptr(y), _abi.stream_ptr()), "qnn_dense_forward")
        kernel = _abi.last_kernel()
        return kernel, host(_abi.unpack(y, N, U, out, nb or 1) if packed else y)

    def both(self, fn, nb):
        """The call under the default preference and on its VALU twin."""
        try:
            got = self.run(fn, nb)
            _abi.set_conv_impl(_abi.IMPL_VALU)
            return got, self.run(fn, nb)
        finally:
            _abi.set_conv_impl(_abi.IMPL_AUTO)


@pytest.mark.parametrize("c", CASES, ids=[c["id"] for c in CASES])
def test_dense_mfma_case_has_the_reference_bits_and_the_twin_s(c):
    call = Call(c)
    for fn, nb in c["acts"]:
        (kernel, got), (twin_kernel, twin) = call.both(fn, nb)
        what = "%s %s(%d): %s / %s" % (c["id"], fn, nb, kernel, twin_kernel)
        if c["on_route"]:
            assert kernel == KERNEL[c["x_store"]], what
        else:
            assert not kernel.startswith("dense_mfma"), what
        assert not twin_kernel.startswith("dense_mfma"), what
        want = M.reference(c, fn, nb)
        assert Q.same_bits(got, want), (what, int(np.count_nonzero(got.view(np.int32) != want.view(np.int32))))
        assert Q.same_bits(got, twin), (what, int(np.count_nonzero(got.view(np.int32) != twin.view(np.int32))))

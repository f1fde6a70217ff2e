"""The cases of sideconv_grid_cases.py on the GPU: each (op, kernel form, epilogue, BN sign) through qnn_depthwise_forward,
qnn_gconv_forward or qnn_tconv_forward with the harness of the three side convolutions' own GPU files (the FILL pattern
under the output, the input's spare bits set), the kernel name asserted, the output equal to the oracle's bit for bit, the
spare bits of the last word zero and no FILL word left.  A fast-form case also runs its plain twin (the same codes written
to another store) and compares the two.  This file holds no test id of its own: every group of the table (one form on one
shape) runs behind a test_epilogues id of test_gpu_depthwise.py, test_gpu_gconv.py or test_gpu_tconv.py on the same input
store (run_hosted; test_sideconv_grid_cpu.py holds that every group has such a host), whether or not the hosting case
holds, and a failure names its cases.  Run as a script, the file takes the cases on their own, all or those whose id holds
a given string.  test_sideconv_grid_cpu.py proves that these cases could fail: each holds the ties, zeros and clip edges
that a wrong rounding, threshold, clip or per-field constant changes."""
import os
import sys

import numpy as np
import pytest
import torch

if __name__ == "__main__":          # run as a script: the repository root (qnn_amd, oracle) is not on the path yet
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from qnn_amd import _abi

import depthwise_cases as D
import sideconv_grid_cases as S

pytestmark = pytest.mark.gpu
ENTRIES = _abi.EXPORTS_DEPTHWISE, _abi.EXPORTS_GCONV, _abi.EXPORTS_TCONV          # read at import
FILL = 0x5A5A5A5A


def dev(a):
    a = np.array(a, order="C")
    t = torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).cuda()
    assert t.data_ptr() % 16 == 0
    return t


def host(t):
    torch.cuda.synchronize()
    a = t.detach().cpu().numpy()
    return a.view(np.uint32) if a.dtype == np.int32 else a


def handle(c, kernel, bias):
    head = (c["wkind"], c["wbits"], 1.0, dev(kernel), dev(bias))
    if c["op"] == "dw":
        return _abi.DepthwiseWeights(*head, c["stride"], c["same"], c["store"], dilation=c["dil"])
    if c["op"] == "gc":
        return _abi.GConvWeights(*head, c["groups"], c["stride"], c["same"], c["store"], dilation=c["dil"])
    return _abi.TConvWeights(*head, c["stride"], c["same"], c["store"])


FORWARD = {"dw": _abi.depthwise, "gc": _abi.gconv, "tc": _abi.tconv}


def run(c):
    """One forward call of case c, checked against the oracle; returns the output as S.stored() shapes it."""
    x, kernel, bias, bn = S.inputs(c)
    want = S.stored(c, S.expected(c))
    N, H, W = c["map"]
    cout = S.cout_of(c)
    w = handle(c, kernel, bias)
    np.testing.assert_array_equal(host(w.dequant()).view(np.uint32), S.base(c)["wq"].view(np.uint32))
    if c["store"] == D.F32:
        xd = dev(x)
    else:
        xd = dev(D.encode(x, c["store"], spare=np.random.RandomState(7)).reshape(N * H * W, -1))
    Ho, Wo = want.shape[1:3]
    assert (Ho, Wo) == w.out_hw(H, W)
    if c["out_store"] == D.F32:
        shape, dt = (N, Ho, Wo, cout), np.float32
    else:
        shape, dt = (N * Ho * Wo, D.words(c["out_store"], cout)), np.uint32
    out = dev(np.full(shape, FILL, np.uint32).view(dt))
    bnd = (dev(bn[0]), dev(bn[1])) if bn is not None else (None, None)
    y, ho, wo = FORWARD[c["op"]](w, xd, c["store"], c["x_bits"], N, H, W, bnd[0], bnd[1], c["fn"], c["act_bits"],
                                 c["out_store"], out=out)
    assert _abi.last_kernel() == c["form"]
    assert (ho, wo) == (Ho, Wo)
    got = host(y)
    assert not (got.view(np.uint32) == FILL).any(), "an output word was not written"
    if c["out_store"] == D.F32:
        np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32))
        return got
    codes, spare = D.decode(got.reshape(N, Ho, Wo, -1), c["out_store"], cout)
    np.testing.assert_array_equal(codes, want)
    assert not spare.any(), "spare bits of the last word are not zero"
    return codes


def as_codes(c, out):
    """The output of run(c) as the integer codes of the case's activation (binary_tanh: -1 / +1), whatever its store."""
    if c["out_store"] == D.F32:
        return np.rint(out.astype(np.float64) * 2.0 ** max(c["act_bits"] - 1, 0)).astype(np.int64)
    return 2 * out - 1 if c["out_store"] == D.BIN else out


_DONE = {}          # case id -> codes of a case that ran and held (a twin runs once, whichever of the pair comes first)


def check(c):
    if c["id"] not in _DONE:
        _DONE[c["id"]] = as_codes(c, run(c))
    t = S.twin(c)
    if t is not None:
        check(t)
        assert t["form"].endswith("_plain")
        np.testing.assert_array_equal(_DONE[c["id"]], _DONE[t["id"]], err_msg="fast and plain form differ")


def run_cases(cases):
    """check() on every case; the failures together, each under its case id (form, shape, fn and width, out_store, BN sign)."""
    failures = []
    for c in cases:
        try:
            check(c)
        except AssertionError as e:
            failures.append("%s: %s" % (c["id"], " ".join(str(e).split())[:300]))
    assert not failures, "sideconv grid, %d of %d cases:\n%s" % (len(failures), len(cases), "\n".join(failures))


def run_hosted(op, host_stores, host):
    """The grid groups that test_epilogues id number `host` of the op's GPU file carries (S.hosted)."""
    run_cases([c for g in S.hosted(op, host_stores)[host] for c in S.group_cases(g)])


if __name__ == "__main__":
    # python tests/test_gpu_sideconv_grid.py [substring of the case ids]: the cases on their own, with the time they take
    import time
    pick = [c for c in S.cases() if not sys.argv[1:] or sys.argv[1] in c["id"]]
    t0 = time.time()
    run_cases(pick)
    print("%d cases held in %.1f s" % (len(pick), time.time() - t0))

"""The spec op {"op": "merge", "fn": ..., "srcs": [...]} on the engines, against a numpy reference written in this file, bit for
bit: four hand-written networks on GraphModel (the kernel_log names the merge kernel each takes) and on LayerModel, one of
them captured with torch.cuda.graph and replayed on fresh images, the refusal of the fused engines and nets.Model's choice
of GraphModel.  The checks below run in turn as ONE test, test_the_merge_spec_op: the suite's list of GPU test ids stays
short; every assertion names its spec.

  gate     two 3 x 3 binary convs + binary_tanh -> mul -> binary conv: the codes stay BIN (merge_bin, no unpack)
  maxout   two 4-bit convs + quantized_tanh(4) -> max -> 4-bit conv: the codes stay I4 (merge_i4, no unpack)
  average  three float32 branches (conv + BN, no clip) -> avg -> flatten -> dense: merge_f32
  diff     two 4-bit code branches -> sub -> quantized_tanh(4) -> conv: merge_i4_f32, the clip fused into the consumer's pack

The reference walks the spec: a merge op is merge_cases.ref_f32 on the float32 tensors, every other op is
spec_graph_cases.reference on that op alone.  The images are 2 x 8 x 8 on k / 8, the weights on their grids, so every
contraction behind a clip is exact in any order (guard() checks it); the dense layer behind the average reads values that
are no longer dyadic and is accumulated in float64 with one rounding by the kernel and by the oracle alike."""
import numpy as np
import pytest
import torch

import qnn_amd                                   # noqa: F401
from qnn_amd import _abi, engine, nets

import merge_cases as M
import spec_graph_cases as S

pytestmark = pytest.mark.gpu
F32 = np.float32
ENTRIES = _abi.EXPORTS_MERGE             # read at import: without the entries and the op nothing below means anything
N = 2


def dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()


def host(t):
    torch.cuda.synchronize()
    return t.detach().cpu().numpy()


def images(seed=77):
    return (np.random.default_rng(seed).integers(0, 9, (N, 8, 8, 3)) / 8.0).astype(F32)


class Net(S.Net):
    def merge(self, fn, srcs, dst):
        assert len({self.shape[s] for s in srcs}) == 1
        self.spec.append({"op": "merge", "fn": fn, "srcs": list(srcs), "dst": dst})
        self.shape[dst] = self.shape[srcs[0]]
        self.cur = dst
        return dst


def gate():
    net = Net(41)
    a0 = net.clipped(16, "bin", "bin", dst="a0")
    g1 = net.clipped(16, "bin", "bin", src=a0, dst="g1")
    g2 = net.clipped(16, "bin", "bin", src=a0, dst="g2")
    net.merge("mul", [g1, g2], "m")
    net.clipped(16, "bin", "bin", dst="a3")
    net.classifier("binary", 1)
    return net.spec


def maxout():
    net = Net(42)
    a0 = net.clipped(16, "q4", "q4", dst="a0")
    g1 = net.clipped(32, "q4", "q4", src=a0, dst="g1")
    g2 = net.clipped(32, "q4", "q4", src=a0, dst="g2")
    net.merge("max", [g1, g2], "m")
    net.clipped(16, "q4", "q4", dst="a3")
    net.classifier()
    return net.spec


def average():
    net = Net(43)
    a0 = net.clipped(16, "q4", "q4", dst="a0")
    branches = []
    for i in range(3):
        net.conv(16, "quantized", 4, src=a0, dst="c%d" % i)
        branches.append(net.bn(dst="f%d" % i))
    net.merge("avg", branches, "m")
    net.flatten()
    net.dense(10, "quantized", 4, bias=True)
    return net.spec


def diff():
    net = Net(44)
    a0 = net.clipped(16, "q4", "q4", dst="a0")
    g1 = net.clipped(24, "q4", "q4", src=a0, dst="g1")
    g2 = net.clipped(24, "q4", "q4", k=1, src=a0, dst="g2")
    net.merge("sub", [g1, g2], "m")
    net.act("quantized_tanh", 4, dst="d")
    net.clipped(16, "q4", "q4", dst="a3")
    net.classifier()
    return net.spec


# name -> (spec, the merge kernel GraphModel's kernel_log names, True if no packed tensor is unpacked on the way)
SPECS = {"gate": (gate(), "merge_bin", True), "maxout": (maxout(), "merge_i4", True),
         "average": (average(), "merge_f32", False), "diff": (diff(), "merge_i4_f32", True)}


def reference(spec, x, return_all=False):
    names = S.names_of(spec)
    env, cur = {"input": np.asarray(x, dtype=F32)}, np.asarray(x, dtype=F32)
    for i, op in enumerate(spec):
        if op["op"] == "merge":
            y = M.ref_f32(op["fn"], [env[s] for s in op["srcs"]])
        else:
            src = env[op["src"]] if "src" in op else cur
            y = S.reference([{k: v for k, v in op.items() if k not in ("src", "dst")}], src)
        env[names[i]] = cur = np.asarray(y, dtype=F32)
    return env if return_all else cur


def guard(spec, x):
    """None where every contraction that reads dyadic values is exact in any order (spec_graph_cases.guard's rule), else
    why not; a contraction behind the average is not held to it (module docstring)."""
    env, names = reference(spec, x, return_all=True), S.names_of(spec)
    for i, op in enumerate(spec):
        if op["op"] not in ("conv", "dense"):
            continue
        src = env[op["src"]] if "src" in op else env[names[i - 1]] if i else env["input"]
        try:
            xc, a = S._codes(src, "input of op %d" % i)
        except ValueError:
            if any(o["op"] == "merge" and o["fn"] == "avg" for o in spec[:i]):
                continue
            return "op %d reads values that are not dyadic" % i
        wc, b = S._codes(S.weights(op), "weights of op %d" % i)
        if S._contract(np.abs(xc), np.abs(wc), op).max(initial=0) >= 2 ** 24:
            return "op %d: partial sums may pass 2^24 units" % i
    return None


def check_graph_model_runs_the_merge(name):
    spec, kernel, packed = SPECS[name]
    x = images()
    assert guard(spec, x) is None
    m = engine.GraphModel(spec)
    m.kernel_log = []
    got = host(m(dev(x)))
    assert kernel in m.kernel_log and [k for k in m.kernel_log if k.startswith("merge")] == [kernel], m.kernel_log
    if packed:
        assert "unpack" not in m.kernel_log, m.kernel_log
    want = reference(spec, x)
    assert got.shape == want.shape == (N, 10)
    np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32))
    assert np.unique(got).size > 5                       # (not a constant network)


def check_the_merged_tensor_is_what_the_table_says():
    """What the op hands on: packed codes of the sources' store and width (mul of BIN, max of I4), float32 otherwise; sources
    of different widths, or a plain tensor among them, go through float32."""
    m = engine.GraphModel(SPECS["maxout"][0])
    m.kernel_log = []
    shape = (2, 4, 4, 12)
    ka, kb = M.codes("i4", 4, 32, 12, 1), M.codes("i4", 4, 32, 12, 2)
    a = engine._Packed(dev(M.encode(ka, "i4").view(np.int32)), _abi.STORE_I4, 4, shape)
    b = engine._Packed(dev(M.encode(kb, "i4").view(np.int32)), _abi.STORE_I4, 4, shape)
    y = m._merge([a, b], {"op": "merge", "fn": "max"})
    assert isinstance(y, engine._Packed) and (y.store, y.bits, y.shape, y.grid) == (_abi.STORE_I4, 4, shape, False)
    np.testing.assert_array_equal(host(y.t).view(np.uint32), M.encode(np.maximum(ka, kb), "i4"))
    y = m._merge([a, b], {"op": "merge", "fn": "sub"})
    assert isinstance(y, torch.Tensor) and y.shape == shape
    assert M.same_f32(host(y).reshape(32, 12), M.ref_f32("sub", [M.values(ka, "i4", 4), M.values(kb, "i4", 4)]))
    assert m.kernel_log == ["merge_i4", "merge_i4_f32"]
    # another width, ternary values beside a clip's codes, a plain tensor: float32
    b3 = engine._Packed(b.t, _abi.STORE_I4, 3, shape)
    bg = engine._Packed(b.t, _abi.STORE_I4, 4, shape)
    bg.grid = True
    for other in (b3, bg, b.to_f32()):
        m.kernel_log = []
        y = m._merge([a, other], {"op": "merge", "fn": "max"})
        assert isinstance(y, torch.Tensor) and m.kernel_log == ["unpack", "merge_f32"]
        assert torch.equal(y, torch.maximum(a.to_f32(), m._plain(other)))
    # clips that are not materialised are packed first: the same codes as the materialised clip's
    op = {"op": "act", "fn": "quantized_tanh", "nb": 4}
    pre = dev(np.linspace(-1.5, 1.5, 2 * 4 * 4 * 12, dtype=F32).reshape(shape))
    va, vb = engine._Virtual(pre, _abi.FN_QUANTIZED_TANH, 4, op), engine._Virtual(-pre, _abi.FN_QUANTIZED_TANH, 4, op)
    m.kernel_log = []
    y = m._merge([va, vb], {"op": "merge", "fn": "min"})
    assert isinstance(y, engine._Packed) and m.kernel_log == ["merge_i4"]
    assert torch.equal(y.to_f32(), torch.minimum(va.materialize(), vb.materialize()))
    with pytest.raises(_abi.QnnError, match="identical shapes"):
        m._merge([a, engine._Packed(b.t, _abi.STORE_I4, 4, (2, 4, 2, 24))], {"op": "merge", "fn": "max"})


def check_layer_model_runs_the_merge_in_float32(name):
    spec = SPECS[name][0]
    x = images(78)
    assert guard(spec, x) is None
    got = host(engine.LayerModel(spec)(dev(x)))
    np.testing.assert_array_equal(got.view(np.uint32), reference(spec, x).view(np.uint32))


def check_a_captured_graph_replays_on_fresh_images():
    spec = SPECS["maxout"][0]
    gm = engine.GraphModel(spec)
    xs = dev(images(1))
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        gm(xs)                                       # prepacks the weights outside the capture
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ys = gm(xs)
    for seed in (2, 3):
        x2 = images(seed)
        assert guard(spec, x2) is None
        xs.copy_(dev(x2))
        graph.replay()
        np.testing.assert_array_equal(host(ys).view(np.uint32), reference(spec, x2).view(np.uint32))


def check_the_fused_engines_refuse_and_the_model_takes_graph_model(name):
    spec = SPECS[name][0]
    for cls in (engine.FusedModel, engine.ResidualFusedModel):
        with pytest.raises(_abi.NotFusable, match="merge"):
            cls(spec)
    cf = nets.Config(network_type="full-qnn", wbits=4, abits=4, architecture="RESNET", nres=1, dim=8)
    model = nets.Model(cf, spec)
    assert isinstance(model.engine, engine.GraphModel)
    x = images(5)
    np.testing.assert_array_equal(host(model.engine(dev(x))).view(np.uint32), reference(spec, x).view(np.uint32))


def test_the_merge_spec_op():
    for name in SPECS:
        check_graph_model_runs_the_merge(name)
    check_the_merged_tensor_is_what_the_table_says()
    for name in SPECS:
        check_layer_model_runs_the_merge_in_float32(name)
    check_a_captured_graph_replays_on_fresh_images()
    for name in SPECS:
        check_the_fused_engines_refuse_and_the_model_takes_graph_model(name)

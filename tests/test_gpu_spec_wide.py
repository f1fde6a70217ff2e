"""GraphModel and LayerModel on the hand-written and generated specs of the wide vocabulary (spec_graph_cases.HAND_WIDE,
generate_wide: concat, crop / upsample / pair-form zeropad, dwconv, tconv) against the shared numpy reference, bit for
bit, the sign of a zero included.  Per spec: GraphModel with and without scaled codes, the launches it logs against the
restated planner (spec_graph_cases.plan) and, for the hand-written specs that carry one, against the log written out by
hand; LayerModel where the spec has no concat; the refusals of the fused engines.

A network that ends in softmax is compared on its logits bit for bit and on its probabilities within the float band
1e-5 max(1, |y|) of test_gpu_spec_graph.py."""
import contextlib

import numpy as np
import pytest
import torch

from qnn_amd import _abi, engine, nets

import spec_graph_cases as S

pytestmark = pytest.mark.gpu
SEEN = set()             # every name a GraphModel.kernel_log of this file held (test_zz_every_kernel_family_was_reached)
POOLED_BEHIND = set()    # pool_max_* names met behind a dwconv / tconv / gconv
LAUNCHERS = ("conv2d", "conv2d_f32in", "dense", "pool2d", "depthwise", "tconv", "gconv", "spatial2d", "concat", "pack",
             "unpack")
WIDE = {c["name"]: c for c in S.HAND_WIDE}


def dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()


def host(t):
    torch.cuda.synchronize()
    return t.detach().cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@contextlib.contextmanager
def counting():
    """The number of calls of the launching entries of _abi inside the block, as a one-element list."""
    n, saved = [0], {k: getattr(_abi, k) for k in LAUNCHERS}

    def wrap(fn):
        def call(*a, **kw):
            n[0] += 1
            return fn(*a, **kw)
        return call
    for k, fn in saved.items():
        setattr(_abi, k, wrap(fn))
    try:
        yield n
    finally:
        for k, fn in saved.items():
            setattr(_abi, k, fn)


def within(got, want, what):
    r = float((np.abs(got.astype(np.float64) - want) / (1e-5 * np.maximum(1.0, np.abs(want)))).max())
    assert got.shape == want.shape and r <= 1.0, "%s: max |d| / (1e-5 * max(1, |y|)) = %.3g" % (what, r)


def graph(spec, xd, scaled):
    m = engine.GraphModel(spec, scaled_codes=scaled)
    m.kernel_log = []
    return host(m(xd)), m.kernel_log


def compare(got, want, spec, what):
    assert got.shape == want.shape and got.dtype == np.float32, (what, got.shape, want.shape)
    if spec[-1]["op"] == "softmax":
        within(got, want, what)
    else:
        np.testing.assert_array_equal(bits(got), bits(want), err_msg=what)


def check(spec, x, image, what, hand_log=None, layer_model=None, same_scaled_log=False):
    """same_scaled_log: the two logs are equal although the spec holds a batch-maximum activation.  Returns the two logs,
    one after the other."""
    want, xd = S.reference(spec, x), dev(x)
    has_max = any(op["op"] == "act" and op["fn"] in S.M.FNS for op in spec)
    has_new = any(op["op"] in ("concat", "crop", "upsample", "dwconv", "tconv", "gconv") or S.spatial_desc(op) is not None
                  for op in spec)
    plain, log = graph(spec, xd, False)
    scaled, log_scaled = graph(spec, xd, True)
    compare(plain, want, spec, "%s GraphModel %s" % (what, log))
    compare(scaled, want, spec, "%s GraphModel scaled_codes %s" % (what, log_scaled))
    if not has_max or same_scaled_log:
        assert log == log_scaled, (what, log, log_scaled)
    SEEN.update(log)
    SEEN.update(log_scaled)
    # the planner's decisions: which launches, in which order, "pack" / "unpack" between them
    assert log == S.plan(spec, image)[1], (what, log)
    if hand_log is not None:
        assert log == hand_log, (what, log)
    for a, b in zip(log, log[1:]):
        if a.startswith(("depthwise_", "tconv_", "gconv_")) and b.startswith("pool_max_"):
            POOLED_BEHIND.add(b)
    # LayerModel: the same bits where the spec has no concat
    with counting() as n:
        if any(op["op"] == "concat" for op in spec):
            with pytest.raises(_abi.NotFusable, match="concat"):
                engine.LayerModel(spec)
            assert n[0] == 0, what
        elif layer_model == "float conv" or any(op["op"] in ("conv", "dense") and op["kind"] == "float" for op in spec):
            with pytest.raises(_abi.QnnError, match="low-bit layers only") as e:
                engine.LayerModel(spec)
            assert not isinstance(e.value, _abi.NotFusable) and n[0] == 0, what
        else:
            compare(host(engine.LayerModel(spec)(xd)), want, spec, what + " LayerModel")
    if has_new:
        with counting() as n:
            for cls in (engine.FusedModel, engine.ResidualFusedModel):
                with pytest.raises(_abi.NotFusable):
                    cls(spec)
            assert n[0] == 0, what
        # (a generated network that drew none of the new ops is one the fused engines take: nets.Model picks them)
        assert isinstance(nets.Model(None, spec).engine, engine.GraphModel), what
    if spec[-1]["op"] == "softmax":          # ... and the logits in front of it, bit for bit
        check(spec[:-1], x, image, what + " logits", same_scaled_log=same_scaled_log)
    return log + log_scaled


@pytest.mark.parametrize("name", list(WIDE))
def test_hand_written_wide_spec(name):
    c = WIDE[name]
    check(c["spec"], c["x"], c["image"], name, c["log"], c["layer_model"])


@pytest.mark.parametrize("seed", list(S.SEEDS_WIDE))
def test_generated_wide_spec(seed):
    spec, x, image = S.generate_wide(seed)
    why = S.guard(spec, x)
    if why is not None:
        pytest.skip("not exact by construction: %s" % why)
    check(spec, x, image, "seed %d" % seed)


def other_images(x):
    """Other images on the same grid k / 8."""
    return np.ascontiguousarray(np.roll(x, 3, axis=2)[::-1, ::-1])


@pytest.mark.parametrize("name", S.CAPTURED)
def test_captured_forward_replays_on_other_images(name):
    """tconv across a skip, a dwconv block and a ternary concat, captured into a graph and replayed in the same buffers."""
    c = WIDE[name]
    spec, x = c["spec"], c["x"]
    x2 = other_images(x)
    assert S.guard(spec, x2) is None and not np.array_equal(x, x2)
    gm = engine.GraphModel(spec)
    xs = dev(x)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        gm(xs)                               # prepacks the weights outside the capture
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ys = gm(xs)                          # (recorded, not run)
    g.replay()
    np.testing.assert_array_equal(bits(host(ys)), bits(S.reference(spec, x)))
    xs.copy_(dev(x2))
    g.replay()
    np.testing.assert_array_equal(bits(host(ys)), bits(S.reference(spec, x2)))


# ---- the kernels this file must have reached (runs last: pytest keeps file order) -------------------------------------
def test_zz_every_kernel_family_was_reached():
    """Needs the tests above in the same process: run the file as a whole."""
    need = ["%s_%s" % (f, s) for f in ("spatial", "concat") for s in ("f32", "bin", "i4", "i8", "t2")]
    need += ["tconv_i4_plain", "tconv_i4_mfma", "tconv_i8_mfma", "depthwise_i4", "depthwise_i4_plain", "depthwise_i8_plain"]
    for k in need:
        assert k in SEEN, (k, sorted(SEEN))
    assert POOLED_BEHIND, sorted(SEEN)

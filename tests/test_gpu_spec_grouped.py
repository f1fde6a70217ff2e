"""GraphModel and LayerModel on the hand-written and generated specs around the grouped convolution
(spec_graph_cases.HAND_GROUPED, generate_grouped) against the shared numpy reference, bit for bit.  The comparisons per
spec are those of test_gpu_spec_wide.check: GraphModel with and without scaled codes, its kernel_log against the restated
planner and against the logs written out by hand, LayerModel where the spec has no concat, the refusals of the fused
engines without a launch, nets.Model's choice of GraphModel."""
import numpy as np
import pytest
import torch

from qnn_amd import engine

import spec_graph_cases as S
import test_gpu_spec_wide as W

pytestmark = pytest.mark.gpu
SEEN = set()             # every name a GraphModel.kernel_log of this file held
POOLED_BEHIND = set()    # pool_max_* names met right behind a gconv
GROUPED = {c["name"]: c for c in S.HAND_GROUPED}


def run(spec, x, image, what, **kw):
    log = W.check(spec, x, image, what, **kw)
    SEEN.update(log)
    POOLED_BEHIND.update(b for a, b in zip(log, log[1:]) if a.startswith("gconv_") and b.startswith("pool_max_"))


@pytest.mark.parametrize("name", list(GROUPED))
def test_hand_written_grouped_spec(name):
    c = GROUPED[name]
    run(c["spec"], c["x"], c["image"], name, hand_log=c["log"], layer_model=c["layer_model"],
        same_scaled_log=c["same_scaled_log"])


@pytest.mark.parametrize("seed", list(S.SEEDS_GROUPED))
def test_generated_grouped_spec(seed):
    spec, x, image = S.generate_grouped(seed)
    why = S.guard(spec, x)
    if why is not None:
        pytest.skip("not exact by construction: %s" % why)
    run(spec, x, image, "seed %d" % seed)


@pytest.mark.parametrize("name", S.CAPTURED_GROUPED)
def test_captured_forward_replays_on_other_images(name):
    """The int4 bottleneck with its add and the ShuffleNet join, captured into a graph on one stream and replayed in the
    same buffers."""
    c = GROUPED[name]
    spec, x = c["spec"], c["x"]
    x2 = W.other_images(x)
    assert S.guard(spec, x2) is None and not np.array_equal(x, x2)
    assert any(op["op"] == "gconv" for op in spec)
    gm = engine.GraphModel(spec)
    xs = W.dev(x)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        gm(xs)                               # prepacks the weights outside the capture
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ys = gm(xs)                          # (recorded, not run)
    g.replay()
    np.testing.assert_array_equal(W.bits(W.host(ys)), W.bits(S.reference(spec, x)))
    xs.copy_(W.dev(x2))
    g.replay()
    np.testing.assert_array_equal(W.bits(W.host(ys)), W.bits(S.reference(spec, x2)))


# ---- the kernels this file must have reached (runs last: pytest keeps file order) -------------------------------------
def test_zz_every_gconv_kernel_was_reached():
    """Needs the tests above in the same process: run the file as a whole."""
    for k in S.GCONV_LAUNCHES:
        assert k in SEEN, (k, sorted(SEEN))
    assert POOLED_BEHIND, sorted(SEEN)

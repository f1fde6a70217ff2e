"""The spec engines on the hand-written and generated specs of spec_graph_cases.py, against its numpy reference, bit for
bit: GraphModel, LayerModel, ResidualFusedModel under every fold / fuse_projection / fuse_tail setting and FusedModel
where it takes the spec (NotFusable, and nothing else, where it does not).  Every model runs first_layer="exact".

A network that ends in softmax is compared on its logits bit for bit and on its probabilities within the float band
1e-5 max(1, |y|); the two LeakyReLU cases (float32 activations, not on a grid) use that band throughout."""
import contextlib
import itertools

import numpy as np
import pytest
import torch

from qnn_amd import _abi, engine

import spec_graph_cases as S

pytestmark = pytest.mark.gpu
F32 = np.float32
SEEN = set()             # every kernel name a case of this file met (test_zz_every_kernel_family_was_reached)
ENTRIES = ("conv2d", "conv2d_f32in", "conv2d_dense", "dense", "pool2d", "avgpool_packed", "avgpool_dense_softmax")
SETTINGS = list(itertools.product((True, False), repeat=3))       # fold, fuse_projection, fuse_tail
HAND = {c["name"]: c for c in S.HAND}


def dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()


def host(t):
    torch.cuda.synchronize()
    return t.detach().cpu().numpy()


@contextlib.contextmanager
def recording():
    """[(entry of _abi, kernel it launched)] for every launch inside the block: the engines and the layer classes call
    the entries through the module, so wrapping its attributes sees them all."""
    log, saved = [], {n: getattr(_abi, n) for n in ENTRIES}

    def wrap(name, fn):
        def call(*a, **kw):
            y = fn(*a, **kw)
            if y is not None:
                log.append((name, _abi.last_kernel()))
            return y
        return call
    for n, fn in saved.items():
        setattr(_abi, n, wrap(n, fn))
    try:
        yield log
    finally:
        for n, fn in saved.items():
            setattr(_abi, n, fn)
        SEEN.update(k for _, k in log)


def within(got, want, what):
    r = float((np.abs(got.astype(np.float64) - want) / (1e-5 * np.maximum(1.0, np.abs(want)))).max())
    assert got.shape == want.shape and r <= 1.0, "%s: max |d| / (1e-5 * max(1, |y|)) = %.3g" % (what, r)


def residual(spec, fold=True, fuse_projection=True, fuse_tail=True):
    m = engine.ResidualFusedModel(spec, first_layer="exact", fold=fold, fuse_projection=fuse_projection)
    m.fuse_tail = fuse_tail
    return m


def run_engines(spec, x):
    """{engine label: output, or the NotFusable / "low-bit layers only" refusal it raised}, {label: launches}.  Any
    other exception from an engine on a legal spec fails the test here."""
    xd, out, logs = dev(x), {}, {}

    def run(label, make):
        with recording() as log:
            try:
                out[label] = host(make()(xd))
            except _abi.NotFusable as e:
                out[label] = e
            except _abi.QnnError as e:
                if label != "LayerModel" or "low-bit layers only" not in str(e):
                    raise
                out[label] = e
        logs[label] = log
    run("GraphModel", lambda: engine.GraphModel(spec))
    run("LayerModel", lambda: engine.LayerModel(spec))
    for s in SETTINGS:
        run("ResidualFusedModel fold=%d proj=%d tail=%d" % s, lambda: residual(spec, *s))
    run("FusedModel", lambda: engine.FusedModel(spec, first_layer="exact"))
    return out, logs


def check(spec, x, exact, fused, float_layers=False, max_acts=False, what=""):
    """Every engine on `spec` against the reference; returns the launches per engine."""
    want = S.reference(spec, x)
    out, logs = run_engines(spec, x)
    band = not exact or spec[-1]["op"] == "softmax"
    for label, got in out.items():
        refusal = None
        if label == "LayerModel" and float_layers:
            refusal = _abi.QnnError
        elif label.startswith("ResidualFusedModel") and max_acts:
            refusal = _abi.NotFusable
        elif label == "FusedModel" and (fused in (S.NO_GROUP, S.NO_CTOR) or (fused is None and isinstance(got, Exception))):
            refusal = _abi.NotFusable
        if refusal is not None:
            assert isinstance(got, refusal) and (refusal is _abi.NotFusable or not isinstance(got, _abi.NotFusable)), \
                "%s %s: expected %s, got %r" % (what, label, refusal.__name__, got)
            assert logs[label] == [], (what, label, logs[label])          # a refusal launches nothing
            continue
        assert not isinstance(got, Exception), "%s %s: %r" % (what, label, got)
        assert got.shape == want.shape and got.dtype == np.float32, (what, label, got.shape, want.shape)
        if band:
            within(got, want, "%s %s" % (what, label))
        else:
            np.testing.assert_array_equal(got, want, err_msg="%s %s %s" % (what, label, [k for _, k in logs[label]]))
    if spec[-1]["op"] == "softmax":          # ... and the logits in front of it, bit for bit (or in the band, as above)
        check(spec[:-1], x, exact, fused, float_layers, max_acts, what + " logits")
    return logs


def kernels(log, *entries):
    return [k for e, k in log if not entries or e in entries]


@pytest.mark.parametrize("name", list(HAND))
def test_hand_written_spec_on_every_engine(name):
    case = HAND[name]
    spec = case["spec"]
    logs = check(spec, case["x"], case["exact"], case["fused"], case.get("float_layers", False), case.get("max_acts", False), name)
    on = kernels(logs["ResidualFusedModel fold=1 proj=1 tail=1"])
    no_proj = kernels(logs["ResidualFusedModel fold=1 proj=0 tail=1"])
    no_tail = kernels(logs["ResidualFusedModel fold=1 proj=1 tail=0"])
    nconv = sum(op["op"] == "conv" for op in spec)
    for k in case.get("kernels", ()):
        assert k in on, (k, on)
    if case.get("projection") == "fused":      # the shortcut conv runs inside the main conv's launch: one launch fewer
        assert sum(k.endswith("_proj") for k in on) == 1 and "pw_i4_f32" not in on, on
        assert any(k in ("strip_i4_c32_proj", "strip_i4_c64_proj") for k in on), on
        assert len(kernels(logs["ResidualFusedModel fold=1 proj=1 tail=1"], "conv2d", "conv2d_f32in")) == nconv - 1
        assert "pw_i4_f32" in no_proj and not any(k.endswith("_proj") for k in no_proj), no_proj
    elif case.get("projection") is not None:   # a near miss: two launches, the 1 x 1 ones on the pointwise kernel
        for label in ("ResidualFusedModel fold=1 proj=1 tail=1", "ResidualFusedModel fold=1 proj=0 tail=1"):
            ks = kernels(logs[label])
            assert not any(k.endswith("_proj") for k in ks), ks
            assert case["projection"] != "pw" or "pw_i4_f32" in ks, ks
            assert len(kernels(logs[label], "conv2d", "conv2d_f32in")) == nconv, ks
    if "packed_pools" in case:                 # pooled on the codes, and no conv launched twice or through float32
        for label in ("GraphModel", "ResidualFusedModel fold=1 proj=1 tail=1", "ResidualFusedModel fold=0 proj=0 tail=0"):
            assert [k for k in kernels(logs[label]) if k.startswith("pool_")] == case["packed_pools"], (label, logs[label])
        assert len(kernels(logs["ResidualFusedModel fold=1 proj=1 tail=1"], "conv2d", "conv2d_f32in")) == nconv, on
    if case.get("tail") is not None:
        t = case["tail"]
        assert on.count(t) == 1, (t, on)
        if t.startswith("tail_avg"):           # one launch; with fuse_tail off the ops run one by one
            assert kernels(logs["GraphModel"]).count(t) == 1, logs["GraphModel"]
            assert "dense_f32" not in on and not any(k.startswith("tail_") for k in no_tail) and "dense_f32" in no_tail, no_tail
        else:
            assert not any(k.startswith("tail_") for k in on), on
    elif "tail" in case:
        assert not any(k.startswith("tail_") for k in on), on
    if case.get("flatten_dense"):              # the dense behind the flatten reads the packed codes
        for label in ("ResidualFusedModel fold=1 proj=1 tail=1", "ResidualFusedModel fold=0 proj=0 tail=0"):
            ks = kernels(logs[label], "dense")
            assert len(ks) == 1 and ks[0] != "dense_f32", (label, logs[label])


@pytest.mark.parametrize("seed", list(S.SEEDS))
def test_generated_spec_on_every_engine(seed):
    spec, x = S.generate(seed)
    why = S.guard(spec, x)
    if why is not None:
        pytest.skip("not exact by construction: %s" % why)
    fused = None if S.chain(spec) else S.NO_GROUP
    check(spec, x, True, fused, what="seed %d" % seed)


@pytest.mark.parametrize("name", S.PIPELINED)
def test_pipelined_replay_and_ragged_tail_have_the_eager_bits(name):
    """N = 3 in batches of 2 on two lanes: one captured replay and a ragged tail of one image."""
    case = HAND[name]
    xd = dev(case["x"])
    model = residual(case["spec"])
    eager = host(model(xd))
    np.testing.assert_array_equal(eager, S.reference(case["spec"], case["x"]))
    pipe = engine.Pipelined(residual(case["spec"]), lanes=2, batch_size=2)
    got = host(pipe(xd))
    # (a network whose activations are batch statistics would differ per batch: none of the three has one)
    assert not any(op["op"] == "act" and op["fn"] in ("ternary_tanh",) + S.M.FNS for op in case["spec"])
    np.testing.assert_array_equal(got, eager)
    pipe.clear()


# ---- the kernels this file must have reached (runs last: pytest keeps file order) -------------------------------------
def test_zz_every_kernel_family_was_reached():
    """Needs the tests above in the same process: run the file as a whole."""
    for need in ("strip_i4_c16", "strip_i4_c32_proj", "pool_max_bin", "pool_max_i4", "dense_i4", "dense_bin",
                 "tail_avg_dense", "generic"):
        assert need in SEEN, (need, sorted(SEEN))

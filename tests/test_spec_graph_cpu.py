"""spec_graph_cases.py on the CPU: its reference against the oracle's own interpreter wherever that one knows the ops and
against torch in float64 on the geometries the hand-written specs use; every hand-written and generated spec legal,
deterministic and exact by construction (guard); the category list covered; FusedModel._group's decision pinned."""
import numpy as np
import torch

from oracle import qnn_oracle as O
from qnn_amd import engine, nets

import conv_dilation_cases as D
import pool_cases as P
import spec_graph_cases as S
import test_gpu_conv_dilation as TD
import test_gpu_pool as TP

F32 = np.float32
CASES = [(c["name"], c["spec"], c["x"]) for c in S.HAND]


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


# ---- the reference --------------------------------------------------------------------------------------------------------
def test_reference_is_the_oracle_on_the_builders_specs():
    for cf in (nets.Config(network_type="full-qnn", architecture="VGG", dim=8, nfa=8, nfb=8, nfc=8),
               nets.Config(network_type="full-bnn", architecture="VGG", dim=8, nfa=8, nfb=8, nfc=8),
               nets.Config(network_type="full-qnn", architecture="RESNET", dim=32, nres=1),
               nets.Config(network_type="full-tnn", architecture="RESNET", dim=32, nres=1),
               nets.Config(network_type="qnn", architecture="RESNET", dim=32, nres=1)):
        spec = nets.build_spec(cf, seed=3)
        x = nets.synthetic_images(cf, 1, seed=1)
        want = O.run_spec(spec, x, float_conv="device", return_all=True)
        got = S.reference(spec, x, return_all=True)
        assert set(got) == set(want)
        for name in want:
            assert same_bits(got[name], want[name]), (cf.network_type, cf.architecture, name)


def test_reference_on_the_dilated_residual_twin_and_the_pool_network():
    x = (D.codes(np.random.default_rng(4), (2, 8, 8, 3), 0, 8) / 8.0).astype(F32)
    assert same_bits(S.reference(TD.residual_spec(2), x), O.run_spec(TD.residual_spec(None), x, float_conv="device"))
    spec, x = TP._net(TP.NEW_POOL), TP._images(3)
    want, want_logits = TP._composed_reference(spec, x)
    assert same_bits(S.reference(spec, x), want) and same_bits(S.reference(spec[:-1], x), want_logits)


def _tf_pad(t, kh, kw, sh, sw, same, value):
    """NCHW float64 tensor padded as TensorFlow's SAME pads it (the odd cell behind)."""
    if not same:
        return t
    _, pt, pb = O.same_padding(t.shape[2], kh, sh)
    _, pl, pr = O.same_padding(t.shape[3], kw, sw)
    return torch.nn.functional.pad(t, (pl, pr, pt, pb), value=value)


def test_convs_and_pools_agree_with_torch_float64_on_the_hand_geometries():
    seen = set()
    for name, spec, x in CASES:
        env = S.reference(spec, x, return_all=True)
        for i, (op, ss) in enumerate(zip(spec, S.sources(spec))):
            src = env[ss[0]]
            key = (op["op"], src.shape[1:], tuple(np.shape(op.get("kernel", ()))), str(op.get("strides")), op.get("padding"),
                   str(op.get("dilation_rate")), str(op.get("size")))
            if key in seen or src.ndim != 4 or op["op"] not in ("conv",) + S.POOLS:
                continue
            seen.add(key)
            t = torch.from_numpy(src.astype(np.float64)).permute(0, 3, 1, 2)
            got = env[S.names_of(spec)[i]]
            if op["op"] == "conv":
                w = S.weights(op)
                kh, kw = w.shape[:2]
                (dh, dw), (sh, sw) = S.dilation(op), op["strides"]
                tp = _tf_pad(t, D.effective(kh, dh), D.effective(kw, dw), sh, sw, op["padding"] == "same", 0.0)
                y = torch.nn.functional.conv2d(tp, torch.from_numpy(w.astype(np.float64)).permute(3, 2, 0, 1), stride=(sh, sw),
                                               dilation=(dh, dw))
                if op.get("bias") is not None:
                    y = (y.float() + torch.from_numpy(op["bias"])[None, :, None, None]).double()
                want = y.permute(0, 2, 3, 1).numpy().astype(F32)          # exact sums: float64 holds what float32 holds
            elif op["op"].startswith("global"):
                want = (t.amax(dim=(2, 3)) if op["op"] == "globalmaxpool" else
                        t.sum(dim=(2, 3)).float() / F32(t.shape[2] * t.shape[3])).numpy().astype(F32)
            else:
                mx = op["op"] == "maxpool"
                if S.new_pool(op):
                    ph, pw = P.pair(op.get("size", 2 if mx else 8))
                    sh, sw = (ph, pw) if op.get("strides") is None else P.pair(op["strides"])
                    same = op.get("padding", "valid") == "same"
                else:
                    ph = pw = sh = sw = op.get("size", 2 if mx else 8)
                    same = False
                if mx:
                    y = torch.nn.functional.max_pool2d(_tf_pad(t, ph, pw, sh, sw, same, float("-inf")), (ph, pw), (sh, sw))
                else:
                    area = float(ph * pw)
                    sums = torch.nn.functional.avg_pool2d(_tf_pad(t, ph, pw, sh, sw, same, 0.0), (ph, pw), (sh, sw)) * area
                    count = torch.nn.functional.avg_pool2d(_tf_pad(torch.ones_like(t), ph, pw, sh, sw, same, 0.0), (ph, pw),
                                                           (sh, sw)) * area
                    y = sums.float() / count.float()
                want = y.permute(0, 2, 3, 1).numpy().astype(F32)
            np.testing.assert_array_equal(got, want, err_msg="%s op %d %r" % (name, i, key))
    assert len(seen) > 40


# ---- the lists ------------------------------------------------------------------------------------------------------------
def _same_spec(a, b):
    return len(a) == len(b) and all(
        o.keys() == p.keys() and all(np.array_equal(o[k], p[k]) if isinstance(o[k], np.ndarray) else o[k] == p[k] for k in o)
        for o, p in zip(a, b))


def test_hand_specs_are_legal_and_exact_by_construction():
    assert len({n for n, _, _ in CASES}) == len(CASES)
    for case in S.HAND:
        y = S.reference(case["spec"], case["x"])
        assert y.shape[0] == S.N and y.size > 0 and np.all(np.isfinite(y)), case["name"]
        assert not case["exact"] or S.guard(case["spec"], case["x"]) is None, (case["name"], S.guard(case["spec"], case["x"]))
        assert sum(op["op"] in ("conv", "dense") for op in case["spec"]) <= 6, case["name"]
    assert [c["name"] for c in S.HAND if not c["exact"]] == ["leaky_relu_0_3", "leaky_relu_0_1"]      # the README's float band
    assert set(S.PIPELINED) <= {n for n, _, _ in CASES}


def test_generated_specs_are_legal_deterministic_and_mostly_exact():
    skipped = []
    for seed in S.SEEDS:
        spec, x = S.generate(seed)
        again, x2 = S.generate(seed)
        assert _same_spec(spec, again) and np.array_equal(x, x2), seed
        y = S.reference(spec, x)
        assert y.shape[0] == S.N == x.shape[0] and y.size > 0 and np.all(np.isfinite(y)), seed
        assert x.shape[1:] in ((8, 8, 3), (9, 7, 3)) and np.array_equal(x * 8, np.rint(x * 8)), seed
        assert sum(op["op"] in ("conv", "dense") for op in spec) <= 6, seed
        for op in spec:
            if op["op"] == "conv":
                assert set(op["kernel"].shape[2:]) <= {3, 8, 12, 16, 24, 32, 64}, seed
        if S.guard(spec, x) is not None:
            skipped.append(seed)
    assert len(S.SEEDS) == 48
    assert len(skipped) == 0, skipped        # the issue's cap is one seed in eight (6); this seed range needs none


def test_every_required_category_appears_twice():
    count = {}
    for _, spec, _ in CASES:
        for c in S.categories(spec):
            count[c] = count.get(c, 0) + 1
    for seed in S.SEEDS:
        spec, x = S.generate(seed)
        if S.guard(spec, x) is None:
            for c in S.categories(spec):
                count[c] = count.get(c, 0) + 1
    assert not {c: count.get(c, 0) for c in S.REQUIRED_OLD if count.get(c, 0) < 2}      # (REQUIRED as it was before the wide lists)
    # the generator reaches the int4 strip / fold / projection channel counts
    gen = [S.generate(s)[0] for s in S.SEEDS]
    for cin in (16, 32, 64):
        assert any(op["op"] == "conv" and op["kind"] == "quantized" and op["nb"] == 4 and op["kernel"].shape[2] == cin
                   for spec in gen for op in spec), cin
    assert any("projection eligible" in S.categories(spec) for spec in gen)


# what FusedModel._group says about each hand-written spec: the chains, as a literal
GROUP_ACCEPTS = sorted(
    ["flatten_%s_c%d" % (k, c) for k in ("q4_dense_q8", "bin_dense_q4", "bin_dense_bin") for c in (8, 12, 24, 32)] +
    ["chain_old_pools", "float_conv_mid_network", "conv_without_bn", "conv_is_last", "bn_is_last", "ternary_through_maxpool",
     "max_activations"])


def test_fusedmodel_group_decision_is_pinned():
    accepts = sorted(c["name"] for c in S.HAND if engine.FusedModel._group(c["spec"]) is not None)
    assert accepts == GROUP_ACCEPTS
    for case in S.HAND:
        assert (case["fused"] != S.NO_GROUP) == (case["name"] in GROUP_ACCEPTS), case["name"]
        assert S.chain(case["spec"]) == (case["name"] in GROUP_ACCEPTS), case["name"]
    for seed in S.SEEDS:                      # the restatement the categories use is the engine's decision
        spec, _ = S.generate(seed)
        assert S.chain(spec) == (engine.FusedModel._group(spec) is not None), seed


# ---- the wide vocabulary: concat, crop / upsample / pair zeropad, dwconv, tconv --------------------------------------------
import json                               # noqa: E402
import os                                 # noqa: E402

import concat_cases as CC                 # noqa: E402
import depthwise_cases as DW              # noqa: E402
import spatial_cases as SP                # noqa: E402
import spec_digest as G                   # noqa: E402
import tconv_cases as TC                  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def test_old_lists_are_the_parent_commits_lists():
    """HAND and generate(seed) yield the specs and images they yielded before this file learnt the wide vocabulary:
    digests of kernels, biases, BN constants, op dicts and images, recorded by golden/make_fixtures_spec_wide.py."""
    with open(os.path.join(GOLDEN, "spec_graph_parent.json")) as f:
        want = json.load(f)
    assert {c["name"]: G.spec_digest(c["spec"], c["x"]) for c in S.HAND} == want["hand"]
    assert {str(seed): G.spec_digest(*S.generate(seed)) for seed in S.SEEDS} == want["generated"]
    assert len(want["hand"]) == 85 and len(want["generated"]) == 48


def _old_reference_cases():
    out = [("concat/" + n, net) for n, (net, _) in CC.SPECS.items()]
    out += [("spatial/" + n, net) for n, (net, _) in SP.SPECS.items()]
    out += [("chain/" + n, net) for n, (net, _) in SP.CHAINS.items()]
    return out + [("spatial/binary_pad", SP.binary_pad()), ("spatial/binary_upsample", SP.binary_upsample())]


def test_shared_reference_and_guard_equal_the_old_concat_and_spatial_ones():
    """concat_cases.reference / guard and spatial_cases.reference / guard as they were before they became calls of the
    shared functions, recorded on every spec they ran: every tensor of every network bit for bit, and the guard's answer."""
    with open(os.path.join(GOLDEN, "spec_wide_old_reference.json")) as f:
        meta = json.load(f)
    last = np.load(os.path.join(GOLDEN, "spec_wide_old_reference.npz"))
    cases = _old_reference_cases()
    assert sorted(n for n, _ in cases) == sorted(meta) == sorted(last.files) and len(cases) == 20
    for name, net in cases:
        x = net.images()
        assert G.spec_digest(net.spec, x) == meta[name]["spec"], name
        for ref, guard in ((S.reference, S.guard), (CC.reference, CC.guard), (SP.reference, SP.guard)):
            env = ref(net.spec, x, return_all=True)
            assert {k: G.array_digest(v) for k, v in env.items()} == meta[name]["tensors"], name
            assert same_bits(env[S.names_of(net.spec)[-1]], last[name]), name
            assert guard(net.spec, x) == meta[name]["guard"], name
            assert meta[name]["guard"] is None


def test_shared_reference_equals_the_separable_and_unet_references():
    import test_gpu_depthwise as TDW
    import test_gpu_tconv as TTC
    for kind, M in (("quantized", 1), ("quantized", 2), ("binary", 1), ("ternary", 1)):
        spec = TDW.separable_spec(kind, M=M)
        for seed in (0, 1):
            x = TDW._inputs(seed)
            assert same_bits(S.reference(spec, x), TDW.separable_reference(spec, x)), (kind, M)
            assert S.guard(spec, x) is None
    for skip in (True, False):
        spec = TTC.unet_spec(skip=skip)
        for seed in (0, 1):
            x = TTC._images(seed)
            assert same_bits(S.reference(spec, x), TTC.unet_reference(spec, x)), skip
            assert S.guard(spec, x) is None


_KIND = {DW.W_FLOAT: "float", DW.W_BINARY: "binary", DW.W_QUANT: "quantized", DW.W_TERNARY: "ternary"}
_FN = {DW.FN_BINARY_TANH: "binary_tanh", DW.FN_QUANTIZED_TANH: "quantized_tanh", DW.FN_QUANTIZED_RELU: "quantized_relu",
       DW.FN_QUANTIZED_LEAKYRELU: "quantized_leakyrelu", DW.FN_LEAKY_RELU: "leaky_relu"}


def _one_op_spec(c, kernel, bias, bn, which):
    """The case of depthwise_cases / tconv_cases / gconv_cases as a spec: dwconv | tconv | gconv [-> bn] [-> act], the BN
    with eps 0, mean 0 and variance 1, so that bn_constants gives the case's (inv, shift) exactly."""
    op = {"op": which, "kind": _KIND[c["wkind"]], "kernel": kernel, "bias": bias, "strides": (c["stride"], c["stride"]),
          "padding": "same" if c["same"] else "valid", "H": 1.0}
    if c["wkind"] == DW.W_QUANT:
        op["nb"] = c["wbits"]
    if which == "dwconv":
        op.update(dilation=c["dil"], depth_multiplier=c["M"])
    if which == "gconv":
        op.update(dilation=c["dil"], groups=c["groups"])
    spec = [op]
    if bn is not None:
        n = len(bn[0])
        spec.append({"op": "bn", "eps": 0.0, "gamma": bn[0], "beta": bn[1], "mean": np.zeros(n, F32), "var": np.ones(n, F32)})
    if c["fn"] != DW.FN_NONE:
        act = {"op": "act", "fn": _FN[c["fn"]]}
        if c["fn"] in DW.QACTS:
            act["nb"] = c["act_bits"]
        spec.append(act)
    return spec


def _one_op_cases(mod, which, lists=("epilogue_cases", "weight_cases"), refused_cases=None):
    """Every case of the lists (the epilogue and weight cases) whose operands pass guard: (compared, refused by guard)."""
    done, refused = 0, 0
    for c in [c for name in lists for c in getattr(mod, name)()]:
        x, kernel, bias, bn = mod.make_inputs(c)
        xv = x if c["store"] == DW.F32 else DW.values_of(x, c["store"], c["x_bits"])
        spec = _one_op_spec(c, kernel, bias, bn, which)
        if S.guard(spec, xv) is not None:
            refused += 1
            if refused_cases is not None:
                refused_cases.append(c)
            continue
        want = mod.reference(c, x, kernel, bias, bn)
        got = S.reference(spec, xv)
        what = mod.case_id(c)
        if c["out_store"] == DW.F32:
            assert same_bits(got, want), what
        else:                                # packed: the values of the decoded codes
            bits = c["act_bits"] if c["fn"] in DW.QACTS else 1
            vals = DW.values_of(want, c["out_store"], bits)
            np.testing.assert_array_equal(got, vals, err_msg=what)
        done += 1
    return done, refused


def test_one_op_dwconv_specs_equal_depthwise_cases_reference():
    done, refused = _one_op_cases(DW, "dwconv")
    assert done >= 250 and refused <= 70, (done, refused)          # refused: the float32-store cases (inputs off the grid)


def test_one_op_tconv_specs_equal_tconv_cases_reference():
    done, refused = _one_op_cases(TC, "tconv")
    assert done >= 200 and refused <= 70, (done, refused)


WIDE = [(c["name"], c["spec"], c["x"], c["image"]) for c in S.HAND_WIDE]


def test_wide_hand_specs_are_legal_and_exact_by_construction():
    assert len({n for n, _, _, _ in WIDE}) == len(WIDE)
    for name, spec, x, image in WIDE:
        y = S.reference(spec, x)
        assert y.shape[0] == S.N == x.shape[0] and y.size > 0 and np.all(np.isfinite(y)), name
        assert S.guard(spec, x) is None, (name, S.guard(spec, x))          # the guard may reject no hand-written spec
        assert sum(op["op"] in ("conv", "dense", "dwconv", "tconv") for op in spec) <= S.MAX_CONTRACTIONS_WIDE, name
        assert x.shape[1:] == image and image[:2] in ((8, 8), (9, 7), (4, 4)), name
    assert set(S.CAPTURED) <= {n for n, _, _, _ in WIDE}
    for case in S.HAND_WIDE:                  # the logs written out by hand are what the restated planner predicts
        if case["log"] is not None:
            assert S.plan(case["spec"], case["image"])[1] == case["log"], case["name"]


def test_wide_generated_specs_are_legal_deterministic_and_mostly_exact():
    rejected, with_max, shapes = [], 0, set()
    for seed in S.SEEDS_WIDE:
        spec, x, image = S.generate_wide(seed)
        again, x2, _ = S.generate_wide(seed)
        assert _same_spec(spec, again) and np.array_equal(x, x2), seed
        y = S.reference(spec, x)
        assert y.shape[0] == S.N == x.shape[0] and y.size > 0 and np.all(np.isfinite(y)), seed
        assert x.shape[1:] in ((8, 8, 3), (9, 7, 3)) and np.array_equal(x * 8, np.rint(x * 8)), seed
        shapes.add(x.shape[1:])
        assert sum(op["op"] in ("conv", "dense", "dwconv", "tconv") for op in spec) <= S.MAX_CONTRACTIONS_WIDE, seed
        env = S.reference(spec, x, return_all=True)
        for op, name in zip(spec, S.names_of(spec)):
            if op["op"] in ("conv", "tconv"):
                assert env[name].shape[-1] in S.CHANNELS_WIDE, (seed, env[name].shape)
            if op["op"] == "avgpool":         # averages over power-of-two areas only
                assert not S.new_pool(op) and op["size"] & (op["size"] - 1) == 0, seed
        with_max += any(op["op"] == "act" and op["fn"] in S.M.FNS for op in spec)
        cats = S.categories_wide(spec, image)
        if seed % 8 == 0:
            assert "tconv matrix-pipe form" in cats, seed
            assert any(op["op"] == "tconv" and op["kernel"].shape[3] == 64 and op["kernel"].shape[2] % 16 == 0 for op in spec)
        if seed % 8 == 1:
            assert "depthwise 16-bit-lane form" in cats, seed
        why = S.guard(spec, x)
        if why is not None:
            rejected.append((seed, why))
    assert len(S.SEEDS_WIDE) == 64 and shapes == {(8, 8, 3), (9, 7, 3)}
    assert len(rejected) <= 8, rejected
    assert 6 <= with_max <= 20, with_max      # about one network in five


def test_all_four_lists_cover_required():
    count = {}
    for _, spec, _, image in WIDE:
        for c in S.categories_wide(spec, image):
            count[c] = count.get(c, 0) + 1
    for seed in S.SEEDS_WIDE:
        spec, x, image = S.generate_wide(seed)
        if S.guard(spec, x) is None:
            for c in S.categories_wide(spec, image):
                count[c] = count.get(c, 0) + 1
    assert S.REQUIRED == S.REQUIRED_OLD | S.REQUIRED_WIDE and len(S.REQUIRED_WIDE) == 42
    assert not {c for c in S.REQUIRED_WIDE if count.get(c, 0) < 1}
    # the decisions the hand-written list visits beyond the required ones
    for k in ("dwconv", "tconv"):
        for reader in ("maxpool (new form)", "avgpool (new form)", "globalmaxpool", "crop", "flatten", "add", "conv", "dwconv",
                       "concat"):
            assert count.get("packed %s output read by %s" % (k, reader), 0) >= 1, (k, reader)
        assert count.get("packed %s output is the last tensor" % k, 0) >= 1 and count.get("clip behind %s read twice" % k, 0) >= 1
    assert count.get("concat: codes meet a clip, joined in float32", 0) >= 1


def test_fused_engines_group_takes_no_wide_spec():
    for name, spec, _, _ in WIDE:
        assert engine.FusedModel._group(spec) is None and not S.chain(spec), name


def test_recorded_coverage_table_is_current():
    """golden/spec_wide_coverage.json: per category of REQUIRED_WIDE the first two hand-written cases or seeds that cover
    it, hand-written cases first (the table the pull request's summary points to)."""
    cover = {}
    for name, spec, _, image in WIDE:
        for c in S.categories_wide(spec, image):
            cover.setdefault(c, []).append(name)
    for seed in S.SEEDS_WIDE:
        spec, x, image = S.generate_wide(seed)
        if S.guard(spec, x) is None:
            for c in S.categories_wide(spec, image):
                cover.setdefault(c, []).append("seed %d" % seed)
    with open(os.path.join(GOLDEN, "spec_wide_coverage.json")) as f:
        assert json.load(f) == {c: cover[c][:2] for c in sorted(S.REQUIRED_WIDE)}


# ---- the grouped convolution: gconv in the shared reference, guard and plan(); HAND_GROUPED, generate_grouped ---------------
import gconv_cases as GC                  # noqa: E402

CONTRACTIONS = ("conv", "dense", "dwconv", "tconv", "gconv")
GROUPED = [(c["name"], c["spec"], c["x"], c["image"]) for c in S.HAND_GROUPED]


def test_all_four_old_lists_are_the_parent_commits_lists():
    """HAND, generate, HAND_WIDE and generate_wide yield what they yielded before this file learnt the gconv op: the
    digests golden/make_fixtures_spec_grouped.py recorded from the parent commit."""
    with open(os.path.join(GOLDEN, "spec_grouped_parent.json")) as f:
        want = json.load(f)
    assert {c["name"]: G.spec_digest(c["spec"], c["x"]) for c in S.HAND} == want["hand"]
    assert {str(seed): G.spec_digest(*S.generate(seed)) for seed in S.SEEDS} == want["generated"]
    assert {c["name"]: G.spec_digest(c["spec"], c["x"]) for c in S.HAND_WIDE} == want["hand_wide"]
    assert {str(seed): G.spec_digest(*S.generate_wide(seed)[:2]) for seed in S.SEEDS_WIDE} == want["generated_wide"]
    assert [len(want[k]) for k in ("hand", "generated", "hand_wide", "generated_wide")] == [85, 48, 58, 64]


def test_one_op_gconv_specs_equal_gconv_cases_reference():
    """Every plain, weight, epilogue and matrix-pipe case of gconv_cases as a one-op spec.  The guard refuses one case, of
    the float32 store: the 16-bit weights of weight_cases on float32 inputs (units of 2^-21, where a 3 x 3 x 3 window of
    magnitudes up to 1 may pass 2^24 units).  No packed case is refused."""
    refused = []
    done, n = _one_op_cases(GC, "gconv", ("plain_cases", "weight_cases", "epilogue_cases", "mfma_cases"), refused)
    assert done >= 200 and n == len(refused) == 1, (done, n)          # (200: what the tconv test demands)
    assert [(c["store"], c["wkind"], c["wbits"]) for c in refused] == [(GC.F32, GC.W_QUANT, 16)]
    assert done == 491


def test_grouped_hand_specs_are_legal_and_exact_by_construction():
    assert len({n for n, _, _, _ in GROUPED}) == len(GROUPED)
    for name, spec, x, image in GROUPED:
        y = S.reference(spec, x)
        assert y.shape[0] == S.N == x.shape[0] and y.size > 0 and np.all(np.isfinite(y)), name
        assert S.guard(spec, x) is None, (name, S.guard(spec, x))          # the guard may reject no hand-written spec
        assert any(op["op"] == "gconv" for op in spec), name
        assert sum(op["op"] in CONTRACTIONS for op in spec) <= S.MAX_CONTRACTIONS_WIDE, name
        assert x.shape[1:] == image and image[:2] in ((8, 8), (9, 7), (4, 4)), name
    assert set(S.CAPTURED_GROUPED) <= {n for n, _, _, _ in GROUPED}
    logs = 0
    for case in S.HAND_GROUPED:               # the logs written out by hand are what the restated planner predicts
        if case["log"] is not None:
            assert S.plan(case["spec"], case["image"])[1] == case["log"], case["name"]
            logs += 1
    assert logs >= 50


def test_grouped_generated_specs_are_legal_deterministic_and_mostly_exact():
    rejected, shapes, groups = [], set(), set()
    for seed in S.SEEDS_GROUPED:
        spec, x, image = S.generate_grouped(seed)
        again, x2, _ = S.generate_grouped(seed)
        assert _same_spec(spec, again) and np.array_equal(x, x2), seed
        y = S.reference(spec, x)
        assert y.shape[0] == S.N == x.shape[0] and y.size > 0 and np.all(np.isfinite(y)), seed
        assert x.shape[1:] in ((8, 8, 3), (9, 7, 3)) and np.array_equal(x * 8, np.rint(x * 8)), seed
        shapes.add(x.shape[1:])
        assert sum(op["op"] in CONTRACTIONS for op in spec) <= S.MAX_CONTRACTIONS_WIDE, seed
        assert any(op["op"] == "gconv" for op in spec), seed
        for op in spec:
            if op["op"] == "gconv":
                kh, kw, cg, cout = op["kernel"].shape
                assert cout % op["groups"] == 0 and cout in S.CHANNELS_WIDE and cg * op["groups"] in S.CHANNELS_WIDE, seed
                groups.add(op["groups"])
        log = S.plan(spec, image)[1]
        if seed % 4 == 0:                     # every forced form appears in its seed's log
            assert "gconv_i4_mfma" in log or "gconv_i8_mfma" in log, (seed, log)
            assert all(op["kind"] == "quantized" and op["nb"] in (4, 8) for op in spec if op["op"] in CONTRACTIONS), seed
        if seed % 4 == 1:
            i = min(log.index(k) for k in ("gconv_i4_plain", "gconv_i8_plain") if k in log)
            assert i > 0 and log[i - 1] == "pack", (seed, log)
        why = S.guard(spec, x)
        if why is not None:
            rejected.append((seed, why))
    assert len(S.SEEDS_GROUPED) == 32 and shapes == {(8, 8, 3), (9, 7, 3)}
    assert len(rejected) <= 4, rejected
    assert {1, 2, 3, 4, 8} <= groups, groups


def _grouped_cover():
    cover = {}
    for name, spec, _, image in GROUPED:
        for c in S.categories_grouped(spec, image):
            cover.setdefault(c, []).append(name)
    for seed in S.SEEDS_GROUPED:
        spec, x, image = S.generate_grouped(seed)
        if S.guard(spec, x) is None:
            for c in S.categories_grouped(spec, image):
                cover.setdefault(c, []).append("seed %d" % seed)
    return cover


def test_grouped_lists_cover_required_and_the_recorded_table_is_current():
    """golden/spec_grouped_coverage.json: per category of REQUIRED_GROUPED the first two hand-written cases or unrejected
    seeds that cover it, hand-written cases first."""
    cover = _grouped_cover()
    need = ({"op gconv", "max activation in front of gconv", "LayerModel chain", "gconv clip in the epilogue",
             "BN behind gconv read twice", "gconv matrix-pipe form", "gconv plain form: other out store"} |
            {"launch %s" % k for k in S.GCONV_LAUNCHES} | {"packed gconv output read by %s" % k for k in S.GCONV_READERS})
    assert need <= S.REQUIRED_GROUPED and len(S.GCONV_LAUNCHES) == 7 and len(S.REQUIRED_GROUPED) == 33
    assert not {c for c in S.REQUIRED_GROUPED if not cover.get(c)}
    with open(os.path.join(GOLDEN, "spec_grouped_coverage.json")) as f:
        assert json.load(f) == {c: cover[c][:2] for c in sorted(S.REQUIRED_GROUPED)}
    # the generator reaches both forms and the join on its own
    for c in ("launch gconv_i4_mfma", "launch gconv_i8_mfma", "launch gconv_i4_plain", "launch gconv_i8_plain", "pack_clips join"):
        assert any(n.startswith("seed") for n in cover[c]), c
    assert S.REQUIRED == S.REQUIRED_OLD | S.REQUIRED_WIDE and len(S.REQUIRED_WIDE) == 42


def test_groups_one_and_groups_cin_equal_the_conv_and_dwconv_twins():
    """The gconv branch of the reference against the conv branch (groups = 1) and the dwconv branch (groups = Cin, M = Fg,
    kernel reshaped): every tensor of the network bit for bit, and the guard agrees."""
    by_name = {c["name"]: c for c in S.HAND_GROUPED}
    for names, twin, kind in ((S.GROUPS_ONE, S.conv_twin, "conv"), (S.GROUPS_CIN, S.dwconv_twin, "dwconv")):
        assert len(names) == 3
        for name in names:
            c = by_name[name]
            other = twin(c["spec"])
            assert not any(op["op"] == "gconv" for op in other) and sum(op["op"] == "gconv" for op in c["spec"]) == 1
            assert [op["op"] for op in other] == [kind if op["op"] == "gconv" else op["op"] for op in c["spec"]]
            got, want = S.reference(c["spec"], c["x"], return_all=True), S.reference(other, c["x"], return_all=True)
            assert set(got) == set(want)
            for k in want:
                assert same_bits(got[k], want[k]), (name, k)
            assert S.guard(other, c["x"]) is None
    # ... and the grouped sum itself against the block-diagonal ordinary convolution, groups in between
    rng = np.random.default_rng(5)
    for g, cg, fg, k, s, same, dil in ((2, 3, 5, (3, 3), 1, True, (1, 1)), (3, 5, 1, (2, 3), 2, False, (1, 1)),
                                       (4, 4, 4, (3, 3), 1, True, (2, 2))):
        x = rng.integers(-8, 8, (2, 9, 7, g * cg))
        w = rng.integers(-8, 8, k + (cg, g * fg))
        full = O.int_conv2d(x, D.stuff(GC.expand_block_diagonal(w, g), *dil), (s, s), "same" if same else "valid")
        np.testing.assert_array_equal(GC.gconv_sum(x, w, g, s, same, dil), full)


def test_shared_reference_equals_the_resnext_reference():
    import test_gpu_gconv as TG
    for skip in (True, False):
        spec = TG.resnext_spec(skip=skip)
        for seed in (0, 1):
            x = TG._features(seed)
            assert same_bits(S.reference(spec, x), TG.resnext_reference(spec, x)), skip
            assert S.guard(spec, x) is None
            assert S.plan(spec, x.shape[1:])[1] == ["pack", "gconv_i4_mfma"]


def test_fused_engines_group_takes_no_grouped_spec():
    for name, spec, _, _ in GROUPED:
        assert engine.FusedModel._group(spec) is None and not S.chain(spec), name
    for seed in S.SEEDS_GROUPED:
        spec = S.generate_grouped(seed)[0]
        assert engine.FusedModel._group(spec) is None and not S.chain(spec), seed

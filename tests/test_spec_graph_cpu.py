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
    assert not {c: count.get(c, 0) for c in S.REQUIRED if count.get(c, 0) < 2}
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

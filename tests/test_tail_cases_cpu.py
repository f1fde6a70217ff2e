"""The case tables of tail_cases.py, checked without a GPU: the tables build, the references written out there agree bit
for bit with the oracle (two independently written references agreeing is what makes the GPU comparison in
test_gpu_tail.py mean something), no case is degenerate, and the dense table covers every branch of route_dense /
launch_dense (csrc/qnn_conv.hip) for every input storage."""
import time

import numpy as np

import tail_cases as T
from oracle import qnn_oracle as O

F32 = np.float32


def _oracle_dense(c, d):
    """The oracle's own evaluation of a case: run_spec on [dense, bn, act] for a plain chain, the same oracle functions
    composed by hand for the residual rows."""
    op = {"op": "dense", "kind": c["wkind"], "kernel": d["kernel"], "bias": d["bias"]}
    if c["wkind"] == "quantized":
        op["nb"] = c["wbits"]
    act = {"binary_tanh": {"op": "act", "fn": "binary_tanh"},
           "quantized_tanh": {"op": "act", "fn": "quantized_tanh", "nb": c["act_bits"]}}.get(c["fn"])
    if d["res"] is None:
        return O.run_spec([s for s in (op, d["bn"], act) if s is not None], d["x"])
    v = O.run_spec([op], d["x"])
    if d["bn"] is not None:
        b = d["bn"]
        v = O.batchnorm_inference(v, b["gamma"], b["beta"], b["mean"], b["var"], b["eps"])
    v = ((d["res"] + v).astype(F32) * F32(d["post_scale"])).astype(F32)
    return O.run_spec([act], v) if act is not None else v


def test_dense_references_agree_with_the_oracle_and_no_case_is_degenerate():
    t0 = time.time()
    cases = T.dense_cases()
    assert len(cases) >= 200 + T.RANDOM_TAIL and len({c["id"] for c in cases}) == len(cases)
    compared = 0
    for c in cases:
        d = T.dense_inputs(c)
        want = T.dense_reference(c, d)
        assert want.shape == (c["N"], c["units"]) and want.dtype == F32 and np.isfinite(want).all(), c["id"]
        if d["codes"] is not None:                   # packed inputs and grid-valued float32 inputs
            np.testing.assert_array_equal(want, _oracle_dense(c, d), err_msg=c["id"])
            compared += 1
        if c["fn"] != "none" and not c["fill"] and want.size >= 16:
            assert np.unique(want).size >= 2, "degenerate case (one output value): " + c["id"]
        if c["out_store"] != T.STORE_F32 and c["N"]:
            w = T.pack_words(T.out_codes(c, want), c["out_store"])
            assert not (w == T.PACKED_FILL).any(), "the packed fill occurs in the expected output of " + c["id"]
    assert compared >= 600
    assert time.time() - t0 < 60.0, "the dense table takes %.0f s to evaluate" % (time.time() - t0)


def test_every_activation_case_has_enough_outputs_to_be_checked_for_degeneracy():
    """The two-distinct-values assertion above needs at least 16 outputs; only rows without an activation are smaller."""
    for c in T.dense_cases():
        if c["fn"] != "none":
            assert c["N"] * c["units"] >= 16, c["id"]


# The predicates of the dispatch, stated here so that a change of route_dense / launch_dense that adds a branch is a
# visible edit of this list (T.dense_branch evaluates them):
#   e.res != NULL                      -> no dense kernel (route_dense lacks CAP_RES)
#   out_store != QNN_STORE_F32         -> route_dense declines
#   x_store == QNN_STORE_F32           -> k_dense_f32in, (cin & 3) == 0 ? float4 loads : scalar loads
#   kwords % 4 != 0                    -> route_dense declines
#   units <= 16 && kwords % 16 == 0    -> k_dense_packed_split<XS, 16, 4>      (4 images per block)
#   units <= 16                        -> k_dense_packed<XS, 16>               (16 images per block)
#   units <= 64                        -> k_dense_packed<XS, 64>               (4 images per block)
#   units <= 256                       -> k_dense_packed<XS, 256>              (1 image per block)
#   otherwise                          -> launch_dense declines
PACKED_BRANCHES = ("residual", "packed_out", "kwords_not_4", "split", "up16", "up64", "up256", "units_over_256")
F32_BRANCHES = ("residual", "packed_out", "f32_vec4", "f32_scalar")


def _kw_class(kwords):
    return "16" if kwords % 16 == 0 else "4" if kwords % 4 == 0 else "odd"


def test_dense_table_covers_every_branch_of_the_dispatch_per_input_storage():
    cases = T.dense_cases()
    table = [c for c in cases if c["why"] != "random tail"]          # the explicit rows alone must cover everything
    for s in T.PACKED:
        rows = [c for c in table if c["x_store"] == s]
        name = T.STORE_NAME[s]
        assert {T.dense_branch(c) for c in rows} == set(PACKED_BRANCHES), name
        # every boundary value of `units` against every class of kwords, as plain float32-output rows
        plain = [c for c in rows if not c["res"] and c["out_store"] == T.STORE_F32]
        seen = {(c["units"], _kw_class(T.words(s, c["K"]))) for c in plain}
        for units in T.BOUNDARY_UNITS:
            for kc in ("16", "4", "odd"):
                assert (units, kc) in seen, (name, units, kc)
        # K that does not fill the last packed word
        for K in T.PARTIAL_K[s]:
            assert K % T.per_word(s) != 0 and any(c["K"] == K for c in plain), (name, K)
        # ... at least once inside each dense kernel form
        for form in ("split", "up16", "up64", "up256"):
            assert any(T.dense_branch(c) == form and c["K"] % T.per_word(s) != 0 for c in plain), (name, form)
        # N against the images per block of each form
        for form, ipb in (("split", 4), ("up16", 16), ("up64", 4), ("up256", 1)):
            ns = {c["N"] for c in plain if T.dense_branch(c) == form}
            assert {0, 1, ipb - 1, ipb, ipb + 1} <= ns, (name, form, sorted(ns))
        # epilogues
        assert {c["bias"] for c in rows} == {True, False} and {c["bn"] for c in rows} == {None, "pos", "neg"}, name
        assert {(c["fn"], c["act_bits"]) for c in rows} >= {("none", 0), ("binary_tanh", 0), ("quantized_tanh", 2),
                                                           ("quantized_tanh", 4), ("quantized_tanh", 8)}, name
        assert {c["out_store"] for c in rows} == {T.STORE_F32, T.STORE_BIN, T.STORE_I4, T.STORE_I8}, name
        assert {c["fill"] for c in rows} >= {None, "max", "min", "alternating"}, name
    # the ipb the table assumes is the one the kernels' template parameters give
    assert [T.dense_ipb(u) for u in (16, 64, 256)] == [(("split", 4), ("up16", 16)), (("up64", 4),) * 2, (("up256", 1),) * 2]
    # the heads of the networks
    assert any(c["N"] == 4096 and c["K"] == 1024 and c["units"] == 10 and T.dense_branch(c) == "split" for c in table)
    assert any(c["N"] == 64 and c["K"] == 512 and c["units"] == 1000 for c in table)
    # widths
    i4 = {(c["x_bits"], c["wkind"], c["wbits"]) for c in table if c["x_store"] == T.STORE_I4}
    i8 = {(c["x_bits"], c["wkind"], c["wbits"]) for c in table if c["x_store"] == T.STORE_I8}
    for xb in (1, 2, 3, 4):
        for w in (("binary", 1), ("ternary", 1), ("quantized", 2), ("quantized", 3), ("quantized", 4)):
            assert (xb,) + w in i4, (xb, w)
    for xb in (5, 8):
        for w in (("binary", 1), ("ternary", 1), ("quantized", 2), ("quantized", 8)):
            assert (xb,) + w in i8, (xb, w)
    # saturated 8-bit operands whose sum exceeds 2^24
    assert any(c["fill"] == "max" and c["x_store"] == T.STORE_I8 and 127 * 127 * c["K"] > 2 ** 24 for c in table)
    assert any(c["fill"] == "min_max" and c["x_store"] == T.STORE_BIN and c["K"] % 32 for c in table)
    # float32 input
    f = [c for c in table if c["x_store"] == T.STORE_F32]
    assert {T.dense_branch(c) for c in f} == set(F32_BRANCHES)
    for cin in T.F32_CIN:
        for units in T.F32_UNITS:
            for xk in ("grid", "normal", "cancel"):
                assert any(c["K"] == cin and c["units"] == units and c["xkind"] == xk for c in f), (cin, units, xk)
    assert all(c["fn"] == "none" and not c["res"] for c in f if c["xkind"] != "grid")
    # the random tail spans the axes
    tail = [c for c in cases if c["why"] == "random tail"]
    assert len(tail) >= 200 and {c["x_store"] for c in tail} == set(T.PACKED) | {T.STORE_F32}
    assert max(c["K"] for c in tail) > 4096 and max(c["units"] for c in tail) > 256 and max(c["N"] for c in tail) > 64


def test_cancelling_inputs_leave_a_sum_far_below_the_terms():
    for c in T.dense_cases():
        if c["xkind"] == "cancel" and c["K"] >= 63:
            d = T.dense_inputs(c)
            wq, _ = T.quantized_kernel(c, d["kernel"])
            s, bound = T.dense_f32_bound(c, d)
            mag = np.abs(d["x"].astype(np.float64)) @ np.abs(wq.astype(np.float64))
            assert (np.abs(s) < 1e-5 * mag).all() and (np.abs(s) > 0).all(), c["id"]
            assert (bound < 0.05 * np.abs(s)).all(), c["id"]     # losing the small term cannot pass


def test_avgpool_references_agree_with_the_oracle():
    cases = T.avgpool_cases()
    assert len({c["id"] for c in cases}) == len(cases)
    for c in cases:
        codes = T.avgpool_codes(c)
        x = (codes.astype(F32) * F32(T.code_scale(c["store"], c["bits"]))).astype(F32)
        want = T.avgpool_reference(c, codes)
        np.testing.assert_array_equal(want, O.avgpool2d(x, c["size"]), err_msg=c["id"])
        assert want.shape == (c["N"], c["H"] // c["size"], c["W"] // c["size"], c["C"])
    wave = [c for c in cases if T.avgpool_wave(c)]
    assert {c["bits"] for c in wave} >= {2, 3} and {c["C"] for c in wave} >= {64, 192, 512}
    assert {c["size"] for c in wave} >= {3, 4, 7, 8}
    assert any(c["H"] % c["size"] and c["W"] % c["size"] for c in wave)
    assert any(c["size"] == c["H"] == c["W"] == 7 for c in wave) and any(c["size"] == c["H"] == c["W"] == 8 for c in wave)
    near = [c for c in cases if not T.avgpool_wave(c)]
    assert any(c["store"] == T.STORE_I4 and c["C"] % 64 and c["size"] ** 2 >= 8 for c in near)
    assert any(c["store"] == T.STORE_I4 and c["C"] % 64 == 0 and c["size"] ** 2 < 8 for c in near)
    assert any(c["store"] == T.STORE_I8 and c["C"] % 64 == 0 and c["size"] ** 2 >= 8 for c in near)
    assert any(c["N"] * (c["H"] // c["size"]) * (c["W"] // c["size"]) * c["C"] > 65535 * 256 for c in near)
    assert any(c["fill"] == "min" and c["size"] == 8 for c in wave) and any(c["fill"] == "min" for c in near)


def test_softmax_references_agree_with_the_oracle():
    cases = T.softmax_cases()
    assert len(cases) == len(T.SOFTMAX_ROWS) * len(T.SOFTMAX_COLS) * len(T.SOFTMAX_KINDS)
    tiny = 0
    for c in cases:
        if c["rows"] == 5000 and c["cols"] > 300:       # the largest tables only on the GPU (same code path here)
            continue
        x = T.softmax_logits(c)
        assert np.isfinite(x).all()
        want = T.softmax_reference(x)
        np.testing.assert_array_equal(want, O.softmax(x), err_msg=c["id"])
        assert (np.abs(want.astype(np.float64).sum(-1) - 1.0) <= c["cols"] * 2.0 ** -24).all(), c["id"]
        if c["kind"] == "tiny" and c["cols"] >= 255:
            small = want[(want > 0) & (want < 1e-8)]
            assert small.size and small.min() < 1.2e-38 and small.min() >= 1e-41, c["id"]      # denormals included
            tiny += 1
        if c["kind"] == "spread1400" and c["cols"] >= 255:
            assert (want == 0).mean() > 0.5, c["id"]
    assert tiny


def test_pack_layout_helpers():
    """pack_words against the layout rules spelled out element by element (small shapes), and the pad-field masks."""
    rng = np.random.default_rng(1)
    for store, bits in T.PACK_FORMATS:
        for C in (1, 3, 31, 32, 33, 65):
            codes = T.random_codes(rng, (5, C), store, bits)
            got = T.pack_words(codes, store)
            assert got.shape == (5, T.words(store, C)) and got.dtype == np.uint32
            want = np.zeros_like(got)
            pw = T.per_word(store)
            for p in range(5):
                for ch in range(C):
                    k = int(codes[p, ch])
                    w, f = ch // pw, ch % pw
                    if store == T.STORE_BIN:
                        want[p, w] |= np.uint32((1 if k > 0 else 0) << f)
                    elif store == T.STORE_T2:
                        want[p, 2 * w] |= np.uint32((1 if k != 0 else 0) << f)
                        want[p, 2 * w + 1] |= np.uint32((1 if k > 0 else 0) << f)
                    else:
                        fb = 32 // pw
                        want[p, w] |= np.uint32((k & ((1 << fb) - 1)) << (f * fb))
            np.testing.assert_array_equal(got, want)
            assert not (got & T.pad_field_mask(store, C)).any()
    for c in T.pack_cases():
        if c["pixels"] <= 65:
            assert not (T.pack_words(T.pack_codes(c), c["store"]) == T.PACKED_FILL).any(), c["id"]
    assert len(T.pack_cases()) == len(T.PACK_FORMATS) * len(T.PACK_PIXELS) * len(T.PACK_CHANNELS)


def test_activation_tables():
    assert T.ACT_UNROLL >= 1 and 4 * 256 * T.ACT_UNROLL + 3 in T.ACT_LENGTHS
    assert {n % 4 for n in T.ACT_LENGTHS} == {0, 1, 2, 3}
    # the wrapping length is in the table exactly when a tensor of it fits the 2 GiB this suite allocates at most
    assert T.ACT_WRAP_LENGTH == T.ACT_MAX_BLOCKS * 1024 + 5
    assert (T.ACT_WRAP_LENGTH in T.ACT_LENGTHS) == (T.ACT_WRAP_LENGTH * 4 <= 2 ** 31)
    for fn, nb in T.ACT_FNS:
        x = T.act_values(5000, nb, 1)
        assert x.size == 5000 and np.unique(T.act_reference(fn, nb, x)).size >= 2
    for n in (64, 65 + 1, 10 ** 6):
        x, t = T.ternary_threshold_tensor(n, 5)
        assert F32(np.mean(np.abs(x), dtype=np.float64)) == F32(0.5) and F32(0.7) * F32(0.5) == t
        y = O.ternary_tanh(x)
        assert (np.abs(x) == t).sum() == 32
        assert (y[x == t] == 0).all() and (y[x == -t] == -1).all()

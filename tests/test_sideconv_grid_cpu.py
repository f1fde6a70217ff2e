"""The case table of sideconv_grid_cases.py, checked with the oracle alone (no GPU): every case names the kernel form the
route rules give it, carries the special points of its activation in numbers that are conditions and not measurements,
those points tell a wrong rounding, threshold, clip or per-field constant from the right one -- and the numpy references
the three side convolutions' GPU tests compare with (depthwise_cases.py and its importers) equal oracle/qnn_oracle.py bit
for bit, on an edge vector and on every case."""
import numpy as np
import pytest

from oracle import qnn_oracle as O
import depthwise_cases as D
import qact_grid_cases as A
import qrelu_cases as Q
import sideconv_grid_cases as S

CASES = S.cases()
GROUPS = S.groups()
GROUP_IDS = ["%s-%s" % g[1:] for g in GROUPS]
f32 = np.float32


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype == np.float32 or b.dtype == np.float32:
        return Q.same_bits(a, b)
    return a.shape == b.shape and np.array_equal(a, b)


def every_case(g, check):
    """check(c) on every case of group g (one form on one shape: its epilogues x BN signs); the failures together, each
    under its case id."""
    cs = S.group_cases(g)
    assert cs
    failures = []
    for c in cs:
        try:
            check(c)
        except AssertionError as e:
            failures.append("%s: %s" % (c["id"], str(e).split("\n")[0]))
    assert not failures, "%d of %d cases:\n%s" % (len(failures), len(cs), "\n".join(failures))


@pytest.mark.parametrize("g", GROUPS, ids=GROUP_IDS)
def test_cases_carry_their_points_and_they_discriminate(g):
    every_case(g, carries_its_points)


def carries_its_points(c):
    assert S.form_name(c) == c["form"]
    p = S.preactivation(c)
    assert p.dtype == np.float32 and np.all(np.isfinite(p)) and np.abs(p).max() < 2048
    assert np.array_equal(p.astype(np.float64) * 4096, np.rint(p.astype(np.float64) * 4096))      # small dyadic numbers
    want = S.expected(c, p)
    n = S.counts(c, p)
    diff = {k: int(np.count_nonzero(w != want)) for k, w in S.wrong(c, p).items()}
    fn, nb = c["fn"], c["act_bits"]
    assert diff["fields"] >= S.MIN_DIFF, (c["id"], diff)
    if fn == D.FN_BINARY_TANH:
        assert n["zeros"] >= S.MIN_ZEROS, (c["id"], n)
        assert np.count_nonzero(p > 0) >= S.MIN_ZEROS and np.count_nonzero(p < 0) >= S.MIN_ZEROS, c["id"]
        assert diff["ge0"] >= S.MIN_DIFF and diff["ge0"] == n["zeros"], (c["id"], diff)
    if fn in D.QACTS:
        fine = S.claims(c, nb)
        assert fine or nb == 8, c["id"]                              # Q(2) and Q(4) are claimed by every case
        assert n["beyond"] >= S.MIN_EDGE, (c["id"], n)               # values beyond the grid on some side: they are clipped
        assert diff["clip_m"] >= S.MIN_DIFF, (c["id"], diff)
        if fn != D.FN_QUANTIZED_RELU:
            assert n["lo"] >= S.MIN_EDGE, (c["id"], n)               # t = -m: always on the grid
        if fine:
            assert n["ties"] >= S.MIN_TIES and n["hi"] >= S.MIN_EDGE, (c["id"], n)
            assert diff["half_away"] >= S.MIN_DIFF and diff["half_up"] >= S.MIN_DIFF and diff["trunc"] >= S.MIN_DIFF, (c["id"], diff)
            if fn == D.FN_QUANTIZED_RELU:
                assert n["lo"] >= S.MIN_EDGE, (c["id"], n)
        else:
            # the exemption is a fact of the grid, not a lowered bar: no tie of an unscaled value (the negative side of
            # quantized_leakyrelu, scaled by 0.1f, has its own claim below)
            assert n["ties"] - n.get("neg", 0) == 0, (c["id"], n)
        if fn == D.FN_QUANTIZED_LEAKYRELU and S.claims(c, nb, negative=True):
            assert n["neg"] >= S.MIN_NEG, (c["id"], n)


def test_wrong_variants_are_wrong_only_where_they_should_be():
    """Truncation and the clip at m on a 1-D sweep: equal to the contract except off the integers and at m - 1/2 and beyond."""
    x = np.concatenate([np.arange(-80, 40) / 16.0, np.arange(-700, 300) / 256.0, [-10.0, -2.5, -7.5]]).astype(f32)
    for fn in D.QACTS:
        for nb in (2, 4, 8):
            c = dict(fn=fn, act_bits=nb)
            m = 2.0 ** (nb - 1)
            want = S.activate(c, x)
            t, off, lo = S._t_off_lo(c, x)
            w = {"trunc": (np.clip(np.trunc(t) - off, lo, m - 1) / m).astype(f32),
                 "clip_m": (np.clip(np.rint(t) - off, lo, m) / m).astype(f32)}
            whole = t == np.rint(t)
            assert np.array_equal(w["trunc"][whole], want[whole]) and np.any(w["trunc"] != want), (fn, nb)
            top = t - off >= m - 0.5
            assert np.array_equal(w["clip_m"][~top], want[~top]) and np.all(w["clip_m"][top] != want[top]), (fn, nb)


def test_table_names_every_form_and_epilogue():
    forms = {c["form"] for c in CASES}
    want = {"depthwise_i4", "depthwise_i8", "depthwise_i4_plain", "depthwise_i8_plain", "depthwise_bin", "depthwise_t2",
            "depthwise_f32"}
    for op in ("gconv", "tconv"):
        want |= {"%s_%s" % (op, s) for s in ("i4_mfma", "i8_mfma", "i4_plain", "i8_plain", "bin", "t2", "f32")}
    assert forms == want
    for form in forms:
        cs = [c for c in CASES if c["form"] == form]
        fast = form.endswith("_mfma") or form in ("depthwise_i4", "depthwise_i8")
        assert {c["sign"] for c in cs} == {None, "pos", "mixed"}
        assert {c["fn"] for c in cs} >= {D.FN_BINARY_TANH} | set(D.QACTS)
        store = cs[0]["store"]
        widths = {2, 4, 8} if not fast or store == D.I8 else {2, 4}
        for fn in D.QACTS:
            assert {c["act_bits"] for c in cs if c["fn"] == fn} == widths, (form, fn)
        if fast:
            assert {c["out_store"] for c in cs} == {store}
            assert all(S.twin(c) is not None and S.twin(c)["form"].endswith("_plain") for c in cs)
        else:
            assert {c["out_store"] for c in cs} == {D.F32, D.BIN, D.I4, D.I8}, form
            assert {c["fn"] for c in cs} >= {D.FN_NONE, D.FN_LEAKY_RELU}
    assert any(c["op"] == "dw" and c["M"] == 2 and c["store"] == s for c in CASES for s in (D.I4,))
    assert any(c["op"] == "dw" and c["M"] == 2 and c["store"] == D.I8 for c in CASES)
    assert any(c["op"] == "tc" and c["window"][0] < c["stride"] for c in CASES)
    # the exemptions, by name: Q(8) without a fine enough grid
    exempt = {(c["form"], c["id"].split("-")[1], c["sign"]) for c in CASES if c["fn"] in D.QACTS and not S.claims(c, c["act_bits"])}
    assert exempt and all(sign is None for _, _, sign in exempt), sorted(exempt, key=str)          # never behind a BN
    assert not any("w8" in tag for _, tag, _ in exempt)


def test_every_group_has_a_host_among_the_gpu_test_ids():
    """test_gpu_sideconv_grid.run_hosted hands every group to a test_epilogues id of its op's GPU file on the same input store
    (S.hosted): the ids are distinct, the groups of all hosts are the whole table, each once, and a depthwise or transposed
    id carries one group at the most (the ten grouped ids: two)."""
    import gconv_cases as GC
    import tconv_cases as TC
    seen = []
    for op, M, most in (("dw", D, 1), ("tc", TC, 1), ("gc", GC, 2)):
        if op == "gc":
            stores = [s_ for s_ in GC.STORES for _ in range(2)]           # test_epilogues of test_gpu_gconv.py: store x (bias, bn)
        else:
            ids = [M.case_id(c) for c in M.epilogue_cases()]
            assert len(set(ids)) == len(ids)
            stores = [c["store"] for c in M.epilogue_cases()]
        per_host = S.hosted(op, stores)
        assert len(per_host) == len(stores) and max(len(h) for h in per_host) == most
        for store, gs in zip(stores, per_host):
            assert all(c["store"] == store for g in gs for c in S.group_cases(g))
        seen += [g for gs in per_host for g in gs]
    assert sorted(seen) == sorted(GROUPS) and len(set(seen)) == len(seen)
    assert sum(len(S.group_cases(g)) for g in GROUPS) == len(CASES) == 2010


# ---- the restated reference, pinned to the oracle -------------------------------------------------------------------------
def edge_vector():
    pts = [0.0, 2.0 ** -24, 2.0 ** -25, 2.0 ** -23, 1.0, 1.5, 3.0, 10.0, 2.5, 7.5, 1e-3, 0.3]
    for nb in (2, 4, 8):
        m = 2.0 ** (nb - 1)
        pts += [(k + 0.5) / m for k in range(0, int(m) + 2)] + [k / m for k in range(0, int(m) + 2)]
        pts += [(10 * k + 5) / m for k in range(8)] + [0.25 / m, 0.75 / m]
    x = np.array(sorted(set(pts)), f32)
    x = np.concatenate([x, -x])
    return np.concatenate([x, np.nextafter(x, f32(np.inf)), np.nextafter(x, f32(-np.inf))]).astype(f32)


def oracle_chain(v, bias, bn, fn, nb):
    p = O.bias_add(v, bias) if bias is not None else np.asarray(v, f32)
    if bn is not None:
        p = O.batchnorm_inference(p, bn["gamma"], bn["beta"], bn["mean"], bn["var"], bn["eps"])
    return S.activate(dict(fn=fn, act_bits=nb), p)


def test_restated_activations_equal_the_oracle_on_the_edge_vector():
    x = edge_vector()
    assert Q.same_bits(D.binary_tanh(x), O.binary_tanh(x))
    assert np.all(O.binary_tanh(np.array([0.0, -0.0, 2.0 ** -24], f32)) == -1) and O.binary_tanh(np.nextafter(f32(2.0 ** -24), f32(1))) == 1
    n = x.size
    ch = np.arange(n)
    bn = dict(gamma=np.where(ch % 3 == 1, -1.0, 1.0).astype(f32) * np.array([0.25, 0.5, 1.0, 2.0], f32)[ch % 4],
              beta=(((ch % 5) - 2) / 16.0).astype(f32), mean=(((ch % 3) - 1) * 0.5).astype(f32),
              var=np.array([0.75, 3.75], f32)[(ch // 4) % 2], eps=0.25)
    bias = (((ch % 7) - 3) / 16.0).astype(f32)
    k = O.bn_constants(bn["gamma"], bn["beta"], bn["mean"], bn["var"], bn["eps"])
    pairs = [(D.FN_NONE, 0), (D.FN_LEAKY_RELU, 0), (D.FN_BINARY_TANH, 0)] + [(fn, nb) for fn in D.QACTS for nb in (2, 4, 8)]
    for fn, nb in pairs:
        for b, n_, kk in ((None, None, None), (bias, bn, k), (bias, None, None), (None, bn, k)):
            want = oracle_chain(x, b, n_, fn, nb)
            assert Q.same_bits(D.chain(x, b, kk, fn, nb, D.F32), want), (fn, nb)
            if fn == D.FN_BINARY_TANH:
                assert np.array_equal(D.chain(x, b, kk, fn, nb, D.BIN), want > 0)
                assert np.array_equal(D.chain(x, b, kk, fn, nb, D.I4), want.astype(np.int64))
            elif fn in D.QACTS:
                assert np.array_equal(D.chain(x, b, kk, fn, nb, D.I8), O.codes_of(want, nb)), (fn, nb)
                m = f32(2 ** (nb - 1))
                assert np.array_equal(D.qact_code(fn, x, m), O.codes_of(oracle_chain(x, None, None, fn, nb), nb).astype(f32))


def _kernel_at_cutoff():
    """A kernel holding its own ternary cutoff 0.7 * mean |W| with both signs (a float32 fixed point)."""
    rs = np.random.RandomState(5)
    w = (rs.randint(-64, 65, (3, 3, 4, 5)) / 64.0).astype(f32)
    for _ in range(64):
        cut = f32(0.7) * f32(np.mean(np.abs(w), dtype=np.float64))
        if w.flat[0] == cut and w.flat[1] == -cut:
            return w, cut
        w.flat[0], w.flat[1] = cut, -cut
    raise AssertionError("no fixed point")


def test_restated_weight_quantisers_equal_the_oracle():
    rs = np.random.RandomState(6)
    ev = edge_vector()
    ks = [np.concatenate([ev, np.zeros(-ev.size % 3, f32)]).reshape(3, 1, -1, 1),
          (rs.randint(-64, 65, (3, 3, 5, 2)) / 64.0).astype(f32), rs.uniform(-1.3, 1.3, (2, 3, 4, 3)).astype(f32)]
    at, cut = _kernel_at_cutoff()
    ks.append(at)
    for k in ks:
        assert Q.same_bits(D.quantize_weights(k, D.W_BINARY)[0], O.binarize(k))
        # (O._ternarize: the Wt of ternary_ops.py, which the oracle's exact mode convolves with; O.ternarize replays
        # W + (Wt - W) in float32 and lands within an ulp of it)
        assert Q.same_bits(D.quantize_weights(k, D.W_TERNARY)[0], O._ternarize(k))
        assert np.array_equal(np.rint(O.ternarize(k)), O._ternarize(k))
        assert Q.same_bits(D.quantize_weights(k, D.W_FLOAT)[0], k)
        for nb in (2, 4, 8, 16):
            q, code, shift = D.quantize_weights(k, D.W_QUANT, nb)
            assert Q.same_bits(q, O.quantize(k, nb)) and shift == nb - 1
            assert np.array_equal(code, O.codes_of(O.quantize(k, nb), nb))
    t = O.ternarize(at)
    assert t.flat[0] == 0 and t.flat[1] == -1                        # W > cutoff fails at the cutoff, W <= -cutoff holds
    assert np.array_equal(D.quantize_weights(at, D.W_TERNARY)[1], np.rint(t))


@pytest.mark.parametrize("g", GROUPS, ids=GROUP_IDS)
def test_restated_reference_equals_the_oracle(g):
    every_case(g, reference_equals_the_oracle)


def reference_equals_the_oracle(c):
    x, kernel, bias, bn = S.inputs(c)
    want = S.stored(c, S.expected(c))
    b = S.base(c)
    q = D.quantize_weights(kernel, c["wkind"], c["wbits"])[0]
    assert Q.same_bits(q, b["wq"])
    assert same_bits(D.chain(b["v"], bias, bn, c["fn"], c["act_bits"], c["out_store"]), want), c["id"]
    got = S.MOD[c["op"]].reference(c, x, kernel, bias, bn)
    assert same_bits(got, want), c["id"]
    # what the GPU test leans on: no expected word is the pattern laid under the output
    if c["out_store"] != D.F32:
        assert not (D.encode(want, c["out_store"]) == 0x5A5A5A5A).any()
    else:
        assert not (want.view(np.uint32) == 0x5A5A5A5A).any()

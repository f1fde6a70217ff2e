"""The case table of qact_grid_cases.py, checked with numpy alone (no GPU): every case carries the special points of
quantized_relu / quantized_leakyrelu it is there for, in numbers that are conditions and not measurements, and those
points tell a wrong rounding -- or a missing one -- from the contract."""
import numpy as np
import pytest

import epilogue_grid_cases as G
import qact_grid_cases as A
import qrelu_cases as Q

CASES = A.cases()


@pytest.mark.parametrize("c", CASES, ids=[c["id"] for c in CASES])
def test_case_carries_its_points_and_they_discriminate(c):
    p = G.preactivation(c)
    assert p.dtype == np.float32 and np.all(np.isfinite(p)) and np.abs(p).max() < 2048
    if c["res"] != G.STORE_F32:           # small dyadic numbers, exact in float32 in any order (see test_epilogue_grid_cpu)
        assert np.array_equal(p.astype(np.float64) * 4096, np.rint(p.astype(np.float64) * 4096))
    zeros = A.zero_count(p)
    line = ["%d zeros" % zeros]
    assert zeros >= A.MIN_ZEROS, (c["id"], zeros)
    for fn, nb in A.kinds(c):
        want = G.expected(c, dict(fn=fn, nb=nb), p)
        ties = A.tie_count(p, nb)
        away, up, one = (int(np.count_nonzero(wrong(c, p, fn, nb) != want))
                         for wrong in (A.wrong_half_away, A.wrong_floor_half, A.wrong_one_rounding))
        lo, hi = A.edge_counts(p, fn, nb)
        edges = "" if A.claims_edges(c) else " (not claimed)"
        assert ties >= A.MIN_TIES, (c["id"], fn, nb, ties)
        assert away >= A.MIN_DIFF and up >= A.MIN_DIFF, (c["id"], fn, nb, away, up)
        if fn == A.RELU:
            line.append("relu(%d): %d ties, half-away differs in %d, floor(x + 0.5) in %d, without the v + 1 rounding in %d, "
                        "edges %d / %d%s" % (nb, ties, away, up, one, lo, hi, edges))
            if A.claims_edges(c):
                assert lo >= A.MIN_EDGE and hi >= A.MIN_EDGE, (c["id"], fn, nb, lo, hi)
            if c["res"] == G.STORE_F32:
                assert one >= A.MIN_DIFF, (c["id"], fn, nb, one)
            else:
                assert one == 0, (c["id"], fn, nb, one)                    # dyadic points never tell these two apart
        else:
            neg = A.neg_tie_count(p, nb)
            line.append("leaky(%d): %d + %d ties, half-away differs in %d, floor(x + 0.5) in %d, one rounding in %d, upper "
                        "edge %d%s%s" % (nb, ties, neg, away, up, one, hi, edges,
                                        "" if A.claims_negative(c, nb) else "; negative ties not claimed"))
            if A.claims_edges(c):
                assert hi >= A.MIN_EDGE, (c["id"], fn, nb, hi)
            if A.claims_negative(c, nb):
                assert neg >= A.MIN_EDGE and one >= A.MIN_DIFF, (c["id"], fn, nb, neg, one)
    print("[qact grid] %s: %s" % (c["id"], "; ".join(line)))


def test_wrong_references_are_wrong_only_at_the_special_points():
    """On a 1-D sweep each wrong model equals the contract except on ties (the two tie rules), on the float32 neighbours
    of ties (quantized_relu without its rounding) and on the negative ties and their neighbours (quantized_leakyrelu
    with one rounding)."""
    dy = np.concatenate([np.arange(-80, 40) / 16.0, np.arange(-700, 300) / 256.0, np.linspace(-3.3, 1.3, 2001), [-0.0]]).astype(np.float32)
    x = np.concatenate([dy, np.nextafter(dy, np.float32(-np.inf)), np.nextafter(dy, np.float32(np.inf))])
    c = dict(pool=1)
    for nb in (2, 4, 8):
        m = 2.0 ** (nb - 1)
        for fn in Q.FNS:
            want = Q.ACT[fn](x, nb)
            t, _, _ = A._t(x, fn, nb)
            tie = A._frac_half(t)
            for wrong in (A.wrong_half_away, A.wrong_floor_half):
                got = wrong(c, x, fn, nb)
                assert np.array_equal(got[~tie], want[~tie]) and np.any(got[tie] != want[tie]), (fn, nb)
            got = A.wrong_one_rounding(c, x, fn, nb)
            # the contract's rounding moved the value onto a tie (or off one): nowhere else can one rounding matter
            exact = x.astype(np.float64) * m if fn == A.RELU else np.where(x >= 0, 1.0, float(Q.ALPHA)) * x.astype(np.float64) * m
            special = tie != A._frac_half(exact if fn == A.LEAKY else exact + m)
            assert np.array_equal(got[~special], want[~special]) and np.any(got[special] != want[special]), (fn, nb)
            assert np.array_equal(got[np.isin(x, dy) & (x >= 0)], want[np.isin(x, dy) & (x >= 0)])


def test_tie_neighbours_and_negative_ties_discriminate_as_documented():
    """v = 3/16 - ulp: code 2 under the contract, 1 without the rounding; the odd ties discriminate from below, the even ones
    from above; half of the dyadic negative ties tell one rounding from two."""
    c = dict(pool=1)
    v = np.nextafter(np.float32(3 / 16), np.float32(0))
    assert Q.quantized_relu(v, 4) * 8 == 2 and A.wrong_one_rounding(c, np.array([v]), A.RELU, 4)[0] * 8 == 1
    for nb, odd, total in ((4, 3, 7), (8, 63, 127)):
        m = 2 ** (nb - 1)
        ties = np.array([(k + 0.5) / m for k in range(m - 1)], np.float32)
        assert ties.size == total
        below, above = np.nextafter(ties, np.float32(0)), np.nextafter(ties, np.float32(1))
        assert np.count_nonzero(A.wrong_one_rounding(c, below, A.RELU, nb) != Q.quantized_relu(below, nb)) == odd
        assert np.count_nonzero(A.wrong_one_rounding(c, above, A.RELU, nb) != Q.quantized_relu(above, nb)) == total - odd
    above = np.nextafter(np.float32(0.25), np.float32(1))
    assert A.wrong_one_rounding(c, np.array([above]), A.RELU, 2)[0] != Q.quantized_relu(above, 2)
    for nb, found in ((2, 1), (4, 3), (8, 8)):
        neg = np.array(A.neg_ties(nb), np.float32)
        assert neg.size == found and A.neg_tie_count(neg, nb) == found
        diff = A.wrong_one_rounding(c, neg, A.LEAKY, nb) != Q.quantized_leakyrelu(neg, nb)
        assert np.array_equal(diff, np.arange(found) % 2 == 0), (nb, diff)          # even k: the tie goes to the even code


def test_table_names_every_kernel_and_form():
    by = {}
    for c in CASES:
        by.setdefault(c["kernel"], []).append(c)
    assert sorted(by) == sorted(["strip_i4_c16", "strip_i4_c32", "strip_i4_c64", "strip_i4_c16_s2", "strip_i4_c32_s2", "generic"])
    for name, cs in by.items():
        for fn in Q.FNS:
            assert any(a["fn"] == fn and a["named"] for c in cs for a in c["acts"]), (name, fn)
    for name in ("strip_i4_c16", "strip_i4_c32", "strip_i4_c64"):
        cs = by[name]
        assert {(c["res"], c["res_bits"]) for c in cs} == {(None, 0), (G.STORE_I4, 4), (G.STORE_I4, 2), (G.STORE_F32, 0)}
        assert {c["base"][8] for c in cs if c["epi"] == "nobn"} == {True, False}          # both BIAS instantiations
        assert {c["post_scale"] for c in cs if c["res"] == G.STORE_I4} == {1.0, 0.5, 0.25}
        assert {c["sign"] for c in cs if c["epi"] == "dyadic"} == {"mixed", "neg"}
    assert all(A.claims_negative(c, nb) for c in CASES for _, nb in A.kinds(c) if nb != 2)
    gen = by["generic"]
    assert {c["x_store"] for c in gen} == {G.STORE_I4, G.STORE_I8, G.STORE_F32}
    assert {a["store"] for c in gen for a in c["acts"]} == {G.STORE_I4, G.STORE_I8, G.STORE_F32}
    assert {a["nb"] for c in gen for a in c["acts"]} == {2, 4, 8}
    assert any(c["d"] == 2 for c in gen) and any(c["res"] == G.STORE_F32 for c in gen)
    pooled = [c for c in CASES if c["pool"] == 2]
    assert pooled and all(c["sign"] in ("neg", "mixed") for c in pooled) and all(c["x_store"] == G.STORE_I8 for c in pooled)


def _carries(cid, c, p, kinds, negative=(4, 8)):
    """The conditions of a case without a shortcut to plant through: zeros, ties, negative ties and the discrimination counts."""
    zeros = A.zero_count(p)
    assert zeros >= A.MIN_ZEROS, (cid, zeros)
    line = ["%d zeros" % zeros]
    for fn, nb in kinds:
        want = G._pool(c, Q.ACT[fn](p, nb))
        ties, neg = A.tie_count(p, nb), A.neg_tie_count(p, nb)
        away, up, one = (int(np.count_nonzero(wrong(c, p, fn, nb) != want))
                         for wrong in (A.wrong_half_away, A.wrong_floor_half, A.wrong_one_rounding))
        line.append("%s(%d): %d + %d ties, half-away differs in %d, floor(x + 0.5) in %d, one rounding in %d"
                    % (fn[10:], nb, ties, neg, away, up, one))
        assert ties >= A.MIN_TIES and away >= A.MIN_DIFF and up >= A.MIN_DIFF, (cid, fn, nb, ties, away, up)
        if fn == A.LEAKY and nb in negative:
            assert neg >= A.MIN_EDGE and one >= A.MIN_DIFF, (cid, fn, nb, neg, one)
        if fn == A.RELU:
            assert one == 0, (cid, fn, nb, one)
    print("[qact grid] %s: %s" % (cid, "; ".join(line)))


PROJ = A.proj_cases()


@pytest.mark.parametrize("pc", PROJ, ids=[pc["id"] for pc in PROJ])
def test_projection_case_carries_what_the_grid_yields(pc):
    p = A.proj_preactivation(pc)
    assert np.array_equal(p.astype(np.float64) * 4096, np.rint(p.astype(np.float64) * 4096)) and np.abs(p).max() < 2048
    _carries(pc["id"], pc, p, A.kinds(pc))


@pytest.mark.parametrize("dc", A.DENSE, ids=[dc["id"] for dc in A.DENSE])
def test_dense_case_carries_its_points(dc):
    p = A.dense_layer(dc)[4]
    assert np.array_equal(p.astype(np.float64) * 4096, np.rint(p.astype(np.float64) * 4096)) and np.abs(p).max() < 2048
    _carries(dc["id"], dict(pool=1), p, [(fn, 4) for fn in Q.FNS])
    for fn in Q.FNS:
        lo, hi = A.edge_counts(p, fn, 4)
        assert hi >= A.MIN_EDGE and (lo is None or lo >= A.MIN_EDGE), (dc["id"], fn, lo, hi)


def test_table_names_the_projection_and_dense_forms():
    assert sorted(pc["main"]["kernel"] for pc in PROJ) == ["strip_i4_c32"] * 2 + ["strip_i4_c64"] * 2
    assert {pc["main"]["sign"] for pc in PROJ} == {None, "mixed"}
    assert {(dc["kernel"], dc["form"]) for dc in A.DENSE} == {("dense_i4", "packed"), ("dense_i4", "split"), ("dense_f32", "f32")}
    for dc in A.DENSE:
        words = dc["K"] // 8                                   # the rule of launch_dense (csrc/qnn_conv.hip)
        assert (dc["form"] == "split") == (dc["x_store"] == G.STORE_I4 and dc["units"] <= 16 and words % 16 == 0), dc["id"]
    assert any(dc["units"] > 16 for dc in A.DENSE if dc["form"] == "packed")
    assert {dc["K"] for dc in A.DENSE if dc["form"] != "split"} == {64, 96}

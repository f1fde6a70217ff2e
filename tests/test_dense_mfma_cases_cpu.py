"""The case table of dense_mfma_cases.py, checked with numpy alone (no GPU): every case's route claim is the route rule's
answer, the table reaches every instantiation, plan and K-share shape of k_dense_mfma, group A carries the points it is there
for in numbers that are conditions and not measurements, and group C passes the float32 range of the accumulator."""
import numpy as np
import pytest

import dense_mfma_cases as M
import epilogue_grid_cases as G
import qact_grid_cases as QG
import tail_cases as T

CASES = M.cases()
GROUP_A = M.group("A")
ONE = dict(pool=1)


def test_every_case_claims_what_the_route_rule_says():
    assert {g: len(M.group(g)) for g in "ABCD"} == {"A": 40, "B": 60, "C": 31, "D": 30}
    for c in CASES:
        assert M.route(c) == c["on_route"], c["id"]
    off = [c for c in CASES if not c["on_route"]]
    assert len(off) == 4 and all(c["K"] == 65600 for c in off)                   # the only rows written to be declined
    just = dict(off[0], K=65536)
    assert M.route(just) and not M.route(dict(just, units=24)) and not M.route(dict(just, K=65504))
    f32 = next(c for c in CASES if c["out_store"] == M.SF32 and c["x_store"] == M.BIN)
    assert not M.route(dict(f32, N=64)) and M.route(dict(f32, N=65)) and not M.route(dict(f32, units=256))
    assert not M.route(dict(f32, out_store=M.I8)) and not M.route(dict(f32, out_store=M.BIN))
    assert not M.route(dict(just, w_store=M.I4 if just["x_store"] == M.I8 else M.I8))


def test_table_covers_every_instantiation_plan_and_share():
    on = [c for c in CASES if c["on_route"]]
    inst = {(c["x_store"], c["out_store"], M.case_plan(c)[0]) for c in on}
    assert inst == {(xs, out, nt) for xs, out in M.PAIRS for nt in (1, 2, 4)} and len(inst) == 24
    assert {M.case_plan(c)[:2] for c in on} == {(nt, ks) for nt in (1, 2, 4) for ks in (1, 2, 4)}
    for c in M.group("A"):
        assert M.case_plan(c)[:2] == (1, 4), c["id"]
    for c in M.group("B"):
        assert M.case_plan(c)[:2] == c["want_plan"], (c["id"], M.case_plan(c))
        if "want_shares" in c:
            assert M.shares(c["K"] // 64, M.case_plan(c)[1]) == c["want_shares"], c["id"]
        # N one past a multiple of 16; NT divides neither 33 nor 65 unit tiles
        assert c["N"] % 16 == 1 and (c["units"] // 16) % max(M.case_plan(c)[0], 2) in (0, 1)
    sh = [M.shares(c["K"] // 64, M.case_plan(c)[1]) for c in on if M.case_plan(c)[0] == 1]
    lengths = {n for s in sh for n in s}
    assert {n % 3 for n in lengths if n} == {0, 1, 2} and {1, 2, 3, 5} <= lengths
    assert any(s[-1] == 0 for s in sh) and any(0 < s[-1] < s[0] for s in sh)              # an empty and a short last share
    assert any(len(s) == 2 for s in sh) and any(len(s) == 1 and s[0] == 2 for s in sh)    # ks = 2 at NT = 1; ks = 1, two steps
    # forms the wide test never sends to this kernel
    fns = {(c["x_store"], fn) for c in on for fn, _ in c["acts"]}
    assert {(M.I4, M.LEAKY), (M.BIN, M.LEAKY), (M.I8, M.LEAKY), (M.I4, M.RELU), (M.I8, M.RELU)} <= fns
    assert any(c["bias"] is False for c in on) and any(c["bn"] is None for c in on)
    d_rows = {(c["x_store"], c["x_bits"], c["wkind"], c["wbits"]) for c in M.group("D")}
    assert len(d_rows) == 15 and all(xb < xs for xs, xb, _, _ in d_rows) and {k for _, _, k, _ in d_rows} == {"binary", "ternary", "quantized"}


@pytest.mark.parametrize("c", GROUP_A, ids=[c["id"] for c in GROUP_A])
def test_group_a_carries_its_points_and_they_discriminate(c):
    d, _, p = M.layer(c)
    assert p.dtype == np.float32 and np.all(np.isfinite(p)) and np.abs(p).max() < 2048
    assert np.array_equal(p.astype(np.float64) * 4096, np.rint(p.astype(np.float64) * 4096))      # small dyadic numbers
    if d["bias"] is not None:
        assert np.array_equal(d["bias"] * 16, np.rint(d["bias"] * 16))
    assert (d["bias"] is None) == (c["variant"] == "nobias") and (d["bn"] is None) == (c["variant"] == "nobn")
    seen = np.zeros(p.shape, bool)
    line = []
    for fn, nb in c["acts"]:
        claim = M.claims(c, fn, nb)
        if fn == "none":
            continue
        want = M.reference(c, fn, nb)
        mask = M.special(p, fn, nb)
        if fn == M.BT:
            zeros, diff = G.zero_count(p), int(np.count_nonzero(G.wrong_binary_ge0(ONE, p) != want))
            line.append("binary: %d zeros, `>= 0` differs in %d" % (zeros, diff))
            assert zeros >= G.MIN_ZEROS and diff >= G.MIN_DIFF, (c["id"], zeros, diff)
        elif fn == M.QT:
            ties = G.tie_count(p, nb)
            away, up = (int(np.count_nonzero(w(ONE, p, nb) != want)) for w in (G.wrong_half_away, G.wrong_floor_half))
            lo, hi = G.edge_counts(p, nb)
            line.append("Q(%d): %d ties, half-away differs in %d, floor(x + 0.5) in %d, clip edges %d / %d" % (nb, ties, away, up, lo, hi))
            if "ties" in claim:
                assert ties >= G.MIN_TIES and away >= G.MIN_DIFF and up >= G.MIN_DIFF, (c["id"], nb, ties, away, up)
            else:
                assert ties == 0, (c["id"], nb, ties)                # not claimed because no input reaches one
            if "edges" in claim:
                assert lo >= G.MIN_EDGE and hi >= G.MIN_EDGE, (c["id"], nb, lo, hi)
                mask = mask | (p == -1) | (p.astype(np.float64) * 2.0 ** (nb - 1) == 2.0 ** (nb - 1) - 1)
        else:
            ties, neg = QG.tie_count(p, nb), QG.neg_tie_count(p, nb)
            away, up, one = (int(np.count_nonzero(w(ONE, p, fn, nb) != want))
                             for w in (QG.wrong_half_away, QG.wrong_floor_half, QG.wrong_one_rounding))
            lo, hi = QG.edge_counts(p, fn, nb)
            line.append("%s(%d): %d + %d ties, half-away differs in %d, floor(x + 0.5) in %d, one rounding in %d, edges %s / %d"
                        % (fn[10:], nb, ties, neg, away, up, one, lo, hi))
            if "ties" in claim:
                assert ties >= G.MIN_TIES and away >= G.MIN_DIFF and up >= G.MIN_DIFF, (c["id"], fn, nb, ties, away, up)
            else:
                assert ties == 0 and neg == 0, (c["id"], fn, nb, ties, neg)
            if "neg" in claim and "ties" in claim:
                assert neg >= G.MIN_EDGE and one >= G.MIN_DIFF, (c["id"], fn, nb, neg, one)
            if "edges" in claim:
                assert hi >= G.MIN_EDGE and (lo is None or lo >= G.MIN_EDGE), (c["id"], fn, nb, lo, hi)
            if fn == M.RELU:
                assert one == 0, (c["id"], fn, nb, one)              # dyadic points never tell these two apart
        if claim:
            seen |= mask
            assert mask[-15:].any(), (c["id"], fn, nb, "no point in the ragged image tile")
    # where a wrong field shift, bias index or tail guard would show: every unit position of a tile, the ragged image tile
    assert c["N"] % 16 == 15 and sorted(set(np.nonzero(seen)[1] % 16)) == list(range(16)), c["id"]
    assert seen[-15:].any() and seen[:16].any(), c["id"]
    print("[dense mfma grid] %s: %s" % (c["id"], "; ".join(line)))


def test_group_a_names_every_form():
    for xs in (M.I4, M.I8, M.BIN):
        cs = [c for c in GROUP_A if c["x_store"] == xs]
        assert {c["variant"] for c in cs} == set(M.A_VARIANTS)
        assert {c["out_store"] for c in cs} == {out for x, out in M.PAIRS if x == xs}
        for c in cs:
            assert c["K"] == 192 and c["units"] == (272 if c["out_store"] == M.SF32 else 48) and tuple(c["acts"]) == M.ACTS_A[c["out_store"]]
    signs = {v: np.sign(M.layer(next(c for c in GROUP_A if c["variant"] == v))[0]["bn"]["gamma"]) for v in ("pos", "neg", "mixed")}
    assert (signs["pos"] > 0).all() and (signs["neg"] < 0).all() and (signs["mixed"] > 0).any() and (signs["mixed"] < 0).any()


def test_group_c_passes_the_float32_range():
    rounds, top = 0, 0
    for c in M.group("C"):
        d, acc, p = M.layer(c)
        assert np.all(np.isfinite(p)) and np.abs(acc).max() < 2 ** 31
        if c["x_store"] == M.I4 and c["on_route"]:
            assert np.abs(acc).max() * 256 <= 2 ** 30            # the kernel's own sums: both operands widened by 16
        inexact = acc != acc.astype(np.float32).astype(np.int64)
        if inexact.any():
            assert np.abs(acc[inexact]).min() > 2 ** 24 and (acc[inexact] % 2 != 0).any()
            rounds += 1
        if c["K"] >= 65536 and not c["dent"]:
            lo, hi = T.code_range(c["x_store"], c["x_bits"])
            assert np.all(acc == c["K"] * lo * (lo if c["fill"] == "min" else hi)), c["id"]
            if c["K"] == 65536 and c["fill"] == "min":           # the int32 limit of the route: 2^30, also for the x 16 widened int4 codes
                assert np.all(acc * (256 if c["x_store"] == M.I4 else 1) == 2 ** 30), c["id"]
            top += c["K"] == 65536
        if c["K"] == 4608 and c["x_store"] == M.I8 and c["fill"] in ("max", "min") and not c["dent"]:
            assert abs(int(acc[0, 0])) == {"max": 74322432, "min": 75497472}[c["fill"]]
        # the int64 contraction of tail_cases.py gives the same float32
        if c["K"] <= 4608:
            assert np.array_equal(M.contraction(c, d, acc), T.dense_contraction(c, d)), c["id"]
        for fn, nb in c["acts"]:
            want = M.reference(c, fn, nb)
            if fn != "none":                                     # outputs do not all clip, nor all agree
                assert len(np.unique(want)) > 1, c["id"]
    assert rounds >= 3 and top == 4
    # the tie of the conversion: image 3 of the dented K = 4608 row lies half-way between two float32
    c = next(c for c in M.group("C") if c["dent"] and c["K"] == 4608 and c["units"] == 16)
    a = int(M.layer(c)[1][3, 0])
    assert a == 74322432 - 508 and a % 8 == 4
    wide = next(c for c in M.group("C") if c["dent"] and c["units"] == 272)
    assert wide["bn"] is None and wide["bias"] is False and np.array_equal(M.layer(wide)[2], M.contraction(wide, M.layer(wide)[0]))


def test_small_layers_agree_with_the_int64_contraction_and_no_reference_holds_the_fill():
    for c in CASES:
        if c["group"] in "AD" or (c["group"] == "B" and c["N"] <= 33):
            d = M.layer(c)[0]
            assert np.array_equal(M.contraction(c, d), T.dense_contraction(c, d)), c["id"]
        if c["out_store"] == M.SF32:
            continue
        for fn, nb in c["acts"]:
            codes = M.codes_of(fn, nb, M.reference(c, fn, nb))
            lo, hi = (-1, 1) if fn == M.BT else (-2 ** (nb - 1), 2 ** (nb - 1) - 1)
            assert codes.min() >= lo and codes.max() <= hi, c["id"]
            words = T.pack_words(codes, c["out_store"])
            assert not np.any(words == T.PACKED_FILL), c["id"]

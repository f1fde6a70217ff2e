"""The case table of epilogue_grid_cases.py, checked with the oracle alone (no GPU): every case carries the special points
it is there for, in numbers that are conditions and not measurements, and those points tell a wrong epilogue from the
right one.  A case "claims" a class through its activations: a quantized output claims ties (and, without BN or
shortcut, both clip edges), a binary output claims exact zeros."""
import numpy as np
import pytest

import epilogue_grid_cases as G
from oracle import qnn_oracle as O

CASES = G.cases()


def _kinds(c):
    """The distinct (fn, nb) of a case's activations."""
    return sorted({(a["fn"], a["nb"]) for a in c["acts"]})


@pytest.mark.parametrize("c", CASES, ids=[c["id"] for c in CASES])
def test_case_carries_its_points_and_they_discriminate(c):
    p = G.preactivation(c)
    assert p.dtype == np.float32 and np.all(np.isfinite(p))
    # everything is a small dyadic number: multiples of 2^-12 below 2^11 have 23 bits, exact in float32 in any order
    assert np.array_equal(p.astype(np.float64) * 4096, np.rint(p.astype(np.float64) * 4096)) and np.abs(p).max() < 2048
    line = []
    for fn, nb in _kinds(c):
        a = dict(fn=fn, nb=nb)
        want = G.expected(c, a, p)
        if fn == G.BT:
            zeros = G.zero_count(p)
            diff = int(np.count_nonzero(G.wrong_binary_ge0(c, p) != want))
            line.append("binary: %d zeros, `>= 0` differs in %d" % (zeros, diff))
            assert zeros >= G.MIN_ZEROS, (c["id"], zeros)
            assert diff >= G.MIN_DIFF, (c["id"], diff)
            continue
        ties = G.tie_count(p, nb)
        away = int(np.count_nonzero(G.wrong_half_away(c, p, nb) != want))
        up = int(np.count_nonzero(G.wrong_floor_half(c, p, nb) != want))
        line.append("Q(%d): %d ties, half-away differs in %d, floor(x + 0.5) in %d" % (nb, ties, away, up))
        assert ties >= G.MIN_TIES, (c["id"], nb, ties)
        assert away >= G.MIN_DIFF and up >= G.MIN_DIFF, (c["id"], nb, away, up)
        if c["epi"] == "nobn":
            lo, hi = G.edge_counts(p, nb)
            line.append("clip edges %d / %d" % (lo, hi))
            assert lo >= G.MIN_EDGE and hi >= G.MIN_EDGE, (c["id"], nb, lo, hi)
    print("[epilogue grid] %s: %s" % (c["id"], "; ".join(line)))


def test_wrong_references_are_wrong_only_at_the_special_points():
    """The three deliberately wrong references agree with the oracle everywhere except on ties / around zero: what the
    discrimination counts above count is the special points and nothing else."""
    x = np.concatenate([np.arange(-40, 40) / 16.0, np.arange(-300, 300) / 256.0, np.linspace(-1.3, 1.3, 1001), [2.0 ** -24, 2.0 ** -25, -0.0]]).astype(np.float32)
    c = dict(pool=1)
    for nb in (2, 4, 8):
        t = x.astype(np.float64) * 2.0 ** (nb - 1)
        tie = t - np.floor(t) == 0.5
        want = O.quantized_tanh(x, nb)
        for wrong in (G.wrong_half_away, G.wrong_floor_half):
            got = wrong(c, x, nb)
            assert np.array_equal(got[~tie], want[~tie]) and np.any(got[tie] != want[tie])
    got, want = G.wrong_binary_ge0(c, x), O.binary_tanh(x)
    near = (x >= 0) & (x <= np.float32(2.0 ** -24))
    assert np.array_equal(got[~near], want[~near]) and np.all(got[near] != want[near])


def test_table_covers_the_kernels_and_classes():
    """Every kernel of the table has a case with ties, one with exact zeros for a binary output, and -- where it pools -- one
    with a negative dyadic scale; the dyadic "mixed" pattern has both signs inside every 16-filter slice."""
    by = {}
    for c in CASES:
        by.setdefault(c["kernel"], []).append(c)
    want = (["strip_i4_c%d" % n for n in (16, 32, 64)] + ["strip_i4_c%d_dil" % n for n in (16, 32, 64)] + ["strip_i4_c16_s2", "strip_i4_c32_s2", "mfma_i4_small_c16",
            "mfma_i4_small_c32", "mfma_i4_areg64x64", "mfma_i4_halo64x64", "mfma_i4_wres256x64", "mfma_i4_256x64",
            "mfma_i4_256x128", "mfma_i4_256x256", "mfma_i8_256x128", "mfma_i8_256x256", "mfma_i8_areg64x64"] +
            ["strip_i8_c%d" % n for n in (16, 32, 64)] + ["xnor_pk_cw2", "generic"])
    assert sorted(by) == sorted(want)
    for name, cs in by.items():
        named = [(c, a) for c in cs for a in c["acts"] if a["named"]]
        assert any(a["fn"] == G.QT for _, a in named) or name == "xnor_pk_cw2", name
        assert any(a["fn"] == G.BT for _, a in named) or name.startswith("strip_i8"), name      # int8 strips: Q(8) and Q(4) only
        if any(c["pool"] == 2 for c in cs):
            assert any(c["pool"] == 2 and c["sign"] in ("neg", "mixed") for c in cs), name
    for cout in (16, 64, 192):
        inv, _ = O.bn_constants(*(G.dyadic_bn(cout, "mixed")[k] for k in ("gamma", "beta", "mean", "var", "eps")))
        s = np.sign(inv).reshape(-1, 16)
        assert np.all(s.min(axis=1) == -1) and np.all(s.max(axis=1) == 1)
    assert any(c["head"] for c in CASES)

"""The float64 reference of the affinity calibrations (tests/_affinity_reference.py) against its own equations,
against scipy's brentq, and in the limit cases DESIGN section 6q names.  No GPU."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _affinity_reference as ref  # noqa: E402

K_VALUES = (1, 2, 3, 15, 33, 64)

def _rows():
    """Sorted float32 distance rows at scales 1e-3, 1 and 1e3, some tied at the minimum, some all zero."""
    rng = np.random.default_rng(0)
    for k in K_VALUES:
        for trial in range(40):
            d = np.sort(np.sqrt(rng.random(k).astype(np.float32) * rng.choice([1e-6, 1, 1e6]))).astype(np.float32)
            if trial % 5 == 0 and k > 2:
                d[:rng.integers(1, k)] = d[0]
            if trial % 7 == 3:
                d[:] = 0
            yield k, d


def _perplexities(k):
    return [perp for perp in (0.5, 1.0, 2.0, 5.0, k / 3.0, k - 0.5, float(k), k + 1.0) if perp > 0]


def test_roots_satisfy_their_equations_and_agree_with_brentq():
    from scipy.optimize import brentq
    worst_eq = worst_p = 0.0
    searched = 0
    for k, d in _rows():
        d64 = d.astype(np.float64)
        s = d64 * d64 - (d64 * d64).min()
        for perp in _perplexities(k):
            p, beta, off = ref.perplexity_row(d64, perp)
            assert abs(p.sum() - 1) <= 1e-12 and off == d64.min()
            if 0 < beta < np.inf:
                searched += 1
                worst_eq = max(worst_eq, abs(ref.entropy(beta, s)[0] - np.log(perp)))
                b2 = brentq(lambda b: ref.entropy(b, s)[0] - np.log(perp), 0.5 * beta, 2 * beta, xtol=1e-300,
                            rtol=1e-15)
                worst_p = max(worst_p, np.abs(ref.entropy(b2, s)[1] - p).max())
        p, sigma, rho, root = ref.umap_row(d64)
        if root is not None:
            searched += 1
            g = ref.umap_gaps(d64)[0]
            total = lambda sg: np.where(g == 0, 1.0, np.exp(-g / sg)).sum()      # noqa: E731
            worst_eq = max(worst_eq, abs(total(root) - np.log2(k)))
            s2 = brentq(lambda sg: total(sg) - np.log2(k), 0.5 * root, 2 * root, xtol=1e-300, rtol=1e-15)
            if sigma == root:
                worst_p = max(worst_p, np.abs(np.where(g == 0, 1.0, np.exp(-g / s2)) - p).max())
    assert searched > 500
    assert worst_eq <= 1e-12, worst_eq
    assert worst_p <= 1e-12, worst_p


def test_perplexity_limit_cases_are_exact():
    d = np.array([0.5, 0.5, 0.5, 1.0, 2.0])
    for perp in (5, 5.5, 100):                                  # perplexity >= k_i
        p, beta, off = ref.perplexity_row(d, perp)
        assert np.array_equal(p, np.full(5, 0.2)) and beta == 0 and off == 0.5
    for perp in (3, 2.5, 0.1):                                  # perplexity <= the ties at the minimum
        p, beta, _ = ref.perplexity_row(d, perp)
        assert np.array_equal(p, [1 / 3, 1 / 3, 1 / 3, 0, 0]) and beta == np.inf
    p, beta, _ = ref.perplexity_row(d, 4.0)
    assert 0 < beta < np.inf and p[0] == p[1] == p[2] > p[3] > p[4] > 0
    for row in (np.full(7, 3.25), np.zeros(7)):                 # all distances equal; an all-zero row
        for perp in (0.5, 2.0, 7.0, 9.0):
            p, beta, off = ref.perplexity_row(row, perp)
            assert np.array_equal(p, np.full(7, 1 / 7)) and beta == 0 and off == row[0]
    p, beta, off = ref.perplexity_row(np.zeros(0), 2.0)         # k_i = 0
    assert p.shape == (0,) and beta == 0 and off == 0
    for perp in (0.3, 1.0, 4.0):                                # k_i = 1
        p, beta, off = ref.perplexity_row(np.array([2.0]), perp)
        assert np.array_equal(p, [1.0]) and beta == 0 and off == 2.0
    p, beta, _ = ref.perplexity_row(np.array([1.0, 2.0]), 2.0)  # k_i = 2
    assert np.array_equal(p, [0.5, 0.5]) and beta == 0
    p, beta, _ = ref.perplexity_row(np.array([1.0, 2.0]), 1.0)
    assert np.array_equal(p, [1.0, 0.0]) and beta == np.inf
    p, beta, _ = ref.perplexity_row(np.array([1.0, 2.0]), 1.5)
    assert 0 < beta < np.inf and abs(ref.entropy(beta, np.array([0.0, 3.0]))[0] - np.log(1.5)) <= 1e-12


def test_umap_limit_cases_are_exact():
    p, sigma, rho, root = ref.umap_row(np.zeros(0))             # k_i = 0
    assert p.shape == (0,) and sigma == 0 and rho == 0 and root is None
    p, sigma, rho, root = ref.umap_row(np.array([2.0]))         # k_i = 1: log2(1) = 0, c = 1
    assert np.array_equal(p, [1.0]) and rho == 2.0 and sigma == 2e-3 and root is None
    p, sigma, rho, root = ref.umap_row(np.array([1.0, 3.0]))    # k_i = 2: log2(2) = 1 <= c = 1, the limit
    assert root is None and rho == 1.0 and sigma == 1e-3 * 2.0
    assert np.array_equal(p, [1.0, np.exp(-2.0 / sigma)])
    p, sigma, rho, root = ref.umap_row(np.zeros(6))             # an all-zero row
    assert np.array_equal(p, np.ones(6)) and sigma == 0 and rho == 0
    p, sigma, rho, root = ref.umap_row(np.full(6, 4.0))         # all distances equal
    assert np.array_equal(p, np.ones(6)) and rho == 4.0 and sigma == 4e-3
    d = np.array([0.0, 0.0, 1.0, 1.0, 5.0, 6.0])                # log2(6) = 2.58 <= c = 4: zeros and the rho entries
    p, sigma, rho, root = ref.umap_row(d)
    assert root is None and rho == 1.0 and sigma == 1e-3 * d.mean()
    assert np.array_equal(p, np.where(d <= 1, 1.0, np.exp(-(d - 1.0) / sigma)))
    d = np.array([1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0, 8.0])      # an ordinary row: the nearest at full strength
    p, sigma, rho, root = ref.umap_row(d)
    assert root == sigma and p[0] == 1.0 and abs(p.sum() - 3.0) <= 1e-12


def test_perplexity_conditionals_do_not_depend_on_the_scale_of_the_distances():
    rng = np.random.default_rng(1)
    worst = 0.0
    for k in (2, 3, 15, 33, 64):
        for _ in range(20):
            d = np.sort(rng.random(k)).astype(np.float32).astype(np.float64)
            for perp in (1.5, k / 3.0, k - 0.5):
                p1, b1, _ = ref.perplexity_row(d, perp)
                p2, b2, _ = ref.perplexity_row(1000.0 * d, perp)
                worst = max(worst, np.abs(p1 - p2).max())
    assert worst <= 1e-12, worst


def test_calibrate_marks_cut_entries_and_symmetrize_equals_a_set_construction():
    rng = np.random.default_rng(2)
    n, k = 60, 6
    idx = np.stack([rng.choice(np.delete(np.arange(n), i), k, replace=False) for i in range(n)]).astype(np.int32)
    val = np.sort(rng.random((n, k)).astype(np.float32), 1)
    idx[3, 4:] = -1
    idx[7] = -1                                                  # a row with no entry
    idx[idx == 11] = -1                                          # a row listed by nobody
    idx_out, p, bandwidth, offset, solved = ref.calibrate(idx, val, "perplexity", perplexity=2.0, max_value=0.8)
    cut = (idx < 0) | (val > np.float32(0.8))
    assert np.array_equal(idx_out, np.where(cut, -1, idx)) and (p[cut] == 0).all()
    assert (p[7] == 0).all() and bandwidth[7] == 0 and offset[7] == 0 and not solved[7] and solved.sum() > 30
    rows = (~cut).any(1)
    assert np.allclose(p.sum(1)[rows], 1.0, atol=1e-12)
    p32 = p.astype(np.float32)
    want = set()
    for i in range(n):
        for c in range(k):
            if idx_out[i, c] >= 0:
                want.add((min(i, int(idx_out[i, c])), max(i, int(idx_out[i, c]))))
    for rule in ("mean", "union"):
        edges, w = ref.symmetrize(idx_out, p32, rule)
        assert [tuple(e) for e in edges.tolist()] == sorted(want)
        for (i, j), wij in zip(edges.tolist(), w):
            a = sum(p32[i, c] for c in range(k) if idx_out[i, c] == j)
            b = sum(p32[j, c] for c in range(k) if idx_out[j, c] == i)
            expect = np.float32(0.5) * (np.float32(a) + np.float32(b)) if rule == "mean" else np.float32(
                float(a) + float(b) - float(a) * float(b))
            assert wij == expect


def test_argument_errors_need_no_device():
    from pymde_amd import affinity
    for bad in ("gaussian", None, 3):
        with pytest.raises(ValueError, match="unknown affinity kind"):
            affinity.resolve_kind(bad)
    with pytest.raises(ValueError, match="unknown symmetrisation rule"):
        affinity.resolve_rule("max")
    for bad in (0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="perplexity must be"):
            affinity.resolve_perplexity("perplexity", bad)
    with pytest.raises(ValueError, match="perplexity belongs to"):
        affinity.parse_weights({"kind": "umap", "perplexity": 5})
    with pytest.raises(ValueError, match="unknown keys"):
        affinity.parse_weights({"kind": "umap", "sigma": 1.0})
    with pytest.raises(ValueError, match="weights must be"):
        affinity.parse_weights(1.0)
    assert affinity.parse_weights(None) is None
    assert affinity.parse_weights("UMAP") == ("umap", None, "union")
    assert affinity.parse_weights({"perplexity": 5}) == ("perplexity", 5.0, "mean")
    assert affinity.resolve_perplexity("perplexity", None, 15) == 5.0

"""pymde_amd.quality's global scores without a GPU: ``_scores_from_moments`` against the textbook formulas
evaluated in numpy float64 on brute-force distance matrices, and the argument errors that are raised before any
device is touched."""
import math

import numpy as np
import pytest
import torch

from pymde_amd import quality

N = 60


def _dist(A):
    A = np.asarray(A, dtype=np.float64)
    return np.sqrt(((A[:, None, :] - A[None, :, :]) ** 2).sum(-1))


def _moments(D, E, rows=None):
    """A PairMoments of the off-diagonal pairs of two dense float64 distance matrices (query rows ``rows``)."""
    n = D.shape[0]
    rows = np.arange(n) if rows is None else np.asarray(rows)
    off = np.ones((len(rows), n), dtype=bool)
    off[np.arange(len(rows)), rows] = False
    d, e = D[rows], E[rows]
    sums = np.stack([np.where(off, v, 0.0).sum(1) for v in (d, e, d * d, e * e, d * e)], 1)
    t = sums.sum(0)
    return quality.PairMoments(int(off.sum()), t[0], t[1], t[2], t[3], t[4], d[off].max(), e[off].max(),
                               torch.tensor(sums, dtype=torch.float64), None)


@pytest.fixture(scope="module")
def case():
    rng = np.random.default_rng(0)
    data = rng.standard_normal((N, 7)) * rng.uniform(0.2, 3.0, 7)
    X = data[:, :2] * 0.7 + 0.3 * rng.standard_normal((N, 2))
    D, E = _dist(data), _dist(X)
    off = ~np.eye(N, dtype=bool)
    return data, D, E, D[off], E[off]


def test_optimal_stress_is_the_minimum_over_alpha(case):
    _, D, E, d, e = case
    s = quality._scores_from_moments(_moments(D, E))
    alpha = (d * e).sum() / (e * e).sum()
    want = math.sqrt(((d - alpha * e) ** 2).sum() / (d * d).sum())
    assert abs(s.alpha - alpha) <= 1e-13 * alpha
    assert abs(s.stress - want) <= 1e-12
    assert 0.05 < want < 1.0                                   # a case with something to measure
    for a in (0.9 * alpha, 1.1 * alpha):                       # and it is the minimum
        assert quality._scores_from_moments(_moments(D, E), scale=a).stress > s.stress


@pytest.mark.parametrize("alpha", [1.0, 0.5, 2.25])
def test_fixed_scale_stress(case, alpha):
    _, D, E, d, e = case
    s = quality._scores_from_moments(_moments(D, E), scale=alpha)
    assert s.alpha == alpha
    assert abs(s.stress - math.sqrt(((d - alpha * e) ** 2).sum() / (d * d).sum())) <= 1e-12


def test_correlation_is_pearson_r(case):
    _, D, E, d, e = case
    s = quality._scores_from_moments(_moments(D, E))
    assert abs(s.correlation - np.corrcoef(d, e)[0, 1]) <= 1e-12
    assert quality._scores_from_moments(_moments(D, E), scale=3.0).correlation == s.correlation


@pytest.mark.parametrize("scale", ["optimal", 1.0])
def test_per_item(case, scale):
    _, D, E, d, e = case
    rows = np.array([5, 3, 59, 0, 17])                         # a sample: per-item follows the query rows
    for m in (_moments(D, E), _moments(D, E, rows)):
        s = quality._scores_from_moments(m, scale=scale, per_item=True)
        q = np.arange(N) if m.row_sums.shape[0] == N else rows
        off = np.ones((len(q), N), dtype=bool)
        off[np.arange(len(q)), q] = False
        num = np.where(off, (D[q] - s.alpha * E[q]) ** 2, 0.0).sum(1)
        want = np.sqrt(num / np.where(off, D[q] ** 2, 0.0).sum(1))
        assert s.per_item.dtype == torch.float32 and s.per_item.shape == (len(q),)
        assert np.abs(s.per_item.numpy() - want).max() <= 2.0 ** -23 * want.max()
    assert quality._scores_from_moments(_moments(D, E), scale=scale).per_item is None


def test_an_isometric_copy_scores_zero_and_one(case):
    data, D, _, _, _ = case
    theta = 0.7
    R = np.eye(7)
    R[:2, :2] = [[math.cos(theta), -math.sin(theta)], [math.sin(theta), math.cos(theta)]]
    E = _dist(data @ R + 3.0)                                   # rotated and translated
    for scale in ("optimal", 1.0):
        s = quality._scores_from_moments(_moments(D, E), scale=scale, per_item=True)
        assert s.stress <= 1e-7                                 # sqrt of float64 cancellation noise
        assert abs(s.correlation - 1.0) <= 1e-12
        assert float(s.per_item.max()) <= 1e-6
    assert abs(quality._scores_from_moments(_moments(D, E)).alpha - 1.0) <= 1e-12


@pytest.mark.parametrize("factor", [0.25, 3.0])
def test_a_scaled_copy(case, factor):
    """E = factor * D: the optimal scale undoes it (stress 0, alpha 1 / factor); a fixed alpha = 1 does not:
    sqrt(sum (D - factor D)^2 / sum D^2) = |1 - factor|, which is |1 - 1 / s| for an embedding shrunk by s."""
    _, D, _, _, _ = case
    m = _moments(D, factor * D)
    s = quality._scores_from_moments(m)
    assert s.stress <= 1e-7 and abs(s.alpha * factor - 1.0) <= 1e-12 and abs(s.correlation - 1.0) <= 1e-12
    fixed = quality._scores_from_moments(m, scale=1.0)
    assert abs(fixed.stress - abs(1.0 - factor)) <= 1e-12
    assert abs(fixed.stress - abs(1.0 - 1.0 / (1.0 / factor))) <= 1e-12


def test_degenerate_moments_are_nan():
    z = torch.zeros((2, 5), dtype=torch.float64)
    s = quality._scores_from_moments(quality.PairMoments(2, 0.0, 2.0, 0.0, 2.0, 0.0, 0.0, 1.0, z, None))
    assert math.isnan(s.stress) and math.isnan(s.correlation)


# ---------------------------------------------------------------- argument errors, before any device
class _Graph:
    edges, n_items = None, 10


def _no_device(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("a device was asked for")
    monkeypatch.setattr(quality, "_device_of", boom)
    monkeypatch.setattr(quality._lib, "load", boom)


ENTRY_POINTS = [quality.pair_moments, quality.stress, quality.distance_correlation, quality.shepard_histogram]


@pytest.mark.parametrize("score", ENTRY_POINTS)
def test_argument_errors_need_no_device(score, monkeypatch):
    _no_device(monkeypatch)
    data, X = np.zeros((10, 4), dtype=np.float32), np.zeros((10, 2), dtype=np.float32)
    with pytest.raises(ValueError, match="'euclidean', 'cosine' and 'correlation'"):
        score(data, X, metric="manhattan")
    with pytest.raises(ValueError, match="Graph"):
        score(_Graph(), X)
    with pytest.raises(ValueError, match="Graph"):
        score(data, _Graph())
    with pytest.raises(ValueError, match="10 rows and the embedding `X` has 9"):
        score(data, X[:9])
    with pytest.raises(ValueError, match="matrix"):
        score(data, X[:, 0])
    with pytest.raises(ValueError, match="at least two rows"):
        score(data[:1], X[:1])
    for sample in (0, 11, -1, 2.5):
        with pytest.raises(ValueError, match="sample"):
            score(data, X, sample=sample)
    with pytest.raises(ValueError, match="unknown metric"):
        score(data, X, metric="chebyshev")


def test_histogram_and_stress_argument_errors_need_no_device(monkeypatch):
    _no_device(monkeypatch)
    data, X = np.zeros((10, 4), dtype=np.float32), np.zeros((10, 2), dtype=np.float32)
    for bins in (0, 65, -3, 2.5):
        with pytest.raises(ValueError, match="bins"):
            quality.shepard_histogram(data, X, bins=bins)
    bad_ranges = [((0.0, 1.0),), ((1.0, 1.0), (0.0, 1.0)), ((0.0, 1.0), (2.0, 1.0)), ((0.0, float("inf")), (0.0, 1.0)),
                  ((0.0, float("nan")), (0.0, 1.0)), (0.0, 1.0), "ab", ((0.0, 1.0, 2.0), (0.0, 1.0))]
    for r in bad_ranges:
        with pytest.raises(ValueError, match="range"):
            quality.shepard_histogram(data, X, range=r)
    for scale in ("best", 0.0, -1.0, float("nan"), float("inf"), None):
        with pytest.raises(ValueError, match="scale"):
            quality.stress(data, X, scale=scale)
    m = quality.PairMoments(2, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, torch.ones((2, 5), dtype=torch.float64), None)
    with pytest.raises(ValueError, match="scale"):
        quality._scores_from_moments(m, scale="best")


def test_sampled_rows_are_distinct_and_follow_the_seed():
    a, b = quality._sample_rows(1000, 70, 0), quality._sample_rows(1000, 70, 0)
    assert torch.equal(a, b) and a.dtype == torch.int64 and a.shape == (70,)
    assert len(set(a.tolist())) == 70 and 0 <= int(a.min()) and int(a.max()) < 1000
    assert not torch.equal(a, quality._sample_rows(1000, 70, 1))
    assert a.tolist() != sorted(a.tolist())                    # out of order

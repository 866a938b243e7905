"""pymde_amd.quality without a GPU: the score formula against the values scikit-learn gave
(tests/golden/quality.npz, recorded by tests/golden/make_quality.py), and the argument errors that are raised
before any device is required."""
import numpy as np
import pytest
import torch

from conftest import load_golden
from pymde_amd import quality


@pytest.fixture(scope="module")
def golden():
    return load_golden("quality")


def _ranks_f64(A):
    """0-based rank of every row among the other rows of each row of ``A``, by (squared distance in float64,
    index): ranks[i, j], and n - 1 on the diagonal (a row is not ranked against itself)."""
    A = np.asarray(A, dtype=np.float64)
    n = A.shape[0]
    d2 = ((A[:, None, :] - A[None, :, :]) ** 2).sum(-1)
    d2[np.arange(n), np.arange(n)] = np.inf
    ranks = np.empty((n, n), dtype=np.int64)
    for i in range(n):
        order = np.lexsort((np.arange(n), d2[i]))
        ranks[i, order] = np.arange(n)
    return ranks


def _cross_ranks(listed, ranked, k):
    """The ranks in ``ranked`` of the k nearest neighbours in ``listed`` of every row: int64 [n, k]."""
    knn = np.argsort(_ranks_f64(listed), axis=1)[:, :k]
    return np.take_along_axis(_ranks_f64(ranked), knn, axis=1)


def test_score_from_ranks_reproduces_sklearn(golden):
    data, X, k = golden["data"], golden["X"], int(golden["n_neighbors"])
    n = data.shape[0]
    t = quality._score_from_ranks(torch.from_numpy(_cross_ranks(X, data, k)), n, k)
    c = quality._score_from_ranks(torch.from_numpy(_cross_ranks(data, X, k)), n, k)
    assert isinstance(t, float) and isinstance(c, float)
    assert abs(t - float(golden["trustworthiness"])) <= 1e-12
    assert abs(c - float(golden["continuity"])) <= 1e-12
    assert abs(t - 0.49688934566632414) <= 1e-12 and abs(c - 0.5083453237410072) <= 1e-12


def test_score_from_ranks_per_item_and_perfect_ranks(golden):
    data, X, k = golden["data"], golden["X"], int(golden["n_neighbors"])
    n = data.shape[0]
    ranks = torch.from_numpy(_cross_ranks(X, data, k)).to(torch.int32)
    score, rows = quality._score_from_ranks(ranks, n, k, per_item=True)
    assert rows.shape == (n,) and rows.dtype == torch.float32
    assert abs(float(rows.double().mean()) - score) <= 1e-6      # float32 rows
    own = torch.arange(k, dtype=torch.int32).repeat(n, 1)          # a search's own lists: nothing is penalised
    assert quality._score_from_ranks(own, n, k) == 1.0
    own[3, 2] = -1                                                 # an entry that is not ranked costs nothing
    assert quality._score_from_ranks(own, n, k) == 1.0


@pytest.mark.parametrize("n,k", [(10, 5), (10, 6), (11, 6), (10, 0), (2, 1)])
def test_too_many_neighbors_raise(n, k):
    ranks = torch.zeros((n, max(k, 1)), dtype=torch.int32)
    with pytest.raises(ValueError, match="n_samples / 2"):
        quality._score_from_ranks(ranks, n, k)
    data, X = np.zeros((n, 3), dtype=np.float32), np.zeros((n, 2), dtype=np.float32)
    for score in (quality.trustworthiness, quality.continuity):
        with pytest.raises(ValueError, match="n_samples / 2"):
            score(data, X, n_neighbors=k)


class _GraphLike(object):
    edges = None
    n_items = 10


def test_unsupported_metric_and_graph_raise_before_any_device():
    data, X = np.zeros((10, 3), dtype=np.float32), np.zeros((10, 2), dtype=np.float32)
    idx = np.zeros((10, 2), dtype=np.int32)
    for name in ("manhattan", "l1", "cityblock"):
        for call in (lambda: quality.trustworthiness(data, X, 2, metric=name),
                     lambda: quality.continuity(data, X, 2, metric=name),
                     lambda: quality.neighbor_overlap(data, X, 2, metric=name),
                     lambda: quality.neighbor_ranks(None, data, idx, self_join=True, metric=name)):
            with pytest.raises(ValueError, match="'euclidean', 'cosine' and 'correlation'"):
                call()
    with pytest.raises(ValueError, match="unknown metric"):
        quality.trustworthiness(data, X, 2, metric="chebyshev")
    for call in (lambda: quality.trustworthiness(_GraphLike(), X, 2),
                 lambda: quality.continuity(_GraphLike(), X, 2),
                 lambda: quality.neighbor_overlap(_GraphLike(), X, 2),
                 lambda: quality.neighbor_ranks(None, _GraphLike(), idx, self_join=True),
                 lambda: quality.neighbor_ranks(_GraphLike(), data, idx)):
        with pytest.raises(ValueError, match="Graph"):
            call()


def test_argument_errors_raise_before_any_device():
    data, X = np.zeros((10, 3), dtype=np.float32), np.zeros((10, 2), dtype=np.float32)
    idx = np.zeros((10, 2), dtype=np.int32)
    with pytest.raises(ValueError, match="1 to 64"):
        quality.neighbor_ranks(None, data, np.zeros((10, 0), dtype=np.int32), self_join=True)
    with pytest.raises(ValueError, match="1 to 64"):
        quality.neighbor_ranks(None, data, np.zeros((10, 65), dtype=np.int32), self_join=True)
    with pytest.raises(ValueError, match="slices"):
        quality.neighbor_ranks(None, data, idx, self_join=True, slices=65536)
    with pytest.raises(ValueError, match="slices"):
        quality.neighbor_ranks(None, data, idx, self_join=True, slices=-1)
    with pytest.raises(ValueError, match="features"):
        quality.neighbor_ranks(np.zeros((10, 4), dtype=np.float32), data, idx)
    with pytest.raises(ValueError, match="rows for"):
        quality.neighbor_ranks(np.zeros((7, 3), dtype=np.float32), data, idx)
    with pytest.raises(ValueError, match="self_join"):
        quality.neighbor_ranks(X, data, idx, self_join=True)
    with pytest.raises(ValueError, match="must agree"):
        quality.trustworthiness(data, X[:9], 2)
    with pytest.raises(ValueError, match="n_neighbors"):
        quality.neighbor_overlap(data, X, 10)
    with pytest.raises(ValueError, match="unknown precision"):
        quality.neighbor_overlap(data, X, 2, precision="float16")
    with pytest.raises(ValueError, match="longest neighbour list"):
        quality.trustworthiness(np.zeros((200, 3), dtype=np.float32), np.zeros((200, 2), dtype=np.float32), 65)

"""The ``metric=`` keyword without a GPU (pymde_amd/metrics.py): names and aliases, and the errors that are
raised before any device is required -- an unknown name, a Graph with a metric of its own choice, the
approximate search under Manhattan."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from pymde_amd import graph, metrics, preprocess, recipes


def test_names_and_aliases_resolve():
    for name in ("euclidean", "cosine", "correlation", "manhattan"):
        assert metrics.resolve(name) == name
        assert metrics.resolve(name.upper()) == name
    assert metrics.resolve("l2") == "euclidean"
    assert metrics.resolve("l1") == "manhattan"
    assert metrics.resolve("cityblock") == "manhattan"
    assert set(metrics.CODES) == set(metrics.METRICS)


def test_metric_codes_match_the_header():
    text = open(os.path.join(ROOT, "include", "mde_hip.h")).read()
    for name, code in metrics.CODES.items():
        m = re.search(r"#define MDE_METRIC_%s (\d+)" % name.upper(), text)
        assert m and int(m.group(1)) == code, name


@pytest.mark.parametrize("bad", ["chebyshev", "jaccard", "", None, 3])
def test_unknown_metric_is_a_value_error_without_a_gpu(bad):
    X = np.zeros((20, 3), dtype=np.float32)
    with pytest.raises(ValueError):
        metrics.resolve(bad)
    with pytest.raises(ValueError):
        preprocess.k_nearest_neighbors(X, 3, metric=bad)
    with pytest.raises(ValueError):
        recipes.distances(X, metric=bad)
    with pytest.raises(ValueError):
        recipes.preserve_neighbors(X, metric=bad)
    with pytest.raises(ValueError):
        recipes.preserve_distances(X, metric=bad)
    with pytest.raises(ValueError):
        recipes.laplacian_embedding(X, metric=bad)


class _GraphLike(object):
    """What ``preprocess.k_nearest_neighbors`` takes for a graph: edges and n_items."""
    edges = np.array([[0, 1], [1, 2]])
    n_items = 3


@pytest.mark.parametrize("metric", ["cosine", "correlation", "manhattan", "l1", "cityblock"])
def test_graph_with_a_metric_is_a_value_error(metric):
    with pytest.raises(ValueError, match="Graph"):
        preprocess.k_nearest_neighbors(_GraphLike(), 1, metric=metric)
    g = object.__new__(graph.Graph)      # (building a Graph needs a device; the check comes before it is used)
    with pytest.raises(ValueError, match="Graph"):
        recipes.preserve_neighbors(g, metric=metric)
    with pytest.raises(ValueError, match="Graph"):
        recipes.preserve_distances(g, metric=metric)
    with pytest.raises(ValueError, match="Graph"):
        recipes.laplacian_embedding(g, metric=metric)


@pytest.mark.parametrize("metric", ["manhattan", "l1", "cityblock"])
def test_approximate_manhattan_is_a_value_error(metric):
    X = np.zeros((20, 3), dtype=np.float32)
    with pytest.raises(ValueError, match="Manhattan"):
        preprocess.k_nearest_neighbors(X, 3, metric=metric, approximate=True)
    with pytest.raises(ValueError, match="Manhattan"):
        recipes.preserve_neighbors(X, metric=metric, approximate_neighbors=True)
    with pytest.raises(ValueError, match="Manhattan"):
        recipes.laplacian_embedding(X, metric=metric, approximate_neighbors={"n_lists": 4, "n_probe": 2})
    metrics.check_approximate("cosine", True)           # the metrics that reduce to a Euclidean search pass
    metrics.check_approximate("correlation", True)
    metrics.check_approximate(metric, False)


def test_translation_rule():
    """A Euclidean search is translated to the column means when |mean|^2 exceeds the summed column variance
    (DESIGN section 6): not on the data the goldens use, on every input whose offset dominates."""
    rng = np.random.default_rng(0)

    def pays(X):
        X = X.astype(np.float32).astype(np.float64)
        return metrics.translation_pays(X.mean(0), X.var(0))

    Z = rng.standard_normal((1037, 50))
    assert not pays(Z)                                  # N(0, 1): |mean|^2 ~ nf / n
    assert not pays(Z + 0.5)                            # 0.25 nf against nf
    assert pays(Z + 1.5) and pays(Z + 100.0) and pays(Z + 1000.0)
    shifted = Z.copy()
    shifted[:, 7] += 1e4                                # one column carries the offset
    assert pays(shifted)
    assert pays(rng.random((1000, 20)))                 # U(0, 1): 0.25 nf against nf / 12
    assert not metrics.translation_pays([1.0, 1.0], [1.0, 1.0])        # equality: searched as given
    assert metrics.translation_pays([1.0, 1.0 + 1e-9], [1.0, 1.0])
    assert not metrics.translation_pays([0.0, 0.0], [0.0, 0.0])        # constant zero data
    assert metrics.translation_pays([3.0], [0.0])                      # identical non-zero rows


def test_translation_vector_stays_on_the_grid_of_the_data():
    """The column means are rounded to a power-of-two grid no coarser than the column's standard deviation:
    within half a standard deviation of the mean, and integer data stay integers (exact float32 arithmetic
    and its ties survive the translation)."""
    rng = np.random.default_rng(1)
    X = rng.integers(0, 4, (3001, 20)).astype(np.float64)
    mu = metrics.grid_means(X.mean(0), X.var(0)).numpy()
    assert set(mu.tolist()) <= {1.0, 2.0}
    Y = 1000.0 + rng.standard_normal((1037, 50)) * rng.uniform(0.01, 30.0, 50)
    Y[:, 3] = 7.25                                      # a constant column keeps its mean
    mean, var = Y.mean(0), Y.var(0)
    mu = metrics.grid_means(mean, var).numpy()
    assert mu[3] == mean[3]
    live = var > 0
    assert (np.abs(mu - mean)[live] <= 0.5 * np.sqrt(var[live])).all()
    step = 2.0 ** np.floor(np.log2(np.sqrt(var[live])))
    np.testing.assert_array_equal(mu[live] / step, np.round(mu[live] / step))
    assert ((mu - mean) ** 2).sum() <= 0.25 * var.sum()

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

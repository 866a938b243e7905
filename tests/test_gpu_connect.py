"""``preprocess.connect_components`` and the ``connect=`` keyword of ``preprocess.neighbor_graph`` and
``recipes.preserve_geodesics`` against tests/_components_reference.py: the bridges of both rules on
integer blobs (exact), and the Isomap replay of three planar clusters, where the two rules differ visibly."""
import numpy as np
import pytest
import torch

import pymde_amd
from pymde_amd import classical, preprocess, quality
from pymde_amd import graph as G

import _components_reference as ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def blobs():
    """6 blobs x 40 rows on the integer grid of R^5, their 3-NN graph, its components by scipy and the float64 table."""
    X = ref.grid_blobs(6, 40, seed=0)
    g = preprocess.neighbor_graph(X, 3)
    edges = g.edges.cpu().numpy()
    count, labels = ref.components(len(X), edges)
    assert count >= 3                                              # several components: the premise of the tests
    d2, row = ref.nearest_pairs(X, labels, count)
    return X, g, count, labels, d2, row


@pytest.mark.parametrize("rule", ["pairs", "tree"])
def test_bridges_equal_the_reference(blobs, rule):
    X, g, count, labels, d2, row = blobs
    got = preprocess.connect_components(X, g, bridges=rule)
    assert isinstance(got, preprocess.Connection)
    assert got.n_components == count and np.array_equal(got.labels.cpu().numpy(), labels)
    want_edges, want_d2 = ref.bridges(d2, row, rule)
    assert len(want_edges) == (count * (count - 1) // 2 if rule == "pairs" else count - 1)
    assert got.bridges.dtype == torch.int64 and np.array_equal(got.bridges.cpu().numpy(), want_edges)
    assert got.lengths.dtype == torch.float32
    assert np.array_equal(got.lengths.cpu().numpy(), np.sqrt(want_d2.astype(np.float32)))   # (d2 is exact in float32)
    assert G.connected_components(got.graph)[0] == 1
    # the new graph: unique sorted edges, the old ones with their old bits, the bridges with their lengths
    n = len(X)
    new_edges, new_values = got.graph.edges.cpu().numpy(), got.graph.distances.cpu().numpy()
    key = new_edges[:, 0] * n + new_edges[:, 1]
    assert (new_edges[:, 0] < new_edges[:, 1]).all() and (np.diff(key) > 0).all()
    assert len(key) == g.n_edges + len(want_edges)
    old_key = g.edges.cpu().numpy()[:, 0] * n + g.edges.cpu().numpy()[:, 1]
    at = np.searchsorted(key, old_key)
    assert np.array_equal(key[at], old_key)
    assert np.array_equal(new_values[at].view(np.int32), g.distances.cpu().numpy().view(np.int32))
    at = np.searchsorted(key, want_edges[:, 0] * n + want_edges[:, 1])
    assert np.array_equal(new_values[at].view(np.int32), got.lengths.cpu().numpy().view(np.int32))


def test_neighbor_graph_keyword(blobs):
    X, g, count, _, _, _ = blobs
    plain = preprocess.neighbor_graph(X, 3, connect=False)
    assert torch.equal(plain.edges, g.edges)
    assert torch.equal(plain.distances.view(torch.int32), g.distances.view(torch.int32))
    for value, rule in ((True, "pairs"), ("pairs", "pairs"), ("tree", "tree")):
        joined = preprocess.neighbor_graph(X, 3, connect=value)
        want = preprocess.connect_components(X, g, bridges=rule).graph
        assert torch.equal(joined.edges, want.edges) and torch.equal(joined.distances, want.distances)
    with pytest.raises(ValueError, match="bridging rule"):
        preprocess.neighbor_graph(X, 3, connect="forest")
    with pytest.raises(ValueError, match="Manhattan"):
        preprocess.neighbor_graph(X, 3, metric="manhattan", connect=True)


def test_a_connected_graph_comes_back_unchanged():
    X = ref.grid_blobs(1, 70, seed=3)
    g = preprocess.neighbor_graph(X, 10)
    assert ref.components(len(X), g.edges.cpu().numpy())[0] == 1
    got = preprocess.connect_components(X, g)
    assert got.graph is g and got.n_components == 1
    assert tuple(got.bridges.shape) == (0, 2) and tuple(got.lengths.shape) == (0,)
    assert int(got.labels.max()) == 0


@pytest.fixture(scope="module")
def clusters():
    X, true = ref.three_clusters()
    return X, true


@pytest.mark.parametrize("rule", ["pairs", "tree"])
def test_isomap_of_three_clusters_follows_the_float64_replay(clusters, rule):
    X, true = clusters
    want, count = ref.isomap_centroid_ratios(X, 6, rule, 60, true)
    assert count == 3
    g = preprocess.neighbor_graph(X, 6, connect=rule)
    D = G.distances_from(g, np.arange(len(X)))
    assert bool(torch.isfinite(D).all())
    Y = classical.classical_mds(distance_matrix=D).X.cpu().numpy()
    got = ref.centroid_distances(Y, 60) / true
    print(rule, "ratios", got, "replay", want)
    assert np.abs(got - want).max() <= 0.05
    if rule == "pairs":
        assert (got < 1.2).all()
    else:
        assert got.max() > 1.3                                     # the long side runs through the third cluster


def test_preserve_geodesics_connect(clusters):
    X, _ = clusters
    mde = pymde_amd.preserve_geodesics(X, n_neighbors=6, landmarks=40, connect=True, seed=0)
    assert mde.init == "classical"
    assert mde.connection.n_components == 3 and tuple(mde.connection.bridges.shape) == (3, 2)
    Y = mde.embed(max_iter=20)
    assert quality.graph_moments(mde.connection.graph, Y).missing == 0
    plain = pymde_amd.preserve_geodesics(X, n_neighbors=6, landmarks=40, seed=0)
    assert plain.init == "random" and not hasattr(plain, "connection")


def test_argument_errors(blobs):
    X, g, _, _, _, _ = blobs
    with pytest.raises(ValueError, match="Graph"):
        pymde_amd.preserve_geodesics(g, landmarks=40, connect=True)
    with pytest.raises(ValueError, match="must agree"):
        preprocess.connect_components(X[:-1], g)
    with pytest.raises(ValueError, match="bridging rule"):
        preprocess.connect_components(X, g, bridges="forest")
    with pytest.raises(ValueError, match="Graph"):
        preprocess.connect_components(X, X)

"""``graph.connected_components`` (csrc/mde_graph_components.hip) against
``scipy.sparse.csgraph.connected_components``: the labels compare with ``==`` (both number the components by their
smallest node), the count agrees, and a second run gives the same tensor."""
import math

import numpy as np
import pytest
import torch

from pymde_amd import graph as G

import _components_reference as ref

pytestmark = pytest.mark.gpu


def build(n, edges, values=None):
    edges = torch.as_tensor(np.asarray(edges, dtype=np.int64).reshape(-1, 2))
    return G.Graph.from_edges(edges, None if values is None else torch.as_tensor(values), n_items=n)


def check(n, edges, values=None):
    g = build(n, edges, values)
    count, labels = G.connected_components(g)
    assert labels.dtype == torch.int64 and labels.is_cuda and tuple(labels.shape) == (n,)
    want_count, want = ref.components(n, edges)
    assert count == want_count
    assert np.array_equal(labels.cpu().numpy(), want)
    again_count, again = G.connected_components(g)
    assert again_count == count and torch.equal(again, labels)
    return G.last_components_stats()


@pytest.mark.parametrize("n,edges", [(1, []), (2, []), (2, [[0, 1]])])
def test_one_and_two_nodes(n, edges):
    stats = check(n, edges)
    if not edges:
        assert stats["rounds"] == 0 and stats["hooks"] == 0


@pytest.mark.parametrize("n", [63, 64, 65, 257])
@pytest.mark.parametrize("degree", [0.5, 1, 3])
def test_random_graphs_of_many_components(n, degree):
    edges = ref.random_edges(n, degree, seed=1000 * n + int(10 * degree))
    count, labels = ref.components(n, edges)
    if degree < 3:
        assert count > 3 and (np.bincount(labels) == 1).any()      # several components, isolated nodes
    stats = check(n, edges)
    assert 1 <= stats["rounds"] <= 8 * math.ceil(math.log2(n))


def test_no_edges_gives_n_components():
    g = build(300, [])
    count, labels = G.connected_components(g)
    assert count == 300 and torch.equal(labels.cpu(), torch.arange(300))


def test_star_takes_the_wave_per_row_launch():
    n, edges = ref.star_with_isolated(5000, 100)
    stats = check(n, edges)
    assert ref.components(n, edges)[0] == 101
    # init + (hook, heavy hook, jump) per round + the three label launches
    assert stats["launches"] == 1 + 3 * stats["rounds"] + 3
    # and the hub elsewhere than at node 0: its leaves hook below it or it below them
    e2 = edges.copy()
    e2[e2 == 0] = -1
    e2[e2 == 2500] = 0
    e2[e2 == -1] = 2500
    check(n, np.stack([e2.min(axis=1), e2.max(axis=1)], axis=1))


def test_edge_values_are_not_read():
    n = 257
    edges = ref.random_edges(n, 1, seed=5)
    values = np.random.default_rng(5).choice(np.array([0.0, 0.5, 2.0], dtype=np.float32), size=len(edges))
    assert (values == 0).any()
    g = G.Graph._from_unique_edges(torch.as_tensor(edges, device="cuda"), torch.as_tensor(values, device="cuda"), n)
    count, labels = G.connected_components(g)
    want_count, want = ref.components(n, edges)
    assert count == want_count and np.array_equal(labels.cpu().numpy(), want)
    g.distances[0] = float("inf")
    assert torch.equal(G.connected_components(g)[1], labels)


def test_long_path_under_a_random_renumbering():
    n = 20000
    edges = ref.renumbered_path(n, seed=0)
    count, labels = G.connected_components(build(n, edges))
    stats = G.last_components_stats()
    print("rounds on the renumbered path of %d nodes: %s" % (n, stats))
    assert count == 1 and int(labels.max()) == 0
    bound = 8 * math.ceil(math.log2(n))
    assert bound == 120 and stats["rounds"] <= bound
    assert ref.hook_and_jump(n, edges)[1] <= bound                 # the host replay, on the same graph


def test_a_non_graph_is_refused():
    with pytest.raises(ValueError):
        G.connected_components(torch.zeros((3, 3)))
    with pytest.raises(ValueError):
        G.connected_components(None)

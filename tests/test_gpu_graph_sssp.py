"""``graph.distances_from`` (csrc/mde_graph_sssp.hip) against scipy's Dijkstra in float64
(tests/_graph_sssp_reference.py).  With edge lengths that are multiples of 2^-6 every path sum is exact in float32 and
the comparison is exact, 0 at the sources and inf at unreachable nodes included; with generic lengths the bound is
the n 2^-24 of L - 1 roundings on a path of L <= n hops, and the bits are those of ``graph.shortest_paths``."""
import numpy as np
import pytest
import torch

from pymde_amd import _lib
from pymde_amd import graph as G

import _graph_sssp_reference as ref

pytestmark = pytest.mark.gpu

GRAPHS = {"cycle": ref.cycle, "random": ref.random_graph, "star": ref.star_with_tail, "pair": ref.pair}


def build(n, edges, lengths):
    return G.Graph.from_edges(torch.as_tensor(edges), torch.as_tensor(lengths), n_items=n)


def source_lists(n):
    rng = np.random.default_rng(n)
    lists = {"m%d" % m: rng.integers(0, n, size=m) for m in (1, 63, 64, 65, 130)}
    lists["descending"] = np.arange(n - 1, -1, -1)[:70]
    lists["repeated"] = np.array([n - 1, 0, n - 1, n // 2])
    lists["all"] = np.arange(n)
    return lists


@pytest.mark.parametrize("name", sorted(GRAPHS))
def test_exact_lengths_equal_float64_dijkstra(name):
    n, edges, lengths = GRAPHS[name]()
    g = build(n, edges, lengths)
    for label, sources in source_lists(n).items():
        got = G.distances_from(g, sources)
        assert got.dtype == torch.float32 and tuple(got.shape) == (n, len(sources)) and got.is_cuda
        want = ref.distances_from(n, edges, lengths, sources)
        assert np.array_equal(got.cpu().numpy().astype(np.float64), want), (name, label)
        assert (got[torch.as_tensor(sources), torch.arange(len(sources))] == 0).all()
        if label == "repeated":
            assert torch.equal(got[:, 0], got[:, 2])
    stats = G.last_distances_stats()
    assert 1 <= stats["sweeps"] <= n and stats["tiles_per_sweep"] == n * ((n + 63) // 64)
    if name == "cycle":
        # half way round is 128 hops; a sweep may carry a value further than one hop (it relaxes in place), so only
        # "the read-back loop went round more than once" is certain
        print("sweeps on the 257-cycle:", stats["sweeps"])
        assert stats["sweeps"] > 4
    if name == "star":
        assert stats["heavy_nodes"] == 1   # the hub went to the many-wave kernel


def test_unreachable_nodes_are_inf():
    n, edges, lengths = ref.random_graph()
    comp = ref.components(n, edges)
    assert len(set(comp)) > 3 and (np.bincount(comp) == 1).any()    # several components, isolated nodes
    got = G.distances_from(build(n, edges, lengths), np.arange(n)).cpu().numpy()
    assert np.array_equal(np.isinf(got), comp[:, None] != comp[None, :])


@pytest.mark.parametrize("name", ["cycle", "random"])
def test_unit_lengths_are_hop_counts(name):
    n, edges, _ = GRAPHS[name]()
    g = build(n, edges, np.ones(len(edges), dtype=np.float32))
    sources = np.arange(0, n, 3)
    got = G.distances_from(g, sources).cpu().numpy().astype(np.float64)
    assert np.array_equal(got, ref.distances_from(n, edges, np.ones(len(edges)), sources))


@pytest.fixture(scope="module")
def generic():
    n, edges, lengths = ref.random_graph(300, 1500, seed=5, generic=True)
    g = build(n, edges, lengths)
    return n, edges, lengths, g, G.distances_from(g, np.arange(n))


def test_generic_lengths_within_the_rounding_bound(generic):
    n, edges, lengths, _, got = generic
    want = ref.distances_from(n, edges, lengths, np.arange(n))
    got = got.cpu().numpy().astype(np.float64)
    finite = np.isfinite(want)
    assert np.array_equal(np.isfinite(got), finite)
    excess = np.abs(got[finite] - want[finite]) - n * 2.0 ** -24 * want[finite]
    print("largest |got - ref| / ref: %.3g (bound %.3g)" % (
        (np.abs(got[finite] - want[finite]) / np.maximum(want[finite], 1e-300)).max(), n * 2.0 ** -24))
    assert (excess <= 0).all()


def test_generic_lengths_have_the_bits_of_shortest_paths(generic):
    n, _, _, g, got = generic
    paths = G.shortest_paths(g)
    s, v = paths.edges[:, 0], paths.edges[:, 1]             # s < v
    assert torch.equal(got[v, s].view(torch.int32), paths.distances.view(torch.int32))
    # and the pairs it does not list are the unreachable ones
    upper = torch.triu(torch.ones(n, n, dtype=torch.bool, device=got.device), diagonal=1)
    assert int((torch.isfinite(got.T) & upper).sum()) == int(s.numel())


@pytest.mark.parametrize("which", ["cycle", "generic"])
def test_max_length(which, generic):
    if which == "cycle":
        n, edges, lengths = ref.cycle()
        g, limit = build(n, edges, lengths), 40.0
        full = G.distances_from(g, np.arange(0, n, 2))
        got = G.distances_from(g, np.arange(0, n, 2), max_length=limit)
        limited = ref.distances_from(n, edges, lengths, np.arange(0, n, 2), max_length=limit)
        assert np.array_equal(got.cpu().numpy().astype(np.float64), limited)
    else:
        n, _, _, g, full = generic
        limit = float(full[torch.isfinite(full)].median())
        got = G.distances_from(g, np.arange(n), max_length=limit)
    want = torch.where(full <= limit, full, torch.full_like(full, float("inf")))
    assert bool(torch.isinf(want).any()) and bool((want > 0).any())
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))


def test_two_calls_return_the_same_bits(generic):
    n, _, _, g, first = generic
    again = G.distances_from(g, torch.arange(n))
    assert torch.equal(first.view(torch.int32), again.view(torch.int32))


def test_errors():
    n, edges, lengths = ref.random_graph()
    g = build(n, edges, lengths)
    for bad in ([0, n], [-1], [], np.zeros(0, dtype=np.int64), [0.5]):
        with pytest.raises(ValueError, match="sources"):
            G.distances_from(g, bad)
    with pytest.raises(ValueError, match="Graph"):
        G.distances_from(np.zeros((4, 4)), [0])
    negative = G.Graph._from_unique_edges(g.edges, -g.distances, n)
    with pytest.raises(ValueError, match="non-negative"):
        G.distances_from(negative, [0])


def test_the_library_refuses_before_it_launches():
    n, edges, lengths = ref.pair()
    g = build(n, edges, lengths)
    lib, plan = _lib.load(), g.plan()
    out = torch.full((n, 1), -7.0, device=plan.device)
    for sources, m in (([n], 1), ([-1], 1), ([0], 0)):
        src = torch.tensor(sources, dtype=torch.int64, device=plan.device)
        rc = lib.mde_graph_distances_from(plan.handle, None, 0.0, m, _lib.ptr(src), _lib.ptr(out),
                                          _lib.stream_ptr(plan.device))
        assert rc == _lib.MDE_E_INVALID and _lib.last_error()
    rc = lib.mde_graph_distances_from(plan.handle, None, 0.0, 1, None, _lib.ptr(out), _lib.stream_ptr(plan.device))
    assert rc == _lib.MDE_E_INVALID
    torch.cuda.synchronize()
    assert bool((out == -7.0).all())

"""The graph kernels of csrc/mde_graph.hip against float64 scipy rows (tests/_graph_reference.py) where the suite had
no check: a graph of n = 16 500 nodes, which ``mde_graph_shortest_paths`` and ``mde_graph_knn`` solve in two batches
of sources (B = 2^28 / n = 16 268, then 232), and small single-batch shapes for the ``max_length`` bound, long
weighted paths, the retained-pair hash, and degenerate graphs.

Edge lengths are multiples of 1/8 in [0.5, 3]: every path sum is exact in float32 and in float64, so every
comparison is ``assert_array_equal``."""
import time

import numpy as np
import pytest
import torch

import _graph_reference as ref

pytestmark = pytest.mark.gpu
DEV = "cuda"

N = 16500                    # > 16 384: two batches of sources
BATCH = (1 << 28) // N       # 16 268 sources in batch 0; its last mask word holds 12 of them
CORE = 16460                 # nodes CORE .. N - 1 are isolated or sit in 3-node components


def _dyadic(rng, size):
    return rng.integers(4, 25, size) / 8.0          # 0.5, 0.625, ..., 3.0


def _unique_edges(e):
    e = np.sort(np.asarray(e, dtype=np.int64), axis=1)
    return np.unique(e[e[:, 0] != e[:, 1]], axis=0)


class Seam:
    """The two-batch graph, its float64 rows from the reference sources, and the device graphs (built once; nothing
    here is modified by a test)."""

    def __init__(self):
        import pymde_amd
        rng = np.random.default_rng(0)
        sparse = rng.integers(0, CORE, (3 * N, 2))
        dense = rng.integers(16200, CORE, (6 * (CORE - 16200), 2))     # plenty of pairs on both sides of the seam
        chains = [[a, a + 1] for a in range(16481, 16499, 3)] + [[a + 1, a + 2] for a in range(16481, 16499, 3)]
        self.edges = _unique_edges(np.concatenate([sparse, dense, np.array(chains)]))
        self.lengths = _dyadic(rng, len(self.edges))
        self.sources = np.unique(np.concatenate([np.arange(32), np.arange(16236, 16300), np.arange(BATCH, N)]))
        assert BATCH == 16268 and (self.sources >= BATCH).sum() == 232 and (self.sources < BATCH).sum() == 64
        self.rows = {False: ref.distance_rows(N, self.edges, None, self.sources),
                     True: ref.distance_rows(N, self.edges, self.lengths, self.sources)}
        assert 6 <= self.rows[False][np.isfinite(self.rows[False])].max() <= 12        # the hop diameter
        assert np.isinf(self.rows[False][-1]).sum() == N - 1                           # node N - 1 is isolated
        assert np.isfinite(self.rows[False][-2]).sum() == 3                            # N - 2 ends a 3-node chain
        e = torch.tensor(self.edges, device=DEV)
        self.graphs = {False: pymde_amd.Graph.from_edges(e, n_items=N),
                       True: pymde_amd.Graph.from_edges(e, torch.tensor(self.lengths, dtype=torch.float32, device=DEV),
                                                        n_items=N)}
        self.connected_pairs = ref.connected_pairs(N, self.edges)


@pytest.fixture(scope="module")
def seam():
    return Seam()


def _timed(fn, *args, **kwargs):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn(*args, **kwargs)
    torch.cuda.synchronize()
    return out, time.perf_counter() - t0


def _rows_of(edges, s):
    lo, hi = np.searchsorted(edges[:, 0], [s, s + 1])
    return slice(lo, hi)


@pytest.mark.parametrize("weighted,max_length", [(False, 2), (True, 1.5)], ids=["unit-2", "weighted-1.5"])
def test_two_batches_shortest_paths_with_max_length(seam, weighted, max_length):
    """For every reference source the output rows with i == s are the reference's pair set and distances.
    Measured on an MI355X: 0.02 s (unit, 380 706 pairs) and 0.14 s (weighted, 33 248 pairs) for the call."""
    from pymde_amd import graph as G
    sp, seconds = _timed(G.shortest_paths, seam.graphs[weighted], max_length=max_length)
    e, d = sp.edges.cpu().numpy(), sp.distances.cpu().numpy()
    print(f"shortest_paths n={N} weighted={weighted} max_length={max_length}: {len(e)} pairs, {seconds:.2f} s")
    for row, s in zip(seam.rows[weighted], seam.sources):
        j, want = ref.pairs_of_source(np.where(row <= max_length, row, np.inf), s)
        sl = _rows_of(e, s)
        np.testing.assert_array_equal(e[sl, 1], j, err_msg=f"source {s}")
        np.testing.assert_array_equal(d[sl], want.astype(np.float32), err_msg=f"source {s}")
    assert (e[:, 0] < e[:, 1]).all() and e.max() < N and (d > 0).all() and (d <= max_length).all()


@pytest.mark.parametrize("weighted", [False, True], ids=["unit", "weighted"])
def test_two_batches_retained_pairs_follow_the_hash(seam, weighted):
    """``retain_fraction=0.02, seed=5`` without a bound: for every reference source the kept rows are the reachable
    targets that the hash replay keeps, with their distances; the total is within 6 sigma of 0.02 x the number of
    connected pairs.  Measured on an MI355X: 0.03 s (unit) and 0.41 s (weighted) for the call, 2 698 067 pairs
    each."""
    from pymde_amd import graph as G
    frac, seed = 0.02, 5
    sp, seconds = _timed(G.shortest_paths, seam.graphs[weighted], retain_fraction=frac, seed=seed)
    e, d = sp.edges.cpu().numpy(), sp.distances.cpu().numpy()
    print(f"shortest_paths n={N} weighted={weighted} retain_fraction={frac}: {len(e)} pairs, {seconds:.2f} s")
    for row, s in zip(seam.rows[weighted], seam.sources):
        j, want = ref.pairs_of_source(row, s)
        keep = ref.retained(N, np.full(len(j), s), j, frac, seed)
        sl = _rows_of(e, s)
        np.testing.assert_array_equal(e[sl, 1], j[keep], err_msg=f"source {s}")
        np.testing.assert_array_equal(d[sl], want[keep].astype(np.float32), err_msg=f"source {s}")
    expected = frac * seam.connected_pairs
    assert abs(len(e) - expected) < 6.0 * np.sqrt(seam.connected_pairs * frac * (1.0 - frac)), (len(e), expected)


@pytest.mark.parametrize("graph_distances", [True, False], ids=["paths", "direct"])
@pytest.mark.parametrize("weighted", [False, True], ids=["unit", "weighted"])
def test_two_batches_neighbor_lists(seam, weighted, graph_distances):
    """``_neighbor_lists(k=6)``: the idx and dist rows of the reference sources equal the reference, -1 /
    3.4028235e38 in the rows of isolated nodes and 3-node components included; in direct mode all n rows are
    compared.  Measured on an MI355X: 0.39 s for the weighted path metric, 0.01 s or less for the other three."""
    from pymde_amd import graph as G
    k = 6
    (idx, dist), seconds = _timed(G._neighbor_lists, seam.graphs[weighted], k, graph_distances=graph_distances)
    idx, dist = idx.cpu().numpy(), dist.cpu().numpy()
    print(f"_neighbor_lists n={N} weighted={weighted} graph_distances={graph_distances}: {seconds:.2f} s")
    assert idx.shape == (N, k) and dist.shape == (N, k)
    if graph_distances:
        want = [ref.top_k(row, s, k) for row, s in zip(seam.rows[weighted], seam.sources)]
        np.testing.assert_array_equal(idx[seam.sources], np.stack([w[0] for w in want]))
        np.testing.assert_array_equal(dist[seam.sources], np.stack([w[1] for w in want]))
    else:
        want_idx, want_dist = ref.direct_lists(N, seam.edges, seam.lengths if weighted else None, k)
        np.testing.assert_array_equal(idx, want_idx)
        np.testing.assert_array_equal(dist, want_dist)
    assert (idx[N - 1] == -1).all() and (dist[N - 1] == ref.FLT_MAX).all()
    assert (idx[N - 2] >= 0).sum() == (2 if graph_distances else 1)


# ---------------------------------------------------------------- small shapes, one batch
def _graph(n, edges, lengths=None):
    import pymde_amd
    w = None if lengths is None else torch.tensor(np.asarray(lengths), dtype=torch.float32, device=DEV)
    return pymde_amd.Graph.from_edges(torch.tensor(np.asarray(edges, dtype=np.int64).reshape(-1, 2), device=DEV), w,
                                      n_items=n)


def _expected_pairs(D, max_length=None, keep=None):
    """All pairs i < j at finite positive distance (<= max_length), in (i, j) order, of a full float64 matrix."""
    iu, ju = np.triu_indices(D.shape[0], 1)
    d = D[iu, ju]
    ok = (d > 0) & np.isfinite(d)
    if max_length is not None:
        ok &= d <= max_length
    if keep is not None:
        ok &= keep(iu, ju)
    return np.stack([iu[ok], ju[ok]], 1), d[ok].astype(np.float32)


def _assert_paths(sp, want):
    np.testing.assert_array_equal(sp.edges.cpu().numpy().reshape(-1, 2), want[0])
    np.testing.assert_array_equal(sp.distances.cpu().numpy(), want[1])


@pytest.fixture(scope="module")
def small():
    """A weighted graph of 300 nodes in several components, its unit twin, and their full float64 matrices."""
    rng = np.random.default_rng(2)
    n = 300
    edges = _unique_edges(rng.integers(0, n - 4, (520, 2)))          # the last four nodes are isolated
    lengths = _dyadic(rng, len(edges))
    every = np.arange(n)
    return {"n": n, "edges": edges, "lengths": lengths,
            "D": {False: ref.distance_rows(n, edges, None, every), True: ref.distance_rows(n, edges, lengths, every)},
            "graph": {False: _graph(n, edges), True: _graph(n, edges, lengths)}}


def test_long_weighted_path_is_exact():
    """A weighted path of 700 nodes: the last pair needs 699 relaxations, far more than a convergence check every
    fourth sweep would excuse, and well within the 4 n + 8 sweeps allowed; all 244 650 pairs are exact."""
    from pymde_amd import graph as G
    rng = np.random.default_rng(4)
    n = 700
    order = rng.permutation(n)                                        # the path does not follow the node order
    lengths = _dyadic(rng, n - 1)
    sp = G.shortest_paths(_graph(n, np.stack([order[:-1], order[1:]], 1), lengths))
    at = np.empty(n)
    at[order] = np.concatenate([[0.0], np.cumsum(lengths)])           # position of every node along the path
    iu, ju = np.triu_indices(n, 1)
    assert len(iu) == 244650
    _assert_paths(sp, (np.stack([iu, ju], 1), np.abs(at[iu] - at[ju]).astype(np.float32)))


def test_max_length_bound_is_inclusive(small):
    from pymde_amd import graph as G
    D = small["D"][True]
    finite = np.unique(D[np.isfinite(D) & (D > 0)])
    bound = float(finite[len(finite) // 3])                           # some pair lies exactly this far apart
    assert bound * 8 == round(bound * 8) and bound - 0.125 > 0
    at, below = _expected_pairs(D, bound), _expected_pairs(D, bound - 0.125)
    assert (at[1] == np.float32(bound)).any() and len(below[0]) < len(at[0])
    _assert_paths(G.shortest_paths(small["graph"][True], max_length=bound), at)
    _assert_paths(G.shortest_paths(small["graph"][True], max_length=bound - 0.125), below)


def test_non_integer_bound_on_a_unit_graph(small):
    from pymde_amd import graph as G
    want = _expected_pairs(small["D"][False], 2.5)
    assert want[1].max() == 2.0
    _assert_paths(G.shortest_paths(small["graph"][False], max_length=2.5), want)
    idx, dist = G._neighbor_lists(small["graph"][False], 5, graph_distances=True, max_distance=2.5)
    cut = np.where(small["D"][False] <= 2.5, small["D"][False], np.inf)
    lists = [ref.top_k(cut[s], s, 5) for s in range(small["n"])]
    np.testing.assert_array_equal(idx.cpu().numpy(), np.stack([w[0] for w in lists]))
    np.testing.assert_array_equal(dist.cpu().numpy(), np.stack([w[1] for w in lists]))


@pytest.mark.parametrize("weighted", [False, True], ids=["unit", "weighted"])
def test_retained_sets_are_nested_and_follow_the_hash(small, weighted):
    from pymde_amd import graph as G
    n, seed = small["n"], 9
    kept = {}
    for frac in (0.1, 0.3, 1.0):
        sp = G.shortest_paths(small["graph"][weighted], retain_fraction=frac, seed=seed)
        _assert_paths(sp, _expected_pairs(small["D"][weighted],
                                          keep=lambda i, j, f=frac: ref.retained(n, i, j, f, seed)))
        e = sp.edges.cpu().numpy()
        kept[frac] = set((e[:, 0] * n + e[:, 1]).tolist())
    assert 0 < len(kept[0.1]) < len(kept[0.3]) < len(kept[1.0])
    assert kept[0.1] < kept[0.3] < kept[1.0]


def test_graph_without_edges():
    from pymde_amd import graph as G
    g = _graph(5, np.zeros((0, 2), dtype=np.int64))
    sp = G.shortest_paths(g)
    assert sp.edges.shape == (0, 2) and sp.distances.shape == (0,)
    for graph_distances in (True, False):
        idx, dist = G._neighbor_lists(g, 3, graph_distances=graph_distances)
        assert (idx.cpu().numpy() == -1).all() and idx.shape == (5, 3)
        assert (dist.cpu().numpy() == ref.FLT_MAX).all()


@pytest.mark.parametrize("length", [None, 0.75])
def test_smallest_graph(length):
    from pymde_amd import graph as G
    g = _graph(2, [[1, 0]], None if length is None else [length])
    sp = G.shortest_paths(g)
    assert sp.edges.cpu().tolist() == [[0, 1]] and sp.distances.cpu().tolist() == [length or 1.0]
    for graph_distances in (True, False):
        idx, dist = G._neighbor_lists(g, 1, graph_distances=graph_distances)
        assert idx.cpu().tolist() == [[1], [0]] and dist.cpu().tolist() == [[length or 1.0]] * 2


@pytest.mark.parametrize("weighted", [False, True], ids=["unit", "weighted"])
def test_star_with_a_hub_of_degree_199(weighted):
    """The hub's CSR row is longer than one wave: direct k-NN of the hub and of the leaves against the reference, and
    the same lists under the path metric (a leaf's nearest targets go through the hub)."""
    from pymde_amd import graph as G
    rng = np.random.default_rng(6)
    n, hub, k = 200, 57, 7
    leaves = np.array([v for v in range(n) if v != hub])
    edges = _unique_edges(np.stack([np.full(n - 1, hub), leaves], 1))
    lengths = _dyadic(rng, len(edges)) if weighted else None
    g = _graph(n, edges, lengths)
    idx, dist = G._neighbor_lists(g, k, graph_distances=False)
    want_idx, want_dist = ref.direct_lists(n, edges, lengths, k)
    assert (want_idx[hub] >= 0).all() and (want_idx[leaves, 0] == hub).all() and (want_idx[leaves, 1:] == -1).all()
    np.testing.assert_array_equal(idx.cpu().numpy(), want_idx)
    np.testing.assert_array_equal(dist.cpu().numpy(), want_dist)
    idx, dist = G._neighbor_lists(g, k, graph_distances=True)
    D = ref.distance_rows(n, edges, lengths, np.arange(n))
    lists = [ref.top_k(D[s], s, k) for s in range(n)]
    np.testing.assert_array_equal(idx.cpu().numpy(), np.stack([w[0] for w in lists]))
    np.testing.assert_array_equal(dist.cpu().numpy(), np.stack([w[1] for w in lists]))

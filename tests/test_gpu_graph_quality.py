"""The graph_* scores of pymde_amd.quality on the GPU: an embedding against the shortest-path lengths of a Graph.

The graphs have edge lengths that are whole multiples of a power of two small enough that every path length is exact
in float32, so ``graph.distances_from`` equals scipy's float64 Dijkstra bit for bit (tests/test_gpu_graph_sssp.py
relies on the same) and the graph-level scores can be compared with the matrix-level ones on scipy's matrix, with
the float64 formulas (bounds: tests/test_gpu_matrix_quality.py) and with scikit-learn."""
import functools

import numpy as np
import pytest
import scipy.sparse
import scipy.sparse.csgraph
import torch

import pymde_amd
from pymde_amd import graph as G
from pymde_amd import quality

import _matrix_quality_reference as ref

pytestmark = pytest.mark.gpu

DEV = "cuda"
RING, PATH = 40, 7
N = RING + PATH


def _dijkstra(n, edges, lengths):
    A = scipy.sparse.coo_matrix((lengths.astype(np.float64), (edges[:, 0], edges[:, 1])), shape=(n, n)).tocsr()
    return scipy.sparse.csgraph.dijkstra(A, directed=False)


def _build(n, edges, lengths):
    return G.Graph.from_edges(torch.as_tensor(edges), torch.as_tensor(lengths.astype(np.float32)), n_items=n)


@functools.lru_cache(maxsize=None)
def _ring_and_path(unit=False):
    """A ring of 40 nodes and a separate path of 7; lengths in multiples of 2^-6 (or all 1: ties everywhere)."""
    rng = np.random.default_rng(0)
    ring = np.stack([np.arange(RING), (np.arange(RING) + 1) % RING], axis=1)
    path = np.stack([RING + np.arange(PATH - 1), RING + np.arange(PATH - 1) + 1], axis=1)
    edges = np.concatenate([ring, path]).astype(np.int64)
    lengths = np.ones(len(edges)) if unit else rng.integers(16, 256, len(edges)) / 64.0
    return edges, lengths, _dijkstra(N, edges, lengths)


def _embedding(d, seed=1):
    return np.random.default_rng(seed).standard_normal((N, d)).astype(np.float32)


def _same_moments(a, b):
    assert a[:8] == b[:8] and (a.count, a.missing) == (b.count, b.missing)
    assert torch.equal(a.row_sums, b.row_sums) and torch.equal(a.row_counts, b.row_counts)


# ---------------------------------------------------------------- 1. the global scores
@pytest.mark.parametrize("d", [1, 2, 8])
def test_graph_scores_equal_the_matrix_scores_on_dijkstras_matrix(d):
    edges, lengths, D = _ring_and_path()
    g, X = _build(N, edges, lengths), _embedding(d)
    assert torch.equal(G.distances_from(g, np.arange(N)).cpu(), torch.as_tensor(D.astype(np.float32)))
    mom = quality.graph_moments(g, X)
    _same_moments(mom, quality.matrix_moments(D, X))
    assert mom.missing == 2 * RING * PATH and mom.count == N * (N - 1) - 2 * RING * PATH and mom.rows is None
    for scale in ("optimal", 1.0, 0.5):
        assert quality.graph_stress(g, X, scale=scale) == quality.matrix_stress(D, X, scale=scale)
    assert quality.graph_correlation(g, X) == quality.matrix_correlation(D, X)
    s, rows = quality.graph_stress(g, torch.as_tensor(X), per_item=True)
    s2, rows2 = quality.matrix_stress(D, X, per_item=True)
    assert s == s2 and torch.equal(rows, rows2) and rows.shape == (N,)
    # ... and the float64 formulas
    w_sums, w_count, _, w_tot = ref.moments(D.astype(np.float32), X)
    tol_e = (d + 4) * 2.0 ** -23
    assert mom.sum_d == w_tot[0] and mom.sum_dd == w_tot[2] and mom.max_d == w_tot[5]      # exact terms
    for got, want in ((mom.sum_e, w_tot[1]), (mom.sum_ee, w_tot[3]), (mom.sum_de, w_tot[4]), (mom.max_e, w_tot[6])):
        assert abs(got - want) <= tol_e * want
    np.testing.assert_allclose(mom.row_sums.cpu().numpy(), w_sums, rtol=tol_e, atol=0.0)
    np.testing.assert_array_equal(mom.row_counts.cpu().numpy(), w_count)
    keep = ref.counted(D.astype(np.float32))
    Dk, Ek = D[keep], ref.embedding_distances(X, np.arange(N))[keep]
    alpha = (Dk * Ek).sum() / (Ek * Ek).sum()
    assert abs(quality.graph_stress(g, X) - np.sqrt(((Dk - alpha * Ek) ** 2).sum() / (Dk * Dk).sum())) <= 1e-6
    assert abs(quality.graph_stress(g, X, scale=1.0) - np.sqrt(((Dk - Ek) ** 2).sum() / (Dk * Dk).sum())) <= 1e-6
    assert abs(quality.graph_correlation(g, X) - np.corrcoef(Dk, Ek)[0, 1]) <= 1e-6


def test_small_batches_give_the_same_bits():
    """Float64 sums regrouped by batch keep their bits only where every partial sum is exact: D in multiples of 2^-6
    and, for E, whole-number coordinates on a line (E, E^2 and D E are then small dyadic numbers).  Counts, maxima and
    histogram counts are the same for any data; the sums that involve a rounded E agree to the rounding of float64."""
    edges, lengths, _ = _ring_and_path()
    g = _build(N, edges, lengths)
    X = np.random.default_rng(2).integers(0, 64, (N, 1)).astype(np.float32)
    one = quality.graph_moments(g, X)
    for batch in (16, 32, 46):
        _same_moments(one, quality.graph_moments(g, X, _batch=batch))
        assert quality.graph_stress(g, X, _batch=batch) == quality.graph_stress(g, X)
    counts = quality.graph_shepard_histogram(g, X, bins=16)
    batched = quality.graph_shepard_histogram(g, X, bins=16, _batch=16)
    assert torch.equal(counts[0], batched[0]) and counts[3] == batched[3] == one.count
    # general data: the same counts, the sums to float64 rounding
    X = _embedding(2)
    one, three = quality.graph_moments(g, X), quality.graph_moments(g, X, _batch=16)
    assert (one.count, one.missing, one.max_d, one.max_e) == (three.count, three.missing, three.max_d, three.max_e)
    assert one.sum_d == three.sum_d and one.sum_dd == three.sum_dd and torch.equal(one.row_counts, three.row_counts)
    np.testing.assert_allclose(np.array(three[1:6]), np.array(one[1:6]), rtol=1e-14, atol=0.0)
    np.testing.assert_allclose(three.row_sums.cpu().numpy(), one.row_sums.cpu().numpy(), rtol=1e-14, atol=0.0)
    t1 = quality.graph_trustworthiness(g, X, 5, per_item=True)
    t3 = quality.graph_trustworthiness(g, X, 5, per_item=True, _batch=16)
    assert t1[0] == t3[0] and torch.equal(t1[1], t3[1])


def test_sample_uses_the_rows_of_sample_rows():
    edges, lengths, D = _ring_and_path()
    g, X = _build(N, edges, lengths), _embedding(2)
    for m, seed in ((10, 0), (33, 5)):
        rows = quality._sample_rows(N, m, seed).numpy()
        mom = quality.graph_moments(g, X, sample=m, seed=seed)
        _same_moments(mom, quality.matrix_moments(D[:, rows], X, items=rows))
        assert mom.count + mom.missing == m * (N - 1)
        assert quality.graph_stress(g, X, sample=m, seed=seed) == quality.matrix_stress(D[:, rows], X, items=rows)
        counts = quality.graph_shepard_histogram(g, X, bins=8, sample=m, seed=seed)
        want = quality.matrix_shepard_histogram(D[:, rows], X, items=rows, bins=8)
        assert torch.equal(counts[0], want[0]) and counts[3] == want[3] == mom.count
        np.testing.assert_array_equal(counts[1], want[1])
    _same_moments(quality.graph_moments(g, X, sample=N), quality.graph_moments(g, X))


# ---------------------------------------------------------------- 2. trustworthiness and continuity
UNIT = 2.0 ** -22


@functools.lru_cache(maxsize=None)
def _plane_graph(seed=13):
    """A connected 200-node 8-NN graph of points in the plane.  Edge lengths: the Euclidean length times a random
    factor, rounded to a multiple of 2^-22; every path length stays below 2^24 of those units, so it is exact in
    float32, and with this seed no row of the float64 matrix holds a tie (both asserted by the test)."""
    rng = np.random.default_rng(seed)
    n, k = 200, 8
    P = rng.uniform(0.0, 1.0, (n, 2))
    E = np.sqrt(((P[:, None, :] - P[None, :, :]) ** 2).sum(-1))
    np.fill_diagonal(E, np.inf)
    nbr = np.argsort(E, axis=1)[:, :k]
    pairs = np.unique(np.sort(np.stack([np.repeat(np.arange(n), k), nbr.ravel()], axis=1), axis=1), axis=0)
    lengths = np.round(E[pairs[:, 0], pairs[:, 1]] * rng.uniform(1.0, 2.0, len(pairs)) / UNIT) * UNIT
    X = (P + 0.05 * rng.standard_normal((n, 2))).astype(np.float32)
    return n, pairs.astype(np.int64), lengths, _dijkstra(n, pairs, lengths), X


def _neighbour_lists(M, k):
    """The first k items of every row of a float64 matrix under (value, index), the row's own item and the
    unreachable ones left out (-1 where fewer than k remain)."""
    n = M.shape[0]
    out = np.full((n, k), -1, dtype=np.int64)
    for i in range(n):
        order = [j for j in np.lexsort((np.arange(n), M[i])) if j != i and np.isfinite(M[i, j])][:k]
        out[i, :len(order)] = order
    return out


@pytest.mark.parametrize("k", [5, 15])
def test_scores_equal_scikit_learn_without_ties(k):
    from sklearn.manifold import trustworthiness
    n, pairs, lengths, D, X = _plane_graph()
    assert np.isfinite(D).all() and D.max() / UNIT < 2 ** 24                  # connected; exact in float32
    assert all(len(np.unique(row)) == n for row in D)                         # no tie within a row
    g = _build(n, pairs, lengths)
    assert torch.equal(G.distances_from(g, np.arange(n)).cpu(), torch.as_tensor(D.astype(np.float32)))
    want = trustworthiness(D, X, n_neighbors=k, metric="precomputed")
    got, rows = quality.graph_trustworthiness(g, X, n_neighbors=k, per_item=True)
    assert abs(got - want) <= 1e-12
    assert rows.shape == (n,) and abs(float(rows.double().mean()) - got) <= 1e-6
    assert abs(quality.matrix_trustworthiness(D, X, n_neighbors=k) - want) <= 1e-12
    # the swapped form: sklearn's formula with the k nearest nodes by path length ranked in the embedding (its
    # function takes coordinates, not a matrix, on the embedding side, so the formula is spelled out here)
    E = ref.embedding_distances(X, np.arange(n))
    assert all(len(np.unique(row)) == n for row in E)
    swapped = ref.sampled_score(ref.ranks(E, _neighbour_lists(D, k)), n, k)
    got, rows = quality.graph_continuity(g, X, n_neighbors=k, per_item=True)
    assert abs(got - swapped) <= 1e-12 and rows.shape == (n,)
    # a sample: the mean over the sampled sources
    m, seed = 37, 2
    src = quality._sample_rows(n, m, seed).numpy()
    lists_x = _neighbour_lists(E, k)
    want = ref.sampled_score(ref.ranks(D[:, src], lists_x[src], src), n, k)
    assert abs(quality.graph_trustworthiness(g, X, k, sample=m, seed=seed) - want) <= 1e-12
    want = ref.sampled_score(ref.ranks(E[:, src], _neighbour_lists(D, k)[src], src), n, k)
    assert abs(quality.graph_continuity(g, X, k, sample=m, seed=seed) - want) <= 1e-12


@pytest.mark.parametrize("k", [3, 8])
def test_scores_with_ties_everywhere_follow_value_then_index(k):
    # hop counts: two nodes at every distance round the ring, and the 7-node path reaches 6 < 8 others
    edges, lengths, D = _ring_and_path(unit=True)
    g, X = _build(N, edges, lengths), _embedding(2, seed=3)
    E = ref.embedding_distances(X, np.arange(N))
    want = ref.sampled_score(ref.ranks(D.astype(np.float32), _neighbour_lists(E, k)), N, k)
    assert abs(quality.graph_trustworthiness(g, X, n_neighbors=k) - want) <= 1e-12
    lists = _neighbour_lists(D, k)
    assert (lists[RING:, 6:] == -1).all() and (lists[:RING] >= 0).all()       # entries of -1 carry no penalty
    want = ref.sampled_score(ref.ranks(E, lists), N, k)
    assert abs(quality.graph_continuity(g, X, n_neighbors=k) - want) <= 1e-12
    assert want < 1.0


# ---------------------------------------------------------------- 3. end to end
def test_an_unrolled_strip_scores_better_against_geodesics():
    # 400 points of a strip rolled one and a half turns; its 10-NN graph with Euclidean edge lengths
    rng = np.random.default_rng(0)
    n, k = 400, 10
    t = 1.5 * np.pi * (1.0 + 2.0 * rng.random(n))
    data = np.stack([t * np.cos(t), 21.0 * rng.random(n), t * np.sin(t)], axis=1).astype(np.float32)
    E = np.sqrt(((data[:, None, :].astype(np.float64) - data[None, :, :]) ** 2).sum(-1))
    np.fill_diagonal(E, np.inf)
    nbr = np.argsort(E, axis=1)[:, :k]
    pairs = np.unique(np.sort(np.stack([np.repeat(np.arange(n), k), nbr.ravel()], axis=1), axis=1), axis=0)
    g = _build(n, pairs, E[pairs[:, 0], pairs[:, 1]])
    Dg = G.distances_from(g, np.arange(n))
    assert bool(torch.isfinite(Dg).all())
    X = pymde_amd.classical_mds(distance_matrix=Dg, embedding_dim=2).X
    against_geodesics = quality.graph_stress(g, X, scale=1.0)
    against_chords = quality.stress(data, X, scale=1.0)
    print("graph_stress %.4f, stress against the chords %.4f" % (against_geodesics, against_chords))
    # measured on an MI355X: 0.1451 against 0.8846
    assert against_geodesics < against_chords
    assert quality.graph_correlation(g, X) > quality.distance_correlation(data, X)

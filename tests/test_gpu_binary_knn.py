"""The exact Jaccard / Hamming self-join on packed rows (mde_bits_knn through preprocess._neighbor_lists) against
tests/_binary_reference.py: indices equal, values bit-equal.  Shapes: one word per row (3, 50 bits), a partial
last word (33, 200, 1025), two staged chunks of 32 words (2048: 64 words; 1025: 33), more query blocks than one
and a last block of 5 rows (4101), exactly k + 1 rows (65 at k = 64), and fewer rows than k + 1 (40 and 2 rows,
where k is clamped to n - 1)."""
import functools

import numpy as np
import pytest
import torch

import _binary_reference as ref
from pymde_amd import affinity, binary, preprocess

pytestmark = pytest.mark.gpu

SHAPES = [(1037, 50, 0.3), (257, 2048, 0.05), (130, 3, 0.5), (300, 33, 0.5), (4101, 200, 0.1), (65, 1025, 0.5)]
KS = [1, 15, 64]
DISTANCES = ["jaccard", "hamming"]


@functools.lru_cache(maxsize=None)
def _data(n, nf, p):
    B = ref.make_bits(n, nf, p)
    return B, binary.pack(B)


@functools.lru_cache(maxsize=None)
def _reference(n, nf, p, distance):
    """The lists at k = 64, computed once per shape and distance; shorter lists are their prefixes."""
    idx, val = ref.knn_lists(_data(n, nf, p)[0], 64, distance)
    idx.setflags(write=False)
    val.setflags(write=False)
    return idx, val


def _lists(bits, k, **kw):
    idx, val, bound, root, scale = preprocess._neighbor_lists(bits, k, **kw)
    assert root is False and scale == 1.0
    assert idx.dtype == torch.int32 and val.dtype == torch.float32
    return idx.cpu().numpy().astype(np.int64), val.cpu().numpy(), bound


@pytest.mark.parametrize("distance", DISTANCES)
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("n,nf,p", SHAPES)
def test_neighbor_lists_equal_the_reference(n, nf, p, k, distance):
    bits = _data(n, nf, p)[1].with_distance(distance)
    want_idx, want_val = _reference(n, nf, p, distance)
    kk = min(k, n - 1)                                     # k above n - 1 is clamped, as for the other searches
    idx, val, bound = _lists(bits, k)
    assert bound is None and idx.shape == (n, kk)
    assert np.array_equal(idx, want_idx[:, :kk])
    assert np.array_equal(val.view(np.uint32), want_val[:, :kk].view(np.uint32))
    again = _lists(bits, k)
    assert np.array_equal(again[0], idx) and np.array_equal(again[1].view(np.uint32), val.view(np.uint32))


@pytest.mark.parametrize("distance", DISTANCES)
@pytest.mark.parametrize("n,nf,k", [(40, 50, 64), (40, 50, 40), (2, 33, 15), (7, 2048, 64)])
def test_k_above_n_minus_1_is_clamped(n, nf, k, distance):
    """Fewer than k other rows: the lists have n - 1 columns, every one filled, as for the other searches."""
    B = ref.make_bits(n, nf, 0.3)
    bits = binary.pack(B, distance)
    want_idx, want_val = ref.knn_lists(B, n - 1, distance)
    assert (want_idx >= 0).all()
    idx, val, bound = _lists(bits, k)
    assert bound is None and idx.shape == (n, n - 1) and val.shape == (n, n - 1)
    assert np.array_equal(idx, want_idx)
    assert np.array_equal(val.view(np.uint32), want_val.view(np.uint32))
    edges, weights = preprocess.k_nearest_neighbors(bits, k)
    assert set(map(tuple, edges.cpu().numpy().tolist())) == {(i, j) for i in range(n) for j in range(i + 1, n)}
    assert (weights == 2.0).all()                          # every pair is listed from both ends
    graph = preprocess.neighbor_graph(bits, k)
    assert graph.edges.shape[0] == n * (n - 1) // 2


def test_a_single_row_has_no_neighbours():
    with pytest.raises(ValueError, match="k must be at least 1"):
        preprocess.k_nearest_neighbors(binary.pack(np.ones((1, 9), bool)), 3)


def test_the_three_feature_shape_is_nearly_all_ties():
    """8 distinct rows among 130: the lists are decided by the index rule."""
    idx, val = _reference(130, 3, 0.5, "jaccard")
    assert (np.diff(val[:, :15], axis=1) == 0).mean() > 0.8


@pytest.mark.parametrize("n,nf,p", SHAPES)
def test_empty_rows_list_each_other_at_zero_under_jaccard(n, nf, p):
    bits = _data(n, nf, p)[1]
    assert int(bits.counts[3]) == 0 and int(bits.counts[5]) == 0
    idx, val, _ = _lists(bits, 15)
    for a, b in ((3, 5), (5, 3)):
        where = list(idx[a]).index(b)
        assert val[a, where] == 0.0
    # an empty row against a non-empty one is at distance 1
    nonempty = bits.counts.cpu().numpy()[idx[3]] > 0
    assert (val[3][nonempty] == 1.0).all()


@pytest.mark.parametrize("distance", DISTANCES)
@pytest.mark.parametrize("n,nf,p", [(1037, 50, 0.3), (130, 3, 0.5), (300, 33, 0.5)])
def test_k_nearest_neighbors_gives_the_edges_of_the_lists(n, nf, p, distance):
    bits = _data(n, nf, p)[1].with_distance(distance)
    want_idx, want_val = _reference(n, nf, p, distance)
    k = 15
    edges, weights = preprocess.k_nearest_neighbors(bits, k)
    got = set(map(tuple, edges.cpu().numpy().tolist()))
    assert got == ref.edge_set(want_idx[:, :k])
    assert set(weights.cpu().numpy().tolist()) <= {1.0, 2.0}
    # max_distance, in the distance's own units, drops exactly the entries above it
    cut = float(np.median(want_val[:, :k]))
    edges, _ = preprocess.k_nearest_neighbors(bits, k, max_distance=cut)
    assert set(map(tuple, edges.cpu().numpy().tolist())) == ref.edge_set(want_idx[:, :k], want_val[:, :k], cut)
    idx, val, bound = _lists(bits, k, max_distance=cut)
    assert bound == cut and np.array_equal(idx, want_idx[:, :k])


def test_neighbor_graph_and_affinities_run_on_the_lists():
    n, nf, p = 300, 33, 0.5
    bits = _data(n, nf, p)[1]
    want_idx, want_val = _reference(n, nf, p, "jaccard")
    graph = preprocess.neighbor_graph(bits, 10)
    assert set(map(tuple, graph.edges.cpu().numpy().tolist())) == ref.edge_set(want_idx[:, :10])
    lengths = {tuple(e): float(v) for e, v in zip(graph.edges.cpu().numpy().tolist(), graph.distances.cpu().numpy())}
    D = ref.cross_distances(_data(n, nf, p)[0], _data(n, nf, p)[0], "jaccard")
    assert all(np.float32(v) == D[i, j] for (i, j), v in lengths.items())
    found = affinity.neighbor_affinities(bits, 10)
    assert set(map(tuple, found.edges.cpu().numpy().tolist())) == ref.edge_set(want_idx[:, :10])
    assert bool(torch.isfinite(found.weights).all())


def test_k_must_be_positive():
    with pytest.raises(ValueError):
        preprocess.k_nearest_neighbors(_data(130, 3, 0.5)[1], 0)

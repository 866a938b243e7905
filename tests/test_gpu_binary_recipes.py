"""The recipes on a BitMatrix: pair distances against tests/_binary_reference.py bit for bit, and the problems
that preserve_neighbors, laplacian_embedding, preserve_distances and extend_embedding build from packed rows."""
import numpy as np
import pytest
import torch

import _binary_reference as ref
import pymde_amd
from pymde_amd import _lib, binary, preprocess, recipes

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("distance", ["jaccard", "hamming"])
def test_distances_over_all_pairs_equal_the_reference(distance):
    B = ref.make_bits(300, 33, 0.5)
    bits = binary.pack(B, distance)
    graph = recipes.distances(bits)
    edges = graph.edges.cpu().numpy()
    assert edges.shape == (300 * 299 // 2, 2) and graph.n_items == 300
    D = ref.cross_distances(B, B, distance)
    want = D[edges[:, 0], edges[:, 1]]
    assert np.array_equal(graph.distances.cpu().numpy().view(np.uint32), want.view(np.uint32))
    sample = recipes.distances(bits, retain_fraction=0.1, seed=0)
    e = sample.edges.cpu().numpy()
    assert 0 < e.shape[0] < edges.shape[0]
    assert np.array_equal(sample.distances.cpu().numpy().view(np.uint32), D[e[:, 0], e[:, 1]].view(np.uint32))


def test_pair_distances_abi_out_of_range_endpoints_are_nan():
    B = ref.make_bits(70, 65, 0.3)
    bits = binary.pack(B, "hamming")
    dev = bits.device
    edges = torch.tensor([[0, 1], [-1, 2], [3, 70], [69, 0], [2 ** 40, 1], [3, 5]], dtype=torch.int64, device=dev)
    out = binary.pair_distances(bits, edges).cpu().numpy()
    D = ref.cross_distances(B, B, "hamming")
    assert np.isnan(out[[1, 2, 4]]).all()
    assert out[0] == D[0, 1] and out[3] == D[69, 0] and out[5] == 0.0
    lib = _lib.load()
    o = torch.empty(6, dtype=torch.float32, device=dev)
    nw = int(bits.words.shape[1])
    for n, w, nf, kind in ((70, nw + 1, 65, 1), (70, nw, 65, 2), (0, nw, 65, 1), (70, nw, 2 ** 24, 1)):
        assert lib.mde_bits_pair_distances(n, w, nf, _lib.ptr(bits.words), _lib.ptr(bits.counts), 6, _lib.ptr(edges),
                                           kind, _lib.ptr(o), _lib.stream_ptr(dev)) == _lib.MDE_E_INVALID


@pytest.fixture(scope="module")
def planted():
    """Three random 256-bit prototypes, 200 rows each, every bit flipped with probability 0.05."""
    rng = np.random.default_rng(7)
    protos = rng.random((3, 256)) < 0.5
    labels = np.repeat(np.arange(3), 200)
    B = protos[labels] ^ (rng.random((600, 256)) < 0.05)
    return B, labels, binary.pack(B)


def _rows(edges):
    return set(map(tuple, edges.cpu().numpy().tolist()))


def _group_means(X, labels):
    X = X.detach().cpu().double()
    D = torch.cdist(X, X).numpy()
    same = labels[:, None] == labels[None, :]
    off = ~np.eye(len(labels), dtype=bool)
    return D[same & off].mean(), D[~same].mean()


@pytest.mark.parametrize("distance", ["jaccard", "hamming"])
def test_preserve_neighbors_separates_planted_groups(planted, distance):
    B, labels, bits = planted
    bits = bits.with_distance(distance)
    mde = recipes.preserve_neighbors(bits, embedding_dim=2, seed=0)
    X = mde.embed(max_iter=100)
    assert bool(torch.isfinite(X).all()) and tuple(X.shape) == (600, 2)
    inside, between = _group_means(X, labels)
    print(f"{distance}: mean embedding distance inside a group {inside:.4f}, between groups {between:.4f}")
    assert inside < between
    # its attractive edges (positive weights) are those of the search
    k = int(max(min(15, (600 * 599 / 2) * 0.01 / 600), 5))
    knn_edges, _ = preprocess.k_nearest_neighbors(bits, k)
    w = mde.distortion_function.weights
    assert _rows(mde.edges[w > 0]) == _rows(knn_edges) and int((w > 0).sum()) == knn_edges.shape[0]
    want_idx, _ = ref.knn_lists(B, k, distance)
    assert set(map(tuple, knn_edges.cpu().numpy().tolist())) == ref.edge_set(want_idx)


def test_laplacian_embedding_and_preserve_distances_embed_to_finite_values(planted):
    _, labels, bits = planted
    X = recipes.laplacian_embedding(bits).embed(max_iter=30)
    assert bool(torch.isfinite(X).all()) and tuple(X.shape) == (600, 2)
    mde = recipes.preserve_distances(bits, max_distances=20000, seed=0)
    assert mde.edges.shape[0] == 20000
    X = mde.embed(max_iter=30)
    assert bool(torch.isfinite(X).all())
    X = recipes.preserve_distances(bits.with_distance("hamming"), constraint=pymde_amd.Standardized(),
                                   max_distances=20000, seed=0).embed(max_iter=30)
    assert bool(torch.isfinite(X).all())
    small = binary.pack(ref.make_bits(60, 40, 0.3))
    X = recipes.preserve_distances(small, ordinal=True).embed(rounds=5)
    assert bool(torch.isfinite(X).all()) and tuple(X.shape) == (60, 2)


def test_extend_embedding_keeps_the_old_rows_and_takes_the_cross_search(planted):
    B, labels, bits = planted
    pick = np.random.default_rng(1).permutation(600)
    old, new = np.sort(pick[:500]), np.sort(pick[500:])
    bits_old, bits_new = binary.pack(B[old]), binary.pack(B[new])
    X = recipes.preserve_neighbors(bits_old, seed=0).embed(max_iter=60)
    mde = recipes.extend_embedding(bits_old, X, bits_new, seed=0)
    k = int(max(min(15, (500 * 499 / 2) * 0.01 / 500), 5))
    idx, _ = preprocess.cross_nearest_neighbors(bits_new, bits_old, k)
    assert int((idx < 0).sum()) == 0
    want = torch.stack([idx.reshape(-1), (500 + torch.arange(100, device=idx.device)).repeat_interleave(k)], 1)
    w = mde.distortion_function.weights
    assert _rows(mde.edges[w > 0]) == _rows(want) and int((w > 0).sum()) == 100 * k
    ref_idx, _ = ref.cross_lists(B[new], B[old], k, "jaccard")
    assert np.array_equal(idx.cpu().numpy(), ref_idx)
    Y = mde.embed(max_iter=60)
    assert tuple(Y.shape) == (600, 2) and bool(torch.isfinite(Y).all())
    assert torch.equal(Y[:500], X.to(Y.device).float())
    # the new rows land nearer to their own group's old rows than to the others'
    Yc, lo, ln = Y.detach().cpu().double(), labels[old], labels[new]
    D = torch.cdist(Yc[500:], Yc[:500]).numpy()
    same = ln[:, None] == lo[None, :]
    assert D[same].mean() < D[~same].mean()
    with pytest.raises(ValueError, match="features"):
        recipes.extend_embedding(bits_old, X, binary.pack(B[new][:, :255]))

"""pymde_amd.binary without a GPU: the names of the binary distances, and every refusal of a BitMatrix that is
raised before a device is required -- a metric of the caller's choice beside it, the searches and problems that
have no form on packed bits, mismatched pairs, malformed packbits input."""
import numpy as np
import pytest
import torch

import pymde_amd
from pymde_amd import binary, classical, landmarks, metrics, preprocess, quality, recipes
from pymde_amd.binary import BitMatrix


def _blank():
    """(building a BitMatrix from data needs a device; these checks come before the words are used)"""
    return object.__new__(BitMatrix)


def _bits(n=40, nf=70, distance="jaccard"):
    """A BitMatrix of zeros whose words live on the CPU: it has a shape, and no search can run on it."""
    return BitMatrix(torch.zeros((n, (nf + 31) // 32), dtype=torch.int32), torch.zeros(n, dtype=torch.int32), nf,
                     distance)


def test_distance_names():
    assert binary.resolve_distance("jaccard") == "jaccard"
    assert binary.resolve_distance(" Tanimoto ") == "jaccard"
    assert binary.resolve_distance("HAMMING") == "hamming"
    assert _bits(distance="tanimoto").distance == "jaccard"
    assert _bits().with_distance("hamming").distance == "hamming"
    assert _bits().with_distance("hamming").words is not None
    for bad in ("dice", "euclidean", "", None, 3):
        with pytest.raises(ValueError, match="binary distance"):
            binary.resolve_distance(bad)
    with pytest.raises(ValueError, match="binary distance"):
        _bits().with_distance("cosine")


def test_the_metric_tables_do_not_know_the_binary_distances():
    assert "jaccard" not in metrics.METRICS and "jaccard" not in metrics.ALIASES and "jaccard" not in metrics.CODES
    with pytest.raises(ValueError, match="binary.pack"):
        metrics.resolve("jaccard")


def test_bitmatrix_shape_and_argument_errors():
    b = _bits(40, 70)
    assert b.shape == (40, 70) and len(b) == 40 and b.device.type == "cpu"
    assert b.with_distance("hamming").words.data_ptr() == b.words.data_ptr()
    assert not preprocess._is_graph(b)
    words, counts = torch.zeros((4, 3), dtype=torch.int32), torch.zeros(4, dtype=torch.int32)
    for nf in (0, 2 ** 24, 64, 97):
        with pytest.raises(ValueError):
            BitMatrix(words, counts, nf)
    with pytest.raises(ValueError):
        BitMatrix(words.to(torch.int64), counts, 70)
    with pytest.raises(ValueError):
        BitMatrix(words, counts[:3], 70)


@pytest.mark.parametrize("metric", ["cosine", "manhattan", "l1"])
def test_a_metric_beside_a_bitmatrix_is_a_value_error(metric):
    b = _bits()
    for call in (lambda: preprocess.k_nearest_neighbors(b, 3, metric=metric),
                 lambda: preprocess._neighbor_lists(b, 3, metric=metric),
                 lambda: preprocess.neighbor_graph(b, 3, metric=metric),
                 lambda: preprocess.cross_nearest_neighbors(b, b, 3, metric=metric),
                 lambda: pymde_amd.affinity.neighbor_affinities(b, 3, metric=metric),
                 lambda: recipes.distances(b, metric=metric),
                 lambda: recipes.preserve_neighbors(b, metric=metric),
                 lambda: recipes.laplacian_embedding(b, metric=metric),
                 lambda: recipes.preserve_distances(b, metric=metric),
                 lambda: recipes.extend_embedding(b, np.zeros((40, 2), np.float32), b, metric=metric)):
        with pytest.raises(ValueError, match="BitMatrix"):
            call()
    with pytest.raises(ValueError):          # an unknown name stays the error it was
        preprocess.k_nearest_neighbors(b, 3, metric="jaccard")


def test_searches_that_have_no_form_on_bits():
    b = _bits()
    for call in (lambda: preprocess.k_nearest_neighbors(b, 3, approximate=True),
                 lambda: preprocess.k_nearest_neighbors(b, 3, precision="bfloat16"),
                 lambda: preprocess.k_nearest_neighbors(b, 3, n_candidates=8),
                 lambda: preprocess.neighbor_graph(b, 3, approximate=True),
                 lambda: preprocess.neighbor_graph(b, 3, connect=True),
                 lambda: preprocess.neighbor_graph(b, 3, connect="tree"),
                 lambda: preprocess.cross_nearest_neighbors(b, b, 3, precision="bf16"),
                 lambda: preprocess.nearest_between_groups(b, np.arange(40) % 2),
                 lambda: preprocess.connect_components(b, None),
                 lambda: preprocess.principal_components(b, 2),
                 lambda: pymde_amd.pca(b, 2),
                 lambda: landmarks.select(b, 5),
                 lambda: classical.classical_mds(b),
                 lambda: recipes.preserve_neighbors(b, approximate_neighbors=True),
                 lambda: recipes.preserve_neighbors(b, approximate_neighbors={"n_lists": 4}),
                 lambda: recipes.preserve_neighbors(b, neighbor_precision="bfloat16"),
                 lambda: recipes.preserve_neighbors(b, n_components=2),
                 lambda: recipes.laplacian_embedding(b, n_components=2),
                 lambda: recipes.preserve_geodesics(b),
                 lambda: recipes.extend_embedding(b, np.zeros((40, 2), np.float32), b, neighbor_precision="bf16")):
        with pytest.raises(ValueError, match="BitMatrix"):
            call()


def test_dense_problems_point_at_distance_matrix():
    b, X = _bits(), np.zeros((40, 2), np.float32)
    for call in (lambda: pymde_amd.DenseMDE(b),
                 lambda: pymde_amd.DensePlacement(b, X, b),
                 lambda: pymde_amd.LandmarkMDE(b, 10),
                 lambda: recipes.preserve_distances(b, dense=True),
                 lambda: recipes.preserve_distances(b, landmarks=10)):
        with pytest.raises(ValueError, match="BitMatrix.*distance_matrix="):
            call()


def test_quality_refuses_bits():
    b, X = _bits(), np.zeros((40, 2), np.float32)
    for call in (lambda: quality.trustworthiness(b, X),
                 lambda: quality.continuity(b, X),
                 lambda: quality.neighbor_overlap(b, X),
                 lambda: quality.neighbor_ranks(b, b, np.zeros((40, 3), np.int64)),
                 lambda: quality.pair_moments(b, X),
                 lambda: quality.stress(b, X),
                 lambda: quality.distance_correlation(b, X),
                 lambda: quality.shepard_histogram(b, X)):
        with pytest.raises(ValueError, match="BitMatrix"):
            call()


def test_refusals_come_before_the_words_are_touched():
    b = _blank()
    with pytest.raises(ValueError, match="BitMatrix"):
        preprocess.k_nearest_neighbors(b, 3, metric="cosine")
    with pytest.raises(ValueError, match="BitMatrix"):
        recipes.preserve_geodesics(b)
    with pytest.raises(ValueError, match="BitMatrix"):
        quality.stress(b, None)
    with pytest.raises(ValueError, match="BitMatrix"):
        pymde_amd.DenseMDE(b)


def test_a_cross_search_needs_two_matching_bitmatrices():
    b, X = _bits(40, 70), np.zeros((40, 2), np.float32)
    dense = np.zeros((8, 70), np.float32)
    for q, c in ((b, _bits(10, 71)), (b, _bits(10, 70, "hamming")), (b, dense), (dense, b)):
        with pytest.raises(ValueError, match="BitMatrix"):
            preprocess.cross_nearest_neighbors(q, c, 3)
    with pytest.raises(ValueError, match="BitMatrix"):
        recipes.extend_embedding(b, X, _bits(10, 71))
    with pytest.raises(ValueError, match="BitMatrix"):
        recipes.extend_embedding(b, X, dense)
    with pytest.raises(ValueError):
        preprocess.cross_nearest_neighbors(b, b, 0)


def test_pack_and_packbits_argument_errors_need_no_device():
    with pytest.raises(ValueError, match="binary distance"):
        binary.pack(np.zeros((4, 8), bool), distance="dice")
    with pytest.raises(ValueError):
        binary.pack(np.zeros(8, bool))
    packed = np.packbits(np.zeros((4, 33), bool), axis=1)              # [4, 5]
    with pytest.raises(ValueError, match=r"\[n, 4\]"):
        binary.from_packbits(packed, 32)
    with pytest.raises(ValueError, match=r"\[n, 6\]"):
        binary.from_packbits(packed, 41)
    with pytest.raises(ValueError, match="uint8"):
        binary.from_packbits(packed.astype(np.int32), 33)
    with pytest.raises(ValueError, match="bitorder"):
        binary.from_packbits(packed, 33, bitorder="msb")
    with pytest.raises(ValueError, match="binary distance"):
        binary.from_packbits(packed, 33, distance="dice")
    with pytest.raises(ValueError):
        binary.from_packbits(packed, 0)

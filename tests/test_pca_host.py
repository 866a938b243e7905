"""Host-side checks of the principal-components feature: the float64 reference against itself, the CSR
transpose on CPU tensors, and the argument errors that need no GPU."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

import pymde_amd
from pymde_amd import preprocess, sparse
from pymde_amd.pca import check_arguments

import _pca_reference as ref


def test_package_level_pca_is_still_the_function():
    assert callable(pymde_amd.pca) and pymde_amd.pca.__name__ == "pca"


# ---------------------------------------------------------------- the reference against itself
def test_reference_replay_meets_the_recorded_figures():
    """The planted data and the float64 replay, against the figures recorded when the generator was written
    (10 oversamples, 4 iterations: sigma within 3e-7, largest principal sine 3.5e-4, variance shortfall 5e-9),
    each within a factor of 3; the spectrum has its gap after the eighth value."""
    A = ref.planted()
    assert A.shape == (600, 900) and A.dtype == np.float32
    assert abs(A.nnz / (600.0 * 900.0) - 0.074) < 0.003
    sigma, V, scores, _, every = ref.exact_pca(A, 8)
    recorded = np.array([289.0, 257.0, 232.0, 207.0, 187.0, 168.0, 142.0, 123.0])
    assert np.all(np.abs(sigma / recorded - 1.0) < 0.03), sigma
    assert 1.7 < every[7] / every[8] < 2.2
    omega = ref.start_block(900, 18)
    s4, V4, scores4, _ = ref.randomized_pca(A, 8, omega, 4)
    sigma_err = np.abs(s4 / sigma - 1.0).max()
    sine = ref.principal_sines(V, V4).max()
    shortfall = 1.0 - (scores4 ** 2).sum() / (sigma ** 2).sum()
    print("replay n_iter=4: sigma %.2e sine %.2e shortfall %.2e" % (sigma_err, sine, shortfall))
    assert sigma_err <= 3 * 3e-7
    assert sine <= 3 * 3.5e-4
    assert 0.0 <= shortfall <= 3 * 5e-9
    s0, V0, _, _ = ref.randomized_pca(A, 8, omega, 0)
    assert ref.principal_sines(V, V0).max() > 0.1           # without iterations the basis is far off


def test_reference_spmm_is_the_dense_product():
    rng = np.random.default_rng(0)
    A = sp.random(7, 9, density=0.4, random_state=1, format="csr", dtype=np.float64)
    B, u, v = rng.standard_normal((9, 3)), rng.standard_normal(7), rng.standard_normal(3)
    want, scale = ref.spmm(A.indptr, A.indices, A.data, B, u, v, with_scale=True)
    assert np.allclose(want, A.toarray() @ B - np.outer(u, v), rtol=0, atol=1e-13)
    assert np.allclose(scale, np.abs(A.toarray()) @ np.abs(B) + np.abs(np.outer(u, v)), rtol=0, atol=1e-13)


# ---------------------------------------------------------------- DeviceCSR.transpose on CPU tensors
def _cpu_csr(matrix):
    indptr, indices, values, shape = sparse.canonical_csr_host(matrix)
    return sparse.DeviceCSR(torch.from_numpy(indptr), torch.from_numpy(indices), torch.from_numpy(values), shape)


def _empty_rows_and_columns():
    A = sp.random(40, 30, density=0.2, random_state=3, format="lil", dtype=np.float32)
    A[[0, 7, 39], :] = 0
    A[:, [0, 11, 29]] = 0
    return A.tocsr()


@pytest.mark.parametrize("matrix", [
    sp.random(50, 70, density=0.1, random_state=2, format="csr", dtype=np.float32),
    _empty_rows_and_columns(),
    sp.random(1, 60, density=0.3, random_state=4, format="csr", dtype=np.float32),
    sp.random(60, 1, density=0.5, random_state=5, format="csr", dtype=np.float32),
    sp.csr_matrix((5, 4), dtype=np.float32),
], ids=["random", "empty-rows-and-columns", "one-row", "one-column", "no-entries"])
def test_transpose_matches_scipy(matrix):
    t = _cpu_csr(matrix).transpose()
    want = matrix.T.tocsr()
    want.sort_indices()
    assert t.shape == want.shape and t.nnz == want.nnz
    assert t.indptr.dtype == torch.int64 and t.indices.dtype == torch.int32 and t.values.dtype == torch.float32
    assert np.array_equal(t.indptr.numpy(), want.indptr)
    assert np.array_equal(t.indices.numpy(), want.indices)
    assert np.array_equal(t.values.numpy(), want.data)


# ---------------------------------------------------------------- argument errors without a device
@pytest.mark.parametrize("m", [0, -1, 30, 31, 100])
def test_n_components_range(m):
    with pytest.raises(ValueError, match="n_components"):
        check_arguments((100, 30), m)
    with pytest.raises(ValueError, match="n_components"):
        preprocess.principal_components(np.zeros((100, 30), dtype=np.float32), m)
    with pytest.raises(ValueError, match="n_components"):
        preprocess.principal_components(sp.random(100, 30, density=0.1, format="csr", dtype=np.float32), m)


def test_accepted_sizes():
    assert check_arguments((100, 30), 29) == (100, 30, 29, 30)           # r is capped at min(n, nf)
    assert check_arguments((1000, 2000), 50, sparse=True) == (1000, 2000, 50, 60)
    assert check_arguments((1000, 2000), 246, sparse=True)[3] == 256
    assert check_arguments((1000, 2000), 300)[3] == 310                   # the dense route has no block


def test_block_wider_than_256_is_refused_for_sparse_data():
    with pytest.raises(ValueError, match="256"):
        check_arguments((1000, 2000), 247, sparse=True)
    with pytest.raises(ValueError, match="256"):
        preprocess.principal_components(sp.random(1000, 2000, density=0.01, format="csr", dtype=np.float32), 200,
                                        n_oversamples=57)


def test_test_matrix_shape_is_checked():
    A = sp.random(100, 30, density=0.1, format="csr", dtype=np.float32)
    with pytest.raises(ValueError, match="test_matrix"):
        preprocess.principal_components(A, 5, test_matrix=np.zeros((30, 14), dtype=np.float32))


@pytest.mark.parametrize("recipe", [pymde_amd.preserve_neighbors, pymde_amd.laplacian_embedding])
@pytest.mark.parametrize("metric", ["cosine", "correlation", "manhattan"])
def test_recipes_refuse_other_metrics(recipe, metric):
    with pytest.raises(ValueError, match="euclidean"):
        recipe(np.zeros((50, 20), dtype=np.float32), n_components=5, metric=metric)


@pytest.mark.parametrize("recipe", [pymde_amd.preserve_neighbors, pymde_amd.laplacian_embedding])
def test_recipes_refuse_a_graph(recipe):
    # (unique sorted edges on CPU tensors: the public constructors put a graph on the GPU)
    graph = pymde_amd.Graph._from_unique_edges(torch.tensor([[0, 1], [1, 2], [2, 3]]), torch.ones(3), 4)
    with pytest.raises(ValueError, match="Graph"):
        recipe(graph, n_components=2)


@pytest.mark.parametrize("recipe", [pymde_amd.preserve_neighbors, pymde_amd.laplacian_embedding])
def test_recipes_check_the_range_before_any_device_work(recipe):
    with pytest.raises(ValueError, match="n_components"):
        recipe(np.zeros((50, 20), dtype=np.float32), n_components=20)

"""Principal components on the GPU (pymde_amd/pca.py): the randomized route on sparse data against its float64
replay and the exact SVD, the exact route on dense data, ``pymde_amd.pca`` on sparse data, and the recipes'
``n_components``.

The sparse fits run on ``_pca_reference.planted()`` (600 x 900, singular values 290 .. 125 | 64: a gap of 1.95 after
the eighth) with ``m = 8``, 10 oversamples (r = 18) and the start block passed as ``test_matrix``, so the replay
sees the same draw.  Replay figures at 4 iterations, against the exact SVD: sigma within 2.2e-7, largest principal
sine 3.1e-4."""
import numpy as np
import pytest
import torch

import pymde_amd
from pymde_amd import preprocess, sparse, util

import _pca_reference as ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
M, R = 8, 18


def EPS(nf):
    return (nf + 2) * 2.0 ** -24      # the Euclidean tolerance of tests/test_gpu_landmarks.py


def _np(t):
    return t.detach().cpu().numpy()


@pytest.fixture(scope="module")
def planted():
    A = ref.planted()
    omega = ref.start_block(A.shape[1], R)
    return {"A": A, "omega": omega, "exact": ref.exact_pca(A, M), "replay": ref.randomized_pca(A, M, omega, 4),
            "fit": preprocess.principal_components(A, M, test_matrix=omega)}


# ---------------------------------------------------------------- consistency, whatever the convergence
def test_fields(planted):
    fit, (n, nf) = planted["fit"], planted["A"].shape
    assert isinstance(fit, preprocess.PrincipalComponents)
    for name, shape, dtype in (("scores", (n, M), torch.float32), ("components", (M, nf), torch.float32),
                               ("mean", (nf,), torch.float32), ("singular_values", (M,), torch.float64),
                               ("explained_variance", (M,), torch.float64), ("total_variance", (), torch.float64)):
        t = getattr(fit, name)
        assert t.is_cuda and tuple(t.shape) == shape and t.dtype == dtype, name
    sigma = _np(fit.singular_values)
    assert np.all(np.diff(sigma) < 0)                                    # descending
    assert np.allclose(_np(fit.explained_variance), sigma ** 2 / (n - 1), rtol=1e-14)
    total = planted["A"].toarray().astype(np.float64).var(axis=0, ddof=1).sum()
    assert abs(float(fit.total_variance) / total - 1.0) < 1e-10
    V = _np(fit.components)
    assert np.all(V[np.arange(M), np.abs(V).argmax(axis=1)] > 0)         # the sign rule


def test_mean_is_the_float64_mean_rounded_once(planted):
    dense = planted["A"].toarray().astype(np.float64)
    err = np.abs(_np(planted["fit"].mean).astype(np.float64) - dense.mean(axis=0))
    bound = 2.0 ** -24 * np.abs(dense).mean(axis=0)
    print("mean: worst error / bound = %.3f" % float((err / np.maximum(bound, 1e-300)).max()))
    assert np.all(err <= bound)


def _reference_scores(fit, A):
    """(A - 1 mean^T) components^T in float64 on the RETURNED float32 components and mean, with its error scale."""
    A = A.tocsr()
    A.sort_indices()
    V, mean = _np(fit.components).astype(np.float64), _np(fit.mean).astype(np.float64)
    return ref.spmm(A.indptr, A.indices, A.data, V.T, None, mean @ V.T, with_scale=True)


def test_scores_are_the_projection_on_the_returned_basis(planted):
    want, scale = _reference_scores(planted["fit"], planted["A"])
    err = np.abs(_np(planted["fit"].scores).astype(np.float64) - want)
    bound = ref.spmm_bound(want, scale)
    print("scores: worst error / bound = %.3f" % float((err / bound).max()))
    assert np.all(err <= bound)


def test_components_are_orthonormal(planted):
    V = _np(planted["fit"].components).astype(np.float64)
    err = np.abs(V @ V.T - np.eye(M)).max()
    print("|V V^T - I|_max = %.2e (bound %.2e)" % (err, 2 * (R + 2) * 2.0 ** -24))
    assert err <= 2 * (R + 2) * 2.0 ** -24


# ---------------------------------------------------------------- against the replay and the exact SVD
def test_against_the_float64_replay(planted):
    """1e-4: float32 accumulation in the Gram products perturbs an entry by at most n 2^-24 = 3.6e-5 at n = 600; one
    power iteration fewer would move sigma by 4e-4 to 2e-2."""
    fit = planted["fit"]
    s_rep, V_rep, scores_rep, _ = planted["replay"]
    sigma = _np(fit.singular_values)
    sigma_err = np.abs(sigma / s_rep - 1.0).max()
    scores_err = np.abs(_np(fit.scores) - scores_rep).max() / np.abs(scores_rep).max()
    print("against the replay: sigma %.2e, scores %.2e of max|score|" % (sigma_err, scores_err))
    assert np.array_equal(np.sign(ref.fix_signs(_np(fit.components))), np.sign(_np(fit.components)))
    assert sigma_err <= 1e-4
    assert scores_err <= 1e-4


def test_against_the_exact_svd(planted):
    """Replay figures: sigma 2.2e-7 and sine 3.1e-4 at four iterations, sine 0.47 at none."""
    s_ex, V_ex = planted["exact"][0], planted["exact"][1]
    fit = planted["fit"]
    sigma_err = np.abs(_np(fit.singular_values) / s_ex - 1.0).max()
    sine = ref.principal_sines(V_ex, _np(fit.components)).max()
    print("against the exact SVD, n_iter=4: sigma %.2e, largest principal sine %.2e" % (sigma_err, sine))
    assert sigma_err <= 1e-5
    assert sine <= 2e-3
    fit0 = preprocess.principal_components(planted["A"], M, test_matrix=planted["omega"], n_iter=0)
    sine0 = ref.principal_sines(V_ex, _np(fit0.components)).max()
    print("against the exact SVD, n_iter=0: largest principal sine %.2e" % sine0)
    assert sine0 > 0.1


def test_seed_gives_the_same_bits_and_another_seed_another_basis(planted):
    A = planted["A"]
    a = preprocess.principal_components(A, M, seed=5)
    b = preprocess.principal_components(A, M, seed=5)
    c = preprocess.principal_components(A, M, seed=6)
    for name in ("scores", "components", "mean", "singular_values"):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    assert not torch.equal(a.scores, c.scores)
    assert np.abs(_np(a.singular_values) / _np(c.singular_values) - 1.0).max() <= 1e-5


def test_transform(planted):
    fit, A = planted["fit"], planted["A"]
    want, scale = _reference_scores(fit, A)
    again = _np(fit.transform(A)).astype(np.float64)
    assert np.all(np.abs(again - want) <= ref.spmm_bound(want, scale))
    top = np.abs(want).max()
    rows = [0, 1, 77, 300, 599]
    sparse_rows = _np(fit.transform(A[rows]))
    for dense_rows in (A[rows].toarray(), torch.as_tensor(A[rows].toarray(), device=DEV)):
        assert np.abs(_np(fit.transform(dense_rows)) - sparse_rows).max() <= 1e-5 * top
    assert np.abs(sparse_rows - want[rows]).max() <= 1e-5 * top
    with pytest.raises(ValueError, match="columns"):
        fit.transform(np.zeros((3, A.shape[1] + 1), dtype=np.float32))
    bad = A[rows].toarray()
    bad[2, 5] = np.nan
    with pytest.raises(ValueError, match="NaN"):
        fit.transform(bad)


def test_non_finite_data_and_rank_loss(planted):
    A = planted["A"].copy()
    A.data[100] = np.inf
    with pytest.raises(ValueError, match="NaN or infinity"):
        preprocess.principal_components(A, M)
    D = np.random.default_rng(0).standard_normal((50, 20)).astype(np.float32)
    D[7, 3] = np.nan
    with pytest.raises(ValueError, match="NaN or infinity"):
        preprocess.principal_components(D, 4)
    import scipy.sparse as sp
    rng = np.random.default_rng(1)
    low = sp.csr_matrix((rng.standard_normal((200, 3)) @ rng.standard_normal((3, 300))).astype(np.float32)
                        * (rng.random((200, 1)) < 0.5))
    with pytest.raises(util.SolverError):
        preprocess.principal_components(low, 5)             # rank 3 + centring < r = 15


# ---------------------------------------------------------------- the dense route
@pytest.fixture(scope="module")
def rank5():
    """500 x 64 of exact rank 5: Z W^T, W orthonormal, built in float64 and cast once.  The rows of Z are distinct
    points of the lattice {-1.5, -0.5, 0.5, 1.5}^5 moved by at most 0.1 per coordinate, so neighbours are at least
    0.8 apart while |x|^2 + |y|^2 is at most 26: the float32 search, which errs relative to |x|^2 + |y|^2, resolves
    every neighbour distance well inside the tolerance used below."""
    rng = np.random.default_rng(7)
    cells = rng.choice(4 ** 5, size=500, replace=False)
    Z = np.stack([(cells // 4 ** j) % 4 for j in range(5)], axis=1) - 1.5 + rng.uniform(-0.1, 0.1, (500, 5))
    W = np.linalg.qr(rng.standard_normal((64, 5)))[0]
    return (Z @ W.T).astype(np.float32)


def test_dense_route(rank5):
    X = rank5
    n = X.shape[0]
    whitened = pymde_amd.pca(torch.as_tensor(X), 5)         # (before any other call: the code it always ran)
    fit = preprocess.principal_components(X, 5)
    s_ex, V_ex, scores_ex, mean_ex, _ = ref.exact_pca(X, 5)
    sigma = _np(fit.singular_values)
    print("dense: sigma error %.2e" % np.abs(sigma / s_ex - 1.0).max())
    assert np.abs(sigma / s_ex - 1.0).max() <= 1e-5
    assert np.abs(_np(fit.mean) - mean_ex).max() <= 2.0 ** -23 * np.abs(X).max()
    assert ref.principal_sines(V_ex, _np(fit.components)).max() <= 1e-5
    assert abs(float(fit.total_variance) / X.astype(np.float64).var(axis=0, ddof=1).sum() - 1.0) <= 1e-5
    want = _np(fit.scores).astype(np.float64) * np.sqrt(float(n)) / sigma
    assert np.abs(_np(whitened) - want).max() <= 1e-5 * np.abs(want).max()
    assert np.abs(_np(fit.transform(X)) - _np(fit.scores)).max() <= 1e-5 * np.abs(scores_ex).max()
    # neighbour distances in the reduced space are those of the full space
    full = preprocess._euclidean_knn_lists(torch.as_tensor(X, device=DEV), 10)[1].sqrt()
    reduced = preprocess._euclidean_knn_lists(fit.scores, 10)[1].sqrt()
    rel = (_np(reduced).astype(np.float64) / _np(full).astype(np.float64) - 1.0)
    print("dense: neighbour distances differ by %.2e relative (bound %.2e)" % (np.abs(rel).max(), 4 * EPS(64)))
    assert np.abs(rel).max() <= 4 * EPS(64)


# ---------------------------------------------------------------- pymde_amd.pca on sparse data
def test_sparse_pca_is_centred_and_white(planted):
    A = planted["A"]
    n = A.shape[0]
    fit = preprocess.principal_components(A, M)
    X = pymde_amd.pca(A, M)
    assert X.is_cuda and X.dtype == torch.float32 and tuple(X.shape) == (n, M)
    Xd = _np(X).astype(np.float64)
    # each entry is rounded to float32 (the scores, then the whitening), and the float32 mean differs from the
    # float64 one by 2^-24 |mean| per column, which moves a whitened column by at most |mean|_2 sqrt(n) / sigma
    mu = _np(fit.mean).astype(np.float64)
    tol = 4 * 2.0 ** -24 * (np.abs(Xd).max() + np.linalg.norm(mu) * np.sqrt(n) / _np(fit.singular_values).min())
    print("sparse pca: |column means| %.2e (bound %.2e), |X^T X / n - I| %.2e"
          % (np.abs(Xd.mean(axis=0)).max(), tol, np.abs(Xd.T @ Xd / n - np.eye(M)).max()))
    assert np.abs(Xd.mean(axis=0)).max() <= tol
    assert np.abs(Xd.T @ Xd / n - np.eye(M)).max() <= 1e-4


# ---------------------------------------------------------------- the recipes
def _weights(mde):
    return mde.distortion_function.weights


@pytest.mark.parametrize("recipe", [pymde_amd.preserve_neighbors, pymde_amd.laplacian_embedding])
def test_recipes_build_the_graph_on_the_scores(planted, recipe):
    A = planted["A"]
    kw = {"seed": 3} if recipe is pymde_amd.preserve_neighbors else {}
    mde = recipe(A, n_components=M, **kw)
    fit = preprocess.principal_components(A, M, seed=kw.get("seed", 0))
    by_hand = recipe(fit.scores, **kw)
    assert torch.equal(mde.edges, by_hand.edges)
    assert torch.equal(_weights(mde), _weights(by_hand))
    assert isinstance(mde.principal_components, preprocess.PrincipalComponents)
    assert torch.equal(mde.principal_components.scores, fit.scores)
    assert not hasattr(by_hand, "principal_components")
    X = mde.embed(max_iter=30)
    assert bool(torch.isfinite(X).all()) and tuple(X.shape) == (A.shape[0], 2)


@pytest.mark.parametrize("recipe", [pymde_amd.preserve_neighbors, pymde_amd.laplacian_embedding])
def test_recipes_without_n_components_are_unchanged(planted, recipe):
    A = planted["A"]
    kw = {"seed": 3} if recipe is pymde_amd.preserve_neighbors else {}
    a, b = recipe(A, n_components=None, **kw), recipe(A, **kw)
    assert torch.equal(a.edges, b.edges) and torch.equal(_weights(a), _weights(b))
    assert not hasattr(a, "principal_components")


def test_recipes_serve_the_other_searches_on_the_scores(planted):
    A = planted["A"]
    exact = pymde_amd.preserve_neighbors(A, n_components=M, seed=3, init="random")
    bf16 = pymde_amd.preserve_neighbors(A, n_components=M, seed=3, init="random", neighbor_precision="bfloat16")
    assert bf16.edges.shape[0] > 0 and abs(bf16.edges.shape[0] / exact.edges.shape[0] - 1.0) < 0.05


def test_recipes_refuse_what_the_reduction_cannot_serve(planted):
    A = planted["A"]
    with pytest.raises(ValueError, match="euclidean"):
        pymde_amd.preserve_neighbors(A, n_components=M, metric="cosine")
    graph = pymde_amd.Graph.from_edges(torch.tensor([[0, 1], [1, 2], [2, 3], [0, 3]]))
    with pytest.raises(ValueError, match="Graph"):
        pymde_amd.preserve_neighbors(graph, n_components=2)
    with pytest.raises(ValueError, match="Graph"):
        pymde_amd.laplacian_embedding(graph, n_components=2)


def test_extend_embedding_in_the_reduced_space(planted):
    """The two documented lines: old and new rows in one coordinate system."""
    A = planted["A"]
    old, new = A[:500], A[500:]
    mde = pymde_amd.preserve_neighbors(old, n_components=M, seed=3, init="random")
    X = mde.embed(max_iter=30)
    pc = mde.principal_components
    ext = pymde_amd.extend_embedding(pc.scores, X, pc.transform(new), seed=3)
    Y = ext.embed(max_iter=20)
    assert tuple(Y.shape) == (600, 2) and bool(torch.isfinite(Y).all()) and torch.equal(Y[:500], X)
    assert sparse.is_sparse(new)

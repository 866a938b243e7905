"""Sparse data matrices on the GPU (csrc/mde_sparse.hip): exact sparse k-NN against the oracle, every
input form, continuous data against float64, the densify dispatcher, pair distances without
cancellation, the recipes on sparse data and the validation of malformed CSR."""
import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla
import torch

from oracle import oracle

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _counts(n, nf, density, seed, empty=3, dups=3):
    """Poisson-like integer counts in [1, 5] (all f32 sums exact), some empty and some duplicated rows."""
    rng = np.random.default_rng(seed)
    A = sp.random(n, nf, density=density, format="lil", random_state=seed, dtype=np.float64,
                  data_rvs=lambda m: np.minimum(rng.poisson(1.5, m) + 1, 5))
    for r in rng.choice(n, size=min(empty, n // 4), replace=False):
        A.rows[r], A.data[r] = [], []
    for _ in range(min(dups, n // 4)):
        a, b = rng.choice(n, 2, replace=False)
        A.rows[b], A.data[b] = list(A.rows[a]), list(A.data[a])
    return A.tocsr()


def _knn(data, k, **kw):
    from pymde_amd import preprocess
    e, w = preprocess.k_nearest_neighbors(data, k, **kw)
    return e.cpu().numpy(), w.cpu().numpy()


def _paths(monkeypatch, path):
    from pymde_amd import preprocess
    monkeypatch.setattr(preprocess, "DENSIFY_DENSITY", {"sparse": 2.0, "dense": 0.0}[path])


SHAPES = [(1000, 2000, 15, 0.02), (3001, 30000, 15, 0.005), (130, 7, 64, 0.4), (65, 100000, 7, 0.001),
          (5000, 50, 10, 0.2)]


@pytest.mark.parametrize("n,nf,k,density", SHAPES)
def test_sparse_knn_bit_exact_on_counts(n, nf, k, density, monkeypatch):
    _paths(monkeypatch, "sparse")      # the sparse kernel itself at every shape
    A = _counts(n, nf, density, seed=n + nf)
    D = A.toarray()
    for md in (None, 3.0):
        e, w = _knn(A, k, max_distance=md)
        we, ww = oracle.knn_graph(D, k, max_distance=md)
        np.testing.assert_array_equal(e, we)
        np.testing.assert_array_equal(w, ww)


def test_every_input_form_gives_the_same_graph():
    A = _counts(700, 900, 0.03, seed=5)
    ref = oracle.knn_graph(A.toarray(), 12)
    coo = A.tocoo()
    dup = sp.coo_matrix((np.concatenate([coo.data - 1.0, np.ones(coo.nnz)]),
                         (np.concatenate([coo.row, coo.row]), np.concatenate([coo.col, coo.col]))), shape=A.shape)
    rev = A.copy()
    for r in range(A.shape[0]):
        lo, hi = rev.indptr[r], rev.indptr[r + 1]
        rev.indices[lo:hi] = rev.indices[lo:hi][::-1].copy()
        rev.data[lo:hi] = rev.data[lo:hi][::-1].copy()
    rev.has_sorted_indices = False
    t = torch.tensor(A.toarray(), dtype=torch.float64)
    forms = [A, A.tocsc(), dup, rev, A.astype(np.float64), A.astype(np.float32),
             t.to_sparse().to(DEV), t.to_sparse_csr().to(DEV), t.float().to_sparse()]
    for m in forms:
        e, w = _knn(m, 12)
        np.testing.assert_array_equal(e, ref[0])
        np.testing.assert_array_equal(w, ref[1])


def test_continuous_data_against_float64():
    from pymde_amd import preprocess, sparse
    rng = np.random.default_rng(3)
    A = sp.random(2000, 500, density=0.03, format="csr", random_state=3, dtype=np.float32,
                  data_rvs=lambda m: rng.standard_normal(m))
    k = 15
    csr = sparse.to_device_csr(A)
    idx, d2 = preprocess._sparse_knn_lists(csr, k)
    idx2, d22 = preprocess._sparse_knn_lists(csr, k)
    assert torch.equal(idx, idx2) and torch.equal(d2, d22)      # bit-identical runs
    idx, d2 = idx.cpu().numpy(), d2.cpu().numpy()
    X = A.toarray().astype(np.float64)
    sq = (X ** 2).sum(1)
    D = sq[:, None] + sq[None, :] - 2.0 * X @ X.T
    np.fill_diagonal(D, np.inf)
    assert (idx >= 0).all() and (idx != np.arange(2000)[:, None]).all()
    np.testing.assert_allclose(d2, np.take_along_axis(D, idx.astype(np.int64), 1), rtol=1e-5, atol=1e-5)
    assert (np.diff(d2, axis=1) >= 0).all()
    truth = np.argsort(D, axis=1, kind="stable")[:, :k]
    for r in range(2000):
        kth = D[r, truth[r, -1]]
        for c in set(idx[r].tolist()) ^ set(truth[r].tolist()):
            assert abs(D[r, c] - kth) <= 1e-5 * kth, (r, c, D[r, c], kth)


@pytest.mark.parametrize("n,nf,k,density", SHAPES[:3] + [(5000, 50, 10, 0.2), (2000, 300, 10, 0.3)])
def test_sparse_equals_dense(n, nf, k, density):
    """Through the dispatcher and through both paths forced."""
    from pymde_amd import preprocess
    A = _counts(n, nf, density, seed=7 * n + nf)
    dense = _knn(torch.tensor(A.toarray(), device=DEV), k)
    for path in ("auto", "sparse", "dense"):
        mp = pytest.MonkeyPatch()
        if path != "auto":
            _paths(mp, path)
        try:
            e, w = _knn(A, k)
        finally:
            mp.undo()
        np.testing.assert_array_equal(e, dense[0])
        np.testing.assert_array_equal(w, dense[1])
    densify = preprocess._densify_sparse_knn(n, nf, A.nnz, torch.device(DEV))
    assert densify == (A.nnz >= preprocess.DENSIFY_DENSITY * n * nf)


def _pair_norms(A, edges):
    A = A.tocsr().astype(np.float64)
    return spla.norm(A[edges[:, 0]] - A[edges[:, 1]], axis=1)


def test_preserve_distances_all_pairs():
    import pymde_amd
    from pymde_amd import recipes
    rng = np.random.default_rng(11)
    A = sp.random(300, 400, density=0.05, format="csr", random_state=11, dtype=np.float32,
                  data_rvs=lambda m: rng.standard_normal(m))
    mde = pymde_amd.preserve_distances(A)
    mdd = pymde_amd.preserve_distances(torch.tensor(A.toarray(), device=DEV))
    np.testing.assert_array_equal(mde.edges.cpu().numpy(), mdd.edges.cpu().numpy())
    g = recipes.distances(A)
    e = g.edges.cpu().numpy()
    assert len(e) == 300 * 299 // 2
    np.testing.assert_allclose(g.distances.cpu().numpy(), _pair_norms(A, e), rtol=1e-6)
    np.testing.assert_allclose(mde.distortion_function.deviations.cpu().numpy(), g.distances.cpu().numpy(),
                               rtol=0, atol=0)
    g2 = recipes.distances(A)
    assert torch.equal(g.distances, g2.distances)                   # reproducible


def test_preserve_distances_sampled_pairs():
    import pymde_amd
    from pymde_amd import recipes
    A = _counts(5000, 20000, 0.01, seed=13).astype(np.float32)
    A.data = A.data * np.float32(0.37)
    g = recipes.distances(A, retain_fraction=300000 / (5000 * 4999 / 2), seed=3)
    e = g.edges.cpu().numpy()
    assert len(e) == 300000
    oracle.check_sampled_edges(5000, e)
    np.testing.assert_allclose(g.distances.cpu().numpy(), _pair_norms(A, e), rtol=1e-6)
    mde = pymde_amd.preserve_distances(A, max_distances=100000, seed=1)
    oracle.check_sampled_edges(5000, mde.edges.cpu().numpy())
    np.testing.assert_allclose(mde.distortion_function.deviations.cpu().numpy(),
                               _pair_norms(A, mde.edges.cpu().numpy()), rtol=1e-6)


def test_near_duplicate_rows_have_small_distances():
    from pymde_amd import recipes
    rng = np.random.default_rng(17)
    n, nf = 200, 5000
    base = sp.random(n // 2, nf, density=0.2, format="csr", random_state=17, dtype=np.float32,
                     data_rvs=lambda m: rng.uniform(0.5, 2.0, m).astype(np.float32))
    twin = base.copy()
    for r in range(n // 2):                    # the twin of row r differs in one entry by 1e-3
        twin.data[twin.indptr[r]] += np.float32(1e-3)
    A = sp.vstack([base, twin]).tocsr()
    g = recipes.distances(A)
    e = g.edges.cpu().numpy()
    d = g.distances.cpu().numpy()
    truth = _pair_norms(A, e)
    twins = e[:, 1] - e[:, 0] == n // 2
    assert twins.sum() == n // 2
    assert (truth[twins] > 0).all()
    np.testing.assert_allclose(d[twins], truth[twins], rtol=1e-3)
    np.testing.assert_allclose(d, truth, rtol=1e-6)


def test_preserve_neighbors_and_laplacian_on_counts():
    import pymde_amd
    A = _counts(1500, 3000, 0.01, seed=19, empty=0)
    D = torch.tensor(A.toarray(), device=DEV)
    for make in (lambda x: pymde_amd.preserve_neighbors(x, seed=0),
                 lambda x: pymde_amd.preserve_neighbors(x, constraint=pymde_amd.Standardized(), n_neighbors=10, seed=0),
                 lambda x: pymde_amd.laplacian_embedding(x)):
        pymde_amd.seed(4)
        ms = make(A)
        pymde_amd.seed(4)
        md = make(D)
        np.testing.assert_array_equal(ms.edges.cpu().numpy(), md.edges.cpu().numpy())
        np.testing.assert_array_equal(ms.distortion_function.weights.cpu().numpy(),
                                      md.distortion_function.weights.cpu().numpy())
        np.testing.assert_array_equal(ms._X_init.cpu().numpy(), md._X_init.cpu().numpy())


def test_preserve_neighbors_on_clustered_sparse_data():
    import pymde_amd
    rng = np.random.default_rng(23)
    n, n_clusters, block = 6000, 6, 400
    labels = rng.integers(0, n_clusters, n)
    rows, cols, vals = [], [], []
    for i in range(n):
        f = labels[i] * block + rng.choice(block, 30, replace=False)      # the cluster's own features
        noise = rng.choice(n_clusters * block, 3, replace=False)          # and a few of anyone's
        c = np.unique(np.concatenate([f, noise]))
        rows.append(np.full(len(c), i))
        cols.append(c)
        vals.append(rng.uniform(0.5, 2.0, len(c)))
    A = sp.csr_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))),
                      shape=(n, n_clusters * block))
    torch.manual_seed(0)
    mde = pymde_amd.preserve_neighbors(A, embedding_dim=2, constraint=pymde_amd.Standardized(), seed=0)
    assert set(np.unique(mde.distortion_function.weights.cpu().numpy()).tolist()) <= {-1.0, 1.0, 2.0}
    X = mde.embed(max_iter=100).cpu().numpy()
    np.testing.assert_allclose(X.T @ X / n, np.eye(2), atol=1e-3)
    cent = np.stack([X[labels == c].mean(0) for c in range(n_clusters)])
    within = np.mean([np.linalg.norm(X[labels == c] - cent[c], axis=1).mean() for c in range(n_clusters)])
    between = np.linalg.norm(cent[:, None] - cent[None], axis=2)[np.triu_indices(n_clusters, 1)].mean()
    assert between > 3 * within, (between, within)


def test_python_validation():
    from pymde_amd import preprocess
    A = _counts(50, 40, 0.1, seed=29)
    with pytest.raises(ValueError):
        preprocess.k_nearest_neighbors(torch.tensor([1.0, 0.0, 2.0]).to_sparse(), 3)
    with pytest.raises(ValueError):
        preprocess.k_nearest_neighbors(sp.csr_matrix((0, 5)), 3)
    with pytest.raises(ValueError):
        preprocess.k_nearest_neighbors(A, 0)


def _c_call(fn, indptr, indices, values, n, nf, *extra):
    from pymde_amd import _lib
    lib = _lib.load()
    ip = torch.tensor(indptr, dtype=torch.int64, device=DEV)
    ix = torch.tensor(indices, dtype=torch.int32, device=DEV)
    vv = torch.tensor(values, dtype=torch.float32, device=DEV)
    nnz = len(values)
    if fn == "knn":
        k = 2
        idx = torch.empty((n, k), dtype=torch.int32, device=DEV)
        d2 = torch.empty((n, k), dtype=torch.float32, device=DEV)
        sqn = torch.empty(n, dtype=torch.float32, device=DEV)
        rc = lib.mde_sparse_knn(n, nf, nnz, _lib.ptr(ip), _lib.ptr(ix), _lib.ptr(vv), k, _lib.ptr(idx),
                                _lib.ptr(d2), _lib.ptr(sqn), _lib.stream_ptr())
    elif fn == "dist":
        edges = torch.tensor([[0, 1], [1, 2]], dtype=torch.int64, device=DEV)
        out = torch.empty(2, dtype=torch.float32, device=DEV)
        rc = lib.mde_sparse_distances(n, nf, nnz, _lib.ptr(ip), _lib.ptr(ix), _lib.ptr(vv), 2, _lib.ptr(edges),
                                      _lib.ptr(out), _lib.stream_ptr())
    else:
        rc = lib.mde_sparse_validate(n, nf, nnz, _lib.ptr(ip), _lib.ptr(ix), _lib.ptr(vv), _lib.stream_ptr())
    torch.cuda.synchronize()
    return rc, (_lib.last_error() if rc != 0 else "")


def test_c_entries_reject_malformed_csr():
    from pymde_amd import _lib
    good = ([0, 2, 3, 5], [0, 3, 1, 0, 2], [1.0, 2.0, 3.0, 4.0, 5.0])
    bad = {
        "column id >= nf": ([0, 2, 3, 5], [0, 4, 1, 0, 2], good[2]),
        "negative column id": ([0, 2, 3, 5], [0, 3, -1, 0, 2], good[2]),
        "indptr decreases": ([0, 3, 2, 5], good[1], good[2]),
        "indptr[0] != 0": ([1, 2, 3, 5], good[1], good[2]),
        "indptr[n] != nnz": ([0, 2, 3, 4], good[1], good[2]),
        "indptr past nnz": ([0, 2, 9, 5], good[1], good[2]),
        "unsorted row": ([0, 2, 3, 5], [3, 0, 1, 0, 2], good[2]),
        "repeated column": ([0, 2, 3, 5], [0, 0, 1, 0, 2], good[2]),
    }
    for fn in ("validate", "knn", "dist"):
        rc, _ = _c_call(fn, *good, 3, 4)
        assert rc == _lib.MDE_OK, fn
        for what, case in bad.items():
            rc, msg = _c_call(fn, *case, 3, 4)
            assert rc == _lib.MDE_E_INVALID, (fn, what)
            assert "malformed CSR" in msg, (fn, what, msg)

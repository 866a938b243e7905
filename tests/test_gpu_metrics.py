"""Cosine, correlation and Manhattan on the original data (csrc/mde_metric.hip, pymde_amd/metrics.py):
neighbour lists against scipy / numpy in float64, ties, pair distances, sparse inputs, degenerate rows,
max_distance in the metric's units, the approximate search under cosine, the recipes, and the default
keyword leaving every result as it was."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch
from scipy.spatial.distance import cdist, pdist

pytestmark = pytest.mark.gpu
DEV = "cuda"
SCIPY = {"cosine": "cosine", "correlation": "correlation", "manhattan": "cityblock"}


def _lists(X, k, metric, **kw):
    """(idx [n, k], distances [n, k] in the metric's units, float64) of the package's search."""
    from pymde_amd import preprocess
    idx, values, _ = preprocess._metric_knn_lists(X, k, metric, **kw)
    dist = values.double() if metric == "manhattan" else 0.5 * values.double()      # d2 = 2 (1 - cos)
    return idx.cpu().numpy().astype(np.int64), dist.cpu().numpy()


def _tolerance(metric, true):
    if metric == "manhattan":
        return 1e-5 * true                  # a sum of non-negative float32 terms
    # |x|^2 + |y|^2 - 2 x.y in f32 on unit rows: rtol on the value plus 2e-6 of the scale (|x|^2 + |y|^2 = 2),
    # halved with d2 / 2
    return 1e-5 * true + 2e-6 * 2.0 / 2.0


def _check_lists(X, idx, dist, metric):
    """Every listed distance is the float64 distance of the listed id; rows ascend; no self entry, no id
    twice; the k-th listed distance is not above the true k-th distance.  Ids are not compared, so ties
    and float32 near-ties need no excluded rows."""
    n, k = idx.shape
    D = cdist(np.asarray(X, dtype=np.float64), np.asarray(X, dtype=np.float64), SCIPY[metric])
    np.fill_diagonal(D, np.inf)
    assert (idx >= 0).all() and (idx < n).all()
    assert not (idx == np.arange(n)[:, None]).any()
    srt = np.sort(idx, axis=1)
    assert not (srt[:, 1:] == srt[:, :-1]).any()
    true = np.take_along_axis(D, idx, 1)
    err = np.abs(dist - true)
    print("%s n=%d nf=%d k=%d: max listed error %.3e" % (metric, n, X.shape[1], k, err.max()))
    assert (err <= _tolerance(metric, true)).all(), float((err - _tolerance(metric, true)).max())
    assert (dist[:, 1:] >= dist[:, :-1]).all()
    kth = np.sort(D, axis=1)[:, k - 1]
    assert (dist[:, -1] <= kth + _tolerance(metric, kth)).all(), float((dist[:, -1] - kth).max())


def _data(n, nf, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((n, nf)) + 0.5).astype(np.float32)


# ---------------------------------------------------------------- 1. neighbour lists against float64
@pytest.mark.parametrize("metric", ["cosine", "correlation", "manhattan"])
@pytest.mark.parametrize("n,nf", [(1037, 50), (1037, 1), (1037, 784), (4101, 50), (130, 3)])
def test_neighbour_lists_against_float64(metric, n, nf):
    X = _data(n, nf, seed=n + nf)
    if metric == "correlation" and nf == 1:
        with pytest.raises(ValueError):      # one feature: every row is constant, the distance is undefined
            _lists(torch.tensor(X, device=DEV), 15, metric)
        return
    for k in (1, 15, 64):
        idx, dist = _lists(torch.tensor(X, device=DEV), k, metric)
        assert idx.shape == (n, k)
        _check_lists(X, idx, dist, metric)


def test_correlation_on_rows_with_a_large_offset():
    """Rows of values 1e3 +- 1: centring happens in double before the float32 copy is rounded."""
    rng = np.random.default_rng(3)
    X = (1000.0 + rng.standard_normal((1037, 50))).astype(np.float32)
    idx, dist = _lists(torch.tensor(X, device=DEV), 15, "correlation")
    _check_lists(X, idx, dist, "correlation")


# ---------------------------------------------------------------- 2. ties
def test_manhattan_ties_on_counts():
    from pymde_amd import preprocess
    rng = np.random.default_rng(5)
    X = rng.integers(0, 4, (3001, 20)).astype(np.float32)
    Xd = torch.tensor(X, device=DEV)
    idx, dist = _lists(Xd, 15, "manhattan")
    _check_lists(X, idx, dist, "manhattan")
    e1, w1 = preprocess.k_nearest_neighbors(Xd, 15, metric="manhattan")
    e2, w2 = preprocess.k_nearest_neighbors(Xd, 15, metric="l1")
    assert torch.equal(e1, e2) and torch.equal(w1, w2)
    assert set(np.unique(w1.cpu().numpy()).tolist()) <= {1.0, 2.0}


# ---------------------------------------------------------------- 3. pair distances
@pytest.mark.parametrize("metric", ["cosine", "correlation", "manhattan"])
def test_pair_distances_against_scipy(metric):
    from pymde_amd import recipes
    X = _data(300, 50, seed=7)
    g = recipes.distances(torch.tensor(X, device=DEV), metric=metric)
    e = g.edges.cpu().numpy()
    assert e.shape[0] == 300 * 299 // 2
    want = pdist(X.astype(np.float64), SCIPY[metric])        # the order of all_edges: i < j, row-major
    np.testing.assert_array_equal(e, np.stack(np.triu_indices(300, 1), 1))
    np.testing.assert_allclose(g.distances.cpu().numpy(), want, rtol=1e-5)
    big = _data(3000, 37, seed=8)
    g = recipes.distances(big, retain_fraction=0.01, seed=1, metric=metric)
    e = g.edges.cpu().numpy()
    assert 0 < e.shape[0] < 3000 * 2999 // 2 and (e[:, 0] < e[:, 1]).all()
    b64 = big.astype(np.float64)
    want = np.array([cdist(b64[i:i + 1], b64[j:j + 1], SCIPY[metric])[0, 0] for i, j in e[:2000]])
    np.testing.assert_allclose(g.distances.cpu().numpy()[:2000], want, rtol=1e-5)


@pytest.mark.parametrize("metric", ["cosine", "correlation"])
def test_near_duplicate_rows_have_small_distances(metric):
    from pymde_amd import recipes
    rng = np.random.default_rng(17)
    n, nf = 200, 500
    base = rng.uniform(0.5, 2.0, (n // 2, nf)).astype(np.float32)
    twin = base.copy()
    twin[:, 0] += np.float32(1e-3)            # the twin of row r differs in one entry by 1e-3
    X = np.concatenate([base, twin])
    g = recipes.distances(torch.tensor(X, device=DEV), metric=metric)
    e = g.edges.cpu().numpy()
    d = g.distances.cpu().numpy()
    X64 = X.astype(np.float64)
    twins = e[:, 1] - e[:, 0] == n // 2
    assert twins.sum() == n // 2
    truth = np.array([cdist(X64[i:i + 1], X64[j:j + 1], metric)[0, 0] for i, j in e[twins]])
    assert (truth > 0).all() and truth.max() < 1e-6
    np.testing.assert_allclose(d[twins], truth, rtol=1e-3)


# ---------------------------------------------------------------- 4. sparse inputs
def _sparse_matrix(n, nf, density, seed):
    rng = np.random.default_rng(seed)
    A = sp.random(n, nf, density=density, format="lil", random_state=seed, dtype=np.float64,
                  data_rvs=lambda m: rng.uniform(0.5, 2.0, m))
    for r in range(n):                                   # no empty row: cosine is undefined there
        if not A.rows[r]:
            A[r, rng.integers(0, nf)] = 1.0
    return A.tocsr().astype(np.float32)


def _knn(data, k, **kw):
    from pymde_amd import preprocess
    e, w = preprocess.k_nearest_neighbors(data, k, **kw)
    return e.cpu().numpy(), w.cpu().numpy()


def test_sparse_cosine_equals_the_dense_copy():
    A = _sparse_matrix(2000, 300, 0.05, seed=11)
    dense = torch.tensor(A.toarray(), device=DEV)
    ed, wd = _knn(dense, 12, metric="cosine")
    coo = A.tocoo()
    t = torch.sparse_coo_tensor(torch.tensor(np.stack([coo.row, coo.col]).astype(np.int64)), torch.tensor(coo.data),
                                A.shape)
    for form in (A, A.tocsc(), t, t.to_sparse_csr()):
        e, w = _knn(form, 12, metric="cosine")
        np.testing.assert_array_equal(e, ed)
        np.testing.assert_array_equal(w, wd)


@pytest.mark.parametrize("metric", ["correlation", "manhattan"])
def test_sparse_correlation_and_manhattan_equal_the_dense_result(metric):
    from pymde_amd import recipes
    A = _sparse_matrix(1500, 200, 0.05, seed=12)
    dense = torch.tensor(A.toarray(), device=DEV)
    e, w = _knn(A, 10, metric=metric)
    ed, wd = _knn(dense, 10, metric=metric)
    np.testing.assert_array_equal(e, ed)
    np.testing.assert_array_equal(w, wd)
    gs = recipes.distances(A[:200], metric=metric)
    gd = recipes.distances(dense[:200], metric=metric)
    assert torch.equal(gs.edges, gd.edges) and torch.equal(gs.distances, gd.distances)


def test_sparse_pair_distances_cosine():
    from pymde_amd import recipes
    A = _sparse_matrix(300, 400, 0.05, seed=13)
    g = recipes.distances(A, metric="cosine")
    want = pdist(A.toarray().astype(np.float64), "cosine")
    # the rows are scaled in float32 before the double sum: 1e-7 of the unit norm, beside the rtol
    np.testing.assert_allclose(g.distances.cpu().numpy(), want, rtol=1e-5, atol=2e-7)


def test_refused_densify(monkeypatch):
    """When the dense copy is not allowed cosine keeps to the sparse kernel; correlation and Manhattan
    say that they cannot."""
    from pymde_amd import preprocess, recipes
    monkeypatch.setattr(preprocess, "_densify_sparse_knn", lambda *a: False)
    A = _sparse_matrix(1037, 120, 0.08, seed=14)
    idx, dist = _lists(A, 15, "cosine")
    _check_lists(A.toarray(), idx, dist, "cosine")
    for metric in ("correlation", "manhattan"):
        with pytest.raises(ValueError, match="does not fit"):
            preprocess.k_nearest_neighbors(A, 5, metric=metric)
        with pytest.raises(ValueError, match="does not fit"):
            recipes.distances(A, metric=metric)
    with pytest.raises(ValueError, match="does not fit"):
        preprocess.k_nearest_neighbors(sp.vstack([A] * 10).tocsr(), 5, metric="cosine", approximate=True)


# ---------------------------------------------------------------- 5. degenerate rows
def test_degenerate_rows_raise_with_the_row_index():
    from pymde_amd import preprocess, recipes
    X = _data(500, 20, seed=15)
    zero = X.copy()
    zero[[7, 300]] = 0.0
    const = X.copy()
    const[[9, 11, 400]] = 2.5
    for data in (torch.tensor(zero, device=DEV), sp.csr_matrix(zero)):
        for call in (lambda d: preprocess.k_nearest_neighbors(d, 5, metric="cosine"),
                     lambda d: recipes.distances(d, metric="cosine")):
            with pytest.raises(ValueError, match=r"2 of the 500 rows.*row 7\b"):
                call(data)
        for call in (lambda d: preprocess.k_nearest_neighbors(d, 5, metric="correlation"),
                     lambda d: recipes.distances(d, metric="correlation")):
            with pytest.raises(ValueError, match=r"2 of the 500 rows.*row 7\b"):
                call(data)                               # an all-zero row is constant as well
    for data in (torch.tensor(const, device=DEV), sp.csr_matrix(const)):
        with pytest.raises(ValueError, match=r"3 of the 500 rows.*row 9\b"):
            preprocess.k_nearest_neighbors(data, 5, metric="correlation")
        with pytest.raises(ValueError, match=r"3 of the 500 rows.*row 9\b"):
            recipes.distances(data, metric="correlation")
        e, w = preprocess.k_nearest_neighbors(data, 5, metric="cosine")      # constant rows have a direction
        assert e.shape[0] > 0
    for bad in (zero, const):
        for data in (torch.tensor(bad, device=DEV), sp.csr_matrix(bad)):
            e, w = preprocess.k_nearest_neighbors(data, 5, metric="manhattan")
            assert e.shape[0] > 0
            g = recipes.distances(data, metric="manhattan")
            assert bool(torch.isfinite(g.distances).all())


# ---------------------------------------------------------------- 6. max_distance in the metric's units
@pytest.mark.parametrize("metric", ["cosine", "correlation", "manhattan"])
def test_max_distance_in_metric_units(metric):
    n, k = 1000, 10
    X = _data(n, 30, seed=16)
    Xd = torch.tensor(X, device=DEV)
    idx, _ = _lists(Xd, k, metric)
    D = cdist(X.astype(np.float64), X.astype(np.float64), SCIPY[metric])
    listed = np.sort(np.take_along_axis(D, idx, 1).ravel())
    mid = listed.shape[0] // 2
    window = listed[mid - 100:mid + 100]
    g = np.argmax(np.diff(window))
    md = 0.5 * (window[g] + window[g + 1])      # in the widest gap near the median: no float32 borderline
    assert window[g + 1] - md > 4 * _tolerance(metric, md), "the gap must clear the float32 error"
    full_e, full_w = _knn(Xd, k, metric=metric)
    e, w = _knn(Xd, k, metric=metric, max_distance=float(md))
    keep = np.take_along_axis(D, idx, 1) <= md                # float64 decides which directions stay
    r, c = np.nonzero(keep)
    lo, hi = np.minimum(r, idx[r, c]), np.maximum(r, idx[r, c])
    want, counts = np.unique(np.stack([lo, hi], 1), axis=0, return_counts=True)
    assert 0 < want.shape[0] < full_e.shape[0]
    np.testing.assert_array_equal(e, want)
    np.testing.assert_array_equal(w, counts.astype(np.float32))
    assert set(map(tuple, e)) <= set(map(tuple, full_e))


# ---------------------------------------------------------------- 7. approximate search under cosine
def _mixture(n, nf, classes=10, seed=0):
    """The generator of tests/test_gpu_ann.py: classes with means ~ N(0, 9 I), each a random 10-12
    dimensional linear patch, plus N(0, 0.25 I) noise."""
    g = torch.Generator(device=DEV)
    g.manual_seed(seed)
    labels = torch.randint(0, classes, (n,), generator=g, device=DEV)
    means = 3.0 * torch.randn(classes, nf, generator=g, device=DEV)
    X = means[labels] + 0.5 * torch.randn(n, nf, generator=g, device=DEV)
    for c in range(classes):
        dim = 10 + c % 3
        basis = torch.randn(dim, nf, generator=g, device=DEV)
        rows = (labels == c).nonzero()[:, 0]
        X[rows] += torch.randn(rows.shape[0], dim, generator=g, device=DEV) @ basis
    return X.contiguous(), labels


@pytest.mark.parametrize("metric", ["cosine", "correlation"])
def test_full_probe_equals_exact(metric):
    g = torch.Generator(device=DEV)
    g.manual_seed(21)
    X = torch.rand(20037, 50, generator=g, device=DEV)
    for k in (1, 15):
        e, w = _knn(X, k, metric=metric)
        ea, wa = _knn(X, k, metric=metric, approximate=True, n_probe=10 ** 6)
        np.testing.assert_array_equal(ea, e)
        np.testing.assert_array_equal(wa, w)


@pytest.mark.parametrize("nf", [64, 784])
def test_cosine_recall_at_defaults_on_mixture(nf):
    """The bound of the Euclidean recall test (0.95 at the defaults) on the unit-normalised rows of its
    mixture.  With every list probed the search is the exact one (test_full_probe_equals_exact), so the
    exact lists clear the bound by construction: recall 1."""
    n, k = 200000, 15
    X, _ = _mixture(n, nf, seed=nf)
    X = (X / X.norm(dim=1, keepdim=True)).contiguous()
    from pymde_amd import preprocess
    truth, _, _ = preprocess._metric_knn_lists(X, k, "cosine")
    idx, _, _ = preprocess._metric_knn_lists(X, k, "cosine", approximate=True)
    recall = float((truth[:, :, None] == idx[:, None, :]).any(2).float().mean())
    print("cosine recall@%d at nf=%d: %.4f" % (k, nf, recall))
    assert recall >= 0.95, recall


# ---------------------------------------------------------------- 8. recipes end to end
def test_preserve_neighbors_cosine():
    """Clusters that differ in direction, not in norm: every row is a class direction (plus a little
    noise) times a scale drawn from the same wide range in every class."""
    import pymde_amd
    from pymde_amd import preprocess
    rng = np.random.default_rng(31)
    n, classes, nf = 6000, 6, 40
    dirs = rng.standard_normal((classes, nf))
    dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    labels = rng.integers(0, classes, n)
    X = (dirs[labels] + 0.03 * rng.standard_normal((n, nf))) * rng.uniform(0.2, 5.0, (n, 1))
    X = torch.tensor(X.astype(np.float32), device=DEV)
    torch.manual_seed(0)
    mde = pymde_amd.preserve_neighbors(X, embedding_dim=2, constraint=pymde_amd.Standardized(), seed=0,
                                       metric="cosine")
    w = mde.distortion_function.weights
    e_cos, w_cos = preprocess.k_nearest_neighbors(X, 15, metric="cosine")
    assert torch.equal(mde.edges[w > 0], e_cos) and torch.equal(w[w > 0], w_cos)
    e_euc, _ = preprocess.k_nearest_neighbors(X, 15)
    both = set(map(tuple, e_cos.cpu().numpy())) & set(map(tuple, e_euc.cpu().numpy()))
    assert len(both) < 0.8 * e_cos.shape[0]                   # Euclidean neighbours are other rows
    Z = mde.embed(max_iter=100).cpu().numpy()
    np.testing.assert_allclose(Z.T @ Z / n, np.eye(2), atol=1e-3)
    lap = pymde_amd.laplacian_embedding(X, metric="cosine")
    assert torch.equal(lap.edges, e_cos)


def test_preserve_distances_manhattan():
    import pymde_amd
    from pymde_amd import preprocess
    X = _data(300, 25, seed=32)
    mde = pymde_amd.preserve_distances(torch.tensor(X, device=DEV), metric="manhattan")
    e = mde.edges.cpu().numpy()
    X64 = X.astype(np.float64)
    want = np.abs(X64[e[:, 0]] - X64[e[:, 1]]).sum(1)
    np.testing.assert_allclose(want, pdist(X64, "cityblock"), rtol=1e-12)      # all pairs, in pdist's order
    dev = mde.distortion_function.deviations
    np.testing.assert_allclose(dev.cpu().numpy(), want, rtol=1e-5)
    std = pymde_amd.preserve_distances(torch.tensor(X, device=DEV), metric="manhattan",
                                       constraint=pymde_amd.Standardized())
    scaled = preprocess.scale(dev, std.constraint.natural_length(300, 2).to(dev.device))
    torch.testing.assert_close(std.distortion_function.deviations, scaled, rtol=1e-6, atol=0)


# ---------------------------------------------------------------- 9. the default is unchanged
def test_default_metric_is_unchanged():
    import pymde_amd
    from pymde_amd import preprocess, recipes
    X, _ = _mixture(15000, 16, seed=13)
    torch.manual_seed(0)
    a = pymde_amd.preserve_neighbors(X, seed=0)
    torch.manual_seed(0)
    b = pymde_amd.preserve_neighbors(X, seed=0, metric="euclidean")
    assert torch.equal(a.edges, b.edges)
    assert torch.equal(a.distortion_function.weights, b.distortion_function.weights)
    assert type(a.constraint) is type(b.constraint) and a.n_items == b.n_items
    for kw in ({}, {"max_distance": 3.0}, {"approximate": True}):
        e1, w1 = preprocess.k_nearest_neighbors(X, 10, **kw)
        e2, w2 = preprocess.k_nearest_neighbors(X, 10, metric="l2", **kw)
        assert torch.equal(e1, e2) and torch.equal(w1, w2)
    g1 = recipes.distances(X[:400])
    g2 = recipes.distances(X[:400], metric="euclidean")
    assert torch.equal(g1.edges, g2.edges) and torch.equal(g1.distances, g2.distances)
    p1 = pymde_amd.preserve_distances(X[:400])
    p2 = pymde_amd.preserve_distances(X[:400], metric="euclidean")
    assert torch.equal(p1.distortion_function.deviations, p2.distortion_function.deviations)

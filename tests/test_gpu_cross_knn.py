"""Query-against-corpus k-NN (``mde_knn_cross``, ``preprocess.cross_nearest_neighbors``): lists against a
float64 brute force under Euclidean, cosine and correlation, independence of the slice count, ties and
exact ids, ``max_distance``, sparse inputs and the refused arguments."""
import ctypes
import functools

import numpy as np
import pytest
import scipy.sparse as sp
import torch
from scipy.spatial.distance import cdist

pytestmark = pytest.mark.gpu
DEV = "cuda"
SHAPES = [(1, 130, 3), (65, 1037, 50), (130, 4101, 1), (70, 1037, 784), (200, 5, 8)]
KS = (1, 15, 64)


@functools.lru_cache(maxsize=None)
def _case(n_q, n_c, nf):
    """(Q, C) float32, read-only: the generator of test_gpu_metrics (standard normal + 0.5)."""
    rng = np.random.default_rng(1000 * n_q + n_c + nf)
    Q = (rng.standard_normal((n_q, nf)) + 0.5).astype(np.float32)
    C = (rng.standard_normal((n_c, nf)) + 0.5).astype(np.float32)
    Q.setflags(write=False)
    C.setflags(write=False)
    return Q, C


@functools.lru_cache(maxsize=None)
def _truth(n_q, n_c, nf, metric):
    """Float64 brute force, computed once per case: (D [n_q, n_c] in the metric's units, D sorted per row,
    the scale |x|^2 + |y|^2 of every pair as the Euclidean kernel sees it)."""
    Q, C = (m.astype(np.float64) for m in _case(n_q, n_c, nf))
    D = cdist(Q, C, metric)
    if metric == "euclidean":
        scale = (Q * Q).sum(1)[:, None] + (C * C).sum(1)[None, :]
    else:
        scale = np.full(D.shape, 2.0)                 # unit rows
    for a in (D, scale):
        a.setflags(write=False)
    Ds = np.sort(D, axis=1)
    Ds.setflags(write=False)
    return D, Ds, scale


def _bounds(metric, true, scale):
    """The interval a listed distance may lie in.  The kernel's arithmetic (|x|^2 + |y|^2 - 2 x.y in f32)
    is held to 1e-5 of d2 plus 2e-6 of |x|^2 + |y|^2 on the squared distance, as in test_gpu_metrics.
    Cosine / correlation report d2 / 2 on unit rows (scale 2): the bound halves.  Euclidean reports
    sqrt(d2): the d2 interval is mapped through the square root, and the float32 square root itself is
    correctly rounded (2^-24 relative)."""
    if metric == "euclidean":
        d2 = true * true
        tol = 1e-5 * d2 + 2e-6 * scale
        ulp = 2.0 ** -24
        return np.sqrt(np.maximum(d2 - tol, 0.0)) * (1 - ulp), np.sqrt(d2 + tol) * (1 + ulp)
    tol = 0.5 * (1e-5 * (2.0 * true) + 2e-6 * scale)
    return true - tol, true + tol


def _check_lists(shape, metric, idx, dist):
    """Every listed distance is the float64 distance of the listed id; rows ascend; no id twice; the k-th
    listed distance is not above the true k-th; empty slots (-1 / inf) exactly where n_c < k.  Ids are not
    compared, so float32 near-ties need no excluded rows."""
    n_q, n_c, nf = shape
    D, Ds, scale = _truth(n_q, n_c, nf, metric)
    k = idx.shape[1]
    assert idx.shape == (n_q, k) and dist.shape == (n_q, k)
    full = min(k, n_c)
    assert (idx[:, full:] == -1).all() and np.isinf(dist[:, full:]).all()
    idx, dist = idx[:, :full], dist[:, :full]
    assert (idx >= 0).all() and (idx < n_c).all() and np.isfinite(dist).all()
    srt = np.sort(idx, axis=1)
    assert not (srt[:, 1:] == srt[:, :-1]).any()
    true = np.take_along_axis(D, idx, 1)
    lo, hi = _bounds(metric, true, np.take_along_axis(scale, idx, 1))
    print("%s %s k=%d: max listed error %.3e" % (metric, shape, k, np.abs(dist - true).max()))
    assert (dist >= lo).all() and (dist <= hi).all(), float(np.abs(dist - true).max())
    assert (dist[:, 1:] >= dist[:, :-1]).all()
    kth = Ds[:, full - 1]
    # the scale of the true k-th pair is not known per row: the largest scale of the row bounds it
    _, kth_hi = _bounds(metric, kth, scale.max(1))
    assert (dist[:, -1] <= kth_hi).all(), float((dist[:, -1] - kth).max())


def _cross(Q, C, k, **kw):
    from pymde_amd import preprocess
    idx, dist = preprocess.cross_nearest_neighbors(Q, C, k, **kw)
    assert idx.dtype == torch.int64 and dist.dtype == torch.float32 and idx.is_cuda and dist.is_cuda
    return idx.cpu().numpy(), dist.double().cpu().numpy()


# ---------------------------------------------------------------- 1. lists against float64 brute force
@pytest.mark.parametrize("metric", ["euclidean", "cosine", "correlation"])
@pytest.mark.parametrize("shape", SHAPES)
def test_lists_against_float64(shape, metric):
    Q, C = _case(*shape)
    Qd, Cd = torch.tensor(Q, device=DEV), torch.tensor(C, device=DEV)
    if metric == "correlation" and shape[2] == 1:
        with pytest.raises(ValueError):      # one feature: every row is constant, the distance is undefined
            _cross(Qd, Cd, 15, metric=metric)
        return
    for k in KS:
        idx, dist = _cross(Qd, Cd, k, metric=metric)
        _check_lists(shape, metric, idx, dist)


# ---------------------------------------------------------------- 2. independence of the slice count
def _direct(Q, C, k, slices):
    """mde_knn_cross itself: (idx int32 [n_q, k], d2 [n_q, k])."""
    from pymde_amd import _lib
    lib = _lib.load()
    n_q, n_c, nf = Q.shape[0], C.shape[0], C.shape[1]
    idx = torch.full((n_q, k), -7, dtype=torch.int32, device=DEV)
    d2 = torch.full((n_q, k), -7.0, dtype=torch.float32, device=DEV)
    nbytes = lib.mde_knn_cross_work_bytes(n_q, n_c, k, slices)
    assert nbytes >= 4 * (n_q + n_c)
    work = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    _lib.check(lib.mde_knn_cross(n_q, n_c, nf, _lib.ptr(Q), _lib.ptr(C), k, slices, _lib.ptr(idx), _lib.ptr(d2),
                                 _lib.ptr(work), _lib.stream_ptr(Q.device)))
    torch.cuda.synchronize()
    return idx, d2


@pytest.mark.parametrize("k", [15, 64])
@pytest.mark.parametrize("shape", [(70, 20000, 50), (65, 130, 50)])   # 7 slices of 130 columns: four are empty
def test_result_does_not_depend_on_the_slice_count(shape, k):
    n_q, n_c, nf = shape
    g = torch.Generator(device=DEV)
    g.manual_seed(n_c)
    Q = torch.randn(n_q, nf, generator=g, device=DEV)
    C = torch.randn(n_c, nf, generator=g, device=DEV)
    idx1, d21 = _direct(Q, C, k, 1)
    assert bool((idx1 >= 0).all()) and bool((idx1 < n_c).all()) and bool((d21 >= 0).all())
    for slices in (2, 7, 0):
        idx, d2 = _direct(Q, C, k, slices)
        assert torch.equal(idx, idx1), slices
        assert torch.equal(d2, d21), slices


# ---------------------------------------------------------------- 3. ties and exact ids
def test_ties_and_exact_ids_on_small_integers():
    """Values 0..3 in 20 features: every product and sum is exact in float32, so the ids must be those of a
    stable argsort of the float64 distances, and a query that is a corpus row lists that row first at 0."""
    rng = np.random.default_rng(5)
    n_c, k = 3001, 15
    C = rng.integers(0, 4, (n_c, 20)).astype(np.float32)
    twins = rng.choice(n_c, 50, replace=False)
    Q = np.concatenate([rng.integers(0, 4, (150, 20)).astype(np.float32), C[twins]])
    assert np.unique(C, axis=0).shape[0] == n_c               # no accidental duplicates: one twin each
    D2 = cdist(Q.astype(np.float64), C.astype(np.float64), "sqeuclidean")
    want = np.argsort(D2, axis=1, kind="stable")[:, :k]
    Qd, Cd = torch.tensor(Q, device=DEV), torch.tensor(C, device=DEV)
    idx, dist = _cross(Qd, Cd, k)
    np.testing.assert_array_equal(idx, want)
    np.testing.assert_array_equal(idx[150:, 0], twins)
    assert (dist[150:, 0] == 0).all()
    # d2 is exact, so the distance is one float32 square root away from the float64 one (1 ulp = 2^-23)
    np.testing.assert_allclose(dist, np.sqrt(np.take_along_axis(D2, want, 1)), rtol=2.0 ** -23, atol=0)
    for slices in (1, 3, 0):                                  # and the kernel's own d2, at every slice count
        i32, d2 = _direct(Qd, Cd, k, slices)
        np.testing.assert_array_equal(i32.cpu().numpy(), want)
        np.testing.assert_array_equal(d2.cpu().numpy(), np.take_along_axis(D2, want, 1))


# ---------------------------------------------------------------- 4. max_distance
@pytest.mark.parametrize("metric", ["euclidean", "cosine"])
def test_max_distance_in_metric_units(metric):
    shape, k = (65, 1037, 50), 15
    Q, C = _case(*shape)
    Qd, Cd = torch.tensor(Q, device=DEV), torch.tensor(C, device=DEV)
    D, _, scale = _truth(*shape, metric)
    idx, dist = _cross(Qd, Cd, k, metric=metric)
    listed = np.take_along_axis(D, idx, 1)
    flat = np.sort(listed.ravel())
    mid = flat.shape[0] // 2
    window = flat[mid - 50:mid + 50]
    g = np.argmax(np.diff(window))
    md = 0.5 * (window[g] + window[g + 1])      # in the widest gap near the median: no float32 borderline
    lo, hi = _bounds(metric, np.array([md]), np.array([scale.max()]))
    assert window[g] < lo[0] and hi[0] < window[g + 1], "the gap must clear the float32 error"
    idx_m, dist_m = _cross(Qd, Cd, k, metric=metric, max_distance=float(md))
    keep = listed <= md                           # float64 decides which slots stay
    assert 0 < keep.sum() < keep.size
    np.testing.assert_array_equal(idx_m, np.where(keep, idx, -1))
    np.testing.assert_array_equal(dist_m, np.where(keep, dist, np.inf))


# ---------------------------------------------------------------- 5. input forms and errors
def test_sparse_pair_equals_the_dense_copy():
    from pymde_amd import preprocess
    A = sp.random(203, 300, density=0.05, format="csr", random_state=3, dtype=np.float64).astype(np.float32)
    B = sp.random(1037, 300, density=0.05, format="csr", random_state=4, dtype=np.float64).astype(np.float32)
    want_i, want_d = preprocess.cross_nearest_neighbors(torch.tensor(A.toarray(), device=DEV),
                                                        torch.tensor(B.toarray(), device=DEV), 12)
    for q, c in ((A, B), (A.tocoo(), B.tocsc()), (A.toarray(), B)):
        idx, dist = preprocess.cross_nearest_neighbors(q, c, 12)
        assert torch.equal(idx, want_i) and torch.equal(dist, want_d)


def test_refused_densify_says_so(monkeypatch):
    from pymde_amd import preprocess
    monkeypatch.setattr(preprocess, "_densify_sparse_knn", lambda *a: False)
    A = sp.random(20, 30, density=0.2, format="csr", random_state=3, dtype=np.float64).astype(np.float32)
    with pytest.raises(ValueError, match="does not fit"):
        preprocess.cross_nearest_neighbors(A, A, 3)


def test_refused_arguments():
    import pymde_amd
    from pymde_amd import preprocess
    Q, C = _case(65, 1037, 50)
    with pytest.raises(ValueError, match="features"):
        preprocess.cross_nearest_neighbors(Q[:, :49], C, 5)
    for name in ("manhattan", "l1", "cityblock"):
        with pytest.raises(ValueError, match="Manhattan"):
            preprocess.cross_nearest_neighbors(Q, C, 5, metric=name)
    with pytest.raises(ValueError):
        preprocess.cross_nearest_neighbors(Q, C, 5, metric="chebyshev")
    graph = pymde_amd.Graph.from_edges(torch.tensor([[0, 1], [1, 2]]), torch.tensor([1.0, 2.0]))
    with pytest.raises(ValueError, match="Graph"):
        preprocess.cross_nearest_neighbors(Q, graph, 5)
    with pytest.raises(ValueError, match="Graph"):
        preprocess.cross_nearest_neighbors(graph, C, 5)
    with pytest.raises(ValueError):
        preprocess.cross_nearest_neighbors(Q, C, 0)

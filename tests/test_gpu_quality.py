"""mde_knn_ranks, mde_knn_list_overlap and pymde_amd.quality on the GPU.

The brute force below is numpy float64 on integer-grid inputs, for which every squared distance is an exact
integer in float32 and in float64 alike, ties included: every rank comparison is array_equal.  The sharpest
check needs no reference at all: the ranks of a search's own lists are 0 .. k - 1 in every row."""
import numpy as np
import pytest
import torch

from conftest import load_golden

pytestmark = pytest.mark.gpu
DEV = "cuda"
FLT_MAX = np.float32(3.402823466e+38)


# ---------------------------------------------------------------- helpers
def _dev(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(DEV).contiguous()


def _knn(X, k):
    from pymde_amd import _lib
    n, nf = X.shape
    idx = torch.empty((n, k), dtype=torch.int32, device=DEV)
    d2 = torch.empty((n, k), dtype=torch.float32, device=DEV)
    work = torch.empty(n, dtype=torch.float32, device=DEV)
    _lib.check(_lib.load().mde_knn(n, nf, _lib.ptr(X), k, _lib.ptr(idx), _lib.ptr(d2), _lib.ptr(work),
                                   _lib.stream_ptr()))
    return idx, d2


def _ranks(Q, C, idx, self_join, slices=0, want_d2=True):
    """The raw C entry: (ranks int32 [n_q, m], d2 float32 [n_q, m]) as numpy arrays."""
    from pymde_amd import _lib
    lib = _lib.load()
    n_q, n_c, nf, m = Q.shape[0], C.shape[0], C.shape[1], idx.shape[1]
    ranks = torch.full((n_q, m), -7, dtype=torch.int32, device=DEV)
    d2 = torch.full((n_q, m), -7.0, dtype=torch.float32, device=DEV) if want_d2 else None
    nbytes = int(lib.mde_knn_ranks_work_bytes(n_q, n_c, m, slices))
    assert nbytes > 0
    work = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    _lib.check(lib.mde_knn_ranks(n_q, n_c, nf, _lib.ptr(Q), _lib.ptr(C), int(self_join), m, _lib.ptr(idx), slices,
                                 _lib.ptr(ranks), _lib.ptr(d2), _lib.ptr(work), _lib.stream_ptr()))
    torch.cuda.synchronize()
    return ranks.cpu().numpy(), (d2.cpu().numpy() if want_d2 else None)


def _brute_ranks(Q, C, idx, self_join):
    """rank(i, j) = #{l : (d2(i, l), l) < (d2(i, j), j)}, l != i in a self-join; -1 for an entry that is
    negative or, in a self-join, the row itself.  float64, exact for integer inputs."""
    Q, C = np.asarray(Q, dtype=np.float64), np.asarray(C, dtype=np.float64)
    n_q, n_c = Q.shape[0], C.shape[0]
    d2 = ((Q[:, None, :] - C[None, :, :]) ** 2).sum(-1)
    out = np.full(idx.shape, -1, dtype=np.int32)
    for i in range(n_q):
        row = d2[i].copy()
        if self_join:
            row[i] = np.inf                                   # ranked last: precedes nothing
        pos = np.empty(n_c, dtype=np.int64)
        pos[np.lexsort((np.arange(n_c), row))] = np.arange(n_c)
        for c, j in enumerate(idx[i]):
            if j >= 0 and not (self_join and j == i):
                out[i, c] = pos[j]
    return out


# ---------------------------------------------------------------- 1. own lists
@pytest.mark.parametrize("k", [1, 7, 15, 64])
@pytest.mark.parametrize("n,nf", [(150, 8), (333, 37), (333, 2), (200, 70)])
def test_own_lists_rank_in_order(n, nf, k):
    X = _dev(np.random.default_rng(n + nf).standard_normal((n, nf)).astype(np.float32))
    idx, d2 = _knn(X, k)
    ranks, t = _ranks(X, X, idx, True)
    assert np.array_equal(ranks, np.tile(np.arange(k, dtype=np.int32), (n, 1)))
    assert np.array_equal(t.view(np.uint32), d2.cpu().numpy().view(np.uint32))


def test_own_lists_rank_in_order_with_duplicate_rows():
    rng = np.random.default_rng(5)
    X = rng.integers(0, 3, (200, 4)).astype(np.float32)       # 81 distinct rows among 200: ties everywhere
    X = _dev(X)
    idx, d2 = _knn(X, 15)
    ranks, t = _ranks(X, X, idx, True)
    assert np.array_equal(ranks, np.tile(np.arange(15, dtype=np.int32), (200, 1)))
    assert np.array_equal(t.view(np.uint32), d2.cpu().numpy().view(np.uint32))


@pytest.mark.parametrize("metric", ["euclidean", "cosine"])
def test_own_lists_through_the_python_doors(metric):
    from pymde_amd import preprocess, quality
    rng = np.random.default_rng(11)
    n, nf, k = 333, 37, 15
    data = (rng.standard_normal((n, nf)) + (1000.0 if metric == "euclidean" else 0.5)).astype(np.float32)
    data = _dev(data)
    if metric == "euclidean":
        from pymde_amd import metrics
        assert metrics.translated_rows(data)[1] is not None    # the translation path is taken
        idx, _ = preprocess._euclidean_knn_lists(data, k)
    else:
        idx, _, _ = preprocess._metric_knn_lists(data, k, metric)
    ranks = quality.neighbor_ranks(None, data, idx, self_join=True, metric=metric)
    assert ranks.dtype == torch.int32 and ranks.is_cuda
    assert np.array_equal(ranks.cpu().numpy(), np.tile(np.arange(k, dtype=np.int32), (n, 1)))
    # and the cross search's own lists
    queries = data[:70] + 0.25
    cidx, _ = preprocess.cross_nearest_neighbors(queries, data, k, metric=metric)
    cranks = quality.neighbor_ranks(queries, data, cidx, metric=metric)
    assert np.array_equal(cranks.cpu().numpy(), np.tile(np.arange(k, dtype=np.int32), (70, 1)))


# ---------------------------------------------------------------- 2., 3. ties and cross, against the brute force
def _ties_case():
    rng = np.random.default_rng(2)
    X = rng.integers(0, 4, (200, 5)).astype(np.float32)
    for dst, src in ((63, 3), (64, 63), (65, 130), (127, 64), (128, 127)):   # exact duplicates across the 64 / 128 row boundaries
        X[dst] = X[src]
    m = 10
    idx = rng.integers(0, 200, (200, m)).astype(np.int32)
    idx[rng.random((200, m)) < 0.1] = -1
    own = rng.random((200, m)) < 0.05
    idx[own] = np.broadcast_to(np.arange(200, dtype=np.int32)[:, None], (200, m))[own]
    assert (idx == -1).any() and own.any()
    return X, idx


def _cross_case():
    rng = np.random.default_rng(3)
    C = rng.integers(0, 6, (333, 7)).astype(np.float32)
    Q = rng.integers(0, 6, (70, 7)).astype(np.float32)
    Q[5] = C[200]                                            # a query identical to a corpus row
    idx = rng.integers(0, 333, (70, 12)).astype(np.int32)
    idx[5, 0] = int(np.flatnonzero((C == C[200]).all(1))[0])  # the first of the rows equal to it
    return Q, C, idx


@pytest.fixture(scope="module")
def ties():
    X, idx = _ties_case()
    return X, idx, _brute_ranks(X, X, idx, True)


@pytest.fixture(scope="module")
def cross():
    Q, C, idx = _cross_case()
    return Q, C, idx, _brute_ranks(Q, C, idx, False)


def test_ties_match_the_brute_force(ties):
    X, idx, want = ties
    Xd = _dev(X)
    ranks, d2 = _ranks(Xd, Xd, _dev(idx), True)
    assert np.array_equal(ranks, want)
    skipped = (idx < 0) | (idx == np.arange(200)[:, None])
    assert (ranks[skipped] == -1).all() and (ranks[~skipped] >= 0).all()
    assert (d2[skipped] == FLT_MAX).all()
    exact = ((X[:, None, :].astype(np.float64) - X[np.clip(idx, 0, None)]) ** 2).sum(-1)
    assert np.array_equal(d2[~skipped].astype(np.float64), exact[~skipped])
    # self = 0 on the same matrix: the row itself counts and may be listed
    ranks0, _ = _ranks(Xd, Xd, _dev(idx), False)
    assert np.array_equal(ranks0, _brute_ranks(X, X, idx, False))


def test_cross_matches_the_brute_force(cross):
    Q, C, idx, want = cross
    ranks, _ = _ranks(_dev(Q), _dev(C), _dev(idx), False, want_d2=False)
    assert np.array_equal(ranks, want)
    assert ranks[5, 0] == 0                                    # distance 0, the smallest index among its equals


def test_entries_past_the_corpus_are_not_ranked(cross):
    Q, C, idx, want = cross
    bad = idx.copy()
    bad[0, 0], bad[69, 11] = 333, 2 ** 31 - 1
    ranks, d2 = _ranks(_dev(Q), _dev(C), _dev(bad), False)
    want = want.copy()
    want[0, 0] = want[69, 11] = -1
    assert np.array_equal(ranks, want)
    assert d2[0, 0] == FLT_MAX and d2[69, 11] == FLT_MAX


# ---------------------------------------------------------------- 4. slices
@pytest.mark.parametrize("slices", [1, 2, 5, 9, 0])
def test_slices_do_not_change_the_ranks(ties, cross, slices):
    X, idx, want = ties
    Xd = _dev(X)
    assert np.array_equal(_ranks(Xd, Xd, _dev(idx), True, slices)[0], want)
    Q, C, cidx, cwant = cross                                  # 6 column tiles: slices = 9 leaves empty slices
    first = _ranks(_dev(Q), _dev(C), _dev(cidx), False, slices)[0]
    assert np.array_equal(first, cwant)
    assert np.array_equal(_ranks(_dev(Q), _dev(C), _dev(cidx), False, slices)[0], first)   # and run to run


# ---------------------------------------------------------------- 5. scores
@pytest.fixture(scope="module")
def golden():
    return load_golden("quality")


def test_scores_match_sklearn(golden):
    from pymde_amd import quality
    data, X, k = golden["data"].astype(np.float32), golden["X"].astype(np.float32), int(golden["n_neighbors"])
    t = quality.trustworthiness(data, X, n_neighbors=k)
    c = quality.continuity(data, _dev(X), n_neighbors=k)
    assert isinstance(t, float) and isinstance(c, float)
    assert abs(t - float(golden["trustworthiness"])) <= 1e-12
    assert abs(c - float(golden["continuity"])) <= 1e-12
    assert abs(t - 0.49688934566632414) <= 1e-12 and abs(c - 0.5083453237410072) <= 1e-12
    for score, want in ((quality.trustworthiness, t), (quality.continuity, c)):
        s, rows = score(_dev(data), _dev(X), n_neighbors=k, per_item=True)
        assert s == want
        assert rows.shape == (150,) and rows.dtype == torch.float32 and rows.is_cuda
        assert abs(float(rows.double().mean()) - s) <= 1e-6     # float32 rows


def test_an_embedding_equal_to_the_data_scores_one(golden):
    from pymde_amd import quality
    X = golden["X"].astype(np.float32)                          # nf = 2 integer grid, n = 150
    assert quality.trustworthiness(X, X, n_neighbors=7) == 1.0
    assert quality.continuity(X, X, n_neighbors=7) == 1.0
    assert quality.neighbor_overlap(X, X, n_neighbors=15) == 1.0
    score, rows = quality.neighbor_overlap(X, X, n_neighbors=15, per_item=True, precision="bfloat16")
    assert rows.shape == (150,) and rows.dtype == torch.float32
    assert abs(float(rows.double().mean()) - score) <= 1e-6 and 0.0 < score <= 1.0


def test_neighbor_overlap_against_numpy(golden):
    from pymde_amd import quality
    data, X, k = golden["data"].astype(np.float32), golden["X"].astype(np.float32), 15

    def knn(A):
        d2 = ((A[:, None, :].astype(np.float64) - A[None]) ** 2).sum(-1)
        np.fill_diagonal(d2, np.inf)
        return np.argsort(d2, axis=1, kind="stable")[:, :k]
    a, b = knn(data), knn(X)
    want = np.array([len(set(a[i]) & set(b[i])) for i in range(150)])
    score, rows = quality.neighbor_overlap(data, X, n_neighbors=k, per_item=True)
    assert score == want.sum() / (150 * float(k))
    assert np.array_equal(rows.cpu().numpy(), (want / float(k)).astype(np.float32))


# ---------------------------------------------------------------- 6. the overlap kernel
def test_list_overlap_kernel():
    from pymde_amd import _lib
    rng = np.random.default_rng(7)
    n, ka, kb = 333, 15, 23
    a = rng.integers(0, 60, (n, ka)).astype(np.int32)
    b = rng.integers(0, 60, (n, kb)).astype(np.int32)
    a[rng.random((n, ka)) < 0.2] = -1
    b[rng.random((n, kb)) < 0.2] = -1
    want = np.array([sum(1 for v in a[i] if v >= 0 and v in set(b[i])) for i in range(n)], dtype=np.int32)
    distinct = np.array([len(set(a[i][a[i] >= 0]) & set(b[i])) for i in range(n)])
    assert (want >= distinct).all()
    for (x, y, w) in ((a, b, want), (np.sort(a, 1)[:, ::-1].copy(), b, want)):
        count = torch.full((n,), -7, dtype=torch.int32, device=DEV)
        xd, yd = _dev(x), _dev(y)
        _lib.check(_lib.load().mde_knn_list_overlap(n, ka, _lib.ptr(xd), kb, _lib.ptr(yd), _lib.ptr(count),
                                                    _lib.stream_ptr()))
        assert np.array_equal(count.cpu().numpy(), w)


# ---------------------------------------------------------------- 7. argument errors
def test_argument_errors_launch_nothing():
    from pymde_amd import _lib, quality
    lib = _lib.load()
    n, nf, m = 100, 5, 4
    X = _dev(np.random.default_rng(0).standard_normal((n, nf)).astype(np.float32))
    other = _dev(np.zeros((n, nf), dtype=np.float32))
    idx = _dev(np.zeros((n, 65), dtype=np.int32))
    ranks = torch.full((n, 65), -7, dtype=torch.int32, device=DEV)
    work = torch.empty(1 << 20, dtype=torch.uint8, device=DEV)
    p, st = _lib.ptr, _lib.stream_ptr()

    def call(n_q=n, n_c=n, nf_=nf, Q=X, C=X, self_=1, m_=m, idx_=idx, slices=1, out=ranks, work_=work):
        return lib.mde_knn_ranks(n_q, n_c, nf_, p(Q), p(C), self_, m_, p(idx_), slices, p(out), None, p(work_), st)
    assert call() == _lib.MDE_OK
    torch.cuda.synchronize()
    ranks.fill_(-7)
    bad = [call(m_=0), call(m_=65), call(slices=65536), call(slices=-1), call(Q=None), call(C=None), call(idx_=None),
           call(out=None), call(work_=None), call(nf_=0), call(n_q=0), call(n_c=0),
           call(C=other), call(n_q=n - 1)]                    # self needs Q == C and n_q == n_c
    assert bad == [_lib.MDE_E_INVALID] * len(bad)
    assert "mde_knn_ranks" in _lib.last_error()
    for args in ((n, n, 0, 1), (n, n, 65, 1), (n, n, m, 65536), (0, n, m, 1), (n, 0, m, 1)):
        assert lib.mde_knn_ranks_work_bytes(*args) == _lib.MDE_E_INVALID
    a = _dev(np.zeros((n, 4), dtype=np.int32))
    count = torch.full((n,), -7, dtype=torch.int32, device=DEV)
    bad = [lib.mde_knn_list_overlap(n, 0, p(a), 4, p(a), p(count), st),
           lib.mde_knn_list_overlap(n, 4, p(a), 65, p(a), p(count), st),
           lib.mde_knn_list_overlap(n, 4, None, 4, p(a), p(count), st),
           lib.mde_knn_list_overlap(n, 4, p(a), 4, p(a), None, st),
           lib.mde_knn_list_overlap(0, 4, p(a), 4, p(a), p(count), st)]
    assert bad == [_lib.MDE_E_INVALID] * len(bad)
    torch.cuda.synchronize()
    assert (ranks == -7).all() and (count == -7).all()          # nothing was launched
    # the Python doors
    with pytest.raises(ValueError, match="1 to 64"):
        quality.neighbor_ranks(None, X, torch.zeros((n, 0), dtype=torch.int32, device=DEV), self_join=True)
    with pytest.raises(ValueError, match="1 to 64"):
        quality.neighbor_ranks(None, X, idx, self_join=True)
    with pytest.raises(ValueError, match="slices"):
        quality.neighbor_ranks(None, X, idx[:, :4], self_join=True, slices=65536)
    with pytest.raises(ValueError, match="features"):
        quality.neighbor_ranks(X[:, :4], X, idx[:, :4])
    with pytest.raises(ValueError, match="n_samples / 2"):
        quality.trustworthiness(X, X[:, :2], n_neighbors=50)
    with pytest.raises(ValueError, match="Graph|'euclidean', 'cosine' and 'correlation'"):
        quality.continuity(X, X[:, :2], metric="manhattan")

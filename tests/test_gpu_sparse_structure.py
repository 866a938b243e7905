"""The sparse k-NN kernel (csrc/mde_sparse.hip) on rows with 64 or more stored entries inside
one feature window, and the sparse pair distances on the same rows.

``k_sparse_knn`` walks a row 64 entries at a time inside a window of ``W`` columns, once when it scatters the
query rows into its panel and once per candidate; with 64 or more entries in a window both loops go round again.
The matrices of ``_sparse_reference.structured_rows`` put exactly 63, 64, 65, 127, 128 and 129 entries, full
windows, dense rows and entries at the window seams into the windows of the ``W`` that the library reports
(``sparse.knn_window``), at feature counts around the multiples of ``W``.  Their values are small integers, so
every float32 sum is exact: ``idx`` and ``d2`` must equal the float64 lists bit for bit, ties to the smaller
index.  Every case first asserts from the matrix itself that it holds a row with at least 65 and a row with
exactly 64 entries in one window of that ``W``.

Accuracy (``test_accuracy_on_non_negative_rows``): values uniform in [0.5, 2), rows of 5, 70 and 300 entries with
more than 64 of the 300 in one window, twins 1e-3 apart; every listed d2 within ``1e-5 * true + 2e-6 * (|x|^2 +
|y|^2)`` of float64, the constants of tests/test_gpu_euclidean_accuracy.py on the untranslated scale.  A float32
emulation of the arithmetic stays below 0.15 of that bound (tests/test_sparse_reference_host.py).  Largest
``err / (|x|^2 + |y|^2)`` of a listed d2 seen on an MI355X, by the length of the query row, at k = 15 and 64:
1.4e-7 (5 entries), 2.7e-7 (70), 6.3e-7 (300, 0.32 of the 2e-6); at k = 1, where every listed entry is a twin,
1.3e-7, 2.7e-7 and 4.7e-7.  The largest ``err / bound`` of any listed entry is 0.24, on a twin pair.  Sparse
cosine on the same matrix: largest listed error 5.0e-7 against its 2e-6.
"""
import functools

import numpy as np
import pytest
import torch

import _sparse_reference as ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
RTOL, STOL = 1e-5, 2e-6
KS = (1, 15, 41, 48, 64)
NS = (129, 257)
BIG_NF = 2 ** 20                # a feature count that narrows no window


def _window(k, nf=BIG_NF):
    from pymde_amd import sparse
    return sparse.knn_window(k, nf)


def _feature_counts(k):
    W = _window(k)
    return (W - 1, W, W + 1, 2 * W, 2 * W + 1, 4 * W + 3)


def _lists(A, k):
    """(idx int64 [n, k], d2 float64 [n, k]) of the sparse kernel, checked to be the same bits on a second run."""
    from pymde_amd import preprocess, sparse
    csr = sparse.to_device_csr(A)
    idx, d2 = preprocess._sparse_knn_lists(csr, k)
    idx2, d22 = preprocess._sparse_knn_lists(csr, k)
    assert torch.equal(idx, idx2) and torch.equal(d2, d22)
    return idx.cpu().numpy().astype(np.int64), d2.cpu().numpy().astype(np.float64)


def _assert_long_rows(A, W):
    """The input takes the second 64-entry step: a row with at least 65 and a row with exactly 64 entries in
    one window of the width the library uses."""
    counts = ref.window_counts(A, W)
    assert counts.max() >= 65 and (counts == 64).any(), (W, int(counts.max()))
    return counts


def _assert_exact(A, k, what):
    idx, d2 = _lists(A, k)
    want_idx, want_d2 = ref.knn_lists(A, k)
    bad = np.flatnonzero((idx != want_idx).any(1) | (d2 != want_d2).any(1))
    assert bad.size == 0, "%s: %d rows differ from float64, first row %d: idx %s d2 %s, want %s %s" % (
        what, bad.size, bad[0], idx[bad[0]], d2[bad[0]], want_idx[bad[0]], want_d2[bad[0]])


# ---------------------------------------------------------------- a. window and batch structure, bit for bit
@pytest.mark.parametrize("case", range(6))
@pytest.mark.parametrize("k", KS)
def test_window_and_batch_structure(k, case):
    nf = _feature_counts(k)[case]
    W = _window(k, nf)
    assert nf <= 5 * W + 1
    for n in NS + ((2, 127, 128) if k == 15 else ()):
        A, pattern, _ = ref.structured_rows(n, nf, W, seed=1000 * k + n + nf)
        _assert_long_rows(A, W)
        _assert_exact(A, k, "k=%d W=%d nf=%d n=%d" % (k, W, nf, n))


# ---------------------------------------------------------------- b. long rows as candidates only, as queries only
@pytest.mark.parametrize("long_first", [True, False])
def test_long_rows_in_a_block_of_their_own(long_first):
    """A workgroup owns 128 query rows and walks the candidates 128 at a time.  With the rows that have 64 or
    more entries in a window in one block of 128 and the shorter ones in the other, the panel scatter (queries)
    and the cursor walk (candidates) each meet the long rows with short partners on the other side."""
    k = 15
    W = _window(k)
    nf = 2 * W + 1
    assert _window(k, nf) == W
    A, pattern, _ = ref.structured_rows(520, nf, W, seed=77)    # enough rows for 128 of either kind
    most = ref.window_counts(A, W).max(1)
    long_rows, short_rows = np.flatnonzero(most >= 64)[:128], np.flatnonzero(most < 64)[:128]
    assert len(long_rows) == 128 and len(short_rows) == 128
    assert len(set(pattern[long_rows])) >= 10 and len(set(pattern[short_rows])) >= 4
    B = A[np.concatenate([long_rows, short_rows] if long_first else [short_rows, long_rows])]
    assert B.shape == (256, nf)
    most = _assert_long_rows(B, W).max(1)
    block, other = (most[:128], most[128:]) if long_first else (most[128:], most[:128])
    assert block.min() >= 64 and other.max() < 64               # every long row is in the one block
    _assert_exact(B, k, "long rows %s" % ("first" if long_first else "last"))


# ---------------------------------------------------------------- c. accuracy on non-negative continuous data
@functools.lru_cache(maxsize=None)
def _accuracy_input():
    A, length = ref.accuracy_rows(256, 3 * _window(15) + 1, seed=7)
    return A, length


def test_accuracy_on_non_negative_rows():
    A, length = _accuracy_input()
    n = A.shape[0]
    assert sorted(set(length.tolist())) == [5, 70, 300]
    for k in (1, 15, 64):
        W = _window(k, A.shape[1])
        assert ref.window_counts(A, W)[length == 300].max(1).min() > 64
        idx, d2 = _lists(A, k)
        ratio = ref.check_lists("sparse, non-negative rows of 5 / 70 / 300 entries (W=%d)" % W, idx, d2, A, RTOL, STOL)
        for m in (5, 70, 300):
            print("    query rows of %3d entries, k=%d: max listed err / scale %.3e" % (m, k, ratio[length == m].max()))
        want = (np.arange(n) + n // 2) % n                      # each row's first neighbour is its twin
        assert (idx[:, 0] == want).all()


# ---------------------------------------------------------------- d. sparse cosine
def test_sparse_cosine_on_long_rows(monkeypatch):
    """``mde_sparse_rows_normalize`` feeding rows of more than 64 entries per window into the kernel."""
    import test_gpu_metrics as metric_tests
    from pymde_amd import preprocess
    monkeypatch.setattr(preprocess, "_densify_sparse_knn", lambda *a: False)
    A, length = _accuracy_input()
    k = 15
    assert ref.window_counts(A, _window(k, A.shape[1])).max() > 64
    idx, dist = metric_tests._lists(A, k, "cosine")
    metric_tests._check_lists(A.toarray(), idx, dist, "cosine")
    e, w = preprocess.k_nearest_neighbors(A, k, metric="cosine")
    rows = np.repeat(np.arange(A.shape[0]), k)
    pairs = np.stack([np.minimum(rows, idx.ravel()), np.maximum(rows, idx.ravel())], 1)
    want, counts = np.unique(pairs, axis=0, return_counts=True)
    np.testing.assert_array_equal(e.cpu().numpy(), want)
    np.testing.assert_array_equal(w.cpu().numpy(), counts.astype(np.float32))


# ---------------------------------------------------------------- e. pair distances
def _c_distances(A, edges):
    """``mde_sparse_distances`` through the C entry: no Python door between the edge list and the kernel."""
    from pymde_amd import _lib, sparse
    csr = sparse.to_device_csr(A)
    ed = torch.tensor(np.asarray(edges, dtype=np.int64), device=DEV).contiguous()
    out = torch.full((ed.shape[0],), -7.0, dtype=torch.float32, device=DEV)
    _lib.check(_lib.load().mde_sparse_distances(csr.n, csr.n_features, csr.nnz, _lib.ptr(csr.indptr),
                                                _lib.ptr(csr.indices), _lib.ptr(csr.values), ed.shape[0],
                                                _lib.ptr(ed), _lib.ptr(out), _lib.stream_ptr()))
    torch.cuda.synchronize()
    return out.cpu().numpy()


def test_pair_distances_on_structured_rows():
    n = 40
    W = _window(15)
    nf = 2 * W + 1
    A, pattern, partner = ref.structured_rows(n, nf, W, seed=5)
    _assert_long_rows(A, W)
    iu = np.triu_indices(n, 1)
    edges = np.concatenate([np.stack(iu, 1), np.stack(iu[::-1], 1), np.stack([np.arange(n)] * 2, 1)])
    d = _c_distances(A, edges)
    np.testing.assert_allclose(d, ref.pair_distances(A, edges), rtol=1e-6)
    assert (d[-n:] == 0).all()                                  # (i, i)
    at = {(i, j): q for q, (i, j) in enumerate(edges.tolist())}
    copies = np.flatnonzero(pattern == "copy")
    assert copies.size > 0
    for r in copies:
        assert d[at[(r, partner[r])]] == 0 and d[at[(partner[r], r)]] == 0
    sq = np.asarray(A.multiply(A).sum(1), dtype=np.float64).ravel()
    pairs = [r for r in np.flatnonzero(pattern == "disjoint_a") if partner[r] >= 0]
    assert pairs
    for r in pairs:
        assert d[at[(r, partner[r])]] == np.float32(np.sqrt(sq[r] + sq[partner[r]]))
    # an endpoint outside [0, n): NaN for that edge alone
    bad = edges[:200].copy()
    where = {3: (n, 0), 50: (0, n), 51: (-1, 5), 120: (7, -1), 199: (n, n), 0: (-1, -1)}
    for q, (i, j) in where.items():
        bad[q] = (i, j)
    d_bad = _c_distances(A, bad)
    mask = np.zeros(200, dtype=bool)
    mask[list(where)] = True
    assert np.isnan(d_bad[mask]).all()
    np.testing.assert_array_equal(d_bad[~mask], d[:200][~mask])


# ---------------------------------------------------------------- f. short lists through the C entry
def test_fewer_rows_than_k_through_the_c_entry():
    """The Python door clamps k to n - 1; the C entry fills the slots that no row is left for with -1 / FLT_MAX."""
    from pymde_amd import preprocess, sparse
    n, k = 3, 5
    W = _window(k)
    assert _window(k, W + 1) == W
    A, _, _ = ref.structured_rows(n, W + 1, W, seed=9)         # rows of 65, 64 and no entries
    assert np.diff(A.indptr).tolist() == [65, 64, 0]
    idx, d2 = preprocess._sparse_knn_lists(sparse.to_device_csr(A), k)
    idx, d2 = idx.cpu().numpy(), d2.cpu().numpy()
    want_idx, want_d2 = ref.knn_lists(A, k)
    assert (want_idx[:, 2:] == -1).all() and (want_idx[:, :2] >= 0).all()
    np.testing.assert_array_equal(idx, want_idx)
    np.testing.assert_array_equal(d2.astype(np.float64), want_d2)
    assert (d2[:, 2:] == np.finfo(np.float32).max).all()

"""The inputs and references of tests/_sparse_reference.py, checked without a GPU: the structured matrices
contain what the GPU tests rely on at every window width and feature count those tests use, the neighbour
lists agree with scipy (ties included), and the accuracy input stays inside its bound by float32 arithmetic
alone.  The window widths are plain numbers here; the GPU tests take theirs from the library."""
import functools

import numpy as np
import pytest
from scipy.spatial.distance import cdist

import _sparse_reference as ref

WINDOWS = (72, 128, 152, 192, 224)           # what the GPU tests meet at k = 41, 15, 1, 64, 48; any width must do


def feature_counts(W):
    return (W - 1, W, W + 1, 2 * W, 2 * W + 1, 4 * W + 3)


def _most(W, nf):
    """The largest per-window count a matrix must reach: 129, or what one window can hold."""
    return min(129, W, nf)


@pytest.mark.parametrize("W", WINDOWS)
def test_structured_rows_hold_every_pattern(W):
    for nf in feature_counts(W):
        for n in (129, 257) + ((2, 127, 128) if W == 128 else ()):
            A, pattern, partner = ref.structured_rows(n, nf, W, seed=n + nf)
            assert A.shape == (n, nf) and A.dtype == np.float32
            assert A.has_canonical_format and set(np.unique(A.data)) <= {1.0, 2.0, 3.0, 4.0, 5.0}
            counts = ref.window_counts(A, W)
            assert counts.shape == (n, ref.n_windows(nf, W)) and (counts.sum(1) == np.diff(A.indptr)).all()
            assert set(pattern) == set(ref.PATTERNS[:n])                        # each pattern occurs
            assert (counts == 64).any() and counts.max() >= 65
            if n >= len(ref.PATTERNS):
                assert counts.max() >= _most(W, nf), (W, nf, n, counts.max())
            length = np.diff(A.indptr)
            for name, m in ref._IN_ONE_WINDOW.items():                          # all inside one window
                rows = np.flatnonzero(pattern == name)
                assert ((counts[rows] > 0).sum(1) == 1).all()
                assert (length[rows] == min(m, W, nf)).all()                    # capped at the window's width
            assert (length[pattern == "empty"] == 0).all() and (length[pattern == "one"] == 1).all()
            assert (length[pattern == "dense"] == nf).all()
            last = counts[pattern == "last_window"]
            assert (last[:, -1] == nf - (ref.n_windows(nf, W) - 1) * W).all() and (last[:, :-1] == 0).all()
            if nf > W:
                step = counts[pattern == "in64_then_1"]
                assert ((step == 64).sum(1) == 1).all() and ((step == 1).sum(1) == 1).all()
                w = np.argmax(step == 64, axis=1)
                assert (step[np.arange(len(w)), w + 1] == 1).all()              # the single entry is in the next window
                seams = A[np.flatnonzero(pattern == "seams")]
                assert (np.diff(seams.indptr) == 3).all()
                c = seams.indices.reshape(-1, 3)
                assert (c[:, 0] % W == 0).all() and (c[:, 1] == c[:, 0] + W - 1).all() and (c[:, 2] == c[:, 0] + W).all()
            if nf >= 2 * W:
                assert ((counts[pattern == "two_full_windows"] == W).sum(1) == 2).all()
            if nf >= W:
                assert ((counts[pattern == "full_window"] == W).sum(1) == 1).all()
            X = A.toarray()
            for r in np.flatnonzero(pattern == "copy"):
                assert pattern[partner[r]] == "long" and abs(partner[r] - r) >= len(ref.PATTERNS)
                assert (X[r] == X[partner[r]]).all() and length[r] > nf // 2
            for r in np.flatnonzero(pattern == "disjoint_a"):
                if partner[r] >= 0:
                    assert pattern[partner[r]] == "disjoint_b" and partner[partner[r]] == r
                    assert not (X[r] * X[partner[r]]).any() and length[r] + length[partner[r]] == nf
            assert (partner[~np.isin(pattern, ("copy", "disjoint_a", "disjoint_b"))] == -1).all()
            again, _, _ = ref.structured_rows(n, nf, W, seed=n + nf)
            assert (again != A).nnz == 0


@pytest.mark.parametrize("k", [1, 15, 41, 48, 64])
def test_structured_rows_at_the_windows_the_library_reports(k):
    """The same two facts at the window the built library reports (a host call: nothing is launched)."""
    from pymde_amd import sparse
    W = sparse.knn_window(k, 2 ** 20)
    assert W > 0 and W % 8 == 0
    for nf in feature_counts(W):
        Wn = sparse.knn_window(k, nf)
        counts = ref.window_counts(ref.structured_rows(129, nf, Wn, seed=nf)[0], Wn)
        assert (counts == 64).any() and counts.max() >= 65, (k, nf, Wn)


def test_knn_window_refuses_invalid_arguments():
    from pymde_amd import _lib, sparse
    for k, nf in ((0, 10), (-1, 10), (65, 10), (15, 0), (15, -3)):
        with pytest.raises(_lib.MdeHipError, match="mde_sparse_knn_window") as e:
            sparse.knn_window(k, nf)
        assert e.value.code == _lib.MDE_E_INVALID
    assert sparse.knn_window(15, 1) == sparse.knn_window(15, 8)              # never narrower than the features need
    assert sparse.knn_window(15, 2 ** 31 - 1) == sparse.knn_window(15, 2 ** 20)


def test_knn_lists_agree_with_scipy_on_ties():
    rng = np.random.default_rng(1)
    X = rng.integers(0, 3, (60, 4)).astype(np.float64)      # few distinct rows: most distances are tied
    X[[5, 17, 40]] = 0.0
    D = cdist(X, X, "sqeuclidean")
    np.fill_diagonal(D, np.inf)
    for k in (1, 7, 59, 64):
        idx, d2 = ref.knn_lists(ref.sp.csr_matrix(X), k)
        assert idx.shape == (60, k) and d2.shape == (60, k)
        kk = min(k, 59)
        for r in range(60):
            want = sorted(range(60), key=lambda c: (D[r, c], c))[:kk]
            assert idx[r, :kk].tolist() == want
            assert (d2[r, :kk] == D[r, want]).all()
        assert (idx[:, kk:] == -1).all() and (d2[:, kk:] == ref.FLT_MAX).all()
    assert (np.diff(d2[:, :7], axis=1) == 0).any()           # there were ties to order
    idx, d2 = ref.knn_lists(ref.sp.csr_matrix(X[:3]), 5)     # fewer other rows than k
    assert (idx[:, 2:] == -1).all() and (idx[:, :2] >= 0).all() and (d2[:, 2:] == ref.FLT_MAX).all()
    edges = np.array([[0, 1], [5, 17], [3, 3], [59, 2]])
    np.testing.assert_allclose(ref.pair_distances(ref.sp.csr_matrix(X), edges),
                               np.sqrt(cdist(X, X, "sqeuclidean")[edges[:, 0], edges[:, 1]]), rtol=1e-15)


def test_emulation_is_exact_on_the_structured_rows():
    A, _, _ = ref.structured_rows(40, 257, 128, seed=3)
    np.testing.assert_array_equal(ref.emulate_float32_d2(A).astype(np.float64), ref.squared_distances(A))


@functools.lru_cache(maxsize=None)
def _accuracy_case():
    A, length = ref.accuracy_rows(256, 3 * 128 + 1, seed=7)
    return A, length, ref.squared_distances(A), ref.emulate_float32_d2(A).astype(np.float64)


def test_accuracy_input():
    A, length, D, _ = _accuracy_case()
    assert A.shape == (256, 385) and (np.diff(A.indptr) == length).all()
    assert sorted(set(length)) == [5, 70, 300] and (A.data >= 0.5).all() and (A.data < 2.001).all()
    for W in (128, 152, 192):                # the windows of k = 15, 1, 64, at which the GPU test searches it
        assert ref.window_counts(A, W)[length == 300].max(1).min() > 64      # every long row, in some window
    twins = D[np.arange(128), np.arange(128) + 128]
    assert (twins > 0).all() and twins.max() < 1.1e-6
    assert (np.argsort(D + np.diag(np.full(256, np.inf)), axis=1)[:128, 0] == np.arange(128) + 128).all()


def test_emulated_float32_error_is_under_half_the_bound():
    """RTOL and STOL of tests/test_gpu_sparse_structure.py: float32 arithmetic in the kernel's order stays
    under half of ``RTOL * true + STOL * (|x|^2 + |y|^2)`` on every pair of the accuracy input."""
    rtol, stol = 1e-5, 2e-6
    A, length, D, E = _accuracy_case()
    sq = np.asarray(A.multiply(A).sum(1), dtype=np.float64).ravel()
    scale = sq[:, None] + sq[None, :]
    off = ~np.eye(256, dtype=bool)
    ratio = np.abs(E - D) / (rtol * D + stol * scale)
    for m in (5, 70, 300):
        rows = length == m
        print("rows of %d entries: emulated err / scale %.3e, err / bound %.3f"
              % (m, (np.abs(E - D) / scale)[rows][off[rows]].max(), ratio[rows][off[rows]].max()))
    assert ratio[off].max() < 0.5, ratio[off].max()

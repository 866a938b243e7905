"""Host-side canonicalisation of sparse data matrices (pymde_amd.sparse): no GPU needed."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

from pymde_amd import sparse


def _check_canonical(indptr, indices, values, shape, dense):
    assert indptr.dtype == np.int64 and indices.dtype == np.int32 and values.dtype == np.float32
    n, nf = shape
    assert indptr.shape == (n + 1,) and indptr[0] == 0 and indptr[-1] == len(indices) == len(values)
    assert (np.diff(indptr) >= 0).all()
    for r in range(n):
        row = indices[indptr[r]:indptr[r + 1]]
        assert (np.diff(row) > 0).all() and (row >= 0).all() and (row < nf).all()
    assert (values != 0).all()
    back = sp.csr_matrix((values, indices, indptr), shape=shape).toarray()
    np.testing.assert_array_equal(back, dense.astype(np.float32))


def test_every_scipy_format_canonicalises_to_the_same_csr():
    rng = np.random.default_rng(0)
    A = sp.random(40, 70, density=0.1, format="csr", random_state=1, dtype=np.float64)
    A.data = rng.integers(1, 6, A.nnz).astype(np.float64)
    dense = A.toarray()
    ref = sparse.canonical_csr_host(A)
    _check_canonical(*ref, dense)
    # a COO with duplicate entries that sum to the same matrix
    coo = A.tocoo()
    dup = sp.coo_matrix((np.concatenate([coo.data - 1.0, np.ones(coo.nnz)]),
                         (np.concatenate([coo.row, coo.row]), np.concatenate([coo.col, coo.col]))), shape=A.shape)
    # a CSR whose rows hold their column ids in reverse order
    rev = A.copy()
    for r in range(A.shape[0]):
        lo, hi = rev.indptr[r], rev.indptr[r + 1]
        rev.indices[lo:hi] = rev.indices[lo:hi][::-1].copy()
        rev.data[lo:hi] = rev.data[lo:hi][::-1].copy()
    rev.has_sorted_indices = False
    forms = [A.tocsc(), A.tocoo(), dup, rev, A.astype(np.float32), A.tolil(), A.todok(), sp.csr_array(A)]
    for m in forms:
        before = m.copy()
        got = sparse.canonical_csr_host(m)
        for a, b in zip(got[:3], ref[:3]):
            np.testing.assert_array_equal(a, b)
        assert got[3] == ref[3] == (40, 70)
        assert (m != before).nnz == 0    # the caller's matrix is left as it was


def test_empty_rows_and_explicit_zeros():
    A = sp.csr_matrix((np.array([0.0, 2.0, 3.0]), np.array([1, 0, 4]), np.array([0, 0, 2, 2, 3])), shape=(4, 5))
    indptr, indices, values, shape = sparse.canonical_csr_host(A)
    np.testing.assert_array_equal(indptr, [0, 0, 1, 1, 2])
    np.testing.assert_array_equal(indices, [0, 4])
    np.testing.assert_array_equal(values, [2.0, 3.0])
    # an all-zero matrix is a valid data matrix (nnz = 0)
    indptr, indices, values, shape = sparse.canonical_csr_host(sp.csr_matrix((3, 7)))
    np.testing.assert_array_equal(indptr, [0, 0, 0, 0])
    assert len(indices) == len(values) == 0 and shape == (3, 7)


def test_shape_checks():
    with pytest.raises(ValueError):
        sparse.canonical_csr_host(sp.csr_matrix((0, 5)))
    with pytest.raises(ValueError):
        sparse.canonical_csr_host(sp.csr_matrix((5, 0)))
    with pytest.raises(ValueError):
        sparse.canonical_csr_host(sp.coo_array(np.array([1.0, 0.0, 2.0])))   # 1-D
    with pytest.raises(TypeError):
        sparse.canonical_csr_host(np.eye(3))


def test_is_sparse():
    A = sp.random(5, 6, density=0.3, random_state=0)
    assert sparse.is_sparse(A) and sparse.is_sparse(A.tocsc())
    t = torch.tensor(A.toarray())
    assert sparse.is_sparse(t.to_sparse()) and sparse.is_sparse(t.to_sparse_csr())
    assert not sparse.is_sparse(t) and not sparse.is_sparse(A.toarray())

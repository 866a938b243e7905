"""Sparse data matrices: scipy.sparse (any format) or torch sparse COO / CSR tensors as a canonical
device CSR for the kernels of ``csrc/mde_sparse.hip`` [ref: preprocess/data_matrix.py:11-178, which
accepts scipy.sparse data matrices throughout].

The canonical form: duplicate entries summed, column ids sorted (strictly increasing within a row),
explicit zeros dropped, float32 values, int32 column ids, int64 row pointers.  scipy inputs are
canonicalised on the host (``canonical_csr_host``, a pure function) and copied to the device once;
torch inputs are canonicalised on their own device.
"""
import numpy as np
import torch

from pymde_amd import util

_MAX_DIM = 2 ** 31 - 1


def _scipy_sparse():
    try:
        import scipy.sparse
    except ImportError:  # no scipy: only torch sparse tensors can be sparse here
        return None
    return scipy.sparse


def is_sparse(data):
    """True for a scipy sparse matrix / array or a torch sparse COO / CSR tensor."""
    if isinstance(data, torch.Tensor):
        return data.layout in (torch.sparse_coo, torch.sparse_csr)
    sp = _scipy_sparse()
    return sp is not None and sp.issparse(data)


def _check_shape(shape):
    if len(shape) != 2:
        raise ValueError(f"a sparse data matrix must be 2-D (got shape {tuple(shape)})")
    n, nf = int(shape[0]), int(shape[1])
    if n < 1:
        raise ValueError("a sparse data matrix needs at least one row")
    if nf < 1:
        raise ValueError("a sparse data matrix needs at least one column")
    if n > _MAX_DIM or nf > _MAX_DIM:
        raise ValueError(f"sparse data matrices are limited to 2^31 - 1 rows and columns (got {n} x {nf})")
    return n, nf


def canonical_csr_host(matrix):
    """scipy sparse matrix (any format) -> ``(indptr int64, indices int32, values float32, (n, nf))``
    as NumPy arrays: duplicates summed, indices sorted, explicit zeros dropped.  ``matrix`` is not
    modified."""
    sp = _scipy_sparse()
    if sp is None or not sp.issparse(matrix):
        raise TypeError("canonical_csr_host expects a scipy sparse matrix")
    n, nf = _check_shape(matrix.shape)
    csr = sp.csr_matrix(matrix, copy=True)   # any format -> CSR (a copy: the caller's matrix stays as it was)
    csr.sum_duplicates()                      # sums duplicates and sorts the column ids of every row
    csr.eliminate_zeros()
    indptr = np.ascontiguousarray(csr.indptr, dtype=np.int64)
    indices = np.ascontiguousarray(csr.indices, dtype=np.int32)
    values = np.ascontiguousarray(csr.data, dtype=np.float32)
    return indptr, indices, values, (n, nf)


class DeviceCSR(object):
    """A canonical CSR on a GPU: ``indptr`` int64 [n + 1], ``indices`` int32 [nnz], ``values`` float32 [nnz]."""

    def __init__(self, indptr, indices, values, shape):
        self.indptr, self.indices, self.values = indptr, indices, values
        self.n, self.n_features = int(shape[0]), int(shape[1])
        self.shape = (self.n, self.n_features)
        self.nnz = int(values.shape[0])
        self.device = values.device

    @property
    def density(self):
        return self.nnz / (float(self.n) * float(self.n_features))

    def to_dense(self):
        """The dense float32 copy [n, n_features] (for the dense kernels)."""
        t = torch.sparse_csr_tensor(self.indptr, self.indices.to(torch.int64), self.values, self.shape,
                                    device=self.device)
        return t.to_dense().contiguous()


def to_device_csr(data, device=None):
    """Canonical device CSR of a sparse data matrix (see ``is_sparse``).  ``device`` defaults to the
    tensor's own device for a CUDA tensor and to the default device otherwise."""
    if isinstance(data, torch.Tensor):
        if data.layout not in (torch.sparse_coo, torch.sparse_csr):
            raise TypeError("to_device_csr expects a sparse tensor")
        if data.layout == torch.sparse_coo and data.dense_dim() != 0:
            raise ValueError("hybrid sparse tensors (dense dimensions) are not data matrices")
        n, nf = _check_shape(data.shape)
        if device is None:
            device = data.device if data.is_cuda else util.get_default_device()
        device = util.require_cuda_device(device)
        t = data.to(device)
        coo = (t if t.layout == torch.sparse_coo else t.to_sparse_coo()).coalesce()   # sums duplicates, sorts
        vals = coo.values().to(torch.float32)
        keep = vals != 0
        rows, cols = coo.indices()[0][keep], coo.indices()[1][keep]
        vals = vals[keep].contiguous()
        counts = torch.bincount(rows, minlength=n)
        indptr = torch.zeros(n + 1, dtype=torch.int64, device=device)
        torch.cumsum(counts, 0, out=indptr[1:])
        return DeviceCSR(indptr, cols.to(torch.int32).contiguous(), vals, (n, nf))
    if not is_sparse(data):
        raise TypeError("to_device_csr expects a scipy sparse matrix or a torch sparse tensor")
    indptr, indices, values, shape = canonical_csr_host(data)
    device = util.require_cuda_device(util.get_default_device() if device is None else device)
    return DeviceCSR(torch.from_numpy(indptr).to(device), torch.from_numpy(indices).to(device),
                     torch.from_numpy(values).to(device), shape)

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

from pymde_amd import _lib
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

    def transpose(self):
        """The canonical CSR of the transposed matrix (``n_features`` rows, ``n`` columns, column ids
        increasing within a row), on the device of this one -- a CPU as well: only torch is used.  A stable
        sort of the column ids keeps the entries of a column in row order."""
        rows = torch.repeat_interleave(torch.arange(self.n, dtype=torch.int32, device=self.device),
                                       self.indptr[1:] - self.indptr[:-1])
        cols = self.indices.to(torch.int64)
        order = torch.sort(cols, stable=True).indices
        indptr = torch.zeros(self.n_features + 1, dtype=torch.int64, device=self.device)
        torch.cumsum(torch.bincount(cols, minlength=self.n_features), 0, out=indptr[1:])
        return DeviceCSR(indptr, rows[order].contiguous(), self.values[order].contiguous(),
                         (self.n_features, self.n))

    def validate(self):
        """``mde_sparse_validate`` on this matrix: an ``MdeHipError`` for a malformed CSR.  The products of
        ``spmm`` index through the arrays unchecked, so a matrix is validated once before the first one."""
        with torch.cuda.device(self.device):
            _lib.check(_lib.load().mde_sparse_validate(self.n, self.n_features, self.nnz, _lib.ptr(self.indptr),
                                                       _lib.ptr(self.indices), _lib.ptr(self.values),
                                                       _lib.stream_ptr(self.device)))
        return self


def from_dense(X):
    """The canonical CSR of the non-zero entries of a dense float32 [n, nf] tensor, on its device (NaN and
    infinity are kept as entries, so a finiteness check of the result sees them)."""
    n, nf = _check_shape(X.shape)
    mask = X != 0
    indptr = torch.zeros(n + 1, dtype=torch.int64, device=X.device)
    torch.cumsum(mask.sum(1), 0, out=indptr[1:])
    cols = mask.nonzero()[:, 1].to(torch.int32).contiguous()       # row-major: ascending within a row
    return DeviceCSR(indptr, cols, X[mask].to(torch.float32).contiguous(), (n, nf))


def spmm_segment():
    """The segment length of ``mde_csr_spmm``: a longer row is summed in pieces of this many entries."""
    return int(_lib.load().mde_csr_spmm_segment())


def knn_window(k, nf):
    """The number of feature columns per window of the sparse k-NN kernel at ``k`` neighbours on a matrix of
    ``nf`` columns (``mde_sparse_knn_window``): a row's stored entries are walked one window at a time."""
    W = int(_lib.load().mde_sparse_knn_window(int(k), int(nf)))
    if W < 0:
        _lib.check(W)
    return W


def spmm(csr, B, u=None, v=None, work=None):
    """``csr @ B - outer(u, v)`` by ``mde_csr_spmm``: ``B`` float32 [n_features, r] on the GPU, ``r <= 256``;
    ``u`` float32 [n] (None: all ones), ``v`` float64 [r] (None: no correction).  Float64 sums, one rounding;
    returns float32 [n, r].  ``csr`` must be a valid canonical CSR (``DeviceCSR.validate``): it is not checked
    here.  ``work``: a buffer from ``spmm_work`` to reuse across calls."""
    lib = _lib.load()
    if B.dim() != 2 or int(B.shape[0]) != csr.n_features:
        raise ValueError(f"spmm: B must be [{csr.n_features}, r] (got shape {tuple(B.shape)})")
    r = int(B.shape[1])
    B = B.to(device=csr.device, dtype=torch.float32).contiguous()
    if u is not None:
        u = u.to(device=csr.device, dtype=torch.float32).contiguous()
        if u.numel() != csr.n:
            raise ValueError(f"spmm: u must hold {csr.n} values (got {u.numel()})")
    if v is not None:
        v = v.to(device=csr.device, dtype=torch.float64).contiguous()
        if v.numel() != r:
            raise ValueError(f"spmm: v must hold {r} values (got {v.numel()})")
    out = torch.empty((csr.n, r), dtype=torch.float32, device=csr.device)
    with torch.cuda.device(csr.device):
        if work is None or work.numel() < max(int(lib.mde_csr_spmm_work_bytes(csr.n, csr.nnz, r)), 0):
            work = spmm_work(csr, r)
        _lib.check(lib.mde_csr_spmm(csr.n, csr.n_features, csr.nnz, _lib.ptr(csr.indptr), _lib.ptr(csr.indices),
                                    _lib.ptr(csr.values), r, _lib.ptr(B), _lib.ptr(u), _lib.ptr(v), _lib.ptr(out),
                                    _lib.ptr(work), _lib.stream_ptr(csr.device)))
    return out


def spmm_work(csr, r):
    """The scratch buffer of ``spmm(csr, B [n_features, r])`` (``mde_csr_spmm_work_bytes``)."""
    return _lib.work_buffer(_lib.load().mde_csr_spmm_work_bytes, csr.n, csr.nnz, int(r), device=csr.device)


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

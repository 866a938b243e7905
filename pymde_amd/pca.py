"""Truncated principal components on the GPU: the reduction that precedes a k-NN search on wide data
(``preprocess.principal_components``).

Dense data take the exact route of ``quadratic.pca``: a centred float32 copy, its Gram matrix by ``mde_gram``, a
host ``eigh`` in float64, the scores by one ``mde_right_multiply``.

Sparse data (scipy sparse, torch sparse COO / CSR) take the randomized range finder with power iterations
(Halko, Martinsson and Tropp 2011, algorithms 4.4 / 5.1) on the CENTRED matrix ``A_c = A - 1 mean^T``, which is
never formed: ``mde_csr_spmm`` subtracts the rank-one term inside the product,
    A_c X   = A X   - 1 (mean^T X)        on the CSR,
    A_c^T Q = A^T Q - mean (1^T Q)        on its transpose (``DeviceCSR.transpose``, once per fit),
with float64 sums, so the cancellation costs nothing.  The blocks are orthonormalised by the two-pass Gram
orthonormalisation of the spectral solver (``quadratic._orthonormal``); only r x r matrices visit the host.
"""
import numpy as np
import torch

from pymde_amd import _lib
from pymde_amd import binary as _binary
from pymde_amd import metrics as _metrics
from pymde_amd import sparse as _sparse
from pymde_amd import util
from pymde_amd.quadratic import _Ops, _centred_basis, _orthonormal, _sym

MAX_RANK = 256      # the widest block of mde_csr_spmm


class PrincipalComponents(object):
    """A fitted truncated PCA; every field is a tensor on the GPU.

    ``scores`` float32 [n, m]: ``(data - mean) @ components.T``, not whitened, so distances between rows of
    ``scores`` approximate the distances between rows of ``data``; ``components`` float32 [m, nf], orthonormal
    rows, each oriented so that its entry of largest magnitude is positive; ``mean`` float32 [nf], the column
    means; ``singular_values`` float64 [m], descending; ``explained_variance`` float64 [m]
    = ``singular_values ** 2 / (n - 1)``; ``total_variance`` float64 scalar, the summed variance of all
    columns (``explained_variance / total_variance`` is the ratio)."""

    def __init__(self, scores, components, mean, singular_values, total_variance):
        self.scores, self.components, self.mean = scores, components, mean
        self.singular_values = singular_values
        self.explained_variance = singular_values ** 2 / max(int(scores.shape[0]) - 1, 1)
        self.total_variance = total_variance
        self._offset = None      # mean^T components^T, float64 [m]

    def transform(self, new_data):
        """``(new_data - mean) @ components.T`` as float32 [n_new, m] on the GPU, for dense or sparse rows of
        ``nf`` columns.  Both go through ``mde_csr_spmm`` (a dense matrix as the CSR of its non-zeros), so the
        sums are float64 and a row gets the same scores in either form."""
        device = self.components.device
        nf = int(self.components.shape[1])
        if not hasattr(new_data, "shape") or len(new_data.shape) != 2 or int(new_data.shape[1]) != nf:
            raise ValueError(f"transform expects a matrix of {nf} columns (got shape "
                             f"{tuple(getattr(new_data, 'shape', ()))})")
        if _sparse.is_sparse(new_data):
            csr = _sparse.to_device_csr(new_data, device).validate()
        else:
            if not isinstance(new_data, torch.Tensor):
                new_data = torch.as_tensor(new_data)
            csr = _sparse.from_dense(new_data.detach().to(device=device, dtype=torch.float32))
        _check_finite_csr(csr)
        with torch.no_grad(), torch.cuda.device(device):
            V = self.components.t().contiguous()
            if self._offset is None:
                self._offset = _gram_device(_Ops(nf, device, int(V.shape[1])), self.mean.unsqueeze(1), V)
            return _sparse.spmm(csr, V, None, self._offset)


def _check_finite_csr(csr):
    from pymde_amd.preprocess import _check_finite_csr as check    # (preprocess imports this module)
    check(csr)


def _gram_device(ops, A, B):
    """``A^T B`` (``mde_gram``, float64) left on the device as a flat float64 [da * db]: the r-vectors
    ``mean^T X`` and ``1^T Q`` of the centred products never visit the host."""
    da, db = int(A.shape[1]), int(B.shape[1])
    out = torch.empty(da * db, dtype=torch.float64, device=ops.device)
    _lib.check(ops.lib.mde_gram(ops.n, da, db, _lib.ptr(A), _lib.ptr(B), _lib.ptr(out), _lib.ptr(ops.work),
                                ops._stream()))
    return out


def check_arguments(shape, n_components, n_oversamples=10, n_iter=4, sparse=False):
    """The argument errors of ``principal_components`` that need no device; returns ``(n, nf, m, r)`` with ``r``
    the width of the randomized route's block."""
    if len(shape) != 2:
        raise ValueError(f"principal_components expects a data matrix [n, n_features] (got shape {tuple(shape)})")
    n, nf = int(shape[0]), int(shape[1])
    m = int(n_components)
    if m < 1 or m >= min(n, nf):
        raise ValueError(f"n_components must satisfy 1 <= n_components < min(n, n_features) = {min(n, nf)} "
                         f"(got {n_components})")
    if int(n_oversamples) < 0 or int(n_iter) < 0:
        raise ValueError("n_oversamples and n_iter must not be negative")
    r = min(m + int(n_oversamples), min(n, nf))
    if sparse and r > MAX_RANK:
        raise ValueError(f"the randomized route works on blocks of n_components + n_oversamples = {r} columns, "
                         f"and the sparse product serves at most {MAX_RANK}; ask for fewer")
    return n, nf, m, r


def principal_components(data, n_components, *, n_oversamples=10, n_iter=4, seed=0, test_matrix=None,
                         device=None):
    """The top ``n_components`` principal components of a data matrix (rows = items) as a
    ``PrincipalComponents``: scores that keep the data's distances, the basis, the mean, the singular values.
    ``1 <= n_components < min(n, n_features)``; NaN or infinity in the data is a ``ValueError``.

    Dense ``data`` (``np.ndarray`` / ``torch.Tensor``): exact, through the ``n_features x n_features`` Gram matrix
    and a host ``eigh`` as in ``pymde_amd.pca`` -- meant for a few thousand features at most;
    ``n_oversamples``, ``n_iter``, ``seed`` and ``test_matrix`` are not used.

    Sparse ``data`` (scipy sparse, torch sparse COO / CSR): randomized, on the centred matrix, which is never
    densified.  With ``r = min(n_components + n_oversamples, n, n_features) <= 256``: a start block
    ``[n_features, r]`` -- standard normal from a ``torch.Generator`` on the device seeded with ``seed``, or
    ``test_matrix`` when given -- is multiplied by the centred data and orthonormalised, ``n_iter`` power
    iterations (two products and two orthonormalisations each) sharpen the basis, and the components come from
    the ``r x r`` eigenproblem of the projected matrix.  ``2 n_iter + 3`` products with ``r`` columns in all,
    plus the transpose and two one-column products for the mean.  The same ``seed`` gives the same bits.  Four
    iterations bring the leading singular values within about 1e-6 of the exact ones when the spectrum has a gap
    after ``n_components``; without a gap the subspace is one that captures as much variance, not the
    eigenvectors themselves.  ``util.SolverError`` when a block loses rank (data of rank below ``r``)."""
    _binary.refuse(data, "principal_components")
    is_sparse = _sparse.is_sparse(data)
    if not is_sparse and not isinstance(data, torch.Tensor):
        data = torch.as_tensor(data)
    n, nf, m, r = check_arguments(data.shape, n_components, n_oversamples, n_iter, is_sparse)
    if is_sparse and test_matrix is not None and tuple(test_matrix.shape) != (nf, r):
        raise ValueError(f"test_matrix must be [n_features, r] = [{nf}, {r}] (got {tuple(test_matrix.shape)})")
    if is_sparse:
        csr = _sparse.to_device_csr(data, device)
        with torch.no_grad(), torch.cuda.device(csr.device):
            return _fit_sparse(csr, m, r, int(n_iter), seed, test_matrix)
    if device is None:
        device = data.device if data.is_cuda else util.get_default_device()
    device = util.require_cuda_device(device)
    with torch.no_grad(), torch.cuda.device(device):
        return _fit_dense(data.detach().to(device=device, dtype=torch.float32).contiguous(), m, device)


def _fit_dense(Y, m, device):
    n = int(Y.shape[0])
    mean, _ = _metrics.column_stats(Y)                       # (and the NaN / infinity check)
    ops, Yc, V, sing, G = _centred_basis(Y, m, device)
    scores = ops.rmul(Yc, V)

    def on_device(a, dtype):
        return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(device)

    return PrincipalComponents(scores, on_device(V.T, torch.float32), mean.to(device=device, dtype=torch.float32),
                               on_device(sing, torch.float64), on_device(np.trace(G) / max(n - 1, 1), torch.float64))


def _column_means(csr_t, n):
    """float64 [nf] column means of the matrix whose transpose is ``csr_t``: the float64 row sums of ``csr_t`` come
    out of the product rounded to float32, so a second product returns the rounding residual
    ``A^T 1 - sums`` (``u = sums``, ``v = 1``; tiny, hence all but exact in float32) and the two are added in
    double: the float32 mean is then the float64 mean rounded once."""
    device = csr_t.device
    ones = torch.ones((n, 1), dtype=torch.float32, device=device)
    sums = _sparse.spmm(csr_t, ones)
    residual = _sparse.spmm(csr_t, ones, sums.reshape(-1), torch.ones(1, dtype=torch.float64, device=device))
    return (sums.double() + residual.double()).reshape(-1) / float(n)


def _fit_sparse(csr, m, r, n_iter, seed, test_matrix):
    device, n, nf = csr.device, csr.n, csr.n_features
    csr.validate()
    _check_finite_csr(csr)
    csr_t = csr.transpose()
    mean64 = _column_means(csr_t, n)
    mean = mean64.to(torch.float32)
    total = (csr.values.double().pow(2).sum() - n * mean64.pow(2).sum()) / max(n - 1, 1)
    ops_n, ops_f = _Ops(n, device, r), _Ops(nf, device, r)
    work, work_t = _sparse.spmm_work(csr, r), _sparse.spmm_work(csr_t, r)
    mean_col = mean.unsqueeze(1).contiguous()
    ones_col = torch.ones((n, 1), dtype=torch.float32, device=device)

    def centred(X):         # A_c X, [n, *]
        return _sparse.spmm(csr, X, None, _gram_device(ops_f, mean_col, X), work)

    def centred_t(Q):       # A_c^T Q, [nf, *]
        return _sparse.spmm(csr_t, Q, mean, _gram_device(ops_n, ones_col, Q), work_t)

    def orth(ops, S):
        out = _orthonormal(ops, [S])
        if int(out.shape[1]) < r:
            raise util.SolverError(f"principal_components: a block of {r} columns lost rank (the centred data "
                                   f"have rank below n_components + n_oversamples = {r}); ask for fewer")
        return out

    if test_matrix is None:
        generator = torch.Generator(device=device)
        generator.manual_seed(int(seed))
        omega = torch.randn((nf, r), generator=generator, device=device, dtype=torch.float32)
    else:
        omega = torch.as_tensor(test_matrix).to(device=device, dtype=torch.float32).contiguous()
    Q = orth(ops_n, centred(omega))
    for _ in range(n_iter):
        Z = orth(ops_f, centred_t(Q))
        Q = orth(ops_n, centred(Z))
    B = centred_t(Q)                                         # [nf, r]; A_c ~ Q B^T
    evals, W = np.linalg.eigh(_sym(ops_f.gram(B, B)))        # B^T B = W S^2 W^T
    order = np.argsort(evals)[::-1][:m]
    sing = np.sqrt(np.maximum(evals[order], 0.0))
    if np.any(sing <= 1e-12 * max(float(sing.max()), 1e-300)):
        raise util.SolverError("principal_components: the centred data matrix has rank below n_components")
    V = ops_f.rmul(B, W[:, order] / sing[None, :])           # [nf, m] = B W S^-1
    top = V.abs().argmax(dim=0)
    V = (V * torch.sign(V[top, torch.arange(m, device=device)])[None, :]).contiguous()
    scores = centred(V)
    return PrincipalComponents(scores, V.t().contiguous(), mean, torch.from_numpy(sing).to(device), total)

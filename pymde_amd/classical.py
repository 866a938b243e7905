"""Classical (Torgerson) scaling and distance-based triangulation on the GPU (``csrc/mde_pair_apply.hip``, DESIGN
section 6p): the closed-form start of the dense problems, and ``cmdscale`` as a function in its own right.

Classical MDS embeds by the top eigenvectors of ``B = -1/2 J S J``, ``S`` the matrix of SQUARED deviations and
``J = I - 1 1^T / n``.  ``S`` is n x n and is never formed: one product ``S V`` with a thin block ``V`` is one walk of
the Gram tile (``mde_pair_sqdist_apply``), the centring on both sides follows as rank-one terms in float64, and the
eigenvectors come from a randomized subspace iteration with the block tools of ``pymde_amd.pca``; only r x r matrices
visit the host.  Euclidean ``data`` need none of this: the classical solution of Euclidean distances is the PCA scores.

``triangulate`` places new rows against embedded ones from their squared deviations to ALL of them, in closed form
(the out-of-sample step of landmark MDS, de Silva and Tenenbaum): one rectangular call of the same kernel.
"""
import numpy as np
import torch

from pymde_amd import _lib
from pymde_amd import metrics as _metrics
from pymde_amd import util
from pymde_amd.quadratic import _Ops, _orthonormal, _sym

MAX_DIM = 8         # the widest embedding of the dense problems
MAX_RANK = 32       # PAIR_APPLY_MAX_R of csrc/mde_pair_apply.hip: the widest block of one product
NOISE_RTOL = 1e-6   # a kept eigenvalue within this fraction of the largest is rounding noise: a zero column
PINV_RCOND = 1e-6   # of the d x d Gram matrix of the embedded rows in `triangulate`


class ClassicalMDS(object):
    """A classical scaling; every field is a tensor on the GPU.

    ``X`` float32 [n, d], centred: column k is ``sqrt(eigenvalues[k])`` times the k-th eigenvector of ``B``, oriented
    so that its entry of largest magnitude is positive.  ``eigenvalues`` float64 [d], descending, the
    ``embedding_dim`` algebraically largest eigenvalues of ``B``, clipped at 0: a negative one (``B`` is indefinite
    for non-Euclidean deviations) and one within 1e-6 of the largest (rounding noise: deviations of rank below d)
    become 0 and a zero column, as in R's ``cmdscale``.  ``total`` float64 scalar: ``trace(B)``, the sum of all
    eigenvalues (``eigenvalues / total`` is the share each axis explains).  ``negative`` bool: a kept eigenvalue was
    negative beyond that noise and was clipped."""

    def __init__(self, X, eigenvalues, total, negative):
        self.X, self.eigenvalues, self.total, self.negative = X, eigenvalues, total, bool(negative)


def sqdist_apply(V, *, Q=None, C=None, mode=0, Dm=None, skip_diagonal=False, slices=0, work=None):
    """``mde_pair_sqdist_apply`` on prepared float32 tensors on one GPU: float64 [n_q, r] ``= S V`` for ``V`` [n_c, r],
    ``r <= 32``.  Either both ``Q`` [n_q, nf] and ``C`` [n_c, nf] (the prepared data rows; ``mode`` 0: squared
    Euclidean distances, 1: squared cosine / correlation distances of unit rows) or ``Dm`` [n_q, n_c] (a matrix of
    deviations, squared in double).  ``skip_diagonal`` leaves out ``j == i``."""
    source = Dm if Dm is not None else Q
    n_c, r, device = int(V.shape[0]), int(V.shape[1]), V.device
    n_q = int(source.shape[0]) if source is not None else n_c
    lib = _lib.load()
    out = torch.empty((n_q, r), dtype=torch.float64, device=device)
    with torch.cuda.device(device):
        if work is None:
            work = _lib.work_buffer(lib.mde_pair_sqdist_apply_work_bytes, n_q, n_c, r, slices, device=device)
        _lib.check(lib.mde_pair_sqdist_apply(n_q, n_c, 0 if Q is None else int(Q.shape[1]), _lib.ptr(Q), _lib.ptr(C),
                                             int(mode), _lib.ptr(Dm), 1 if skip_diagonal else 0, r, _lib.ptr(V),
                                             slices, _lib.ptr(out), _lib.ptr(work), _lib.stream_ptr(device)))
    return out


def check_arguments(n, embedding_dim, n_oversamples=10, n_iter=4):
    """The argument errors of ``classical_mds`` that need no device; returns ``(d, r)`` with ``r`` the width of the
    iteration's block."""
    d = int(embedding_dim)
    if not 1 <= d <= MAX_DIM:
        raise ValueError(f"embedding_dim must lie in [1, {MAX_DIM}] (got {embedding_dim})")
    if int(n_oversamples) < 0 or int(n_iter) < 0:
        raise ValueError("n_oversamples and n_iter must not be negative")
    r = d + int(n_oversamples)
    if r > min(MAX_RANK, int(n) - 1):
        raise ValueError(f"the subspace iteration works on blocks of embedding_dim + n_oversamples = {r} columns, at "
                         f"most min({MAX_RANK}, n - 1) = {min(MAX_RANK, int(n) - 1)}; ask for fewer")
    return d, r


def _kept(evals, d):
    """The ``d`` algebraically largest of the Ritz values ``evals`` as ``(order, eigenvalues, negative)``: clipped at
    0, noise (within ``NOISE_RTOL`` of the largest) set to 0, padded with zeros where the block was narrower."""
    order = np.argsort(evals)[::-1][:d]
    lam = evals[order]
    floor = NOISE_RTOL * max(float(lam[0]), 0.0) if lam.size else 0.0
    negative = bool(np.any(lam < -floor))
    lam = np.where(lam > floor, lam, 0.0)
    return order, np.concatenate([lam, np.zeros(d - lam.size)]), negative


def _oriented(X):
    """Every column of ``X`` with its entry of largest magnitude positive (the sign rule of ``pymde_amd.pca``)."""
    top = X.abs().argmax(dim=0)
    sign = torch.sign(X[top, torch.arange(int(X.shape[1]), device=X.device)])
    return X * torch.where(sign == 0, torch.ones_like(sign), sign)[None, :]


def _scale(A=None, mode=0, Dm=None, deviation_scale=1.0, d=2, r=12, n_iter=4, seed=0, test_matrix=None):
    """The classical scaling of a prepared source on one GPU -- ``A`` float32 [n, nf] with ``mode``, or ``Dm`` float32
    [n, n] -- by the randomized subspace iteration on ``B``; a ``ClassicalMDS``."""
    source = A if A is not None else Dm
    n, device = int(source.shape[0]), source.device
    if test_matrix is not None and tuple(test_matrix.shape) != (n, r):
        raise ValueError(f"test_matrix must be [n, r] = [{n}, {r}] (got {tuple(test_matrix.shape)})")
    scale2 = float(deviation_scale) ** 2
    lib = _lib.load()
    work = _lib.work_buffer(lib.mde_pair_sqdist_apply_work_bytes, n, n, r, 0, device=device)
    ops = _Ops(n, device, r)

    def S(V):
        return sqdist_apply(V.contiguous(), Q=A, C=A, mode=mode, Dm=Dm, skip_diagonal=True, work=work)

    s = S(torch.ones((n, 1), dtype=torch.float32, device=device)).reshape(-1)          # S 1, float64 [n]

    def B(V):
        """-1/2 J S J V as float64 [n, *]: S (V - 1 m^T) = S V - s m^T with m the column means of V, then centred."""
        Y = S(V)
        Y -= s[:, None] * V.double().mean(0)[None, :]
        Y -= Y.mean(0, keepdim=True)
        return Y.mul_(-0.5 * scale2)

    def orth(Y):
        out = _orthonormal(ops, [Y.to(torch.float32).contiguous()])
        if int(out.shape[1]) < 1:
            raise util.SolverError("classical_mds: every deviation is zero (B = 0): there is nothing to embed")
        return out

    if test_matrix is None:
        generator = torch.Generator(device=device)
        generator.manual_seed(int(seed))
        omega = torch.randn((n, r), generator=generator, device=device, dtype=torch.float32)
    else:
        omega = torch.as_tensor(test_matrix).to(device=device, dtype=torch.float32).contiguous()
    Qb = orth(B(omega))
    for _ in range(n_iter):
        Qb = orth(B(Qb))
    T = (Qb.double().t() @ B(Qb)).cpu().numpy()                      # Q^T B Q, r x r
    evals, Z = np.linalg.eigh(_sym(T))
    order, lam, negative = _kept(evals, d)
    X = torch.zeros((n, d), dtype=torch.float64, device=device)
    basis = torch.from_numpy(np.ascontiguousarray(Z[:, order] * np.sqrt(lam[:order.size])[None, :])).to(device)
    X[:, :order.size] = Qb.double() @ basis
    X -= X.mean(0, keepdim=True)
    total = s.sum() * (scale2 / (2.0 * n))
    return ClassicalMDS(_oriented(X).to(torch.float32).contiguous(), torch.from_numpy(lam).to(device), total, negative)


def _from_scores(pc, n, deviation_scale):
    """The ``ClassicalMDS`` of Euclidean rows from their ``PrincipalComponents``: the scores are the solution."""
    scale = float(deviation_scale)
    X = pc.scores if scale == 1.0 else (pc.scores * scale).contiguous()
    lam = pc.singular_values.double() ** 2 * scale ** 2
    total = pc.total_variance.double() * (max(n - 1, 1) * scale ** 2)
    return ClassicalMDS(X, lam, total, False)


def classical_mds(data=None, embedding_dim=2, *, distance_matrix=None, metric="euclidean", deviation_scale=1.0,
                  n_oversamples=10, n_iter=4, seed=0, test_matrix=None, device=None):
    """Classical (Torgerson) multidimensional scaling, R's ``cmdscale``: the ``embedding_dim`` leading eigenvectors
    of the double-centred matrix of squared deviations, as a ``ClassicalMDS``.  The minimiser of the STRAIN, the
    usual start of a stress minimisation (``DenseMDE(init="classical")``), and the baseline stress numbers are
    compared with.

    Exactly one source, prepared and checked as ``DenseMDE`` prepares its own: ``data`` [n, n_features], dense or
    sparse, under ``metric`` ``"euclidean"``, ``"cosine"`` or ``"correlation"``; or ``distance_matrix`` [n, n]
    (finite, non-negative, symmetric; the diagonal is never used).  ``deviation_scale`` multiplies every deviation.
    ``1 <= embedding_dim <= 8`` and ``embedding_dim + n_oversamples <= min(32, n - 1)``.

    Euclidean ``data`` take ``preprocess.principal_components`` (exact for dense data, randomized for sparse): its
    scores ARE the classical solution, and the eigenvalues are its squared singular values; ``embedding_dim`` must
    then be below ``min(n, n_features)``.  Everything else runs a randomized subspace iteration on ``B``: a start
    block [n, r], ``r = embedding_dim + n_oversamples`` -- standard normal from a ``torch.Generator`` on the device
    seeded with ``seed``, or ``test_matrix`` when given -- ``n_iter + 1`` rounds of one product with ``B``
    (``mde_pair_sqdist_apply``, O(n^2) pairs each, nothing n x n stored) and one orthonormalisation, and the r x r
    eigenproblem of the projected matrix on the host.  The iteration finds the eigenvalues of largest MAGNITUDE and
    keeps the algebraically largest of those; the same ``seed`` gives the same bits."""
    from pymde_amd import dense, quality                    # (dense imports this module)
    if (data is None) == (distance_matrix is None):
        raise ValueError("exactly one of `data` and `distance_matrix` must be given")
    deviation_scale = float(deviation_scale)
    if not (deviation_scale > 0.0 and np.isfinite(deviation_scale)):
        raise ValueError(f"deviation_scale must be a positive finite number, got {deviation_scale!r}")
    source = data if data is not None else distance_matrix
    if data is not None:
        metric = dense.check_source(data, metric)
        quality._check_matrix(data, "data")
    elif not hasattr(source, "shape") or len(source.shape) != 2 or int(source.shape[0]) != int(source.shape[1]):
        raise ValueError("`distance_matrix` must be a square matrix [n, n], got shape "
                         f"{tuple(getattr(source, 'shape', ()))}")
    n = int(source.shape[0])
    if n < 2:
        raise ValueError("classical scaling needs at least two items")
    d, r = check_arguments(n, embedding_dim, n_oversamples, n_iter)
    if data is not None and metric == _metrics.EUCLIDEAN:
        from pymde_amd.pca import principal_components
        try:
            pc = principal_components(data, d, n_oversamples=n_oversamples, n_iter=n_iter, seed=seed,
                                      test_matrix=test_matrix, device=device)
            return _from_scores(pc, n, deviation_scale)
        except util.SolverError:        # rows of rank below embedding_dim: the walk below returns zero columns
            test_matrix = None
    if device is None:
        device = source.device if isinstance(source, torch.Tensor) and source.is_cuda else util.get_default_device()
    device = util.require_cuda_device(device)
    with torch.no_grad(), torch.cuda.device(device):
        if data is not None:
            A, Dm, mode = quality._self_rows(data, metric, device, "data"), None, quality._pair_modes(metric)[0]
        else:
            A, mode = None, 0
            Dm = torch.as_tensor(distance_matrix).to(device=device, dtype=torch.float32).contiguous()
            dense._check_distance_matrix(Dm)
        return _scale(A, mode, Dm, deviation_scale, d, r, int(n_iter), seed, test_matrix)


def scale_problem(A, mode, Dm, deviation_scale, embedding_dim, n_oversamples=10, n_iter=4, seed=0, test_matrix=None):
    """The classical scaling of a dense problem's own prepared source (``DenseMDE._A`` / ``_mode`` / ``_Dm``).
    Euclidean rows with more features than dimensions go through their principal components, as in
    ``classical_mds``; the block is narrowed where ``n`` is small."""
    source = A if A is not None else Dm
    n, device = int(source.shape[0]), source.device
    d = int(embedding_dim)
    with torch.no_grad(), torch.cuda.device(device):
        if A is not None and mode == 0 and d < min(n, int(A.shape[1])):
            from pymde_amd.pca import principal_components
            try:
                return _from_scores(principal_components(A, d, device=device), n, deviation_scale)
            except util.SolverError:    # rows of rank below d: the walk below returns zero columns
                pass
        n_oversamples = max(0, min(int(n_oversamples), min(MAX_RANK, n - 1) - d))
        d_fit, r = check_arguments(n, min(d, n - 1), n_oversamples, n_iter)
        fit = _scale(A, mode, Dm, deviation_scale, d_fit, r, int(n_iter), seed, test_matrix)
        if d_fit < d:       # (fewer items than dimensions: the other columns are flat)
            pad = torch.zeros((n, d - d_fit), dtype=torch.float32, device=device)
            fit = ClassicalMDS(torch.cat([fit.X, pad], 1).contiguous(),
                               torch.cat([fit.eigenvalues, torch.zeros(d - d_fit, dtype=torch.float64,
                                                                       device=device)]), fit.total, fit.negative)
        return fit


def triangulate(X_old, *, Q=None, C=None, mode=0, Dm=None, deviation_scale=1.0):
    """Distance-based triangulation: float32 [n_new, d], the least-squares position of every new row from its
    squared deviations ``delta`` to ALL embedded rows ``X_old`` [n_old, d], in closed form.  The deviations come from
    prepared float32 tensors on one GPU: both ``Q`` [n_new, nf] and ``C`` [n_old, nf] (``mode`` as in
    ``sqdist_apply``), or ``Dm`` [n_new, n_old]; ``deviation_scale`` multiplies them.

    With ``m`` the mean of ``X_old``, ``L = X_old - m``, ``n2_j = |L_j|^2`` and ``P = pinv(L)^T`` [n_old, d]:
    ``x_new = m + pinv(L) n2 / 2 - (S_cross P) / 2``, where ``S_cross P`` is one rectangular
    ``mde_pair_sqdist_apply`` with ``r = d`` and everything else is O(n_old d) in float64.  ``pinv(L)`` is formed from
    the d x d Gram matrix ``L^T L`` with ``rcond = 1e-6``: embedded rows of rank below d (on a line in the plane)
    give a finite result whose null directions stay at ``m``'s.  Exact when the deviations are Euclidean and ``X_old``
    realises them."""
    gram = Q is not None and C is not None and Dm is None
    if not gram and not (Q is None and C is None and Dm is not None):
        raise ValueError("exactly one source of the deviations must be given: both `Q` and `C`, or `Dm` alone")
    if not hasattr(X_old, "shape") or len(X_old.shape) != 2 or not 1 <= int(X_old.shape[1]) <= MAX_DIM:
        raise ValueError(f"`X_old` must be the embedding [n_old, d] of the embedded rows, 1 <= d <= {MAX_DIM}, got "
                         f"shape {tuple(getattr(X_old, 'shape', ()))}")
    n_old = int(X_old.shape[0])
    if int((C if gram else Dm).shape[0 if gram else 1]) != n_old:
        raise ValueError(f"`X_old` must hold one embedding vector per embedded row ({n_old} given)")
    with torch.no_grad(), torch.cuda.device(X_old.device):
        X64 = X_old.detach().double()
        mean = X64.mean(0, keepdim=True)
        L = X64 - mean
        n2 = (L * L).sum(1)
        P = L @ torch.linalg.pinv(L.t() @ L, rcond=PINV_RCOND, hermitian=True)           # pinv(L)^T, [n_old, d]
        SP = sqdist_apply(P.to(torch.float32).contiguous(), Q=Q, C=C, mode=mode, Dm=Dm)   # [n_new, d]
        X_new = mean + 0.5 * (n2 @ P)[None, :] - (0.5 * float(deviation_scale) ** 2) * SP
        return X_new.to(torch.float32).contiguous()

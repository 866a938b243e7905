"""NumPy float64 references for the sparse product ``mde_csr_spmm`` and the principal components
(``pymde_amd/pca.py``), and the planted data they are tested on.  Nothing here touches a GPU."""
import numpy as np


def spmm(indptr, indices, values, B, u=None, v=None, with_scale=False):
    """``C[i, c] = sum_e values[e] * B[indices[e], c] - u[i] * v[c]`` in float64, row by row, a row's entries in
    ascending column order (the order of a canonical CSR).  ``u`` None: all ones; ``v`` None: no correction.
    ``with_scale``: also ``sum_e |values[e] B[indices[e], c]| + |u[i] v[c]|``, the scale of the summation error."""
    indptr = np.asarray(indptr, dtype=np.int64)
    B = np.asarray(B, dtype=np.float64)
    n, r = len(indptr) - 1, B.shape[1]
    C, S = np.zeros((n, r)), np.zeros((n, r))
    for i in range(n):
        for e in range(indptr[i], indptr[i + 1]):
            t = float(values[e]) * B[indices[e]]
            C[i] += t
            S[i] += np.abs(t)
    if v is not None:
        uv = np.outer(np.ones(n) if u is None else np.asarray(u, dtype=np.float64), np.asarray(v, dtype=np.float64))
        C -= uv
        S += np.abs(uv)
    return (C, S) if with_scale else C


def spmm_bound(want, scale):
    """The bound on ``|got - want|`` for a float32 result of float64 sums: one float32 rounding, plus a float64
    summation order that may differ across the segments of a long row."""
    return 2.0 ** -24 * np.abs(want) + 2.0 ** -40 * scale


def fix_signs(V):
    """Rows of ``V`` [m, nf], each oriented so that its entry of largest magnitude is positive."""
    top = np.abs(V).argmax(axis=1)
    return V * np.sign(V[np.arange(V.shape[0]), top])[:, None]


def _dense64(data):
    return np.asarray(data.toarray() if hasattr(data, "toarray") else data, dtype=np.float64)


def exact_pca(dense, m):
    """``(singular_values [m], components [m, nf], scores [n, m], mean [nf], all singular values)`` from
    ``np.linalg.svd`` of the centred matrix, components oriented by ``fix_signs``."""
    A = _dense64(dense)
    mean = A.mean(axis=0)
    Ac = A - mean
    _, s, Vt = np.linalg.svd(Ac, full_matrices=False)
    V = fix_signs(Vt[:m])
    return s[:m], V, Ac @ V.T, mean, s


def randomized_pca(data, m, test_matrix, n_iter):
    """Float64 replay of the randomized route of ``principal_components`` with the start block ``test_matrix``
    [nf, r]: ``(singular_values [m], components [m, nf], scores [n, m], mean [nf])``.  The result does not depend
    on which orthonormal basis of a block's span is taken, so ``orth`` is a QR factorisation here."""
    A = _dense64(data)
    mean = A.mean(axis=0)
    Ac = A - mean

    def orth(S):
        return np.linalg.qr(S)[0]

    Q = orth(Ac @ np.asarray(test_matrix, dtype=np.float64))
    for _ in range(n_iter):
        Z = orth(Ac.T @ Q)
        Q = orth(Ac @ Z)
    B = Ac.T @ Q
    evals, W = np.linalg.eigh(B.T @ B)
    order = np.argsort(evals)[::-1][:m]
    sing = np.sqrt(evals[order])
    V = fix_signs((B @ W[:, order] / sing[None, :]).T)
    return sing, V, Ac @ V.T, mean


def principal_sines(V, W):
    """Sines of the principal angles between the row spaces of ``V`` and ``W`` (orthonormal rows, [m, nf]),
    descending: the singular values of ``(I - V^T V) W^T``."""
    V, W = np.asarray(V, dtype=np.float64), np.asarray(W, dtype=np.float64)
    return np.linalg.svd(W.T - V.T @ (V @ W.T), compute_uv=False)


def planted(n=600, nf=900, groups=9, seed=0):
    """Sparse data with ``groups - 1`` strong principal directions, as a float32 ``scipy.sparse.csr_matrix``: the
    rows are dealt to ``groups`` groups, each of which owns ``nf // groups`` columns; a row is non-zero on half
    (Bernoulli 0.5) of its group's columns, with values ``N(3, 0.5) * (1 + 0.15 g)``; a 2 % background of
    ``N(0, 1)`` lies over everything.  Density about 0.074 at the defaults."""
    import scipy.sparse
    rng = np.random.default_rng(seed)
    width = nf // groups
    g = rng.integers(0, groups, n)
    A = np.zeros((n, nf))
    for i in range(n):
        on = rng.random(width) < 0.5
        A[i, g[i] * width:(g[i] + 1) * width] = on * rng.normal(3.0, 0.5, width) * (1.0 + 0.15 * g[i])
    A += (rng.random((n, nf)) < 0.02) * rng.standard_normal((n, nf))
    return scipy.sparse.csr_matrix(A.astype(np.float32))


def start_block(nf, r, seed=0):
    """A fixed standard-normal start block [nf, r] (float32) for the device and the replay alike."""
    return np.random.default_rng(seed).standard_normal((nf, r)).astype(np.float32)

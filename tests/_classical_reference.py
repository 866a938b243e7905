"""Float64 NumPy restatement of ``pymde_amd.classical``; no device.

``S`` is the dense matrix of squared deviations with a zero diagonal, ``B = -1/2 J S J``.  ``classical_exact`` is
classical MDS by a full ``eigh``; ``replay`` is the randomized subspace iteration the device runs, from a given start
block; ``triangulate`` the closed-form placement; the rest are the planted inputs the tests share.
"""
import numpy as np

NOISE_RTOL = 1e-6
PINV_RCOND = 1e-6


# ---------------------------------------------------------------------------------------------------------- S and B
def unit_rows(X, metric="cosine"):
    X = np.asarray(X, dtype=np.float64)
    if metric == "correlation":
        X = X - X.mean(1, keepdims=True)
    return X / np.linalg.norm(X, axis=1, keepdims=True)


def d2_rows(Q, C):
    """|q_i - c_j|^2 in float64, in difference form."""
    Q, C = np.asarray(Q, dtype=np.float64), np.asarray(C, dtype=np.float64)
    diff = Q[:, None, :] - C[None, :, :]
    return np.einsum("ijk,ijk->ij", diff, diff)


def S_cross(Q, C, mode=0):
    """The squared deviations of prepared rows: ``d2`` (mode 0), ``(d2 / 2)^2`` (mode 1: unit rows)."""
    d2 = d2_rows(Q, C)
    return d2 if mode == 0 else (0.5 * d2) ** 2


def S_from_rows(A, mode=0):
    S = S_cross(A, A, mode)
    np.fill_diagonal(S, 0.0)
    return S


def S_from_matrix(D):
    S = np.asarray(D, dtype=np.float64) ** 2
    if S.shape[0] == S.shape[1]:
        np.fill_diagonal(S, 0.0)
    return S


def B_matrix(S):
    n = S.shape[0]
    J = np.eye(n) - np.ones((n, n)) / n
    return -0.5 * J @ S @ J


def apply_B(S, V):
    """``B V`` the way the device forms it: ``S V - s m^T`` with ``s = S 1`` and ``m`` the column means of ``V``,
    centred, times -1/2."""
    V = np.asarray(V, dtype=np.float64)
    Y = S @ V - np.outer(S.sum(1), V.mean(0))
    return -0.5 * (Y - Y.mean(0, keepdims=True))


# ------------------------------------------------------------------------------------------------------ classical MDS
def _orient(X):
    top = np.abs(X).argmax(0)
    sign = np.sign(X[top, np.arange(X.shape[1])])
    return X * np.where(sign == 0, 1.0, sign)[None, :]


def _kept(evals, vecs, d):
    order = np.argsort(evals)[::-1][:d]
    lam = evals[order]
    floor = NOISE_RTOL * max(lam[0], 0.0)
    negative = bool(np.any(lam < -floor))
    lam = np.where(lam > floor, lam, 0.0)
    return vecs[:, order], lam, negative


def classical_exact(S, d):
    """``(X [n, d], eigenvalues [d] clipped, negative, all eigenvalues ascending)`` by ``eigh`` of ``B``."""
    evals, vecs = np.linalg.eigh(B_matrix(S))
    U, lam, negative = _kept(evals, vecs, d)
    return _orient(U * np.sqrt(lam)[None, :]), lam, negative, evals


def replay(S, omega, d, n_iter=4):
    """The randomized subspace iteration from the start block ``omega`` [n, r], in float64: ``(X, eigenvalues,
    negative, Q)`` with ``Q`` the final orthonormal block."""
    Q = np.linalg.qr(apply_B(S, omega))[0]
    for _ in range(n_iter):
        Q = np.linalg.qr(apply_B(S, Q))[0]
    T = Q.T @ apply_B(S, Q)
    evals, Z = np.linalg.eigh(0.5 * (T + T.T))
    Zk, lam, negative = _kept(evals, Z, d)
    X = Q @ (Zk * np.sqrt(lam)[None, :])
    return _orient(X - X.mean(0, keepdims=True)), lam, negative, Q


def principal_sines(U, V):
    """The sines of the principal angles between the column spaces of ``U`` and ``V`` (descending)."""
    U, V = np.linalg.qr(U)[0], np.linalg.qr(V)[0]
    return np.linalg.svd(V - U @ (U.T @ V), compute_uv=False)


def gram_gap(X, Y):
    """max |X X^T - Y Y^T| / max |Y Y^T|: two configurations compared up to rotation and reflection."""
    G = Y @ Y.T
    return float(np.abs(X @ X.T - G).max() / np.abs(G).max())


def pair_distances(X):
    return np.sqrt(d2_rows(X, X))


# ------------------------------------------------------------------------------------------------------ triangulation
def triangulate(X_old, delta):
    """``x_new = m + pinv(L) n2 / 2 - delta P / 2`` for the squared deviations ``delta`` [n_new, n_old]."""
    X_old = np.asarray(X_old, dtype=np.float64)
    mean = X_old.mean(0, keepdims=True)
    L = X_old - mean
    n2 = (L * L).sum(1)
    P = L @ np.linalg.pinv(L.T @ L, rcond=PINV_RCOND, hermitian=True)
    return mean + 0.5 * (n2 @ P)[None, :] - 0.5 * (np.asarray(delta, dtype=np.float64) @ P), P


# -------------------------------------------------------------------------------------------------------- the inputs
def planted_rows(n=300, nf=40, seed=0):
    """A 3-D structure (axes of spread 27, 18, 10) in ``nf`` features plus noise of spread 0.4, as float32: the
    eigenvalues of ``B`` are about n times 729, 324, 100 and then n times 0.16."""
    rng = np.random.default_rng(seed)
    Z = rng.standard_normal((n, 3)) * np.array([27.0, 18.0, 10.0])
    W = np.linalg.qr(rng.standard_normal((nf, 3)))[0]
    return (Z @ W.T + 0.4 * rng.standard_normal((n, nf))).astype(np.float32)


def planted_cosine_rows(n=300, nf=40, seed=0):
    """The planted rows shifted by +2, for the cosine distance: its ``B`` is indefinite."""
    return (planted_rows(n, nf, seed) + 2.0).astype(np.float32)


def cycle_matrix(n):
    """The shortest-path lengths of the n-cycle."""
    i = np.arange(n)
    gap = np.abs(i[:, None] - i[None, :])
    return np.minimum(gap, n - gap).astype(np.float32)


def points(n, d, seed=0, spread=1.0):
    return np.random.default_rng(seed).standard_normal((n, d)) * spread


def isometry(dim, nf, seed=0):
    """[dim, nf] with orthonormal rows: ``P @ isometry`` maps R^dim isometrically into nf features."""
    return np.linalg.qr(np.random.default_rng(seed).standard_normal((nf, dim)))[0].T


def rotation(d, seed=0):
    return np.linalg.qr(np.random.default_rng(seed).standard_normal((d, d)))[0]

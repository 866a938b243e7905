"""Inputs of the bfloat16 k-NN tests and a CPU emulation of the bfloat16 shortlist, shared by
test_knn_bf16_host.py (which asserts that the inputs leave the shortlist a margin) and test_gpu_knn_bf16.py
(which asserts that the GPU result is then the float32 result)."""
import functools

import numpy as np
import torch

from pymde_amd import metrics, preprocess

GENERATORS = ("gauss", "offset", "mixture", "uniform", "ints")
SELF_SHAPES = [(1037, 50, 15), (3001, 784, 15), (130, 3, 10), (65, 130, 7), (2000, 64, 32)]     # (n, nf, k)
CROSS_SHAPES = [(65, 1037, 50, 15), (70, 4101, 784, 15)]                                        # (n_q, n_c, nf, k), mixture
MARGIN = 8          # places a true neighbour must sit inside the shortlist


@functools.lru_cache(maxsize=None)
def make(kind, n, nf):
    """The float32 [n, nf] input `kind`, read-only."""
    if kind in ("gauss", "offset"):
        X = np.random.default_rng(n).standard_normal((n, nf))
        if kind == "offset":
            X = X + 1000
    elif kind == "mixture":
        r = np.random.default_rng(1)
        cen = r.standard_normal((10, nf))
        lab = r.integers(0, 10, n)
        X = cen[lab] + 0.3 * r.standard_normal((n, nf))
    elif kind == "uniform":
        X = np.random.default_rng(n + 1).random((n, nf))
    elif kind == "ints":
        X = np.random.default_rng(n + 2).integers(0, 4, (n, nf))
    else:
        raise KeyError(kind)
    X = X.astype(np.float32)
    X.setflags(write=False)
    return X


def cross_pair(kind, n_q, n_c, nf):
    """(queries, corpus): the first n_q and the other n_c rows of make(kind, n_q + n_c, nf)."""
    X = make(kind, n_q + n_c, nf)
    return X[:n_q], X[n_q:]


def bf16_points(Q, C):
    """The points the bfloat16 shortlist ranks, as float64 arrays: both matrices minus the grid column means of
    the corpus C (subtracted in double, rounded to float32, then to bfloat16 on the CPU)."""
    C64 = np.asarray(C, dtype=np.float64)
    mu = metrics.grid_means(torch.tensor(C64.mean(0)), torch.tensor(C64.var(0))).numpy()

    def rounded(X):
        t = torch.tensor((np.asarray(X, dtype=np.float64) - mu).astype(np.float32))
        return t.to(torch.bfloat16).to(torch.float64).numpy()
    return rounded(Q), rounded(C)


def _ranked(D, self_join):
    """Column order of every row of D by (distance, index), the row's own column dropped for a self-join."""
    if self_join:
        D = D.copy()
        np.fill_diagonal(D, np.inf)
    order = np.argsort(D, axis=1, kind="stable")
    return order[:, :-1] if self_join else order


def _sqdist(A, B):
    return (A * A).sum(1)[:, None] + (B * B).sum(1)[None, :] - 2.0 * (A @ B.T)


def worst_place(Q, C, k, self_join):
    """The worst (largest, 1-based) place in the bfloat16 ranking of a row's candidates that any of the row's k
    float64 true neighbours takes, over all rows."""
    Q64, C64 = np.asarray(Q, dtype=np.float64), np.asarray(C, dtype=np.float64)
    # distances are translation invariant and centring keeps float64 accurate; integer means keep integer data
    # (and so their ties) exact
    m = np.round(C64.mean(0))
    true = _ranked(_sqdist(Q64 - m, C64 - m), self_join)[:, :k]
    Qb, Cb = bf16_points(Q, C)
    short = _ranked(_sqdist(Qb, Cb), self_join)
    place = np.empty(short.shape, dtype=np.int64)
    rows = np.arange(short.shape[0])[:, None]
    place[rows, short - (short > rows if self_join else 0)] = np.arange(1, short.shape[1] + 1)[None, :]
    cols = true - (true > rows if self_join else 0)      # column ids with the row's own column squeezed out
    return int(place[rows, cols].max())


def shortlist_is_safe(Q, C, k, self_join, n_candidates=None):
    """True when every float64 true neighbour sits at least MARGIN places inside the shortlist (or the
    shortlist holds every candidate there is)."""
    available = int(np.asarray(C).shape[0]) - (1 if self_join else 0)
    k = min(k, available)
    if k < 1:
        return True
    n_cand = preprocess.default_n_candidates(k, available) if n_candidates is None else n_candidates
    if n_cand >= available:
        return True
    return worst_place(Q, C, k, self_join) <= n_cand - MARGIN

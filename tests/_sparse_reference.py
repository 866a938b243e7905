"""Inputs and float64 references for the sparse kernels (csrc/mde_sparse.hip).  numpy and scipy only: no
torch, no GPU.

The sparse k-NN kernel walks a row's stored entries one window of ``W`` feature columns at a time, 64 entries
per step, so what can go wrong depends on how many entries a row has inside one window and where they sit
relative to the window seams.  ``structured_rows`` builds a matrix whose rows cycle through those cases for a
given ``W`` (the caller takes ``W`` from the library: nothing here knows the rule that chooses it), with
integer values so that every float32 sum is exact and the kernel's lists can be compared bit for bit.
"""
import numpy as np
import scipy.sparse as sp

FLT_MAX = float(np.finfo(np.float32).max)

# The row patterns, in the order the rows cycle through them.  The two that a search must contain to take a
# second 64-entry step come first, so that even a two-row matrix has them.
PATTERNS = ("in65", "in64", "empty", "one", "in63", "in127", "in128", "in129", "full_window", "two_full_windows",
            "dense", "seams", "last_window", "in64_then_1", "long", "copy", "disjoint_a", "disjoint_b")
_IN_ONE_WINDOW = {"in63": 63, "in64": 64, "in65": 65, "in127": 127, "in128": 128, "in129": 129}


def n_windows(nf, W):
    return (nf + W - 1) // W


def structured_rows(n, nf, W, seed):
    """``(A, pattern, partner)``: a CSR [n, nf] (float32, integer values in [1, 5]) whose row ``r`` follows
    ``pattern[r] = PATTERNS[r % len(PATTERNS)]`` for windows of ``W`` columns:

    - ``empty``, ``one``: no entry, one entry;
    - ``in63`` .. ``in129``: exactly that many entries, all inside one window (at most the window's width);
    - ``full_window``, ``two_full_windows``: every column of one window, of two adjacent windows;
    - ``dense``: every column;
    - ``seams``: columns ``w0``, ``w0 + W - 1`` and ``w0 + W`` only;
    - ``last_window``: every column of the last window (a partial one when ``W`` does not divide ``nf``);
    - ``in64_then_1``: 64 entries in one window and one in the next (none where there is no next window);
    - ``long``: about three quarters of all columns; ``copy``: the values and columns of the ``long`` row that is
      farthest away by row index (of the farthest row of any other pattern where there is no ``long`` row);
    - ``disjoint_a``, ``disjoint_b``: the even columns, the odd columns.

    The window of a pattern moves on by one from one cycle to the next, over the windows of full width where
    there are any.  ``partner[r]`` is the row that a ``copy`` row repeats and the other row of a disjoint pair
    (-1 elsewhere, and where the partner lies past the last row)."""
    rng = np.random.default_rng(seed)
    L = len(PATTERNS)
    nwin, nfull = n_windows(nf, W), nf // W
    pattern = np.array([PATTERNS[r % L] for r in range(n)])
    partner = np.full(n, -1, dtype=np.int64)
    cols = [np.zeros(0, dtype=np.int64)] * n

    def window(win):
        return win * W, min(win * W + W, nf)

    def pick(win, m):
        lo, hi = window(win)
        return np.sort(rng.choice(np.arange(lo, hi), size=min(m, hi - lo), replace=False))

    for r in range(n):
        what, cycle = pattern[r], r // L
        win = cycle % nfull if nfull else 0                 # a window of full width where there is one
        lo, hi = window(win)
        if what == "one":
            c = rng.integers(0, nf, 1)
        elif what in _IN_ONE_WINDOW:
            c = pick(win, _IN_ONE_WINDOW[what])
        elif what == "full_window":
            c = np.arange(lo, hi)
        elif what == "two_full_windows":
            win = cycle % max(nfull - 1, 1)
            c = np.arange(win * W, min((win + 2) * W, nf))
        elif what == "dense":
            c = np.arange(nf)
        elif what == "seams":
            win = cycle % max(nwin - 1, 1)
            c = np.array([s for s in (win * W, win * W + W - 1, win * W + W) if s < nf])
        elif what == "last_window":
            c = np.arange((nwin - 1) * W, nf)
        elif what == "in64_then_1":
            win = cycle % max(nfull if nfull < nwin else nwin - 1, 1)
            c = pick(win, 64)
            if win + 1 < nwin:
                c = np.concatenate([c, pick(win + 1, 1)])
        elif what == "long":
            c = np.flatnonzero(rng.random(nf) < 0.75)
        elif what == "disjoint_a":
            c = np.arange(0, nf, 2)
            partner[r] = r + 1 if r + 1 < n else -1
        elif what == "disjoint_b":
            c = np.arange(1, nf, 2)
            partner[r] = r - 1
        else:                                               # empty, and copy (filled in below)
            c = np.zeros(0, dtype=np.int64)
        cols[r] = np.asarray(c, dtype=np.int64)
    vals = [rng.integers(1, 6, len(c)).astype(np.float32) for c in cols]
    for r in np.flatnonzero(pattern == "copy"):
        source = np.flatnonzero(pattern == "long")
        if len(source) == 0:
            source = np.flatnonzero(pattern != "copy")
        partner[r] = source[np.argmax(np.abs(source - r))]
        cols[r], vals[r] = cols[partner[r]].copy(), vals[partner[r]].copy()
    indptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum([len(c) for c in cols], out=indptr[1:])
    A = sp.csr_matrix((np.concatenate(vals) if indptr[-1] else np.zeros(0, dtype=np.float32),
                       np.concatenate(cols) if indptr[-1] else np.zeros(0, dtype=np.int64), indptr), shape=(n, nf))
    return A, pattern, partner


def accuracy_rows(n, nf, seed, lengths=(5, 70, 300), delta=1e-3):
    """``(A, length)``: a CSR [n, nf] of float32 values uniform in [0.5, 2).  The first ``n // 2`` rows have
    ``lengths[r % 3]`` entries at random columns; row ``n // 2 + r`` is the twin of row ``r``, the same row
    with ``delta`` added to its first entry.  ``length[r]`` is the number of entries of row ``r``."""
    rng = np.random.default_rng(seed)
    half = n // 2
    cols = [np.sort(rng.choice(nf, size=lengths[r % len(lengths)], replace=False)) for r in range(half)]
    vals = [rng.uniform(0.5, 2.0, len(c)).astype(np.float32) for c in cols]
    twin = [v.copy() for v in vals]
    for v in twin:
        v[0] += np.float32(delta)
    length = np.array([len(c) for c in cols] * 2)
    indptr = np.zeros(2 * half + 1, dtype=np.int64)
    np.cumsum(length, out=indptr[1:])
    A = sp.csr_matrix((np.concatenate(vals + twin), np.concatenate(cols + cols), indptr), shape=(2 * half, nf))
    return A, length


def window_counts(A, W):
    """int64 [n, number of windows]: the stored entries of every row of the CSR ``A`` inside each window of
    ``W`` columns."""
    A = sp.csr_matrix(A)
    n, nf = A.shape
    counts = np.zeros((n, n_windows(nf, W)), dtype=np.int64)
    rows = np.repeat(np.arange(n), np.diff(A.indptr))
    np.add.at(counts, (rows, A.indices // W), 1)
    return counts


def _dense64(A):
    return np.asarray(sp.csr_matrix(A).toarray(), dtype=np.float64)


def squared_distances(A):
    """float64 [n, n]: squared Euclidean distances of the rows of ``A``, summed over squared differences."""
    X = _dense64(A)
    return np.stack([((X - x) ** 2).sum(1) for x in X])


def knn_lists(A, k):
    """``(idx int64 [n, k], d2 float64 [n, k])``: for every row the ``k`` other rows nearest to it, ordered by
    ``(d2, index)``, the squared distances from differences in float64.  Where fewer than ``k`` other rows
    exist the remaining slots hold -1 and ``FLT_MAX``, what ``mde_sparse_knn`` writes there."""
    D = squared_distances(A)
    n = D.shape[0]
    np.fill_diagonal(D, np.inf)
    order = np.argsort(D, axis=1, kind="stable")[:, :min(k, n - 1)]      # stable: ties to the smaller index
    idx = np.full((n, k), -1, dtype=np.int64)
    d2 = np.full((n, k), FLT_MAX, dtype=np.float64)
    idx[:, :order.shape[1]] = order
    d2[:, :order.shape[1]] = np.take_along_axis(D, order, 1)
    return idx, d2


def pair_distances(A, edges):
    """float64 [p]: the Euclidean distance of rows ``edges[:, 0]`` and ``edges[:, 1]``, from differences."""
    X = _dense64(A)
    edges = np.asarray(edges, dtype=np.int64)
    return np.sqrt(((X[edges[:, 0]] - X[edges[:, 1]]) ** 2).sum(1))


def emulate_float32_d2(A):
    """float32 [n, n]: ``max(|q|^2 + |c|^2 - 2 q.c, 0)`` as float32 arithmetic gives it when every sum runs
    over the stored entries in column order, one rounding per product and one per addition.  It is here only
    to show, without the kernel, that an input stays inside its bound."""
    X = np.asarray(sp.csr_matrix(A).toarray(), dtype=np.float32)
    n, nf = X.shape
    dot = np.zeros((n, n), dtype=np.float32)
    sq = np.zeros(n, dtype=np.float32)
    for f in range(nf):                      # adding the zero of an absent entry changes nothing
        x = X[:, f]
        dot += x[:, None] * x[None, :]
        sq += x * x
    return np.maximum((sq[:, None] + sq[None, :]) - np.float32(2.0) * dot, np.float32(0.0))


def check_lists(label, idx, d2, A, rtol, stol):
    """Neighbour lists ``idx [n, k]``, ``d2 [n, k]`` of a self-join on the rows of ``A`` against float64: no
    self match, no id twice, distances ascending, every listed ``d2`` within ``rtol * true + stol * (|x|^2 +
    |y|^2)`` of the float64 squared distance of the listed id, and the k-th listed distance not above the
    true k-th by more than the same bound.  Ids are never compared.  Returns ``err / (|x|^2 + |y|^2)`` of
    every listed entry [n, k]."""
    idx, d2 = np.asarray(idx, dtype=np.int64), np.asarray(d2, dtype=np.float64)
    n, k = idx.shape
    D = squared_distances(A)
    sq = (_dense64(A) ** 2).sum(1)
    rows = np.arange(n)
    assert (idx >= 0).all() and (idx < n).all(), label
    assert not (idx == rows[:, None]).any(), label
    srt = np.sort(idx, axis=1)
    assert not (srt[:, 1:] == srt[:, :-1]).any(), label
    assert (d2[:, 1:] >= d2[:, :-1]).all(), label
    true = np.take_along_axis(D, idx, 1)
    scale = sq[:, None] + sq[idx]
    assert (scale > 0).all(), label
    tol = rtol * true + stol * scale
    err = np.abs(d2 - true)
    print("%s k=%d: max listed err / scale %.3e (bound %.1e + %.0e true / scale), max err / tol %.3f"
          % (label, k, (err / scale).max(), stol, rtol, (err / tol).max()))
    assert (err <= tol).all(), (label, k, float((err / scale).max()), float((err / tol).max()))
    np.fill_diagonal(D, np.inf)
    kid = np.argsort(D, axis=1, kind="stable")[:, k - 1]
    kth = D[rows, kid]
    tol_k = rtol * kth + stol * (sq + sq[kid])
    assert (d2[:, -1] <= kth + tol_k).all(), (label, k, float(((d2[:, -1] - kth) / tol_k).max()))
    return err / scale

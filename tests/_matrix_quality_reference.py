"""Float64 numpy brute force of the three kernels of csrc/mde_matrix_quality.hip (no GPU, no torch): the sums over
the counted pairs of a dissimilarity matrix against an embedding, the Shepard counts with the kernels' float32 bin
formula, and the ranks within the columns under the (value, index) order."""
import numpy as np

FLT_MAX = float(np.finfo(np.float32).max)


def _items(n, m, items):
    if items is None:
        assert m == n
        return np.arange(n)
    items = np.asarray(items, dtype=np.int64)
    assert items.shape == (m,) and items.min() >= 0 and items.max() < n
    return items


def counted(Dm, items=None):
    """Boolean [n, m]: pair (i, b) counts unless items[b] == i or Dm[i, b] is not finite or is FLT_MAX."""
    Dm = np.asarray(Dm, dtype=np.float32)
    n, m = Dm.shape
    items = _items(n, m, items)
    return (np.arange(n)[:, None] != items[None, :]) & (np.abs(Dm.astype(np.float64)) < FLT_MAX)


def embedding_distances(X, items):
    """E [n, m] in float64 from the float32 coordinates."""
    X = np.asarray(X, dtype=np.float32).astype(np.float64)
    diff = X[:, None, :] - X[None, np.asarray(items), :]
    return np.sqrt((diff * diff).sum(axis=2))


def moments(Dm, X, items=None):
    """``(row_sums [n, 5], row_count [n], row_max [n, 2], totals [8])`` as mde_matrix_moments defines them, in
    float64: the sums of D, E, D^2, E^2, D E over every row's counted pairs, the count, the largest D and E (0
    without a counted pair), and the totals ``sum D, E, D^2, E^2, D E, max D, max E, count``."""
    Dm = np.asarray(Dm, dtype=np.float32)
    n, m = Dm.shape
    items = _items(n, m, items)
    keep = counted(Dm, items)
    D = np.where(keep, Dm.astype(np.float64), 0.0)
    E = np.where(keep, embedding_distances(X, items), 0.0)
    row_sums = np.stack([D.sum(1), E.sum(1), (D * D).sum(1), (E * E).sum(1), (D * E).sum(1)], axis=1)
    row_count = keep.sum(axis=1).astype(np.int64)
    row_max = np.stack([D.max(axis=1), E.max(axis=1)], axis=1)
    totals = np.concatenate([row_sums.sum(axis=0), row_max.max(axis=0), [float(row_count.sum())]])
    return row_sums, row_count, row_max, totals


def histogram(Dm, X, items, bins, d_range, e_range):
    """int64 [bins, bins]: every counted pair with d_lo <= D <= d_hi and e_lo <= E <= e_hi adds one to
    ``[min(bins - 1, int((D - d_lo) * s_d)), min(bins - 1, int((E - e_lo) * s_e))]`` with ``s = float32(bins) /
    (hi - lo)``, every operation in float32 as the kernel's; E is rounded to float32 from float64 (exact inputs
    only: an integer grid)."""
    Dm = np.asarray(Dm, dtype=np.float32)
    n, m = Dm.shape
    items = _items(n, m, items)
    keep = counted(Dm, items)
    E = embedding_distances(X, items).astype(np.float32)
    f = np.float32
    d_lo, d_hi, e_lo, e_hi = f(d_range[0]), f(d_range[1]), f(e_range[0]), f(e_range[1])
    s_d, s_e = f(bins) / (d_hi - d_lo), f(bins) / (e_hi - e_lo)
    counts = np.zeros((bins, bins), dtype=np.int64)
    for i in range(n):
        for b in range(m):
            D, e = Dm[i, b], E[i, b]
            if keep[i, b] and d_lo <= D <= d_hi and e_lo <= e <= e_hi:
                bd = min(bins - 1, int(f(D - d_lo) * s_d))
                be = min(bins - 1, int(f(e - e_lo) * s_e))
                counts[bd, be] += 1
    return counts


def ranks(Dm, idx, items=None):
    """int32 [m, k]: ``ranks[b, c]`` = the number of items j != items[b] with (Dm[j, b], j) < (Dm[l, b], l) for
    l = idx[b, c]; -1 for an entry that is negative, >= n or the column's own item.  +inf is an ordinary value."""
    Dm = np.asarray(Dm, dtype=np.float32)
    idx = np.asarray(idx, dtype=np.int64)
    n, m = Dm.shape
    items = _items(n, m, items)
    out = np.full(idx.shape, -1, dtype=np.int32)
    for b in range(m):
        col = Dm[:, b].astype(np.float64)
        order = [j for j in np.lexsort((np.arange(n), col)) if j != items[b]]     # by value, then by index
        position = {int(j): r for r, j in enumerate(order)}
        for c, l in enumerate(idx[b]):
            if 0 <= l < n and l != items[b]:
                out[b, c] = position[int(l)]
    return out


def sampled_score(ranks_, n, k):
    """``1 - 2 / (m k (2 n - 3 k - 1)) * sum max(0, rank + 1 - k)`` over the m rows of ``ranks_`` [m, k]."""
    r = np.asarray(ranks_, dtype=np.int64)
    m = r.shape[0]
    return 1.0 - 2.0 / (m * k * (2.0 * n - 3.0 * k - 1.0)) * float(np.maximum(r + 1 - k, 0).sum())

"""A numpy restatement of one neighbour-of-neighbour pass over k-NN lists, for the tests
of pymde_amd.ann.refine_lists.  Lists are idx int [n, k] with -1 for an empty slot and d2 [n, k]; the pair
distances come from the caller: ``pair_d2(i, cand)`` returns the squared distances of row i to the rows
``cand`` (an int array) in whatever number format the caller compares in."""
import numpy as np

FLT_MAX = np.float32(3.402823466e+38)


def reverse_lists(idx, d2, cap=None):
    """int32 [n, cap]: for every row t the ``cap`` (default k) rows j listing t with the smallest (d2(j, t), j),
    in that order, -1 padded: a lexicographic sort of the entries on (target, d2, source)."""
    n, k = idx.shape
    cap = k if cap is None else cap
    source = np.repeat(np.arange(n), k)
    target = idx.reshape(-1)
    dist = np.asarray(d2).reshape(-1)
    listed = target >= 0
    source, target, dist = source[listed], target[listed], dist[listed]
    order = np.lexsort((source, dist, target))            # the last key is the primary one
    rev = np.full((n, cap), -1, dtype=np.int32)
    filled = np.zeros(n, dtype=np.int64)
    for e in order:
        t = target[e]
        if filled[t] < cap:
            rev[t, filled[t]] = source[e]
            filled[t] += 1
    return rev


def candidates(i, idx, rev):
    """The distinct candidate rows of row i: its reverse neighbours and the lists of its forward and reverse
    neighbours, without i itself and without the rows it already lists."""
    mine = idx[i][idx[i] >= 0]
    back = rev[i][rev[i] >= 0]
    joins = np.concatenate([mine, back])
    cand = np.concatenate([back] + [idx[j] for j in joins]) if joins.size else back
    cand = np.unique(cand[cand >= 0])
    return cand[(cand != i) & ~np.isin(cand, mine)]


def top_k(ids, dist, k, dtype):
    """The k smallest of (dist, ids) under (d2, index) as (idx [k] with -1 padding, d2 [k] with FLT_MAX)."""
    order = np.lexsort((ids, dist))[:k]
    out_i = np.full(k, -1, dtype=np.int32)
    out_d = np.full(k, FLT_MAX, dtype=dtype)
    out_i[:order.size] = ids[order]
    out_d[:order.size] = dist[order]
    return out_i, out_d


def refine_pass(idx, d2, pair_d2, rev=None):
    """One pass: (idx, d2, number of rows whose list changed).  Reads the old lists only (Jacobi)."""
    n, k = idx.shape
    d2 = np.asarray(d2)
    rev = reverse_lists(idx, d2) if rev is None else rev
    new_i = np.empty((n, k), dtype=np.int32)
    new_d = np.empty((n, k), dtype=d2.dtype)
    changed = 0
    for i in range(n):
        have = idx[i] >= 0
        cand = candidates(i, idx, rev)
        ids = np.concatenate([idx[i][have], cand])
        dist = np.concatenate([d2[i][have], np.asarray(pair_d2(i, cand), dtype=d2.dtype).reshape(-1)])
        new_i[i], new_d[i] = top_k(ids, dist, k, d2.dtype)
        changed += int(not np.array_equal(new_i[i], np.where(have, idx[i], -1)))
    return new_i, new_d, changed

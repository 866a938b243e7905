"""NumPy reference of the binary distances of pymde_amd.binary (csrc/mde_bits.hip): the intersection counts by an
int64 matrix product, the value of a pair as one float32 division of exact integers, neighbour lists by a stable
lexicographic sort on (float32 value, index).  With a, b the row counts and t the intersection:
Hamming (a + b - 2 t) / nf; Jaccard (a + b - 2 t) / (a + b - t), 0 where a + b - t == 0."""
import numpy as np


def make_bits(n, nf, p, seed=0, clear=(3, 5)):
    """The test data of the k-NN tests: random bits of density p with the rows `clear` emptied."""
    B = np.random.default_rng(seed).random((n, nf)) < p
    for r in clear:
        if r < n:
            B[r] = False
    return B


def cross_distances(Q, C, distance):
    """float32 [n_q, n_c]: the distance of every row of the bool matrix Q to every row of C."""
    Q, C = np.asarray(Q, dtype=bool), np.asarray(C, dtype=bool)
    nf = Q.shape[1]
    t = Q.astype(np.int64) @ C.astype(np.int64).T
    a = Q.sum(1, dtype=np.int64)[:, None]
    b = C.sum(1, dtype=np.int64)[None, :]
    num = a + b - 2 * t
    if distance == "hamming":
        den = np.full_like(num, nf)
    elif distance == "jaccard":
        den = a + b - t
    else:
        raise ValueError(distance)
    safe = np.where(den == 0, 1, den)
    d = np.float32(num) / np.float32(safe)
    return np.where(den == 0, np.float32(0.0), d).astype(np.float32)


def _lists(D, k):
    n_q, n_c = D.shape
    idx = np.full((n_q, k), -1, dtype=np.int64)
    val = np.full((n_q, k), np.inf, dtype=np.float32)
    cols = np.arange(n_c)
    for i in range(n_q):
        ok = np.isfinite(D[i])
        order = np.lexsort((cols[ok], D[i][ok]))[:k]       # by value, then index: a stable order
        idx[i, :order.size] = cols[ok][order]
        val[i, :order.size] = D[i][ok][order]
    return idx, val


def knn_lists(B, k, distance):
    """(idx int64 [n, k], values float32 [n, k]) of the self-join: a row does not list itself (by index; a duplicate
    row is listed at 0); -1 / inf where fewer than k other rows exist."""
    D = cross_distances(B, B, distance)
    np.fill_diagonal(D, np.inf)
    return _lists(D, k)


def cross_lists(Q, C, k, distance):
    """The same for queries against a corpus, nothing excluded."""
    return _lists(cross_distances(Q, C, distance), k)


def edge_set(idx, val=None, max_distance=None):
    """The undirected edges {(i, j), i < j} of directed lists, entries above max_distance dropped."""
    out = set()
    for i in range(idx.shape[0]):
        for c in range(idx.shape[1]):
            j = int(idx[i, c])
            if j < 0 or (max_distance is not None and not val[i, c] <= max_distance):
                continue
            out.add((min(i, j), max(i, j)))
    return out

"""float64 references for the graph kernels of csrc/mde_graph.hip (no GPU): scipy Dijkstra / BFS rows from chosen
sources, what ``shortest_paths`` and the k-NN lists must hold for such a source, and a ``numpy.uint64`` replay of the
hash that decides which pairs ``retain_fraction`` keeps."""
import numpy as np
import scipy.sparse as sp
import scipy.sparse.csgraph as cs

FLT_MAX = np.float32(3.4028235e38)     # what an empty slot of a distance list holds


def adjacency(n, edges, weights=None):
    """The symmetric CSR matrix of unique undirected ``edges`` [p, 2] (unit ``weights`` by default), float64."""
    edges = np.asarray(edges, dtype=np.int64).reshape(-1, 2)
    w = np.ones(len(edges)) if weights is None else np.asarray(weights, dtype=np.float64)
    A = sp.coo_matrix((w, (edges[:, 0], edges[:, 1])), shape=(n, n))
    return (A + A.T).tocsr()


def distance_rows(n, edges, weights, sources, max_length=None):
    """float64 [len(sources), n]: the shortest-path length from each source to every node (BFS for unit lengths,
    Dijkstra otherwise); ``inf`` where there is no path or the length exceeds ``max_length``."""
    sources = np.asarray(sources, dtype=np.int64)
    if len(edges) == 0:
        D = np.full((len(sources), n), np.inf)
        D[np.arange(len(sources)), sources] = 0.0
        return D
    D = cs.shortest_path(adjacency(n, edges, weights), method="D", directed=False, unweighted=weights is None,
                         indices=sources)
    if max_length is not None:
        D = np.where(D <= max_length, D, np.inf)
    return D


def pairs_of_source(row, s):
    """``(targets j, distances)`` that ``shortest_paths`` holds for source ``s`` with every pair retained: ``j > s`` at
    finite positive distance, ascending in ``j``."""
    j = np.nonzero((np.arange(len(row)) > s) & (row > 0) & np.isfinite(row))[0]
    return j, row[j]


def top_k(row, s, k):
    """``(idx int32 [k], dist float32 [k])``: the ``k`` nearest targets of source ``s`` by (distance, index), targets
    at finite positive distance only; empty slots hold -1 / FLT_MAX."""
    ok = (np.arange(len(row)) != s) & (row > 0) & np.isfinite(row)
    j = np.nonzero(ok)[0]
    j = j[np.lexsort((j, row[j]))][:k]
    idx = np.full(k, -1, dtype=np.int32)
    dist = np.full(k, FLT_MAX, dtype=np.float32)
    idx[:len(j)] = j
    dist[:len(j)] = row[j]
    return idx, dist


def direct_lists(n, edges, weights, k):
    """The k-NN lists among a node's own graph neighbours by edge length, ties to the smaller index:
    ``(idx int32 [n, k], dist float32 [n, k])``."""
    edges = np.asarray(edges, dtype=np.int64).reshape(-1, 2)
    w = np.ones(len(edges)) if weights is None else np.asarray(weights, dtype=np.float64)
    a = np.concatenate([edges[:, 0], edges[:, 1]])
    b = np.concatenate([edges[:, 1], edges[:, 0]])
    ww = np.concatenate([w, w])
    order = np.lexsort((b, ww, a))                    # by node, then length, then neighbour
    a, b, ww = a[order], b[order], ww[order]
    rank = np.arange(len(a)) - np.searchsorted(a, a)  # position within the node's run
    keep = rank < k
    idx = np.full((n, k), -1, dtype=np.int32)
    dist = np.full((n, k), FLT_MAX, dtype=np.float32)
    idx[a[keep], rank[keep]] = b[keep]
    dist[a[keep], rank[keep]] = ww[keep]
    return idx, dist


def gsplitmix64(x):
    """SplitMix64's output function on a ``numpy.uint64`` array (wrapping arithmetic)."""
    x = np.asarray(x, dtype=np.uint64)
    with np.errstate(over="ignore"):
        x = x + np.uint64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return x ^ (x >> np.uint64(31))


def retained(n, i, j, retain_fraction, seed):
    """Which of the pairs ``(i, j)`` (arrays, ``i < j``) a call with ``retain_fraction`` and ``seed`` keeps:
    ``gsplitmix64(seed ^ gsplitmix64(i n + j)) < uint64(retain_fraction 2^64)``; every pair at 1.0 and above."""
    i, j = np.asarray(i, dtype=np.uint64), np.asarray(j, dtype=np.uint64)
    if retain_fraction >= 1.0:
        return np.ones(i.shape, dtype=bool)
    t = 0.0 if retain_fraction <= 0.0 else retain_fraction * 18446744073709551616.0
    threshold = np.uint64(2 ** 64 - 1 if t >= 18446744073709549568.0 else int(t))
    key = i * np.uint64(n) + j
    return gsplitmix64(np.uint64(seed & (2 ** 64 - 1)) ^ gsplitmix64(key)) < threshold


def connected_pairs(n, edges):
    """The number of unordered pairs of distinct nodes joined by a path: the sum of C(size, 2) over components."""
    if len(edges) == 0:
        return 0
    _, label = cs.connected_components(adjacency(n, edges), directed=False)
    size = np.bincount(label).astype(np.int64)
    return int((size * (size - 1) // 2).sum())

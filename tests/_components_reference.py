"""Host references (numpy / scipy, float64) for the component and bridging code: ``graph.connected_components``,
``preprocess.nearest_between_groups`` and ``preprocess.connect_components``.

* components: ``scipy.sparse.csgraph.connected_components``, whose labels number the components by their smallest
  node;
* the table of nearest pairs between groups in float64, minimum under the key ``(d, a, b)``;
* the ``"pairs"`` and ``"tree"`` bridges of such a table (Kruskal under the key ``(d, a, b)``);
* a synchronous replay of the hook-and-jump rounds of ``csrc/mde_graph_components.hip`` that counts the rounds;
* the Isomap replay of the three planar clusters: neighbour graph, bridges, Dijkstra, classical MDS, and the
  distances between the embedded centroids.
"""
import numpy as np
import scipy.sparse as sp
from scipy.sparse.csgraph import connected_components, dijkstra
from scipy.spatial.distance import cdist


# ---------------------------------------------------------------- graphs
def components(n, edges):
    """(count, labels) of the undirected graph on n nodes with edge list ``edges`` [p, 2]."""
    edges = np.asarray(edges, dtype=np.int64).reshape(-1, 2)
    A = sp.coo_matrix((np.ones(len(edges)), (edges[:, 0], edges[:, 1])), shape=(n, n)).tocsr()
    count, labels = connected_components(A, directed=False)
    return int(count), labels.astype(np.int64)


def random_edges(n, mean_degree, seed):
    """About ``n mean_degree / 2`` distinct random edges i < j (none for n < 2)."""
    rng = np.random.default_rng(seed)
    p = int(round(n * mean_degree / 2))
    if n < 2 or p == 0:
        return np.zeros((0, 2), dtype=np.int64)
    i = rng.integers(0, n, p)
    j = (i + 1 + rng.integers(0, n - 1, p)) % n
    e = np.unique(np.stack([np.minimum(i, j), np.maximum(i, j)], axis=1), axis=0)
    return e.astype(np.int64)


def star_with_isolated(leaves=5000, isolated=100):
    """Node 0 joined to ``leaves`` leaves, then ``isolated`` nodes without an edge."""
    n = 1 + leaves + isolated
    e = np.stack([np.zeros(leaves, dtype=np.int64), np.arange(1, leaves + 1, dtype=np.int64)], axis=1)
    return n, e


def renumbered_path(n, seed=0):
    """A path through all n nodes whose order along the path is a random permutation of the numbering."""
    order = np.random.default_rng(seed).permutation(n)
    e = np.stack([order[:-1], order[1:]], axis=1)
    return np.stack([e.min(axis=1), e.max(axis=1)], axis=1).astype(np.int64)


def hook_and_jump(n, edges, jumps=4, max_rounds=256):
    """The rounds of the kernel, every launch applied to a snapshot: ``(labels, rounds)``.  Hook: node u offers the
    smallest parent m among its neighbours to the slots par[par[u]] and par[u] when m < par[u]; jump: up to ``jumps``
    steps up the tree.  The round that changes nothing is counted, as the kernel counts it; no edge, no round."""
    edges = np.asarray(edges, dtype=np.int64).reshape(-1, 2)
    par = np.arange(n, dtype=np.int64)
    u = np.concatenate([edges[:, 0], edges[:, 1]])
    v = np.concatenate([edges[:, 1], edges[:, 0]])
    rounds = 0
    while len(edges) and rounds < max_rounds:
        before = par.copy()
        m = np.full(n, n, dtype=np.int64)
        np.minimum.at(m, u, before[v])
        offer = m < before
        np.minimum.at(par, before[offer], m[offer])
        np.minimum.at(par, np.flatnonzero(offer), m[offer])
        snap = par.copy()
        p = snap.copy()
        for _ in range(jumps):
            p = snap[p]
        par = np.minimum(par, p)
        rounds += 1
        if np.array_equal(par, before):
            break
    roots = np.flatnonzero(par == np.arange(n))
    return np.searchsorted(roots, par), rounds


# ---------------------------------------------------------------- nearest pairs and bridges
def nearest_pairs(X, labels, groups, sqdist=None):
    """``(d2 float64 [g, g], row int64 [g, g])``: for A != B the smallest squared distance between a row of group A
    and a row of group B and, in ``row[A, B]``, the row of group A in that pair; the minimum under the key (d2, a, b)
    with A < B.  inf / -1 on the diagonal and for a group without rows.  ``sqdist(XA, XB)``: the squared distances
    (default: squared Euclidean in float64)."""
    X = np.asarray(X, dtype=np.float64)
    labels = np.asarray(labels)
    if sqdist is None:
        def sqdist(P, Q):
            return cdist(P, Q, "sqeuclidean")
    d2 = np.full((groups, groups), np.inf)
    row = np.full((groups, groups), -1, dtype=np.int64)
    members = [np.flatnonzero(labels == g) for g in range(groups)]
    for A in range(groups):
        for B in range(A + 1, groups):
            if not len(members[A]) or not len(members[B]):
                continue
            S = sqdist(X[members[A]], X[members[B]])
            i, j = np.unravel_index(np.argmin(S), S.shape)     # (the first minimum in row-major order: key (d, a, b))
            d2[A, B] = d2[B, A] = S[i, j]
            row[A, B], row[B, A] = members[A][i], members[B][j]
    return d2, row


def brute_force_pairs(X, labels, groups):
    """``nearest_pairs`` by a plain loop over every pair of rows."""
    X = np.asarray(X, dtype=np.float64)
    best = {}
    for a in range(len(X)):
        for b in range(len(X)):
            A, B = int(labels[a]), int(labels[b])
            if A < B:
                key = (float(((X[a] - X[b]) ** 2).sum()), a, b)
                if (A, B) not in best or key < best[A, B]:
                    best[A, B] = key
    d2 = np.full((groups, groups), np.inf)
    row = np.full((groups, groups), -1, dtype=np.int64)
    for (A, B), (d, a, b) in best.items():
        d2[A, B] = d2[B, A] = d
        row[A, B], row[B, A] = a, b
    return d2, row


def tree_pairs(d2, row):
    """The g - 1 group pairs (A, B), A < B, of the minimum spanning tree under the key (d2, row[A, B], row[B, A])."""
    g = d2.shape[0]
    keys = sorted((d2[A, B], row[A, B], row[B, A], A, B) for A in range(g) for B in range(A + 1, g))
    parent = list(range(g))

    def find(x):
        while parent[x] != x:
            x = parent[x]
        return x

    out = []
    for _, _, _, A, B in keys:
        ra, rb = find(A), find(B)
        if ra != rb:
            parent[ra] = rb
            out.append((A, B))
    return out


def bridges(d2, row, rule):
    """``(edges int64 [b, 2] with i < j, sorted; d2 float64 [b])`` of the rule ``"pairs"`` or ``"tree"``."""
    g = d2.shape[0]
    pairs = [(A, B) for A in range(g) for B in range(A + 1, g)] if rule == "pairs" else tree_pairs(d2, row)
    rec = sorted((min(row[A, B], row[B, A]), max(row[A, B], row[B, A]), d2[A, B]) for A, B in pairs)
    return (np.array([(i, j) for i, j, _ in rec], dtype=np.int64).reshape(-1, 2),
            np.array([d for _, _, d in rec], dtype=np.float64))


# ---------------------------------------------------------------- data
BLOB_LAYOUTS = [(6, 40, 3, 8.0), (10, 30, 2, 5.0), (17, 12, 2, 3.0), (3, 100, 5, 20.0)]   # blobs, rows each, k, separation


def blobs(n_blobs, per, separation, seed, dim=5):
    """Gaussian blobs in R^dim with centres of scale ``separation``, rows shuffled, representable in float32."""
    rng = np.random.default_rng(seed)
    C = rng.normal(size=(n_blobs, dim)) * separation
    X = np.concatenate([c + rng.normal(size=(per, dim)) for c in C]).astype(np.float32).astype(np.float64)
    return X[rng.permutation(len(X))]


def grid_blobs(n_blobs=6, per=40, seed=0, dim=5):
    """Blobs on the integer grid (float32, |x| <= 64): every squared distance is exact in float32."""
    rng = np.random.default_rng(seed)
    C = rng.integers(-50, 51, size=(n_blobs, dim))
    X = np.concatenate([c + rng.integers(-4, 5, size=(per, dim)) for c in C])
    X = X[rng.permutation(len(X))]
    assert np.abs(X).max() <= 64
    return X.astype(np.float32)


def knn_edges(X, k):
    """``(edges i < j unique, lengths)`` of the k-nearest-neighbour graph in float64 (stable order on ties)."""
    D = cdist(X, X)
    M = D.copy()
    np.fill_diagonal(M, np.inf)
    idx = np.argsort(M, axis=1, kind="stable")[:, :k]
    i = np.repeat(np.arange(len(X)), k)
    j = idx.ravel()
    e = np.unique(np.stack([np.minimum(i, j), np.maximum(i, j)], axis=1), axis=0)
    return e, D[e[:, 0], e[:, 1]]


def three_clusters(per=60, seed=1):
    """Three planar clusters of ``per`` points centred at (0, 0), (30, 0) and (0, 40), mapped isometrically into
    R^5: ``(X float32 [3 per, 5], true centroid distances (30, 40, 50) for the pairs (0,1), (0,2), (1,2))``."""
    rng = np.random.default_rng(seed)
    cent = np.array([[0.0, 0.0], [30.0, 0.0], [0.0, 40.0]])
    P = np.concatenate([c + rng.uniform(-3, 3, size=(per, 2)) for c in cent])
    Q, _ = np.linalg.qr(rng.normal(size=(5, 2)))
    return (P @ Q.T).astype(np.float32), cdist(cent, cent)[np.triu_indices(3, 1)]


def centroid_distances(Y, per):
    """The distances between the centroids of consecutive blocks of ``per`` rows, pairs in ``triu`` order."""
    Y = np.asarray(Y, dtype=np.float64)
    cen = np.array([Y[b * per:(b + 1) * per].mean(axis=0) for b in range(len(Y) // per)])
    return cdist(cen, cen)[np.triu_indices(len(cen), 1)]


def isomap_centroid_ratios(X, k, rule, per, true):
    """The float64 Isomap replay: k-NN graph, bridges by ``rule``, Dijkstra, classical MDS in two dimensions; the
    embedded centroid distances over the ``true`` ones, and the number of components before bridging."""
    X = np.asarray(X, dtype=np.float64)
    n = len(X)
    e, w = knn_edges(X, k)
    count, labels = components(n, e)
    if count > 1:
        d2, row = nearest_pairs(X, labels, count)
        be, bd2 = bridges(d2, row, rule)
        e, w = np.concatenate([e, be]), np.concatenate([w, np.sqrt(bd2)])
    W = sp.coo_matrix((w, (e[:, 0], e[:, 1])), shape=(n, n)).tocsr()
    G = dijkstra(W, directed=False)
    assert np.isfinite(G).all()
    J = np.eye(n) - 1.0 / n
    evals, V = np.linalg.eigh(-0.5 * J @ (G ** 2) @ J)
    Y = V[:, -2:] * np.sqrt(evals[-2:])
    return centroid_distances(Y, per) / true, count

"""The float64 reference of ``graph.distances_from`` and the small graphs its tests share (no device needed):
``scipy.sparse.csgraph.dijkstra(directed=False, indices=sources)`` on the float32 edge lengths converted to float64,
returned node-major ([n, m], as the kernel writes it), and a numpy replay of farthest-point selection over it."""
import functools

import numpy as np
import scipy.sparse as sp
from scipy.sparse.csgraph import connected_components, dijkstra


def dyadic(rng, size):
    """Lengths that are multiples of 2^-6 in [2^-6, 4]: every path sum below 2^18 is exact in float32."""
    return (rng.integers(1, 257, size=size) / 64.0).astype(np.float32)


def _unique(n, edges, lengths):
    """Edges as i < j, sorted, one length each (the first of repeats; self pairs dropped)."""
    edges = np.asarray(edges, dtype=np.int64).reshape(-1, 2)
    keep = edges[:, 0] != edges[:, 1]
    edges, lengths = np.sort(edges[keep], axis=1), np.asarray(lengths, dtype=np.float32)[keep]
    _, first = np.unique(edges[:, 0] * n + edges[:, 1], return_index=True)
    return edges[first], lengths[first]


@functools.lru_cache(maxsize=None)
def cycle(n=257, seed=1):
    edges = np.stack([np.arange(n), (np.arange(n) + 1) % n], axis=1)
    return (n,) + _unique(n, edges, dyadic(np.random.default_rng(seed), n))


@functools.lru_cache(maxsize=None)
def random_graph(n=400, n_edges=500, seed=2, generic=False):
    """About ``n_edges`` random edges: at 400 / 500 several components and isolated nodes.  ``generic``: lengths
    uniform in [0.5, 3) instead of dyadic."""
    rng = np.random.default_rng(seed)
    edges = rng.integers(0, n, size=(n_edges, 2))
    lengths = rng.uniform(0.5, 3.0, n_edges).astype(np.float32) if generic else dyadic(rng, n_edges)
    return (n,) + _unique(n, edges, lengths)


@functools.lru_cache(maxsize=None)
def star_with_tail(leaves=300, tail=40, seed=3):
    """Node 0 joined to ``leaves`` leaves (degree far above 64), and a path of ``tail`` nodes hanging off leaf 1."""
    n = 1 + leaves + tail
    hub = np.stack([np.zeros(leaves, dtype=np.int64), 1 + np.arange(leaves)], axis=1)
    chain = np.concatenate([[1], 1 + leaves + np.arange(tail)])
    path = np.stack([chain[:-1], chain[1:]], axis=1)
    edges = np.concatenate([hub, path])
    return (n,) + _unique(n, edges, dyadic(np.random.default_rng(seed), len(edges)))


def pair():
    return 2, np.array([[0, 1]], dtype=np.int64), np.array([0.75], dtype=np.float32)


@functools.lru_cache(maxsize=None)
def path_graph(n=400, seed=4):
    edges = np.stack([np.arange(n - 1), np.arange(1, n)], axis=1)
    return (n,) + _unique(n, edges, dyadic(np.random.default_rng(seed), n - 1))


def two_cycles(size=60, extra=0):
    """Two disjoint cycles of ``size`` nodes with unit lengths, and ``extra`` isolated nodes after them."""
    ring = np.stack([np.arange(size), (np.arange(size) + 1) % size], axis=1)
    edges = np.concatenate([ring, ring + size])
    return (2 * size + extra,) + _unique(2 * size + extra, edges, np.ones(len(edges), dtype=np.float32))


def adjacency(n, edges, lengths):
    lengths = np.asarray(lengths, dtype=np.float32).astype(np.float64)
    return sp.csr_matrix((lengths, (edges[:, 0], edges[:, 1])), shape=(n, n))


def distances_from(n, edges, lengths, sources, max_length=None):
    """float64 [n, m]: column b holds the shortest-path lengths from sources[b] (inf where there is no path, or none of
    length <= max_length)."""
    sources = np.asarray(sources, dtype=np.int64).reshape(-1)
    d = dijkstra(adjacency(n, edges, lengths), directed=False, indices=sources,
                 limit=np.inf if max_length is None else float(max_length))
    return np.ascontiguousarray(d.T)


def components(n, edges):
    return connected_components(adjacency(n, edges, np.ones(len(edges))), directed=False)[1]


def farthest(D, m, start):
    """Farthest-point selection replayed over all-pairs lengths ``D`` [n, n]: ``(indices, radius, nearest,
    distance)``, ties to the smallest index, a chosen node never taken again."""
    n = D.shape[0]
    distance = np.full(n, np.inf)
    nearest = np.zeros(n, dtype=np.int64)
    chosen = np.zeros(n, dtype=bool)
    indices, radius = [], []
    node = int(start)
    for t in range(m):
        indices.append(node)
        radius.append(distance[node])
        chosen[node] = True
        closer = D[node] < distance
        nearest[closer] = t
        distance = np.minimum(distance, D[node])
        score = np.where(chosen, -1.0, distance)
        node = int(np.flatnonzero(score == score.max())[0])
    return np.array(indices), np.array(radius), nearest, distance

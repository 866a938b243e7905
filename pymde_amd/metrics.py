"""Metrics on the original data: ``metric=`` of ``preprocess.k_nearest_neighbors``, ``recipes.distances``
and the recipes (csrc/mde_metric.hip).  The reference has no such keyword (its
pynndescent call is Euclidean); the definitions are those of ``scipy.spatial.distance``:

  * ``"euclidean"`` (alias ``"l2"``) -- the default, every path as before;
  * ``"cosine"`` -- ``1 - u.v / (|u| |v|)``;
  * ``"correlation"`` -- cosine of the row-centred vectors;
  * ``"manhattan"`` (aliases ``"l1"``, ``"cityblock"``) -- ``sum |u - v|``.

For unit rows the squared chord is ``2 (1 - cos)``: cosine and correlation neighbours are the Euclidean
neighbours of a normalised (centred and normalised) float32 copy of the data, found by the unchanged
Euclidean kernels, and ``d2 / 2`` is the metric's distance.  Manhattan has a kernel of its own
(``mde_knn_l1``).  Pair distances of every metric come from one per-edge kernel on the original rows.
The name is resolved before any device is required.
"""
import torch

from pymde_amd import _lib

EUCLIDEAN, COSINE, CORRELATION, MANHATTAN = "euclidean", "cosine", "correlation", "manhattan"
METRICS = (EUCLIDEAN, COSINE, CORRELATION, MANHATTAN)
ALIASES = {"l2": EUCLIDEAN, "l1": MANHATTAN, "cityblock": MANHATTAN}
CODES = {EUCLIDEAN: 0, COSINE: 1, CORRELATION: 2, MANHATTAN: 3}     # MDE_METRIC_* of include/mde_hip.h


def resolve(metric):
    """Canonical name of a metric or alias (case-insensitive); ``ValueError`` for anything else."""
    name = metric.strip().lower() if isinstance(metric, str) else metric
    name = ALIASES.get(name, name) if isinstance(name, str) else name
    if name not in METRICS:
        raise ValueError(f"unknown metric {metric!r}; the metrics are {', '.join(METRICS)} "
                         f"(aliases: {', '.join(sorted(ALIASES))})")
    return name


def check_graph(metric):
    """A ``Graph`` input has its own shortest-path metric: only the default may accompany it."""
    if resolve(metric) != EUCLIDEAN:
        raise ValueError(f"metric={metric!r} applies to data matrices; a Graph has its own shortest-path metric")


def check_approximate(metric, approximate):
    """The inverted file's k-means lists are Euclidean: approximate search serves the metrics that reduce
    to a Euclidean search (euclidean, cosine, correlation), not Manhattan."""
    if approximate and resolve(metric) == MANHATTAN:
        raise ValueError("approximate=True has no Manhattan search (the inverted file's k-means lists are "
                         "Euclidean); use approximate=False, or metric='cosine' / 'correlation' / 'euclidean'")


def _raise_degenerate(metric, deg, n):
    count, first = (int(v) for v in deg.tolist())
    if count:
        what = "all-zero" if metric == COSINE else "constant"
        raise ValueError(f"metric='{metric}' is undefined for {what} rows (and for rows that hold NaN or "
                         f"infinity): {count} of the {n} rows are such rows, the first one is row {first}")


def normalized_rows(data, metric):
    """The unit rows (centred first for correlation) of a dense float32 [n, nf] on the GPU, as a new
    float32 [n, nf] (``4 n nf`` bytes).  ``ValueError`` when a row has no direction."""
    n, nf = int(data.shape[0]), int(data.shape[1])
    out = torch.empty_like(data)
    deg = torch.empty(2, dtype=torch.int32, device=data.device)
    with torch.cuda.device(data.device):
        _lib.check(_lib.load().mde_rows_normalize(n, nf, _lib.ptr(data), int(metric == CORRELATION), _lib.ptr(out),
                                                  _lib.ptr(deg), _lib.stream_ptr(data.device)))
    _raise_degenerate(metric, deg, n)
    return out


def check_rows(data, metric):
    """``ValueError`` when cosine / correlation is undefined for a row of the dense float32 [n, nf] (one
    reduction over the rows, no copy).  Euclidean and Manhattan accept every row."""
    if metric not in (COSINE, CORRELATION):
        return
    n, nf = int(data.shape[0]), int(data.shape[1])
    deg = torch.empty(2, dtype=torch.int32, device=data.device)
    with torch.cuda.device(data.device):
        _lib.check(_lib.load().mde_rows_normalize(n, nf, _lib.ptr(data), int(metric == CORRELATION), None,
                                                  _lib.ptr(deg), _lib.stream_ptr(data.device)))
    _raise_degenerate(metric, deg, n)


def normalized_csr(csr):
    """The ``sparse.DeviceCSR`` with unit rows (cosine; the sparsity pattern is shared with ``csr``).
    ``ValueError`` when a row is all zero."""
    from pymde_amd import sparse as _sparse
    values = torch.empty_like(csr.values)
    deg = torch.empty(2, dtype=torch.int32, device=csr.device)
    with torch.cuda.device(csr.device):
        _lib.check(_lib.load().mde_sparse_rows_normalize(
            csr.n, csr.n_features, csr.nnz, _lib.ptr(csr.indptr), _lib.ptr(csr.indices), _lib.ptr(csr.values),
            _lib.ptr(values), _lib.ptr(deg), _lib.stream_ptr(csr.device)))
    _raise_degenerate(COSINE, deg, csr.n)
    return _sparse.DeviceCSR(csr.indptr, csr.indices, values, csr.shape)


def manhattan_knn_lists(data, k):
    """Directed neighbour lists (idx [n, k] int32, distances [n, k]) of a dense float32 [n, nf] on the GPU
    under the Manhattan distance (``mde_knn_l1``)."""
    n, nf = int(data.shape[0]), int(data.shape[1])
    idx = torch.empty((n, k), dtype=torch.int32, device=data.device)
    dist = torch.empty((n, k), dtype=torch.float32, device=data.device)
    with torch.cuda.device(data.device):
        _lib.check(_lib.load().mde_knn_l1(n, nf, _lib.ptr(data), k, _lib.ptr(idx), _lib.ptr(dist),
                                          _lib.stream_ptr(data.device)))
    return idx, dist


def pair_distances(data, edges, metric):
    """Distances under ``metric`` between the rows of a dense float32 [n, nf] named by edges [p, 2]
    (int64), both on the GPU: one pass over the two original rows per edge, sums in double."""
    n, nf = int(data.shape[0]), int(data.shape[1])
    out = torch.empty(edges.shape[0], dtype=torch.float32, device=data.device)
    with torch.cuda.device(data.device):
        _lib.check(_lib.load().mde_pair_distances_metric(n, nf, _lib.ptr(data), edges.shape[0], _lib.ptr(edges),
                                                         CODES[metric], _lib.ptr(out),
                                                         _lib.stream_ptr(data.device)))
    return out

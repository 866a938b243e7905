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
                         f"(aliases: {', '.join(sorted(ALIASES))}); binary data under the Jaccard or Hamming "
                         "distance enter as a BitMatrix, pymde_amd.binary.pack(data)")
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


def translation_pays(mean, variance):
    """The rule of DESIGN section 6: a Euclidean search runs on the rows minus their column means when
    ``|mean|^2`` exceeds the summed column variance (``mean``, ``variance``: float64 sequences of one entry
    per column).  The float32 expansion ``|x|^2 + |y|^2 - 2 x.y`` errs by ~1e-7 of ``|x|^2 + |y|^2``, whose
    mean over the rows is ``2 (|mean|^2 + sum variance)``: below the threshold that is at most twice the
    centred scale ``2 sum variance``, and the data are searched as they are, bit for bit as before."""
    mean = torch.as_tensor(mean, dtype=torch.float64)
    return float((mean * mean).sum()) > float(torch.as_tensor(variance, dtype=torch.float64).sum())


def grid_means(mean, variance):
    """The vector a Euclidean search is translated by: every column mean rounded to a multiple of the largest
    power of two that does not exceed the column's standard deviation (float64 [nf], on the CPU; a column of
    zero variance keeps its mean).  The rounding moves a column by at most half its standard deviation, so
    the translated norms grow by at most a quarter of the summed variance; and data on a binary grid -- small
    integers, counts, values k / 2^j -- stay on it, so arithmetic that was exact in float32 before the
    translation (every product and sum of small integers) stays exact and ties stay ties."""
    mean = torch.as_tensor(mean, dtype=torch.float64).cpu()
    sd = torch.as_tensor(variance, dtype=torch.float64).cpu().sqrt()
    step = torch.exp2(torch.floor(torch.log2(sd.clamp(min=1e-300))))
    return torch.where(sd > 0, torch.round(mean / step) * step, mean)


def column_stats(data, what="the data matrix"):
    """(mean, variance) of the columns of a dense float32 [n, nf] on the GPU, summed in double there
    (``mde_col_stats``) and returned as float64 [nf] tensors on the CPU (one transfer).  ``ValueError`` naming
    ``what`` and the first such row when a row holds a NaN or an infinity: the Euclidean kernels would rank
    such a row at distance 0 of every other [ref: sklearn's check_array raises in the reference]."""
    n, nf = int(data.shape[0]), int(data.shape[1])
    lib = _lib.load()
    out = torch.empty(2 * nf + 1, dtype=torch.float64, device=data.device)      # the statistics, then the row
    bad = out[2 * nf:].view(torch.int32)
    with torch.cuda.device(data.device):
        nbytes = int(lib.mde_col_stats_work_bytes(n, nf))
        if nbytes < 0:
            _lib.check(nbytes)
        work = torch.empty(nbytes, dtype=torch.uint8, device=data.device)
        _lib.check(lib.mde_col_stats(n, nf, _lib.ptr(data), _lib.ptr(out), _lib.ptr(bad), _lib.ptr(work),
                                     _lib.stream_ptr(data.device)))
    host = out.cpu()
    raise_non_finite(int(host[2 * nf:].view(torch.int32)[0]), what)
    return host[:nf], host[nf:2 * nf]


def check_finite(data, what):
    """``ValueError`` naming ``what`` and the first row of the dense float32 [n, nf] on the GPU that holds a
    NaN or an infinity: the scan of ``mde_col_stats`` alone (one pass, no statistics)."""
    bad = torch.empty(1, dtype=torch.int32, device=data.device)
    with torch.cuda.device(data.device):
        _lib.check(_lib.load().mde_col_stats(int(data.shape[0]), int(data.shape[1]), _lib.ptr(data), None,
                                             _lib.ptr(bad), None, _lib.stream_ptr(data.device)))
    raise_non_finite(int(bad.item()), what)


def raise_non_finite(first, what):
    if first != 2 ** 31 - 1:
        raise ValueError(f"{what} holds NaN or infinity (the Euclidean distance to such a row is undefined); "
                         f"the first such row is row {first}")


def subtract_columns(data, mu):
    """``data - mu`` as a new float32 [n, nf] (``4 n nf`` bytes): ``mu`` float64 [nf] on the device, the
    subtraction in double, one rounding (``mde_rows_subtract``)."""
    out = torch.empty_like(data)
    mu = mu.contiguous()
    with torch.cuda.device(data.device):
        _lib.check(_lib.load().mde_rows_subtract(int(data.shape[0]), int(data.shape[1]), _lib.ptr(data),
                                                 _lib.ptr(mu), _lib.ptr(out),
                                                 _lib.stream_ptr(data.device)))
    return out


def translated_rows(data, what="the data matrix"):
    """The dense float32 [n, nf] a Euclidean search of ``data`` runs on, and the float64 vector it was
    translated by -- the column means on the grid of ``grid_means`` -- (None when ``translation_pays`` says
    that ``data`` itself is searched).  ``ValueError`` for a row that holds NaN or infinity."""
    mean, var = column_stats(data, what)
    if not translation_pays(mean, var):
        return data, None
    mu = grid_means(mean, var).to(data.device)
    return subtract_columns(data, mu), mu


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

"""How good is an embedding: trustworthiness, continuity and the k-NN overlap between the original data and
the embedding (``csrc/mde_knn_rank.hip``).  The reference has no such scores;
the definitions are those of Venna & Kaski and of ``sklearn.manifold.trustworthiness``.

``MDE.distortions()`` sees only the edges a problem was built from.  These scores see every pair: points that
land next to each other in the embedding without being neighbours in the data lower the trustworthiness, and
neighbours in the data that the embedding tore apart lower the continuity.  sklearn ranks through a dense
n x n distance matrix and an argsort per row; here a rank is a count over one pass of the Gram tile of the
exact k-NN search, so the scores cost about as much as the searches they are built on and need O(n k) memory.

A rank is 0-based and ties go to the smaller index: ``rank(i, j)`` is the number of rows ``l`` (other than
``i`` in a self-join) with ``(d2(i, l), l) < (d2(i, j), j)``, where ``d2`` is the float32 squared distance of
the Euclidean k-NN kernels, bit for bit.  The ranks of a search's own lists are therefore ``0 .. k - 1``.
"""
import torch

from pymde_amd import _lib, util
from pymde_amd import metrics as _metrics
from pymde_amd import preprocess as _preprocess

MAX_LIST = 64          # KNN_MAXK of csrc/mde_knn_tile.h: the longest list the kernels take
MAX_SLICES = 65535     # CROSS_MAX_SLICES of csrc/mde_knn_slices.h
_RANKED_METRICS = (_metrics.EUCLIDEAN, _metrics.COSINE, _metrics.CORRELATION)


def _resolve_metric(metric, *matrices):
    """Canonical name of a metric the rank kernel serves; ``ValueError`` otherwise, and for a ``Graph``
    (no device is needed to say so)."""
    metric = _metrics.resolve(metric)
    if metric not in _RANKED_METRICS:
        raise ValueError(f"metric={metric!r} has no rank kernel; the metrics pymde_amd.quality supports are "
                         "'euclidean', 'cosine' and 'correlation'")
    if any(_preprocess._is_graph(m) for m in matrices):
        raise ValueError("pymde_amd.quality ranks the rows of data matrices; a Graph has no rows to rank "
                         "(the metrics it supports are 'euclidean', 'cosine' and 'correlation' on a data matrix)")
    return metric


def _check_matrix(m, name):
    if not hasattr(m, "shape") or len(m.shape) != 2:
        raise ValueError(f"`{name}` must be a matrix [n, n_features]")


def _device_of(*arrays):
    on_gpu = [a.device for a in arrays if isinstance(a, torch.Tensor) and a.is_cuda]
    return util.require_cuda_device(on_gpu[0] if on_gpu else util.get_default_device())


def _self_rows(data, metric, device, what):
    """The dense float32 rows a self-join search of ``data`` under ``metric`` runs on (what
    ``preprocess.k_nearest_neighbors`` searches): translated for Euclidean data far from the origin, unit rows
    for cosine / correlation."""
    rows = _preprocess._dense_rows_for_cross(data, device, what)
    if metric == _metrics.EUCLIDEAN:
        return _metrics.translated_rows(rows, f"`{what}`")[0]
    return _metrics.normalized_rows(rows, metric)


def _ranks(Q, C, idx, self_join, slices=0):
    """``mde_knn_ranks`` on prepared dense float32 matrices and an int32 [n_q, m] list, all on one GPU."""
    n_q, n_c, nf, m = int(Q.shape[0]), int(C.shape[0]), int(C.shape[1]), int(idx.shape[1])
    device = C.device
    lib = _lib.load()
    ranks = torch.empty((n_q, m), dtype=torch.int32, device=device)
    with torch.cuda.device(device):
        nbytes = int(lib.mde_knn_ranks_work_bytes(n_q, n_c, m, slices))
        if nbytes < 0:
            _lib.check(nbytes)
        work = torch.empty(nbytes, dtype=torch.uint8, device=device)
        _lib.check(lib.mde_knn_ranks(n_q, n_c, nf, _lib.ptr(Q), _lib.ptr(C), int(self_join), m, _lib.ptr(idx),
                                     slices, _lib.ptr(ranks), None, _lib.ptr(work), _lib.stream_ptr(device)))
    return ranks


def neighbor_ranks(queries, data, idx, self_join=False, metric="euclidean", slices=0):
    """The rank, among all rows of ``data``, of the rows listed for every query: int32 [n_q, m] on the GPU.

    ``idx`` [n_q, m] (``1 <= m <= 64``) lists rows of ``data`` [n_c, n_features] for every row of ``queries``
    [n_q, n_features]; ``ranks[i, c]`` is the number of rows of ``data`` that precede ``idx[i, c]`` in the
    order ``(distance to query i, index)`` -- 0 for the nearest row, ties to the smaller index, the order the
    k-NN searches list by.  ``self_join=True``: the queries are the rows of ``data`` themselves (``queries`` is
    ``None`` or ``data``); row ``i`` does not count for query ``i``, as in ``preprocess.k_nearest_neighbors``.
    Entries that are not ranked come back as -1: negative entries, entries past the last row of ``data``, and
    in a self-join the query's own row.

    The matrices are prepared exactly as the searches prepare them, so the ranks refer to the rows the
    searches rank: the lists of ``preprocess.k_nearest_neighbors`` (``self_join=True``) and of
    ``preprocess.cross_nearest_neighbors`` get the ranks ``0 .. k - 1``.  Euclidean data far from the origin
    are translated (``metrics.translated_rows``; a cross search translates both matrices by the vector of
    ``data``); cosine and correlation rank the unit rows (``metrics.normalized_rows``).  Dense and sparse
    inputs as in ``cross_nearest_neighbors``.  ``metric``: ``"euclidean"``, ``"cosine"`` or ``"correlation"``
    (and their aliases); Manhattan and ``Graph`` inputs are a ``ValueError``.  ``slices``: the corpus split of
    the kernel's grid (0: automatic); the ranks do not depend on it."""
    metric = _resolve_metric(metric, queries, data)
    _check_matrix(data, "data")
    if self_join:
        if queries is not None and queries is not data:
            raise ValueError("self_join=True ranks the rows of `data` against `data`: pass queries=None (or `data`)")
        queries = data
    else:
        _check_matrix(queries, "queries")
        if int(queries.shape[1]) != int(data.shape[1]):
            raise ValueError(f"`queries` has {int(queries.shape[1])} features and `data` has "
                             f"{int(data.shape[1])}; they must agree")
    _check_matrix(idx, "idx")
    n_q, n_c, m = int(queries.shape[0]), int(data.shape[0]), int(idx.shape[1])
    if int(idx.shape[0]) != n_q:
        raise ValueError(f"`idx` has {int(idx.shape[0])} rows for {n_q} queries")
    if not 1 <= m <= MAX_LIST:
        raise ValueError(f"`idx` lists {m} rows per query; the rank kernel takes 1 to {MAX_LIST}")
    slices = int(slices)
    if not 0 <= slices <= MAX_SLICES:
        raise ValueError(f"slices must lie in [0, {MAX_SLICES}] (0: automatic), got {slices}")
    if n_q < 1 or n_c < 1 or int(data.shape[1]) < 1:
        raise ValueError("`queries` and `data` need at least one row and one feature")
    device = _device_of(data, queries)
    idx = torch.as_tensor(idx).to(device=device, dtype=torch.int32).contiguous()
    if self_join:
        Q = C = _self_rows(data, metric, device, "data")
    else:
        Q = _preprocess._dense_rows_for_cross(queries, device, "queries")
        C = _preprocess._dense_rows_for_cross(data, device, "data")
        if metric == _metrics.EUCLIDEAN:
            Q, C = _preprocess._translated_pair(Q, C)
        else:
            Q, C = _metrics.normalized_rows(Q, metric), _metrics.normalized_rows(C, metric)
    return _ranks(Q, C, idx, self_join, slices)


def _score_from_ranks(ranks, n, k, per_item=False):
    """Trustworthiness (continuity) from the 0-based ranks [n, k] in one space of every row's k nearest
    neighbours in the other: ``1 - 2 / (n k (2 n - 3 k - 1)) * sum max(0, rank + 1 - k)`` (sklearn's formula;
    its ranks are 1-based).  An integer tensor on any device; the sum is int64 and is read back once.
    ``per_item``: also every row's own term, normalised so that the rows average to the score (float32 [n])."""
    n, k = int(n), int(k)
    if not 1 <= k < n / 2:
        raise ValueError(f"n_neighbors ({k}) must be at least 1 and less than n_samples / 2 ({n / 2})")
    penalty = (ranks.to(torch.int64) + (1 - k)).clamp_(min=0).sum(dim=1)
    scale = 2.0 / (n * k * (2.0 * n - 3.0 * k - 1.0))
    score = 1.0 - int(penalty.sum().item()) * scale
    if not per_item:
        return score
    return score, (1.0 - penalty.to(torch.float64) * (scale * n)).to(torch.float32)


def _check_k(n_neighbors, n):
    k = int(n_neighbors)
    if not 1 <= k < n / 2:
        raise ValueError(f"n_neighbors ({k}) must be at least 1 and less than n_samples / 2 ({n / 2})")
    if k > MAX_LIST:
        raise ValueError(f"n_neighbors ({k}) exceeds the longest neighbour list of the k-NN kernels ({MAX_LIST})")
    return k


def _check_pair(data, X, n_neighbors, metric):
    """The argument checks the three scores share, before any device is required: (metric, n, k)."""
    metric = _resolve_metric(metric, data, X)
    _check_matrix(data, "data")
    _check_matrix(X, "X")
    n = int(data.shape[0])
    if int(X.shape[0]) != n:
        raise ValueError(f"`data` has {n} rows and the embedding `X` has {int(X.shape[0])}; they must agree")
    return metric, n, _check_k(n_neighbors, n)


def _rank_score(listed, ranked, k, per_item):
    """Rows ``listed``: their exact k nearest neighbours; ranked in the rows ``ranked``; the score."""
    idx, _ = _preprocess._dense_knn_lists(listed, k)
    return _score_from_ranks(_ranks(ranked, ranked, idx, True), int(listed.shape[0]), k, per_item)


def trustworthiness(data, X, n_neighbors=5, metric="euclidean", per_item=False):
    """To what extent the neighbours of a point in the embedding ``X`` [n, d] are its neighbours in ``data``
    [n, n_features]: ``1 - 2 / (n k (2 n - 3 k - 1)) * sum_i sum_{j in kNN_X(i)} max(0, rank_data(i, j) - k)``
    with 1-based ranks, as ``sklearn.manifold.trustworthiness`` (here 0-based, ties to the smaller index).  1.0
    when no point has an embedding neighbour from beyond its ``n_neighbors`` nearest rows of ``data``.

    ``data``: a dense or sparse data matrix (as ``preprocess.cross_nearest_neighbors`` takes them); ``X``: a
    float32 embedding on the GPU -- what ``MDE.embed`` returns -- or a CPU tensor / ndarray, which is copied
    there.  ``metric`` names the distance in ``data`` (``"euclidean"``, ``"cosine"``, ``"correlation"``); the
    embedding side is always Euclidean.  ``kNN_X`` is the exact float32 self-join of the embedding, and
    ``rank_data`` ranks among the rows the search of ``data`` runs on (``neighbor_ranks``).  ``n_neighbors``
    must satisfy ``1 <= n_neighbors < n / 2`` (a ``ValueError`` otherwise, as in sklearn) and is at most 64.

    Returns a Python float; ``per_item=True`` returns ``(score, per_row)`` with ``per_row`` float32 [n] on the
    GPU, every row's own term normalised so that the rows average to the score (colour a plot by it)."""
    metric, n, k = _check_pair(data, X, n_neighbors, metric)
    device = _device_of(X, data)
    return _rank_score(_self_rows(X, _metrics.EUCLIDEAN, device, "X"), _self_rows(data, metric, device, "data"),
                       k, per_item)


def continuity(data, X, n_neighbors=5, metric="euclidean", per_item=False):
    """To what extent the neighbours of a point in ``data`` stay its neighbours in the embedding ``X``:
    ``trustworthiness`` with the roles of the two spaces swapped -- the exact ``n_neighbors`` nearest rows of
    ``data`` (under ``metric``) of every point are ranked in the embedding.  Arguments and return value as in
    ``trustworthiness``."""
    metric, n, k = _check_pair(data, X, n_neighbors, metric)
    device = _device_of(X, data)
    return _rank_score(_self_rows(data, metric, device, "data"), _self_rows(X, _metrics.EUCLIDEAN, device, "X"),
                       k, per_item)


def _list_overlap(a, b):
    """``mde_knn_list_overlap``: per row, how many entries (>= 0) of the int32 list ``a`` occur in ``b``."""
    n = int(a.shape[0])
    count = torch.empty(n, dtype=torch.int32, device=a.device)
    with torch.cuda.device(a.device):
        _lib.check(_lib.load().mde_knn_list_overlap(n, int(a.shape[1]), _lib.ptr(a), int(b.shape[1]), _lib.ptr(b),
                                                    _lib.ptr(count), _lib.stream_ptr(a.device)))
    return count


def neighbor_overlap(data, X, n_neighbors=15, metric="euclidean", per_item=False, precision="float32"):
    """The mean over the points of ``|kNN_data(i) & kNN_X(i)| / n_neighbors``: the recall of the data
    neighbourhoods in the embedding ``X``.  Arguments and return value as in ``trustworthiness``, with
    ``1 <= n_neighbors <= min(64, n - 1)``.  ``precision`` (``"float32"`` / ``"bfloat16"``) is passed to the
    search of ``data`` only (``preprocess.k_nearest_neighbors``), so the bfloat16 search can be scored as
    well; the embedding is searched exactly in float32."""
    metric = _resolve_metric(metric, data, X)
    _check_matrix(data, "data")
    _check_matrix(X, "X")
    n, k = int(data.shape[0]), int(n_neighbors)
    if int(X.shape[0]) != n:
        raise ValueError(f"`data` has {n} rows and the embedding `X` has {int(X.shape[0])}; they must agree")
    if not 1 <= k <= min(MAX_LIST, n - 1):
        raise ValueError(f"n_neighbors ({k}) must lie in [1, min({MAX_LIST}, n - 1)] (n = {n})")
    precision = _preprocess._check_precision_arguments(precision, None, k, metric)
    device = _device_of(X, data)
    rows = _preprocess._dense_rows_for_cross(data, device, "data")
    if metric == _metrics.EUCLIDEAN:
        idx_data, _ = _preprocess._euclidean_knn_lists(rows, k, precision=precision)
    else:
        idx_data, _, _ = _preprocess._metric_knn_lists(rows, k, metric, precision=precision)
    idx_x, _ = _preprocess._dense_knn_lists(_self_rows(X, _metrics.EUCLIDEAN, device, "X"), k)
    count = _list_overlap(idx_data, idx_x)
    score = int(count.sum(dtype=torch.int64).item()) / (n * float(k))
    if not per_item:
        return score
    return score, (count.to(torch.float64) / k).to(torch.float32)

"""How good is an embedding: trustworthiness, continuity and the k-NN overlap between the original data and
the embedding (``csrc/mde_knn_rank.hip``).  The reference has no such scores;
the definitions are those of Venna & Kaski and of ``sklearn.manifold.trustworthiness``.

``MDE.distortions()`` sees only the edges a problem was built from.  These scores see every pair: points that
land next to each other in the embedding without being neighbours in the data lower the trustworthiness, and
neighbours in the data that the embedding tore apart lower the continuity.  sklearn ranks through a dense
n x n distance matrix and an argsort per row; here a rank is a count over one pass of the Gram tile of the
exact k-NN search, so the scores cost about as much as the searches they are built on and need O(n k) memory.

Those are rank statistics of the nearest few rows.  Whether far things stay far is what the global scores at the
end of this module tell: Kruskal's ``stress``, the ``distance_correlation`` of all pairwise distances and the
``shepard_histogram``, all functions of sums over every pair that one more pass of the same Gram tile forms in
O(n) memory (``pair_moments``, ``csrc/mde_pair_moments.hip``).

All of those form the data-side distance from data rows.  Where it exists only as a matrix -- the shortest-path lengths
of a ``Graph``, which an Isomap embedding is to be judged by, or a caller's precomputed dissimilarities -- the
``matrix_*`` and ``graph_*`` functions at the end of this module give the same scores from walks of that matrix
(``csrc/mde_matrix_quality.hip``).

A rank is 0-based and ties go to the smaller index: ``rank(i, j)`` is the number of rows ``l`` (other than
``i`` in a self-join) with ``(d2(i, l), l) < (d2(i, j), j)``, where ``d2`` is the float32 squared distance of
the Euclidean k-NN kernels, bit for bit.  The ranks of a search's own lists are therefore ``0 .. k - 1``.
"""
import collections
import math

import numpy as np
import torch

from pymde_amd import _lib, util
from pymde_amd import binary as _binary
from pymde_amd import metrics as _metrics
from pymde_amd import preprocess as _preprocess

MAX_LIST = 64          # KNN_MAXK of csrc/mde_knn_tile.h: the longest list the kernels take
MAX_SLICES = 65535     # CROSS_MAX_SLICES of csrc/mde_knn_slices.h
_RANKED_METRICS = (_metrics.EUCLIDEAN, _metrics.COSINE, _metrics.CORRELATION)


def _resolve_metric(metric, *matrices):
    """Canonical name of a metric the rank kernel serves; ``ValueError`` otherwise, and for a ``Graph``
    (no device is needed to say so)."""
    for m in matrices:
        _binary.refuse(m, "pymde_amd.quality", "the matrix_* scores take the distances themselves")
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


# ---------------------------------------------------------------- global scores: all pairs, not the nearest few
# (csrc/mde_pair_moments.hip)
MAX_BINS = 64          # PAIR_MAX_BINS of csrc/mde_pair_moments.hip

PairMoments = collections.namedtuple(
    "PairMoments", ["count", "sum_d", "sum_e", "sum_dd", "sum_ee", "sum_de", "max_d", "max_e", "row_sums", "rows"])
PairMoments.__doc__ = """Sums over the counted pairs (i, j), j != i, of the data distance D and the embedding distance
E: ``count`` pairs; ``sum_d``, ``sum_e``, ``sum_dd``, ``sum_ee``, ``sum_de`` (Python floats, summed in float64 on
the GPU); ``max_d``, ``max_e`` the largest D and E; ``row_sums`` float64 [n_q, 5] on the GPU, every query row's own
five sums in that order; ``rows`` int64 [n_q] on the CPU, the sampled query rows (None: every row, in order)."""


def _pair_modes(metric):
    """(mode_a, mode_b) of ``mde_pair_moments``: the data side returns ``0.5 d2`` of the unit rows for cosine /
    correlation (the distance the searches return), the embedding side is always Euclidean."""
    return (0 if metric == _metrics.EUCLIDEAN else 1), 0


def _pair_work(lib, n, n_q, slices, device):
    nbytes = int(lib.mde_pair_moments_work_bytes(n, n_q, slices))
    if nbytes < 0:
        _lib.check(nbytes)
    return torch.empty(nbytes, dtype=torch.uint8, device=device)


def _pair_moments(A, B, mode_a=0, mode_b=0, q_rows=None, slices=0):
    """``mde_pair_moments`` on prepared dense float32 matrices (and an int32 list of query rows) on one GPU:
    ``(row_sums float64 [n_q, 5], row_max float32 [n_q, 2], totals float64 [8])`` on that GPU."""
    n, device = int(A.shape[0]), A.device
    n_q = n if q_rows is None else int(q_rows.shape[0])
    lib = _lib.load()
    row_sums = torch.empty((n_q, 5), dtype=torch.float64, device=device)
    row_max = torch.empty((n_q, 2), dtype=torch.float32, device=device)
    totals = torch.empty(8, dtype=torch.float64, device=device)
    with torch.cuda.device(device):
        work = _pair_work(lib, n, n_q, slices, device)
        _lib.check(lib.mde_pair_moments(n, int(A.shape[1]), _lib.ptr(A), mode_a, int(B.shape[1]), _lib.ptr(B), mode_b,
                                        n_q, _lib.ptr(q_rows), slices, _lib.ptr(row_sums), _lib.ptr(row_max),
                                        _lib.ptr(totals), _lib.ptr(work), _lib.stream_ptr(device)))
    return row_sums, row_max, totals


def _pair_histogram(A, B, bins, a_range, b_range, mode_a=0, mode_b=0, q_rows=None, slices=0):
    """``mde_pair_histogram`` on prepared matrices: int64 [bins, bins] on their GPU."""
    n, device = int(A.shape[0]), A.device
    n_q = n if q_rows is None else int(q_rows.shape[0])
    lib = _lib.load()
    counts = torch.zeros((bins, bins), dtype=torch.int64, device=device)
    with torch.cuda.device(device):
        work = _pair_work(lib, n, n_q, slices, device)
        _lib.check(lib.mde_pair_histogram(n, int(A.shape[1]), _lib.ptr(A), mode_a, int(B.shape[1]), _lib.ptr(B),
                                          mode_b, n_q, _lib.ptr(q_rows), slices, bins, a_range[0], a_range[1],
                                          b_range[0], b_range[1], _lib.ptr(counts), _lib.ptr(work),
                                          _lib.stream_ptr(device)))
    return counts


def _check_global(data, X, metric, sample, slices=0):
    """The argument checks the global scores share, before any device is required: (metric, n, m) with ``m`` the
    number of sampled query rows, None for all of them."""
    metric = _resolve_metric(metric, data, X)
    _check_matrix(data, "data")
    _check_matrix(X, "X")
    n = int(data.shape[0])
    if int(X.shape[0]) != n:
        raise ValueError(f"`data` has {n} rows and the embedding `X` has {int(X.shape[0])}; they must agree")
    if n < 2 or int(data.shape[1]) < 1 or int(X.shape[1]) < 1:
        raise ValueError("`data` and `X` need at least two rows and one feature")
    if not 0 <= int(slices) <= MAX_SLICES:
        raise ValueError(f"slices must lie in [0, {MAX_SLICES}] (0: automatic), got {slices}")
    if sample is not None:
        if isinstance(sample, bool) or int(sample) != sample or not 1 <= int(sample) <= n:
            raise ValueError(f"sample must be None or a whole number of query rows in [1, {n}], got {sample!r}")
        sample = int(sample) if int(sample) < n else None
    return metric, n, sample


def _check_scale(scale):
    if isinstance(scale, str):
        if scale != "optimal":
            raise ValueError(f"scale must be 'optimal' or a positive finite number, got {scale!r}")
        return scale
    try:
        value = float(scale)
    except (TypeError, ValueError):
        raise ValueError(f"scale must be 'optimal' or a positive finite number, got {scale!r}") from None
    if isinstance(scale, bool) or not (value > 0.0 and math.isfinite(value)):
        raise ValueError(f"scale must be 'optimal' or a positive finite number, got {scale!r}")
    return value


def _check_bins(bins):
    if isinstance(bins, bool) or int(bins) != bins or not 1 <= int(bins) <= MAX_BINS:
        raise ValueError(f"bins must be a whole number in [1, {MAX_BINS}], got {bins!r}")
    return int(bins)


def _check_range(range_):
    """``((d_lo, d_hi), (e_lo, e_hi))`` as float32-representable floats, or None."""
    if range_ is None:
        return None
    message = f"range must be None or ((d_lo, d_hi), (e_lo, e_hi)) with finite lo < hi, got {range_!r}"
    try:
        (d_lo, d_hi), (e_lo, e_hi) = range_
        out = tuple(float(torch.tensor(float(v), dtype=torch.float32)) for v in (d_lo, d_hi, e_lo, e_hi))
    except (TypeError, ValueError):
        raise ValueError(message) from None
    if not all(math.isfinite(v) for v in out) or not (out[0] < out[1] and out[2] < out[3]):
        raise ValueError(message)
    return (out[0], out[1]), (out[2], out[3])


def _sample_rows(n, m, seed):
    """``m`` distinct rows of ``range(n)`` from a ``torch.Generator`` seeded with ``seed`` (int64, on the CPU)."""
    g = torch.Generator()
    g.manual_seed(int(seed))
    return torch.randperm(n, generator=g)[:m].contiguous()


def _prepared_pair(data, X, metric, m, seed):
    """The two matrices as ``trustworthiness`` prepares them, on one GPU, and the sampled rows:
    (A, B, rows int64 on the CPU or None, q_rows int32 on the GPU or None)."""
    device = _device_of(X, data)
    A = _self_rows(data, metric, device, "data")
    B = _self_rows(X, _metrics.EUCLIDEAN, device, "X")
    if m is None:
        return A, B, None, None
    rows = _sample_rows(int(A.shape[0]), m, seed)
    return A, B, rows, rows.to(device=device, dtype=torch.int32)


def pair_moments(data, X, metric="euclidean", sample=None, seed=0, slices=0):
    """The sums every global score here is a function of: over all pairs (i, j), j != i, of the distance D in
    ``data`` [n, n_features] under ``metric`` and the Euclidean distance E in the embedding ``X`` [n, d], the sums
    of D, E, D^2, E^2 and D E, the two maxima and the pair count (a ``PairMoments``).  One pass of the Gram tile of
    the exact k-NN search over both matrices: O(n) memory, about the cost of one exact search of ``data``.

    ``data``, ``X`` and ``metric`` as in ``trustworthiness``, and prepared the same way; for ``"cosine"`` and
    ``"correlation"`` D is ``1 - cos``, the distance the searches return.  Each distance is the float32 distance
    of the k-NN kernels; the sums are float64, in a fixed order, the same bits on every run (for one ``slices``,
    the corpus split of the kernel's grid; 0: automatic -- another split changes the last bits).

    ``sample=m`` (``1 <= m <= n``): ``m`` distinct query rows, drawn with a ``torch.Generator`` seeded with
    ``seed``, against all ``n`` rows -- ``m (n - 1)`` ordered pairs, an unbiased estimate of every mean at
    ``m / n`` of the cost.  ``None``: every row, all ``n (n - 1)`` ordered pairs (each unordered pair twice).
    Manhattan and ``Graph`` inputs are a ``ValueError``."""
    metric, n, m = _check_global(data, X, metric, sample, slices)
    A, B, rows, q_rows = _prepared_pair(data, X, metric, m, seed)
    row_sums, _, totals = _pair_moments(A, B, *_pair_modes(metric), q_rows=q_rows, slices=int(slices))
    t = totals.cpu().tolist()
    return PairMoments(int(round(t[7])), t[0], t[1], t[2], t[3], t[4], t[5], t[6], row_sums, rows)


Scores = collections.namedtuple("Scores", ["stress", "alpha", "correlation", "per_item"])


def _scores_from_moments(moments, scale="optimal", per_item=False):
    """Every score as a float64 function of a ``PairMoments`` (no GPU needed): ``Scores(stress, alpha,
    correlation, per_item)``.

    ``stress``: Kruskal's stress-1 ``sqrt(sum (D - alpha E)^2 / sum D^2)``.  ``scale="optimal"``: the ``alpha =
    sum D E / sum E^2`` that minimises it, for which it is ``sqrt(max(0, 1 - (sum D E)^2 / (sum D^2 sum E^2)))``;
    a number: that ``alpha``, through ``sum D^2 - 2 alpha sum D E + alpha^2 sum E^2``.  Both forms subtract
    nearly equal numbers when the stress is small: of a stress ``s`` about ``1e-16 / s^2`` relative digits are
    lost, so values below ~1e-4 mean "zero" (the float32 distances put their own floor at ~1e-3 to 1e-4).
    ``correlation``: Pearson's r of D and E over the counted pairs.  ``per_item``: float32, one value per query
    row -- the row's ``sum_j (D - alpha E)^2`` over its ``sum_j D^2``, square-rooted, with the global ``alpha``
    (on the device of ``moments.row_sums``); NaN for a row whose D are all zero.
    No pairs, or a space in which every distance is zero, has no stress / correlation: NaN."""
    scale = _check_scale(scale)
    c = float(moments.count)
    sd, se, sdd, see, sde = (float(moments.sum_d), float(moments.sum_e), float(moments.sum_dd),
                             float(moments.sum_ee), float(moments.sum_de))
    nan = float("nan")
    if scale == "optimal":
        alpha = sde / see if see > 0.0 else nan
        stress = math.sqrt(max(0.0, 1.0 - (sde * sde) / (sdd * see))) if sdd > 0.0 and see > 0.0 else nan
    else:
        alpha = scale
        stress = math.sqrt(max(0.0, sdd - 2.0 * alpha * sde + alpha * alpha * see) / sdd) if sdd > 0.0 else nan
    var_d, var_e = c * sdd - sd * sd, c * see - se * se
    correlation = (c * sde - sd * se) / math.sqrt(var_d * var_e) if var_d > 0.0 and var_e > 0.0 else nan
    rows = None
    if per_item:
        s = moments.row_sums.to(torch.float64)
        rows = ((s[:, 2] - 2.0 * alpha * s[:, 4] + alpha * alpha * s[:, 3]).clamp_(min=0.0) / s[:, 2]).sqrt_()
        rows = rows.to(torch.float32)
    return Scores(stress, alpha, correlation, rows)


def stress(data, X, scale="optimal", per_item=False, metric="euclidean", sample=None, seed=0):
    """Kruskal's normalised stress (stress-1) of the embedding ``X`` of ``data``: ``sqrt(sum (D - alpha E)^2 /
    sum D^2)`` over all pairs, D the distance in ``data`` under ``metric`` and E the Euclidean distance in ``X``.
    0 for an embedding that keeps every distance (up to ``alpha``); it sees the far pairs that
    ``trustworthiness`` and ``continuity`` do not.

    ``scale="optimal"``: ``alpha = sum D E / sum E^2``, the factor that minimises the stress, which makes it
    invariant to the scale of the embedding -- right for ``Standardized`` and ``preserve_neighbors`` embeddings.
    ``scale=<number>``: that ``alpha``; 1.0 takes ``preserve_distances`` at its word.  Near zero the formula
    loses half its digits (``_scores_from_moments``): an exact copy scores ~1e-4 or less, not 0.0 exactly unless
    the two matrices are the same bits.  Other arguments as in ``pair_moments``.

    Returns a Python float; ``per_item=True`` returns ``(stress, per_row)`` with ``per_row`` float32 [n_q] on
    the GPU, every query row's own stress under the same ``alpha`` (colour a plot by it; with ``sample`` the
    rows are ``pair_moments(...).rows``, drawn from the same ``seed``)."""
    _check_scale(scale)
    scores = _scores_from_moments(pair_moments(data, X, metric, sample, seed), scale, per_item)
    return (scores.stress, scores.per_item) if per_item else scores.stress


def distance_correlation(data, X, metric="euclidean", sample=None, seed=0):
    """Pearson's correlation of the pairwise distances in ``data`` (under ``metric``) and in the embedding ``X``
    over all pairs -- the number behind a Shepard diagram; 1.0 when the embedding distances are an increasing
    linear function of the data distances.  This is NOT Szekely's distance correlation (dCor, the statistic of
    independence built from doubly centred distance matrices), only the plain correlation coefficient of two
    lists of distances.  Arguments as in ``pair_moments``; a Python float."""
    return _scores_from_moments(pair_moments(data, X, metric, sample, seed)).correlation


def shepard_histogram(data, X, bins=64, range=None, metric="euclidean", sample=None, seed=0):
    """The Shepard diagram as a 2-D histogram: ``(counts, d_edges, e_edges, n_counted)`` with ``counts`` int64
    [bins, bins] on the GPU -- ``counts[a, b]`` pairs whose data distance D falls in bin ``a`` and whose
    embedding distance E in bin ``b`` -- the float64 numpy arrays of the ``bins + 1`` bin edges on each axis, and
    the number of pairs counted.  ``1 <= bins <= 64``; the bins are uniform, the last one closed on the right, as
    in ``numpy.histogram2d``, with the bin of a value computed in float32.

    ``range=((d_lo, d_hi), (e_lo, e_hi))``: a pair outside either interval is not counted (``n_counted`` tells).
    ``None``: ``[0, max D] x [0, max E]`` from a ``pair_moments`` pass first, so every pair is counted.  Other
    arguments as in ``pair_moments``."""
    bins, range_ = _check_bins(bins), _check_range(range)
    metric, n, m = _check_global(data, X, metric, sample)
    A, B, rows, q_rows = _prepared_pair(data, X, metric, m, seed)
    modes = _pair_modes(metric)
    if range_ is None:
        top = _pair_moments(A, B, *modes, q_rows=q_rows)[2][5:7].cpu().tolist()
        range_ = tuple((0.0, v if v > 0.0 else 1.0) for v in top)   # a space whose distances are all zero: one unit
    counts = _pair_histogram(A, B, bins, range_[0], range_[1], *modes, q_rows=q_rows)
    d_edges, e_edges = (np.linspace(lo, hi, bins + 1, dtype=np.float64) for lo, hi in range_)
    return counts, d_edges, e_edges, int(counts.sum().item())


# ---------------------------------------------------------------- scores against a matrix of dissimilarities or a Graph
# (csrc/mde_matrix_quality.hip)
MAX_EMBEDDING_DIM = 8  # MQ_MAX_D of csrc/mde_matrix_quality.hip: the limit of the dense problems
_BATCH_ELEMENTS = 2 ** 29   # a batch of graph_* sources holds at most this many float32 path lengths (2 GiB)

MatrixMoments = collections.namedtuple(
    "MatrixMoments", PairMoments._fields + ("row_counts", "missing"))
MatrixMoments.__doc__ = """A ``PairMoments`` over the counted pairs (i, b) of a dissimilarity matrix [n, m] -- ``row_sums``
float64 [n, 5] holds every item's own sums over its counted columns, ``rows`` is None -- with ``row_counts`` int64 [n]
on the GPU, the number of counted pairs of every item, and ``missing``, the number of pairs skipped because their
entry is ``inf`` or ``FLT_MAX`` (the ``m`` pairs of an item with itself are neither counted nor missing)."""


def _check_items(items, n, m):
    """``items`` as a contiguous int32 tensor (on the device it came on), or None: ``ValueError`` unless it is a
    vector of ``m`` whole numbers in [0, n)."""
    if items is None:
        if m != n:
            raise ValueError(f"`distances` is [{n}, {m}]: without `items` its columns are the items themselves and "
                             "it must be square")
        return None
    t = items.detach() if isinstance(items, torch.Tensor) else torch.as_tensor(np.asarray(items))
    if t.dim() != 1 or int(t.numel()) != m:
        raise ValueError(f"`items` must be a vector with one entry per column of `distances` ({m}), got shape "
                         f"{tuple(t.shape)}")
    if t.dtype == torch.bool or t.is_floating_point() or t.is_complex():
        raise ValueError(f"`items` must hold item indices (integers), got dtype {t.dtype}")
    lo, hi = int(t.min()), int(t.max())
    if lo < 0 or hi >= n:
        raise ValueError(f"`items` must lie in [0, n) = [0, {n}); it holds {lo if lo < 0 else hi}")
    return t.to(torch.int32).contiguous()


def _check_embedding(X, n):
    _check_matrix(X, "X")
    if int(X.shape[0]) != n:
        raise ValueError(f"the distances have {n} rows and the embedding `X` has {int(X.shape[0])}; they must agree")
    d = int(X.shape[1])
    if not 1 <= d <= MAX_EMBEDDING_DIM:
        raise ValueError(f"the embedding `X` has {d} columns; the matrix scores take 1 to {MAX_EMBEDDING_DIM}")
    return d


def _check_distances(distances, X, items):
    """The argument checks of the matrix-level scores, before any device is required: (n, m, items)."""
    if _preprocess._is_graph(distances):
        raise ValueError("`distances` must be a matrix [n, m]; score a Graph with the graph_* functions")
    if not hasattr(distances, "shape") or len(distances.shape) != 2:
        raise ValueError("`distances` must be a matrix [n, m]")
    n, m = int(distances.shape[0]), int(distances.shape[1])
    if n < 1 or m < 1:
        raise ValueError("`distances` needs at least one row and one column")
    if X is not None:
        _check_embedding(X, n)
    return n, m, _check_items(items, n, m)


def _device_distances(distances, device):
    """``distances`` as float32 on ``device``, checked with one reduction to hold no NaN and no negative entry."""
    Dm = torch.as_tensor(distances).to(device=device, dtype=torch.float32).contiguous()
    if not bool((Dm >= 0).all()):
        raise ValueError("`distances` must not hold NaN or negative entries (inf marks a missing pair)")
    return Dm


def _device_embedding(X, device):
    return torch.as_tensor(X).detach().to(device=device, dtype=torch.float32).contiguous()


def _matrix_moments(Dm, X, items):
    """``mde_matrix_moments`` on prepared tensors of one GPU: (row_sums, row_count, row_max, totals) on that GPU."""
    n, m, device = int(Dm.shape[0]), int(Dm.shape[1]), Dm.device
    lib = _lib.load()
    row_sums = torch.empty((n, 5), dtype=torch.float64, device=device)
    row_count = torch.empty(n, dtype=torch.int64, device=device)
    row_max = torch.empty((n, 2), dtype=torch.float32, device=device)
    totals = torch.empty(8, dtype=torch.float64, device=device)
    with torch.cuda.device(device):
        work = _lib.work_buffer(lib.mde_matrix_moments_work_bytes, n, m, device=device)
        _lib.check(lib.mde_matrix_moments(n, m, _lib.ptr(Dm), _lib.ptr(items), int(X.shape[1]), _lib.ptr(X),
                                          _lib.ptr(row_sums), _lib.ptr(row_count), _lib.ptr(row_max),
                                          _lib.ptr(totals), _lib.ptr(work), _lib.stream_ptr(device)))
    return row_sums, row_count, row_max, totals


def _matrix_histogram(Dm, X, items, bins, d_range, e_range, counts):
    """``mde_matrix_histogram``: adds to ``counts`` int64 [bins, bins] on the GPU of the tensors."""
    device = Dm.device
    with torch.cuda.device(device):
        _lib.check(_lib.load().mde_matrix_histogram(int(Dm.shape[0]), int(Dm.shape[1]), _lib.ptr(Dm), _lib.ptr(items),
                                                    int(X.shape[1]), _lib.ptr(X), bins, d_range[0], d_range[1],
                                                    e_range[0], e_range[1], _lib.ptr(counts),
                                                    _lib.stream_ptr(device)))
    return counts


def _moments_from_parts(n_pairs, row_sums, row_count, totals):
    """A ``MatrixMoments`` from ``totals`` (a list of 8 floats) and the row outputs; ``n_pairs`` pairs were walked,
    the item itself excluded."""
    count = int(round(totals[7]))
    return MatrixMoments(count, totals[0], totals[1], totals[2], totals[3], totals[4], totals[5], totals[6], row_sums,
                         None, row_count, n_pairs - count)


def _prepared_matrix(distances, X, items):
    n, m, items = _check_distances(distances, X, items)
    device = _device_of(*(a for a in (distances, X) if isinstance(a, torch.Tensor)))
    Dm = _device_distances(distances, device)
    return Dm, _device_embedding(X, device) if X is not None else None, (None if items is None else items.to(device))


def matrix_moments(distances, X, items=None):
    """The sums the matrix scores are functions of, for any precomputed dissimilarities (sklearn's
    ``metric="precomputed"``): a ``MatrixMoments``.

    ``distances`` [n, m] (a torch or numpy array, copied to the GPU as float32): row ``i`` is item ``i`` and column
    ``b`` holds the dissimilarity D to item ``items[b]`` -- the layout of ``graph.distances_from``.  ``items``: ``m``
    item indices, repeats and any order allowed; ``None``: a square matrix, column ``b`` is item ``b``.  ``X`` [n, d],
    ``1 <= d <= 8``: the embedding; E is the float32 Euclidean distance formed from the differences.  The pair of an
    item with itself is not counted; an entry that is ``inf`` (or FLT_MAX) is a missing pair, skipped and reported in
    ``missing``.  NaN and negative entries are a ``ValueError`` (one reduction on the GPU).  Sums in float64 in a
    fixed order: the same bits on every run."""
    Dm, X, items = _prepared_matrix(distances, X, items)
    row_sums, row_count, _, totals = _matrix_moments(Dm, X, items)
    n, m = int(Dm.shape[0]), int(Dm.shape[1])
    return _moments_from_parts(n * m - m, row_sums, row_count, totals.cpu().tolist())


def _stress_from(moments, scale, per_item):
    scores = _scores_from_moments(moments, scale, per_item)
    return (scores.stress, scores.per_item) if per_item else scores.stress


def matrix_stress(distances, X, items=None, scale="optimal", per_item=False):
    """Kruskal's stress-1 of the embedding ``X`` against the dissimilarities ``distances`` over the counted pairs:
    ``stress`` with D read from a matrix.  ``distances``, ``X``, ``items`` as in ``matrix_moments``; ``scale`` as in
    ``stress``.  ``per_item=True`` returns ``(stress, per_row)``: float32 [n] on the GPU, one value per item over its
    counted columns under the same ``alpha``; an item without a counted pair (or whose D are all zero) is NaN."""
    _check_scale(scale)
    return _stress_from(matrix_moments(distances, X, items), scale, per_item)


def matrix_correlation(distances, X, items=None):
    """Pearson's correlation of D and E over the counted pairs of a dissimilarity matrix: ``distance_correlation``
    with D read from a matrix (not Szekely's dCor).  Arguments as in ``matrix_moments``; a Python float."""
    return _scores_from_moments(matrix_moments(distances, X, items)).correlation


def _range_from_maxima(top):
    return tuple((0.0, v if v > 0.0 else 1.0) for v in top)      # a space whose distances are all zero: one unit


def matrix_shepard_histogram(distances, X, items=None, bins=64, range=None):
    """``shepard_histogram`` with D read from a matrix: ``(counts, d_edges, e_edges, n_counted)``.  ``range=None``
    takes ``[0, max D] x [0, max E]`` over the counted pairs from a moments pass first.  Other arguments as in
    ``matrix_moments``; missing pairs are not counted."""
    bins, range_ = _check_bins(bins), _check_range(range)
    Dm, X, items = _prepared_matrix(distances, X, items)
    if range_ is None:
        range_ = _range_from_maxima(_matrix_moments(Dm, X, items)[3][5:7].cpu().tolist())
    counts = torch.zeros((bins, bins), dtype=torch.int64, device=Dm.device)
    _matrix_histogram(Dm, X, items, bins, range_[0], range_[1], counts)
    d_edges, e_edges = (np.linspace(lo, hi, bins + 1, dtype=np.float64) for lo, hi in range_)
    return counts, d_edges, e_edges, int(counts.sum().item())


def _check_lists(idx, m):
    _check_matrix(idx, "idx")
    if int(idx.shape[0]) != m:
        raise ValueError(f"`idx` has {int(idx.shape[0])} rows for {m} columns of `distances`")
    k = int(idx.shape[1])
    if not 1 <= k <= MAX_LIST:
        raise ValueError(f"`idx` lists {k} items per column; the rank kernel takes 1 to {MAX_LIST}")
    return k


def _matrix_ranks(Dm, idx, items):
    """``mde_matrix_ranks`` on prepared tensors of one GPU: int32 [m, k]."""
    device = Dm.device
    ranks = torch.empty(tuple(idx.shape), dtype=torch.int32, device=device)
    with torch.cuda.device(device):
        _lib.check(_lib.load().mde_matrix_ranks(int(Dm.shape[0]), int(Dm.shape[1]), _lib.ptr(Dm), _lib.ptr(items),
                                                int(idx.shape[1]), _lib.ptr(idx), _lib.ptr(ranks),
                                                _lib.stream_ptr(device)))
    return ranks


def matrix_ranks(distances, idx, items=None):
    """The rank, within its column of ``distances`` [n, m], of every listed item: int32 [m, k] on the GPU.

    ``idx`` [m, k] (``1 <= k <= 64``) lists items for every column; ``ranks[b, c]`` is the number of items ``j``
    other than ``items[b]`` that precede ``l = idx[b, c]`` in the order ``(distances[j, b], j)``: 0-based, ties to
    the smaller index, the rule of ``neighbor_ranks``.  ``inf`` is an ordinary value that sorts last: unreachable
    items rank after all reachable ones, by index.  Entries that are negative, ``>= n`` or the column's own item
    come back as -1.  ``distances`` and ``items`` as in ``matrix_moments``."""
    n, m, items = _check_distances(distances, None, items)
    _check_lists(idx, m)
    device = _device_of(*(a for a in (distances, idx) if isinstance(a, torch.Tensor)))
    Dm = _device_distances(distances, device)
    idx = torch.as_tensor(idx).to(device=device, dtype=torch.int32).contiguous()
    return _matrix_ranks(Dm, idx, None if items is None else items.to(device))


def _sampled_score(ranks, n, k, per_item=False):
    """``_score_from_ranks`` with the mean taken over the ``m`` listed items, the rows of ``ranks`` [m, k], of ``n``:
    ``1 - 2 / (m k (2 n - 3 k - 1)) * sum max(0, rank + 1 - k)``; sklearn's value when every item is listed once."""
    n, k, m = int(n), int(k), int(ranks.shape[0])
    _check_k(k, n)
    penalty = (ranks.to(torch.int64) + (1 - k)).clamp_(min=0).sum(dim=1)
    scale = 2.0 / (m * k * (2.0 * n - 3.0 * k - 1.0))
    score = 1.0 - int(penalty.sum().item()) * scale
    if not per_item:
        return score
    return score, (1.0 - penalty.to(torch.float64) * (scale * m)).to(torch.float32)


def _embedding_lists(X, k, items):
    """The exact float32 k-NN lists of the embedding (its self-join, as ``trustworthiness`` takes them) for the
    rows ``items`` (int64 on the GPU; None: every row)."""
    rows = _self_rows(X, _metrics.EUCLIDEAN, X.device, "X")
    if items is None or k == MAX_LIST or 2 * int(items.numel()) > int(X.shape[0]):
        idx, _ = _preprocess._dense_knn_lists(rows, k)
        return idx if items is None else idx[items].contiguous()
    # A few rows of many: their k + 1 nearest rows by the query-against-corpus search, which orders by the same
    # (d2, index) with the same bits, and the row itself taken out.  The first k of the others among the k + 1
    # nearest are the k nearest of the others whether or not the row itself is among them: the self-join's lists.
    idx, _ = _preprocess._cross_knn_lists(rows[items].contiguous(), rows, k + 1)
    others = idx != items.to(torch.int32)[:, None]
    keep = torch.argsort((~others).to(torch.int8), dim=1, stable=True)[:, :k]
    return torch.gather(idx, 1, keep).contiguous()


def matrix_trustworthiness(distances, X, n_neighbors=5, items=None, per_item=False):
    """``trustworthiness`` against precomputed dissimilarities: the exact ``n_neighbors`` nearest neighbours in the
    embedding ``X`` of every item ``items[b]`` are ranked within column ``b`` of ``distances`` (``matrix_ranks``),
    and the score is ``1 - 2 / (m k (2 n - 3 k - 1)) * sum max(0, rank + 1 - k)``: the mean over the ``m`` listed
    items, and the value of ``sklearn.manifold.trustworthiness(distances, X, metric="precomputed")`` when ``items``
    is every item (ties apart: here they go to the smaller index).  ``inf`` entries rank last.  ``X`` may have any
    number of columns.  ``per_item=True`` returns ``(score, per_column)``, float32 [m] on the GPU."""
    n, m, items = _check_distances(distances, None, items)
    _check_matrix(X, "X")
    if int(X.shape[0]) != n:
        raise ValueError(f"the distances have {n} rows and the embedding `X` has {int(X.shape[0])}; they must agree")
    k = _check_k(n_neighbors, n)
    device = _device_of(*(a for a in (distances, X) if isinstance(a, torch.Tensor)))
    Dm = _device_distances(distances, device)
    items = None if items is None else items.to(device)
    idx = _embedding_lists(_device_embedding(X, device), k, None if items is None else items.to(torch.int64))
    return _sampled_score(_matrix_ranks(Dm, idx, items), n, k, per_item)


# ---- the same against the shortest-path lengths of a Graph, from all nodes or a sample of them
def _check_graph(graph, X, sample, limit_d=True):
    """The argument checks of the graph-level scores, before any device is required: (n, m) with ``m`` the number of
    sampled sources, None for all nodes."""
    from pymde_amd import graph as _graph
    if not isinstance(graph, _graph.Graph):
        raise ValueError("`graph` must be a pymde_amd.Graph instance.")
    n = int(graph.n_items)
    if limit_d:
        _check_embedding(X, n)
    else:
        _check_matrix(X, "X")
        if int(X.shape[0]) != n:
            raise ValueError(f"`graph` has {n} nodes and the embedding `X` has {int(X.shape[0])} rows; they must agree")
    if sample is not None:
        if isinstance(sample, bool) or int(sample) != sample or not 1 <= int(sample) <= n:
            raise ValueError(f"sample must be None or a whole number of source nodes in [1, {n}], got {sample!r}")
        sample = int(sample) if int(sample) < n else None
    return n, sample


def _batch_columns(n, batch=None):
    """The number of sources of one ``distances_from`` call: at most 2 GiB of path lengths, a multiple of 64."""
    if batch is not None:
        return int(batch)
    return max(64, (_BATCH_ELEMENTS // n) // 64 * 64)


def _graph_batches(graph, n, m, seed, max_length, batch):
    """Yields ``(sources int64 on the GPU, Dm [n, len(sources)])`` for the sources of a graph-level score, in order:
    every node, or the ``m`` nodes of ``_sample_rows(n, m, seed)``."""
    from pymde_amd import graph as _graph
    plan, w = _graph._path_lengths(graph)
    sources = torch.arange(n) if m is None else _sample_rows(n, m, seed)
    sources = sources.to(plan.device)
    step = _batch_columns(n, batch)
    for lo in range(0, int(sources.numel()), step):
        src = sources[lo:lo + step].contiguous()
        yield src, _graph._distances_from(plan, w, src, max_length)


def graph_moments(graph, X, sample=None, seed=0, max_length=None, _batch=None):
    """``matrix_moments`` against the shortest-path lengths of ``graph`` (a ``MatrixMoments``): D is the geodesic
    from a source node to every node (``graph.distances_from``), E the Euclidean distance in the embedding ``X``
    [n, d], ``1 <= d <= 8`` -- the yardstick of ``preserve_geodesics``, ``DenseMDE.from_graph`` and
    ``LandmarkMDE.from_graph`` embeddings.  ``sample=None``: every node is a source, all ``n (n - 1)`` ordered pairs;
    ``sample=m``: the ``m`` nodes ``_sample_rows(n, m, seed)``, the rule of ``pair_moments``' ``sample=``.
    Pairs without a path (or none of length ``<= max_length``) are missing: skipped, and counted in ``missing``.

    The sources go through ``distances_from`` in batches of at most ``max(64, 2^29 / n rounded down to a multiple of
    64)`` columns (2 GiB); the batches' float64 row sums and totals are added in batch order, so the result is the
    same bits on every run (another batch size changes the last bits of the sums that involve E)."""
    n, m = _check_graph(graph, X, sample)
    X = _device_embedding(X, graph.plan().device)
    row_sums = row_count = None
    totals, n_pairs = [0.0] * 8, 0
    for src, Dm in _graph_batches(graph, n, m, seed, max_length, _batch):
        s, c, _, t = _matrix_moments(Dm, X, src.to(torch.int32))
        t = t.cpu().tolist()
        if row_sums is None:
            row_sums, row_count = s, c
        else:
            row_sums += s
            row_count += c
        totals = [a + b for a, b in zip(totals[:5], t[:5])] + [max(totals[5], t[5]), max(totals[6], t[6]),
                                                                totals[7] + t[7]]
        n_pairs += (n - 1) * int(src.numel())
    return _moments_from_parts(n_pairs, row_sums, row_count, totals)


def graph_stress(graph, X, scale="optimal", per_item=False, sample=None, seed=0, max_length=None, _batch=None):
    """Kruskal's stress-1 of the embedding ``X`` against the shortest-path lengths of ``graph``: what an Isomap
    embedding is to be judged by (the Euclidean ``stress`` penalises a rolled strip for being unrolled).  ``scale``
    and ``per_item`` as in ``matrix_stress`` (``per_item``: one value per node over the sources that reach it);
    other arguments as in ``graph_moments``."""
    _check_scale(scale)
    return _stress_from(graph_moments(graph, X, sample, seed, max_length, _batch), scale, per_item)


def graph_correlation(graph, X, sample=None, seed=0, max_length=None, _batch=None):
    """Pearson's correlation of the shortest-path lengths of ``graph`` and the distances in the embedding ``X``
    over the connected pairs.  Arguments as in ``graph_moments``; a Python float."""
    return _scores_from_moments(graph_moments(graph, X, sample, seed, max_length, _batch)).correlation


def graph_shepard_histogram(graph, X, bins=64, range=None, sample=None, seed=0, max_length=None, _batch=None):
    """``shepard_histogram`` against the shortest-path lengths of ``graph``: ``(counts, d_edges, e_edges,
    n_counted)``.  ``range=None`` takes the maxima from a ``graph_moments`` pass first (the paths are solved twice).
    The counts of the batches add.  Other arguments as in ``graph_moments``."""
    bins, range_ = _check_bins(bins), _check_range(range)
    n, m = _check_graph(graph, X, sample)
    if range_ is None:
        mom = graph_moments(graph, X, sample, seed, max_length, _batch)
        range_ = _range_from_maxima((mom.max_d, mom.max_e))
    X = _device_embedding(X, graph.plan().device)
    counts = torch.zeros((bins, bins), dtype=torch.int64, device=X.device)
    for src, Dm in _graph_batches(graph, n, m, seed, max_length, _batch):
        _matrix_histogram(Dm, X, src.to(torch.int32), bins, range_[0], range_[1], counts)
    d_edges, e_edges = (np.linspace(lo, hi, bins + 1, dtype=np.float64) for lo, hi in range_)
    return counts, d_edges, e_edges, int(counts.sum().item())


def graph_trustworthiness(graph, X, n_neighbors=5, sample=None, seed=0, per_item=False, _batch=None):
    """``trustworthiness`` against the shortest-path lengths of ``graph``: the exact ``n_neighbors`` nearest
    neighbours in the embedding ``X`` of every source node are ranked among the path lengths from that node
    (``matrix_ranks``); nodes without a path rank last, by index.  The mean is over the sources: every node, or the
    ``sample`` nodes of ``_sample_rows(n, sample, seed)``.  With every node and no tied path lengths this is
    ``sklearn.manifold.trustworthiness(D, X, metric="precomputed")`` of the matrix of path lengths.  ``X`` may have
    any number of columns.  ``per_item=True`` returns ``(score, per_source)``, float32 on the GPU in source order."""
    n, m = _check_graph(graph, X, sample, limit_d=False)
    k = _check_k(n_neighbors, n)
    X = _device_embedding(X, graph.plan().device)
    ranks = [_matrix_ranks(Dm, _embedding_lists(X, k, None if m is None and int(src.numel()) == n else src),
                           src.to(torch.int32))
             for src, Dm in _graph_batches(graph, n, m, seed, None, _batch)]
    return _sampled_score(torch.cat(ranks), n, k, per_item)


def graph_continuity(graph, X, n_neighbors=5, sample=None, seed=0, per_item=False):
    """``continuity`` against the shortest-path lengths of ``graph``: every node's ``n_neighbors`` nearest nodes
    under the shortest-path metric (``graph.k_nearest_neighbors(graph_distances=True)``'s lists, ties to the smaller
    index) are ranked in the embedding ``X``, and the mean is taken over all nodes or the ``sample`` nodes of
    ``_sample_rows(n, sample, seed)``.  A node that reaches fewer than ``n_neighbors`` others has entries of -1 in
    its list; they carry no penalty.  Arguments and return value as in ``graph_trustworthiness``."""
    from pymde_amd import graph as _graph
    n, m = _check_graph(graph, X, sample, limit_d=False)
    k = _check_k(n_neighbors, n)
    device = graph.plan().device
    idx, _ = _graph._neighbor_lists(graph, k, graph_distances=True)
    rows = _self_rows(_device_embedding(X, device), _metrics.EUCLIDEAN, device, "X")
    ranks = _ranks(rows, rows, idx.contiguous(), True)
    if m is not None:
        ranks = ranks[_sample_rows(n, m, seed).to(device)]
    return _sampled_score(ranks, n, k, per_item)

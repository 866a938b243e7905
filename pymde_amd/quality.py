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

A rank is 0-based and ties go to the smaller index: ``rank(i, j)`` is the number of rows ``l`` (other than
``i`` in a self-join) with ``(d2(i, l), l) < (d2(i, j), j)``, where ``d2`` is the float32 squared distance of
the Euclidean k-NN kernels, bit for bit.  The ranks of a search's own lists are therefore ``0 .. k - 1``.
"""
import collections
import math

import numpy as np
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

"""Edge-list preprocessing on the GPU: de-duplication and negative-edge sampling.

Same functions as the reference's ``pymde/preprocess/preprocess.py`` [ref: preprocess.py:11-138]
(``sample_edges``, ``dissimilar_edges``, ``deduplicate_edges``, ``scale``), running on
``csrc/mde_edges.hip`` (64-bit edge keys, rocPRIM radix sort / unique / select).  Differences:
  * results live on the GPU and are sorted by (i, j) (the reference returns sampled edges in draw
    order; order carries no meaning);
  * the sampler draws with a counter-based generator, so a given ``seed`` reproduces the same
    edges here but not the reference's NumPy stream -- parity is distributional (uniform over the
    complement, no duplicates, no excluded edge, requested count).
"""
import collections
import ctypes
import logging

import torch

from pymde_amd import _lib
from pymde_amd import ann as _ann
from pymde_amd import binary as _binary
from pymde_amd import metrics as _metrics
from pymde_amd import sparse as _sparse
from pymde_amd import util
from pymde_amd.pca import PrincipalComponents, principal_components  # noqa: F401  (public here)

_LOGGER = logging.getLogger("__pymde_amd__")   # problem.LOGGER

FLOAT32, BFLOAT16 = "float32", "bfloat16"
PRECISIONS = {"float32": FLOAT32, "fp32": FLOAT32, "f32": FLOAT32, "bfloat16": BFLOAT16, "bf16": BFLOAT16}
MAX_CANDIDATES = 64      # KNN_MAXK of csrc/mde_knn_tile.h: the longest shortlist


def resolve_precision(precision):
    """``"float32"`` or ``"bfloat16"`` for a ``precision=`` value or alias (case-insensitive); ``ValueError``
    for anything else.  Needs no device."""
    name = precision.strip().lower() if isinstance(precision, str) else precision
    if not isinstance(name, str) or name not in PRECISIONS:
        raise ValueError(f"unknown precision {precision!r}; the neighbour searches run in 'float32' (the default) "
                         "or 'bfloat16' (alias 'bf16': a bfloat16 shortlist re-ranked in float32)")
    return PRECISIONS[name]


def default_n_candidates(k, available=None):
    """The shortlist length of the bfloat16 search for ``k`` neighbours: ``min(64, max(2 k, k + 16))``, and no
    longer than the ``available`` corpus rows (but never shorter than ``k``)."""
    k = int(k)
    n_cand = min(MAX_CANDIDATES, max(2 * k, k + 16))
    if available is not None:
        n_cand = min(n_cand, max(int(available), k))
    return max(n_cand, k)


def _check_precision_arguments(precision, n_candidates, k, metric, approximate=False, graph=False):
    """The argument errors of the bfloat16 search that need no device; returns the canonical precision."""
    precision = resolve_precision(precision)
    if precision != BFLOAT16:
        if n_candidates is not None:
            raise ValueError("n_candidates is the shortlist length of precision='bfloat16'; the float32 search has "
                             "no shortlist")
        return precision
    if metric == _metrics.MANHATTAN:
        raise ValueError("precision='bfloat16' has no Manhattan search (the shortlist is a Gram product); the "
                         "metrics it serves are 'euclidean', 'cosine' and 'correlation'")
    if graph:
        raise ValueError("precision='bfloat16' applies to data matrices; a Graph has its own shortest-path search")
    if approximate:
        raise ValueError("precision='bfloat16' with approximate=True is not served: the inverted-file scan is "
                         "float32; use one or the other")
    if n_candidates is not None:
        n_candidates, k = int(n_candidates), int(k)
        if n_candidates < k or n_candidates > MAX_CANDIDATES:
            raise ValueError(f"n_candidates must lie in [k, {MAX_CANDIDATES}] (k = {k}, got {n_candidates})")
    return precision


def _resolve_n_candidates(n_candidates, k, available):
    """The shortlist length for ``k`` (already clamped to the rows available) neighbours."""
    if n_candidates is None:
        return default_n_candidates(k, available)
    n_candidates = int(n_candidates)
    if n_candidates < k or n_candidates > MAX_CANDIDATES:
        raise ValueError(f"n_candidates must lie in [k, {MAX_CANDIDATES}] (k = {k}, got {n_candidates})")
    return n_candidates


def _edges_on_device(edges, device=None):
    if not isinstance(edges, torch.Tensor):
        edges = torch.as_tensor(edges)
    if device is None:
        device = edges.device if edges.is_cuda else util.get_default_device()
    device = util.require_cuda_device(device)
    return edges.to(device=device, dtype=torch.int64).contiguous(), device


def _check_edge_call(rc):
    """``_lib.check`` for the edge-list functions: what they refuse as invalid -- an item outside ``[0, n_items)``
    above all, with a message naming the first such row -- is a ``ValueError``, as in the reference (which fails to
    build its ``(n, n)`` matrix there)."""
    if rc == _lib.MDE_E_INVALID:
        raise ValueError(_lib.last_error())
    _lib.check(rc)


def deduplicate_edges(edges, n_items=None):
    """Unique edges with ``e[0] <= e[1]``, sorted lexicographically [ref: preprocess.py:116-129].  ``ValueError``
    for a negative item or one that is not below ``n_items``."""
    edges, device = _edges_on_device(edges)
    p = edges.shape[0]
    if p == 0:
        return edges
    n = int(n_items) if n_items is not None else int(edges.max().item()) + 1
    n = max(n, 2)
    out = torch.empty_like(edges)
    count = ctypes.c_int64(0)
    lib = _lib.load()
    with torch.cuda.device(device):
        _check_edge_call(lib.mde_edges_deduplicate(n, p, _lib.ptr(edges), _lib.ptr(out), ctypes.byref(count),
                                                   _lib.stream_ptr(device)))
    return out[:count.value]


def sample_edges(n, num_edges, exclude=None, seed=None, device=None):
    """Randomly sample ``num_edges`` distinct edges (i < j), none of them in ``exclude``
    [ref: preprocess.py:11-80].  The result may hold fewer rows when the complement of
    ``exclude`` is almost exhausted (never when ``n`` is so small that the sampler enumerates the pairs:
    ``C(n, 2) <= 1.02 num_edges / (share of eligible pairs) + 1024``).  ``ValueError`` for an item of ``exclude``
    outside ``[0, n)``: its key would be another edge's."""
    n, num_edges = int(n), int(num_edges)
    ex = None
    if exclude is not None:
        ex, device = _edges_on_device(exclude, device)
    elif device is None:
        device = util.get_default_device()
    device = util.require_cuda_device(device)
    n_excluded = 0 if ex is None else int(ex.shape[0])
    n_all = n * (n - 1) // 2
    if num_edges > n_all - n_excluded:
        raise ValueError(
            f"Cannot sample more than ({n} choose 2) - {n_excluded} ="
            f"{n_all - n_excluded} edges. (requested: {num_edges} edges)")
    if seed is None:
        seed = int(util.np_rng().integers(0, 2 ** 63 - 1))
    out = torch.empty((max(num_edges, 1), 2), dtype=torch.int64, device=device)
    count = ctypes.c_int64(0)
    lib = _lib.load()
    with torch.cuda.device(device):
        _check_edge_call(lib.mde_sample_edges(n, num_edges, ctypes.c_uint64(int(seed) & (2 ** 64 - 1)),
                                              _lib.ptr(ex), n_excluded, _lib.ptr(out), ctypes.byref(count),
                                              _lib.stream_ptr(device)))
    return out[:count.value]


def dissimilar_edges(n_items, similar_edges, num_edges=None, seed=None):
    """Sample edges not in ``similar_edges`` (as many as ``similar_edges`` by default)
    [ref: preprocess.py:83-113]."""
    if num_edges is None:
        num_edges = similar_edges.shape[0]
    return sample_edges(n_items, num_edges, exclude=similar_edges, seed=seed)


def _neighbor_lists_to_graph(n, k, idx, values, max_value, device):
    """Directed neighbour lists [n, k] -> unique undirected edges with weights 1 / 2."""
    lib = _lib.load()
    pairs = torch.empty((n * k, 2), dtype=torch.int64, device=device)
    edges = torch.empty_like(pairs)
    weights = torch.empty(pairs.shape[0], dtype=torch.float32, device=device)
    count = ctypes.c_int64(0)
    with torch.cuda.device(device):
        _lib.check(lib.mde_knn_pairs(n, k, _lib.ptr(idx), _lib.ptr(values) if max_value is not None else None,
                                     float(max_value) if max_value is not None else 0.0,
                                     _lib.ptr(pairs), _lib.stream_ptr(device)))
        _lib.check(lib.mde_edges_count_unique(n, pairs.shape[0], _lib.ptr(pairs), _lib.ptr(edges),
                                              _lib.ptr(weights), ctypes.byref(count),
                                              _lib.stream_ptr(device)))
    return edges[:count.value], weights[:count.value]


def k_nearest_neighbors(data, k, max_distance=None, device=None, graph_distances=True, approximate=False,
                        n_lists=None, n_probe=None, seed=0, verbose=False, metric="euclidean",
                        precision="float32", n_candidates=None, n_refine=0):
    """Exact k-nearest-neighbour graph of the rows of a data matrix (Euclidean distance by default)
    [ref: preprocess/data_matrix.py:91-178] or of the nodes of a ``Graph`` (shortest-path metric,
    ``pymde_amd.graph.k_nearest_neighbors``) [ref: preprocess/generic.py dispatch].

    Returns ``(edges, weights)`` on the GPU: unique edges i < j sorted by (i, j); the weight is 2
    when i and j are neighbours of each other, 1 when only one is a neighbour of the other.
    Neighbours farther than ``max_distance`` do not count (an edge whose both directions are too
    long disappears).  The reference is exact (sklearn brute force) below 10 000 items and
    approximate (pynndescent) above; this search is exact at every size unless ``approximate=True``.
    Self matches are excluded by index, so duplicated rows become ordinary zero-distance neighbours.

    The kernels form ``|x|^2 + |y|^2 - 2 x.y`` in float32, which errs by ~1e-7 of ``|x|^2 + |y|^2``.  When
    the common offset of the rows dominates their spread (``|column means|^2`` above the summed column
    variance, both in double) the Euclidean search -- exact, approximate, densified sparse -- runs on a
    float32 copy of the rows minus their column means (each rounded to a power-of-two grid no coarser than the
    column's standard deviation, so integer data stay exact; ``4 n n_features`` bytes beside the data; DESIGN
    section 6); data near the origin are searched as given.  The exact sparse kernel cannot subtract a dense
    vector and keep its sparsity: a sparse matrix whose dense copy does not fit is searched untranslated and
    keeps the float32 error relative to its own norms.  That kernel sums a row's products one after the other,
    so its error grows with the number of stored entries: on non-negative values in [0.5, 2) it is 1.4e-7 of
    ``|x|^2 + |y|^2`` for rows of 5 entries, 2.7e-7 for 70 and 6.3e-7 for 300.  A row that
    holds NaN or infinity is a ``ValueError``
    naming the row, as in the reference (sklearn's ``check_array``).

    ``approximate=True`` searches data matrices of at least 10 000 rows by an inverted file on the GPU
    (``pymde_amd.ann``, ``csrc/mde_ann.hip``): k-means (``seed``) splits the rows into ``n_lists`` lists
    (default round(sqrt(n))), and each row is compared with the rows of the ``n_probe`` lists whose
    centroids are nearest to its own list's (default min(32, n_lists); ``n_probe >= n_lists`` probes every
    list and gives the exact graph).  Smaller inputs take the exact kernel.  Recall depends on the data:
    it is high on clustered data and can be poor on structureless data (an isotropic Gaussian); with
    ``verbose=True`` the sizes of the lists and a recall@k estimated from 1 000 sampled rows against the
    exact search are logged.  Sparse inputs are densified (an error if the dense copy does not fit);
    ``Graph`` inputs have no approximate search.

    ``n_refine`` (with ``approximate=True``; default 0) runs that many neighbour-of-neighbour passes over the
    lists of the inverted file (``ann.refine_lists``, ``csrc/mde_ann_refine.hip``): every row is offered the
    rows that list it and the lists of its forward and reverse neighbours, and keeps the k nearest.  A pass
    repairs the neighbours missed at the borders of the lists at a few hundred distances per row; it only
    ever replaces an entry by a nearer one, and it does not rescue a search that probes far too few lists.
    Every metric and input form of the approximate search takes it, ``max_distance`` applies afterwards and
    the logged recall is that of the refined lists.  With ``approximate=False`` it is a ``ValueError`` (an
    exact list is a fixed point of the pass); below 10 000 rows it is not used, like ``n_probe``.

    ``data`` is a dense ``np.ndarray`` / ``torch.Tensor`` [n, n_features], a sparse data matrix (a
    scipy sparse matrix of any format, or a torch sparse COO / CSR tensor; searched by the sparse
    kernel, or densified into the dense one where that is faster, ``_densify_sparse_knn``), or a
    ``Graph``.

    ``metric`` (data matrices only): ``"euclidean"`` (``"l2"``), ``"cosine"``, ``"correlation"`` or
    ``"manhattan"`` (``"l1"``, ``"cityblock"``), defined as in ``scipy.spatial.distance``; ``max_distance``
    is in the metric's own units and the weights keep their meaning.  Cosine and correlation search a
    normalised (centred and normalised) float32 copy of the data -- ``4 n n_features`` bytes beside the
    data -- with the Euclidean kernels, exact or approximate; a sparse matrix keeps its sparsity under
    cosine (its rows are scaled in place of a copy) and is densified under correlation and Manhattan (an
    error if the dense copy does not fit).  Manhattan has an exact kernel of its own and no approximate
    search.  A row without a direction (all zero under cosine, constant under correlation) is an error.
    See ``pymde_amd.metrics``.

    ``precision="bfloat16"`` (alias ``"bf16"``; data matrices, not Manhattan, not ``approximate=True``)
    selects the two-stage search (``mde_knn_bf16``): every pair is ranked by a bfloat16
    Gram product on the bfloat16 matrix cores, each row keeps a shortlist of ``n_candidates`` rows, and the
    shortlist is re-ranked with the float32 squared distances of the float32 search, bit for bit.  The result
    is the float32 result whenever the bfloat16 ranking keeps each row's true ``k`` nearest within its
    shortlist; a neighbour it misses is replaced by the next nearest one, and every returned distance is
    still the float32 distance of its pair.  ``n_candidates`` defaults to ``min(64, max(2 k, k + 16))`` (at
    most the other rows there are) and must lie in ``[k, 64]``: above k = 48 the margin shrinks below 16 and
    at k = 64 there is none, so recall falls below 1 there.  The bfloat16 copy is always of the rows minus
    their column means (on the grid of ``metrics.grid_means``): bfloat16 keeps 8 significant bits and an
    offset would use them up.  It takes ``2 n n_features`` bytes (rows padded to a multiple of 32) beside what
    the float32 search takes.  Data whose neighbours differ by less than bfloat16 resolves -- points on a
    line, say -- lose recall.  A sparse matrix is served when it is densified; one that would stay on the
    sparse kernel is an error.  ``verbose=True`` logs a recall@k estimated on 1 000 sampled rows against the
    float32 search.

    A ``BitMatrix`` (``pymde_amd.binary.pack``: bit-packed binary data) is searched exactly under its own Jaccard
    or Hamming distance by ``mde_bits_knn``; ``max_distance`` is in that distance's units.
    ``metric``, ``precision``, ``n_candidates``, ``approximate`` and ``n_refine`` stay at their defaults beside it (a
    ``ValueError`` otherwise); ``n_lists``, ``n_probe``, ``seed``, ``verbose`` and ``graph_distances`` have no effect
    on it."""
    idx, values, bound, _, _ = _neighbor_lists(data, k, max_distance, device, graph_distances, approximate, n_lists,
                                               n_probe, seed, verbose, metric, precision, n_candidates, n_refine)
    return _neighbor_lists_to_graph(idx.shape[0], idx.shape[1], idx, values, bound, idx.device)


def neighbor_graph(data, k, *, metric="euclidean", max_distance=None, connect=False, **search):
    """The k-nearest-neighbour graph of the rows of a data matrix as a ``Graph`` whose edge values are LENGTHS: the
    union of the directed neighbour lists of ``_neighbor_lists`` (``search``: every keyword of that search --
    ``device``, ``approximate``, ``n_lists``, ``n_probe``, ``seed``, ``verbose``, ``precision``, ``n_candidates``,
    ``n_refine``), each edge with the metric's distance of its two rows; an edge listed from both ends takes the
    smaller of the two values (they are the same pair computed twice and can differ in the last bits).  What
    ``graph.distances_from`` and ``LandmarkMDE.from_graph`` walk for Isomap.

    ``connect`` (default False: nothing changes): ``True`` or ``"pairs"`` joins every two connected components of
    that graph by their nearest pair of rows, ``"tree"`` joins them by the minimum spanning tree of those pairs
    (``connect_components``, whose ``Connection.graph`` is returned); not under Manhattan."""
    if _is_graph(data):
        raise ValueError("neighbor_graph takes a data matrix; a Graph is already a graph")
    if connect:
        _binary.refuse(data, "neighbor_graph(connect=...)")
        rule = resolve_connect(connect)
        if _metrics.resolve(metric) == _metrics.MANHATTAN:
            raise ValueError(_NO_MANHATTAN_WALK)
        graph = neighbor_graph(data, k, metric=metric, max_distance=max_distance, **search)
        return connect_components(data, graph, bridges=rule, metric=metric, device=search.get("device")).graph
    from pymde_amd import graph as _graph
    idx, values, bound, root, scale = _neighbor_lists(data, k, max_distance=max_distance, metric=metric, **search)
    n, device = int(idx.shape[0]), idx.device
    i = torch.arange(n, dtype=torch.int64, device=device).unsqueeze(1).expand_as(idx).reshape(-1)
    j = idx.reshape(-1).to(torch.int64)
    values = values.reshape(-1)
    keep = (j >= 0) & (j != i)
    if bound is not None:
        keep &= values <= bound
    i, j, values = i[keep], j[keep], values[keep]
    lengths = (values.clamp_min(0.0).sqrt() if root else values) * scale
    key = torch.minimum(i, j) * n + torch.maximum(i, j)
    uniq, inverse = torch.unique(key, sorted=True, return_inverse=True)
    # (Graph.from_edges would SUM the two listings of a mutual pair)
    shortest = torch.full((uniq.shape[0],), float("inf"), dtype=torch.float32, device=device)
    shortest.scatter_reduce_(0, inverse, lengths.to(torch.float32), reduce="amin")
    edges = torch.stack([uniq // n, uniq % n], dim=1).contiguous()
    return _graph.Graph._from_unique_edges(edges, shortest, n)


MAX_GROUPS = 1024        # GN_MAX_GROUPS of csrc/mde_group_nearest.hip: one LDS slot per group
PAIRS, TREE = "pairs", "tree"
_NO_MANHATTAN_WALK = ("the nearest pairs between groups have no Manhattan walk (the L1 tile has none); the metrics "
                      "served are 'euclidean', 'cosine' and 'correlation'")

GroupNearest = collections.namedtuple("GroupNearest", ["groups", "distance", "row"])
GroupNearest.__doc__ = """The nearest pairs between groups of rows (``nearest_between_groups``): ``groups`` the
distinct labels in ascending order [g]; ``distance`` float32 [g, g] in the metric's units, ``inf`` on the diagonal;
``row`` int64 [g, g]: the nearest pair of groups ``A`` and ``B`` is ``(row[A, B], row[B, A])``, -1 on the diagonal."""

Connection = collections.namedtuple("Connection", ["graph", "bridges", "lengths", "labels", "n_components"])
Connection.__doc__ = """A graph joined into one component (``connect_components``): ``graph`` the old edges with
their values plus the bridges; ``bridges`` int64 [b, 2] (``i < j``, sorted) and their ``lengths`` float32 [b];
``labels`` int64 [n] and ``n_components``: the components of the graph that came in."""


def resolve_connect(connect):
    """``"pairs"`` or ``"tree"`` for a ``connect=`` / ``bridges=`` value (``True`` is ``"pairs"``); ``ValueError``
    for anything else.  Needs no device."""
    if connect is True:
        return PAIRS
    name = connect.strip().lower() if isinstance(connect, str) else connect
    if not isinstance(name, str) or name not in (PAIRS, TREE):
        raise ValueError(f"unknown bridging rule {connect!r}; components are joined by 'pairs' (the nearest pair of "
                         "every two components; True means this) or 'tree' (the minimum spanning tree of those pairs)")
    return name


def _prepared_rows(data, metric, device, who):
    """The dense float32 rows on the GPU that the searches of ``_neighbor_lists`` run on under ``metric`` (a canonical
    name, not Manhattan): the translated copy for Euclidean data far from the origin, unit rows for cosine and
    correlation; a sparse matrix is densified (``ValueError`` when the dense copy does not fit)."""
    if _sparse.is_sparse(data):
        csr = _sparse.to_device_csr(data, device)
        if metric == _metrics.COSINE:
            csr = _metrics.normalized_csr(csr)
        if not _densify_sparse_knn(csr.n, csr.n_features, csr.nnz, csr.device):
            raise ValueError(f"{who} densifies sparse data, and the dense copy of this {csr.n} x {csr.n_features} "
                             "matrix does not fit in the device memory allowed for it")
        rows = csr.to_dense()
        if metric == _metrics.CORRELATION:
            rows = _metrics.normalized_rows(rows, metric)
    else:
        if not isinstance(data, torch.Tensor):
            data = torch.as_tensor(data)
        if data.dim() != 2:
            raise ValueError(f"`data` must be a matrix [n, n_features] (got shape {tuple(data.shape)})")
        if device is None:
            device = data.device if data.is_cuda else util.get_default_device()
        device = util.require_cuda_device(device)
        rows = data.to(device=device, dtype=torch.float32).contiguous()
        if metric != _metrics.EUCLIDEAN:
            rows = _metrics.normalized_rows(rows, metric)
    if metric == _metrics.EUCLIDEAN:
        rows, _ = _metrics.translated_rows(rows)
    return rows


def _group_nearest_table(rows, labels, groups, slices=0):
    """``(d2 float32 [groups, groups], row int32 [groups, groups])`` of ``mde_group_nearest`` for prepared dense
    float32 ``rows`` and int32 ``labels`` on the same GPU.  The C entry does not check the labels (they live on the
    device): one reduction here does, and a label outside ``[0, groups)`` is a ``ValueError``."""
    n, nf = int(rows.shape[0]), int(rows.shape[1])
    device = rows.device
    if labels.dim() != 1 or int(labels.shape[0]) != n:
        raise ValueError(f"`labels` must hold one label per row: {n} rows, labels of shape {tuple(labels.shape)}")
    labels = labels.to(device=device, dtype=torch.int32).contiguous()
    lo, hi = (int(v) for v in torch.aminmax(labels)) if n else (0, 0)
    if lo < 0 or hi >= int(groups):
        raise ValueError(f"`labels` must lie in [0, groups) = [0, {int(groups)}); it holds {lo if lo < 0 else hi}")
    lib = _lib.load()
    d2 = torch.empty((groups, groups), dtype=torch.float32, device=device)
    row = torch.empty((groups, groups), dtype=torch.int32, device=device)
    with torch.cuda.device(device):
        nbytes = int(lib.mde_group_nearest_work_bytes(n, groups, slices))
        if nbytes < 0:
            _lib.check(nbytes)
        work = torch.empty(nbytes, dtype=torch.uint8, device=device)
        _lib.check(lib.mde_group_nearest(n, nf, _lib.ptr(rows), _lib.ptr(labels), groups, slices, _lib.ptr(d2),
                                         _lib.ptr(row), _lib.ptr(work), _lib.stream_ptr(device)))
    return d2, row


def nearest_between_groups(data, labels, *, metric="euclidean", device=None, slices=0):
    """For a data matrix and a group label per row, the nearest pair of rows between every two groups
    (``mde_group_nearest``): a ``GroupNearest(groups, distance, row)``.  With one label per row --
    classes, clusters, the components of a neighbour graph -- ``distance`` is the single-linkage distance matrix
    between the groups, and ``(row[A, B], row[B, A])`` the pair that realises it.

    ``labels``: any integers, one per row; they are compacted (``torch.unique``) and ``groups`` lists them in
    ascending order.  ``distance`` is in the metric's own units, as ``neighbor_graph`` reports lengths, and a pair's
    value has the bits the k-NN searches give that pair; ties go to the smaller row of the group with the smaller
    label, then to the smaller row of the other.  ``data`` is prepared as the searches prepare it: rows minus their
    column means for Euclidean data far from the origin, unit rows for cosine and correlation; a sparse matrix is
    densified (``ValueError`` if the dense copy does not fit).  The walk forms no distance inside a group and each
    pair of groups once.  ``slices``: the candidate split of the walk, 0 = automatic; the result does not depend on
    it.  ``ValueError`` under ``"manhattan"`` (the L1 tile has no such walk), for a ``Graph``, for labels of the
    wrong length or type, for a single group and for more than 1024."""
    _binary.refuse(data, "nearest_between_groups")
    metric = _metrics.resolve(metric)
    if metric == _metrics.MANHATTAN:
        raise ValueError(_NO_MANHATTAN_WALK)
    if _is_graph(data):
        raise ValueError("nearest_between_groups measures between the rows of a data matrix; a Graph has no rows")
    if not isinstance(labels, torch.Tensor):
        import numpy as np
        labels = torch.as_tensor(np.asarray(labels))
    labels = labels.detach().reshape(-1)
    if labels.dtype == torch.bool or labels.is_floating_point() or labels.is_complex():
        raise ValueError(f"`labels` must be integers, got dtype {labels.dtype}")
    if not hasattr(data, "shape") or len(data.shape) != 2:
        raise ValueError("`data` must be a matrix [n, n_features]")
    n = int(data.shape[0])
    if int(labels.shape[0]) != n:
        raise ValueError(f"`labels` must hold one label per row: `data` has {n} rows and `labels` {int(labels.shape[0])}")
    rows = _prepared_rows(data, metric, device, "nearest_between_groups")
    groups, compact = torch.unique(labels.to(rows.device), sorted=True, return_inverse=True)
    g = int(groups.shape[0])
    if g < 2:
        raise ValueError("nearest_between_groups needs at least two groups; `labels` holds one distinct value")
    if g > MAX_GROUPS:
        raise ValueError(f"nearest_between_groups serves at most {MAX_GROUPS} groups; `labels` holds {g} distinct "
                         "values")
    d2, row = _group_nearest_table(rows, compact, g, int(slices))
    root, scale = (True, 1.0) if metric == _metrics.EUCLIDEAN else (False, 0.5)
    distance = (d2.clamp_min(0.0).sqrt() if root else d2) * scale
    distance.fill_diagonal_(float("inf"))
    return GroupNearest(groups, distance, row.to(torch.int64))


def _spanning_tree_pairs(d2, row):
    """The ``g - 1`` pairs ``(A, B)``, ``A < B``, of the minimum spanning tree of the complete graph on the groups
    under the key ``(d2[A, B], row[A, B], row[B, A])`` (Kruskal on the host: at most 1024 groups).  Keys are distinct
    (no two pairs of groups share a pair of rows), so the tree is unique."""
    import numpy as np
    d2, row = d2.cpu().numpy(), row.cpu().numpy()
    g = d2.shape[0]
    A, B = np.triu_indices(g, 1)
    order = np.lexsort((row[B, A], row[A, B], d2[A, B]))
    parent = list(range(g))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    chosen = []
    for e in order:
        ra, rb = find(int(A[e])), find(int(B[e]))
        if ra != rb:
            parent[ra] = rb
            chosen.append((int(A[e]), int(B[e])))
            if len(chosen) == g - 1:
                break
    return chosen


def connect_components(data, graph, *, bridges="pairs", metric="euclidean", device=None, slices=0):
    """Join the connected components of ``graph`` -- a graph on the rows of ``data``, usually their neighbour graph
    -- by bridges between nearest rows: a ``Connection(graph, bridges, lengths, labels, n_components)``.

    The components come from ``graph.connected_components``; with one component the input graph object itself is
    returned, with no bridge, and nothing else runs.  Otherwise ``nearest_between_groups`` finds the nearest pair of
    rows of every two components under ``metric``, and ``bridges="pairs"`` (the default) adds all ``c (c - 1) / 2``
    of them, the rule of ``sklearn.manifold.Isomap``; ``"tree"`` adds the ``c - 1`` pairs of the minimum spanning
    tree of the components under the key ``(distance, row, row)``.  Under ``"tree"`` a geodesic between two
    components may run through a third and overstate their distance; ``"pairs"`` bounds every inter-component
    distance by a direct bridge.  The new ``Graph`` holds the old edges with their old values, bit for
    bit, and the bridges with their lengths in the metric's units.  ``ValueError`` when ``data`` and ``graph``
    disagree on the number of rows, under ``"manhattan"``, and for more than 1024 components (use a larger
    ``n_neighbors``)."""
    from pymde_amd import graph as _graph
    rule = resolve_connect(bridges)
    _binary.refuse(data, "connect_components")
    metric = _metrics.resolve(metric)
    if metric == _metrics.MANHATTAN:
        raise ValueError(_NO_MANHATTAN_WALK)
    if not isinstance(graph, _graph.Graph):
        raise ValueError("`graph` must be a pymde_amd.Graph instance.")
    if _is_graph(data) or not hasattr(data, "shape"):
        raise ValueError("`data` must be the data matrix whose rows are the nodes of `graph`")
    n = int(graph.n_items)
    if int(data.shape[0]) != n:
        raise ValueError(f"`data` has {int(data.shape[0])} rows and `graph` has {n} nodes; they must agree")
    count, labels = _graph.connected_components(graph)
    dev = labels.device
    if count == 1:
        return Connection(graph, torch.empty((0, 2), dtype=torch.int64, device=dev),
                          torch.empty(0, dtype=torch.float32, device=dev), labels, 1)
    if count > MAX_GROUPS:
        raise ValueError(f"the graph has {count} connected components and at most {MAX_GROUPS} can be joined; a "
                         "larger n_neighbors gives fewer components")
    rows = _prepared_rows(data, metric, dev if device is None else device, "connect_components")
    d2, row = _group_nearest_table(rows, labels, count, int(slices))
    if rule == PAIRS:
        A, B = torch.triu_indices(count, count, 1, device=dev)
    else:
        A, B = torch.as_tensor(_spanning_tree_pairs(d2, row), dtype=torch.int64, device=dev).T
    a, b, value = row[A, B].to(torch.int64), row[B, A].to(torch.int64), d2[A, B]
    root, scale = (True, 1.0) if metric == _metrics.EUCLIDEAN else (False, 0.5)
    lengths = (value.clamp_min(0.0).sqrt() if root else value) * scale
    key, order = torch.sort(torch.minimum(a, b) * n + torch.maximum(a, b))
    lengths = lengths[order].contiguous()
    new_edges = torch.stack([key // n, key % n], dim=1).contiguous()
    # a bridge joins two components, so it is no edge of the graph: the merge is a sort of distinct keys
    old = graph.edges.to(dev)
    merged, where = torch.sort(torch.cat([old[:, 0] * n + old[:, 1], key]))
    values = torch.cat([graph.distances.to(dev), lengths])[where].contiguous()
    edges = torch.stack([merged // n, merged % n], dim=1).contiguous()
    return Connection(_graph.Graph._from_unique_edges(edges, values, n), new_edges, lengths, labels, count)


def _neighbor_lists(data, k, max_distance=None, device=None, graph_distances=True, approximate=False,
                    n_lists=None, n_probe=None, seed=0, verbose=False, metric="euclidean",
                    precision="float32", n_candidates=None, n_refine=0):
    """The list-producing half of ``k_nearest_neighbors`` (same arguments, same errors): the directed neighbour
    lists of whichever search serves ``data``, ``(idx [n, k] int32, values [n, k] float32, bound, root, scale)``.
    ``idx`` holds -1 in an empty slot; an entry with ``values > bound`` (``bound`` is ``max_distance`` in the
    units of ``values``, None without one or when the search applied it itself) does not count; the metric's
    distance of an entry is ``scale * (sqrt(values) if root else values)``: ``(True, 1.0)`` for the Euclidean
    searches, which rank by the squared distance, ``(False, 0.5)`` for cosine and correlation (the squared
    chord of the unit rows), ``(False, 1.0)`` for Manhattan and for a ``Graph``."""
    if _binary.is_bits(data):
        return _bits_neighbor_lists(data, k, max_distance, device, approximate, metric, precision, n_candidates,
                                    n_refine)
    metric = _metrics.resolve(metric)
    _metrics.check_approximate(metric, approximate)
    precision = _check_precision_arguments(precision, n_candidates, k, metric, approximate, _is_graph(data))
    n_refine = _ann.check_n_refine(n_refine)
    if n_refine and not approximate:
        raise ValueError("n_refine refines the lists of approximate=True; the exact search has nothing to refine "
                         "(an exact list is a fixed point of the pass)")
    if hasattr(data, "edges") and hasattr(data, "n_items") and not isinstance(data, torch.Tensor):
        _metrics.check_graph(metric)
        if approximate:
            raise ValueError("approximate=True applies to data matrices; a Graph has no approximate search")
        from pymde_amd import graph as _graph
        idx, dist = _graph._neighbor_lists(data, k, graph_distances=graph_distances, max_distance=max_distance)
        return idx, dist, None, False, 1.0
    if metric != _metrics.EUCLIDEAN:
        idx, values, bound = _metric_knn_lists(data, k, metric, max_distance, device, approximate, n_lists,
                                               n_probe, seed, verbose, precision, n_candidates, n_refine)
        return idx, values, bound, False, 1.0 if metric == _metrics.MANHATTAN else 0.5
    if _sparse.is_sparse(data):
        csr = _sparse.to_device_csr(data, device)
        k = _clamp_k(k, csr.n)
        if approximate:
            _ann.resolve_params(csr.n, n_lists, n_probe)
        if approximate and csr.n >= _ann.MIN_ITEMS:
            if not _densify_sparse_knn(csr.n, csr.n_features, csr.nnz, csr.device):
                raise ValueError(
                    f"approximate=True densifies sparse data, and the dense copy of this {csr.n} x "
                    f"{csr.n_features} matrix does not fit in the device memory allowed for it; "
                    "use approximate=False (the exact sparse kernel)")
            idx, d2 = _euclidean_knn_lists(csr.to_dense(), k, True, n_lists, n_probe, seed, verbose,
                                           n_refine=n_refine)
        elif _densify_sparse_knn(csr.n, csr.n_features, csr.nnz, csr.device):
            idx, d2 = _euclidean_knn_lists(csr.to_dense(), k, verbose=verbose, precision=precision,
                                           n_candidates=n_candidates)
        elif precision == BFLOAT16:
            raise ValueError(_BF16_SPARSE_DOES_NOT_FIT.format(n=csr.n, nf=csr.n_features))
        else:
            _check_finite_csr(csr)
            idx, d2 = _sparse_knn_lists(csr, k)
        max_d2 = None if max_distance is None else float(max_distance) ** 2
        return idx, d2, max_d2, True, 1.0
    if not isinstance(data, torch.Tensor):
        data = torch.as_tensor(data)
    if device is None:
        device = data.device if data.is_cuda else util.get_default_device()
    device = util.require_cuda_device(device)
    data = data.to(device=device, dtype=torch.float32).contiguous()
    n = int(data.shape[0])
    k = _clamp_k(k, n)
    if approximate:
        _ann.resolve_params(n, n_lists, n_probe)      # the same argument checks at every size
    idx, d2 = _euclidean_knn_lists(data, k, approximate, n_lists, n_probe, seed, verbose, precision, n_candidates,
                                   n_refine)
    max_d2 = None if max_distance is None else float(max_distance) ** 2
    return idx, d2, max_d2, True, 1.0


def _check_bits_search(metric, approximate, precision, n_candidates, n_refine=0):
    """The argument errors of a search on a ``BitMatrix`` (they need no device): ``metric=`` at its default, no
    approximate search, no bfloat16 shortlist."""
    _binary.check_metric(metric)
    if approximate or n_refine:
        raise ValueError("approximate=True applies to float data matrices; a BitMatrix has no approximate search "
                         "(the inverted file's k-means lists are Euclidean)")
    if resolve_precision(precision) != FLOAT32 or n_candidates is not None:
        raise ValueError("precision='bfloat16' and n_candidates apply to float data matrices; a BitMatrix is "
                         "searched exactly, in integers")


def _bits_neighbor_lists(bits, k, max_distance, device, approximate, metric, precision, n_candidates, n_refine):
    """``_neighbor_lists`` of a ``BitMatrix``: the exact self-join of ``mde_bits_knn`` under the matrix's own
    distance; the values are the distances themselves (``root=False, scale=1.0``).  ``approximate``, ``n_refine``,
    a ``precision`` other than float32 and ``n_candidates`` are refused; the knobs that only steer those searches
    or a ``Graph`` -- ``n_lists``, ``n_probe``, ``seed``, ``verbose``, ``graph_distances`` -- have no effect here,
    as ``n_lists`` / ``n_probe`` have none on float data without ``approximate=True``."""
    _check_bits_search(metric, approximate, precision, n_candidates, n_refine)
    if device is not None:
        bits = bits.to(util.require_cuda_device(device))
    k = _clamp_k(k, bits.shape[0])
    idx, dist = _binary.knn_lists(bits, bits, k, self_join=True)
    return idx, dist, None if max_distance is None else float(max_distance), False, 1.0


_BF16_SPARSE_DOES_NOT_FIT = (
    "precision='bfloat16' densifies sparse data, and the dense copy of this {n} x {nf} matrix does not fit in "
    "the device memory allowed for it; use precision='float32' (the exact sparse kernel)")


def _metric_knn_lists(data, k, metric, max_distance=None, device=None, approximate=False, n_lists=None,
                      n_probe=None, seed=0, verbose=False, precision=FLOAT32, n_candidates=None, n_refine=0):
    """Directed neighbour lists of a data matrix under cosine, correlation or Manhattan (a canonical name):
    ``(idx [n, k] int32, values [n, k], bound)``.  ``values`` are what the kernels rank by -- the squared
    chord ``d2 = 2 (1 - cos)`` of the unit rows for cosine / correlation, the distance itself for Manhattan
    -- and ``bound`` is ``max_distance`` in those units (None without one): the lists become a graph
    without a pass that converts them."""
    sparse_kernel = metric == _metrics.COSINE    # the others need the dense copy
    csr = None
    if _sparse.is_sparse(data):
        csr = _sparse.to_device_csr(data, device)
        n, device = csr.n, csr.device
        if metric == _metrics.COSINE:
            csr = _metrics.normalized_csr(csr)
        needs_dense = not sparse_kernel or (approximate and n >= _ann.MIN_ITEMS)
        if _densify_sparse_knn(csr.n, csr.n_features, csr.nnz, device):
            data, csr = csr.to_dense(), None
        elif needs_dense:
            raise ValueError(
                f"metric='{metric}'" + (" with approximate=True" if sparse_kernel else "") + " densifies sparse "
                f"data, and the dense copy of this {csr.n} x {csr.n_features} matrix does not fit in the device "
                "memory allowed for it; " + ("use approximate=False (the exact sparse kernel)" if sparse_kernel
                                             else "metric='cosine' and 'euclidean' have a sparse kernel"))
    else:
        if not isinstance(data, torch.Tensor):
            data = torch.as_tensor(data)
        if device is None:
            device = data.device if data.is_cuda else util.get_default_device()
        device = util.require_cuda_device(device)
        data = data.to(device=device, dtype=torch.float32).contiguous()
        n = int(data.shape[0])
        if metric == _metrics.COSINE:
            data = _metrics.normalized_rows(data, metric)
    if metric == _metrics.CORRELATION:
        data = _metrics.normalized_rows(data, metric)
    k = _clamp_k(k, n)
    if approximate:
        _ann.resolve_params(n, n_lists, n_probe)
    if metric == _metrics.MANHATTAN:
        idx, values = _metrics.manhattan_knn_lists(data, k)
    elif csr is not None:
        if precision == BFLOAT16:
            raise ValueError(_BF16_SPARSE_DOES_NOT_FIT.format(n=csr.n, nf=csr.n_features))
        idx, values = _sparse_knn_lists(csr, k)
    elif approximate and n >= _ann.MIN_ITEMS:
        idx, values = _approximate_knn_lists(data, k, n_lists, n_probe, seed, verbose, n_refine)
    elif precision == BFLOAT16:
        # the unit rows are searched as they are by the float32 kernel; the bfloat16 copy is centred
        idx, values = _bf16_self_search(data, k, n_candidates, _bf16_mu(data), verbose, seed)
    else:
        idx, values = _dense_knn_lists(data, k)
    if max_distance is None:
        return idx, values, None
    return idx, values, float(max_distance) * (1.0 if metric == _metrics.MANHATTAN else 2.0)


def _clamp_k(k, n):
    k = int(k)
    if k > n - 1:
        k = n - 1
    if k < 1:
        raise ValueError("k must be at least 1")
    return k


def _euclidean_knn_lists(data, k, approximate=False, n_lists=None, n_probe=None, seed=0, verbose=False,
                         precision=FLOAT32, n_candidates=None, n_refine=0):
    """Directed Euclidean neighbour lists (idx [n, k] int32, d2 [n, k]) of a dense float32 [n, nf] on the GPU:
    what ``k_nearest_neighbors`` calls for Euclidean data.  The search -- exact, or the inverted file with its
    recall estimate when ``approximate`` and n >= ``ann.MIN_ITEMS`` -- runs on the rows minus their float64
    column means when the offset of the data dominates its spread (``metrics.translated_rows``, DESIGN
    section 6), on ``data`` itself otherwise.  ``ValueError`` for a row that holds NaN or infinity, before
    any list is produced.  ``precision=BFLOAT16``: the two-stage search on the same float32 rows, its bfloat16
    copy centred whether or not the float32 rows are (``_bf16_rows``)."""
    if precision == BFLOAT16:
        rows, mu, _ = _bf16_rows(data)
        return _bf16_self_search(rows, k, n_candidates, mu, verbose, seed)
    data, _ = _metrics.translated_rows(data)
    if approximate and int(data.shape[0]) >= _ann.MIN_ITEMS:
        return _approximate_knn_lists(data, k, n_lists, n_probe, seed, verbose, n_refine)
    return _dense_knn_lists(data, k)


def _check_finite_csr(csr):
    """``ValueError`` naming the first row of a ``sparse.DeviceCSR`` that stores a NaN or an infinity."""
    bad = ~torch.isfinite(csr.values)
    if bool(bad.any()):
        entry = bad.nonzero()[0]
        row = int(torch.searchsorted(csr.indptr, entry, right=True).item()) - 1
        _metrics.raise_non_finite(row, "the data matrix")


def _dense_knn_lists(data, k):
    """Directed neighbour lists (idx [n, k] int32, d2 [n, k]) of a dense float32 [n, nf] on the GPU by
    ``mde_knn`` on the rows as given (``_euclidean_knn_lists`` translates them first where that matters)."""
    n, nf = int(data.shape[0]), int(data.shape[1])
    device = data.device
    lib = _lib.load()
    idx = torch.empty((n, k), dtype=torch.int32, device=device)
    d2 = torch.empty((n, k), dtype=torch.float32, device=device)
    sqn = torch.empty(n, dtype=torch.float32, device=device)
    with torch.cuda.device(device):
        _lib.check(lib.mde_knn(n, nf, _lib.ptr(data), k, _lib.ptr(idx), _lib.ptr(d2), _lib.ptr(sqn),
                               _lib.stream_ptr(device)))
    return idx, d2


def _bf16_mu(data, what="the data matrix"):
    """The float64 [nf] vector on the device by which the bfloat16 copy of a search of the corpus ``data``
    (dense float32 on the GPU) is centred: its column means on the grid of ``metrics.grid_means``."""
    mean, var = _metrics.column_stats(data, what)
    return _metrics.grid_means(mean, var).to(data.device)


def _bf16_rows(data, what="the data matrix"):
    """What the bfloat16 search of the corpus ``data`` (dense float32 on the GPU) runs on: ``(rows, mu,
    shift)``.  ``rows`` are the float32 rows of the float32 search -- ``data`` minus ``shift``, the grid column
    means, when ``metrics.translation_pays``, ``data`` itself (``shift`` None) otherwise -- and ``mu`` is what
    remains to be subtracted for the bfloat16 copy: None for rows that are centred already, the grid column
    means otherwise.  ``ValueError`` for a row that holds NaN or infinity."""
    mean, var = _metrics.column_stats(data, what)
    mu = _metrics.grid_means(mean, var).to(data.device)
    if _metrics.translation_pays(mean, var):
        return _metrics.subtract_columns(data, mu), None, mu
    return data, mu, None


def _knn_bf16(queries, data, self_join, k, n_candidates, mu, slices):
    n_q, n_c, nf = int(queries.shape[0]), int(data.shape[0]), int(data.shape[1])
    device = data.device
    lib = _lib.load()
    idx = torch.empty((n_q, k), dtype=torch.int32, device=device)
    d2 = torch.empty((n_q, k), dtype=torch.float32, device=device)
    if mu is not None:
        mu = mu.to(device=device, dtype=torch.float64).contiguous()
    with torch.cuda.device(device):
        nbytes = int(lib.mde_knn_bf16_work_bytes(n_q, n_c, nf, k, n_candidates, slices))
        if nbytes < 0:
            _lib.check(nbytes)
        work = torch.empty(nbytes, dtype=torch.uint8, device=device)
        _lib.check(lib.mde_knn_bf16(n_q, n_c, nf, _lib.ptr(queries), _lib.ptr(data), _lib.ptr(mu), int(self_join), k,
                                    n_candidates, slices, _lib.ptr(idx), _lib.ptr(d2), _lib.ptr(work),
                                    _lib.stream_ptr(device)))
    return idx, d2


def _dense_knn_lists_bf16(data, k, n_candidates=None, mu=None, slices=0):
    """``_dense_knn_lists`` by the two-stage search ``mde_knn_bf16``: the bfloat16 shortlist of ``n_candidates``
    per row (default ``default_n_candidates``) of the rows minus ``mu`` (float64 [nf]; None: the rows as
    given), re-ranked with the float32 distances of ``mde_knn`` on ``data`` itself."""
    k = int(k)
    n_candidates = _resolve_n_candidates(n_candidates, k, int(data.shape[0]) - 1)
    return _knn_bf16(data, data, True, k, n_candidates, mu, slices)


def _cross_knn_lists_bf16(queries, data, k, n_candidates=None, mu=None, slices=0):
    """``_cross_knn_lists`` by the two-stage search ``mde_knn_bf16``; ``mu`` centres the bfloat16 copies of
    both matrices."""
    k = int(k)
    n_candidates = _resolve_n_candidates(n_candidates, k, int(data.shape[0]))
    return _knn_bf16(queries, data, False, k, n_candidates, mu, slices)


def _bf16_self_search(rows, k, n_candidates, mu, verbose=False, seed=0):
    idx, d2 = _dense_knn_lists_bf16(rows, k, n_candidates, mu)
    if verbose:
        n_cand = _resolve_n_candidates(n_candidates, k, int(rows.shape[0]) - 1)
        recall = _estimated_recall(rows, idx, k, seed=seed)
        _LOGGER.info(f"bfloat16 {k}-NN: shortlist of {n_cand} per row, estimated recall@{k} {recall:.4f} against "
                     "the float32 search (1000 sampled rows)")
    return idx, d2


def _is_graph(data):
    return hasattr(data, "edges") and hasattr(data, "n_items") and not isinstance(data, torch.Tensor)


def _dense_rows_for_cross(data, device, what):
    """The dense float32 [n, nf] copy on ``device`` of one argument of ``cross_nearest_neighbors``."""
    if _sparse.is_sparse(data):
        csr = _sparse.to_device_csr(data, device)
        if not _densify_sparse_knn(csr.n, csr.n_features, csr.nnz, csr.device):
            raise ValueError(
                f"cross_nearest_neighbors densifies sparse data, and the dense copy of the {csr.n} x "
                f"{csr.n_features} `{what}` matrix does not fit in the device memory allowed for it")
        return csr.to_dense()
    if not isinstance(data, torch.Tensor):
        data = torch.as_tensor(data)
    if data.dim() != 2:
        raise ValueError(f"`{what}` must be a matrix [n, n_features] (got shape {tuple(data.shape)})")
    return data.to(device=device, dtype=torch.float32).contiguous()


def _translated_pair(queries, data):
    """The two dense float32 matrices a Euclidean cross search runs on: both minus the float64 column means
    of the corpus ``data`` when its offset dominates its spread (one vector for both, so every distance is
    kept; ``metrics.translated_rows``), the matrices themselves otherwise.  ``ValueError`` naming the argument
    and the row when either holds a NaN or an infinity."""
    if int(queries.shape[0]):
        _metrics.check_finite(queries, "`queries`")
    data, mu = _metrics.translated_rows(data, "`data`")
    if mu is not None and int(queries.shape[0]):
        queries = _metrics.subtract_columns(queries, mu)
    return queries, data


def _cross_knn_lists(queries, data, k, slices=0):
    """(idx [n_q, k] int32, d2 [n_q, k]) of ``mde_knn_cross``: for every row of the dense float32 ``queries``
    its k nearest rows of the dense float32 ``data`` (same GPU), ordered by (d2, index); empty slots
    (``data`` has fewer than k rows) hold -1 / FLT_MAX.  ``slices``: the corpus split, 0 = automatic."""
    n_q, n_c, nf = int(queries.shape[0]), int(data.shape[0]), int(data.shape[1])
    device = data.device
    lib = _lib.load()
    idx = torch.empty((n_q, k), dtype=torch.int32, device=device)
    d2 = torch.empty((n_q, k), dtype=torch.float32, device=device)
    with torch.cuda.device(device):
        nbytes = int(lib.mde_knn_cross_work_bytes(n_q, n_c, k, slices))
        if nbytes < 0:
            _lib.check(nbytes)
        work = torch.empty(nbytes, dtype=torch.uint8, device=device)
        _lib.check(lib.mde_knn_cross(n_q, n_c, nf, _lib.ptr(queries), _lib.ptr(data), k, slices, _lib.ptr(idx),
                                     _lib.ptr(d2), _lib.ptr(work), _lib.stream_ptr(device)))
    return idx, d2


def cross_nearest_neighbors(queries, data, k, max_distance=None, metric="euclidean", device=None,
                            precision="float32", n_candidates=None):
    """For every row of ``queries`` [n_q, n_features] its ``k`` nearest rows of ``data`` [n_c, n_features]:
    the exact query-against-corpus search (``mde_knn_cross``).  The reference leaves
    this search to the user; here it is what ``recipes.extend_embedding`` places new points with.

    Returns ``(idx int64 [n_q, k], dist float32 [n_q, k])`` on the GPU, each row ascending; ties go to the
    smaller row of ``data``.  ``dist`` is in the metric's own units (Euclidean: the distance, not its
    square; cosine / correlation: ``1 - cos`` of the (centred) rows).  Nothing is excluded as "self": a
    query that equals a row of ``data`` lists it at distance 0.  Slots beyond ``max_distance`` (in the
    metric's units), and slots beyond the number of rows of ``data`` when ``k`` exceeds it, hold -1 / +inf.

    ``queries`` and ``data`` are dense ``np.ndarray`` / ``torch.Tensor`` or sparse data matrices (scipy
    sparse, torch sparse COO / CSR); sparse inputs are densified (an error if the dense copy does not fit
    in the device memory allowed for it, ``_densify_sparse_knn``).  ``metric``: ``"euclidean"``,
    ``"cosine"`` or ``"correlation"`` (and their aliases); cosine and correlation normalise the two matrices
    separately and search the unit rows with the Euclidean kernel, and a row without a direction in either
    matrix is an error.  The Euclidean search runs on both matrices minus the column means of ``data`` when
    that offset dominates the spread of ``data`` (as in ``k_nearest_neighbors``), and a row of either matrix
    that holds NaN or infinity is a ``ValueError`` naming the argument and the row.  There is no Manhattan cross kernel and no approximate cross search; a ``Graph``
    is not a data matrix.

    ``precision="bfloat16"`` and ``n_candidates`` as in ``k_nearest_neighbors``: a bfloat16 shortlist of
    ``n_candidates`` rows of ``data`` per query (default ``min(64, max(2 k, k + 16))``, at most the rows of
    ``data``), re-ranked with the float32 distances of the float32 search; the bfloat16 copies of both
    matrices are centred at the column means of ``data``.

    Two ``BitMatrix`` arguments of equal ``n_features`` and ``distance`` are searched by ``mde_bits_knn`` under
    that distance (the other keywords at their defaults); one ``BitMatrix`` beside a float matrix is a
    ``ValueError``."""
    if _binary.is_bits(queries) or _binary.is_bits(data):
        return _bits_cross_nearest_neighbors(queries, data, k, max_distance, metric, device, precision, n_candidates)
    metric = _metrics.resolve(metric)
    precision = _check_precision_arguments(precision, n_candidates, k, metric,
                                           graph=_is_graph(queries) or _is_graph(data))
    if metric == _metrics.MANHATTAN:
        raise ValueError("cross_nearest_neighbors has no Manhattan kernel; the metrics it serves are "
                         "'euclidean', 'cosine' and 'correlation'")
    if _is_graph(queries) or _is_graph(data):
        raise ValueError("cross_nearest_neighbors searches data matrices; a Graph has no rows to search")
    for name, m in (("queries", queries), ("data", data)):
        if not hasattr(m, "shape") or len(m.shape) != 2:
            raise ValueError(f"`{name}` must be a matrix [n, n_features]")
    if int(queries.shape[1]) != int(data.shape[1]):
        raise ValueError(f"`queries` has {int(queries.shape[1])} features and `data` has {int(data.shape[1])}; "
                         "they must agree")
    k = int(k)
    if k < 1:
        raise ValueError("k must be at least 1")
    n_q, n_c = int(queries.shape[0]), int(data.shape[0])
    if n_c < 1:
        raise ValueError("`data` needs at least one row")
    if device is None:
        on_gpu = [m.device for m in (data, queries) if isinstance(m, torch.Tensor) and m.is_cuda]
        device = on_gpu[0] if on_gpu else util.get_default_device()
    device = util.require_cuda_device(device)
    Q = _dense_rows_for_cross(queries, device, "queries")
    C = _dense_rows_for_cross(data, device, "data")
    mu = None
    if metric != _metrics.EUCLIDEAN:
        if n_q:
            Q = _metrics.normalized_rows(Q, metric)
        C = _metrics.normalized_rows(C, metric)
        if precision == BFLOAT16:
            mu = _bf16_mu(C, "`data`")
    elif precision == BFLOAT16:
        if n_q:
            _metrics.check_finite(Q, "`queries`")
        C, mu, shift = _bf16_rows(C, "`data`")
        if shift is not None and n_q:
            Q = _metrics.subtract_columns(Q, shift)
    else:
        Q, C = _translated_pair(Q, C)
    if n_q == 0:
        return (torch.empty((0, k), dtype=torch.int64, device=device),
                torch.empty((0, k), dtype=torch.float32, device=device))
    if precision == BFLOAT16:
        idx32, d2 = _cross_knn_lists_bf16(Q, C, k, n_candidates, mu)
    else:
        idx32, d2 = _cross_knn_lists(Q, C, k)
    dist = d2.sqrt() if metric == _metrics.EUCLIDEAN else 0.5 * d2
    empty = idx32 < 0
    if max_distance is not None:
        empty = empty | ~(dist <= float(max_distance))
    idx = idx32.to(torch.int64)
    idx[empty] = -1
    dist[empty] = float("inf")
    return idx, dist


def _bits_cross_nearest_neighbors(queries, data, k, max_distance, metric, device, precision, n_candidates):
    """``cross_nearest_neighbors`` of two ``BitMatrix`` arguments (equal ``n_features`` and ``distance``)."""
    _check_bits_search(metric, False, precision, n_candidates)
    _binary.check_pair(queries, data)
    k = int(k)
    if k < 1:
        raise ValueError("k must be at least 1")
    n_q, n_c = queries.shape[0], data.shape[0]
    if n_c < 1:
        raise ValueError("`data` needs at least one row")
    device = util.require_cuda_device(data.device if device is None else device)
    queries, data = queries.to(device), data.to(device)
    if n_q == 0:
        return (torch.empty((0, k), dtype=torch.int64, device=device),
                torch.empty((0, k), dtype=torch.float32, device=device))
    idx32, dist = _binary.knn_lists(queries, data, k)
    empty = idx32 < 0
    if max_distance is not None:
        empty = empty | ~(dist <= float(max_distance))
    idx = idx32.to(torch.int64)
    idx[empty] = -1
    dist[empty] = float("inf")
    return idx, dist


def _approximate_knn_lists(data, k, n_lists, n_probe, seed, verbose, n_refine=0):
    """Directed neighbour lists of a dense float32 [n, nf] on the GPU by the inverted-file search and
    ``n_refine`` neighbour-of-neighbour passes over its lists."""
    n_lists, n_probe = _ann.resolve_params(int(data.shape[0]), n_lists, n_probe)
    if k > _ann.MAX_K:      # the exact kernel's error, before any work
        raise _lib.MdeHipError(_lib.MDE_E_INVALID, "mde_ann_search: invalid arguments (1 <= k <= %d)" % _ann.MAX_K)
    stats = {} if verbose else None
    with torch.cuda.device(data.device):
        idx, d2 = _ann.knn_lists(data, k, n_lists=n_lists, n_probe=n_probe, seed=seed, timings=stats,
                                 n_refine=n_refine)
    if verbose:
        sizes = stats["list_sizes"].double()
        _LOGGER.info(
            f"approximate {k}-NN: {n_lists} lists (sizes min {int(sizes.min())}, median "
            f"{int(sizes.median())}, max {int(sizes.max())}), {n_probe} probed per list, "
            f"{stats['candidate_pairs'] / float(data.shape[0]) ** 2:.3f} of all pairs scanned in "
            f"{stats['tiles']} tiles (estimated load imbalance {stats['imbalance']:.2f})")
        if n_refine:
            _LOGGER.info(f"approximate {k}-NN: {len(stats['refine_changed'])} refinement pass(es) changed "
                         f"{stats['refine_changed']} rows")
        recall = _estimated_recall(data, idx, k, seed=seed)
        _LOGGER.info(f"approximate {k}-NN: estimated recall@{k} {recall:.3f} (1000 sampled rows)")
    return idx, d2


def _estimated_recall(data, idx, k, n_samples=1000, seed=0):
    """Recall@k of neighbour lists idx [n, k] of dense float32 data on the GPU, estimated on ``n_samples``
    seeded random rows against the exact query-against-base search."""
    with torch.cuda.device(data.device):
        return _ann.sampled_recall(data, idx, k, n_samples=n_samples, seed=seed)


def _sparse_knn_lists(csr, k):
    """Directed neighbour lists of a ``sparse.DeviceCSR`` by the sparse kernel."""
    device = csr.device
    lib = _lib.load()
    idx = torch.empty((csr.n, k), dtype=torch.int32, device=device)
    d2 = torch.empty((csr.n, k), dtype=torch.float32, device=device)
    sqn = torch.empty(csr.n, dtype=torch.float32, device=device)
    with torch.cuda.device(device):
        _lib.check(lib.mde_sparse_knn(csr.n, csr.n_features, csr.nnz, _lib.ptr(csr.indptr), _lib.ptr(csr.indices),
                                      _lib.ptr(csr.values), k, _lib.ptr(idx), _lib.ptr(d2), _lib.ptr(sqn),
                                      _lib.stream_ptr(device)))
    return idx, d2


# Sparse k-NN dispatcher.  Both kernels cost ~n^2: the dense one per feature, the sparse one per stored
# entry plus a fixed price per feature window.  Measured at k = 15 (tools/sparse_knn_scale.py,
# profiles/r07_sparse_knn.txt): the dense MFMA kernel runs ~73 TFLOP/s, the sparse kernel 0.04-1.5 TFMA/s
# (per query x stored entry), so densifying wins at every recorded shape whose dense copy fits -- 70k x 784
# at 17 %: 0.12 s against 0.44 s; 100k x 20k at 4.9 %: 5.4 s against 12.5 s; 400k x 20k at 2 %: 74 s against
# 143 s; 100k x 100k at 0.1 %: 27.3 s against 27.5 s.  The sparse kernel serves the
# inputs whose dense copy does not fit in DENSIFY_MAX_FRACTION of the free device memory.
DENSIFY_DENSITY = 0.0
DENSIFY_MAX_FRACTION = 0.25   # the dense copy may take at most this share of the free device memory


def _densify_sparse_knn(n, nf, nnz, device):
    """True when the sparse data matrix should be densified into the dense k-NN kernel."""
    if nnz < DENSIFY_DENSITY * float(n) * float(nf):
        return False
    free, _ = torch.cuda.mem_get_info(device)
    return 4.0 * n * nf <= DENSIFY_MAX_FRACTION * free


def _rms(distances):
    return distances.pow(2).mean().sqrt()


def scale(distances, natural_length):
    """Rescale distances so that their RMS equals ``natural_length`` [ref: preprocess.py:132-138]."""
    return (natural_length / _rms(distances)) * distances

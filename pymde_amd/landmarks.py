"""Landmark selection on the GPU: farthest-point (maxmin) and k-means++ (D^2) sampling of the rows of a data matrix
(``csrc/mde_landmarks.hip``).

A uniform draw follows the density of the data: a small group far from the bulk usually gets no landmark, and
landmark MDS then never sees that part of the space.  Farthest-point selection takes, one after the other, the row
farthest from the landmarks chosen so far -- the classic choice for landmark MDS; k-means++ draws the next row with
probability proportional to its squared distance to them, which is less drawn to single outliers.  Both cost one
pass over the data per landmark, and how well ``m`` landmarks cover the data is the covering radius: the largest
distance from a row to its nearest landmark (``LandmarkSelection.distance.max()``).

``select_graph`` is farthest-point selection among the nodes of a ``Graph`` under its shortest-path metric (one
``graph.distances_from`` solve per landmark).

``LandmarkMDE(..., selection=...)`` and ``preserve_distances(..., landmarks=m, landmark_selection=...)`` use it.
"""
import collections

import torch

from pymde_amd import _lib, util
from pymde_amd import binary as _binary
from pymde_amd import graph as _graph
from pymde_amd import metrics as _metrics
from pymde_amd import preprocess as _preprocess
from pymde_amd import quality as _quality

FARTHEST, KMEANSPP = "farthest", "kmeans++"
UNIFORM = "uniform"
_METHODS = {FARTHEST: 0, KMEANSPP: 1}
_ALIASES = {"farthest": FARTHEST, "kmeans++": KMEANSPP, "k-means++": KMEANSPP}
_METRICS = (_metrics.EUCLIDEAN, _metrics.COSINE, _metrics.CORRELATION)

LandmarkSelection = collections.namedtuple("LandmarkSelection", ["indices", "radius", "nearest", "distance"])
LandmarkSelection.__doc__ = """What ``select`` returns, all on the GPU: ``indices`` int64 [m], the chosen rows in
selection order; ``radius`` float32 [m], the distance of each chosen row to the rows chosen before it (``inf`` at
position 0); ``nearest`` int64 [n], the position in ``indices`` of every row's nearest landmark (ties to the earlier
one); ``distance`` float32 [n], the distance to it (0 for the landmarks).  ``distance.max()`` is the covering radius."""


def resolve_method(method):
    """Canonical name of a selection method of ``select``; ``ValueError`` otherwise."""
    name = _ALIASES.get(method.lower()) if isinstance(method, str) else None
    if name is None:
        raise ValueError(f"Unknown landmark selection method {method!r}; the methods are 'farthest' and 'kmeans++' "
                         "(alias 'k-means++')")
    return name


def resolve_selection(selection):
    """``"uniform"`` or a method of ``select``, as ``LandmarkMDE(selection=...)`` takes them."""
    if isinstance(selection, str) and selection.lower() == UNIFORM:
        return UNIFORM
    try:
        return resolve_method(selection)
    except ValueError:
        raise ValueError(f"Unknown landmark selection {selection!r}; the selections are 'uniform', 'farthest' and "
                         "'kmeans++' (alias 'k-means++')") from None


def _check_source(data, metric):
    _binary.refuse(data, "landmarks.select")
    metric = _metrics.resolve(metric)
    if _preprocess._is_graph(data):
        raise ValueError("landmarks are selected among the rows of a data matrix; a Graph has no rows (the metrics "
                         "supported are 'euclidean', 'cosine' and 'correlation' on a data matrix)")
    if metric not in _METRICS:
        raise ValueError(f"metric={metric!r} has no landmark selection kernel; the metrics supported are "
                         "'euclidean', 'cosine' and 'correlation'")
    return metric


def check_arguments(data, m, method, metric, start):
    """The argument checks of ``select``, before any device is required: ``(method, metric, n, m, start)``."""
    method = resolve_method(method)
    metric = _check_source(data, metric)
    _quality._check_matrix(data, "data")
    n = int(data.shape[0])
    if isinstance(m, bool) or int(m) != m:
        raise ValueError(f"`m` must be a number of rows (an int), got {m!r}")
    m = int(m)
    if not 1 <= m <= n:
        raise ValueError(f"`m` must lie in [1, n] = [1, {n}], got {m}")
    if int(data.shape[1]) < 1:
        raise ValueError("`data` needs at least one feature")
    if start is not None:
        if isinstance(start, bool) or int(start) != start:
            raise ValueError(f"`start` must be a row index (an int), got {start!r}")
        start = int(start)
        if not 0 <= start < n:
            raise ValueError(f"`start` must lie in [0, n) = [0, {n}), got {start}")
    return method, metric, n, m, start


def _select_rows(rows, m, method, start, seed):
    """``mde_select_landmarks`` on prepared dense float32 rows on one GPU: ``(idx int32 [m], radius2 [m], mind2 [n],
    nearest int32 [n])``, the squared distances of the kernel as they come."""
    n, nf, device = int(rows.shape[0]), int(rows.shape[1]), rows.device
    lib = _lib.load()
    idx = torch.empty(m, dtype=torch.int32, device=device)
    radius2 = torch.empty(m, dtype=torch.float32, device=device)
    mind2 = torch.empty(n, dtype=torch.float32, device=device)
    nearest = torch.empty(n, dtype=torch.int32, device=device)
    with torch.cuda.device(device):
        work = _lib.work_buffer(lib.mde_select_landmarks_work_bytes, n, nf, m, device=device)
        _lib.check(lib.mde_select_landmarks(n, nf, _lib.ptr(rows), m, _METHODS[method], int(start),
                                            int(seed) & 0xFFFFFFFFFFFFFFFF, _lib.ptr(idx), _lib.ptr(radius2),
                                            _lib.ptr(mind2), _lib.ptr(nearest), _lib.ptr(work),
                                            _lib.stream_ptr(device)))
    return idx, radius2, mind2, nearest


def select(data, m, method="farthest", metric="euclidean", start=None, seed=None, device=None):
    """``m`` distinct rows of ``data`` [n, n_features] to serve as landmarks, chosen one after the other on the GPU:
    a ``LandmarkSelection(indices, radius, nearest, distance)``.

    ``method="farthest"``: every further landmark is the row farthest from the landmarks chosen so far (ties to the
    smallest row); ``radius`` is then non-increasing from position 1 on, and ``radius[t]`` is the covering radius of
    the first ``t`` landmarks.  ``method="kmeans++"`` (alias ``"k-means++"``): the next row is drawn with probability
    proportional to its squared distance to the landmarks so far (D^2 sampling), from ``seed``.  A row that equals a
    landmark is at distance exactly 0 and is taken only when nothing else is left, so the ``m`` rows are distinct
    even when ``data`` has fewer than ``m`` distinct rows.

    ``data`` is prepared as a self-join search prepares it: a dense or sparse data matrix, Euclidean rows translated
    when they lie far from the origin, unit rows for ``"cosine"`` / ``"correlation"`` (whose distance ``1 - cos`` is
    half the squared distance of the unit rows, and monotone in it); NaN / inf rows and rows without a direction are
    that path's ``ValueError``.  ``metric``: ``"euclidean"``, ``"cosine"`` or ``"correlation"`` (and their aliases);
    Manhattan and a ``Graph`` are a ``ValueError``.  ``radius`` and ``distance`` are in the metric's units.

    ``start``: the first landmark, an int in ``[0, n)``; ``None`` draws it from ``seed``
    (``quality._sample_rows(n, 1, seed)``).  ``seed=None`` draws one from ``util.np_rng()``.  The same arguments
    give the same bits on every run."""
    method, metric, n, m, start = check_arguments(data, m, method, metric, start)
    if seed is None:
        seed = int(util.np_rng().integers(0, 2 ** 63 - 1))
    seed = int(seed)
    if start is None:
        start = int(_quality._sample_rows(n, 1, seed)[0])
    if device is None:
        device = data.device if isinstance(data, torch.Tensor) and data.is_cuda else util.get_default_device()
    device = util.require_cuda_device(device)
    rows = _quality._self_rows(data, metric, device, "data")
    idx, radius2, mind2, nearest = _select_rows(rows, m, method, start, seed)
    if metric == _metrics.EUCLIDEAN:
        radius, distance = radius2.sqrt_(), mind2.sqrt_()
    else:
        radius, distance = radius2.mul_(0.5), mind2.mul_(0.5)
    return LandmarkSelection(idx.to(torch.int64), radius, nearest.to(torch.int64), distance)


def _check_count(m, n, what="m"):
    if isinstance(m, bool) or int(m) != m:
        raise ValueError(f"`{what}` must be a number of nodes (an int), got {m!r}")
    m = int(m)
    if not 1 <= m <= n:
        raise ValueError(f"`{what}` must lie in [1, n] = [1, {n}], got {m}")
    return m


def select_graph(graph, m, start=None, seed=None, max_length=None):
    """``m`` distinct nodes of a ``Graph`` chosen by farthest-point selection under its shortest-path metric: the
    ``LandmarkSelection(indices, radius, nearest, distance)`` of ``select``, with path lengths for distances.

    Every step is one single-source ``graph.distances_from`` solve from the node just chosen, a running minimum and
    an arg-max; ties go to the smallest node index.  A node no landmark reaches (none within ``max_length``, if given)
    is at distance ``inf`` and is therefore taken next: every component of the graph gets a landmark before any gets
    a second one, and ``radius`` is ``inf`` at those positions (and at position 0).  ``start`` and ``seed`` as in
    ``select``.  k-means++ has no graph form here."""
    if not isinstance(graph, _graph.Graph):
        raise ValueError("`graph` must be a pymde_amd.Graph instance; the rows of a data matrix go to `select`")
    n = int(graph.n_items)
    m = _check_count(m, n)
    if start is not None:
        if isinstance(start, bool) or int(start) != start:
            raise ValueError(f"`start` must be a node index (an int), got {start!r}")
        start = int(start)
        if not 0 <= start < n:
            raise ValueError(f"`start` must lie in [0, n) = [0, {n}), got {start}")
    if seed is None:
        seed = int(util.np_rng().integers(0, 2 ** 63 - 1))
    if start is None:
        start = int(_quality._sample_rows(n, 1, int(seed))[0])
    plan, w = _graph._path_lengths(graph)
    device = plan.device
    inf = float("inf")
    order = torch.arange(n, dtype=torch.int64, device=device)
    distance = torch.full((n,), inf, dtype=torch.float32, device=device)
    nearest = torch.zeros(n, dtype=torch.int64, device=device)
    chosen = torch.zeros(n, dtype=torch.bool, device=device)
    indices = torch.empty(m, dtype=torch.int64, device=device)
    radius = torch.empty(m, dtype=torch.float32, device=device)
    node = torch.tensor([start], dtype=torch.int64, device=device)
    for t in range(m):
        indices[t] = node[0]
        radius[t] = distance[node[0]]
        chosen[node[0]] = True
        d = _graph._distances_from(plan, w, node, max_length).reshape(-1)
        closer = d < distance                     # (strict: ties stay with the earlier landmark)
        nearest[closer] = t
        distance = torch.minimum(distance, d)
        # the farthest node not chosen yet; among equals the smallest index, whatever argmax would return
        score = torch.where(chosen, torch.full_like(distance, -1.0), distance)
        node = torch.where(score == score.max(), order, n).min().reshape(1)
    return LandmarkSelection(indices, radius, nearest, distance)

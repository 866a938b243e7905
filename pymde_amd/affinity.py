"""Edge weights from the distances of neighbour lists: perplexity and UMAP affinities on the GPU.

``preprocess.k_nearest_neighbors`` weighs an edge 1, or 2 when its two rows list each other; the distances the
searches return play no part.  This module turns the same directed lists into the weights of the two methods
this package is compared with (``csrc/mde_affinity.hip``):

  * ``calibrate`` gives every row a kernel over its own entries: t-SNE's Gaussian, its bandwidth set so that the
    row's conditional distribution has a given perplexity, or UMAP's exponential of the distance beyond the
    nearest neighbour, its scale set so that the row's memberships sum to ``log2(k)``;
  * ``symmetrize`` combines the two directions of every undirected edge, by the mean (t-SNE) or the
    probabilistic union (UMAP), into exactly the edges ``k_nearest_neighbors`` returns for those lists;
  * ``neighbor_affinities`` runs a search, the calibration and the symmetrisation in one call.

Out of scope: a fixed-bandwidth heat kernel, UMAP's ``local_connectivity`` other than 1 and its
``set_op_mix_ratio``, t-SNE's global normalisation and early exaggeration, lists longer than 64.
"""
import collections
import ctypes

import torch

from pymde_amd import _lib
from pymde_amd import preprocess
from pymde_amd import util

PERPLEXITY, UMAP = "perplexity", "umap"
KINDS = {PERPLEXITY: 0, UMAP: 1}
MEAN, UNION = "mean", "union"
RULES = {MEAN: 0, UNION: 1}
DEFAULT_RULE = {PERPLEXITY: MEAN, UMAP: UNION}
MAX_K = preprocess.MAX_CANDIDATES      # KNN_MAXK: the longest list

Calibration = collections.namedtuple("Calibration", ["idx", "conditionals", "bandwidth", "offset"])
Calibration.__doc__ = """What ``calibrate`` returns, all on the GPU: ``idx`` int32 [n, k] (the lists with -1 at every
entry that does not count), ``conditionals`` float32 [n, k] (0 there), and per row ``bandwidth`` (perplexity: the
Gaussian's ``beta``; umap: ``sigma``) and ``offset`` (perplexity: the nearest kept distance; umap: ``rho``)."""
NeighborAffinities = collections.namedtuple("NeighborAffinities", ["edges", "weights", "calibration"])
NeighborAffinities.__doc__ = """What ``neighbor_affinities`` returns: ``edges`` int64 [m, 2] (i < j, sorted by
(i, j)), their float32 ``weights`` and the ``Calibration`` they were symmetrised from."""


def resolve_kind(kind):
    """``"perplexity"`` or ``"umap"`` for a ``kind=`` value (case-insensitive); ``ValueError`` otherwise."""
    name = kind.strip().lower() if isinstance(kind, str) else kind
    if not isinstance(name, str) or name not in KINDS:
        raise ValueError(f"unknown affinity kind {kind!r}; the kinds are 'perplexity' and 'umap'")
    return name


def resolve_rule(rule, kind=PERPLEXITY):
    """``"mean"`` or ``"union"`` for a ``symmetrize=`` value; None gives the default of ``kind`` (mean for
    perplexity, union for umap); ``ValueError`` for anything else."""
    if rule is None:
        return DEFAULT_RULE[kind]
    name = rule.strip().lower() if isinstance(rule, str) else rule
    if not isinstance(name, str) or name not in RULES:
        raise ValueError(f"unknown symmetrisation rule {rule!r}; the rules are 'mean' and 'union'")
    return name


def resolve_perplexity(kind, perplexity, k=None):
    """The perplexity ``calibrate`` uses: ``perplexity`` (a positive finite number), ``k / 3`` when it is None
    (None when ``k`` is None too: not known yet); with ``kind="umap"`` it must be None.  Needs no device."""
    if kind == UMAP:
        if perplexity is not None:
            raise ValueError("perplexity belongs to kind='perplexity'; kind='umap' calibrates every row to log2(k)")
        return None
    if perplexity is None:
        return None if k is None else int(k) / 3.0
    perplexity = float(perplexity)
    if not (perplexity > 0.0) or perplexity == float("inf"):
        raise ValueError(f"perplexity must be a positive finite number (got {perplexity})")
    return perplexity


WEIGHT_KEYS = ("kind", "perplexity", "symmetrize")
# the keywords of preprocess.k_nearest_neighbors that neighbor_affinities passes on to the search
_SEARCH_KEYS = {"approximate", "n_lists", "n_probe", "n_refine", "seed", "precision", "n_candidates", "verbose",
                "device", "graph_distances"}


def parse_weights(weights):
    """``(kind, perplexity, rule)`` for the ``weights=`` value of a recipe -- ``"perplexity"``, ``"umap"`` or a dict
    with the keys ``kind``, ``perplexity`` and ``symmetrize`` -- or None for None.  ``perplexity`` stays None where
    the default ``k / 3`` applies.  ``ValueError`` for anything else; needs no device."""
    if weights is None:
        return None
    if isinstance(weights, dict):
        unknown = set(weights) - set(WEIGHT_KEYS)
        if unknown:
            raise ValueError(f"weights: unknown keys {sorted(unknown, key=str)}; the keys are 'kind', 'perplexity' "
                             "and 'symmetrize'")
        kind = resolve_kind(weights.get("kind", PERPLEXITY))
        perplexity, rule = weights.get("perplexity"), weights.get("symmetrize")
    elif isinstance(weights, str):
        kind, perplexity, rule = resolve_kind(weights), None, None
    else:
        raise ValueError("weights must be None, 'perplexity', 'umap' or a dict {'kind': .., 'perplexity': .., "
                         "'symmetrize': ..}")
    return kind, resolve_perplexity(kind, perplexity), resolve_rule(rule, kind)


def _lists_on_device(idx, values, what):
    if not isinstance(idx, torch.Tensor) or not isinstance(values, torch.Tensor):
        raise ValueError(f"`idx` and `{what}` must be torch tensors on the GPU")
    if idx.dim() != 2 or tuple(values.shape) != tuple(idx.shape):
        raise ValueError(f"`idx` and `{what}` must both be [n, k] (got {tuple(idx.shape)} and {tuple(values.shape)})")
    n, k = int(idx.shape[0]), int(idx.shape[1])
    if n < 1 or k < 1 or k > MAX_K:
        raise ValueError(f"neighbour lists must be [n, k] with n >= 1 and 1 <= k <= {MAX_K} (got [{n}, {k}])")
    device = util.require_cuda_device(idx.device)
    return (idx.to(dtype=torch.int32).contiguous(), values.to(device=device, dtype=torch.float32).contiguous(),
            n, k, device)


def calibrate(idx, values, kind="perplexity", *, perplexity=None, root=False, scale=1.0, max_value=None):
    """Calibrate one kernel per row over directed neighbour lists: ``idx`` int32 [n, k] (-1 = empty slot) and
    ``values`` float32 [n, k] on the GPU, ``k <= 64``.  The metric's distance of an entry is
    ``d = scale * (sqrt(values) if root else values)``, formed in double (negative values under ``root`` count as
    0): ``root=True`` for the squared Euclidean distances the Euclidean searches return, ``scale=0.5`` for the
    squared chords of the cosine and correlation searches.  An entry with ``values > max_value`` (in the units of
    ``values``), with an index outside ``[0, n)`` or with the index of its own row does not count, like an empty
    slot.  With ``k_i`` the entries of row i that count:

    ``kind="perplexity"`` (``perplexity > 0``, default ``k / 3``): ``p_j = exp(-beta s_j) / sum`` with
    ``s_j = d_j^2 - min_j d_j^2`` and ``beta >= 0`` the root of ``-sum p log p = log(perplexity)``.  With ``c`` the
    entries at the minimum: ``perplexity >= k_i`` or ``c == k_i`` gives the uniform ``1 / k_i`` and ``beta = 0``;
    ``perplexity <= c`` gives ``1 / c`` on those entries, 0 elsewhere and ``beta = inf``.

    ``kind="umap"``: ``p_j = exp(-max(d_j - rho, 0) / sigma)`` with ``rho`` the smallest positive distance of the
    row (0 when it has none) and ``sigma`` the root of ``sum_j p_j = log2(k_i)``, raised to at least
    ``1e-3 * mean_j d_j``.  With ``c`` the entries at or below ``rho``: ``c == k_i`` gives all ones, and
    ``log2(k_i) <= c`` has its root at ``sigma -> 0``, so ``sigma`` is that floor.

    Every row is computed in double, summed in a fixed order and rounded to float32 once; the roots are bisected
    until the bracket is below 2^-48 of its upper end.  The result has the same bits on every run.  A row without
    entries holds zeros.  Returns a ``Calibration``."""
    kind = resolve_kind(kind)
    idx, values, n, k, device = _lists_on_device(idx, values, "values")
    perplexity = resolve_perplexity(kind, perplexity, k)
    scale = float(scale)
    if not (scale > 0.0) or scale == float("inf"):
        raise ValueError(f"scale must be a positive finite number (got {scale})")
    if max_value is not None:
        max_value = float(max_value)
        if max_value != max_value:
            raise ValueError("max_value must not be NaN")
    idx_out = torch.empty_like(idx)
    p = torch.empty((n, k), dtype=torch.float32, device=device)
    bandwidth = torch.empty(n, dtype=torch.float32, device=device)
    offset = torch.empty(n, dtype=torch.float32, device=device)
    lib = _lib.load()
    with torch.cuda.device(device):
        _lib.check(lib.mde_knn_calibrate(n, k, _lib.ptr(idx), _lib.ptr(values), int(bool(root)), scale,
                                         int(max_value is not None), 0.0 if max_value is None else max_value,
                                         KINDS[kind], 0.0 if perplexity is None else perplexity, _lib.ptr(idx_out),
                                         _lib.ptr(p), _lib.ptr(bandwidth), _lib.ptr(offset),
                                         _lib.stream_ptr(device)))
    return Calibration(idx_out, p, bandwidth, offset)


def symmetrize(idx, conditionals, rule="mean"):
    """The undirected edges of directed neighbour lists with the two directions' conditionals combined.  ``idx``
    int32 [n, k] and ``conditionals`` float32 [n, k] are those of a ``Calibration``: -1 marks a slot that does
    not count, the other entries of a row are distinct and none is the row itself.  For the edge {i, j} let ``a``
    be the conditional of j in row i (0 when i does not list j) and ``b`` that of i in row j:

      * ``rule="mean"``: ``0.5 * (a + b)`` in float32 (t-SNE);
      * ``rule="union"``: ``a + b - a b`` in double, rounded to float32 (UMAP's fuzzy union).

    Returns ``(edges int64 [m, 2], weights float32 [m])`` with i < j, sorted by (i, j), each edge once: the edges
    of ``preprocess.k_nearest_neighbors`` on the same lists, bit for bit.  An edge whose weight underflows to 0
    stays in."""
    rule = resolve_rule(rule)
    idx, conditionals, n, k, device = _lists_on_device(idx, conditionals, "conditionals")
    edges = torch.empty((n * k, 2), dtype=torch.int64, device=device)
    weights = torch.empty(n * k, dtype=torch.float32, device=device)
    count = ctypes.c_int64(0)
    lib = _lib.load()
    with torch.cuda.device(device):
        _lib.check(lib.mde_knn_symmetrize(n, k, _lib.ptr(idx), _lib.ptr(conditionals), RULES[rule], _lib.ptr(edges),
                                          _lib.ptr(weights), ctypes.byref(count), _lib.stream_ptr(device)))
    return edges[:count.value], weights[:count.value]


_symmetrize = symmetrize      # (``neighbor_affinities`` has a keyword of that name)


def neighbor_affinities(data, k, kind="perplexity", *, perplexity=None, symmetrize=None, max_distance=None,
                        metric="euclidean", **search):
    """Search the ``k`` nearest neighbours of every row of ``data``, calibrate the lists and symmetrise them.

    ``data``, ``k``, ``max_distance`` and ``metric`` are those of ``preprocess.k_nearest_neighbors`` (a dense or
    sparse data matrix, or a ``Graph``), and ``**search`` takes its other keywords: ``approximate``, ``n_lists``,
    ``n_probe``, ``n_refine``, ``seed``, ``precision``, ``n_candidates``, ``verbose``, ``device``, ``graph_distances``.
    The distances
    are the metric's own -- the Euclidean distance rather than its square, ``1 - cos`` for cosine and correlation
    -- and a neighbour beyond ``max_distance`` does not count.  ``kind`` and ``perplexity`` as for ``calibrate``;
    ``symmetrize`` is ``"mean"`` or ``"union"`` (default: mean for perplexity, union for umap).

    Returns ``NeighborAffinities(edges, weights, calibration)``; ``edges`` are the edges
    ``preprocess.k_nearest_neighbors`` returns for the same arguments."""
    kind = resolve_kind(kind)
    rule = resolve_rule(symmetrize, kind)
    resolve_perplexity(kind, perplexity)
    unknown = set(search) - _SEARCH_KEYS
    if unknown:
        raise ValueError(f"neighbor_affinities: unknown keywords {sorted(unknown)}; the search takes "
                         f"{sorted(_SEARCH_KEYS)}")
    idx, values, bound, root, scale = preprocess._neighbor_lists(data, k, max_distance=max_distance, metric=metric,
                                                                 **search)
    calibration = calibrate(idx, values, kind, perplexity=perplexity, root=root, scale=scale, max_value=bound)
    edges, weights = _symmetrize(calibration.idx, calibration.conditionals, rule)
    return NeighborAffinities(edges, weights, calibration)


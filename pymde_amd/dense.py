"""Dense MDE problems: a loss of ``pymde_amd.losses`` over ALL ``n (n - 1) / 2`` pairs, without an edge list
(``csrc/mde_pair_loss.hip``).  The reference has no such problem class: its ``MDE`` needs the
edges, 16 bytes each, and a data structure over them.

``DenseMDE`` is ``MDE(n, d, all_edges(n), loss(deviations))`` in O(n) memory beside its deviations.  These come from a
data matrix -- every evaluation forms the distances on the fly with the Gram tile of the exact k-NN search, as
``quality.pair_moments`` does, so metric MDS of 100 000 rows needs no 40 GB of pairs -- or from a precomputed
``distance_matrix`` (sklearn's ``dissimilarity="precomputed"``), which is read once per evaluation.  What
``quality.stress`` measures, ``DenseMDE(data, loss=losses.Quadratic)`` minimises.

The solver is the one ``MDE.embed`` calls (``optim.lbfgs``), on its generic path: the objective is a
``torch.autograd.Function`` around ``mde_pair_loss``, the constraint any ``Constraint``.

``DensePlacement`` is the rectangular form (``mde_pair_loss_cross``): the loss of every (new row,
embedded row) pair with the embedded rows held fixed, which places new rows into a finished distance-preserving
embedding.  ``LandmarkMDE`` (``preserve_distances(landmarks=m)``) is landmark MDS on the two: a ``DenseMDE`` of m
landmark rows, then a ``DensePlacement`` of all the others against them.

``weights=`` gives every pair a weight: a number ``p`` weighs by ``D^-p`` (``Quadratic`` with
``weights=1`` is Sammon mapping), a matrix weighs pair by pair, and a zero in it is a MISSING pair -- an incomplete
dissimilarity matrix, or the pairs of a ``Graph`` that no path joins (``DenseMDE.from_graph``).
"""
import collections
import math
import numbers

import numpy as np
import torch

from pymde_amd import _lib
from pymde_amd import binary as _binary
from pymde_amd import classical as _classical
from pymde_amd import constraints
from pymde_amd import graph as _graph
from pymde_amd import landmarks as _landmarks
from pymde_amd import metrics as _metrics
from pymde_amd import optim
from pymde_amd import preprocess
from pymde_amd import problem as _problem
from pymde_amd import quality
from pymde_amd import rows as _rows
from pymde_amd import util
from pymde_amd.functions import function as _function
from pymde_amd.functions import losses

MAX_DIM = 8            # PAIR_LOSS_MAX_D of csrc/mde_pair_loss.hip
MAX_SLICES = 65535     # CROSS_MAX_SLICES of csrc/mde_knn_slices.h
SYMMETRY_RTOL = 1e-5   # |D - D^T| may reach this fraction of the largest entry (a float32 product of two roundings)
_FIRST_LOSS = _function.KIND["L_QUADRATIC"]
W_NONE, W_POWER, W_MATRIX = 0, 1, 2   # MDE_PAIR_W_* of include/mde_hip.h

Weights = collections.namedtuple("Weights", ["source", "p", "W"])
Weights.__doc__ = """The ``weights=`` of a dense problem as the kernels take it: ``source`` (MDE_PAIR_W_*), the exponent
``p`` of the power form, and ``W``, the matrix of the matrix form (as it was passed, until the problem puts it on its
device as float32)."""
NO_WEIGHTS = Weights(W_NONE, 0.0, None)

INITS = ("random", "classical")                     # the `init=` of DenseMDE and LandmarkMDE
PLACEMENT_INITS = ("neighbors", "triangulation")    # the `init` of DensePlacement


def check_init(init, accepted=INITS, name="init"):
    """``init`` if it is one of ``accepted``; ``ValueError`` otherwise (no device is needed to say so)."""
    if not isinstance(init, str) or init not in accepted:
        raise ValueError(f"`{name}` must be one of {', '.join(repr(a) for a in accepted)}; got {init!r}")
    return init

WeightStats = collections.namedtuple("WeightStats", ["nonfinite", "negative", "kept", "empty_rows", "bad_deviations",
                                                     "asymmetry", "largest", "deviation_asymmetry",
                                                     "largest_deviation", "row_kept"])
WeightStats.__doc__ = """What ``mde_pair_weights_check`` reports of a weight matrix (and the deviations it weighs)."""


def parse_weights(weights, shape=None, allow_matrix=True):
    """The ``Weights`` of a ``weights=`` argument; needs no GPU.  ``None``: no weights.  A real number ``p`` (not a
    bool; finite, ``>= 0``): the power form ``w = D^-p``.  A two-dimensional numpy array or torch tensor (bool,
    integer or floating point): the matrix form, which must have the shape ``shape``.  ``ValueError`` otherwise, and
    for a matrix where ``allow_matrix`` is false."""
    if weights is None:
        return NO_WEIGHTS
    accepted = ("`weights` is None, a real number p >= 0 (every pair is weighed by D^-p), or a matrix of non-negative "
                "weights with one entry per pair (0: the pair is missing)")
    if isinstance(weights, (bool, np.bool_, str, bytes)):
        raise ValueError(f"`weights` is {weights!r}; {accepted}")
    if isinstance(weights, numbers.Real) or (isinstance(weights, (np.ndarray, torch.Tensor)) and weights.ndim == 0
                                             and weights.dtype not in (torch.bool, np.bool_)):
        p = float(weights)
        if not (math.isfinite(p) and p >= 0.0):
            raise ValueError(f"the exponent `weights`={weights!r} must be finite and >= 0; {accepted}")
        return Weights(W_POWER, p, None)
    if not isinstance(weights, (np.ndarray, torch.Tensor)):
        raise ValueError(f"`weights` is a {type(weights).__name__}; {accepted}, as a numpy array or a torch tensor")
    if not allow_matrix:
        raise ValueError("a weight matrix is not supported here: landmark MDS draws its rows itself, so only the "
                         "power form `weights=p` can be handed to both of its stages")
    if isinstance(weights, torch.Tensor):
        ok = not weights.is_complex() and weights.layout == torch.strided
    else:
        ok = weights.dtype.kind in "biuf"
    if not ok:
        raise ValueError(f"`weights` has dtype {weights.dtype}; {accepted}")
    if weights.ndim != 2 or (shape is not None and tuple(int(v) for v in weights.shape) != tuple(shape)):
        raise ValueError(f"a `weights` matrix must have one entry per pair, shape {tuple(shape) if shape else '[., .]'}"
                         f"; got shape {tuple(weights.shape)}")
    return Weights(W_MATRIX, 0.0, weights)


def weight_stats(W, Dm=None, square=True):
    """``mde_pair_weights_check`` on a float32 ``W`` on one GPU (and the float32 ``Dm`` of the same shape it weighs):
    a ``WeightStats``; one launch sequence and one read-back, ``row_kept`` (int32) stays on the device."""
    n_q, n_c, device = int(W.shape[0]), int(W.shape[1]), W.device
    counts = torch.empty(5, dtype=torch.int64, device=device)
    tops = torch.empty(4, dtype=torch.float32, device=device)
    row_kept = torch.empty(n_q, dtype=torch.int32, device=device)
    with torch.cuda.device(device):
        _lib.check(_lib.load().mde_pair_weights_check(n_q, n_c, 1 if square else 0, _lib.ptr(W), _lib.ptr(Dm),
                                                      _lib.ptr(counts), _lib.ptr(tops), _lib.ptr(row_kept),
                                                      _lib.stream_ptr(device)))
    c, t = counts.tolist(), tops.tolist()
    return WeightStats(c[0], c[1], c[2], c[3], c[4], t[0], t[1], t[2], t[3], row_kept)


def _device_weights(weights, Dm, square, device):
    """The matrix form on the device, checked: ``(Weights with W float32 on `device`, WeightStats)``; ``ValueError``
    saying which rule the matrix (or a deviation it keeps) breaks."""
    W = torch.as_tensor(weights.W).to(device=device, dtype=torch.float32).contiguous()
    stats = weight_stats(W, Dm, square)
    if stats.nonfinite:
        raise ValueError(f"`weights` is not finite: {stats.nonfinite} of its entries are NaN or infinite")
    if stats.negative:
        raise ValueError(f"`weights` is not non-negative: {stats.negative} of its entries are below zero")
    if square and stats.asymmetry > SYMMETRY_RTOL * stats.largest:
        raise ValueError(f"`weights` is not symmetric: an entry differs from its mirror image by "
                         f"{stats.asymmetry:.3g} (the largest entry is {stats.largest:.3g})")
    if stats.empty_rows:
        raise ValueError(f"`weights` leaves {stats.empty_rows} of the {int(W.shape[0])} rows without a pair (every "
                         "weight of the row is zero): such an item has no position")
    if stats.bad_deviations:
        raise ValueError(f"`distance_matrix` is NaN, infinite or negative at {stats.bad_deviations} entries that "
                         "`weights` keeps (only the pairs of weight zero may be unknown)")
    if square and stats.deviation_asymmetry > SYMMETRY_RTOL * stats.largest_deviation:
        raise ValueError(f"`distance_matrix` is not symmetric on the pairs that `weights` keeps: an entry differs "
                         f"from its mirror image by {stats.deviation_asymmetry:.3g} (the largest kept entry is "
                         f"{stats.largest_deviation:.3g})")
    return Weights(W_MATRIX, 0.0, W), stats

LossSpec = collections.namedtuple("LossSpec", ["kind", "scalars", "weighted"])
LossSpec.__doc__ = """What ``mde_pair_loss`` needs of a loss: its ``kind`` (MDE_F_L_* of include/mde_hip.h), its three
``scalars``, and whether it is ``weighted`` (by the default ``1 / delta^2``, which the kernel forms itself)."""

_ACCEPTED = ("a dense problem takes a loss of pymde_amd.losses as a callable of the deviations -- a class (Quadratic, "
             "WeightedQuadratic, Huber, Cubic, Power, Absolute, Logistic, Fractional, SoftFractional) or a "
             "functools.partial of one that fixes its threshold / exponent / gamma -- with the default weights")


def loss_spec(loss):
    """The ``LossSpec`` of ``loss``, a callable of the deviations as the recipes take it.  Needs no GPU: the callable
    is tried on ``torch.ones(1)``.  ``ValueError`` (naming what is accepted) for a penalty, for a callable whose
    result has no ``_hip_spec``, and for weights other than the default ``1 / delta^2``: per-pair weights go to the
    problem's ``weights=``, not into the loss."""
    if isinstance(loss, torch.nn.Module) or not callable(loss):
        raise ValueError(f"`loss` is {loss!r}, not a callable of the deviations; {_ACCEPTED}")

    def probe(value):
        f = loss(torch.full((1,), value))
        spec = f._hip_spec() if hasattr(f, "_hip_spec") else None
        if spec is None:
            raise ValueError(f"`loss` returned {type(f).__name__}, which has no closed form in the kernels "
                             f"(_hip_spec); {_ACCEPTED}")
        return f, spec
    f, spec = probe(1.0)
    if spec.kind < _FIRST_LOSS or spec.kind_neg != 0:
        raise ValueError(f"{type(f).__name__} is a penalty (a function of the distance and a weight), not a loss of "
                         f"the deviations; {_ACCEPTED}")
    weighted = spec.a1 is not None
    if weighted:
        # the default weights are 1 at delta = 1 and 1 / 4 at delta = 2; anything else was passed in
        for value, want in ((1.0, 1.0), (2.0, 0.25)):
            a1 = probe(value)[1].a1
            if not isinstance(a1, torch.Tensor) or a1.numel() != 1 or float(a1.reshape(-1)[0]) != want:
                raise ValueError(f"{type(f).__name__} was given weights of its own; a dense problem takes a loss with "
                                 f"the default 1 / delta^2 and its per-pair weights through `weights=`; {_ACCEPTED}")
    return LossSpec(int(spec.kind), tuple(float(s) for s in spec.scalars), weighted)


def check_source(data, metric):
    """Canonical name of a metric the Gram tile serves; ``ValueError`` for Manhattan and for a ``Graph`` (no device is
    needed to say so)."""
    _binary.refuse(data, "a dense problem (DenseMDE, DensePlacement, LandmarkMDE, dense=True, landmarks=, "
                         "classical_mds(data=...))", "pass the distances themselves as distance_matrix=")
    metric = _metrics.resolve(metric)
    if preprocess._is_graph(data):
        raise ValueError("a dense problem forms its deviations from the rows of a data matrix; for a Graph pass its "
                         "shortest-path lengths as DenseMDE(distance_matrix=...), or use the edge-list problem "
                         "(preserve_distances(graph) with dense=False)")
    if metric not in quality._RANKED_METRICS:
        raise ValueError(f"metric={metric!r} has no Gram tile; dense problems support 'euclidean', 'cosine' and "
                         "'correlation' (pass other distances as DenseMDE(distance_matrix=...))")
    return metric


def _pair_loss(X, spec, A=None, mode=0, Dm=None, d_scale=1.0, slices=0, work=None, weights=None, pairs=None):
    """``mde_pair_loss`` on prepared float32 tensors on one GPU: ``(loss float64 [1], grad float32 [n, d], row_loss
    float64 [n])`` on that GPU.  Exactly one of ``A`` (the prepared data rows) and ``Dm`` (the [n, n] matrix).  With
    ``weights`` (a ``Weights`` whose ``W`` is float32 on that GPU) ``mde_pair_loss_weighted``; ``pairs`` is then the
    number of pairs that count (default: all)."""
    n, d, device = int(X.shape[0]), int(X.shape[1]), X.device
    lib = _lib.load()
    loss = torch.empty(1, dtype=torch.float64, device=device)
    grad = torch.empty((n, d), dtype=torch.float32, device=device)
    row_loss = torch.empty(n, dtype=torch.float64, device=device)
    with torch.cuda.device(device):
        if work is None:
            work = _work(lib, n, d, slices, device)
        head = (n, 0 if A is None else int(A.shape[1]), _lib.ptr(A), mode, _lib.ptr(Dm), float(d_scale), d,
                _lib.ptr(X), spec.kind, spec.scalars[0], spec.scalars[1], spec.scalars[2], slices)
        tail = (_lib.ptr(loss), _lib.ptr(grad), _lib.ptr(row_loss), _lib.ptr(work), _lib.stream_ptr(device))
        if weights is None:
            _lib.check(lib.mde_pair_loss(*head, *tail))
        else:
            pairs = 0.5 * n * (n - 1) if pairs is None else float(pairs)
            _lib.check(lib.mde_pair_loss_weighted(*head, weights.source, weights.p, _lib.ptr(weights.W), pairs, *tail))
    return loss, grad, row_loss


def _work(lib, n, d, slices, device):
    return _lib.work_buffer(lib.mde_pair_loss_work_bytes, n, d, slices, device=device)


class _DenseDistortion(torch.autograd.Function):
    """The average distortion of a ``DenseMDE``: one launch sequence yields the value and the gradient."""

    @staticmethod
    def forward(ctx, X, owner):
        loss, grad, _ = owner._evaluate(X.detach())
        ctx.save_for_backward(grad)
        return loss.to(torch.float32).reshape(())

    @staticmethod
    def backward(ctx, grad_output):
        (grad,) = ctx.saved_tensors
        return grad_output * grad, None


def _check_distance_matrix(D, square=True):
    """Finite and non-negative and, for a ``square`` matrix, symmetric (a rectangular one has no symmetry to check): one
    pass on the GPU in row blocks, one read-back; ``ValueError`` saying which."""
    rows, cols = int(D.shape[0]), int(D.shape[1])
    flags = torch.zeros(2, dtype=torch.int64, device=D.device)
    worst = torch.zeros(2, dtype=torch.float32, device=D.device)          # the largest entry, the largest |D - D^T|
    step = max(1, min(rows, (1 << 24) // cols))
    for lo in range(0, rows, step):
        block = D[lo:lo + step]
        flags[0] += (~torch.isfinite(block)).sum()
        flags[1] += (block < 0).sum()
        if square:
            worst[0] = torch.maximum(worst[0], block.abs().max())
            worst[1] = torch.maximum(worst[1], (block - D[:, lo:lo + step].T).abs().max())
    bad, negative = flags.tolist()
    if bad:
        raise ValueError(f"`distance_matrix` is not finite: {bad} of its entries are NaN or infinite")
    if negative:
        raise ValueError(f"`distance_matrix` is not non-negative: {negative} of its entries are below zero")
    top, asym = worst.tolist() if square else (0.0, 0.0)
    if asym > SYMMETRY_RTOL * top:
        raise ValueError(f"`distance_matrix` is not symmetric: an entry differs from its mirror image by {asym:.3g} "
                         f"(the largest entry is {top:.3g})")


class DenseMDE(object):
    """An MDE problem over ALL pairs of ``n`` items: minimise the mean over the ``p = n (n - 1) / 2`` pairs of
    ``loss(|x_i - x_j|, D_ij)`` over the constraint set -- ``MDE(n, embedding_dim, all_edges(n), loss(deviations))``
    without the edge list.

    Exactly one source of the deviations ``D``:

    ``data``: a dense or sparse data matrix [n, n_features] (as ``quality.stress`` takes it), prepared as the
    searches prepare it; ``D_ij`` is the distance of rows i and j under ``metric`` (``"euclidean"``, ``"cosine"``,
    ``"correlation"``), formed on the fly in every evaluation, bit for bit the D of ``quality.pair_moments``.
    ``distance_matrix``: a square [n, n] matrix of dissimilarities (sklearn's ``dissimilarity="precomputed"``),
    kept as float32 on the GPU; it is checked once for finiteness, non-negativity and symmetry (to a relative 1e-5
    of its largest entry); its diagonal is never used.

    ``loss``: a class of ``pymde_amd.losses`` or a ``functools.partial`` of one (``loss_spec``); weighted losses
    use their default weights ``1 / D^2``.  ``deviation_scale``: every deviation is multiplied by it (what
    ``preserve_distances`` does for ``Standardized``).  ``1 <= embedding_dim <= 8``.

    ``weights``: ``None``, or a weight per pair.  A real number ``p >= 0`` weighs every pair by
    ``D^-p`` (``D`` after ``deviation_scale``), formed in the kernel: ``Quadratic`` with ``weights=1`` is Sammon
    mapping.  A matrix [n, n] (numpy or torch; bool or numeric; kept as float32 on the GPU) gives the weights
    themselves: it must be finite, non-negative and symmetric (to a relative 1e-5), its diagonal is ignored, and a
    ZERO marks a missing pair -- the pair takes no part, ``p`` becomes the number of pairs that are kept, the mean is
    over those, and a ``distance_matrix`` may hold anything (NaN included) there; it is then checked on the kept pairs
    only.  Every row must keep a pair.  For the weighted losses (``WeightedQuadratic``) the weight replaces the default
    ``1 / D^2``; every other loss is multiplied by it.  ``DenseMDE.from_graph`` builds such a problem from a
    ``Graph``'s shortest paths.

    ``init``: where ``embed()`` starts when it is given no ``X``.  ``"random"`` (the default): the constraint's own
    draw.  ``"classical"``: ``classical_initialization()``, the closed-form classical scaling of the problem's own
    deviations (``pymde_amd.classical``); a ``ValueError`` with ``Anchored`` and when a weight
    matrix leaves out pairs.  Power weights are ignored by the start and used by the solve.

    After ``embed()``: ``X``, ``solve_stats``, ``value`` and ``residual_norm``, as for ``MDE``.  The per-pair
    ``distances`` / ``distortions`` / ``high_distortion_pairs`` of ``MDE`` are n^2 values and are not provided;
    ``item_distortions`` has one value per item.  With ``Anchored`` the anchor-anchor pairs stay in the mean: they
    add a constant to the value and nothing to the gradient of the free rows."""

    def __init__(self, data=None, embedding_dim=2, loss=losses.Absolute, constraint=None, distance_matrix=None,
                 metric="euclidean", deviation_scale=1.0, device=None, weights=None, init="random"):
        if (data is None) == (distance_matrix is None):
            raise ValueError("exactly one of `data` and `distance_matrix` must be given")
        self.init = check_init(init)
        if init == "classical" and isinstance(constraint, constraints.Anchored):
            raise ValueError("init='classical' is not available with an Anchored constraint: classical scaling fixes "
                             "the position of every row, the anchors' included")
        self._set_loss(int(embedding_dim), loss, deviation_scale, "embedding_dim",
                       " (the kernel keeps a row of the embedding in registers)")
        source = data if data is not None else distance_matrix
        if data is not None:
            metric = check_source(data, metric)
            quality._check_matrix(data, "data")
        elif not hasattr(source, "shape") or len(source.shape) != 2 or int(source.shape[0]) != int(source.shape[1]):
            raise ValueError("`distance_matrix` must be a square matrix [n, n], got shape "
                             f"{tuple(getattr(source, 'shape', ()))}")
        n = int(source.shape[0])
        if n < 2:
            raise ValueError("a dense problem needs at least two items")
        weights = parse_weights(weights, (n, n))
        if device is None:
            device = source.device if isinstance(source, torch.Tensor) and source.is_cuda else util.get_default_device()
        self.device = util.require_cuda_device(device)
        self._A, self._Dm, self._mode = None, None, 0
        if data is not None:
            self._A = quality._self_rows(data, metric, self.device, "data")
            self._mode = quality._pair_modes(metric)[0]
        else:
            self._Dm = torch.as_tensor(distance_matrix).to(device=self.device, dtype=torch.float32).contiguous()
            if weights.source != W_MATRIX:
                _check_distance_matrix(self._Dm)
        self.n_items = n
        self._item_pairs = n - 1
        self.n_all_pairs = n * (n - 1) // 2
        self._set_weights(weights, True)
        if init == "classical" and self.p != self.n_all_pairs:
            raise ValueError(f"init='classical' needs every pair, and `weights` leaves out "
                             f"{self.n_all_pairs - self.p} of {self.n_all_pairs} (the pairs of a disconnected graph, "
                             "or the zeros of a weight matrix)")
        self.metric = metric if data is not None else None
        self.constraint = constraints.Centered() if constraint is None else constraint
        self._reset()

    # ------------------------------------------------------------------ what the constructors of both problems share
    def _set_loss(self, embedding_dim, loss, deviation_scale, dimension, reason):
        """Checks and installs ``embedding_dim``, ``loss`` (and its ``_spec``) and ``deviation_scale``; the message
        names the dimension as ``dimension`` and adds ``reason``."""
        if not 1 <= embedding_dim <= MAX_DIM:
            raise ValueError(f"{dimension} must lie in [1, {MAX_DIM}] for a dense problem{reason}, got "
                             f"{embedding_dim}")
        self._spec = loss_spec(loss)
        deviation_scale = float(deviation_scale)
        if not (deviation_scale > 0.0 and math.isfinite(deviation_scale)):
            raise ValueError(f"deviation_scale must be a positive finite number, got {deviation_scale!r}")
        self.embedding_dim, self.loss, self.deviation_scale = embedding_dim, loss, deviation_scale

    def _set_weights(self, weights, square):
        """Installs a ``parse_weights`` result (a matrix goes to the device and is checked, with ``_Dm``): ``_weights``,
        ``_row_kept`` and ``p``, the number of pairs that count."""
        self.p = self.n_all_pairs
        self._weights, self._row_kept = (None if weights.source == W_NONE else weights), None
        if weights.source == W_MATRIX:
            self._weights, stats = _device_weights(weights, self._Dm, square, self.device)
            self.p, self._row_kept = int(stats.kept), stats.row_kept

    def _reset(self):
        self.X = None
        self.solve_stats = None
        self.value = None
        self.residual_norm = None
        self._work_buffer = None
        self._rows_work_buffer = None

    def __str__(self):
        source = "data matrix, metric %s" % self.metric if self._A is not None else "distance matrix"
        return ("Dense MDE problem:\n\tn (number of items) {0}\n\tm (embedding dimension) {1}\n"
                "\tp (number of pairs, {2}) {3}\n\tdeviations from a {4}{5}\n\tconstraint {6}\n\tdevice {7}".format(
                    self.n_items, self.embedding_dim, self._pairs_note(), self.p, source, self._weights_note(),
                    self.constraint.name(), self.device))

    def _pairs_note(self):
        if self._row_kept is None:
            return "all of them"
        return "those of non-zero weight, of %d" % self.n_all_pairs

    def _weights_note(self):
        if self._weights is None:
            return ""
        if self._weights.source == W_POWER:
            return "\n\tweights D^-%g" % self._weights.p
        return "\n\tweights from a matrix"

    # ------------------------------------------------------------------ plumbing
    def _embedding_arg(self, X):
        if X is None:
            X = self.X
        if X is None:
            raise ValueError("Call this function after running the `embed` method, or provide a value for the "
                             "embedding argument `X`")
        if tuple(X.shape) != (self.n_items, self.embedding_dim):
            raise ValueError(f"the embedding must have shape ({self.n_items}, {self.embedding_dim}), got "
                             f"{tuple(X.shape)}")
        if X.device != self.device:
            X = X.to(self.device)
        if X.dtype != torch.float32:
            if X.dtype == torch.float64 and not _problem._WARNED_F64:
                _problem.LOGGER.warning("pymde_amd computes in float32: float64 embeddings are cast to float32 "
                                        "(gradients flow back through the cast)")
                _problem._WARNED_F64 = True
            X = X.to(torch.float32)
        return X

    def _evaluate(self, X):
        """(loss float64 [1], grad float32 [n, d], row_loss float64 [n]) at a float32 X on the problem's device."""
        if self._work_buffer is None:
            with torch.cuda.device(self.device):
                self._work_buffer = _work(_lib.load(), self.n_items, self.embedding_dim, 0, self.device)
        return _pair_loss(X.contiguous(), self._spec, A=self._A, mode=self._mode, Dm=self._Dm,
                          d_scale=self.deviation_scale, work=self._work_buffer, weights=self._weights, pairs=self.p)

    # ------------------------------------------------------------------ evaluators
    def average_distortion(self, X=None):
        """The average distortion of ``X`` over all pairs (a 0-dim float32 tensor; differentiable w.r.t. ``X``)."""
        return _DenseDistortion.apply(self._embedding_arg(X), self)

    def item_distortions(self, X=None):
        """float32 [n]: for every item the mean of the loss over its pairs (colour a plot by it) -- ``n - 1`` of them,
        ``n_old`` for a new row of a placement.  Their mean is the average distortion.  With a weight matrix: over the
        pairs the item keeps (their mean, weighted by those counts, is then the average distortion)."""
        row_loss = self._evaluate(self._embedding_arg(X).detach())[2]
        if self._row_kept is not None:
            return (row_loss / self._row_kept.to(torch.float64)).to(torch.float32)
        return (row_loss / float(self._item_pairs)).to(torch.float32)

    @classmethod
    def from_graph(cls, graph, embedding_dim=2, loss=losses.Absolute, constraint=None, max_length=None):
        """The dense problem over the pairs of nodes of a ``Graph`` that a path joins: the deviations are the
        shortest-path lengths (``graph.shortest_paths``, all of them), scattered into a float32 [n, n] matrix, and
        the weight matrix is 1 where a path exists (of length at most ``max_length``, if given) and 0 where none
        does -- pairs in different components are missing, not infinitely far.  A node that reaches no other is a
        ``ValueError`` (a row without a pair).  O(n^2) memory: two float32 matrices."""
        if not isinstance(graph, _graph.Graph):
            raise ValueError("`graph` must be a pymde_amd.Graph instance.")
        paths = _graph.shortest_paths(graph, max_length=max_length)
        n, device = int(graph.n_items), paths.edges.device
        D = torch.zeros((n, n), dtype=torch.float32, device=device)
        W = torch.zeros((n, n), dtype=torch.float32, device=device)
        i, j = paths.edges[:, 0], paths.edges[:, 1]
        D[i, j] = paths.distances
        D[j, i] = paths.distances
        W[i, j] = 1.0
        W[j, i] = 1.0
        return cls(distance_matrix=D, embedding_dim=embedding_dim, loss=loss, constraint=constraint, device=device,
                   weights=W)

    # ------------------------------------------------------------------ the solve
    def classical_initialization(self, **solver_keywords):
        """The classical start [n, d]: the classical scaling of the problem's own source and ``deviation_scale``
        (``solver_keywords``: the ``n_oversamples``, ``n_iter``, ``seed`` and ``test_matrix`` of ``classical_mds``);
        the columns whose eigenvalue is at most 1e-6 of the largest get ``1e-3 sqrt(lambda_1 / n)`` times standard
        normal noise, since a flat start is a saddle of the loss; the result is projected onto the constraint."""
        if isinstance(self.constraint, constraints.Anchored) or self.p != self.n_all_pairs:
            raise ValueError("the classical start needs every pair and no anchors")
        fit = _classical.scale_problem(self._A, self._mode, self._Dm, self.deviation_scale, self.embedding_dim,
                                       **solver_keywords)
        X = fit.X.clone()
        lam = fit.eigenvalues
        flat = lam <= _classical.NOISE_RTOL * lam[0]
        if bool(flat.any()):
            noise = 1e-3 * math.sqrt(max(float(lam[0]), 0.0) / self.n_items)
            X[:, flat] += noise * torch.randn((self.n_items, int(flat.sum())), device=self.device,
                                              dtype=torch.float32)
        return self.constraint.project_onto_constraint(X.contiguous(), inplace=True)

    def embed(self, X=None, eps=1e-5, max_iter=300, memory_size=10, verbose=False, print_every=None,
              snapshot_every=None):
        """Compute an embedding; stores it in ``self.X`` and returns it.  Arguments as in ``MDE.embed``; without
        ``X`` the start is the one ``init`` names."""
        if X is None and self.init == "classical":
            X = self.classical_initialization()
        elif X is None:
            X = self.constraint.initialization(self.n_items, self.embedding_dim, self.device)
        else:
            X = X.detach().clone()
        if X.device != self.device:
            if X.is_cuda:
                _problem.LOGGER.warning(
                    f"The initial iterate's device ({X.device}) does not match the requested "
                    f"device ({self.device}). Copying the iterate to {self.device}.")
            X = X.to(self.device)
        if max_iter < 0:
            raise ValueError("`max_iter` must be greater than 0")
        if memory_size <= 0:
            raise ValueError("`memory_size` must be greater than 0")
        if X.dtype != torch.float32:
            X = X.to(torch.float32)
        if verbose:
            _problem.LOGGER.info(f"Fitting a {self.constraint.name()} embedding into R^{self.embedding_dim}, for "
                                 f"{self.n_items} items and all their {self.p} pairs.")
            _problem.LOGGER.info(f"`embed` method parameters: eps={eps:.1e}, "
                                 f"max_iter={max_iter}, memory_size={memory_size}")
        if print_every is None:
            print_every = max(1, max_iter // 10)
        X_star, solve_stats = optim.lbfgs(
            X=X, objective_fn=self.average_distortion, constraint=self.constraint, eps=eps,
            max_iter=max_iter, memory_size=memory_size, use_line_search=True,
            use_cached_loss=True, verbose=verbose, print_every=print_every,
            snapshot_every=snapshot_every, logger=_problem.LOGGER)
        self.X = X_star
        self.solve_stats = solve_stats
        if solve_stats.iterations > 0:
            self.value = solve_stats.average_distortions[-1]
            self.residual_norm = solve_stats.residual_norms[-1]
        if verbose:
            _problem.LOGGER.info(f"Finished fitting in {solve_stats.solve_time:.3f} seconds "
                                 f"and {solve_stats.iterations} iterations.")
            if solve_stats.iterations > 0:
                _problem.LOGGER.info(f"average distortion {self.value:.3g} | "
                                     f"residual norm {self.residual_norm:.1e}")
        return self.X


# ---------------------------------------------------------------------- the rectangular problem
def _pair_loss_cross(XQ, XC, spec, Q=None, C=None, mode=0, Dm=None, d_scale=1.0, slices=0, work=None, weights=None,
                     pairs=None):
    """``mde_pair_loss_cross`` on prepared float32 tensors on one GPU: ``(loss float64 [1], grad float32 [n_q, d],
    row_loss float64 [n_q])`` on that GPU.  Either both ``Q`` and ``C`` (the prepared data rows of the free and of
    the fixed items) or ``Dm`` (the [n_q, n_c] matrix).  With ``weights`` (a ``Weights``; ``W`` [n_q, n_c] float32 on
    that GPU) ``mde_pair_loss_cross_weighted``; ``pairs`` is then the number of pairs that count (default: all)."""
    n_q, n_c, d, device = int(XQ.shape[0]), int(XC.shape[0]), int(XQ.shape[1]), XQ.device
    lib = _lib.load()
    loss = torch.empty(1, dtype=torch.float64, device=device)
    grad = torch.empty((n_q, d), dtype=torch.float32, device=device)
    row_loss = torch.empty(n_q, dtype=torch.float64, device=device)
    with torch.cuda.device(device):
        if work is None:
            work = _work_cross(lib, n_q, n_c, d, slices, device)
        head = (n_q, n_c, 0 if Q is None else int(Q.shape[1]), _lib.ptr(Q), _lib.ptr(C), mode, _lib.ptr(Dm),
                float(d_scale), d, _lib.ptr(XQ), _lib.ptr(XC), spec.kind, spec.scalars[0], spec.scalars[1],
                spec.scalars[2], slices)
        tail = (_lib.ptr(loss), _lib.ptr(grad), _lib.ptr(row_loss), _lib.ptr(work), _lib.stream_ptr(device))
        if weights is None:
            _lib.check(lib.mde_pair_loss_cross(*head, *tail))
        else:
            pairs = float(n_q) * n_c if pairs is None else float(pairs)
            _lib.check(lib.mde_pair_loss_cross_weighted(*head, weights.source, weights.p, _lib.ptr(weights.W), pairs,
                                                        *tail))
    return loss, grad, row_loss


def _work_cross(lib, n_q, n_c, d, slices, device):
    return _lib.work_buffer(lib.mde_pair_loss_cross_work_bytes, n_q, n_c, d, slices, device=device)


class _Free(constraints.Constraint):
    """The constraint of a placement: none.  The new rows are free and the fixed rows are not variables of the
    solve, so there is nothing to project onto, not even the centring of ``Centered``."""

    def name(self):
        return "free"

    def initialization(self, n_items, embedding_dim, device=None):
        return constraints._randn(n_items, embedding_dim, device)

    def project_onto_constraint(self, Z, inplace=True):
        return Z if inplace else Z.detach().clone()

    def project_onto_tangent_space(self, X, Z, inplace=True):
        del X
        return Z if inplace else Z.detach().clone()


class DensePlacement(DenseMDE):
    """Out-of-sample placement into a distance-preserving embedding: minimise, over the ``n_new`` new rows alone, the
    mean over all ``p = n_new * n_old`` (new row, embedded row) pairs of ``loss(|x_new - x_old|, D)``, with the
    embedded rows held where they are -- the rectangular form of ``DenseMDE`` (``mde_pair_loss_cross``, DESIGN section
    6k).  No new-new pair and no old-old pair takes part; a second ``DenseMDE`` over old + new rows with ``Anchored``
    would walk ``(n_old + n_new)^2`` pairs and include both.

    Exactly one source of the deviations ``D``:

    ``data`` [n_old, n_features] and ``new_data`` [n_new, n_features]: dense or sparse data matrices, prepared as
    ``preprocess.cross_nearest_neighbors`` prepares its corpus and its queries (Euclidean: both minus the column
    means of ``data`` when that offset dominates; cosine / correlation: unit rows), so ``D`` is the distance that
    search reports, formed on the fly in every evaluation.
    ``distance_matrix`` [n_new, n_old] (with ``data=None, new_data=None``): rectangular, new against old, kept as
    float32 on the GPU and checked once to be finite and non-negative.

    ``X`` [n_old, d] is the embedding of the old rows; it is used as float32 and never modified, and ``d`` (1 .. 8)
    is taken from it.  ``loss`` and ``deviation_scale`` as for ``DenseMDE``.  A new row identical to an old one in
    both spaces is an ordinary pair (D = E = 0).  ``DensePlacement.weighted(..., weights=)`` builds the same problem
    with a weight per pair, or with missing pairs.

    ``embed()`` starts every new row where ``initialization()`` puts it: by default (the attribute ``init`` is
    ``"neighbors"``; set it, or pass ``init=`` to ``weighted``, for ``"triangulation"``) every new row at the mean of the embedding vectors of its ``d + 1`` nearest old
    rows (``d + 1`` points fix a position in R^d; perturbed by 1e-4 if a new row lands exactly on an old one).  The
    objective is separable over the new rows, and ``embed`` has two solvers for it.  ``solver="joint"`` (the default)
    runs ONE L-BFGS over all new rows: one step length and one set of curvature pairs for rows that do not interact.
    ``solver="rows"`` (``pymde_amd.rows``) runs a BFGS with its own line search and its own
    stopping test for every row, all rows in lock step, and evaluates only the rows that are still working; it ends
    when every row has converged (``|g_i| <= eps``, which implies the joint criterion) or stalled.  After either:
    ``X`` (the new rows, [n_new, d]), ``solve_stats``, ``value`` and ``residual_norm``; after ``"rows"`` also
    ``row_status`` (int32 [n_new]: 0 still active when ``max_iter`` ran out, 1 converged, 2 stalled).
    ``embedding()`` is ``cat([X_old, X_new])``."""

    def __init__(self, data, X, new_data, loss=losses.Absolute, metric="euclidean", deviation_scale=1.0,
                 distance_matrix=None, device=None):
        self._setup(data, X, new_data, loss, metric, deviation_scale, distance_matrix, device, None)

    @classmethod
    def weighted(cls, data, X, new_data, *, weights, loss=losses.Absolute, metric="euclidean", deviation_scale=1.0,
                 distance_matrix=None, device=None, init="neighbors"):
        """The placement with a weight per (new row, embedded row) pair: the arguments of the constructor and
        ``weights``, as for ``DenseMDE`` -- ``None``, a number ``p`` (every pair is weighed by ``D^-p``), or a matrix
        [n_new, n_old] (no symmetry to ask for) whose zeros are MISSING pairs.  Every new row must keep a pair; ``p``
        is the number kept; a ``distance_matrix`` is then checked on its kept pairs only; with ``solver="rows"`` the
        reported values are those of this joint problem.  ``init`` sets the attribute of that name.  (The
        constructor's own parameter list is fixed.)"""
        check_init(init, PLACEMENT_INITS)
        self = cls.__new__(cls)
        self._setup(data, X, new_data, loss, metric, deviation_scale, distance_matrix, device, weights)
        if init == "triangulation":
            self._check_triangulation()
        self.init = init
        return self

    def _check_triangulation(self):
        if self.p != self.n_all_pairs:
            raise ValueError(f"the triangulated start needs the deviation of every (new row, embedded row) pair, and "
                             f"`weights` leaves out {self.n_all_pairs - self.p} of {self.n_all_pairs}")

    def _setup(self, data, X, new_data, loss, metric, deviation_scale, distance_matrix, device, weights):
        from_data = data is not None or new_data is not None
        if from_data == (distance_matrix is not None):
            raise ValueError("exactly one source of the deviations must be given: `data` and `new_data`, or "
                             "`distance_matrix` [n_new, n_old] with data=None and new_data=None")
        if from_data and (data is None or new_data is None):
            raise ValueError("`data` (the embedded rows) and `new_data` (the rows to place) must be given together")
        if not hasattr(X, "shape") or len(X.shape) != 2:
            raise ValueError("`X` must be the embedding [n_old, d] of the embedded rows, got shape "
                             f"{tuple(getattr(X, 'shape', ()))}")
        n_old, embedding_dim = int(X.shape[0]), int(X.shape[1])
        self._set_loss(embedding_dim, loss, deviation_scale, "the embedding dimension (the columns of `X`)", "")
        if from_data:
            for m in (data, new_data):
                metric = check_source(m, metric)
            quality._check_matrix(data, "data")
            quality._check_matrix(new_data, "new_data")
            if int(data.shape[0]) != n_old:
                raise ValueError(f"`X` must hold one embedding vector per row of `data` ({int(data.shape[0])}); got "
                                 f"shape {tuple(X.shape)}")
            if int(new_data.shape[1]) != int(data.shape[1]):
                raise ValueError(f"`new_data` has {int(new_data.shape[1])} features and `data` has "
                                 f"{int(data.shape[1])}; they must agree")
            n_new = int(new_data.shape[0])
        else:
            shape = tuple(getattr(distance_matrix, "shape", ()))
            if len(shape) != 2 or int(shape[1]) != n_old:
                raise ValueError(f"`distance_matrix` must be rectangular [n_new, n_old = {n_old}], new rows against "
                                 f"the rows of `X`; got shape {shape}")
            n_new = int(shape[0])
        if n_old < 1:
            raise ValueError("a placement needs at least one embedded row")
        if n_new < 1:
            raise ValueError("`new_data` needs at least one row" if from_data else
                             "`distance_matrix` needs at least one row")
        weights = parse_weights(weights, (n_new, n_old))
        if device is None:
            on_gpu = [t.device for t in (X, data, new_data, distance_matrix)
                      if isinstance(t, torch.Tensor) and t.is_cuda]
            device = on_gpu[0] if on_gpu else util.get_default_device()
        self.device = util.require_cuda_device(device)
        # (a copy: the caller's tensor is neither written nor followed)
        self._X_old = torch.as_tensor(X).detach().to(device=self.device, dtype=torch.float32, copy=True).contiguous()
        if not bool(torch.isfinite(self._X_old).all()):
            raise ValueError("`X` holds NaN or infinite entries")
        self._A, self._Q, self._Dm, self._mode = None, None, None, 0
        if from_data:
            Q = preprocess._dense_rows_for_cross(new_data, self.device, "new_data")
            C = preprocess._dense_rows_for_cross(data, self.device, "data")
            if metric == _metrics.EUCLIDEAN:
                _metrics.check_finite(Q, "`new_data`")
                Q, C = preprocess._translated_pair(Q, C)
            else:
                Q, C = _metrics.normalized_rows(Q, metric), _metrics.normalized_rows(C, metric)
            self._Q, self._A = Q.contiguous(), C.contiguous()
            self._mode = quality._pair_modes(metric)[0]
        else:
            self._Dm = torch.as_tensor(distance_matrix).to(device=self.device, dtype=torch.float32).contiguous()
            if weights.source != W_MATRIX:
                _check_distance_matrix(self._Dm, square=False)
        self.n_items = n_new
        self.n_old = self._item_pairs = n_old
        self.n_all_pairs = n_new * n_old
        self._set_weights(weights, False)
        self.metric = metric if from_data else None
        self.constraint = _Free()
        self._reset()
        self.row_status = None
        self.init = "neighbors"

    def __str__(self):
        source = "data matrices, metric %s" % self.metric if self._A is not None else "distance matrix"
        return ("Dense placement problem:\n\tn (number of new items) {0}\n\tembedded items, held fixed {1}\n"
                "\tm (embedding dimension) {2}\n\tp (number of pairs, new against embedded{3}) {4}\n"
                "\tdeviations from {5}{6}\n\tdevice {7}".format(
                    self.n_items, self.n_old, self.embedding_dim,
                    "" if self._row_kept is None else ": " + self._pairs_note(), self.p, source,
                    self._weights_note(), self.device))

    def _evaluate(self, X):
        """(loss float64 [1], grad float32 [n_new, d], row_loss float64 [n_new]) at a float32 X on the device."""
        if self._work_buffer is None:
            with torch.cuda.device(self.device):
                self._work_buffer = _work_cross(_lib.load(), self.n_items, self.n_old, self.embedding_dim, 0,
                                                self.device)
        return _pair_loss_cross(X.contiguous(), self._X_old, self._spec, Q=self._Q, C=self._A, mode=self._mode,
                                Dm=self._Dm, d_scale=self.deviation_scale, work=self._work_buffer,
                                weights=self._weights, pairs=self.p)

    def average_distortion(self, X=None):
        """The average distortion of the new rows ``X`` [n_new, d] over all ``n_new * n_old`` pairs with the embedded
        rows (a 0-dim float32 tensor; differentiable w.r.t. ``X``)."""
        return _DenseDistortion.apply(self._embedding_arg(X), self)

    def initialization(self, method=None):
        """The start [n_new, d] of ``embed()``; ``method`` defaults to the attribute ``init`` (``"neighbors"`` unless
        it was set).  ``"neighbors"``: every new row at the mean of the embedding vectors of its ``d + 1`` nearest
        embedded rows (fewer when there are fewer), perturbed by 1e-4 if a new row lands exactly on one of them.
        ``"triangulation"``: ``classical.triangulate``, the closed-form least-squares position of every new row from
        its squared deviations to ALL embedded rows (a ``ValueError`` when a weight matrix leaves out pairs)."""
        method = check_init(self.init if method is None else method, PLACEMENT_INITS, "method")
        if method == "triangulation":
            self._check_triangulation()
            return _classical.triangulate(self._X_old, Q=self._Q, C=self._A if self._Q is not None else None,
                                          mode=self._mode, Dm=self._Dm, deviation_scale=self.deviation_scale)
        k = min(self.embedding_dim + 1, self.n_old)
        if self._Dm is not None and self._row_kept is not None:
            # (a missing pair's entry may be anything: it is never among the nearest)
            known = torch.where(self._weights.W > 0, self._Dm, torch.full_like(self._Dm, float("inf")))
            idx = torch.topk(known, k, dim=1, largest=False).indices
        elif self._Dm is not None:
            idx = torch.topk(self._Dm, k, dim=1, largest=False).indices
        else:
            # (the prepared rows: translating both by one vector, or normalising each, is idempotent)
            idx = preprocess._cross_knn_lists(self._Q, self._A, k)[0].to(torch.int64)
        X_new = self._X_old[idx].mean(1)
        on_old = (self._X_old[idx] == X_new.unsqueeze(1)).all(2).any()
        if bool(on_old):
            X_new = X_new + 1e-4 * torch.randn(X_new.shape, device=self.device, dtype=X_new.dtype)
        return X_new.contiguous()

    def _evaluate_rows(self, X, rows, row_loss, row_grad):
        """``mde_pair_loss_cross_rows`` at a float32 X: the sums of the rows of ``rows`` (``None``: all), in place."""
        if self._rows_work_buffer is None:
            with torch.cuda.device(self.device):
                self._rows_work_buffer = _rows.work_cross_rows(_lib.load(), self.n_items, self.n_old,
                                                               self.embedding_dim, 0, self.device)
        return _rows.pair_loss_cross_rows(X.contiguous(), self._X_old, self._spec, row_loss, row_grad, rows=rows,
                                          Q=self._Q, C=self._A, mode=self._mode, Dm=self._Dm,
                                          d_scale=self.deviation_scale, work=self._rows_work_buffer,
                                          weights=self._weights)

    def embed(self, X=None, eps=1e-5, max_iter=300, memory_size=10, verbose=False, print_every=None,
              snapshot_every=None, solver="joint"):
        """Place the new rows; stores them in ``self.X`` [n_new, d] and returns them.  ``X``: their start (default:
        ``initialization()``).  ``solver``: ``"joint"``, one L-BFGS over all rows, or ``"rows"``, a BFGS per row
        (``pymde_amd.rows``; ``max_iter`` then counts sweeps, ``eps`` bounds every row's own gradient norm, and
        ``memory_size`` is not used: a row keeps a full d x d matrix).  Other arguments as in ``MDE.embed``."""
        _rows.check_solver(solver)
        if max_iter < 0:
            raise ValueError("`max_iter` must be greater than 0")
        if X is None:
            X = self.initialization()
        if solver == "joint":
            return super().embed(X, eps=eps, max_iter=max_iter, memory_size=memory_size, verbose=verbose,
                                 print_every=print_every, snapshot_every=snapshot_every)
        X = self._embedding_arg(X).detach().contiguous()
        if verbose:
            _problem.LOGGER.info(f"Placing {self.n_items} rows in R^{self.embedding_dim} against {self.n_old} "
                                 f"embedded rows, each row on its own: eps={eps:.1e}, max_iter={max_iter}")
        # (the rows divide by n_old; n_new n_old / p turns their mean into the mean over the pairs that count)
        result = _rows.solve(self._evaluate_rows, X, self.n_old, eps=eps, max_iter=max_iter,
                             snapshot_every=snapshot_every, verbose=verbose, print_every=print_every,
                             logger=_problem.LOGGER, scale=float(self.n_all_pairs) / float(self.p))
        self.X, self.solve_stats, self.row_status = result.X, result.solve_stats, result.row_status
        self.value, self.residual_norm = result.value, result.residual_norm
        if verbose:
            _problem.LOGGER.info(f"Finished placing in {result.solve_stats.solve_time:.3f} seconds and "
                                 f"{result.solve_stats.iterations} sweeps ({result.solve_stats.evaluations:.1f} full "
                                 f"evaluations): average distortion {self.value:.3g} | residual norm "
                                 f"{self.residual_norm:.1e}")
        return self.X

    def embedding(self, X=None):
        """``cat([X_old, X_new])`` [n_old + n_new, d]: the embedded rows, bit for bit, then the placed ones."""
        return torch.cat([self._X_old, self._embedding_arg(X).detach()])


LandmarkSolveStats = collections.namedtuple("LandmarkSolveStats", ["landmarks", "placement"])
LandmarkSolveStats.__doc__ = """The ``SolveStats`` of the two stages of ``LandmarkMDE.embed``."""


def _take_rows(data, rows):
    """The rows ``rows`` (int64, on the CPU) of a dense or sparse data matrix, in the container it came in."""
    if isinstance(data, torch.Tensor):
        if data.layout != torch.strided:
            return data.to_sparse_coo().index_select(0, rows.to(data.device)).coalesce()
        return data[rows.to(data.device)]
    if hasattr(data, "tocsr"):
        return data.tocsr()[rows.numpy()]
    return data[rows.numpy()]


def check_landmarks(landmarks, n_items, constraint):
    """``landmarks`` as an int in ``[2, n_items)``; ``ValueError`` otherwise, and for a constraint the placed rows
    cannot keep (no device is needed to say so)."""
    if isinstance(landmarks, bool) or int(landmarks) != landmarks:
        raise ValueError(f"`landmarks` must be a number of rows (an int), got {landmarks!r}")
    landmarks = int(landmarks)
    if not 2 <= landmarks < n_items:
        raise ValueError(f"`landmarks` must lie in [2, n) = [2, {n_items}): the landmarks need a pair among "
                         f"themselves and at least one row must be left to place; got {landmarks}")
    if constraint is not None and not isinstance(constraint, constraints._Centered):
        raise ValueError(f"landmarks take constraint=None or Centered(), not {constraint.name()}: the placed rows "
                         "are unconstrained (each is put where its distances to the landmarks say), so the whole "
                         "embedding would be neither standardized nor anchored")
    return landmarks


class LandmarkMDE(object):
    """Landmark MDS: embed ``landmarks`` rows of ``data``, drawn uniformly without replacement, with a ``DenseMDE``
    over all their pairs, then place every other row against them with a ``DensePlacement``.  A sweep costs
    O(m^2 + n m) pair evaluations instead of the O(n^2) of the full dense problem, and the pairs among the placed
    rows are never looked at.  ``preserve_distances(data, landmarks=m)`` builds it.

    ``data``, ``embedding_dim``, ``loss``, ``metric`` as for ``DenseMDE``; ``constraint`` is ``None`` or
    ``Centered()``: the result is centred, and the placed rows can keep no other constraint.  ``seed`` draws the
    landmarks (``quality._sample_rows``): the same seed gives the same ``landmarks``.  ``weights``: ``None`` or a
    number ``p``, the power form ``D^-p`` of ``DenseMDE``, handed to both stages; a matrix is a ``ValueError``.
    ``init``: ``"random"`` (the default) or ``"classical"``, which starts the landmarks from their classical scaling
    and every other row from its triangulation against them (``initialization()`` returns that start).

    After ``embed()``: ``X`` [n, d] in the row order of ``data``, ``landmarks`` (int64 indices), ``landmark_problem``
    (the ``DenseMDE``), ``placement`` (the ``DensePlacement``), ``value`` (the placement's value) and ``solve_stats``
    (a ``LandmarkSolveStats`` of both stages).  Score the result with ``quality.stress(data, X, sample=...)``.

    ``LandmarkMDE.from_graph(graph, landmarks, ...)`` is the same problem on a ``Graph`` under its shortest-path
    metric; this constructor refuses a ``Graph``."""

    def __init__(self, data, landmarks, embedding_dim=2, loss=losses.Absolute, constraint=None, metric="euclidean",
                 seed=None, device=None, weights=None, selection="uniform", init="random"):
        parse_weights(weights, allow_matrix=False)
        self.init = check_init(init)
        selection = _landmarks.resolve_selection(selection)
        metric = check_source(data, metric)
        quality._check_matrix(data, "data")
        n = int(data.shape[0])
        m = check_landmarks(landmarks, n, constraint)
        embedding_dim = int(embedding_dim)
        if not 1 <= embedding_dim <= MAX_DIM:
            raise ValueError(f"embedding_dim must lie in [1, {MAX_DIM}] for a dense problem, got {embedding_dim}")
        loss_spec(loss)
        if seed is None:
            seed = int(util.np_rng().integers(0, 2 ** 63 - 1))
        self.n_items = n
        self.embedding_dim = embedding_dim
        self.metric = metric
        self.loss = loss
        self.weights = weights
        self.selection = selection
        self.landmark_radius = None
        if selection == _landmarks.UNIFORM:
            self.landmarks = quality._sample_rows(n, m, seed).to(torch.int64)
        else:
            chosen = _landmarks.select(data, m, method=selection, metric=metric, seed=seed, device=device)
            self.landmarks = chosen.indices.cpu()
            self.landmark_radius = float(chosen.distance.max())
        placed = torch.ones(n, dtype=torch.bool)
        placed[self.landmarks] = False
        self.placed = placed.nonzero().reshape(-1)
        self._data = data
        self._landmark_data = _take_rows(data, self.landmarks)
        self.landmark_problem = DenseMDE(self._landmark_data, embedding_dim=embedding_dim, loss=loss,
                                         constraint=constraints.Centered(), metric=metric, device=device,
                                         weights=weights, init=init)
        self.device = self.landmark_problem.device
        self.placement = None
        self.X = None
        self.value = None
        self.solve_stats = None

    @classmethod
    def from_graph(cls, graph, landmarks, embedding_dim=2, loss=losses.Absolute, constraint=None, seed=None,
                   selection="uniform", init="random", max_length=None, weights=None):
        """Landmark MDS on a ``Graph`` under its shortest-path metric (Landmark Isomap when the graph is a k-NN
        graph, ``preprocess.neighbor_graph``): one ``graph.distances_from(graph, landmarks)`` call gives the lengths
        ``D`` [n, m] from the ``landmarks`` chosen nodes to every node; the landmark stage is a ``DenseMDE`` on the
        m x m block of ``D`` (made symmetric by the element-wise minimum of the two directions, which are both lengths
        of real paths and can differ in the last bit), the placement stage a ``DensePlacement`` of every other node
        against its row of ``D``.  O(n m) memory, never n^2.

        A (node, landmark) pair that no path joins (of length at most ``max_length``, if given) is MISSING, not
        infinitely far: both stages then get a zero/one weight matrix, as ``DenseMDE.from_graph`` builds one (only
        then: it doubles the memory).  A node joined to no landmark has no position and is a ``ValueError``.
        ``selection``: ``"uniform"`` or ``"farthest"`` (``landmarks.select_graph``: every component gets a landmark
        before any gets a second one); ``"kmeans++"`` is a ``ValueError`` on a graph.  ``init="classical"`` needs
        every pair.  ``weights``: ``None`` or a number ``p`` (the power form), and only when no pair is missing, since
        the reachability mask then takes the matrix slot.  Everything else as for ``LandmarkMDE``, whose attributes
        and ``embed()`` these are; ``metric`` is ``None``."""
        check_init(init)
        return cls._build_from_graph(graph, landmarks, embedding_dim, loss, constraint, seed, selection, init,
                                     max_length, weights)

    @classmethod
    def _build_from_graph(cls, graph, landmarks, embedding_dim, loss, constraint, seed, selection, init, max_length,
                          weights):
        """``from_graph``; ``init=None`` (``preserve_geodesics``) is "classical" when every (node, landmark) pair is
        joined and "random" otherwise, with one logged line saying why."""
        parsed = parse_weights(weights, allow_matrix=False)
        selection = _landmarks.resolve_selection(selection)
        if selection == _landmarks.KMEANSPP:
            raise ValueError("selection='kmeans++' draws by squared distances to the rows of a data matrix; on a Graph "
                             "the selections are 'uniform' and 'farthest'")
        if not isinstance(graph, _graph.Graph):
            raise ValueError("`graph` must be a pymde_amd.Graph instance.")
        n = int(graph.n_items)
        m = check_landmarks(landmarks, n, constraint)
        embedding_dim = int(embedding_dim)
        if not 1 <= embedding_dim <= MAX_DIM:
            raise ValueError(f"embedding_dim must lie in [1, {MAX_DIM}] for a dense problem, got {embedding_dim}")
        loss_spec(loss)
        if seed is None:
            seed = int(util.np_rng().integers(0, 2 ** 63 - 1))
        self = cls.__new__(cls)
        self.n_items, self.embedding_dim, self.metric, self.loss = n, embedding_dim, None, loss
        self.weights, self.selection, self.landmark_radius = weights, selection, None
        if selection == _landmarks.UNIFORM:
            self.landmarks = quality._sample_rows(n, m, seed).to(torch.int64)
        else:
            chosen = _landmarks.select_graph(graph, m, seed=seed, max_length=max_length)
            self.landmarks = chosen.indices.cpu()
            self.landmark_radius = float(chosen.distance.max())
        placed = torch.ones(n, dtype=torch.bool)
        placed[self.landmarks] = False
        self.placed = placed.nonzero().reshape(-1)
        D = _graph.distances_from(graph, self.landmarks, max_length=max_length)
        device = D.device
        joined = torch.isfinite(D)
        others = joined.sum(dim=1)
        others[self.landmarks.to(device)] -= 1           # (a landmark's own column does not place it)
        stranded = int((others == 0).sum())
        if stranded:
            raise ValueError(f"{stranded} of the {n} nodes are joined to no landmark but themselves (no path"
                             + (f" of length at most {max_length}" if max_length is not None else "")
                             + " reaches them from any of the chosen nodes): such a node has no position; use more "
                             "landmarks or selection='farthest', which visits every component first")
        missing = int(joined.numel() - int(joined.sum()))
        if missing and parsed.source != W_NONE:
            raise ValueError(f"`weights`={weights!r} cannot be combined with missing pairs: {missing} (node, landmark) "
                             "pairs of this graph are joined by no path, and the zero/one mask that leaves them out "
                             "takes the place of the weight matrix")
        if init is None:
            init = "random" if missing else "classical"
            if missing:
                _problem.LOGGER.info(f"init='random': {missing} of the {n * m} (node, landmark) pairs are joined by no "
                                     "path, and the classical start needs every pair")
        elif init == "classical" and missing:
            raise ValueError(f"init='classical' needs every pair, and {missing} of the {n * m} (node, landmark) pairs "
                             "of this graph are joined by no path")
        self.init = init
        at = self.landmarks.to(device)
        block = D[at]
        block = torch.minimum(block, block.T).contiguous()
        self._data = self._landmark_data = None
        self._D = D[self.placed.to(device)]
        self._W = torch.isfinite(self._D).to(torch.float32) if missing else None
        del D, joined
        self.landmark_problem = DenseMDE(distance_matrix=block, embedding_dim=embedding_dim, loss=loss,
                                         constraint=constraints.Centered(), device=device,
                                         weights=torch.isfinite(block).to(torch.float32) if missing else weights,
                                         init=init)
        self.device = self.landmark_problem.device
        self.placement = None
        self.X = None
        self.value = None
        self.solve_stats = None
        return self

    def _placement(self, X_l):
        start = "triangulation" if self.init == "classical" else "neighbors"
        if self._data is None:   # from_graph: the rows of the shortest-path lengths
            return DensePlacement.weighted(None, X_l, None, distance_matrix=self._D, loss=self.loss,
                                           device=self.device, weights=self.weights if self._W is None else self._W,
                                           init=start)
        return DensePlacement.weighted(self._landmark_data, X_l, _take_rows(self._data, self.placed), loss=self.loss,
                                       metric=self.metric, device=self.device, weights=self.weights,
                                       init="triangulation" if self.init == "classical" else "neighbors")

    def initialization(self):
        """The [n, d] start of both stages, without solving: the landmarks where their problem starts (with
        ``init="classical"`` their classical scaling) and every other row where the placement starts against those
        (triangulated)."""
        problem = self.landmark_problem
        if self.init == "classical":
            X_l = problem.classical_initialization()
        else:
            X_l = problem.constraint.initialization(problem.n_items, self.embedding_dim, self.device)
        out = torch.empty((self.n_items, self.embedding_dim), dtype=torch.float32, device=self.device)
        out[self.landmarks.to(self.device)] = X_l
        out[self.placed.to(self.device)] = self._placement(X_l).initialization()
        return out

    def embed(self, X=None, placement_solver="joint", **solver_args):
        """Embed the landmarks, place the other rows, centre the whole: stores the [n, d] embedding in ``self.X`` and
        returns it.  ``X``: an optional [n, d] start for both stages; ``solver_args`` as in ``DenseMDE.embed``, for
        both stages; ``placement_solver`` (``"joint"`` or ``"rows"``) is the ``solver`` of ``DensePlacement.embed``,
        for the placement stage only."""
        _rows.check_solver(placement_solver, "placement_solver")
        start_l = start_p = None
        if X is not None:
            if tuple(X.shape) != (self.n_items, self.embedding_dim):
                raise ValueError(f"the start must have shape ({self.n_items}, {self.embedding_dim}), got "
                                 f"{tuple(X.shape)}")
            X = X.detach().to(device=self.device, dtype=torch.float32)
            start_l, start_p = X[self.landmarks.to(self.device)], X[self.placed.to(self.device)]
        X_l = self.landmark_problem.embed(start_l, **solver_args)
        self.placement = self._placement(X_l)
        X_p = self.placement.embed(start_p, solver=placement_solver, **solver_args)
        out = torch.empty((self.n_items, self.embedding_dim), dtype=torch.float32, device=self.device)
        out[self.landmarks.to(self.device)] = X_l
        out[self.placed.to(self.device)] = X_p
        self.X = constraints.Centered().project_onto_constraint(out, inplace=True)
        self.value = self.placement.value
        self.solve_stats = LandmarkSolveStats(self.landmark_problem.solve_stats, self.placement.solve_stats)
        return self.X

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
"""
import collections
import math

import torch

from pymde_amd import _lib
from pymde_amd import constraints
from pymde_amd import metrics as _metrics
from pymde_amd import optim
from pymde_amd import preprocess
from pymde_amd import problem as _problem
from pymde_amd import quality
from pymde_amd import util
from pymde_amd.functions import function as _function
from pymde_amd.functions import losses

MAX_DIM = 8            # PAIR_LOSS_MAX_D of csrc/mde_pair_loss.hip
MAX_SLICES = 65535     # CROSS_MAX_SLICES of csrc/mde_knn_slices.h
SYMMETRY_RTOL = 1e-5   # |D - D^T| may reach this fraction of the largest entry (a float32 product of two roundings)
_FIRST_LOSS = _function.KIND["L_QUADRATIC"]

LossSpec = collections.namedtuple("LossSpec", ["kind", "scalars", "weighted"])
LossSpec.__doc__ = """What ``mde_pair_loss`` needs of a loss: its ``kind`` (MDE_F_L_* of include/mde_hip.h), its three
``scalars``, and whether it is ``weighted`` (by the default ``1 / delta^2``, which the kernel forms itself)."""

_ACCEPTED = ("a dense problem takes a loss of pymde_amd.losses as a callable of the deviations -- a class (Quadratic, "
             "WeightedQuadratic, Huber, Cubic, Power, Absolute, Logistic, Fractional, SoftFractional) or a "
             "functools.partial of one that fixes its threshold / exponent / gamma -- with the default weights")


def loss_spec(loss):
    """The ``LossSpec`` of ``loss``, a callable of the deviations as the recipes take it.  Needs no GPU: the callable
    is tried on ``torch.ones(1)``.  ``ValueError`` (naming what is accepted) for a penalty, for a callable whose
    result has no ``_hip_spec``, and for weights other than the default ``1 / delta^2``: a dense problem has no
    per-pair arrays."""
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
                raise ValueError(f"{type(f).__name__} was given weights of its own; a dense problem has no per-pair "
                                 f"arrays and weighs by the default 1 / delta^2; {_ACCEPTED}")
    return LossSpec(int(spec.kind), tuple(float(s) for s in spec.scalars), weighted)


def check_source(data, metric):
    """Canonical name of a metric the Gram tile serves; ``ValueError`` for Manhattan and for a ``Graph`` (no device is
    needed to say so)."""
    metric = _metrics.resolve(metric)
    if preprocess._is_graph(data):
        raise ValueError("a dense problem forms its deviations from the rows of a data matrix; for a Graph pass its "
                         "shortest-path lengths as DenseMDE(distance_matrix=...), or use the edge-list problem "
                         "(preserve_distances(graph) with dense=False)")
    if metric not in quality._RANKED_METRICS:
        raise ValueError(f"metric={metric!r} has no Gram tile; dense problems support 'euclidean', 'cosine' and "
                         "'correlation' (pass other distances as DenseMDE(distance_matrix=...))")
    return metric


def _pair_loss(X, spec, A=None, mode=0, Dm=None, d_scale=1.0, slices=0, work=None):
    """``mde_pair_loss`` on prepared float32 tensors on one GPU: ``(loss float64 [1], grad float32 [n, d], row_loss
    float64 [n])`` on that GPU.  Exactly one of ``A`` (the prepared data rows) and ``Dm`` (the [n, n] matrix)."""
    n, d, device = int(X.shape[0]), int(X.shape[1]), X.device
    lib = _lib.load()
    loss = torch.empty(1, dtype=torch.float64, device=device)
    grad = torch.empty((n, d), dtype=torch.float32, device=device)
    row_loss = torch.empty(n, dtype=torch.float64, device=device)
    with torch.cuda.device(device):
        if work is None:
            work = _work(lib, n, d, slices, device)
        _lib.check(lib.mde_pair_loss(n, 0 if A is None else int(A.shape[1]), _lib.ptr(A), mode, _lib.ptr(Dm),
                                     float(d_scale), d, _lib.ptr(X), spec.kind, spec.scalars[0], spec.scalars[1],
                                     spec.scalars[2], slices, _lib.ptr(loss), _lib.ptr(grad), _lib.ptr(row_loss),
                                     _lib.ptr(work), _lib.stream_ptr(device)))
    return loss, grad, row_loss


def _work(lib, n, d, slices, device):
    nbytes = int(lib.mde_pair_loss_work_bytes(n, d, slices))
    if nbytes < 0:
        _lib.check(nbytes)
    return torch.empty(nbytes, dtype=torch.uint8, device=device)


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


def _check_distance_matrix(D):
    """Finite, non-negative, symmetric: one pass on the GPU in row blocks, one read-back; ``ValueError`` saying which."""
    n = int(D.shape[0])
    flags = torch.zeros(2, dtype=torch.int64, device=D.device)
    worst = torch.zeros(2, dtype=torch.float32, device=D.device)          # the largest entry, the largest |D - D^T|
    step = max(1, min(n, (1 << 24) // n))
    for lo in range(0, n, step):
        block = D[lo:lo + step]
        flags[0] += (~torch.isfinite(block)).sum()
        flags[1] += (block < 0).sum()
        worst[0] = torch.maximum(worst[0], block.abs().max())
        worst[1] = torch.maximum(worst[1], (block - D[:, lo:lo + step].T).abs().max())
    (bad, negative), (top, asym) = flags.tolist(), worst.tolist()
    if bad:
        raise ValueError(f"`distance_matrix` is not finite: {bad} of its entries are NaN or infinite")
    if negative:
        raise ValueError(f"`distance_matrix` is not non-negative: {negative} of its entries are below zero")
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

    After ``embed()``: ``X``, ``solve_stats``, ``value`` and ``residual_norm``, as for ``MDE``.  The per-pair
    ``distances`` / ``distortions`` / ``high_distortion_pairs`` of ``MDE`` are n^2 values and are not provided;
    ``item_distortions`` has one value per item.  With ``Anchored`` the anchor-anchor pairs stay in the mean: they
    add a constant to the value and nothing to the gradient of the free rows."""

    def __init__(self, data=None, embedding_dim=2, loss=losses.Absolute, constraint=None, distance_matrix=None,
                 metric="euclidean", deviation_scale=1.0, device=None):
        if (data is None) == (distance_matrix is None):
            raise ValueError("exactly one of `data` and `distance_matrix` must be given")
        embedding_dim = int(embedding_dim)
        if not 1 <= embedding_dim <= MAX_DIM:
            raise ValueError(f"embedding_dim must lie in [1, {MAX_DIM}] for a dense problem (the kernel keeps a "
                             f"row of the embedding in registers), got {embedding_dim}")
        self._spec = loss_spec(loss)
        deviation_scale = float(deviation_scale)
        if not (deviation_scale > 0.0 and math.isfinite(deviation_scale)):
            raise ValueError(f"deviation_scale must be a positive finite number, got {deviation_scale!r}")
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
        if device is None:
            device = source.device if isinstance(source, torch.Tensor) and source.is_cuda else util.get_default_device()
        self.device = util.require_cuda_device(device)
        self._A, self._Dm, self._mode = None, None, 0
        if data is not None:
            self._A = quality._self_rows(data, metric, self.device, "data")
            self._mode = quality._pair_modes(metric)[0]
        else:
            self._Dm = torch.as_tensor(distance_matrix).to(device=self.device, dtype=torch.float32).contiguous()
            _check_distance_matrix(self._Dm)
        self.n_items = n
        self.embedding_dim = embedding_dim
        self.p = n * (n - 1) // 2
        self.metric = metric if data is not None else None
        self.deviation_scale = deviation_scale
        self.loss = loss
        self.constraint = constraints.Centered() if constraint is None else constraint
        self.X = None
        self.solve_stats = None
        self.value = None
        self.residual_norm = None
        self._work_buffer = None

    def __str__(self):
        source = "data matrix, metric %s" % self.metric if self._A is not None else "distance matrix"
        return ("Dense MDE problem:\n\tn (number of items) {0}\n\tm (embedding dimension) {1}\n"
                "\tp (number of pairs, all of them) {2}\n\tdeviations from a {3}\n\tconstraint {4}\n\tdevice {5}".format(
                    self.n_items, self.embedding_dim, self.p, source, self.constraint.name(), self.device))

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
                          d_scale=self.deviation_scale, work=self._work_buffer)

    # ------------------------------------------------------------------ evaluators
    def average_distortion(self, X=None):
        """The average distortion of ``X`` over all pairs (a 0-dim float32 tensor; differentiable w.r.t. ``X``)."""
        return _DenseDistortion.apply(self._embedding_arg(X), self)

    def item_distortions(self, X=None):
        """float32 [n]: for every item the mean of the loss over its ``n - 1`` pairs (colour a plot by it).  Their
        mean is the average distortion."""
        row_loss = self._evaluate(self._embedding_arg(X).detach())[2]
        return (row_loss / float(self.n_items - 1)).to(torch.float32)

    # ------------------------------------------------------------------ the solve
    def embed(self, X=None, eps=1e-5, max_iter=300, memory_size=10, verbose=False, print_every=None,
              snapshot_every=None):
        """Compute an embedding; stores it in ``self.X`` and returns it.  Arguments as in ``MDE.embed``."""
        if X is None:
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

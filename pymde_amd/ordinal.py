"""Ordinal (non-metric) MDS over an edge list: Kruskal's alternation on the GPU.

A metric problem takes its deviations at face value.  ``OrdinalMDE`` uses their ORDER only: it looks for an
embedding whose distances are a monotone function of the deviations, whatever that function is -- similarity
judgements, ranks, hop counts, distances that went through an unknown monotone distortion.  A round

  1. takes the embedding distances of the current ``X`` into the rank order of the deviations,
  2. fits the disparities: the isotonic regression of those distances (``pymde_amd.isotonic``), tied deviations
     pooled beforehand into their mean distance and weighed by their number (the secondary treatment of ties,
     scikit-learn's: tied deviations receive one disparity),
  3. rescales the disparities to a fixed root mean square and writes them, in place, over the deviations of an
     inner metric ``MDE``,
  4. runs a few L-BFGS iterations of that problem from ``X``.

The inner problem is an ordinary edge-list ``MDE``: its binding re-expands the per-edge parameter stream when the
deviations tensor has been written, so no edge kernel, solver or plan knows about any of this.

Out of scope: Kruskal's primary treatment of ties, ordinal dense and landmark problems, ``Anchored`` constraints,
sharded problems, monotone splines, and folding the regression into every evaluation.
"""
import torch

from pymde_amd import constraints
from pymde_amd import dense as _dense
from pymde_amd import isotonic
from pymde_amd import preprocess
from pymde_amd import problem
from pymde_amd import util
from pymde_amd.functions import losses

METRIC_START_ITER = 300     # iterations of the metric solve of round 0: MDE.embed's own default


class OrdinalMDE(object):
    """``OrdinalMDE(n_items, embedding_dim, edges, deviations, *, loss=losses.Quadratic, constraint=None,
    device=None)``: an ordinal MDS problem over ``edges`` (int64 [p, 2]).  Only the order of ``deviations`` and its
    ties are used; they are sorted once, in the floating-point type they come in (anything else as float64).

    ``loss``: a class of ``pymde_amd.losses`` or a ``functools.partial`` of one, as ``dense.loss_spec`` takes them;
    the inner ``MDE`` (``.problem``) minimises it between the distances and the rescaled disparities.  A loss with
    per-edge weights is a ``ValueError``: ``WeightedQuadratic``'s ``1 / delta^2`` would go stale when the
    deviations are replaced.  ``constraint``: ``None`` / ``Centered()`` or ``Standardized()``; the disparities are
    rescaled to root mean square 1, or to the constraint's natural length under ``Standardized``.  ``Anchored`` is
    a ``ValueError``: pinned rows fix a scale that this normalisation would fight.  NaN or infinite deviations
    are a ``ValueError``.

    After ``embed()``: ``X``, ``stress_`` (Kruskal's stress-1), ``stress_history`` (the stress at the start and
    after every round), ``rounds_``, ``disparities_`` (of ``X``, in edge order), ``solve_stats`` (of the last
    inner solve) and ``problem``."""

    def __init__(self, n_items, embedding_dim, edges, deviations, *, loss=losses.Quadratic, constraint=None,
                 device=None):
        if _dense.loss_spec(loss).weighted:
            raise ValueError("an ordinal problem replaces the deviations every round, and per-edge weights derived "
                             "from them (WeightedQuadratic's 1 / delta^2) would go stale; pass an unweighted loss")
        if isinstance(constraint, constraints.Anchored):
            raise ValueError("OrdinalMDE does not take an Anchored constraint: the pinned rows fix a scale, and the "
                             "disparities are rescaled every round")
        if constraint is None:
            constraint = constraints.Centered()
        if device is None:
            device = edges.device if isinstance(edges, torch.Tensor) and edges.is_cuda else util.get_default_device()
        self.device = util.require_cuda_device(device)
        if not isinstance(edges, torch.Tensor):
            edges = torch.as_tensor(edges, dtype=torch.int64)
        edges = edges.to(self.device)
        if not isinstance(deviations, torch.Tensor):
            deviations = torch.as_tensor(deviations)
        deviations = deviations.detach().to(self.device)
        if not deviations.is_floating_point() or deviations.dtype not in (torch.float32, torch.float64):
            deviations = deviations.to(torch.float64)
        if deviations.dim() != 1 or edges.dim() != 2 or deviations.shape[0] != edges.shape[0]:
            raise ValueError(f"`deviations` must hold one value per edge (got {tuple(deviations.shape)} for edges "
                             f"of shape {tuple(edges.shape)})")
        if deviations.numel() == 0:
            raise ValueError("an ordinal problem needs at least one edge")
        if not bool(torch.isfinite(deviations).all()):
            raise ValueError("`deviations` must be finite")
        self.n_items, self.embedding_dim = int(n_items), int(embedding_dim)
        self.constraint = constraint
        self.length = (float(constraint.natural_length(self.n_items, self.embedding_dim))
                       if isinstance(constraint, constraints._Standardized) else 1.0)

        # the rank order, once: a stable sort, and the groups of tied deviations (contiguous in rank order)
        ranked, self._order = torch.sort(deviations, stable=True)
        self._rank = torch.empty_like(self._order)
        p = int(ranked.numel())
        self._rank[self._order] = torch.arange(p, device=self.device)
        first = torch.ones(p, dtype=torch.bool, device=self.device)
        first[1:] = ranked[1:] != ranked[:-1]
        starts = torch.nonzero(first).reshape(-1)
        self.n_groups = int(starts.numel())
        self._deviations_ranked = ranked
        if self.n_groups < p:
            ends = torch.cat([starts[1:], torch.tensor([p], device=self.device)])
            self._group = torch.cumsum(first.to(torch.int64), 0) - 1
            self._starts, self._ends = starts, ends
            self._sizes = (ends - starts).to(torch.float64)
            self._weights = self._sizes.to(torch.float32)
        else:
            self._group = self._weights = None
        self._work = isotonic.work_buffer(self.n_groups, self.device)

        self._d0 = preprocess.scale(deviations.to(torch.float32), self.length)
        self.problem = problem.MDE(self.n_items, self.embedding_dim, edges, loss(self._d0.clone()),
                                   constraint=constraint, device=self.device)
        self.edges = self.problem.edges
        self.X = None
        self.stress_ = None
        self.stress_history = []
        self.rounds_ = 0
        self.disparities_ = None
        self.solve_stats = None

    def __str__(self):
        ties = "no ties" if self._group is None else f"{self.n_groups} distinct deviations"
        return (f"Ordinal MDE problem:\n\tn (number of items) {self.n_items}\n\tm (embedding dimension) "
                f"{self.embedding_dim}\n\tp (number of edges) {int(self._order.numel())} ({ties})\n"
                f"\tconstraint {self.constraint.name()}\n\tdevice {self.device}")

    # ------------------------------------------------------------------ disparities
    def _group_means(self, ranked):
        """What the regression is run on: float32 ``ranked`` distances themselves when no deviations are tied,
        else the mean distance of every tie group (the regression then weighs it by the group's size)."""
        if self._group is None:
            return ranked
        # a group's sum as a difference of double prefix sums: a fixed order of additions, no atomics
        prefix = torch.cumsum(ranked.double(), 0)
        upper = prefix[self._ends - 1]
        lower = torch.where(self._starts > 0, prefix[(self._starts - 1).clamp_(min=0)],
                            torch.zeros((), dtype=torch.float64, device=self.device))
        means = ((upper - lower) / self._sizes).to(torch.float32)
        return means.clamp_(min=0.0)               # (the difference of two rounded prefixes can fall below 0)

    def _regress(self, values):
        """The isotonic regression of ``_group_means``' result, one value per tie group."""
        return isotonic.run(values, self._weights, torch.empty_like(values), self._work)

    def _expand(self, fit):
        """A value per tie group, in rank order, to a value per edge in edge order."""
        if self._group is not None:
            fit = fit[self._group]
        return fit[self._rank]

    def _fit(self, distances):
        """The disparities, in edge order, of float32 ``distances`` in edge order."""
        return self._expand(self._regress(self._group_means(distances[self._order])))

    def _distances(self, X):
        return self.problem.distances(X).detach()

    def disparities(self, X=None):
        """The disparities of ``X`` (default: the embedding of the last ``embed()``): float32, one per edge in edge
        order, not rescaled -- the monotone function of the deviations' ranks that is closest to the embedding
        distances in least squares, tied deviations sharing one value."""
        return self._fit(self._distances(self._X_arg(X)))

    @staticmethod
    def _stress(distances, disparities):
        d = distances.double()
        return float(((d - disparities.double()).pow(2).sum() / d.pow(2).sum()).sqrt())

    def stress(self, X=None):
        """Kruskal's stress-1 of ``X``: ``sqrt(sum (d - dhat)^2 / sum d^2)`` over the edges, summed in float64."""
        d = self._distances(self._X_arg(X))
        return self._stress(d, self._fit(d))

    def shepard(self, X=None):
        """``(deviations, distances, disparities)`` of ``X`` in rank order: the three columns of a Shepard
        diagram."""
        d = self._distances(self._X_arg(X))
        return self._deviations_ranked, d[self._order], self._fit(d)[self._order]

    def _X_arg(self, X):
        if X is None:
            X = self.X
        if X is None:
            raise ValueError("Call this function after running the `embed` method, or provide a value for the "
                             "embedding argument `X`")
        return X

    # ------------------------------------------------------------------ the alternation
    def embed(self, X=None, rounds=50, inner_iter=15, tol=1e-4, eps=1e-5, memory_size=10, metric_start=True,
              verbose=False):
        """Alternate disparities and a few iterations of the inner metric problem; stores the embedding in
        ``self.X`` and returns it.

        With ``X=None`` and ``metric_start=True`` round 0 solves the inner problem on the (rescaled) deviations
        themselves -- the metric solution, ``MDE.embed`` with its defaults -- and the alternation starts there; a
        random start can stall far from the order the data has.  With ``X`` given the alternation starts at ``X``,
        which must satisfy the constraint.  Every round then computes the disparities of the current embedding,
        rescales them to the root mean square the constraint asks for, writes them over the inner problem's
        deviations and calls its ``embed(X, max_iter=inner_iter, eps=eps, memory_size=memory_size)``.  The
        alternation stops after ``rounds`` rounds, when a round has improved the stress by less than ``tol``
        relative, or -- keeping the earlier embedding -- when a round has made it worse.

        The defaults (50 rounds of 15 iterations, ``tol=1e-4``) are choices, not measurements."""
        if rounds < 0 or inner_iter < 0:
            raise ValueError("`rounds` and `inner_iter` must not be negative")
        inner = self.problem.distortion_function
        if X is None:
            if metric_start:
                inner.deviations.copy_(self._d0)
                X = self.problem.embed(eps=eps, max_iter=METRIC_START_ITER, memory_size=memory_size)
            else:
                X = self.constraint.initialization(self.n_items, self.embedding_dim, self.device)
        X = X.detach().to(device=self.device, dtype=torch.float32).clone()
        history = []
        fit = None
        self.rounds_ = 0
        for r in range(rounds + 1):
            d = self._distances(X)
            new_fit = self._fit(d)
            s = self._stress(d, new_fit)
            if history and s > history[-1]:
                X = previous                       # the round made it worse: keep what there was
                self.rounds_ -= 1
                break
            fit = new_fit
            history.append(s)
            if verbose:
                problem.LOGGER.info(f"ordinal round {r}: stress-1 {s:.6g}")
            if r == rounds or (r > 0 and history[-2] - s < tol * history[-2]):
                break
            rms = float(fit.double().pow(2).mean().sqrt())
            if not rms > 0.0:
                break                              # every distance is 0: there is nothing to fit
            inner.deviations.copy_(fit * (self.length / rms))
            previous = X
            X = self.problem.embed(X, eps=eps, max_iter=inner_iter, memory_size=memory_size)
            self.rounds_ += 1
        self.X = X
        self.problem.X = X
        self.stress_history = history
        self.stress_ = history[-1]
        self.disparities_ = fit
        self.solve_stats = self.problem.solve_stats
        return self.X

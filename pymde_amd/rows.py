"""The per-row solver of a dense placement (``csrc/mde_rows.hip``).

The objective of ``DensePlacement`` is a sum of independent d-dimensional problems (d <= 8), one per new row.  The
joint solver minimises it with ONE L-BFGS, so one step length must suit every row and the curvature pairs mix rows
that do not interact.  Here every row runs its own BFGS with its own backtracking line search and its own stopping
test, all rows in lock step: a sweep is one ``mde_pair_loss_cross_rows`` over the rows that are still working, one
``mde_rows_step`` over all rows, and one read-back of three counters.  A row that has converged (``|g_i| <= eps``) or
stalled leaves the list, so the later sweeps cost what the unfinished rows cost.

``|g_i|_2 <= eps`` for every row gives a joint residual norm ``sqrt(sum |g_i|^2) / n <= eps``: the per-row criterion
implies the joint solver's.
"""
import collections
import time

import torch

from pymde_amd import _lib
from pymde_amd import optim

ACTIVE, CONVERGED, STALLED = 0, 1, 2   # MDE_ROWS_* of include/mde_hip.h
REBUILD_BELOW = 0.75                   # the list is rebuilt when the active rows fall below this share of it
SOLVERS = ("joint", "rows")

RowsResult = collections.namedtuple("RowsResult", ["X", "solve_stats", "row_status", "value", "residual_norm"])
RowsResult.__doc__ = """What ``solve`` returns: the rows, the ``SolveStats``, the status of every row (int32: 0 still
active, 1 converged, 2 stalled), and the value and residual norm at ``X`` (also the last entries of the stats, when
there was a sweep)."""


def check_solver(solver, name="solver"):
    """``solver`` if it names one; ``ValueError`` otherwise (no device is needed to say so)."""
    if solver not in SOLVERS:
        raise ValueError(f"`{name}` must be 'joint' (one L-BFGS over all new rows) or 'rows' (a BFGS per row, "
                         f"pymde_amd.rows), got {solver!r}")
    return solver


def work_cross_rows(lib, n_q, n_c, d, slices, device):
    return _lib.work_buffer(lib.mde_pair_loss_cross_rows_work_bytes, n_q, n_c, d, slices, device=device)


def pair_loss_cross_rows(XQ, XC, spec, row_loss, row_grad, rows=None, Q=None, C=None, mode=0, Dm=None, d_scale=1.0,
                         slices=0, work=None, weights=None):
    """``mde_pair_loss_cross_rows`` on prepared float32 tensors on one GPU: writes ``row_loss`` (float64 [n_q]) and
    ``row_grad`` (float32 [n_q, d]) at the rows of ``rows`` (int32, distinct; ``None``: all rows) and nowhere else.
    With ``weights`` (a ``dense.Weights``; ``W`` [n_q, n_c] float32 on that GPU) ``mde_pair_loss_cross_rows_weighted``:
    the same sums with a weight per pair, still divided by ``n_c``."""
    n_q, n_c, d, device = int(XQ.shape[0]), int(XC.shape[0]), int(XQ.shape[1]), XQ.device
    lib = _lib.load()
    n_rows = n_q if rows is None else int(rows.shape[0])
    with torch.cuda.device(device):
        if work is None:
            work = work_cross_rows(lib, n_q, n_c, d, slices, device)
        head = (n_q, n_c, 0 if Q is None else int(Q.shape[1]), _lib.ptr(Q), _lib.ptr(C), mode, _lib.ptr(Dm),
                float(d_scale), d, _lib.ptr(XQ), _lib.ptr(XC), spec.kind, spec.scalars[0], spec.scalars[1],
                spec.scalars[2], slices, n_rows, _lib.ptr(rows))
        tail = (_lib.ptr(row_loss), _lib.ptr(row_grad), _lib.ptr(work), _lib.stream_ptr(device))
        if weights is None:
            _lib.check(lib.mde_pair_loss_cross_rows(*head, *tail))
        else:
            _lib.check(lib.mde_pair_loss_cross_rows_weighted(*head, weights.source, weights.p, _lib.ptr(weights.W),
                                                             *tail))
    return row_loss, row_grad


class RowState(object):
    """The device arrays of ``mde_rows_init`` / ``mde_rows_step`` for ``n`` rows of dimension ``d``, and the calls."""

    def __init__(self, n, d, n_c, eps, device):
        self.n, self.d, self.n_c, self.eps, self.device = int(n), int(d), int(n_c), float(eps), device
        f32 = dict(dtype=torch.float32, device=device)
        self.x = torch.empty((n, d), **f32)
        self.f = torch.empty(n, dtype=torch.float64, device=device)
        self.g = torch.empty((n, d), **f32)
        self.H = torch.empty((n, d, d), **f32)
        self.p = torch.empty((n, d), **f32)
        self.t = torch.empty(n, **f32)
        self.flags = torch.empty(n, dtype=torch.int32, device=device)
        self.x_trial = torch.empty((n, d), **f32)
        self.counts = torch.empty(3, dtype=torch.int64, device=device)

    def status(self):
        return self.flags & 3

    def init(self, x, row_loss, row_grad):
        self.x.copy_(x)
        with torch.cuda.device(self.device):
            _lib.check(_lib.load().mde_rows_init(
                self.n, self.d, self.n_c, self.eps, _lib.ptr(self.x), _lib.ptr(row_loss), _lib.ptr(row_grad),
                _lib.ptr(self.f), _lib.ptr(self.g), _lib.ptr(self.H), _lib.ptr(self.p), _lib.ptr(self.t),
                _lib.ptr(self.flags), _lib.ptr(self.x_trial), _lib.ptr(self.counts), _lib.stream_ptr(self.device)))

    def step(self, row_loss, row_grad):
        with torch.cuda.device(self.device):
            _lib.check(_lib.load().mde_rows_step(
                self.n, self.d, self.n_c, self.eps, _lib.ptr(self.x), _lib.ptr(self.f), _lib.ptr(self.g),
                _lib.ptr(self.H), _lib.ptr(self.p), _lib.ptr(self.t), _lib.ptr(self.flags), _lib.ptr(self.x_trial),
                _lib.ptr(row_loss), _lib.ptr(row_grad), _lib.ptr(self.counts), _lib.stream_ptr(self.device)))


def solve(evaluate, X, n_c, eps=1e-5, max_iter=300, snapshot_every=None, verbose=False, print_every=None,
          logger=None, scale=1.0):
    """Minimise ``sum_i f_i(x_i)`` row by row.  ``evaluate(X, rows, row_loss, row_grad)`` writes, for the rows of
    ``rows`` (int32 on the device; ``None``: all), ``row_loss[i] = n_c f_i(X[i])`` (float64) and ``row_grad[i] = grad
    f_i`` (float32), as ``mde_pair_loss_cross_rows`` does.  ``X`` float32 [n, d] on the GPU is the start and is not
    modified.

    Returns a ``RowsResult``.  One entry per sweep in the stats: ``average_distortions`` the mean
    of f over all rows, ``residual_norms`` the Frobenius norm of the joint gradient ``sqrt(sum |g_i|^2) / n``,
    ``step_size_percents`` ``100 |dX|_F / |X|_F``; ``evaluations`` is in units of a full evaluation, the sum of the
    list lengths over ``n``, the first one included.  A row is still active only when ``max_iter`` ran out.

    ``scale`` multiplies the reported ``value``, ``residual_norm`` and the ``average_distortions`` / ``residual_norms``
    of the stats, afterwards: a placement that keeps ``p`` of its ``n n_c`` pairs passes ``n n_c / p``, which makes
    them the joint problem's (mean over the kept pairs).  The solve itself, and ``eps``, do not see it."""
    start_time = time.time()
    n, d, device = int(X.shape[0]), int(X.shape[1]), X.device
    state = RowState(n, d, n_c, eps, device)
    row_loss = torch.empty(n, dtype=torch.float64, device=device)
    row_grad = torch.empty((n, d), dtype=torch.float32, device=device)
    evaluate(X, None, row_loss, row_grad)
    state.init(X, row_loss, row_grad)
    active = int(state.counts.tolist()[ACTIVE])
    rows, listed, evaluated = None, n, n
    previous = torch.empty_like(state.x)
    per_sweep, times, snapshots = [], [], []
    if print_every is None:
        print_every = max(1, max_iter // 10)
    sweep = 0
    while active > 0 and sweep < max_iter:
        if active < REBUILD_BELOW * listed:
            # (every active row is in the old list, so the new one is a subset of it)
            rows = (state.status() == ACTIVE).nonzero().reshape(-1).to(torch.int32)
            listed = int(rows.shape[0])
        if snapshot_every is not None and sweep % snapshot_every == 0:
            snapshots.append(state.x.detach().cpu().clone())
        evaluate(state.x_trial, rows, row_loss, row_grad)
        evaluated += listed
        previous.copy_(state.x)
        state.step(row_loss, row_grad)
        per_sweep.append(torch.stack([state.f.mean(), state.g.double().square().sum().sqrt() / n,
                                      (state.x - previous).double().square().sum().sqrt(),
                                      state.x.double().square().sum().sqrt()]))
        counts = state.counts.tolist()          # the sweep's one read-back
        active = int(counts[ACTIVE])
        times.append(time.time() - start_time)
        sweep += 1
        if verbose and logger is not None and (sweep % print_every == 0 or active == 0):
            logger.info(f"sweep {sweep:03d} | active {active} converged {counts[CONVERGED]} stalled "
                        f"{counts[STALLED]} | rows evaluated {listed}")
    values, residuals, percents = [], [], []
    if per_sweep:
        table = torch.stack(per_sweep).cpu()
        values, residuals = table[:, 0].tolist(), table[:, 1].tolist()
        percents = (100.0 * table[:, 2] / table[:, 3]).tolist()
    value, residual = torch.stack([state.f.mean(), state.g.double().square().sum().sqrt() / n]).tolist()
    if scale != 1.0:
        values, residuals = [scale * v for v in values], [scale * v for v in residuals]
        value, residual = scale * value, scale * residual
    stats = optim.SolveStats(values, residuals, percents, time.time() - start_time, times, snapshots, snapshot_every,
                             evaluations=evaluated / float(n))
    return RowsResult(state.x, stats, state.status().to(torch.int32), value, residual)

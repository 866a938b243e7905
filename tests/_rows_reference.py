"""A float64 numpy mirror of the per-row placement solver (``csrc/mde_rows.hip``): the yardstick
for the kernel and, against scipy's BFGS on every row alone, for the algorithm itself.  Needs no GPU.

``state_dtype=np.float32`` rounds the state where the kernel rounds it (x, g, H, p, t and the trial point are float32;
every product and sum is formed in double from those terms), so that one step of the kernel can be compared with one
step of the mirror to float32 rounding.  ``np.float64`` keeps everything in double: the algorithm without the
storage format.
"""
import numpy as np

ACTIVE, CONVERGED, STALLED = 0, 1, 2
C1 = 1e-4
CURVATURE = 1e-10
SMALL = 1e-7
FLOOR = 1e-10


# ---------------------------------------------------------------------- the losses of the separable objective
def quadratic(E, D):
    return (E - D) ** 2, 2.0 * (E - D)


def huber(threshold):
    def loss(E, D):
        r = E - D
        a = np.abs(r)
        return (np.where(a < threshold, r * r, threshold * (2.0 * a - threshold)),
                np.where(a < threshold, 2.0 * r, 2.0 * threshold * np.sign(r)))
    return loss


def cubic(E, D):
    r = E - D
    return np.abs(r) ** 3, 3.0 * r * np.abs(r)


def absolute(E, D):
    return np.abs(E - D), np.sign(E - D)


def row_objective(loss, X_old, D):
    """``fun(X, rows) -> (f [len(rows)], g [len(rows), d])``: f_i = mean_j loss(|x_i - xold_j|, D[i, j]) and its
    gradient, in float64.  ``D`` [n_new, n_old]."""
    X_old = np.asarray(X_old, dtype=np.float64)
    D = np.asarray(D, dtype=np.float64)

    def fun(X, rows):
        diff = np.asarray(X, dtype=np.float64)[:, None, :] - X_old[None, :, :]
        E = np.sqrt((diff * diff).sum(2))
        l, dl = loss(E, D[rows])
        with np.errstate(divide="ignore", invalid="ignore"):
            w = dl / E
        w = np.where(np.isfinite(w), w, 1.0)                    # the NaN / Inf -> 1 rule of the kernels
        return l.mean(1), (w[:, :, None] * diff).mean(1)
    return fun


# ---------------------------------------------------------------------- the state and the two kernels
class State(object):
    """x [n, d], f [n], g [n, d], H [n, d, d], p [n, d], t [n], status / fresh / small [n] ints, x_trial [n, d]."""

    def __init__(self, x, f, g, H, p, t, status, fresh, small, x_trial, dtype):
        self.dtype = dtype
        self.x, self.g, self.H, self.p, self.t, self.x_trial = (np.array(a, dtype=dtype) for a in (x, g, H, p, t, x_trial))
        self.f = np.array(f, dtype=np.float64)
        self.status, self.fresh, self.small = (np.array(a, dtype=np.int32) for a in (status, fresh, small))

    def counts(self):
        return [int((self.status == v).sum()) for v in (ACTIVE, CONVERGED, STALLED)]

    def copy(self):
        return State(self.x, self.f, self.g, self.H, self.p, self.t, self.status, self.fresh, self.small,
                     self.x_trial, self.dtype)


def _d(a):
    return np.array(a, dtype=np.float64)       # (a copy: the state is updated in place)


def init(x, f, g, eps, state_dtype=np.float64):
    x = np.array(x, dtype=state_dtype)
    g = np.array(g, dtype=state_dtype)
    n, d = x.shape
    f = _d(f)
    finite = np.isfinite(f) & np.isfinite(g).all(1)
    with np.errstate(divide="ignore"):
        t = np.minimum(1.0, 1.0 / np.abs(_d(g)).sum(1)).astype(state_dtype)
    norm = np.sqrt((_d(g) ** 2).sum(1))
    status = np.where(~finite, STALLED, np.where(norm <= eps, CONVERGED, ACTIVE))
    H = np.broadcast_to(np.eye(d), (n, d, d))
    p = -g
    active = (status == ACTIVE)[:, None]
    x_trial = np.where(active, (_d(x) + _d(t)[:, None] * _d(p)).astype(state_dtype), x)
    return State(x, f, g, H, p, t, status, np.ones(n), np.zeros(n), x_trial, state_dtype)


def step(state, f_t, g_t, eps):
    """One lock-step update, in place: ``f_t`` [n] and ``g_t`` [n, d] are the evaluation at ``state.x_trial`` (only
    the entries of the active rows are read)."""
    S, dt = state, state.dtype
    d = S.x.shape[1]
    for i in np.nonzero(S.status == ACTIVE)[0]:
        x, g, p, t, f = _d(S.x[i]), _d(S.g[i]), _d(S.p[i]), float(S.t[i]), float(S.f[i])
        xt, gt, ft = _d(S.x_trial[i]), _d(np.asarray(g_t[i], dtype=dt)), float(f_t[i])
        gp = float(g @ p)
        if np.isfinite(ft) and np.isfinite(gt).all() and ft <= f + C1 * t * gp:
            s, y = xt - x, gt - g
            sy, ss, yy = float(s @ y), float(s @ s), float(y @ y)
            H = _d(S.H[i])
            if sy > CURVATURE * np.sqrt(ss) * np.sqrt(yy):
                if S.fresh[i]:
                    H = _d(dt(sy / yy)) * np.eye(d)
                    S.fresh[i] = 0
                rho = 1.0 / sy
                V = np.eye(d) - rho * np.outer(s, y)
                H = _d((V @ H @ V.T + rho * np.outer(s, s)).astype(dt))
                S.H[i] = H
            S.small[i] = S.small[i] + 1 if f - ft <= SMALL * abs(f) else 0
            S.x[i], S.f[i], S.g[i] = xt, ft, gt
            if np.sqrt(float(gt @ gt)) <= eps:
                S.status[i] = CONVERGED
            elif (xt == x).all() or S.small[i] >= 2:
                S.status[i] = STALLED
            else:
                p = _d((-(H @ gt)).astype(dt))
                if not float(gt @ p) < 0.0:
                    S.H[i] = np.eye(d)
                    S.fresh[i] = 1
                    p = -gt
                S.p[i] = p
                S.t[i] = 1.0
        else:
            denom = ft - f - gp * t
            tn = 0.5 * t
            if np.isfinite(denom) and denom > 0.0:
                tn = min(max(-gp * t * t / (2.0 * denom), 0.1 * t), 0.5 * t)
            S.t[i] = tn
            if float(S.t[i]) * np.abs(p).max() <= FLOOR * max(1.0, np.abs(x).max()):
                S.status[i] = STALLED
    active = (S.status == ACTIVE)[:, None]
    S.x_trial = np.where(active, (_d(S.x) + _d(S.t)[:, None] * _d(S.p)).astype(dt), S.x)
    return S


def solve(fun, x0, eps=1e-5, max_iter=300, state_dtype=np.float64):
    """The solve loop of ``pymde_amd.rows``: returns ``(state, sweeps, evaluations)``, evaluations in units of one
    evaluation of every row, only the active rows being evaluated in a sweep."""
    x0 = np.array(x0, dtype=state_dtype)
    n = x0.shape[0]
    every = np.arange(n)
    f, g = fun(x0, every)
    S = init(x0, f, g, eps, state_dtype)
    work, sweeps = n, 0
    f_t, g_t = np.zeros(n), np.zeros_like(_d(x0))
    while sweeps < max_iter and (S.status == ACTIVE).any():
        rows = np.nonzero(S.status == ACTIVE)[0]
        f_t[rows], g_t[rows] = fun(S.x_trial[rows], rows)
        step(S, f_t, g_t, eps)
        work += len(rows)
        sweeps += 1
    return S, sweeps, work / float(n)


def seed31_problem(d, n_old=300, n_new=150, nf=20):
    """The inputs of the issue's scipy comparison: float32 rows centred on the old ones, X_old their first d
    principal components, the start the mean of the d + 1 nearest old rows.  Returns ``(old, new, X_old, start, D)``
    with D [n_new, n_old] the float64 Euclidean distances of the float32 rows."""
    rng = np.random.default_rng(31)
    rows = rng.standard_normal((n_old + n_new, nf)) * rng.uniform(0.5, 2, nf)
    rows = (rows - rows[:n_old].mean(0)).astype(np.float32)
    old, new = rows[:n_old], rows[n_old:]
    _, _, vt = np.linalg.svd(old.astype(np.float64), full_matrices=False)
    X_old = (old.astype(np.float64) @ vt[:d].T).astype(np.float32)
    diff = new.astype(np.float64)[:, None, :] - old.astype(np.float64)[None, :, :]
    D = np.sqrt((diff * diff).sum(2))
    nearest = np.argsort(D, axis=1, kind="stable")[:, :d + 1]
    start = X_old.astype(np.float64)[nearest].mean(1).astype(np.float32)
    return old, new, X_old, start, D


def scipy_row_minima(fun, start, rows=None, gtol=1e-8):
    """scipy's BFGS on every row alone, in float64: ``(minimum [n], start value [n])``."""
    from scipy.optimize import minimize
    start = _d(start)
    n = start.shape[0]
    best, first = np.empty(n), np.empty(n)
    for i in range(n):
        one = np.array([i])

        def fg(z):
            f, g = fun(z[None, :], one)
            return float(f[0]), g[0]
        first[i] = fg(start[i])[0]
        best[i] = minimize(fg, start[i], jac=True, method="BFGS", options={"gtol": gtol, "maxiter": 2000}).fun
    return best, first

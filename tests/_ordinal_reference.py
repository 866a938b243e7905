"""float64 numpy reference of isotonic regression and ordinal MDS: pool-adjacent-violators by
the stack algorithm, the optimality conditions of a fit tested from the fit alone, tie groups and disparities under
the secondary treatment of ties, Kruskal's stress-1, and a replay of ``OrdinalMDE.embed`` with scipy's L-BFGS-B as
the inner solver.  Also the input patterns and recovery problems the host and the GPU tests share."""
import numpy as np


# ---------------------------------------------------------------- isotonic regression
def pava(y, w=None):
    """The nondecreasing minimiser of sum w (y - out)^2: a stack of blocks (weight, weighted sum, length)."""
    y = np.asarray(y, np.float64)
    w = np.ones_like(y) if w is None else np.asarray(w, np.float64)
    bw, bs, bn = [], [], []
    for yi, wi in zip(y, w):
        cw, cs, cn = wi, wi * yi, 1
        while bw and bs[-1] * cw >= cs * bw[-1]:         # mean of the block before >= mean of this one
            cw, cs, cn = cw + bw.pop(), cs + bs.pop(), cn + bn.pop()
        bw.append(cw), bs.append(cs), bn.append(cn)
    if not bw:
        return np.zeros(0)
    return np.repeat(np.asarray(bs) / np.asarray(bw), bn)


def isotonic(y, w=None):
    """``pava`` for the GPU tests: the Python loop up to 4096 values, beyond that scipy's float64 implementation of
    the same algorithm, which tests/test_ordinal_host.py pins to ``pava`` within 1e-12."""
    if len(y) <= 4096:
        return pava(y, w)
    from scipy.optimize import isotonic_regression
    return isotonic_regression(np.asarray(y, np.float64), weights=None if w is None else np.asarray(w, np.float64)).x


def kkt_violation(y, w, out):
    """How far ``out`` is from optimal, from ``out`` alone: over every maximal run of equal values of ``out``, the
    weighted mean of ``y`` must equal the value (the sum of w (y - out) over the run is 0) and every proper prefix
    of the run must have sum w (y - out) >= 0 (else splitting there would lower the objective).  Returns
    ``(violation, weight)``: the largest |run sum| or negative prefix sum, and the weight of the run it sits
    on; a decreasing step in ``out`` returns ``(inf, 0)``."""
    y = np.asarray(y, np.float64)
    out = np.asarray(out, np.float64)
    w = np.ones_like(y) if w is None else np.asarray(w, np.float64)
    if y.size == 0:
        return 0.0, 0.0
    if np.any(np.diff(out) < 0):
        return np.inf, 0.0
    starts = np.flatnonzero(np.concatenate([[True], out[1:] != out[:-1]]))
    r = w * (y - out)
    prefix = np.cumsum(r)
    before = np.concatenate([[0.0], prefix])[starts]          # the sum before each run
    run = np.searchsorted(starts, np.arange(y.size), side="right") - 1
    within = prefix - before[run]                             # the sum from the start of the run to i
    ends = np.concatenate([starts[1:], [y.size]]) - 1
    weight = np.add.reduceat(w, starts)
    viol = np.maximum(-within, 0.0)
    viol[ends] = np.abs(within[ends])
    worst = int(np.argmax(viol))
    return float(viol[worst]), float(weight[run[worst]])


def bound(y, w=None):
    """The accuracy bound of ``mde_isotonic``: 2^-23 max|y| + 2^-47 sum(w |y|) / min(w)."""
    y = np.asarray(y, np.float64)
    w = np.ones_like(y) if w is None else np.asarray(w, np.float64)
    return 2.0 ** -23 * np.abs(y).max() + 2.0 ** -47 * (w * np.abs(y)).sum() / w.min()


PATTERNS = ("normal", "increasing", "decreasing", "constant", "last_low", "first_high", "noisy_ramp", "integers",
            "alternating")


def pattern(name, p, seed=0):
    """float32 input of length ``p``."""
    rng = np.random.default_rng(seed)
    t = np.arange(p, dtype=np.float64)
    if name == "normal":
        y = rng.standard_normal(p)
    elif name == "increasing":
        y = t / max(p, 1) + 0.25
    elif name == "decreasing":
        y = 2.0 - t / max(p, 1)
    elif name == "constant":
        y = np.full(p, 0.7)
    elif name == "last_low":                 # the tangent from the last point reaches the far left
        y = t / max(p, 1)
        y[-1] = -1000.0
    elif name == "first_high":               # ... and from the first the far right
        y = t / max(p, 1)
        y[0] = 1000.0
    elif name == "noisy_ramp":               # noise three times the step
        y = t + 3.0 * rng.standard_normal(p)
    elif name == "integers":                 # many ties
        y = np.round(t / max(p, 1) * 10.0 + rng.standard_normal(p))
    elif name == "alternating":              # an alternating-sign ramp of growing amplitude
        y = (1.0 + t) * np.where(np.arange(p) % 2 == 0, 1.0, -1.0)
    else:
        raise ValueError(name)
    return y.astype(np.float32)


# ---------------------------------------------------------------- ordinal MDS
def tie_groups(deviations):
    """``(order, group, sizes)``: the stable sort of the deviations, the tie-group number of every rank and the
    groups' sizes."""
    deviations = np.asarray(deviations)
    order = np.argsort(deviations, kind="stable")
    ranked = deviations[order]
    first = np.concatenate([[True], ranked[1:] != ranked[:-1]])
    group = np.cumsum(first) - 1
    return order, group, np.bincount(group)


def disparities(deviations, distances):
    """The disparities (edge order) of ``distances`` under the order of ``deviations``, ties secondary: the
    isotonic regression of the tie groups' mean distances weighted by their sizes."""
    order, group, sizes = tie_groups(deviations)
    d = np.asarray(distances, np.float64)[order]
    means = np.bincount(group, weights=d) / sizes
    fit = pava(means, sizes.astype(np.float64))[group]
    out = np.empty_like(fit)
    out[order] = fit
    return out


def stress1(distances, dhat):
    d = np.asarray(distances, np.float64)
    return float(np.sqrt(((d - np.asarray(dhat, np.float64)) ** 2).sum() / (d ** 2).sum()))


def _distances(X, edges):
    diff = X[edges[:, 0]] - X[edges[:, 1]]
    return np.sqrt((diff ** 2).sum(1))


def _solve(edges, delta, n, d, X0, max_iter):
    """Minimise mean (|x_i - x_j| - delta)^2 over centred X with L-BFGS-B."""
    from scipy.optimize import minimize

    def fun(x):
        X = x.reshape(n, d)
        diff = X[edges[:, 0]] - X[edges[:, 1]]
        dist = np.sqrt((diff ** 2).sum(1))
        r = dist - delta
        g = np.zeros_like(X)
        c = (2.0 * r / np.maximum(dist, 1e-300))[:, None] * diff / len(delta)
        np.add.at(g, edges[:, 0], c)
        np.add.at(g, edges[:, 1], -c)
        return (r ** 2).mean(), g.ravel()
    res = minimize(fun, X0.ravel(), jac=True, method="L-BFGS-B",
                   options={"maxiter": max_iter, "maxcor": 10, "ftol": 0.0, "gtol": 1e-12})
    X = res.x.reshape(n, d)
    return X - X.mean(0)


def replay(edges, deviations, n, d, X0, rounds, inner_iter, metric_iter=300):
    """The alternation of ``OrdinalMDE.embed`` in float64: the metric solution on the deviations rescaled to rms 1
    from ``X0``, then ``rounds`` rounds of disparities (rescaled to rms 1) and ``inner_iter`` L-BFGS-B iterations.
    Returns ``(X, stress history, X of the metric start)``."""
    edges = np.asarray(edges)
    dev = np.asarray(deviations, np.float64)
    d0 = dev / np.sqrt((dev ** 2).mean())
    X = _solve(edges, d0, n, d, np.asarray(X0, np.float64), metric_iter)
    X_metric = X.copy()
    history = []
    for r in range(rounds + 1):
        dist = _distances(X, edges)
        dhat = disparities(dev, dist)
        history.append(stress1(dist, dhat))
        if r == rounds:
            break
        X = _solve(edges, dhat / np.sqrt((dhat ** 2).mean()), n, d, X, inner_iter)
    return X, history, X_metric


RECOVERY = ("cube", "exp", "sparse_cube")


def recovery_problem(name):
    """``(points, edges, true distances, deviations)`` of a recovery problem: 60 points uniform in [-1, 1]^2 with all
    pairs and deviations D^3 or exp(3 D), or 120 points keeping a fixed random 30 % of the pairs with D^3."""
    rng = np.random.default_rng(0)
    n = 120 if name == "sparse_cube" else 60
    P = rng.uniform(-1.0, 1.0, (n, 2))
    i, j = np.triu_indices(n, 1)
    edges = np.stack([i, j], 1)
    if name == "sparse_cube":
        keep = np.sort(rng.permutation(len(edges))[:int(0.3 * len(edges))])
        edges = edges[keep]
    D = _distances(P, edges)
    deviations = np.exp(3.0 * D) if name == "exp" else D ** 3
    return P, edges, D, deviations

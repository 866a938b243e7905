"""Float64 numpy replay of ``pymde_amd.affinity``: both row calibrations and both symmetrisation rules, reading
the same float32 lists as the kernels.  Written from the definitions, one row at a time;
shared by ``test_affinity_host.py`` (no GPU) and ``test_gpu_affinity.py``."""
import numpy as np

MAX_STEPS = 400
BRACKET = 2.0 ** -48


def kept_mask(idx, val, n, max_value=None):
    """[n, k] bool: the entries that count (an index in [0, n) other than the row, a value within the bound)."""
    idx = np.asarray(idx)
    rows = np.arange(idx.shape[0])[:, None]
    keep = (idx >= 0) & (idx < n) & (idx != rows)
    if max_value is not None:
        with np.errstate(invalid="ignore"):
            keep &= np.asarray(val, np.float32) <= np.float32(max_value)
    return keep


def distances(val, root=False, scale=1.0):
    """d = scale * (sqrt(v) if root else v), in double from the float32 values (negative v under root: 0)."""
    v = np.asarray(val, np.float32).astype(np.float64)
    return float(scale) * (np.sqrt(np.maximum(v, 0.0)) if root else v)


def entropy(beta, s):
    """(H, p) of p_j = exp(-beta s_j) / sum, H = -sum p log p over the entries with p > 0."""
    e = np.exp(-beta * s)
    p = e / e.sum()
    nz = p > 0
    return float(-(p[nz] * np.log(p[nz])).sum()), p


def _root(x0, above):
    """Doubling from x0 until the root is bracketed, then bisection to 2^-48 of the upper end."""
    lo, hi, x = 0.0, np.inf, float(x0)
    for _ in range(MAX_STEPS):
        if above(x):
            lo = x
            x = 2.0 * x if np.isinf(hi) else 0.5 * (lo + hi)
        else:
            hi = x
            x = 0.5 * (lo + hi)
        if np.isfinite(hi) and hi - lo <= BRACKET * hi:
            break
    return 0.5 * (lo + hi)


def perplexity_row(d, perplexity):
    """(p [k_i], beta, offset) of one row's kept distances ``d`` (float64)."""
    d = np.asarray(d, np.float64)
    k = len(d)
    if k == 0:
        return np.zeros(0), 0.0, 0.0
    q = d * d
    s = q - q.min()
    c = int((s == 0).sum())
    if perplexity >= k or c == k:
        return np.full(k, 1.0 / k), 0.0, float(d.min())
    if perplexity <= c:
        return np.where(s == 0, 1.0 / c, 0.0), np.inf, float(d.min())
    target = np.log(perplexity)
    beta = _root((k - c) / s.sum(), lambda b: entropy(b, s)[0] > target)
    return entropy(beta, s)[1], beta, float(d.min())


def umap_gaps(d):
    d = np.asarray(d, np.float64)
    positive = d[d > 0]
    rho = float(positive.min()) if len(positive) else 0.0
    return np.maximum(d - rho, 0.0), rho


def umap_row(d):
    """(p [k_i], sigma, rho, root) of one row's kept distances; ``root`` is the sigma that solves
    sum_j p_j = log2(k_i) before the floor applies (None where there is no finite positive root)."""
    d = np.asarray(d, np.float64)
    k = len(d)
    if k == 0:
        return np.zeros(0), 0.0, 0.0, None
    g, rho = umap_gaps(d)
    floor = 1e-3 * (d.sum() / k)
    c = int((g == 0).sum())
    target = np.log2(k)
    if c == k:
        return np.ones(k), floor, rho, None
    root = None
    if target > c:
        root = _root(g.sum() / (k - c), lambda sg: np.where(g == 0, 1.0, np.exp(-g / sg)).sum() < target)
    sigma = max(root if root is not None else 0.0, floor)
    if sigma == 0:
        return (g == 0).astype(np.float64), sigma, rho, root
    return np.where(g == 0, 1.0, np.exp(-g / sigma)), sigma, rho, root


def calibrate(idx, val, kind="perplexity", perplexity=None, root=False, scale=1.0, max_value=None):
    """``affinity.calibrate`` in float64: (idx_out int32 [n, k], p float64 [n, k], bandwidth float64 [n], offset
    float64 [n], solved bool [n]).  ``p`` is not rounded to float32; ``solved`` marks the rows whose bandwidth is
    the finite positive root of the row's equation (no limit case, and for umap no floor in its place)."""
    idx = np.asarray(idx, np.int32)
    n, k = idx.shape
    if perplexity is None:
        perplexity = k / 3.0
    keep = kept_mask(idx, val, n, max_value)
    d_all = distances(val, root, scale)
    idx_out = np.where(keep, idx, -1).astype(np.int32)
    p = np.zeros((n, k))
    bandwidth, offset, solved = np.zeros(n), np.zeros(n), np.zeros(n, bool)
    for i in range(n):
        d = d_all[i][keep[i]]
        if kind == "perplexity":
            p[i][keep[i]], bandwidth[i], offset[i] = perplexity_row(d, perplexity)
            solved[i] = 0 < bandwidth[i] < np.inf
        else:
            p[i][keep[i]], bandwidth[i], offset[i], root = umap_row(d)
            solved[i] = root is not None and root == bandwidth[i]
    return idx_out, p, bandwidth, offset, solved


def symmetrize(idx, p, rule="mean"):
    """``affinity.symmetrize`` on float32 conditionals: (edges int64 [m, 2] sorted by (i, j), weights float32)."""
    idx = np.asarray(idx)
    p = np.asarray(p, np.float32)
    n, k = idx.shape
    pair = {}
    for i in range(n):
        for c in range(k):
            j = int(idx[i, c])
            if j >= 0:
                pair[(i, j)] = p[i, c]
    edges = sorted({(min(i, j), max(i, j)) for i, j in pair})
    weights = np.empty(len(edges), np.float32)
    zero = np.float32(0)
    for e, (i, j) in enumerate(edges):
        a, b = pair.get((i, j), zero), pair.get((j, i), zero)
        if rule == "mean":
            weights[e] = np.float32(0.5) * (a + b)
        else:
            weights[e] = np.float32(float(a) + float(b) - float(a) * float(b))
    return np.asarray(edges, np.int64).reshape(-1, 2), weights

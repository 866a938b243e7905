"""A float64 numpy replay of the landmark selection of csrc/mde_landmarks.hip (no GPU): farthest-point and k-means++
selection with the kernel's marking rule (a selected row holds mind2 = -1 and is never offered again), its tie rules
(the largest mind2 goes to the smallest row; a row's nearest landmark is the earlier of equals) and its draws
``u_t = (splitmix64(seed ^ splitmix64(t)) >> 11) * 2^-53`` in Python integers.  On integer data every distance and
every sum is exact in float32 and float64 alike, so the kernel must give this sequence bit for bit."""
import numpy as np

MASK = (1 << 64) - 1
FARTHEST, KMEANSPP = "farthest", "kmeans++"


def splitmix64(x):
    x = (x + 0x9E3779B97F4A7C15) & MASK
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & MASK
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & MASK
    return x ^ (x >> 31)


def uniform01(seed, t):
    """Draw ``t`` of ``seed``: a float64 in [0, 1), exact (53 bits)."""
    return float(splitmix64((seed & MASK) ^ splitmix64(t)) >> 11) * 2.0 ** -53


def d2_to(X, row):
    """float64 squared distances of every row of ``X`` to row ``row``, in difference form."""
    diff = X - X[row]
    return np.einsum("ij,ij->i", diff, diff)


def update(X, mind2, nearest, row, position):
    """The pass of landmark ``position`` = row ``row``: lower mind2 / nearest (strictly: ties keep the earlier
    landmark; a marked row is never touched), then mark the landmark."""
    d2 = d2_to(X, row)
    lower = d2 < mind2
    mind2[lower] = d2[lower]
    nearest[lower] = position
    mind2[row] = -1.0


def choose(mind2, method, u=None):
    """The next landmark from the state ``mind2``: ``(row, target, prefix)`` -- target and prefix are ``None`` for
    the farthest point and when every remaining row duplicates a landmark."""
    if method == FARTHEST:
        return int(np.argmax(mind2)), None, None        # (the first of equal maxima; marked rows hold -1)
    prefix = np.cumsum(np.where(mind2 > 0.0, mind2, 0.0))   # float64, in row order
    total = prefix[-1]
    if not total > 0.0:
        return int(np.nonzero(mind2 >= 0.0)[0][0]), None, None
    target = u * total
    over = np.nonzero(prefix > target)[0]
    row = int(over[0]) if over.size else int(np.nonzero(mind2 > 0.0)[0][-1])
    return row, target, prefix


def select(data, m, method, start, seed=0):
    """``(indices int64 [m], radius2 float64 [m], nearest int64 [n], mind2 float64 [n])`` of the selection on the
    rows of ``data``, computed in float64: squared distances throughout, ``radius2[0] = inf``, ``mind2`` 0 at the
    landmarks."""
    X = np.asarray(data, dtype=np.float64)
    n = X.shape[0]
    assert 1 <= m <= n and 0 <= start < n
    mind2 = np.full(n, np.inf)
    nearest = np.zeros(n, dtype=np.int64)
    indices, radius2 = [int(start)], [np.inf]
    for t in range(1, m + 1):
        update(X, mind2, nearest, indices[t - 1], t - 1)
        if t == m:
            break
        row, _, _ = choose(mind2, method, uniform01(seed, t) if method == KMEANSPP else None)
        indices.append(row)
        radius2.append(mind2[row])
    mind2[indices] = 0.0
    return np.asarray(indices, dtype=np.int64), np.asarray(radius2), nearest, mind2


def replay(data, indices):
    """Follow somebody else's choices ``indices`` in float64: yields ``(t, mind2)`` for t = 1 .. m - 1, the state
    from which ``indices[t]`` was chosen (marked rows at -1), and finally ``(m, mind2, nearest)`` with the finished
    state (landmarks at 0)."""
    X = np.asarray(data, dtype=np.float64)
    n, m = X.shape[0], len(indices)
    mind2 = np.full(n, np.inf)
    nearest = np.zeros(n, dtype=np.int64)
    for t in range(1, m + 1):
        update(X, mind2, nearest, int(indices[t - 1]), t - 1)
        if t < m:
            yield t, mind2.copy()
    mind2[np.asarray(indices)] = 0.0
    yield m, mind2, nearest


def blobs_with_far_group(n, nf, seed=0):
    """float32 [n, nf]: six Gaussian blobs (centres ~ N(0, 16 I), unit noise), and rows 0..4 shifted by +25 in
    every coordinate: a small group far from the bulk, which a uniform draw of a few rows usually misses."""
    rng = np.random.default_rng(seed)
    centres = 4.0 * rng.standard_normal((6, nf))
    X = centres[rng.integers(0, 6, n)] + rng.standard_normal((n, nf))
    X[:5] += 25.0
    return X.astype(np.float32)


def covering_radius2(data, rows):
    """The largest squared distance (float64) from a row of ``data`` to its nearest row among ``rows``."""
    X = np.asarray(data, dtype=np.float64)
    best = np.full(X.shape[0], np.inf)
    for r in rows:
        best = np.minimum(best, d2_to(X, int(r)))
    return float(best.max())

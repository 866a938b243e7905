"""An integer replay of the edge sampler of csrc/mde_edges.hip and a restatement of its edge counter (no GPU).

The sampler's contract (csrc/mde_rng.h, csrc/mde_tri_index.h): draw ``t`` of a round's seed is
``r = splitmix64(seed ^ splitmix64(t))``; its pair index is ``idx = floor(r * C(n, 2) / 2^64)``; the pair ``(u, v)``,
``u < v``, is the ``idx``-th in the (i, j) order: ``u`` the largest row with ``off(u) = u n - u (u + 1) / 2 <= idx``
and ``v = idx - off(u) + u + 1``.  Round ``r`` of a call draws with the seed ``seed + ROUND_STRIDE * (r + 1)`` and asks
for ``need / keep * 1.02 + 1024`` draws, ``need`` the edges still missing and ``keep`` the share of pairs neither
excluded nor taken (at least 0.05); a round that would draw at least ``C(n, 2)`` times offers every pair once
instead.  Everything here is Python integers (``math.isqrt``), so it holds at every
``n < 2^31``, where the kernel's double-precision square root is only a first guess."""
import math

import numpy as np

MASK = (1 << 64) - 1
ROUND_STRIDE = 0x632BE59BD9B4E019
MAX_ROUNDS = 8


def splitmix64(x):
    x = (x + 0x9E3779B97F4A7C15) & MASK
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & MASK
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & MASK
    return x ^ (x >> 31)


def draw(seed, t):
    """The 64 bits of draw ``t`` of ``seed``."""
    return splitmix64((seed & MASK) ^ splitmix64(t))


def n_pairs(n):
    return n * (n - 1) // 2


def row_offset(n, u):
    """The index of the pair (u, u + 1): the number of pairs whose first item is smaller than ``u``."""
    return u * n - u * (u + 1) // 2


def pair_of_index(n, idx):
    """``(u, v)`` of the ``idx``-th pair in the (i, j) order of the ``C(n, 2)`` pairs, in integers."""
    assert n >= 2 and 0 <= idx < n_pairs(n)
    # off(u) <= idx  <=>  (2 n - 1 - 2 u)^2 >= (2 n - 1)^2 - 8 idx
    s = math.isqrt((2 * n - 1) ** 2 - 8 * idx)
    if s * s < (2 * n - 1) ** 2 - 8 * idx:
        s += 1                                   # the ceiling of the root
    u = (2 * n - 1 - s) // 2
    assert row_offset(n, u) <= idx < row_offset(n, u + 1)
    return u, idx - row_offset(n, u) + u + 1


def index_of_pair(n, u, v):
    """The inverse of ``pair_of_index``; integers or integer arrays with ``u < v``."""
    return u * n - u * (u + 1) // 2 + v - u - 1


def index_of_draw(n, seed, t):
    return (draw(seed, t) * n_pairs(n)) >> 64


def round_seed(seed, rnd):
    return ((seed & MASK) + ROUND_STRIDE * (rnd + 1)) & MASK


def round_draws(need, n, n_exclude=0, have=0):
    """How many draws a round makes that still needs ``need`` edges (the kernel's double arithmetic)."""
    keep = 1.0 - (float(n_exclude) + float(have)) / (float(n) * float(n - 1) / 2.0)
    return min(int(float(need) / (keep if keep > 0.05 else 0.05) * 1.02) + 1024, 1 << 30)


def replay_round(n, seed, rnd, draws):
    """The set of pairs ``(u, v)`` that round ``rnd`` of a call with ``seed`` offers: its ``draws`` draws, or every
    pair once when there are no more pairs than draws (the round enumerates them then)."""
    if n_pairs(n) <= draws:
        return {pair_of_index(n, idx) for idx in range(n_pairs(n))}
    rs = round_seed(seed, rnd)
    return {pair_of_index(n, index_of_draw(n, rs, t)) for t in range(draws)}


def replay(n, num_edges, seed):
    """The rounds of a call without exclusion: ``(pairs, rounds)``, the set of all pairs drawn until at least
    ``num_edges`` distinct ones are there, and the number of rounds that took.  What the sampler returns is a subset
    of ``pairs`` of size ``num_edges`` (all of it when the sizes agree)."""
    pairs = set()
    for rnd in range(MAX_ROUNDS):
        if len(pairs) >= num_edges:
            return pairs, rnd
        have = len(pairs)
        pairs |= replay_round(n, seed, rnd, round_draws(num_edges - have, n, 0, have))
    return pairs, MAX_ROUNDS


def count_unique(pairs):
    """``mde_edges_count_unique`` restated: rows with ``i == j`` or a negative entry are dropped, the others put in
    (min, max) order; returns ``(edges int64 [m, 2] sorted by (i, j), multiplicities float64 [m])``."""
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    keep = (pairs[:, 0] != pairs[:, 1]) & (pairs[:, 0] >= 0) & (pairs[:, 1] >= 0)
    ordered = np.sort(pairs[keep], axis=1)
    if len(ordered) == 0:
        return np.zeros((0, 2), dtype=np.int64), np.zeros(0)
    edges, counts = np.unique(ordered, axis=0, return_counts=True)
    return edges, counts.astype(np.float64)


def cell_chi2(n, edges, n_cells, excluded_indices=()):
    """Chi-square of sampled ``edges`` [m, 2] against the uniform law on the eligible pairs: pair indices are binned
    into ``n_cells`` equal cells of the (i, j) order, a cell's expected count is ``m`` times its exact share of the
    eligible (not excluded) indices.  A cell without eligible indices must stay empty and adds nothing."""
    edges = np.asarray(edges, dtype=np.int64)
    total = n_pairs(n)
    idx = index_of_pair(n, edges[:, 0], edges[:, 1])
    observed = np.bincount(idx * n_cells // total, minlength=n_cells).astype(np.float64)
    eligible = np.ones(total, dtype=bool)
    eligible[np.asarray(excluded_indices, dtype=np.int64)] = False
    assert eligible[idx].all(), "an excluded pair was sampled"
    share = np.bincount(np.arange(total) * n_cells // total, weights=eligible, minlength=n_cells)
    expected = share / share.sum() * len(edges)
    live = expected > 0
    assert (observed[~live] == 0).all()
    return float(((observed[live] - expected[live]) ** 2 / expected[live]).sum())

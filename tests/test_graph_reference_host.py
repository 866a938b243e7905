"""The float64 references of the graph tests (tests/_graph_reference.py) against brute force on tiny inputs: distance
rows against Floyd-Warshall, the pair sets and k-NN lists against loops, the hash replay against Python integers.
No GPU."""
import numpy as np
import pytest

import _edges_reference as eref
import _graph_reference as ref


def _random_graph(rng, n, p, weighted):
    e = np.unique(np.sort(rng.integers(0, n, (p, 2)), axis=1), axis=0)
    e = e[e[:, 0] != e[:, 1]]
    w = rng.integers(4, 25, len(e)) / 8.0 if weighted else None      # multiples of 1/8 in [0.5, 3]
    return e, w


def _floyd_warshall(n, e, w):
    D = np.full((n, n), np.inf)
    np.fill_diagonal(D, 0.0)
    for (a, b), x in zip(e.tolist(), np.ones(len(e)) if w is None else w):
        D[a, b] = D[b, a] = min(D[a, b], x)
    for m in range(n):
        D = np.minimum(D, D[:, m:m + 1] + D[m:m + 1, :])
    return D


@pytest.mark.parametrize("weighted", [False, True])
def test_distance_rows_against_floyd_warshall(weighted):
    rng = np.random.default_rng(3)
    n = 23
    e, w = _random_graph(rng, n - 3, 30, weighted)                   # nodes n - 3 .. n - 1 stay isolated
    want = _floyd_warshall(n, e, w)
    assert np.isinf(want).any() and np.isfinite(want[want > 0]).any()
    sources = [0, 5, 19, 20, 22]
    np.testing.assert_array_equal(ref.distance_rows(n, e, w, sources), want[sources])
    present = np.unique(want[sources][np.isfinite(want[sources]) & (want[sources] > 0)])
    cut = float(present[len(present) // 2])                          # a distance that occurs
    got = ref.distance_rows(n, e, w, sources, max_length=cut)
    np.testing.assert_array_equal(got, np.where(want[sources] <= cut, want[sources], np.inf))
    assert (got == cut).any()                                        # the bound is inclusive
    none = ref.distance_rows(4, np.zeros((0, 2), dtype=np.int64), None, [2])
    assert none.tolist() == [[np.inf, np.inf, 0.0, np.inf]]


def test_pairs_and_top_k_of_a_row():
    inf = np.inf
    row = np.array([2.0, inf, 0.0, 1.0, 2.0, inf, 1.0, 0.5])          # source 2
    j, d = ref.pairs_of_source(row, 2)
    assert j.tolist() == [3, 4, 6, 7] and d.tolist() == [1.0, 2.0, 1.0, 0.5]
    idx, dist = ref.top_k(row, 2, 4)
    assert idx.tolist() == [7, 3, 6, 0] and dist.tolist() == [0.5, 1.0, 1.0, 2.0]      # ties: the smaller index
    assert idx.dtype == np.int32 and dist.dtype == np.float32
    idx, dist = ref.top_k(row, 2, 7)
    assert idx.tolist() == [7, 3, 6, 0, 4, -1, -1] and dist[5] == dist[6] == ref.FLT_MAX
    idx, dist = ref.top_k(np.array([inf, 0.0, inf]), 1, 2)
    assert idx.tolist() == [-1, -1] and dist.tolist() == [ref.FLT_MAX] * 2
    assert float(ref.FLT_MAX) == 3.4028234663852886e38


def test_direct_lists_against_loops():
    rng = np.random.default_rng(1)
    n, k = 15, 3
    e, w = _random_graph(rng, n - 1, 40, True)
    idx, dist = ref.direct_lists(n, e, w, k)
    for u in range(n):
        nb = sorted([(w[i], int(b if a == u else a)) for i, (a, b) in enumerate(e.tolist()) if u in (a, b)])[:k]
        assert idx[u].tolist() == [j for _, j in nb] + [-1] * (k - len(nb))
        assert dist[u].tolist() == [np.float32(x) for x, _ in nb] + [ref.FLT_MAX] * (k - len(nb))
    assert idx[n - 1].tolist() == [-1] * k
    idx, dist = ref.direct_lists(3, [[0, 1], [1, 2]], None, 2)
    assert idx.tolist() == [[1, -1], [0, 2], [1, -1]] and dist[1].tolist() == [1.0, 1.0]


def test_hash_replay_against_python_integers():
    rng = np.random.default_rng(0)
    x = rng.integers(0, 2 ** 64, 200, dtype=np.uint64)
    x[:3] = [0, 2 ** 64 - 1, 2 ** 63]
    assert ref.gsplitmix64(x).tolist() == [eref.splitmix64(int(v)) for v in x]
    n, seed = 16500, 5
    i = rng.integers(0, n - 1, 500)
    j = i + 1 + rng.integers(0, n - 1 - i)
    for frac in (0.02, 0.3, 0.999):
        threshold = int(frac * 2.0 ** 64)
        want = [eref.splitmix64(seed ^ eref.splitmix64(int(a) * n + int(b))) < threshold for a, b in zip(i, j)]
        assert ref.retained(n, i, j, frac, seed).tolist() == want
    assert ref.retained(n, i, j, 1.0, seed).all() and not ref.retained(n, i, j, 0.0, seed).any()
    small, large = ref.retained(n, i, j, 0.1, seed), ref.retained(n, i, j, 0.3, seed)
    assert 20 < small.sum() < 90 and (large | ~small).all()           # nested in the fraction
    assert (ref.retained(n, i, j, 0.3, seed) != ref.retained(n, i, j, 0.3, seed + 1)).any()


def test_connected_pairs():
    assert ref.connected_pairs(7, np.array([[0, 1], [1, 2], [4, 5]])) == 3 + 1
    assert ref.connected_pairs(5, np.zeros((0, 2), dtype=np.int64)) == 0
    assert ref.connected_pairs(4, np.array([[0, 1], [1, 2], [2, 3], [0, 3]])) == 6

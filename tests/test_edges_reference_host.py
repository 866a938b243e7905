"""The integer replay of the edge sampler (tests/_edges_reference.py) against brute force on tiny inputs, and the
chi-square statistic the GPU tests use against samplers whose law is known.  No GPU."""
import itertools

import numpy as np
import pytest

import _edges_reference as ref

LARGE_N = [2 ** 26 + 3, 2 ** 30 + 7, 2 ** 31 - 1]


def test_draws():
    assert ref.splitmix64(0) == 0xE220A8397B1DCDAF       # the published first output of SplitMix64 from state 0
    assert ref.draw(0, 1) == ref.splitmix64(ref.splitmix64(1))
    assert ref.draw(2 ** 64 + 5, 3) == ref.draw(5, 3) and ref.draw(5, 3) != ref.draw(6, 3)
    assert ref.round_seed(2 ** 64 - 1, 0) == (ref.ROUND_STRIDE - 1) & ref.MASK
    # floor(r C / 2^64): the smallest and the largest draw land on the first and the last pair
    assert (0 * ref.n_pairs(10)) >> 64 == 0 and (ref.MASK * ref.n_pairs(10)) >> 64 == 44


@pytest.mark.parametrize("n", [2, 3, 4, 5, 9, 45, 60])
def test_pair_of_index_enumerates_the_pairs_in_order(n):
    pairs = list(itertools.combinations(range(n), 2))    # the (i, j) order
    assert len(pairs) == ref.n_pairs(n)
    for idx, (u, v) in enumerate(pairs):
        assert ref.pair_of_index(n, idx) == (u, v)
        assert ref.index_of_pair(n, u, v) == idx
    assert [ref.row_offset(n, u) for u in range(n)] == [sum(n - 1 - r for r in range(u)) for u in range(n)]


@pytest.mark.parametrize("n", LARGE_N)
def test_pair_of_index_at_row_boundaries_of_large_n(n):
    total = ref.n_pairs(n)
    assert ref.pair_of_index(n, 0) == (0, 1) and ref.pair_of_index(n, 1) == (0, 2)
    assert ref.pair_of_index(n, total - 1) == (n - 2, n - 1)
    assert ref.pair_of_index(n, total - 2) == (n - 3, n - 1)
    assert ref.pair_of_index(n, total - 3) == (n - 3, n - 2)
    for u in (1, 2, 1000, n // 3, n // 2, n - 70000, n - 3, n - 2):
        off = ref.row_offset(n, u)
        assert ref.pair_of_index(n, off - 1) == (u - 1, n - 1)
        assert ref.pair_of_index(n, off) == (u, u + 1)
        if u < n - 2:
            assert ref.pair_of_index(n, off + 1) == (u, u + 2)
        assert ref.index_of_pair(n, u, u + 1) == off


def test_round_draws():
    assert ref.round_draws(10, 2000) == 1034 and ref.round_draws(100, 2000) == 1126
    assert ref.round_draws(20000, 2 ** 31 - 1) == 21424
    assert ref.round_draws(10, 45, n_exclude=500) == int(10 / (490.0 / 990.0) * 1.02) + 1024
    assert ref.round_draws(5, 60, n_exclude=1000, have=765) == int(5 / 0.05 * 1.02) + 1024     # the floor of `keep`


def test_replay_covers_a_small_n_in_one_round_and_a_dense_request_in_several():
    pairs, rounds = ref.replay(3, 3, seed=4)
    assert pairs == {(0, 1), (0, 2), (1, 2)} and rounds == 1
    # C(60, 2) = 1770 pairs against 1.02 * 1770 + 1024 draws: the round enumerates the pairs
    pairs, rounds = ref.replay(60, ref.n_pairs(60), seed=4)
    assert pairs == set(itertools.combinations(range(60), 2)) and rounds == 1
    # 40 000 of C(300, 2) = 44 850 pairs: 41 824 draws repeat themselves too often for one round
    pairs, rounds = ref.replay(300, 40000, seed=4)
    first = ref.replay_round(300, 4, 0, ref.round_draws(40000, 300))
    assert 1 < rounds <= ref.MAX_ROUNDS and len(pairs) >= 40000
    assert first < pairs and 20000 < len(first) < 40000
    assert all(0 <= u < v < 300 for u, v in pairs)


def test_count_unique_against_a_dictionary():
    rng = np.random.default_rng(0)
    pairs = rng.integers(-1, 7, (300, 2))
    want = {}
    for i, j in pairs.tolist():
        if i != j and i >= 0 and j >= 0:
            key = (min(i, j), max(i, j))
            want[key] = want.get(key, 0) + 1
    edges, counts = ref.count_unique(pairs)
    assert [tuple(e) for e in edges.tolist()] == sorted(want)
    assert counts.tolist() == [float(want[k]) for k in sorted(want)]
    edges, counts = ref.count_unique([[1, 1], [-1, 3], [2, -1]])
    assert edges.shape == (0, 2) and counts.shape == (0,)
    edges, counts = ref.count_unique(np.zeros((0, 2), dtype=np.int64))
    assert edges.shape == (0, 2) and counts.shape == (0,)


def test_chi2_is_zero_on_the_exact_law_and_counts_only_eligible_pairs():
    n = 12
    allp = np.array(list(itertools.combinations(range(n), 2)))        # 66 pairs, 11 cells of 6
    assert ref.cell_chi2(n, allp, 11) == 0.0
    assert ref.cell_chi2(n, allp[12:], 11, excluded_indices=range(12)) == 0.0
    # cells of 6, 6, 3 (half excluded) ... : a sample with 2 per eligible pair
    twice = np.concatenate([allp[15:], allp[15:]])
    assert ref.cell_chi2(n, twice, 11, excluded_indices=range(15)) == 0.0
    with pytest.raises(AssertionError, match="excluded"):
        ref.cell_chi2(n, allp, 11, excluded_indices=[3])
    # everything in one cell of 11: chi2 = m (cells - 1)
    assert ref.cell_chi2(n, np.repeat(allp[:6], 11, axis=0), 11) == pytest.approx(66.0 * 10)


def _stride_thinned(rng, n, num_edges):
    """The rule the sampler used to thin a surplus with: drop the sorted keys at fixed ranks."""
    total = ref.n_pairs(n)
    keys = np.unique(rng.integers(0, total, ref.round_draws(num_edges, n)))
    drop = len(keys) - num_edges
    flags = np.ones(len(keys), dtype=bool)
    flags[((np.arange(drop) + 0.5) * len(keys) / drop).astype(np.int64)] = False
    return keys[flags][:num_edges]


def test_chi2_tells_a_uniform_sampler_from_stride_thinning():
    """The statistic and the bound of the GPU test (n = 2000, 10 edges per call, 1500 calls, 53 cells, 115.5 = the
    1e-6 tail of chi-square with 52 degrees of freedom): numpy's sampler without replacement passes, the stride
    rule misses by two orders of magnitude."""
    n, calls, per_call = 2000, 1500, 10
    total = ref.n_pairs(n)
    rng = np.random.default_rng(1)

    def edges_of(indices):
        return np.array([ref.pair_of_index(n, int(i)) for i in indices])

    uniform = np.concatenate([rng.choice(total, per_call, replace=False) for _ in range(calls)])
    assert ref.cell_chi2(n, edges_of(uniform), 53) < 115.5
    strided = np.concatenate([_stride_thinned(rng, n, per_call) for _ in range(calls)])
    assert ref.cell_chi2(n, edges_of(strided), 53) > 5000.0

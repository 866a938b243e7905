"""The matrix- and graph-level scores of pymde_amd.quality without a GPU: the brute-force reference of the kernels
(tests/_matrix_quality_reference.py) against cases worked by hand, the argument errors of every new function, which
are raised before any device is touched, and the sampled trustworthiness formula against ``_score_from_ranks``."""
import math

import numpy as np
import pytest
import torch

from pymde_amd import quality
from pymde_amd.graph import Graph

import _matrix_quality_reference as ref

INF = float("inf")


# ---------------------------------------------------------------- 1. the reference against hand-worked cases
def test_reference_moments_3x3():
    # items on a line at 0, 3, 7: E(0,1) = 3, E(0,2) = 7, E(1,2) = 4.  The pair (1, 2) is missing one way only.
    X = np.array([[0.0], [3.0], [7.0]], dtype=np.float32)
    Dm = np.array([[9.0, 1.0, 2.0],
                   [1.0, 9.0, INF],
                   [2.0, 5.0, 9.0]], dtype=np.float32)     # the diagonal is never used
    row_sums, row_count, row_max, totals = ref.moments(Dm, X)
    # row 0: D = 1, 2 with E = 3, 7;  row 1: D = 1 with E = 3;  row 2: D = 2, 5 with E = 7, 4
    np.testing.assert_array_equal(row_sums, [[3.0, 10.0, 5.0, 58.0, 17.0],
                                             [1.0, 3.0, 1.0, 9.0, 3.0],
                                             [7.0, 11.0, 29.0, 65.0, 34.0]])
    np.testing.assert_array_equal(row_count, [2, 1, 2])
    np.testing.assert_array_equal(row_max, [[2.0, 7.0], [1.0, 3.0], [5.0, 7.0]])
    np.testing.assert_array_equal(totals, [11.0, 24.0, 35.0, 132.0, 54.0, 5.0, 7.0, 5.0])


def test_reference_moments_4x2_with_items():
    # columns are the items 2 and 2 (a repeat); points at (0, 0), (3, 4), (0, 0), (6, 8)
    X = np.array([[0, 0], [3, 4], [0, 0], [6, 8]], dtype=np.float32)
    fmax = np.finfo(np.float32).max
    Dm = np.array([[1.0, 2.0],
                   [4.0, fmax],          # FLT_MAX: a missing pair
                   [0.5, 0.25],          # the item itself, in both columns
                   [INF, 8.0]], dtype=np.float32)
    row_sums, row_count, row_max, totals = ref.moments(Dm, X, items=[2, 2])
    # E to item 2 = (0, 0): 0, 5, -, 10
    np.testing.assert_array_equal(row_sums, [[3.0, 0.0, 5.0, 0.0, 0.0],
                                             [4.0, 5.0, 16.0, 25.0, 20.0],
                                             [0.0, 0.0, 0.0, 0.0, 0.0],
                                             [8.0, 10.0, 64.0, 100.0, 80.0]])
    np.testing.assert_array_equal(row_count, [2, 1, 0, 1])
    np.testing.assert_array_equal(row_max, [[2.0, 0.0], [4.0, 5.0], [0.0, 0.0], [8.0, 10.0]])
    np.testing.assert_array_equal(totals, [15.0, 15.0, 85.0, 125.0, 100.0, 8.0, 10.0, 4.0])
    np.testing.assert_array_equal(ref.counted(Dm, [2, 2]),
                                  [[True, True], [True, False], [False, False], [False, True]])


def test_reference_histogram_3x3():
    X = np.array([[0.0], [3.0], [7.0]], dtype=np.float32)
    Dm = np.array([[0.0, 1.0, 2.0], [1.0, 0.0, INF], [2.0, 4.0, 0.0]], dtype=np.float32)
    counts = ref.histogram(Dm, X, None, 2, (0.0, 4.0), (0.0, 8.0))
    # (D, E): (1, 3) (2, 7) | (1, 3) | (2, 7) (4, 4); D bins [0, 2) [2, 4], E bins [0, 4) [4, 8]
    np.testing.assert_array_equal(counts, [[2, 0], [0, 3]])
    # D = 4 falls outside a range that ends at 3; the closed last bin holds D = 3 only
    np.testing.assert_array_equal(ref.histogram(Dm, X, None, 2, (0.0, 3.0), (0.0, 8.0)), [[2, 0], [0, 2]])


def test_reference_ranks_3x3_and_4x2():
    Dm = np.array([[0.0, 1.0, 2.0], [1.0, 0.0, INF], [1.0, INF, 0.0]], dtype=np.float32)
    # column 0: items 1 and 2 tie at 1.0 -> 1 first.  column 1: 0 (1.0), then 2 (inf).  column 2: 0 (2.0), then 1 (inf)
    got = ref.ranks(Dm, [[1, 2, 0], [2, 0, 3], [-1, 1, 0]])
    np.testing.assert_array_equal(got, [[0, 1, -1], [1, 0, -1], [-1, 1, 0]])
    Dm = np.array([[3.0, INF], [1.0, INF], [7.0, 0.0], [1.0, 2.0]], dtype=np.float32)
    # column 0 is item 1: the others by (value, index): 3 (1.0), 0 (3.0), 2 (7.0)
    # column 1 is item 2: 3 (2.0), then the unreachable 0 and 1 by index
    got = ref.ranks(Dm, [[3, 0, 2, 1], [1, 0, 3, 2]], items=[1, 2])
    np.testing.assert_array_equal(got, [[0, 1, 2, -1], [2, 1, 0, -1]])


# ---------------------------------------------------------------- 2. argument errors, no device
def _cpu_graph(n):
    return Graph._from_unique_edges(torch.zeros((0, 2), dtype=torch.int64), torch.zeros(0), n)


MATRIX_CALLS = [
    lambda D, X, **kw: quality.matrix_moments(D, X, **kw),
    lambda D, X, **kw: quality.matrix_stress(D, X, **kw),
    lambda D, X, **kw: quality.matrix_correlation(D, X, **kw),
    lambda D, X, **kw: quality.matrix_shepard_histogram(D, X, **kw),
]
GRAPH_CALLS = [quality.graph_moments, quality.graph_stress, quality.graph_correlation,
               quality.graph_shepard_histogram, quality.graph_trustworthiness, quality.graph_continuity]


@pytest.mark.parametrize("call", MATRIX_CALLS)
def test_matrix_argument_errors(call):
    D, X = np.zeros((6, 6), dtype=np.float32), np.zeros((6, 2), dtype=np.float32)
    with pytest.raises(ValueError, match="graph_"):
        call(_cpu_graph(6), X)
    with pytest.raises(ValueError, match=r"matrix \[n, m\]"):
        call(np.zeros(6), X)
    with pytest.raises(ValueError, match="must agree"):
        call(D, X[:5])
    with pytest.raises(ValueError, match="1 to 8"):
        call(D, np.zeros((6, 9), dtype=np.float32))
    with pytest.raises(ValueError, match="square"):
        call(D[:, :4], X)
    with pytest.raises(ValueError, match="one entry per column"):
        call(D[:, :4], X, items=[0, 1, 2])
    with pytest.raises(ValueError, match=r"\[0, n\)"):
        call(D[:, :4], X, items=[0, 1, 2, 6])
    with pytest.raises(ValueError, match=r"\[0, n\)"):
        call(D[:, :4], X, items=torch.tensor([0, -1, 2, 3]))
    with pytest.raises(ValueError, match="integers"):
        call(D[:, :4], X, items=[0.0, 1.0, 2.0, 3.0])


def test_matrix_score_specific_errors():
    D, X = np.zeros((6, 6), dtype=np.float32), np.zeros((6, 2), dtype=np.float32)
    with pytest.raises(ValueError, match="scale"):
        quality.matrix_stress(D, X, scale="best")
    with pytest.raises(ValueError, match="bins"):
        quality.matrix_shepard_histogram(D, X, bins=65)
    with pytest.raises(ValueError, match="range"):
        quality.matrix_shepard_histogram(D, X, range=((0, 1), (2, 1)))
    # ranks: the list
    with pytest.raises(ValueError, match="rows for 6 columns"):
        quality.matrix_ranks(D, np.zeros((5, 3), dtype=np.int32))
    with pytest.raises(ValueError, match="1 to 64"):
        quality.matrix_ranks(D, np.zeros((6, 65), dtype=np.int32))
    with pytest.raises(ValueError, match="matrix"):
        quality.matrix_ranks(D, np.zeros(6, dtype=np.int32))
    with pytest.raises(ValueError, match="square"):
        quality.matrix_ranks(D[:, :4], np.zeros((4, 2), dtype=np.int32))
    # trustworthiness: rows, k
    with pytest.raises(ValueError, match="must agree"):
        quality.matrix_trustworthiness(D, X[:5])
    with pytest.raises(ValueError, match="n_neighbors"):
        quality.matrix_trustworthiness(D, X, n_neighbors=3)        # not < n / 2
    with pytest.raises(ValueError, match="n_neighbors"):
        quality.matrix_trustworthiness(D, X, n_neighbors=0)
    with pytest.raises(ValueError, match=r"\[0, n\)"):
        quality.matrix_trustworthiness(D[:, :2], X, n_neighbors=2, items=[0, 7])
    big = np.zeros((200, 1), dtype=np.float32)
    with pytest.raises(ValueError, match="longest neighbour list"):
        quality.matrix_trustworthiness(big, np.zeros((200, 2), dtype=np.float32), n_neighbors=65, items=[0])


@pytest.mark.parametrize("call", GRAPH_CALLS)
def test_graph_argument_errors(call):
    X = np.zeros((10, 2), dtype=np.float32)
    with pytest.raises(ValueError, match="Graph instance"):
        call(np.zeros((10, 10), dtype=np.float32), X)
    g = _cpu_graph(10)
    with pytest.raises(ValueError, match="must agree"):
        call(g, X[:9])
    with pytest.raises(ValueError, match="matrix"):
        call(g, np.zeros(10, dtype=np.float32))
    for bad in (0, 11, 2.5, True):
        with pytest.raises(ValueError, match="sample"):
            call(g, X, sample=bad)


@pytest.mark.parametrize("call", GRAPH_CALLS[:4])
def test_graph_global_scores_take_at_most_eight_columns(call):
    with pytest.raises(ValueError, match="1 to 8"):
        call(_cpu_graph(10), np.zeros((10, 9), dtype=np.float32))


@pytest.mark.parametrize("call", GRAPH_CALLS[4:])
def test_graph_rank_scores_check_k(call):
    g, X = _cpu_graph(10), np.zeros((10, 2), dtype=np.float32)
    for bad in (0, 5, 6):
        with pytest.raises(ValueError, match="n_neighbors"):
            call(g, X, n_neighbors=bad)
    with pytest.raises(ValueError, match="longest neighbour list"):
        call(_cpu_graph(200), np.zeros((200, 2), dtype=np.float32), n_neighbors=65)


def test_graph_score_specific_errors():
    g, X = _cpu_graph(10), np.zeros((10, 2), dtype=np.float32)
    with pytest.raises(ValueError, match="scale"):
        quality.graph_stress(g, X, scale=-1.0)
    with pytest.raises(ValueError, match="bins"):
        quality.graph_shepard_histogram(g, X, bins=0)
    with pytest.raises(ValueError, match="range"):
        quality.graph_shepard_histogram(g, X, range=((0, 1),))


def test_the_existing_scores_still_refuse_a_graph():
    with pytest.raises(ValueError, match="Graph"):
        quality.stress(_cpu_graph(10), np.zeros((10, 2), dtype=np.float32))


# ---------------------------------------------------------------- 3. formulas
def test_batch_columns():
    assert quality._batch_columns(47) == (2 ** 29 // 47) // 64 * 64
    assert quality._batch_columns(1_000_000) == 512                  # 536 rounded down to a multiple of 64
    assert quality._batch_columns(2 ** 24) == 64                     # the floor of 64 columns
    assert quality._batch_columns(10 ** 9) == 64
    assert quality._batch_columns(47, 64) == 64
    for n in (47, 20_000, 1_000_000, 2 ** 23):
        assert 4 * n * quality._batch_columns(n) <= 2 ** 31         # 2 GiB


@pytest.mark.parametrize("n, k", [(11, 1), (40, 5), (200, 64), (131, 15)])
def test_sampled_score_with_every_item_is_score_from_ranks(n, k):
    rng = np.random.default_rng(n + k)
    ranks = torch.tensor(rng.integers(-1, n - 1, (n, k)), dtype=torch.int32)
    want, want_rows = quality._score_from_ranks(ranks, n, k, per_item=True)
    got, got_rows = quality._sampled_score(ranks, n, k, per_item=True)
    assert got == want and quality._sampled_score(ranks, n, k) == want
    assert torch.equal(got_rows, want_rows)
    assert abs(got - ref.sampled_score(ranks.numpy(), n, k)) <= 1e-14


def test_sampled_score_is_the_mean_over_the_listed_items():
    n, k, m = 50, 4, 7
    rng = np.random.default_rng(3)
    ranks = torch.tensor(rng.integers(0, n - 1, (m, k)), dtype=torch.int32)
    got, rows = quality._sampled_score(ranks, n, k, per_item=True)
    penalty = np.maximum(ranks.numpy().astype(np.int64) + 1 - k, 0).sum()
    assert abs(got - (1.0 - 2.0 * penalty / (m * k * (2 * n - 3 * k - 1)))) <= 1e-15
    assert rows.shape == (m,) and abs(float(rows.double().mean()) - got) <= 1e-6
    assert math.isclose(quality._sampled_score(torch.zeros((m, k), dtype=torch.int32), n, k), 1.0)


def test_matrix_moments_is_a_pair_moments_with_two_more_fields():
    assert quality.MatrixMoments._fields[:len(quality.PairMoments._fields)] == quality.PairMoments._fields
    assert quality.MatrixMoments._fields[-2:] == ("row_counts", "missing")
    mom = quality._moments_from_parts(12, torch.zeros((4, 5), dtype=torch.float64), torch.zeros(4, dtype=torch.int64),
                                      [6.0, 3.0, 14.0, 5.0, 8.0, 3.0, 2.0, 9.0])
    assert (mom.count, mom.missing, mom.max_d, mom.max_e) == (9, 3, 3.0, 2.0)
    s = quality._scores_from_moments(mom)                            # serves it unchanged
    assert abs(s.alpha - 8.0 / 5.0) <= 1e-15 and abs(s.stress - math.sqrt(1.0 - 64.0 / 70.0)) <= 1e-15

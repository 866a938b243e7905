"""The host references of tests/_components_reference.py against independent computations (no GPU): the table of
nearest pairs against brute force, the "tree" bridges against scipy's minimum spanning tree of the table, the replay
of the hook-and-jump rounds against scipy's labels, and the number of rounds it takes on a long path."""
import math

import numpy as np
import pytest
from scipy.sparse.csgraph import minimum_spanning_tree

import _components_reference as ref


def test_nearest_pair_table_equals_brute_force():
    rng = np.random.default_rng(3)
    X = rng.integers(-6, 7, size=(200, 3)).astype(np.float64)      # a coarse grid: many ties in distance
    labels = rng.integers(0, 7, size=200)
    labels[labels == 4] = 5                                        # group 4 is empty
    d2, row = ref.nearest_pairs(X, labels, 7)
    want_d2, want_row = ref.brute_force_pairs(X, labels, 7)
    assert np.array_equal(d2, want_d2) and np.array_equal(row, want_row)
    assert np.isinf(d2[4]).all() and (row[4] == -1).all() and (row[:, 4] == -1).all()
    assert np.array_equal(d2, d2.T)
    ties = sum(int((((X[labels == A][:, None] - X[labels == B][None]) ** 2).sum(-1) == d2[A, B]).sum() > 1)
               for A in range(7) for B in range(A + 1, 7) if np.isfinite(d2[A, B]))
    assert ties > 0                                                # the key decided something


@pytest.mark.parametrize("layout", range(len(ref.BLOB_LAYOUTS)))
def test_tree_bridges_are_the_minimum_spanning_tree_of_the_table(layout):
    n_blobs, per, k, separation = ref.BLOB_LAYOUTS[layout]
    X = ref.blobs(n_blobs, per, separation, seed=layout)
    edges, _ = ref.knn_edges(X, k)
    count, labels = ref.components(len(X), edges)
    assert count > 1
    d2, row = ref.nearest_pairs(X, labels, count)
    be, bd2 = ref.bridges(d2, row, "tree")
    assert len(be) == count - 1 and (be[:, 0] < be[:, 1]).all()
    T = minimum_spanning_tree(np.where(np.isinf(d2), 0.0, np.triu(d2, 1))).toarray()
    assert np.array_equal(np.sort(T[T > 0]), np.sort(bd2))
    # the bridges join the components, and the "pairs" rule holds them all
    assert ref.components(len(X), np.concatenate([edges, be]))[0] == 1
    pe, _ = ref.bridges(d2, row, "pairs")
    assert len(pe) == count * (count - 1) // 2
    assert set(map(tuple, be)) <= set(map(tuple, pe))
    # every bridge is the nearest pair of its two components
    for (i, j), d in zip(be, bd2):
        A, B = sorted((labels[i], labels[j]))
        assert A != B and d == d2[A, B] and {row[A, B], row[B, A]} == {i, j}


@pytest.mark.parametrize("n,degree", [(1, 0), (2, 0), (2, 1), (65, 0.5), (257, 1), (257, 3), (1000, 1)])
def test_round_replay_gives_scipys_labels(n, degree):
    edges = ref.random_edges(n, degree, seed=n) if n > 2 else np.array([[0, 1]] * int(degree)).reshape(-1, 2)
    count, labels = ref.components(n, edges)
    got, rounds = ref.hook_and_jump(n, edges)
    assert np.array_equal(got, labels) and got.max() + 1 == count
    assert rounds <= 8 * max(1, math.ceil(math.log2(max(n, 2))))


def test_round_replay_on_a_star_and_a_long_path():
    n, edges = ref.star_with_isolated()
    got, rounds = ref.hook_and_jump(n, edges)
    assert np.array_equal(got, ref.components(n, edges)[1]) and rounds <= 3
    n = 20000
    edges = ref.renumbered_path(n, seed=0)
    got, rounds = ref.hook_and_jump(n, edges)
    print("rounds on the renumbered path of %d nodes: %d" % (n, rounds))
    assert (got == 0).all()
    assert rounds <= 8 * math.ceil(math.log2(n))                   # = 120; label propagation needs thousands
    # the numbering that is worst for label propagation: the path in order
    ordered = np.stack([np.arange(n - 1), np.arange(1, n)], axis=1)
    got, rounds = ref.hook_and_jump(n, ordered)
    assert (got == 0).all() and rounds <= 8 * math.ceil(math.log2(n))


def test_isomap_replay_separates_the_two_rules():
    X, true = ref.three_clusters()
    pairs, count = ref.isomap_centroid_ratios(X, 6, "pairs", 60, true)
    tree, _ = ref.isomap_centroid_ratios(X, 6, "tree", 60, true)
    print("pairs", pairs, "tree", tree)
    assert count == 3
    assert (pairs < 1.2).all() and (pairs > 0.9).all()
    assert tree.max() > 1.3                                        # the long side runs through the third cluster

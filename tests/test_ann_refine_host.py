"""The neighbour-of-neighbour pass without a device: the numpy restatement (tests/_ann_refine_reference.py) has
the properties the kernel is held to -- exact lists are a fixed point, entries only move earlier, lists stay
valid, recall rises --, ``ann.reverse_lists`` agrees with it, and the argument checks of ``n_refine``."""
import numpy as np
import pytest
import torch

import _ann_refine_reference as ref

N, NF, K, BLOCKS = 2000, 16, 15, 12


def _mixture(n, nf, classes=10, seed=0):
    rng = np.random.default_rng(seed)
    labels = rng.integers(0, classes, n)
    X = 3.0 * rng.standard_normal((classes, nf))[labels] + 0.5 * rng.standard_normal((n, nf))
    for c in range(classes):
        rows = np.nonzero(labels == c)[0]
        dim = min(nf, 4 + c % 3)
        X[rows] += rng.standard_normal((rows.size, dim)) @ rng.standard_normal((dim, nf))
    return X


def _lists_within(D, groups, k, n_groups=1, probe=1):
    """Each row's k nearest rows under (d2, index), from the full float64 matrix D, among the rows of its own
    group and of the ``probe - 1`` groups after it (cyclically)."""
    n = D.shape[0]
    idx = np.full((n, k), -1, dtype=np.int32)
    d2 = np.full((n, k), np.float64(ref.FLT_MAX))
    for g in range(n_groups):
        seen = np.nonzero(np.isin(groups, (g + np.arange(probe)) % n_groups))[0]
        for i in np.nonzero(groups == g)[0]:
            others = seen[seen != i]
            idx[i], d2[i] = ref.top_k(others, D[i, others], k, np.float64)
    return idx, d2


@pytest.fixture(scope="module")
def world():
    X = _mixture(N, NF)
    sq = (X * X).sum(1)
    D = np.maximum(sq[:, None] + sq[None, :] - 2.0 * X @ X.T, 0.0)
    exact = _lists_within(D, np.zeros(N, dtype=int), K)
    groups = np.random.default_rng(1).integers(0, BLOCKS, N)
    # Lists searched inside a row's own block alone are closed under the pass (a neighbour's neighbours and the
    # rows that list it are all of that block: a fixed point, whatever its recall), so each row also searches
    # the block after its own -- one-sided, as the probing of an inverted file is.
    degraded = _lists_within(D, groups, K, BLOCKS, 2)
    passes = [degraded]
    for _ in range(2):
        i, d, _ = ref.refine_pass(passes[-1][0], passes[-1][1], lambda r, c: D[r, c])
        passes.append((i, d))
    return D, exact, passes


def _recall(idx, truth):
    return float((truth[:, :, None] == idx[:, None, :]).any(2).mean())


def test_exact_lists_are_a_fixed_point(world):
    D, (idx, d2), _ = world
    new_i, new_d, changed = ref.refine_pass(idx, d2, lambda r, c: D[r, c])
    assert changed == 0
    np.testing.assert_array_equal(new_i, idx)
    np.testing.assert_array_equal(new_d, d2)


def test_a_pass_never_moves_an_entry_later(world):
    _, _, passes = world
    for (i0, d0), (i1, d1) in zip(passes[:-1], passes[1:]):
        later = (d1 > d0) | ((d1 == d0) & (np.where(i1 < 0, 2 ** 31, i1) > np.where(i0 < 0, 2 ** 31, i0)))
        assert not later.any()
    assert (passes[1][0] != passes[0][0]).any()


def test_lists_stay_valid(world):
    D, _, passes = world
    for idx, d2 in passes:
        valid = idx >= 0
        assert (valid[:, 1:] <= valid[:, :-1]).all()                 # -1 slots trail
        assert not (idx == np.arange(N)[:, None]).any()              # no self entry
        for i in range(N):
            row = idx[i][valid[i]]
            assert np.unique(row).size == row.size                   # no row twice
            np.testing.assert_array_equal(d2[i][valid[i]], D[i, row])
            assert (np.lexsort((row, d2[i][valid[i]])) == np.arange(row.size)).all()


def test_recall_rises_over_two_passes(world):
    _, (truth, _), passes = world
    r = [_recall(idx, truth) for idx, _ in passes]
    print("recall of the block lists, after one pass, after two:", r)
    assert r[0] < r[1] < r[2]


def test_reverse_lists_against_the_reference():
    from pymde_amd import ann
    rng = np.random.default_rng(2)
    n, k = 40, 3
    idx = np.empty((n, k), dtype=np.int32)
    for i in range(n):
        pool = np.setdiff1d(np.arange(1, n - 1), [i])                # row n - 1 is listed by nobody
        idx[i] = np.concatenate([[0] if i else [], rng.choice(pool, k - (1 if i else 0), replace=False)])
    d2 = rng.integers(0, 4, (n, k)).astype(np.float32)               # many equal distances: the source decides
    idx[5, 2] = -1
    idx[7] = -1
    for cap in (None, 2, 5):
        want = ref.reverse_lists(idx, d2, cap)
        got = ann.reverse_lists(torch.from_numpy(idx), torch.from_numpy(d2), cap)
        assert got.dtype == torch.int32
        np.testing.assert_array_equal(got.numpy(), want)
    want = ref.reverse_lists(idx, d2)
    assert (want[n - 1] == -1).all()                                 # the row nobody lists
    assert (want[0] >= 0).all() and (idx == 0).sum() > k             # the row more than k rows list


def test_n_refine_argument_checks_need_no_device():
    from pymde_amd import ann, preprocess
    X = np.zeros((20, 3), dtype=np.float32)
    assert ann.check_n_refine(0) == 0 and ann.check_n_refine(3) == 3
    for bad in (True, False, 1.0, 1.5, "1", None, -1):
        with pytest.raises(ValueError, match="n_refine"):
            ann.check_n_refine(bad)
        with pytest.raises(ValueError, match="n_refine"):
            preprocess.k_nearest_neighbors(X, 3, approximate=True, n_refine=bad)
    with pytest.raises(ValueError, match="n_refine"):
        preprocess.k_nearest_neighbors(X, 3, n_refine=1)             # the exact search has nothing to refine


def test_recipe_options():
    from pymde_amd import recipes
    assert recipes._approximate_options({"n_refine": 1}) == {"n_refine": 1, "approximate": True}
    assert recipes._approximate_options({"n_lists": 7, "n_probe": 2, "n_refine": 2}) == {
        "n_lists": 7, "n_probe": 2, "n_refine": 2, "approximate": True}
    assert recipes._approximate_options(False) == {} and recipes._approximate_options(None) == {}
    assert recipes._approximate_options(True) == {"approximate": True}
    assert recipes._approximate_options({"n_probe": 4}) == {"n_probe": 4, "approximate": True}
    with pytest.raises(ValueError, match="'n_lists', 'n_probe' and 'n_refine'"):
        recipes._approximate_options({"n_refined": 1})

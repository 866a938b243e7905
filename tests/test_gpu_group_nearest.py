"""``preprocess.nearest_between_groups`` / ``mde_group_nearest`` (csrc/mde_group_nearest.hip)
against the float64 table of tests/_components_reference.py.  The data are integers with ``|x| <= 64``: every product
and sum of the squared distance is exact in float32, so the table compares with ``==`` and the float64 reference
decides ties by the same key (d2, a, b)."""
import numpy as np
import pytest
import torch
from scipy.spatial.distance import cdist, cosine

from pymde_amd import preprocess

import _components_reference as ref

pytestmark = pytest.mark.gpu

FLT_MAX = float(np.finfo(np.float32).max)
SIZES = [2, 63, 64, 65, 130, 257]
FEATURES = [1, 31, 32, 33, 70]


def integer_rows(n, nf, seed):
    return np.random.default_rng(seed).integers(-64, 65, size=(n, nf)).astype(np.float32)


def label_patterns(n, seed):
    """name -> labels in [0, groups), every group non-empty unless the name says otherwise."""
    rng = np.random.default_rng(seed)
    out = {"interleaved": np.arange(n) % 2}
    if n > 64:
        out["blocks_of_64"] = np.arange(n) // 64                    # whole tiles of one label: skipped tiles
    single = np.arange(n) % 2
    single[-1] = 2 if n > 2 else 1
    out["singleton"] = single                                       # the last row is a group of its own
    if n >= 63:
        sizes = rng.multinomial(n - 17, np.arange(1, 18) / np.arange(1, 18).sum()) + 1
        out["seventeen"] = rng.permutation(np.repeat(np.arange(17), sizes))
        gap = out["seventeen"].copy()
        gap[gap == 5] = 6
        out["seventeen_one_empty"] = gap                            # group 5 has no rows
    return out


def table(X, labels, groups, slices=0):
    d2, row = preprocess._group_nearest_table(torch.as_tensor(X, device="cuda"), torch.as_tensor(labels), groups, slices)
    return d2.cpu().numpy(), row.cpu().numpy()


def expected(X, labels, groups):
    d2, row = ref.nearest_pairs(X, labels, groups)
    return np.where(np.isinf(d2), FLT_MAX, d2).astype(np.float32), row.astype(np.int32)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("nf", FEATURES)
def test_table_equals_the_float64_reference(n, nf):
    X = integer_rows(n, nf, seed=100 * n + nf)
    for name, labels in label_patterns(n, seed=n).items():
        groups = 17 if name.startswith("seventeen") else int(labels.max()) + 1
        want_d2, want_row = expected(X, labels, groups)
        got_d2, got_row = table(X, labels, groups)
        assert got_d2.dtype == np.float32 and got_row.dtype == np.int32
        assert np.array_equal(got_d2, want_d2), (name, n, nf)
        assert np.array_equal(got_row, want_row), (name, n, nf)
        # the symmetry the header states, the diagonal, and that a row lies in the group it is listed for
        assert np.array_equal(got_d2, got_d2.T)
        assert (np.diag(got_d2) == FLT_MAX).all() and (np.diag(got_row) == -1).all()
        A, B = np.nonzero(got_row >= 0)
        assert np.array_equal(labels[got_row[A, B]], A)
        if name == "seventeen_one_empty":
            assert (got_d2[5] == FLT_MAX).all() and (got_row[5] == -1).all() and (got_row[:, 5] == -1).all()
        for slices in (1, 2, 5):
            d2_s, row_s = table(X, labels, groups, slices)
            assert np.array_equal(d2_s.view(np.int32), got_d2.view(np.int32)), (name, slices)
            assert np.array_equal(row_s, got_row), (name, slices)
        again_d2, again_row = table(X, labels, groups)
        assert np.array_equal(again_d2.view(np.int32), got_d2.view(np.int32)) and np.array_equal(again_row, got_row)


def test_1024_groups():
    n, groups = 2048, 1024
    X = integer_rows(n, 7, seed=9)
    labels = np.random.default_rng(9).permutation(np.arange(n) % groups)
    want_d2, want_row = expected(X, labels, groups)
    got_d2, got_row = table(X, labels, groups)
    assert np.array_equal(got_d2, want_d2) and np.array_equal(got_row, want_row)
    d2_s, row_s = table(X, labels, groups, slices=5)
    assert np.array_equal(d2_s, got_d2) and np.array_equal(row_s, got_row)


def test_duplicate_rows_in_different_groups_tie_to_the_smaller_rows():
    n = 130
    X = integer_rows(n, 33, seed=4)
    labels = np.arange(n) % 3
    # rows 100 (group 1) and 7, 40 (group 0) and 128 (group 2) are one point: distance 0 three times over
    X[100] = X[40] = X[128] = X[7]
    assert labels[7] == 1 and labels[40] == 1      # (7 % 3 == 1, 40 % 3 == 1)
    labels[7], labels[40] = 0, 0
    labels[100], labels[128] = 1, 2
    got_d2, got_row = table(X, labels, 3)
    want_d2, want_row = expected(X, labels, 3)
    assert np.array_equal(got_d2, want_d2) and np.array_equal(got_row, want_row)
    assert got_d2[0, 1] == 0 and (got_row[0, 1], got_row[1, 0]) == (7, 100)
    assert got_d2[0, 2] == 0 and (got_row[0, 2], got_row[2, 0]) == (7, 128)
    assert got_d2[1, 2] == 0 and (got_row[1, 2], got_row[2, 1]) == (100, 128)


def test_public_result_any_integer_labels_and_units():
    n = 257
    X = integer_rows(n, 31, seed=2)
    compact = label_patterns(n, seed=n)["seventeen"]
    names = np.sort(np.random.default_rng(1).choice(np.arange(-500, 500), size=17, replace=False))
    got = preprocess.nearest_between_groups(X, names[compact])
    assert isinstance(got, preprocess.GroupNearest)
    assert np.array_equal(got.groups.cpu().numpy(), names)
    want_d2, want_row = expected(X, compact, 17)
    assert got.row.dtype == torch.int64 and np.array_equal(got.row.cpu().numpy(), want_row)
    dist = got.distance.cpu().numpy()
    assert dist.dtype == np.float32 and np.isinf(np.diag(dist)).all()
    off = ~np.eye(17, dtype=bool)
    assert np.array_equal(dist[off], np.sqrt(want_d2[off]))        # (float32 sqrt is correctly rounded on both sides)
    # the same through torch labels on the GPU and a torch matrix
    again = preprocess.nearest_between_groups(torch.as_tensor(X, device="cuda"),
                                              torch.as_tensor(names[compact], device="cuda"), slices=2)
    assert torch.equal(again.distance, got.distance) and torch.equal(again.row, got.row)


def test_float_data_has_the_bits_of_the_cross_search():
    n, nf, groups = 257, 70, 5
    X = np.random.default_rng(6).standard_normal((n, nf)).astype(np.float32)
    labels = np.arange(n) % groups
    got = preprocess.nearest_between_groups(X, labels)
    members = [np.flatnonzero(labels == g) for g in range(groups)]
    for A in range(groups):
        for B in range(A + 1, groups):
            idx, dist = preprocess.cross_nearest_neighbors(X[members[A]], X[members[B]], k=len(members[B]))
            idx, dist = idx.cpu().numpy(), dist.cpu().numpy()
            a, b = int(got.row[A, B]), int(got.row[B, A])
            qa, cb = int(np.searchsorted(members[A], a)), int(np.searchsorted(members[B], b))
            assert members[A][qa] == a and members[B][cb] == b
            at = np.flatnonzero(idx[qa] == cb)
            assert len(at) == 1
            value = np.float32(got.distance[A, B].item())
            assert value.view(np.int32) == dist[qa, at[0]].view(np.int32)
            assert value == dist.min()                              # and no pair of the two groups is nearer


def test_cosine():
    n, nf, groups = 130, 33, 3
    X = np.random.default_rng(8).standard_normal((n, nf)).astype(np.float32)
    labels = np.random.default_rng(8).integers(0, groups, size=n)
    got = preprocess.nearest_between_groups(X, labels, metric="cosine")
    X64 = X.astype(np.float64)
    for A in range(groups):
        for B in range(A + 1, groups):
            ia, ib = np.flatnonzero(labels == A), np.flatnonzero(labels == B)
            S = cdist(X64[ia], X64[ib], "cosine")
            i, j = np.unravel_index(np.argmin(S), S.shape)
            a, b = int(got.row[A, B]), int(got.row[B, A])
            assert (a, b) == (ia[i], ib[j])
            assert abs(float(got.distance[A, B]) - cosine(X64[a], X64[b])) <= 1e-6
            assert float(got.distance[A, B]) == float(got.distance[B, A])


def test_errors():
    X = integer_rows(70, 4, seed=0)
    labels = np.arange(70) % 3
    with pytest.raises(ValueError, match="Manhattan"):
        preprocess.nearest_between_groups(X, labels, metric="manhattan")
    with pytest.raises(ValueError, match="two groups"):
        preprocess.nearest_between_groups(X, np.zeros(70, dtype=np.int64))
    with pytest.raises(ValueError, match="1025"):
        preprocess.nearest_between_groups(integer_rows(1025, 2, seed=1), np.arange(1025))
    with pytest.raises(ValueError, match="one label per row"):
        preprocess.nearest_between_groups(X, labels[:-1])
    with pytest.raises(ValueError, match="integers"):
        preprocess.nearest_between_groups(X, labels.astype(np.float32))
    rows = torch.as_tensor(X, device="cuda")
    bad = labels.copy()
    bad[11] = -1
    with pytest.raises(ValueError, match=r"\[0, groups\)"):
        preprocess._group_nearest_table(rows, torch.as_tensor(bad), 3)
    bad[11] = 3
    with pytest.raises(ValueError, match=r"\[0, groups\)"):
        preprocess._group_nearest_table(rows, torch.as_tensor(bad), 3)
    with pytest.raises(ValueError, match="one label per row"):
        preprocess._group_nearest_table(rows, torch.as_tensor(labels[:-1]), 3)

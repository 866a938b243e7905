"""mde_matrix_moments, mde_matrix_histogram, mde_matrix_ranks and the matrix_* scores of pymde_amd.quality on the GPU,
against the float64 brute force of tests/_matrix_quality_reference.py.

Bounds.  Counts, the largest D and the ranks are exact.  The sums of D and D^2 are float64 sums of exact terms: 1e-12
relative.  A float32 E from d squared differences and one square root carries at most about (d / 2 + 2) ulps, every
term of a sum is non-negative, and the products double that: the sums that involve E are within (d + 4) 2^-23
relative.  The histogram and rank cases use an integer grid for X and multiples of 2^-6 for D, so E, every bin and
every comparison are exact and the results are ``array_equal`` to the reference."""
import functools

import numpy as np
import pytest
import torch

from pymde_amd import _lib, quality

import _matrix_quality_reference as ref

pytestmark = pytest.mark.gpu

DEV = "cuda"
INF = np.float32(np.inf)
SIZES_N = [1, 2, 63, 64, 65, 257, 1000]
SIZES_M = [1, 63, 64, 65, 130]
DIMS = [1, 2, 3, 8]


def _dev(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(DEV)


def _matrix(rng, n, m):
    """Positive float32 entries with scattered inf, one all-inf row and one all-inf column (when there is room)."""
    Dm = rng.uniform(0.1, 9.0, (n, m)).astype(np.float32)
    Dm[rng.random((n, m)) < 0.1] = INF
    if n >= 2:
        Dm[n // 2, :] = INF
    if m >= 2:
        Dm[:, m // 3] = INF
    return Dm


def _items(rng, n, m):
    """Item indices in any order, with a repeat; every row meets its own item when m >= n."""
    items = rng.integers(0, n, m)
    if m >= 2:
        items[-1] = items[0]
    return items.astype(np.int32)


def _run(Dm, X, items):
    out = quality._matrix_moments(_dev(Dm), _dev(X), None if items is None else _dev(items))
    return [o.cpu().numpy() for o in out]


def _check_moments(got, want, d, label):
    row_sums, row_count, row_max, totals = got
    w_sums, w_count, w_max, w_totals = want
    tol_e = (d + 4) * 2.0 ** -23
    np.testing.assert_array_equal(row_count, w_count, err_msg=label)
    assert totals[7] == w_totals[7], label
    np.testing.assert_array_equal(row_max[:, 0], w_max[:, 0].astype(np.float32), err_msg=label)
    assert totals[5] == w_totals[5], label
    for v in (0, 2):                                             # sum D, sum D^2
        np.testing.assert_allclose(row_sums[:, v], w_sums[:, v], rtol=1e-12, atol=0.0, err_msg=label)
        np.testing.assert_allclose(totals[v], w_totals[v], rtol=1e-12, atol=0.0, err_msg=label)
    for v in (1, 3, 4):                                          # sum E, sum E^2, sum D E
        np.testing.assert_allclose(row_sums[:, v], w_sums[:, v], rtol=tol_e, atol=0.0, err_msg=label)
        np.testing.assert_allclose(totals[v], w_totals[v], rtol=tol_e, atol=0.0, err_msg=label)
    np.testing.assert_allclose(row_max[:, 1], w_max[:, 1], rtol=tol_e, atol=0.0, err_msg=label)
    np.testing.assert_allclose(totals[6], w_totals[6], rtol=tol_e, atol=0.0, err_msg=label)


# ---------------------------------------------------------------- 1. moments
@pytest.mark.parametrize("n", SIZES_N)
def test_moments_against_float64(n):
    rng = np.random.default_rng(100 + n)
    for d in DIMS:
        X = rng.standard_normal((n, d)).astype(np.float32)
        for m in SIZES_M:
            Dm, items = _matrix(rng, n, m), _items(rng, n, m)
            got = _run(Dm, X, items)
            _check_moments(got, ref.moments(Dm, X, items), d, f"n={n} m={m} d={d}")
            again = _run(Dm, X, items)
            for a, b in zip(got, again):                          # the same bits on two runs
                assert a.tobytes() == b.tobytes(), f"n={n} m={m} d={d}"
        Dm = _matrix(rng, n, n)                                   # the square matrix of the items themselves
        _check_moments(_run(Dm, X, None), ref.moments(Dm, X), d, f"n={n} square d={d}")


def test_rows_without_a_counted_pair():
    rng = np.random.default_rng(5)
    n, m, d = 65, 130, 2
    Dm, X, items = _matrix(rng, n, m), rng.standard_normal((n, d)).astype(np.float32), _items(rng, n, m)
    row_sums, row_count, row_max, _ = _run(Dm, X, items)
    assert row_count[n // 2] == 0 and not row_sums[n // 2].any() and not row_max[n // 2].any()
    # through the front door: the row is NaN per item, the all-inf column and the scattered inf are `missing`
    mom = quality.matrix_moments(Dm, X, items)
    keep = ref.counted(Dm, items)
    self_pairs = int((np.arange(n)[:, None] == items[None, :]).sum())
    assert self_pairs == m and mom.count == int(keep.sum()) and mom.missing == n * m - m - mom.count
    assert torch.equal(mom.row_counts.cpu(), torch.as_tensor(keep.sum(1)))
    stress, per_item = quality.matrix_stress(Dm, X, items, per_item=True)
    assert per_item.shape == (n,) and bool(torch.isnan(per_item[n // 2])) and 0.0 < stress <= 1.0
    assert int(torch.isnan(per_item).sum()) == 1


def test_a_rows_sums_do_not_depend_on_the_other_rows():
    rng = np.random.default_rng(6)
    n, m, d = 257, 130, 3
    Dm, X, items = _matrix(rng, n, m), rng.standard_normal((n, d)).astype(np.float32), _items(rng, n, m)
    full = _run(Dm, X, items)
    # the first 100 items alone (a different grid); columns that name a later item are re-pointed at item 0 and
    # made missing in both runs, so every remaining pair is the same pair
    late = items >= 100
    Dm2, items2 = Dm.copy(), items.copy()
    Dm2[:, late] = INF
    items2[late] = 0
    a = _run(Dm2, X, items2)
    b = _run(Dm2[:100], X[:100], items2)
    assert a[0][:100].tobytes() == b[0].tobytes() and np.array_equal(a[1][:100], b[1])
    assert not np.array_equal(full[0], a[0])                     # (the masking did change something)


def test_scores_against_the_numpy_formulas():
    rng = np.random.default_rng(7)
    n, m, d = 257, 65, 2
    Dm, X, items = _matrix(rng, n, m), rng.standard_normal((n, d)).astype(np.float32), _items(rng, n, m)
    keep = ref.counted(Dm, items)
    D, E = Dm.astype(np.float64)[keep], ref.embedding_distances(X, items)[keep]
    alpha = (D * E).sum() / (E * E).sum()
    want = np.sqrt(((D - alpha * E) ** 2).sum() / (D * D).sum())
    assert abs(quality.matrix_stress(Dm, X, items) - want) <= 1e-6
    want1 = np.sqrt(((D - E) ** 2).sum() / (D * D).sum())
    assert abs(quality.matrix_stress(_dev(Dm), _dev(X), _dev(items), scale=1.0) - want1) <= 1e-6
    assert abs(quality.matrix_correlation(Dm, X, torch.as_tensor(items)) - np.corrcoef(D, E)[0, 1]) <= 1e-6


def test_nan_and_negative_entries_are_refused():
    X = np.zeros((4, 2), dtype=np.float32)
    for bad in (np.nan, -1.0):
        Dm = np.ones((4, 4), dtype=np.float32)
        Dm[1, 2] = bad
        with pytest.raises(ValueError, match="NaN or negative"):
            quality.matrix_moments(Dm, X)
        with pytest.raises(ValueError, match="NaN or negative"):
            quality.matrix_ranks(Dm, np.zeros((4, 1), dtype=np.int32))


# ---------------------------------------------------------------- 2. exact cases: histogram and ranks
def _hops(n):
    """Hop counts of a ring of n nodes: heavy ties, two per value in every column."""
    i = np.arange(n)
    gap = np.abs(i[:, None] - i[None, :])
    return np.minimum(gap, n - gap).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _exact_case(n, m, d, kind):
    rng = np.random.default_rng(n * 1000 + m * 10 + d)
    X = rng.integers(0, 8, (n, d)).astype(np.float32)
    if kind == "hops":
        assert m == n
        Dm, items = _hops(n), None
    else:
        Dm = (rng.integers(0, 512, (n, m)) / 64.0).astype(np.float32)
        items = _items(rng, n, m)
    Dm = Dm.copy()
    Dm[rng.random(Dm.shape) < 0.15] = INF
    if n >= 2:
        Dm[n // 2, :] = INF
    return Dm, X, items


@pytest.mark.parametrize("n, m, d, kind", [(1, 1, 1, "grid"), (2, 65, 2, "grid"), (65, 63, 3, "grid"),
                                           (257, 130, 2, "grid"), (130, 130, 3, "hops"), (64, 64, 1, "hops")])
@pytest.mark.parametrize("bins", [1, 7, 64])
def test_histogram_is_exact(n, m, d, kind, bins):
    Dm, X, items = _exact_case(n, m, d, kind)
    finite = Dm[np.isfinite(Dm)]
    d_range = (0.0, float(max(finite.max(), 1.0)) if finite.size else 1.0)
    e_range = (0.0, 16.0)                                        # past the grid's diagonal, sqrt(3) 7
    counts = torch.zeros((bins, bins), dtype=torch.int64, device=DEV)
    args = (_dev(Dm), _dev(X), None if items is None else _dev(items), bins, d_range, e_range, counts)
    quality._matrix_histogram(*args)
    want = ref.histogram(Dm, X, items, bins, d_range, e_range)
    np.testing.assert_array_equal(counts.cpu().numpy(), want)
    assert int(want.sum()) == int(ref.counted(Dm, items).sum())  # the ranges hold every counted pair
    quality._matrix_histogram(*args)                             # counts are added to
    np.testing.assert_array_equal(counts.cpu().numpy(), 2 * want)
    # a narrow range leaves pairs out
    narrow = ((0.5, 3.0), (1.0, 5.0))
    counts = torch.zeros((bins, bins), dtype=torch.int64, device=DEV)
    quality._matrix_histogram(*args[:4], narrow[0], narrow[1], counts)
    np.testing.assert_array_equal(counts.cpu().numpy(), ref.histogram(Dm, X, items, bins, *narrow))


def test_histogram_with_more_row_blocks_than_workgroups():
    # 20 000 rows are 1250 blocks of 16 for at most 1024 workgroups: some take a second block
    n, m, bins = 20000, 3, 7
    Dm, X, items = _exact_case(n, m, 2, "grid")
    counts = torch.zeros((bins, bins), dtype=torch.int64, device=DEV)
    quality._matrix_histogram(_dev(Dm), _dev(X), _dev(items), bins, (0.0, 8.0), (0.0, 16.0), counts)
    np.testing.assert_array_equal(counts.cpu().numpy(), ref.histogram(Dm, X, items, bins, (0.0, 8.0), (0.0, 16.0)))
    got = _run(Dm, X, items)                                     # the moments of the same case: one block each
    _check_moments(got, ref.moments(Dm, X, items), 2, "n=20000")
    assert int(counts.sum()) == int(got[3][7])


def test_histogram_through_the_front_door():
    Dm, X, items = _exact_case(257, 130, 2, "grid")
    counts, d_edges, e_edges, n_counted = quality.matrix_shepard_histogram(Dm, X, items, bins=16)
    _, _, w_max, _ = ref.moments(Dm, X, items)
    top_d, top_e = float(w_max[:, 0].max()), float(np.float32(w_max[:, 1].max()))
    assert d_edges[-1] == top_d and e_edges[-1] == top_e and d_edges[0] == e_edges[0] == 0.0
    np.testing.assert_array_equal(counts.cpu().numpy(), ref.histogram(Dm, X, items, 16, (0.0, top_d), (0.0, top_e)))
    assert n_counted == int(ref.counted(Dm, items).sum())


def _lists(rng, n, m, k, items):
    """Lists with valid items, -1, entries >= n and the column's own item."""
    idx = rng.integers(0, n, (m, k)).astype(np.int32)
    own = np.arange(n) if items is None else items
    idx[rng.random((m, k)) < 0.05] = -1
    idx[rng.random((m, k)) < 0.05] = n
    idx[rng.random((m, k)) < 0.02] = n + 7
    mask = rng.random((m, k)) < 0.05
    idx[mask] = np.broadcast_to(own[:, None], (m, k))[mask]
    idx[0, 0] = own[0]
    return idx


@pytest.mark.parametrize("n, m, d, kind", [(2, 65, 2, "grid"), (65, 63, 3, "grid"), (257, 130, 2, "grid"),
                                           (130, 130, 3, "hops"), (1000, 65, 1, "grid")])
@pytest.mark.parametrize("k", [1, 15, 33, 64])
def test_ranks_are_exact(n, m, d, kind, k):
    Dm, _, items = _exact_case(n, m, d, kind)
    idx = _lists(np.random.default_rng(k), n, m, k, items)
    got = quality.matrix_ranks(Dm, idx, items)
    assert got.dtype == torch.int32 and tuple(got.shape) == (m, k)
    np.testing.assert_array_equal(got.cpu().numpy(), ref.ranks(Dm, idx, items))
    again = quality._matrix_ranks(_dev(Dm), _dev(idx), None if items is None else _dev(items))
    assert torch.equal(got, again)


@pytest.mark.parametrize("k", [1, 15, 33, 64])
def test_a_columns_own_order_ranks_0_to_k_minus_1(k):
    # a full matrix with ties and inf: the first k items of every column under (value, index), the own item left out
    n = 200
    Dm, _, _ = _exact_case(n, n, 2, "hops")
    idx = np.empty((n, k), dtype=np.int32)
    for b in range(n):
        order = np.lexsort((np.arange(n), Dm[:, b].astype(np.float64)))
        idx[b] = order[order != b][:k]
    got = quality.matrix_ranks(_dev(Dm), _dev(idx)).cpu().numpy()
    np.testing.assert_array_equal(got, np.broadcast_to(np.arange(k, dtype=np.int32), (n, k)))


def test_matrix_trustworthiness_lists_and_formula():
    rng = np.random.default_rng(11)
    n, k = 130, 7
    X = rng.standard_normal((n, 2)).astype(np.float32)
    Dm, _, _ = _exact_case(n, n, 3, "hops")
    E = ref.embedding_distances(X, np.arange(n))
    np.fill_diagonal(E, np.inf)
    lists = np.argsort(E, axis=1, kind="stable")[:, :k]          # no ties among gaussian points
    want = ref.sampled_score(ref.ranks(Dm, lists), n, k)
    got, rows = quality.matrix_trustworthiness(Dm, X, n_neighbors=k, per_item=True)
    assert abs(got - want) <= 1e-12 and rows.shape == (n,)
    items = np.array([5, 129, 5, 0, 77], dtype=np.int32)         # a sample with a repeat: the mean over the listed
    want = ref.sampled_score(ref.ranks(Dm[:, items], lists[items], items), n, k)
    assert abs(quality.matrix_trustworthiness(Dm[:, items], X, n_neighbors=k, items=items) - want) <= 1e-12


@pytest.mark.parametrize("k", [1, 15, 63, 64])
def test_the_lists_of_a_few_rows_are_the_self_joins(k):
    # an integer grid: duplicate points and ties everywhere; 300 points on 64 cells, so rows with k + 1 twins exist
    rng = np.random.default_rng(k)
    n = 300
    X = _dev(rng.integers(0, 8, (n, 2)).astype(np.float32))
    X[:70] = X[0]                                                # 70 copies of one point: more than k + 1 at distance 0
    full = quality._embedding_lists(X, k, None)
    items = _dev(np.array([0, 5, 69, 70, 299, 5, 123], dtype=np.int64))
    assert torch.equal(quality._embedding_lists(X, k, items), full[items])
    assert not bool((full == torch.arange(n, device=DEV, dtype=torch.int32)[:, None]).any())


# ---------------------------------------------------------------- 3. the library's own argument checks
def test_invalid_arguments_launch_nothing():
    lib = _lib.load()
    p, st = _lib.ptr, _lib.stream_ptr(torch.device(DEV))
    n, m, d, k = 8, 4, 2, 3
    Dm, X = torch.ones((n, m), device=DEV), torch.zeros((n, d), device=DEV)
    items = torch.zeros(m, dtype=torch.int32, device=DEV)
    sums, count = torch.zeros((n, 5), dtype=torch.float64, device=DEV), torch.zeros(n, dtype=torch.int64, device=DEV)
    maxs, totals = torch.zeros((n, 2), device=DEV), torch.zeros(8, dtype=torch.float64, device=DEV)
    work = torch.zeros(64, dtype=torch.uint8, device=DEV)
    counts = torch.zeros((4, 4), dtype=torch.int64, device=DEV)
    idx = torch.zeros((m, k), dtype=torch.int32, device=DEV)
    ranks = torch.full((m, k), 99, dtype=torch.int32, device=DEV)

    def moments(n_=n, m_=m, D_=Dm, it_=items, d_=d, X_=X, s_=sums, w_=work):
        return lib.mde_matrix_moments(n_, m_, p(D_), p(it_), d_, p(X_), p(s_), p(count), p(maxs), p(totals), p(w_), st)

    def hist(n_=n, m_=m, it_=items, d_=d, bins_=4, dr=(0.0, 1.0), er=(0.0, 1.0), c_=counts):
        return lib.mde_matrix_histogram(n_, m_, p(Dm), p(it_), d_, p(X), bins_, dr[0], dr[1], er[0], er[1], p(c_), st)

    def rank(n_=n, m_=m, it_=items, k_=k, idx_=idx):
        return lib.mde_matrix_ranks(n_, m_, p(Dm), p(it_), k_, p(idx_), p(ranks), st)

    bad = [moments(n_=0), moments(m_=0), moments(n_=2 ** 31), moments(m_=2 ** 31), moments(D_=None),
           moments(it_=None), moments(d_=0), moments(d_=9), moments(X_=None), moments(s_=None), moments(w_=None),
           hist(n_=0), hist(it_=None), hist(d_=9), hist(bins_=0), hist(bins_=65), hist(dr=(1.0, 1.0)),
           hist(er=(2.0, 1.0)), hist(c_=None),
           rank(n_=0), rank(m_=2 ** 31), rank(it_=None), rank(k_=0), rank(k_=65), rank(idx_=None)]
    assert all(rc == _lib.MDE_E_INVALID for rc in bad)
    assert "mde_matrix_ranks" in _lib.last_error()
    assert lib.mde_matrix_moments_work_bytes(0, 1) == _lib.MDE_E_INVALID
    assert lib.mde_matrix_moments_work_bytes(1, 2 ** 31) == _lib.MDE_E_INVALID
    assert lib.mde_matrix_moments_work_bytes(4097, 1) == 2 * 8 * 8
    torch.cuda.synchronize()
    assert int(counts.sum()) == 0 and bool((ranks == 99).all()) and not bool(sums.any())
    assert moments() == _lib.MDE_OK and hist() == _lib.MDE_OK and rank() == _lib.MDE_OK
    torch.cuda.synchronize()

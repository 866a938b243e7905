"""mde_pair_moments, mde_pair_histogram and the global scores of pymde_amd.quality on the GPU.

The reference throughout is numpy float64 brute force on the dense n x n distance matrices.  The shapes are the
smallest that reach every branch: partial query and column tiles (193, 257, 300 rows), partial and multiple feature
chunks (37, 70, 784 features), one query block (64) and one pair (2), empty slices (40 slices of 4 column tiles)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"


# ---------------------------------------------------------------- helpers
def _dev(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(DEV).contiguous()


def _dist64(A, mode=0):
    """Dense float64 distances of the rows of A: Euclidean (mode 0) or half the squared distance (mode 1)."""
    A = np.asarray(A, dtype=np.float64)
    d2 = np.empty((A.shape[0], A.shape[0]))
    for i in range(0, A.shape[0], 16):
        d2[i:i + 16] = ((A[i:i + 16, None, :] - A[None, :, :]) ** 2).sum(-1)
    return 0.5 * d2 if mode else np.sqrt(d2)


def _reference(D, E, rows=None):
    """(row_sums [n_q, 5], row_max [n_q, 2], totals [8]) of the pairs (rows[r], j), j != rows[r], in float64."""
    n = D.shape[0]
    rows = np.arange(n) if rows is None else np.asarray(rows)
    off = np.ones((len(rows), n), dtype=bool)
    off[np.arange(len(rows)), rows] = False
    d, e = np.where(off, D[rows], 0.0), np.where(off, E[rows], 0.0)
    sums = np.stack([v.sum(1) for v in (d, e, d * d, e * e, d * e)], 1)
    maxs = np.stack([d.max(1), e.max(1)], 1)
    totals = np.concatenate([sums.sum(0), maxs.max(0), [float(off.sum())]])
    return sums, maxs, totals


def _run(A, B, mode_a=0, mode_b=0, rows=None, slices=1):
    from pymde_amd import quality
    q = None if rows is None else _dev(rows, torch.int32)
    sums, maxs, totals = quality._pair_moments(_dev(A, torch.float32), _dev(B, torch.float32), mode_a, mode_b, q, slices)
    torch.cuda.synchronize()
    return sums.cpu().numpy(), maxs.cpu().numpy(), totals.cpu().numpy()


def _worst(got, want):
    """The largest |got - want| / |want| (0 where both are 0)."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    err = np.abs(got - want)
    return float(np.where(err == 0.0, 0.0, err / np.where(want == 0.0, 1e-300, np.abs(want))).max())


def _check(got, want, tol, label):
    sums, maxs, totals = got
    wsums, wmaxs, wtotals = want
    e_rows, e_tot = _worst(sums, wsums), _worst(totals[:5], wtotals[:5])
    print("%s: worst relative error of a row sum %.3g, of a total %.3g (bound %.3g)" % (label, e_rows, e_tot, tol))
    assert e_rows <= tol and e_tot <= tol
    assert totals[7] == wtotals[7]
    return e_rows, e_tot


def _grid_case(n, nfa, nfb):
    rng = np.random.default_rng(1000 * n + nfa + 1)
    return rng.integers(-3, 4, (n, nfa)).astype(np.float32), rng.integers(-3, 4, (n, nfb)).astype(np.float32)


def _gauss_case(n, nfa, nfb):
    rng = np.random.default_rng(7 * n + nfa)
    A = rng.standard_normal((n, nfa)) * rng.uniform(0.2, 3.0, nfa)
    B = rng.standard_normal((n, nfb)) * rng.uniform(0.2, 3.0, nfb)
    return (A - A.mean(0)).astype(np.float32), (B - B.mean(0)).astype(np.float32)


_CACHE = {}


def _cached(key, make):
    """Inputs and float64 references are computed once per module and shared (never modified)."""
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _case(kind, n, nfa, nfb):
    def make():
        A, B = (_grid_case if kind == "grid" else _gauss_case)(n, nfa, nfb)
        D, E = _dist64(A), _dist64(B)
        return A, B, D, E, _reference(D, E)
    return _cached((kind, n, nfa, nfb), make)


# ---------------------------------------------------------------- 1. integer grids: exact d2
@pytest.mark.parametrize("slices", [1, 3])
@pytest.mark.parametrize("n,nfa,nfb", [(193, 37, 2), (64, 8, 3), (2, 1, 1)])
def test_exact_grid(n, nfa, nfb, slices):
    """Every d2 is an exact integer in float32 and float64, so D is one correctly rounded sqrtf away from the
    reference (2^-24 relative; a mode-1 product is exact): 2^-21 leaves room to spare."""
    A, B, D, E, want = _case("grid", n, nfa, nfb)
    if n == 2:
        assert D[0, 1] > 0 and E[0, 1] > 0
    got = _run(A, B, slices=slices)
    _check(got, want, 2.0 ** -21, "grid %dx%d/%d slices=%d" % (n, nfa, nfb, slices))
    assert got[2][7] == n * (n - 1)
    assert np.array_equal(got[1], want[1].astype(np.float32))              # the maxima, rounded once
    assert np.array_equal(got[2][5:7], want[2][5:7].astype(np.float32).astype(np.float64))


@pytest.mark.parametrize("slices", [1, 3])
@pytest.mark.parametrize("mode_a,mode_b", [(0, 0), (1, 0), (0, 1)])
def test_exact_grid_with_duplicate_rows(mode_a, mode_b, slices):
    """81 distinct rows among 200: zero distances everywhere, and a duplicate of the query counts (D = 0 adds
    nothing to the sums, but the pair is in the count)."""
    def make():
        rng = np.random.default_rng(5)
        A = rng.integers(0, 3, (200, 4)).astype(np.float32)
        B = rng.integers(0, 3, (200, 2)).astype(np.float32)
        return A, B
    A, B = _cached("dup", make)
    want = _cached(("dup", mode_a, mode_b), lambda: _reference(_dist64(A, mode_a), _dist64(B, mode_b)))
    got = _run(A, B, mode_a, mode_b, slices=slices)
    _check(got, want, 2.0 ** -21, "duplicates modes %d%d slices=%d" % (mode_a, mode_b, slices))
    assert got[2][7] == 200 * 199
    assert np.array_equal(got[1], want[1].astype(np.float32))


# ---------------------------------------------------------------- 2. Gaussian data
GAUSS = [(193, 37, 2), (300, 70, 3), (257, 784, 2)]


def _gauss_tol(nfa, nfb):
    """Four times the worst case of a float32 dot-product chain over the features plus the three roundings of
    |x|^2 + |y|^2 - 2 x.y, as a relative bound."""
    return 4.0 * (max(nfa, nfb) + 4) * 2.0 ** -24


@pytest.mark.parametrize("n,nfa,nfb", GAUSS)
def test_gaussian_data(n, nfa, nfb):
    """Columns scaled by U(0.2, 3) and centred.  A float32 emulation of the kernel's arithmetic on the CPU, without
    fused multiply-add, has worst row errors of 1.1e-7, 2.0e-7 and 7.5e-7 at these three shapes: >= 10 x under the
    bound."""
    A, B, D, E, want = _case("gauss", n, nfa, nfb)
    for slices in (1, 0):
        got = _run(A, B, slices=slices)
        _check(got, want, _gauss_tol(nfa, nfb), "gauss %dx%d/%d slices=%d" % (n, nfa, nfb, slices))
        assert _worst(got[1], want[1]) <= _gauss_tol(nfa, nfb)
        assert _worst(got[2][5:7], want[2][5:7]) <= _gauss_tol(nfa, nfb)


# ---------------------------------------------------------------- 3. mode 1 through the Python door
def test_cosine_through_pair_moments():
    from scipy.spatial.distance import cdist
    from pymde_amd import quality
    n, nfa, nfb = 193, 37, 2
    rng = np.random.default_rng(3)
    data = rng.standard_normal((n, nfa)) * rng.uniform(0.2, 3.0, nfa) + 0.5
    data = (data / np.linalg.norm(data, axis=1, keepdims=True)).astype(np.float32)   # unit rows (to float32)
    X = _gauss_case(n, nfa, nfb)[1]
    D = cdist(data.astype(np.float64), data.astype(np.float64), "cosine")
    wsums, wmaxs, wtotals = _reference(D, _dist64(X))
    m = quality.pair_moments(_dev(data), X, metric="cosine")
    tol = _gauss_tol(nfa, nfb)
    got = (m.row_sums.cpu().numpy(), None, np.array([m.sum_d, m.sum_e, m.sum_dd, m.sum_ee, m.sum_de, m.max_d, m.max_e,
                                                      m.count], dtype=np.float64))
    _check(got, (wsums, wmaxs, wtotals), tol, "cosine %dx%d/%d" % (n, nfa, nfb))
    assert m.count == n * (n - 1) and m.rows is None
    assert m.row_sums.dtype == torch.float64 and m.row_sums.is_cuda and m.row_sums.shape == (n, 5)
    assert abs(m.max_d - wtotals[5]) <= tol * wtotals[5] and abs(m.max_e - wtotals[6]) <= tol * wtotals[6]
    # correlation distance = cosine distance of the row-centred data
    Dc = cdist(data.astype(np.float64), data.astype(np.float64), "correlation")
    mc = quality.pair_moments(data, _dev(X), metric="correlation")
    assert abs(mc.sum_d - Dc.sum()) <= tol * Dc.sum()


# ---------------------------------------------------------------- 4. sampled query rows
@pytest.mark.parametrize("slices", [1, 3])
def test_sampled_rows_equal_the_full_run_bit_for_bit(slices):
    A, B, D, E, _ = _case("gauss", 193, 37, 2)
    rows = np.random.default_rng(4).permutation(193)[:70].astype(np.int32)     # out of order, a partial block
    assert (np.diff(rows) < 0).any()
    full = _run(A, B, slices=slices)
    part = _run(A, B, rows=rows, slices=slices)
    assert np.array_equal(part[0].view(np.uint64), full[0][rows].view(np.uint64))
    assert np.array_equal(part[1].view(np.uint32), full[1][rows].view(np.uint32))
    assert part[2][7] == 70 * 192
    _check(part, _reference(D, E, rows), _gauss_tol(37, 2), "sample 70 of 193 slices=%d" % slices)


def test_self_exclusion_follows_the_index():
    """Row 7 is a copy of row 150.  Query 7 skips row 7, not its twin: the pair (7, 150) counts with D = E = 0,
    and a query listed twice is two queries."""
    A, B = (v.copy() for v in _case("grid", 193, 37, 2)[:2])
    A[7], B[7] = A[150], B[150]
    rows = np.array([150, 7, 7, 3], dtype=np.int32)
    D, E = _dist64(A), _dist64(B)
    want = _reference(D, E, rows)
    got = _run(A, B, rows=rows)
    _check(got, want, 2.0 ** -21, "twin rows")
    assert got[2][7] == 4 * 192
    assert np.array_equal(got[0][1].view(np.uint64), got[0][2].view(np.uint64))
    # had the twin been skipped by value, the sums would be the same: the histogram sees the zero pair
    from pymde_amd import quality
    counts = quality._pair_histogram(_dev(A), _dev(B), 2, (-0.5, 0.5), (-0.5, 0.5), q_rows=_dev(rows[:2]))
    assert int(counts.sum()) == 2 and int(counts[1, 1]) == 2      # (150, 7) and (7, 150), D = E = 0 -> bin 1


def test_sample_through_the_python_door():
    from pymde_amd import quality
    A, B, D, E, _ = _case("gauss", 193, 37, 2)
    m = quality.pair_moments(A, B, sample=70, seed=3)
    assert m.rows is not None and m.rows.shape == (70,) and len(set(m.rows.tolist())) == 70
    assert torch.equal(m.rows, quality._sample_rows(193, 70, 3))
    assert m.count == 70 * 192 and m.row_sums.shape == (70, 5)
    full = quality.pair_moments(A, B)
    assert torch.equal(m.row_sums, full.row_sums[m.rows.to(DEV)])           # bit for bit (same automatic slices)
    assert quality.pair_moments(A, B, sample=193).rows is None              # every row: no sample


# ---------------------------------------------------------------- 5. slices
def test_slices():
    from pymde_amd import quality
    A, B, D, E, want = _case("gauss", 193, 37, 2)
    Ad, Bd = _dev(A), _dev(B)
    top = (0.0, float(want[2][5])), (0.0, float(want[2][6]))
    base_totals, base_hist = None, None
    for slices in (1, 2, 5, 40):                                # 4 column tiles: 5 and 40 leave empty slices
        got = _run(A, B, slices=slices)
        again = _run(A, B, slices=slices)
        for a, b in zip(got, again):
            assert np.array_equal(a.view(np.uint8), b.view(np.uint8))       # run to run: the same bits
        _check(got, want, _gauss_tol(37, 2), "slices=%d" % slices)
        hist = quality._pair_histogram(Ad, Bd, 16, top[0], top[1], slices=slices).cpu().numpy()
        if base_totals is None:
            base_sums, base_totals, base_hist = got[0], got[2], hist
        assert _worst(got[2], base_totals) <= 1e-12 and _worst(got[0], base_sums) <= 1e-12
        assert np.array_equal(hist, base_hist)
    assert base_hist.sum() > 0.99 * 193 * 192


# ---------------------------------------------------------------- 6. the histogram
def test_histogram_of_points_on_a_line():
    from pymde_amd import quality
    rng = np.random.default_rng(6)
    n, M = 150, 40
    a = rng.integers(0, M + 1, n)
    b = rng.integers(0, 31, n)
    a[0], a[1], b[0], b[1] = 0, M, 0, 30                        # the extremes are present
    data = np.stack([a, 0 * a, 0 * a], 1).astype(np.float32)
    X = np.stack([0 * b, b], 1).astype(np.float32)
    off = ~np.eye(n, dtype=bool)
    d, e = np.abs(a[:, None] - a[None, :])[off].astype(np.float64), np.abs(b[:, None] - b[None, :])[off].astype(np.float64)
    bins = M + 1
    rng_ = ((-0.5, M + 0.5), (-0.5, M + 0.5))
    counts, d_edges, e_edges, n_counted = quality.shepard_histogram(data, X, bins=bins, range=rng_)
    want, wd, we = np.histogram2d(d, e, bins=bins, range=rng_)
    assert counts.dtype == torch.int64 and counts.is_cuda and counts.shape == (bins, bins)
    assert np.array_equal(counts.cpu().numpy(), want.astype(np.int64))
    assert n_counted == n * (n - 1)
    assert d_edges.dtype == np.float64 and np.allclose(d_edges, wd, atol=1e-12) and np.allclose(e_edges, we, atol=1e-12)
    # a narrower range drops what lies outside either interval and says how many remain
    narrow = ((-0.5, 9.5), (-0.5, 19.5))
    counts, _, _, n_counted = quality.shepard_histogram(data, X, bins=10, range=narrow)
    want, _, _ = np.histogram2d(d, e, bins=10, range=narrow)
    assert np.array_equal(counts.cpu().numpy(), want.astype(np.int64))
    assert n_counted == int(((d <= 9) & (e <= 19)).sum()) and 0 < n_counted < n * (n - 1)
    # one bin, and a sample
    counts, _, _, n_counted = quality.shepard_histogram(data, X, bins=1, range=rng_, sample=20, seed=1)
    assert counts.shape == (1, 1) and n_counted == int(counts[0, 0]) == 20 * (n - 1)


def test_histogram_with_the_automatic_range():
    from pymde_amd import quality
    A, B, D, E, want = _case("gauss", 300, 70, 3)
    n = 300
    counts, d_edges, e_edges, n_counted = quality.shepard_histogram(A, _dev(B), bins=64)
    assert n_counted == n * (n - 1) == int(counts.sum())
    assert d_edges[0] == 0.0 and e_edges[0] == 0.0 and len(d_edges) == len(e_edges) == 65
    m = quality.pair_moments(A, B)
    assert d_edges[-1] == m.max_d and e_edges[-1] == m.max_e
    c = counts.cpu().numpy().astype(np.float64)
    for axis, edges, mean in ((1, d_edges, m.sum_d / m.count), (0, e_edges, m.sum_e / m.count)):
        centres = 0.5 * (edges[:-1] + edges[1:])
        assert abs((c.sum(axis) * centres).sum() / n_counted - mean) <= edges[1] - edges[0]


# ---------------------------------------------------------------- 7. the Python entry points
def test_scores_against_the_float64_formulas():
    from pymde_amd import quality
    A, _, D, _, _ = _case("gauss", 300, 70, 3)
    rng = np.random.default_rng(8)
    top = np.argsort(A.var(0))[-2:]                             # an embedding that keeps something: the two widest
    X = (A[:, top] + 0.5 * rng.standard_normal((300, 2))).astype(np.float32)   # columns, blurred
    E = _dist64(X)
    off = ~np.eye(300, dtype=bool)
    d, e = D[off], E[off]
    alpha = (d * e).sum() / (e * e).sum()
    want_opt = np.sqrt(((d - alpha * e) ** 2).sum() / (d * d).sum())
    want_one = np.sqrt(((d - e) ** 2).sum() / (d * d).sum())
    want_r = np.corrcoef(d, e)[0, 1]
    s = quality.stress(A, X)
    assert isinstance(s, float) and abs(s - want_opt) <= 1e-5
    assert abs(quality.stress(_dev(A), _dev(X), scale=1.0) - want_one) <= 1e-5
    r = quality.distance_correlation(A, X)
    assert isinstance(r, float) and abs(r - want_r) <= 1e-5
    assert 0.05 < want_opt < 0.95 and 0.05 < want_r < 0.999
    for scale, a in (("optimal", alpha), (1.0, 1.0)):
        value, rows = quality.stress(A, X, scale=scale, per_item=True)
        want_rows = np.sqrt((np.where(off, (D - a * E) ** 2, 0.0)).sum(1) / np.where(off, D * D, 0.0).sum(1))
        assert rows.dtype == torch.float32 and rows.is_cuda and rows.shape == (300,)
        assert np.abs(rows.cpu().numpy() - want_rows).max() <= 1e-5
        assert value == quality.stress(A, X, scale=scale)
    # a sample estimates the same numbers (70 of 300 rows: 20 930 pairs)
    assert abs(quality.stress(A, X, sample=70, seed=1) - want_opt) <= 0.05
    value, rows = quality.stress(A, X, per_item=True, sample=70, seed=1)
    assert rows.shape == (70,)


def test_the_identity_embedding():
    """The same matrix on both sides gives the same float32 distance twice.  Near stress = 0 the formula loses
    half its digits (1 - (sum D E)^2 / (sum D^2 sum E^2) in float64): <= 1e-3 is what is promised."""
    from pymde_amd import quality
    A = _case("gauss", 300, 70, 3)[0]
    assert quality.stress(A, A[:, :]) <= 1e-3
    assert quality.stress(A, A[:, :], scale=1.0) <= 1e-3
    assert quality.distance_correlation(A, A[:, :]) >= 1.0 - 1e-6


def test_sparse_data_gives_the_dense_result():
    import scipy.sparse
    from pymde_amd import quality
    rng = np.random.default_rng(9)
    dense = (rng.standard_normal((193, 37)) * (rng.random((193, 37)) < 0.3)).astype(np.float32)
    dense[np.arange(193), rng.integers(0, 37, 193)] = 1.0       # no empty row
    X = _case("gauss", 193, 37, 2)[1]
    for metric in ("euclidean", "cosine"):
        a = quality.pair_moments(scipy.sparse.csr_matrix(dense), X, metric=metric)
        b = quality.pair_moments(dense, X, metric=metric)
        assert a[:8] == b[:8] and torch.equal(a.row_sums, b.row_sums)
        assert quality.stress(scipy.sparse.csr_matrix(dense), X, metric=metric) == quality.stress(dense, X, metric=metric)


# ---------------------------------------------------------------- 8. the C ABI refuses and launches nothing
def test_invalid_arguments_launch_nothing():
    from pymde_amd import _lib
    lib = _lib.load()
    n, nfa, nfb, bins = 100, 5, 2, 8
    A = _dev(np.random.default_rng(0).standard_normal((n, nfa)).astype(np.float32))
    B = _dev(np.random.default_rng(1).standard_normal((n, nfb)).astype(np.float32))
    q = _dev(np.arange(10, dtype=np.int32))
    sums = torch.full((n, 5), -7.0, dtype=torch.float64, device=DEV)
    maxs = torch.full((n, 2), -7.0, dtype=torch.float32, device=DEV)
    totals = torch.full((8,), -7.0, dtype=torch.float64, device=DEV)
    counts = torch.zeros((bins, bins), dtype=torch.int64, device=DEV)
    work = torch.full((1 << 20,), 0x5A, dtype=torch.uint8, device=DEV)
    p, st = _lib.ptr, _lib.stream_ptr()

    def moments(n_=n, nfa_=nfa, A_=A, ma=0, nfb_=nfb, B_=B, mb=0, n_q=n, q_=None, slices=1, sums_=sums, maxs_=maxs,
                totals_=totals, work_=work):
        return lib.mde_pair_moments(n_, nfa_, p(A_), ma, nfb_, p(B_), mb, n_q, p(q_), slices, p(sums_), p(maxs_),
                                    p(totals_), p(work_), st)

    def hist(n_=n, nfa_=nfa, A_=A, ma=0, nfb_=nfb, B_=B, mb=0, n_q=n, q_=None, slices=1, bins_=bins, a=(0.0, 9.0),
             b=(0.0, 9.0), counts_=counts, work_=work):
        return lib.mde_pair_histogram(n_, nfa_, p(A_), ma, nfb_, p(B_), mb, n_q, p(q_), slices, bins_, a[0], a[1],
                                      b[0], b[1], p(counts_), p(work_), st)
    bad = [moments(n_=1, n_q=1), moments(n_=0, n_q=0), moments(n_q=0, q_=q), moments(n_q=-1, q_=q),
           moments(n_=2 ** 31, n_q=2 ** 31), moments(n_=2 ** 31, n_q=10, q_=q), moments(ma=2), moments(ma=-1),
           moments(mb=2), moments(mb=-1), moments(A_=None), moments(B_=None), moments(sums_=None), moments(maxs_=None),
           moments(totals_=None), moments(work_=None), moments(slices=-1), moments(slices=65536), moments(nfa_=0),
           moments(nfb_=0), moments(n_q=10),                    # without q_rows every row is a query
           hist(n_=1, n_q=1), hist(n_q=0, q_=q), hist(n_=2 ** 31, n_q=10, q_=q), hist(ma=2), hist(mb=-1),
           hist(bins_=0), hist(bins_=65), hist(bins_=-1), hist(a=(1.0, 1.0)), hist(a=(2.0, 1.0)), hist(b=(1.0, 1.0)),
           hist(b=(0.0, -1.0)), hist(a=(0.0, float("nan"))), hist(A_=None), hist(B_=None), hist(counts_=None),
           hist(work_=None), hist(slices=-1), hist(slices=65536)]
    assert bad == [_lib.MDE_E_INVALID] * len(bad)
    assert "mde_pair_histogram" in _lib.last_error()
    assert moments(slices=65536) == _lib.MDE_E_INVALID and "mde_pair_moments" in _lib.last_error()
    for args in ((1, 1, 1), (n, 0, 1), (2 ** 31, 10, 1), (n, n, -1), (n, n, 65536)):
        assert lib.mde_pair_moments_work_bytes(*args) == _lib.MDE_E_INVALID
    torch.cuda.synchronize()
    assert (sums == -7).all() and (maxs == -7).all() and (totals == -7).all() and (counts == 0).all()
    assert (work == 0x5A).all()                                 # not even the row norms
    # and the same calls with valid arguments run
    assert lib.mde_pair_moments_work_bytes(n, n, 3) == 8 * n + 3 * n * 48
    assert moments(slices=3) == _lib.MDE_OK and hist() == _lib.MDE_OK
    assert moments(n_q=10, q_=q) == _lib.MDE_OK
    torch.cuda.synchronize()
    assert totals[7].item() == 10 * (n - 1) and 0 < int(counts.sum()) <= n * (n - 1)

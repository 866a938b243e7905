"""``mde_csr_spmm`` (csrc/mde_spmm.hip): C = A B - u v^T for a CSR A and a thin dense B, against the float64
row-by-row reference of ``_pca_reference.spmm``.

Bound.  With ``want`` the float64 reference, ``|got - want| <= 2^-24 |want| + 2^-40 (sum |a b| + |u v|)``: the one
float32 rounding at the store, plus a float64 summation order that may differ across the segments of a long row.
Integer-valued data must come out exactly."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

from pymde_amd import _lib, sparse

import _pca_reference as ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
WIDTHS = [1, 3, 32, 64, 65, 200, 256]


def _device(A):
    return sparse.to_device_csr(sp.csr_matrix(A), DEV).validate()


def _host(csr):
    return csr.indptr.cpu().numpy(), csr.indices.cpu().numpy(), csr.values.cpu().numpy()


def _spmm(csr, B, u=None, v=None):
    out = sparse.spmm(csr, torch.as_tensor(B, device=DEV),
                      None if u is None else torch.as_tensor(u, device=DEV),
                      None if v is None else torch.as_tensor(v, device=DEV))
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _assert_within_bound(got, want, scale, what):
    assert got.dtype == np.float32 and got.shape == want.shape
    err, bound = np.abs(got.astype(np.float64) - want), ref.spmm_bound(want, scale)
    worst = float((err / np.maximum(bound, 1e-300)).max()) if err.size else 0.0
    print("%s: worst error / bound = %.3f" % (what, worst))
    assert np.all(err <= bound), (what, worst)


def _random_csr(n, nf, density, seed, empty=()):
    rng = np.random.default_rng(seed)
    A = sp.random(n, nf, density=density, format="lil", random_state=seed, dtype=np.float32,
                  data_rvs=lambda m: rng.standard_normal(m).astype(np.float32))
    for r in empty:
        A.rows[r], A.data[r] = [], []
    return A.tocsr()


@pytest.fixture(scope="module")
def general():
    """A 300 x 500 CSR at 5 % with some empty rows, B of 256 columns, u, v, and the references of the four
    (u, v) combinations at the full width: a narrower product is a prefix of the columns."""
    A = _random_csr(300, 500, 0.05, seed=11, empty=(0, 17, 18, 150, 299))
    rng = np.random.default_rng(12)
    B = rng.standard_normal((500, 256)).astype(np.float32)
    u = rng.standard_normal(300).astype(np.float32)
    v = rng.standard_normal(256)
    csr = _device(A)
    refs = {(hu, hv): ref.spmm(*_host(csr), B, u if hu else None, v if hv else None, with_scale=True)
            for hu in (False, True) for hv in (False, True)}
    return csr, B, u, v, refs


def _long_rows(L, seed, integer=False):
    """nf = 2 L + 1 columns; one row each of 2 L, L - 1, L, L + 1 and 2 L + 1 entries beside short and empty rows;
    a long row first (so the next row starts on a segment boundary of the arrays) and a long row last."""
    rng = np.random.default_rng(seed)
    nf = 2 * L + 1
    lengths = [2 * L, 0, 5, L - 1, 0, 0, 1, L, 70, L + 1, 3, 0, 2 * L + 1]
    rows, cols, vals = [], [], []
    for i, length in enumerate(lengths):
        c = np.sort(rng.choice(nf, size=length, replace=False))
        rows.append(np.full(length, i))
        cols.append(c)
        vals.append(rng.integers(1, 4, length).astype(np.float32) if integer
                    else rng.standard_normal(length).astype(np.float32))
    A = sp.csr_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))),
                      shape=(len(lengths), nf), dtype=np.float32)
    assert list(np.diff(A.indptr)) == lengths
    return A


@pytest.mark.parametrize("r", WIDTHS)
def test_widths_and_corrections(general, r):
    csr, B, u, v, refs = general
    Br = np.ascontiguousarray(B[:, :r])
    for (has_u, has_v), (want, scale) in refs.items():
        got = _spmm(csr, Br, u if has_u else None, v[:r] if has_v else None)
        _assert_within_bound(got, want[:, :r], scale[:, :r], "r=%d u=%s v=%s" % (r, has_u, has_v))
    # u without v corrects nothing
    assert np.array_equal(_spmm(csr, Br, u, None), _spmm(csr, Br, None, None))


@pytest.mark.parametrize("r", [3, 65])
def test_integer_data_is_exact(r):
    rng = np.random.default_rng(r)
    L = sparse.spmm_segment()
    short = _random_csr(300, 500, 0.05, seed=3, empty=(5, 299))
    short.data = rng.integers(1, 4, short.nnz).astype(np.float32)
    for A in (short, _long_rows(L, seed=4, integer=True)):
        n, nf = A.shape
        B = rng.integers(0, 4, (nf, r)).astype(np.float32)
        u = rng.integers(0, 4, n).astype(np.float32)
        v = rng.integers(0, 4, r).astype(np.float64)
        csr = _device(A)
        want = ref.spmm(*_host(csr), B, u, v)
        assert np.abs(want).max() < 2 ** 24                  # every value is a float32
        assert np.array_equal(_spmm(csr, B, u, v).astype(np.float64), want)


@pytest.mark.parametrize("r", [3, 65])
def test_long_rows(r):
    L = sparse.spmm_segment()
    A = _long_rows(L, seed=20 + r)
    n, nf = A.shape
    rng = np.random.default_rng(r)
    B = rng.standard_normal((nf, r)).astype(np.float32)
    u = rng.standard_normal(n).astype(np.float32)
    v = rng.standard_normal(r)
    csr = _device(A)
    want, scale = ref.spmm(*_host(csr), B, u, v, with_scale=True)
    got = _spmm(csr, B, u, v)
    _assert_within_bound(got, want, scale, "long rows r=%d" % r)
    assert np.array_equal(got, _spmm(csr, B, u, v))          # the same bits on two calls
    want0, scale0 = ref.spmm(*_host(csr), B, with_scale=True)
    _assert_within_bound(_spmm(csr, B), want0, scale0, "long rows, no correction, r=%d" % r)


def test_many_short_rows_per_segment():
    """More than 64 rows start inside one segment length of the arrays (their pointers are read 64 at a time)."""
    A = _random_csr(3000, 50, 0.05, seed=31, empty=tuple(range(100, 180)))
    rng = np.random.default_rng(32)
    B, u, v = rng.standard_normal((50, 5)).astype(np.float32), rng.standard_normal(3000).astype(np.float32), \
        rng.standard_normal(5)
    csr = _device(A)
    want, scale = ref.spmm(*_host(csr), B, u, v, with_scale=True)
    _assert_within_bound(_spmm(csr, B, u, v), want, scale, "3000 short rows")


@pytest.mark.parametrize("shape,density", [((1, 40), 0.5), ((40, 1), 0.5), ((6, 9), 0.0)],
                         ids=["one-row", "one-column", "no-entries"])
def test_degenerate_shapes(shape, density):
    n, nf = shape
    A = _random_csr(n, nf, density, seed=41) if density else sp.csr_matrix(shape, dtype=np.float32)
    rng = np.random.default_rng(42)
    B, u, v = rng.standard_normal((nf, 7)).astype(np.float32), rng.standard_normal(n).astype(np.float32), \
        rng.standard_normal(7)
    csr = _device(A)
    want, scale = ref.spmm(*_host(csr), B, u, v, with_scale=True)
    got = _spmm(csr, B, u, v)
    _assert_within_bound(got, want, scale, "shape %s" % (shape,))
    if not density:
        assert csr.nnz == 0
        assert np.array_equal(got, (-np.outer(u.astype(np.float64), v)).astype(np.float32))     # C = -u v


def test_same_bits_on_two_calls(general):
    csr, B, u, v, _ = general
    assert np.array_equal(_spmm(csr, B[:, :200].copy(), u, v[:200]), _spmm(csr, B[:, :200].copy(), u, v[:200]))


def test_transposed_product(general):
    csr, _, _, _, _ = general
    t = csr.transpose().validate()
    A = sp.csr_matrix((csr.values.cpu().numpy(), csr.indices.cpu().numpy(), csr.indptr.cpu().numpy()), shape=csr.shape)
    At = A.T.tocsr()
    At.sort_indices()
    rng = np.random.default_rng(51)
    Q, mu, v = rng.standard_normal((300, 18)).astype(np.float32), rng.standard_normal(500).astype(np.float32), \
        rng.standard_normal(18)
    want, scale = ref.spmm(At.indptr, At.indices, At.data, Q, mu, v, with_scale=True)
    _assert_within_bound(_spmm(t, Q, mu, v), want, scale, "transpose")
    assert np.allclose(want, A.toarray().astype(np.float64).T @ Q - np.outer(mu, v), rtol=0, atol=1e-10)


@pytest.mark.parametrize("r", [0, 257])
def test_bad_width_is_an_error_and_nothing_is_written(general, r):
    csr = general[0]
    lib = _lib.load()
    width = max(r, 1)
    B = torch.zeros((500, width), device=DEV)
    C = torch.full((300, width), -7.0, device=DEV)
    work = torch.empty(1 << 20, dtype=torch.uint8, device=DEV)
    assert lib.mde_csr_spmm_work_bytes(csr.n, csr.nnz, r) == _lib.MDE_E_INVALID
    rc = lib.mde_csr_spmm(csr.n, csr.n_features, csr.nnz, _lib.ptr(csr.indptr), _lib.ptr(csr.indices),
                          _lib.ptr(csr.values), r, _lib.ptr(B), None, None, _lib.ptr(C), _lib.ptr(work),
                          _lib.stream_ptr(torch.device(DEV)))
    assert rc == _lib.MDE_E_INVALID and "r must lie in [1, 256]" in _lib.last_error()
    torch.cuda.synchronize()
    assert bool((C == -7.0).all())
    with pytest.raises(_lib.MdeHipError):
        sparse.spmm(csr, B if r else torch.zeros((500, 0), device=DEV))


def test_null_pointers_are_an_error(general):
    csr = general[0]
    lib = _lib.load()
    B = torch.zeros((500, 4), device=DEV)
    rc = lib.mde_csr_spmm(csr.n, csr.n_features, csr.nnz, _lib.ptr(csr.indptr), _lib.ptr(csr.indices),
                          _lib.ptr(csr.values), 4, _lib.ptr(B), None, None, None, None,
                          _lib.stream_ptr(torch.device(DEV)))
    assert rc == _lib.MDE_E_INVALID
    assert lib.mde_csr_spmm_work_bytes(-1, 0, 4) == _lib.MDE_E_INVALID
    assert isinstance(sparse.spmm_segment(), int) and sparse.spmm_segment() >= 64

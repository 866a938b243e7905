"""mde_pair_loss_cross_rows on the GPU: the rectangular walk over a list of query rows against mde_pair_loss_cross,
which is checked against the edge-list problem elsewhere.  At the same slice count the listed rows must hold the very
bits of the walk over all rows, and nothing else may be written."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
N_Q, N_C, NF = 150, 300, 20

_CACHE = {}


def _inputs(d):
    """Prepared float32 tensors on the GPU: Q [N_Q, NF], C [N_C, NF], Dm [N_Q, N_C], XQ [N_Q, d], XC [N_C, d]."""
    if d not in _CACHE:
        rng = np.random.default_rng(41 + d)
        rows = (rng.standard_normal((N_Q + N_C, NF)) * rng.uniform(0.5, 2.0, NF)).astype(np.float32)
        X = (rng.standard_normal((N_Q + N_C, d)) * 3.0).astype(np.float32)
        Q, C = rows[:N_Q], rows[N_Q:]
        Dm = np.sqrt(((Q.astype(np.float64)[:, None] - C.astype(np.float64)[None]) ** 2).sum(-1)).astype(np.float32)
        _CACHE[d] = tuple(torch.as_tensor(a).to(DEV).contiguous() for a in (Q, C, Dm, X[:N_Q], X[N_Q:]))
    return _CACHE[d]


def _spec():
    import pymde_amd
    from pymde_amd import dense
    return dense.loss_spec(pymde_amd.losses.Quadratic)


def _source(d, source):
    Q, C, Dm, XQ, XC = _inputs(d)
    return (XQ, XC), (dict(Q=Q, C=C) if source == "gram" else dict(Dm=Dm))


def _rows_call(d, source, slices, rows=None):
    """(row_loss, row_grad) of the list call into NaN-prefilled outputs."""
    from pymde_amd import rows as rows_module
    (XQ, XC), kw = _source(d, source)
    row_loss = torch.full((N_Q,), float("nan"), dtype=torch.float64, device=DEV)
    row_grad = torch.full((N_Q, d), float("nan"), dtype=torch.float32, device=DEV)
    rows_module.pair_loss_cross_rows(XQ, XC, _spec(), row_loss, row_grad, rows=rows, slices=slices, **kw)
    torch.cuda.synchronize()
    return row_loss, row_grad


@pytest.mark.parametrize("slices", [1, 3])
@pytest.mark.parametrize("source", ["gram", "matrix"])
@pytest.mark.parametrize("d", [2, 5])
def test_all_rows_equal_the_cross_walk(d, source, slices):
    from pymde_amd import dense
    (XQ, XC), kw = _source(d, source)
    _, grad, want_loss = dense._pair_loss_cross(XQ, XC, _spec(), slices=slices, **kw)
    row_loss, row_grad = _rows_call(d, source, slices)
    assert torch.equal(row_loss, want_loss)                     # the same sums in the same order
    want = grad.double() * N_Q                                  # grad = G / (n_q n_c), row_grad = G / n_c
    err = ((row_grad.double() - want).abs() / want.abs().clamp_min(1e-300)).max().item()
    print("d=%d %s slices=%d: row_grad against n_q * grad, worst rel. error %.3g (bound 2^-22 = %.3g)"
          % (d, source, slices, err, 2.0 ** -22))
    assert bool(torch.isfinite(row_grad).all())
    assert err <= 2.0 ** -22


@pytest.mark.parametrize("slices", [1, 3])
@pytest.mark.parametrize("source", ["gram", "matrix"])
@pytest.mark.parametrize("d", [2, 5])
def test_listed_rows_hold_the_bits_of_all_rows_and_the_others_are_not_written(d, source, slices):
    all_loss, all_grad = _rows_call(d, source, slices)
    rng = np.random.default_rng(7)
    for listed in (rng.permutation(N_Q)[:70], np.array([N_Q - 1])):        # shuffled, two blocks; a single row
        rows = torch.as_tensor(listed.astype(np.int32)).to(DEV)
        row_loss, row_grad = _rows_call(d, source, slices, rows=rows)
        mask = torch.zeros(N_Q, dtype=torch.bool, device=DEV)
        mask[rows.long()] = True
        assert torch.equal(row_loss[mask], all_loss[mask])
        assert torch.equal(row_grad[mask], all_grad[mask])
        assert bool(torch.isnan(row_loss[~mask]).all()) and bool(torch.isnan(row_grad[~mask]).all())


def test_bad_arguments_are_refused_on_the_host():
    from pymde_amd import _lib
    lib = _lib.load()
    Q, C, Dm, XQ, XC = _inputs(2)
    spec = _spec()
    row_loss = torch.zeros(N_Q, dtype=torch.float64, device=DEV)
    row_grad = torch.zeros((N_Q, 2), dtype=torch.float32, device=DEV)
    rows = torch.arange(10, dtype=torch.int32, device=DEV)
    work = torch.empty(int(lib.mde_pair_loss_cross_rows_work_bytes(N_Q, N_C, 2, 1)), dtype=torch.uint8, device=DEV)

    def call(n_rows, rows_arg):
        return lib.mde_pair_loss_cross_rows(N_Q, N_C, NF, _lib.ptr(Q), _lib.ptr(C), 0, None, 1.0, 2, _lib.ptr(XQ),
                                            _lib.ptr(XC), spec.kind, spec.scalars[0], spec.scalars[1],
                                            spec.scalars[2], 1, n_rows, _lib.ptr(rows_arg), _lib.ptr(row_loss),
                                            _lib.ptr(row_grad), _lib.ptr(work), _lib.stream_ptr(torch.device(DEV)))
    assert call(10, None) == _lib.MDE_E_INVALID                      # NULL means all rows
    assert call(0, rows) == _lib.MDE_E_INVALID
    assert call(-1, rows) == _lib.MDE_E_INVALID
    assert call(N_Q + 1, rows) == _lib.MDE_E_INVALID
    assert "mde_pair_loss_cross_rows" in _lib.last_error()
    assert call(10, rows) == 0 and call(N_Q, None) == 0
    torch.cuda.synchronize()

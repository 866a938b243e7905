"""mde_pair_loss on the GPU (csrc/mde_pair_loss.hip): the loss, gradient and per-row loss of a dense MDE problem, through
the thin wrapper pymde_amd.dense._pair_loss.

The reference is the CPU oracle's edge-order average distortion over all_edges(n) with float64 numpy deviations
rounded once to float32.  The data are integer grids, so every squared data distance is exact in float32 and the
kernel's D is that rounding bit for bit: the comparison isolates the new arithmetic (E from differences, the loss,
the double sums).  The shapes are the smallest that reach every branch: one pair, one full tile, partial row and
column tiles (193), one row in the last tile (257), partial and multiple feature chunks (37, 70), every compile-time
variant of the embedding dimension (1, 2, 3, and 8 for 4 .. 8), empty slices (40 slices of 5 column tiles).
Tolerances: LOSS_RTOL and assert_grad_close of tests/conftest.py."""
import numpy as np
import pytest
import torch

from conftest import GRAD_ATOL_REL, GRAD_RTOL, LOSS_RTOL, assert_grad_close

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


def _edges(n):
    iu, ju = np.triu_indices(n, 1)
    return np.stack([iu, ju], 1).astype(np.int64)


def _spec(kind, scalars=(), weighted=False):
    from pymde_amd import dense
    from pymde_amd.functions.function import KIND
    return dense.LossSpec(KIND[kind], tuple(scalars) + (0.0,) * (3 - len(scalars)), weighted)


def _oracle(X, D, kind, scalars=(), weighted=False):
    """(loss, grad [n, d], row_loss [n]) of the oracle over all pairs; D float64 [n, n], rounded once to float32."""
    from oracle import oracle
    n = X.shape[0]
    edges = _edges(n)
    dev64 = D[edges[:, 0], edges[:, 1]]
    a0 = dev64.astype(np.float32)
    with np.errstate(divide="ignore"):
        a1 = (1.0 / dev64 ** 2).astype(np.float32) if weighted else None
    fd = oracle.func(kind, a0, a1, scalars)
    loss, grad = oracle.average_distortion(edges, X, fd)
    per_edge = oracle.distortions(oracle.distances(edges, X), fd).astype(np.float64)
    rows = np.zeros(n)
    np.add.at(rows, edges[:, 0], per_edge)
    np.add.at(rows, edges[:, 1], per_edge)
    return loss, grad, rows


def _run(X, spec, A=None, Dm=None, mode=0, d_scale=1.0, slices=1, raw=False):
    from pymde_amd import dense
    out = dense._pair_loss(_dev(X, torch.float32), spec, A=None if A is None else _dev(A, torch.float32), mode=mode,
                           Dm=None if Dm is None else _dev(Dm, torch.float32), d_scale=d_scale, slices=slices)
    torch.cuda.synchronize()
    if raw:
        return out
    return float(out[0].item()), out[1].cpu().numpy(), out[2].cpu().numpy()


def _compare(label, got, want, rows=True):
    """Prints the worst error of the value, the gradient (as a fraction of its allowance) and the row losses next to
    each bound, then asserts."""
    loss, grad, row_loss = got
    wloss, wgrad, wrows = want
    e_loss = abs(loss - wloss) / abs(wloss) if wloss != 0 else abs(loss)
    allow = GRAD_ATOL_REL * max(float(np.abs(wgrad).max()), 1e-30) + GRAD_RTOL * np.abs(wgrad.astype(np.float64))
    e_grad = float((np.abs(grad.astype(np.float64) - wgrad) / allow).max())
    e_rows = float((np.abs(row_loss - wrows) / np.where(wrows == 0, 1.0, np.abs(wrows))).max())
    print("%s: value rel. error %.3g (bound %.3g); gradient error %.3g of its allowance (rtol %.3g, atol %.3g max|g|); "
          "row loss rel. error %.3g (bound %.3g)" % (label, e_loss, LOSS_RTOL, e_grad, GRAD_RTOL, GRAD_ATOL_REL, e_rows,
                                                    LOSS_RTOL))
    assert np.isfinite(loss) and np.isfinite(grad).all() and np.isfinite(row_loss).all()
    assert e_loss <= LOSS_RTOL
    assert_grad_close(grad, wgrad)
    if rows:
        assert e_rows <= LOSS_RTOL
    return e_loss, e_grad, e_rows


_CACHE = {}


def _cached(key, make):
    """Inputs and references are computed once per module and shared (never modified)."""
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _grid_case(n, nf, d):
    """(A integer grid [n, nf] float32, X centred Gaussian [n, d] float32 at the scale of the data distances,
    D float64 [n, n])."""
    def make():
        rng = np.random.default_rng(1000 * n + 10 * nf + d)
        A = rng.integers(-3, 4, (n, nf)).astype(np.float32)
        if n == 2:
            A[1] = A[0] + 2.0
        D = _dist64(A)
        X = rng.standard_normal((n, d)) * (D.mean() / np.sqrt(2.0 * d))
        return A, (X - X.mean(0)).astype(np.float32), D
    return _cached(("grid", n, nf, d), make)


# ---------------------------------------------------------------- 1. shapes, both sources
SHAPES = [(2, 1, 1, 1), (64, 37, 2, 1), (64, 37, 1, 3), (193, 37, 2, 1), (193, 37, 2, 3), (193, 70, 5, 3),
          (193, 37, 8, 1), (257, 70, 3, 1), (257, 70, 3, 40), (257, 37, 2, 40)]


@pytest.mark.parametrize("n,nf,d,slices", SHAPES)
def test_shapes_from_both_sources(n, nf, d, slices):
    A, X, D = _grid_case(n, nf, d)
    want = _cached(("quad", n, nf, d), lambda: _oracle(X, D, "L_QUADRATIC"))
    spec = _spec("L_QUADRATIC")
    _compare("gram %dx%d d=%d slices=%d" % (n, nf, d, slices), _run(X, spec, A=A, slices=slices), want)
    _compare("matrix %d d=%d slices=%d" % (n, d, slices), _run(X, spec, Dm=D.astype(np.float32), slices=slices), want)


def test_automatic_slices():
    A, X, D = _grid_case(257, 70, 3)
    want = _cached(("quad", 257, 70, 3), lambda: _oracle(X, D, "L_QUADRATIC"))
    _compare("gram 257x70 d=3 slices=0", _run(X, _spec("L_QUADRATIC"), A=A, slices=0), want)


# ---------------------------------------------------------------- 2. every public loss
def _loss_cases():
    import functools
    from pymde_amd import losses
    return {
        "Quadratic": (losses.Quadratic, "L_QUADRATIC", ()),
        "WeightedQuadratic": (losses.WeightedQuadratic, "L_WEIGHTED_QUADRATIC", ()),
        "Huber": (functools.partial(losses.Huber, threshold=3.0), "L_HUBER", (3.0,)),
        "Cubic": (losses.Cubic, "L_CUBIC", ()),
        "Power1.5": (functools.partial(losses.Power, exponent=1.5), "L_POWER", (1.5,)),
        "Power2.5": (functools.partial(losses.Power, exponent=2.5), "L_POWER", (2.5,)),
        "Absolute": (losses.Absolute, "L_ABSOLUTE", ()),
        "Logistic": (losses.Logistic, "L_LOGISTIC", ()),
        "Fractional": (losses.Fractional, "L_FRACTIONAL", ()),
        "SoftFractional": (losses.SoftFractional, "L_SOFT_FRACTIONAL", (10.0,)),
    }


@pytest.mark.parametrize("name", ["Quadratic", "WeightedQuadratic", "Huber", "Cubic", "Power1.5", "Power2.5", "Absolute",
                                  "Logistic", "Fractional", "SoftFractional"])
def test_every_public_loss(name):
    from pymde_amd import dense
    make, kind, scalars = _loss_cases()[name]
    spec = dense.loss_spec(make)
    assert spec == _spec(kind, scalars, weighted=name.startswith("Weighted"))
    A, X, D = _grid_case(193, 37, 2)
    assert D[~np.eye(193, dtype=bool)].min() >= 1.0            # no duplicate rows: every deviation is positive
    if name == "Huber":
        r = np.abs(D - _dist64(X))[~np.eye(193, dtype=bool)]
        assert (r < 3.0).mean() > 0.05 and (r > 3.0).mean() > 0.05      # both branches
    want = _oracle(X, D, kind, scalars, spec.weighted)
    _compare("%s gram" % name, _run(X, spec, A=A), want)
    _compare("%s matrix" % name, _run(X, spec, Dm=D.astype(np.float32), slices=3), want)


# ---------------------------------------------------------------- 3. d_scale and mode 1
def test_d_scale():
    A, X, D = _grid_case(193, 37, 2)
    for name, kind in (("Quadratic", "L_QUADRATIC"), ("Absolute", "L_ABSOLUTE")):
        want = _oracle(X, 0.375 * D, kind)
        _compare("%s d_scale=0.375 gram" % name, _run(X, _spec(kind), A=A, d_scale=0.375), want)
        _compare("%s d_scale=0.375 matrix" % name, _run(X, _spec(kind), Dm=D.astype(np.float32), d_scale=0.375), want)
    plain = _cached(("quad", 193, 37, 2), lambda: _oracle(X, D, "L_QUADRATIC"))
    assert abs(want[0] - plain[0]) > 0.1 * abs(plain[0])        # the scale matters


def test_mode_1_is_half_the_squared_distance():
    A, X, _ = _grid_case(193, 37, 2)
    H = _dist64(A, mode=1)                                      # integers and halves: exact in float32
    Xs = (X * (H.mean() / _dist64(A).mean())).astype(np.float32)
    for kind in ("L_QUADRATIC", "L_ABSOLUTE"):
        _compare("%s mode 1" % kind, _run(Xs, _spec(kind), A=A, mode=1, slices=3), _oracle(Xs, H, kind))


# ---------------------------------------------------------------- 4. degenerate pairs
@pytest.mark.parametrize("kind", ["L_QUADRATIC", "L_ABSOLUTE"])
def test_zero_deviations_and_coincident_embedding_rows(kind):
    """200 rows with 81 distinct data rows (D = 0 pairs), and an embedding whose rows 30 .. 49 coincide (E = 0, where
    l'(E) / E is infinite or NaN and the reference's rule makes it 1, times a zero difference)."""
    def make():
        rng = np.random.default_rng(5)
        A = rng.integers(0, 3, (200, 4)).astype(np.float32)
        X = rng.standard_normal((200, 2)).astype(np.float32)
        X[30:50] = X[30]
        return A, X, _dist64(A)
    A, X, D = _cached("degenerate", make)
    off = ~np.eye(200, dtype=bool)
    assert (D[off] == 0).sum() > 0 and (_dist64(X)[off] == 0).sum() == 20 * 19
    want = _oracle(X, D, kind)
    for slices in (1, 3):
        _compare("%s degenerate gram slices=%d" % (kind, slices), _run(X, _spec(kind), A=A, slices=slices), want)
        _compare("%s degenerate matrix slices=%d" % (kind, slices),
                 _run(X, _spec(kind), Dm=D.astype(np.float32), slices=slices), want)


def test_self_exclusion_follows_the_index():
    """Row 7 is a copy of row 150 in both spaces: the pair (7, 150) counts (D = E = 0), the pair (7, 7) does not."""
    A, X, _ = (v.copy() for v in _grid_case(193, 37, 2))
    A[7], X[7] = A[150], X[150]
    D = _dist64(A)
    want = _oracle(X, D, "L_ABSOLUTE")
    _compare("twin rows", _run(X, _spec("L_ABSOLUTE"), A=A), want)
    # a matrix source whose diagonal is poisoned gives the same bits: the diagonal is never used
    Dm = D.astype(np.float32)
    clean = _run(X, _spec("L_ABSOLUTE"), Dm=Dm, raw=True)
    np.fill_diagonal(Dm, np.nan)
    dirty = _run(X, _spec("L_ABSOLUTE"), Dm=Dm, raw=True)
    assert all(torch.equal(a, b) for a, b in zip(clean, dirty))


# ---------------------------------------------------------------- 5. determinism
def test_two_runs_give_the_same_bits():
    A, X, D = _grid_case(257, 70, 3)
    spec = _spec("L_QUADRATIC")
    by_slices = {}
    for slices in (1, 3):
        for source in (dict(A=A), dict(Dm=D.astype(np.float32))):
            first = _run(X, spec, slices=slices, raw=True, **source)
            again = _run(X, spec, slices=slices, raw=True, **source)
            assert all(torch.equal(a, b) for a, b in zip(first, again))
        by_slices[slices] = (float(first[0].item()), first[1].cpu().numpy(), first[2].cpu().numpy())
    _compare("slices 3 against slices 1", by_slices[3], by_slices[1])


# ---------------------------------------------------------------- 6. the C ABI refuses and launches nothing
def test_invalid_arguments_launch_nothing():
    from pymde_amd import _lib
    from pymde_amd.functions.function import KIND
    lib = _lib.load()
    n, nf, d = 100, 5, 2
    A = _dev(np.random.default_rng(0).standard_normal((n, nf)).astype(np.float32))
    Dm = _dev(np.ones((n, n), dtype=np.float32))
    X = _dev(np.random.default_rng(1).standard_normal((n, 8)).astype(np.float32))
    loss = torch.full((1,), -7.0, dtype=torch.float64, device=DEV)
    grad = torch.full((n, 8), -7.0, dtype=torch.float32, device=DEV)
    rows = torch.full((n,), -7.0, dtype=torch.float64, device=DEV)
    work = torch.full((1 << 20,), 0x5A, dtype=torch.uint8, device=DEV)
    p, st = _lib.ptr, _lib.stream_ptr()
    quad = KIND["L_QUADRATIC"]

    def call(n_=n, nf_=nf, A_=A, mode=0, Dm_=None, scale=1.0, d_=d, X_=X, kind=quad, slices=1, loss_=loss, grad_=grad,
             rows_=rows, work_=work):
        return lib.mde_pair_loss(n_, nf_, p(A_), mode, p(Dm_), scale, d_, p(X_), kind, 0.0, 0.0, 0.0, slices, p(loss_),
                                 p(grad_), p(rows_), p(work_), st)
    bad = [call(d_=0), call(d_=9), call(d_=-1), call(kind=KIND["QUADRATIC"]), call(kind=KIND["LOG1P"]), call(kind=0),
           call(kind=44), call(scale=0.0), call(scale=-1.0), call(scale=float("inf")), call(scale=float("nan")),
           call(A_=None), call(Dm_=Dm), call(X_=None), call(loss_=None), call(grad_=None), call(rows_=None),
           call(work_=None), call(slices=-1), call(slices=65536), call(n_=1), call(n_=0), call(n_=2 ** 31),
           call(nf_=0), call(mode=2), call(mode=-1)]
    assert bad == [_lib.MDE_E_INVALID] * len(bad)
    assert "mde_pair_loss" in _lib.last_error()
    for args in ((1, 2, 1), (n, 0, 1), (n, 9, 1), (2 ** 31, 2, 1), (n, 2, -1), (n, 2, 65536)):
        assert lib.mde_pair_loss_work_bytes(*args) == _lib.MDE_E_INVALID
    assert "mde_pair_loss_work_bytes" in _lib.last_error()
    torch.cuda.synchronize()
    assert (loss == -7).all() and (grad == -7).all() and (rows == -7).all()
    assert (work == 0x5A).all()                                 # not even the row norms
    # and the same call with valid arguments runs, from either source and at the largest dimension
    assert lib.mde_pair_loss_work_bytes(n, d, 3) == 3 * n * (1 + d) * 8 + 4 * n
    assert call(slices=3) == _lib.MDE_OK and call(A_=None, Dm_=Dm, nf_=0, d_=8) == _lib.MDE_OK
    torch.cuda.synchronize()
    assert torch.isfinite(loss).all() and torch.isfinite(grad).all() and (rows >= 0).all()

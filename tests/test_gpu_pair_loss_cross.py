"""mde_pair_loss_cross on the GPU (csrc/mde_pair_loss.hip): the loss, the gradient of the query rows
and the per-row loss of the rectangular dense problem, through the thin wrapper pymde_amd.dense._pair_loss_cross.

The reference is the CPU oracle's edge-order average distortion over the bipartite edge list {(j, n_c + i)} on the
stacked [XC; XQ], with float64 numpy deviations rounded once to float32: its mean over the n_q n_c edges and the rows
[n_c:] of its gradient are what the kernel defines.  The data are integer grids in [-3, 3], so every squared data
distance is exact in float32 and the kernel's D is that rounding bit for bit.  The shapes are the smallest that reach
every branch: one pair, a single query row, a single corpus row, one full tile, one row in the last row tile with a
partial column tile, several feature chunks with d in 4 .. 8, more slices than column tiles, automatic slices.
Tolerances: LOSS_RTOL and assert_grad_close of tests/conftest.py.  Helpers and the loss table: test_gpu_pair_loss."""
import numpy as np
import pytest
import torch

from conftest import GRAD_ATOL_REL, GRAD_RTOL, LOSS_RTOL, assert_grad_close
from test_gpu_pair_loss import _dev, _loss_cases, _spec

pytestmark = pytest.mark.gpu
DEV = "cuda"
FLT_MAX = float(np.finfo(np.float32).max)


# ---------------------------------------------------------------- helpers
def _cross64(Q, C, mode=0):
    """Dense float64 distances [n_q, n_c] of the rows of Q to the rows of C: Euclidean (mode 0) or half the squared
    distance (mode 1)."""
    Q, C = np.asarray(Q, dtype=np.float64), np.asarray(C, dtype=np.float64)
    d2 = np.empty((Q.shape[0], C.shape[0]))
    for i in range(0, Q.shape[0], 16):
        d2[i:i + 16] = ((Q[i:i + 16, None, :] - C[None, :, :]) ** 2).sum(-1)
    return 0.5 * d2 if mode else np.sqrt(d2)


def _oracle(XQ, XC, D, kind, scalars=(), weighted=False, skip=None):
    """(loss, grad [n_q, d], row_loss [n_q]) of the oracle over the bipartite pairs; D float64 [n_q, n_c], rounded once
    to float32.  `skip`: one (i, j) left out of the edge list; the mean is still over n_q n_c."""
    from oracle import oracle
    n_q, n_c = D.shape
    i, j = np.divmod(np.arange(n_q * n_c, dtype=np.int64), n_c)
    if skip is not None:
        keep = ~((i == skip[0]) & (j == skip[1]))
        i, j = i[keep], j[keep]
    edges = np.stack([j, n_c + i], 1)
    dev64 = D[i, j]
    a0 = dev64.astype(np.float32)
    with np.errstate(divide="ignore"):
        a1 = (1.0 / dev64 ** 2).astype(np.float32) if weighted else None
    fd = oracle.func(kind, a0, a1, scalars)
    X = np.ascontiguousarray(np.concatenate([XC, XQ]).astype(np.float32))
    loss, grad = oracle.average_distortion(edges, X, fd)
    per_edge = oracle.distortions(oracle.distances(edges, X), fd).astype(np.float64)
    rows = np.zeros(n_q)
    np.add.at(rows, i, per_edge)
    factor = len(i) / float(n_q * n_c)
    return loss * factor, np.asarray(grad)[n_c:] * factor, rows


def _run(XQ, XC, spec, Q=None, C=None, Dm=None, mode=0, d_scale=1.0, slices=1, raw=False):
    from pymde_amd import dense
    f32 = torch.float32
    out = dense._pair_loss_cross(_dev(XQ, f32), _dev(XC, f32), spec, Q=None if Q is None else _dev(Q, f32),
                                 C=None if C is None else _dev(C, f32), mode=mode,
                                 Dm=None if Dm is None else _dev(Dm, f32), d_scale=d_scale, slices=slices)
    torch.cuda.synchronize()
    if raw:
        return out
    return float(out[0].item()), out[1].cpu().numpy(), out[2].cpu().numpy()


def _compare(label, got, want):
    """Prints the worst error of the value, the gradient (as a fraction of its allowance) and the row losses next to
    each bound, then asserts.

    A row loss is held to LOSS_RTOL of itself or of the mean row loss, whichever is larger.  A row of the rectangular
    problem may hold a single pair (n_c = 1), and one float32 term l(E, D) is not accurate to a relative bound: the
    kernel and the oracle round E = |xq - xc| in different orders, E carries a relative 6e-8, and l = (E - D)^2 turns
    that into 2 * 6e-8 * E / |E - D| of itself, which has no bound as E -> D.  In absolute terms the error of a term is
    about 1.2e-7 E |E - D|, some 1e-6 of a typical term of these cases (E, D and |E - D| are of one scale), so it
    stays well inside 1e-5 of the mean row."""
    loss, grad, row_loss = got
    wloss, wgrad, wrows = want
    e_loss = abs(loss - wloss) / abs(wloss) if wloss != 0 else abs(loss)
    allow = GRAD_ATOL_REL * max(float(np.abs(wgrad).max()), 1e-30) + GRAD_RTOL * np.abs(wgrad.astype(np.float64))
    e_grad = float((np.abs(grad.astype(np.float64) - wgrad) / allow).max())
    floor = float(np.abs(wrows).mean())
    e_rows = float((np.abs(row_loss - wrows) / np.maximum(np.maximum(np.abs(wrows), floor), 1e-300)).max())
    print("%s: value rel. error %.3g (bound %.3g); gradient error %.3g of its allowance (rtol %.3g, atol %.3g max|g|); "
          "row loss rel. error %.3g (bound %.3g)" % (label, e_loss, LOSS_RTOL, e_grad, GRAD_RTOL, GRAD_ATOL_REL, e_rows,
                                                    LOSS_RTOL))
    assert np.isfinite(loss) and np.isfinite(grad).all() and np.isfinite(row_loss).all()
    assert e_loss <= LOSS_RTOL
    assert_grad_close(grad, wgrad)
    assert e_rows <= LOSS_RTOL


_CACHE = {}


def _cached(key, make):
    """Inputs and references are computed once per module and shared (never modified)."""
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _grid_case(n_q, n_c, nf, d):
    """(Q [n_q, nf], C [n_c, nf] integer grids float32, XQ [n_q, d], XC [n_c, d] Gaussian float32 at the scale of the
    data distances, D float64 [n_q, n_c])."""
    def make():
        rng = np.random.default_rng(100000 * n_q + 100 * n_c + 10 * nf + d)
        Q = rng.integers(-3, 4, (n_q, nf)).astype(np.float32)
        C = rng.integers(-3, 4, (n_c, nf)).astype(np.float32)
        if n_q == 1 and n_c == 1:
            Q[0] = C[0] + 2.0
        D = _cross64(Q, C)
        scale = D.mean() / np.sqrt(2.0 * d)
        XQ = (rng.standard_normal((n_q, d)) * scale).astype(np.float32)
        XC = (rng.standard_normal((n_c, d)) * scale).astype(np.float32)
        return Q, C, XQ, XC, D
    return _cached(("grid", n_q, n_c, nf, d), make)


# ---------------------------------------------------------------- 1. shapes, both sources
SHAPES = [(1, 1, 1, 1, 1), (1, 193, 37, 2, 1), (193, 1, 37, 2, 1), (64, 64, 37, 3, 1), (65, 193, 37, 2, 3),
          (193, 65, 70, 5, 1), (257, 193, 70, 8, 40), (193, 257, 37, 1, 0)]


@pytest.mark.parametrize("n_q,n_c,nf,d,slices", SHAPES)
def test_shapes_from_both_sources(n_q, n_c, nf, d, slices):
    Q, C, XQ, XC, D = _grid_case(n_q, n_c, nf, d)
    want = _oracle(XQ, XC, D, "L_QUADRATIC")
    spec = _spec("L_QUADRATIC")
    label = "%dx%d nf=%d d=%d slices=%d" % (n_q, n_c, nf, d, slices)
    _compare("gram " + label, _run(XQ, XC, spec, Q=Q, C=C, slices=slices), want)
    _compare("matrix " + label, _run(XQ, XC, spec, Dm=D.astype(np.float32), slices=slices), want)


# ---------------------------------------------------------------- 2. every public loss
@pytest.mark.parametrize("name", ["Quadratic", "WeightedQuadratic", "Huber", "Cubic", "Power1.5", "Power2.5", "Absolute",
                                  "Logistic", "Fractional", "SoftFractional"])
def test_every_public_loss(name):
    from pymde_amd import dense
    make, kind, scalars = _loss_cases()[name]
    spec = dense.loss_spec(make)
    assert spec == _spec(kind, scalars, weighted=name.startswith("Weighted"))
    Q, C, XQ, XC, D = _grid_case(193, 257, 37, 2)
    assert D.min() >= 1.0                       # no grid row of Q equals a row of C: every deviation is positive
    if name == "Huber":
        r = np.abs(D - _cross64(XQ, XC))
        assert (r < 3.0).mean() > 0.05 and (r > 3.0).mean() > 0.05      # both branches
    want = _oracle(XQ, XC, D, kind, scalars, spec.weighted)
    _compare("%s gram" % name, _run(XQ, XC, spec, Q=Q, C=C), want)
    _compare("%s matrix" % name, _run(XQ, XC, spec, Dm=D.astype(np.float32), slices=3), want)


# ---------------------------------------------------------------- 3. d_scale and mode 1
def test_d_scale():
    Q, C, XQ, XC, D = _grid_case(193, 257, 37, 2)
    for name, kind in (("Quadratic", "L_QUADRATIC"), ("Absolute", "L_ABSOLUTE")):
        want = _oracle(XQ, XC, 0.375 * D, kind)
        _compare("%s d_scale=0.375 gram" % name, _run(XQ, XC, _spec(kind), Q=Q, C=C, d_scale=0.375), want)
        _compare("%s d_scale=0.375 matrix" % name,
                 _run(XQ, XC, _spec(kind), Dm=D.astype(np.float32), d_scale=0.375), want)
    plain = _oracle(XQ, XC, D, "L_ABSOLUTE")
    assert abs(want[0] - plain[0]) > 0.1 * abs(plain[0])        # the scale matters


def test_mode_1_is_half_the_squared_distance():
    Q, C, XQ, XC, D = _grid_case(193, 257, 37, 2)
    H = _cross64(Q, C, mode=1)                                  # integers and halves: exact in float32
    s = H.mean() / D.mean()
    XQs, XCs = (XQ * s).astype(np.float32), (XC * s).astype(np.float32)
    for kind in ("L_QUADRATIC", "L_ABSOLUTE"):
        _compare("%s mode 1" % kind, _run(XQs, XCs, _spec(kind), Q=Q, C=C, mode=1, slices=3),
                 _oracle(XQs, XCs, H, kind))


# ---------------------------------------------------------------- 4. nothing is "self"
@pytest.mark.parametrize("kind", ["L_QUADRATIC", "L_ABSOLUTE"])
def test_twin_rows_are_an_ordinary_pair(kind):
    """Query row 7 is a copy of corpus row 150 in both spaces: the pair counts, with D = E = 0, where l'(E) / E is
    infinite or NaN and the reference's rule makes it 1, times a zero difference."""
    Q, C, XQ, XC, _ = (v.copy() for v in _grid_case(193, 257, 37, 2))
    Q[7], XQ[7] = C[150], XC[150]
    D = _cross64(Q, C)
    assert D[7, 150] == 0 and (D == 0).sum() == 1
    want = _oracle(XQ, XC, D, kind)
    for slices in (1, 3):
        _compare("%s twin gram slices=%d" % (kind, slices), _run(XQ, XC, _spec(kind), Q=Q, C=C, slices=slices), want)
        _compare("%s twin matrix slices=%d" % (kind, slices),
                 _run(XQ, XC, _spec(kind), Dm=D.astype(np.float32), slices=slices), want)


@pytest.mark.parametrize("kind", ["L_QUADRATIC", "L_ABSOLUTE"])
@pytest.mark.parametrize("slices", [1, 3])
def test_tie_to_the_square_kernel(kind, slices):
    """Q = C = A and XQ = XC = X: the diagonal pair has D = E = 0 exactly and adds +0.0 in double, so the row losses
    are those of mde_pair_loss bit for bit; the gradients differ by the divisor, n^2 against n (n - 1) / 2."""
    from pymde_amd import dense
    from test_gpu_pair_loss import _grid_case as square_case
    A, X, _ = square_case(193, 37, 2)
    n = A.shape[0]
    f32 = torch.float32
    square = dense._pair_loss(_dev(X, f32), _spec(kind), A=_dev(A, f32), slices=slices)
    cross = _run(X, X, _spec(kind), Q=A, C=A, slices=slices, raw=True)
    torch.cuda.synchronize()
    assert torch.equal(cross[2], square[2])
    scaled = cross[1].cpu().numpy().astype(np.float64) * (float(n) * n / (n * (n - 1) / 2.0))
    wgrad = square[1].cpu().numpy()
    allow = GRAD_ATOL_REL * float(np.abs(wgrad).max()) + GRAD_RTOL * np.abs(wgrad.astype(np.float64))
    print("%s slices=%d: row losses equal; gradient error %.3g of its allowance"
          % (kind, slices, float((np.abs(scaled - wgrad) / allow).max())))
    assert_grad_close(scaled, wgrad)
    # the value: every pair is in two rows of the square problem and the diagonal adds nothing
    assert abs(float(cross[0]) * n * n - float(square[0]) * n * (n - 1)) <= LOSS_RTOL * float(square[0]) * n * (n - 1)


def test_a_flt_max_entry_of_the_matrix_is_skipped():
    Q, C, XQ, XC, D = _grid_case(65, 193, 37, 2)
    Dm = D.astype(np.float32)
    Dm[64, 130] = FLT_MAX
    for kind in ("L_QUADRATIC", "L_ABSOLUTE"):
        want = _oracle(XQ, XC, D, kind, skip=(64, 130))
        full = _oracle(XQ, XC, D, kind)
        assert abs(want[2][64] - full[2][64]) > 10.0 * LOSS_RTOL * full[2][64]       # the check would see the pair
        _compare("%s FLT_MAX entry" % kind, _run(XQ, XC, _spec(kind), Dm=Dm, slices=3), want)


# ---------------------------------------------------------------- 5. determinism
def test_two_runs_give_the_same_bits():
    Q, C, XQ, XC, D = _grid_case(257, 193, 70, 8)
    spec = _spec("L_QUADRATIC")
    by_slices = {}
    for slices in (1, 3):
        for source in (dict(Q=Q, C=C), dict(Dm=D.astype(np.float32))):
            first = _run(XQ, XC, spec, slices=slices, raw=True, **source)
            again = _run(XQ, XC, spec, slices=slices, raw=True, **source)
            assert all(torch.equal(a, b) for a, b in zip(first, again))
        by_slices[slices] = (float(first[0].item()), first[1].cpu().numpy(), first[2].cpu().numpy())
    _compare("slices 3 against slices 1", by_slices[3], by_slices[1])


# ---------------------------------------------------------------- 6. the C ABI refuses and launches nothing
def test_invalid_arguments_launch_nothing():
    from pymde_amd import _lib
    from pymde_amd.functions.function import KIND
    lib = _lib.load()
    n_q, n_c, nf, d = 100, 70, 5, 2
    rng = np.random.default_rng(0)
    Q = _dev(rng.standard_normal((n_q, nf)).astype(np.float32))
    C = _dev(rng.standard_normal((n_c, nf)).astype(np.float32))
    Dm = _dev(np.ones((n_q, n_c), dtype=np.float32))
    XQ = _dev(rng.standard_normal((n_q, 8)).astype(np.float32))
    XC = _dev(rng.standard_normal((n_c, 8)).astype(np.float32))
    loss = torch.full((1,), -7.0, dtype=torch.float64, device=DEV)
    grad = torch.full((n_q, 8), -7.0, dtype=torch.float32, device=DEV)
    rows = torch.full((n_q,), -7.0, dtype=torch.float64, device=DEV)
    work = torch.full((1 << 20,), 0x5A, dtype=torch.uint8, device=DEV)
    p, st = _lib.ptr, _lib.stream_ptr()
    quad = KIND["L_QUADRATIC"]

    def call(nq_=n_q, nc_=n_c, nf_=nf, Q_=Q, C_=C, mode=0, Dm_=None, scale=1.0, d_=d, XQ_=XQ, XC_=XC, kind=quad,
             slices=1, loss_=loss, grad_=grad, rows_=rows, work_=work):
        return lib.mde_pair_loss_cross(nq_, nc_, nf_, p(Q_), p(C_), mode, p(Dm_), scale, d_, p(XQ_), p(XC_), kind, 0.0,
                                       0.0, 0.0, slices, p(loss_), p(grad_), p(rows_), p(work_), st)
    bad = [call(d_=0), call(d_=9), call(d_=-1), call(kind=KIND["QUADRATIC"]), call(kind=KIND["LOG1P"]), call(kind=0),
           call(kind=44), call(scale=0.0), call(scale=-1.0), call(scale=float("inf")), call(scale=float("nan")),
           call(Q_=None), call(C_=None), call(Q_=None, C_=None), call(Dm_=Dm), call(Q_=None, Dm_=Dm),
           call(C_=None, Dm_=Dm), call(XQ_=None), call(XC_=None), call(loss_=None), call(grad_=None),
           call(rows_=None), call(work_=None), call(slices=-1), call(slices=65536), call(nq_=0), call(nc_=0),
           call(nq_=-1), call(nc_=-1), call(nq_=2 ** 31), call(nc_=2 ** 31), call(nf_=0), call(mode=2), call(mode=-1)]
    assert bad == [_lib.MDE_E_INVALID] * len(bad)
    assert "mde_pair_loss_cross:" in _lib.last_error()
    for args in ((0, n_c, 2, 1), (n_q, 0, 2, 1), (n_q, n_c, 0, 1), (n_q, n_c, 9, 1), (2 ** 31, n_c, 2, 1),
                 (n_q, 2 ** 31, 2, 1), (n_q, n_c, 2, -1), (n_q, n_c, 2, 65536)):
        assert lib.mde_pair_loss_cross_work_bytes(*args) == _lib.MDE_E_INVALID
    assert "mde_pair_loss_cross_work_bytes" in _lib.last_error()
    torch.cuda.synchronize()
    assert (loss == -7).all() and (grad == -7).all() and (rows == -7).all()
    assert (work == 0x5A).all()                                 # not even the row norms
    # and the same call with valid arguments runs, from either source and at the largest dimension
    assert lib.mde_pair_loss_cross_work_bytes(n_q, n_c, d, 3) == 3 * n_q * (1 + d) * 8 + 4 * (n_q + n_c)
    assert lib.mde_pair_loss_cross_work_bytes(1, 1, 8, 1) == 1 * 1 * 9 * 8 + 4 * 2
    assert call(slices=3) == _lib.MDE_OK and call(Q_=None, C_=None, Dm_=Dm, nf_=0, d_=8) == _lib.MDE_OK
    torch.cuda.synchronize()
    assert torch.isfinite(loss).all() and torch.isfinite(grad).all() and (rows >= 0).all()

"""Per-pair weights and missing pairs in the dense walk (csrc/mde_pair_loss.hip): the three
*_weighted entry points through the thin wrappers of pymde_amd.dense / pymde_amd.rows, and mde_pair_weights_check.

The reference is the CPU oracle over an edge list, as in test_gpu_pair_loss.py, whose helpers and integer grids these
tests share (D is exact in float32, so the comparison isolates the new arithmetic).  The loss is linear in the
weights: for a matrix drawn from {0, 0.5, 2, 3} the expected value, row losses and gradient are the float64
combination, weight value by weight value, of oracle evaluations over the edges that carry that value (for the weighted
kinds with a1 = 1), divided by the number of kept pairs.  Continuous weights are checked on the weighted kinds, where
the oracle takes them as a1; the power form against a1 = float32(D64^-p).  Shapes: one pair, one full tile, partial
row and column tiles (193), one row in the last tile and empty slices (257, 40 slices), d = 1, 2, 3, 5, 8.
Tolerances: LOSS_RTOL and assert_grad_close of tests/conftest.py."""
import numpy as np
import pytest
import torch

from test_gpu_pair_loss import _compare, _dev, _grid_case, _loss_cases, _spec
from test_gpu_pair_loss_cross import _compare as _compare_cross
from test_gpu_pair_loss_cross import _grid_case as _cross_case

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32 = torch.float32
VALUES = (0.0, 0.5, 2.0, 3.0)
_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


# ---------------------------------------------------------------- helpers
def _weights(source, p=0.0, W=None):
    from pymde_amd import dense
    return dense.Weights(source, float(p), None if W is None else _dev(W, F32))


def _power(p):
    from pymde_amd import dense
    return _weights(dense.W_POWER, p)


def _matrix(W):
    from pymde_amd import dense
    return _weights(dense.W_MATRIX, 0.0, W)


def _run(X, spec, weights, pairs=None, A=None, Dm=None, slices=1, raw=False):
    from pymde_amd import dense
    out = dense._pair_loss(_dev(X, F32), spec, A=None if A is None else _dev(A, F32),
                           Dm=None if Dm is None else _dev(Dm, F32), slices=slices, weights=weights, pairs=pairs)
    torch.cuda.synchronize()
    if raw:
        return out
    return float(out[0].item()), out[1].cpu().numpy(), out[2].cpu().numpy()


def _run_cross(XQ, XC, spec, weights, pairs=None, Q=None, C=None, Dm=None, slices=1, raw=False):
    from pymde_amd import dense
    out = dense._pair_loss_cross(_dev(XQ, F32), _dev(XC, F32), spec, Q=None if Q is None else _dev(Q, F32),
                                 C=None if C is None else _dev(C, F32), Dm=None if Dm is None else _dev(Dm, F32),
                                 slices=slices, weights=weights, pairs=pairs)
    torch.cuda.synchronize()
    if raw:
        return out
    return float(out[0].item()), out[1].cpu().numpy(), out[2].cpu().numpy()


def _sums(X, edges, a0, a1, kind, scalars, row_of):
    """The oracle's SUMS over an edge list: (sum of the losses, the gradient of that sum [n, d], per-row sums through
    `row_of(edges)` -> list of index arrays), all float64."""
    from oracle import oracle
    fd = oracle.func(kind, a0, a1, scalars)
    m = len(edges)
    loss, grad = oracle.average_distortion(edges, X, fd)
    per_edge = oracle.distortions(oracle.distances(edges, X), fd).astype(np.float64)
    rows = np.zeros(X.shape[0])
    for idx in row_of(edges):
        np.add.at(rows, idx, per_edge)
    return loss * m, np.asarray(grad, dtype=np.float64) * m, rows


def _is_weighted(kind):
    return kind in ("L_WEIGHTED_QUADRATIC", "L_WEIGHTED_POWER")


def _oracle_square(X, D, W, kind, scalars=(), continuous=False):
    """(loss, grad, row_loss) of the weighted square problem: mean over the pairs with W > 0 (strict upper triangle).
    `continuous`: a weighted kind takes float32(W) as a1 in one evaluation; otherwise the combination by weight value."""
    X = np.ascontiguousarray(X, dtype=np.float32)
    iu, ju = np.triu_indices(X.shape[0], 1)
    w = W[iu, ju]
    kept = w > 0
    both = lambda e: [e[:, 0], e[:, 1]]
    total, G, rows = 0.0, np.zeros(X.shape, dtype=np.float64), np.zeros(X.shape[0])
    groups = [None] if continuous else [v for v in np.unique(w) if v > 0]
    for v in groups:
        sel = kept if v is None else (w == v)
        edges = np.stack([iu[sel], ju[sel]], 1).astype(np.int64)
        a0 = D[iu[sel], ju[sel]].astype(np.float32)
        if v is None:
            a1, factor = w[sel].astype(np.float32), 1.0
        else:
            a1, factor = (np.ones(len(a0), dtype=np.float32) if _is_weighted(kind) else None), float(v)
        s, g, r = _sums(X, edges, a0, a1, kind, scalars, both)
        total, G, rows = total + factor * s, G + factor * g, rows + factor * r
    pairs = int(kept.sum())
    return (total / pairs, G / pairs, rows), pairs


def _oracle_cross(XQ, XC, D, W, kind, scalars=(), continuous=False):
    """The same for the rectangular problem over the bipartite pairs with W > 0: gradient rows of the queries."""
    n_q, n_c = D.shape
    X = np.ascontiguousarray(np.concatenate([XC, XQ]).astype(np.float32))
    i, j = np.divmod(np.arange(n_q * n_c, dtype=np.int64), n_c)
    w = W[i, j]
    kept = w > 0
    queries = lambda e: [e[:, 1]]
    total, G, rows = 0.0, np.zeros(X.shape, dtype=np.float64), np.zeros(X.shape[0])
    groups = [None] if continuous else [v for v in np.unique(w) if v > 0]
    for v in groups:
        sel = kept if v is None else (w == v)
        edges = np.stack([j[sel], n_c + i[sel]], 1)
        a0 = D[i[sel], j[sel]].astype(np.float32)
        if v is None:
            a1, factor = w[sel].astype(np.float32), 1.0
        else:
            a1, factor = (np.ones(len(a0), dtype=np.float32) if _is_weighted(kind) else None), float(v)
        s, g, r = _sums(X, edges, a0, a1, kind, scalars, queries)
        total, G, rows = total + factor * s, G + factor * g, rows + factor * r
    pairs = int(kept.sum())
    return (total / pairs, G[n_c:] / pairs, rows[n_c:]), pairs


def _sym_weights(n, seed):
    """A seeded symmetric [n, n] float32 matrix over VALUES in which every row keeps a pair."""
    def make():
        rng = np.random.default_rng(seed)
        U = np.triu(rng.choice(np.asarray(VALUES, dtype=np.float32), size=(n, n)), 1)
        if n == 2:
            U[0, 1] = 2.0
        W = (U + U.T).astype(np.float32)
        assert ((W > 0).sum(1) >= 1).all()                       # every row keeps a pair
        return W
    return _cached(("sym", n, seed), make)


def _equal(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


# ---------------------------------------------------------------- 1. matrix weights from {0, 0.5, 2, 3}
SHAPES = [(2, 1, 1, 1), (64, 37, 2, 1), (64, 37, 1, 3), (193, 37, 2, 1), (193, 37, 2, 3), (193, 70, 5, 3),
          (193, 37, 8, 0), (257, 70, 3, 1), (257, 70, 3, 40), (257, 37, 2, 40)]


@pytest.mark.parametrize("n,nf,d,slices", SHAPES)
def test_matrix_weights_shapes_from_both_sources(n, nf, d, slices):
    A, X, D = _grid_case(n, nf, d)
    W = _sym_weights(n, 7 * n + d)
    want, pairs = _cached(("quad", n, nf, d), lambda: _oracle_square(X, D, W, "L_QUADRATIC"))
    assert 1 <= pairs < n * (n - 1) // 2 or n == 2
    spec, label = _spec("L_QUADRATIC"), "%dx%d d=%d slices=%d" % (n, nf, d, slices)
    _compare("W gram " + label, _run(X, spec, _matrix(W), pairs, A=A, slices=slices), want)
    _compare("W matrix " + label, _run(X, spec, _matrix(W), pairs, Dm=D.astype(np.float32), slices=slices), want)


@pytest.mark.parametrize("name", ["Quadratic", "WeightedQuadratic", "Huber", "Cubic", "Power1.5", "Power2.5", "Absolute",
                                  "Logistic", "Fractional", "SoftFractional"])
def test_matrix_weights_every_public_loss(name):
    from pymde_amd import dense
    make, kind, scalars = _loss_cases()[name]
    spec = dense.loss_spec(make)
    A, X, D = _grid_case(193, 37, 2)
    W = _sym_weights(193, 11)
    want, pairs = _oracle_square(X, D, W, kind, scalars)
    _compare("W %s gram" % name, _run(X, spec, _matrix(W), pairs, A=A), want)
    _compare("W %s matrix" % name, _run(X, spec, _matrix(W), pairs, Dm=D.astype(np.float32), slices=3), want)


# ---------------------------------------------------------------- 2. continuous weights on the weighted kinds
@pytest.mark.parametrize("kind,scalars", [("L_WEIGHTED_QUADRATIC", ()), ("L_WEIGHTED_POWER", (1.7,))])
def test_continuous_weights_are_a1(kind, scalars):
    A, X, D = _grid_case(193, 37, 2)
    rng = np.random.default_rng(3)
    U = np.triu(rng.uniform(0.1, 4.0, (193, 193)) * (rng.random((193, 193)) < 0.8), 1)
    W = (U + U.T).astype(np.float32)
    assert ((W > 0).sum(1) >= 1).all()
    want, pairs = _oracle_square(X, D, W, kind, scalars, continuous=True)
    spec = _spec(kind, scalars, weighted=True)
    _compare("continuous %s gram" % kind, _run(X, spec, _matrix(W), pairs, A=A, slices=3), want)
    _compare("continuous %s matrix" % kind, _run(X, spec, _matrix(W), pairs, Dm=D.astype(np.float32)), want)


# ---------------------------------------------------------------- 3. the power form
@pytest.mark.parametrize("p", [1.0, 2.5])
def test_power_weights_against_the_oracle(p):
    A, X, D = _grid_case(193, 37, 2)
    off = ~np.eye(193, dtype=bool)
    assert D[off].min() >= 1.0
    with np.errstate(divide="ignore"):
        Wp = np.where(off, D ** -p, 0.0)                         # float64; rounded once where the oracle takes it
    all_pairs = 193 * 192 // 2
    # a weighted kind takes w as a1; Quadratic times w is the same function (Sammon's, at p = 1); Absolute times w is
    # the weighted power loss of exponent 1
    for spec, kind, scalars in ((_spec("L_WEIGHTED_QUADRATIC", weighted=True), "L_WEIGHTED_QUADRATIC", ()),
                                (_spec("L_QUADRATIC"), "L_WEIGHTED_QUADRATIC", ()),
                                (_spec("L_ABSOLUTE"), "L_WEIGHTED_POWER", (1.0,))):
        want, pairs = _oracle_square(X, D, Wp, kind, scalars, continuous=True)
        assert pairs == all_pairs
        label = "p=%g kind %d as %s" % (p, spec.kind, kind)
        _compare(label + " gram", _run(X, spec, _power(p), A=A, slices=3), want)
        _compare(label + " matrix", _run(X, spec, _power(p), Dm=D.astype(np.float32), slices=0), want)


def _old(X, spec, A=None, Dm=None, slices=1):
    from pymde_amd import dense
    out = dense._pair_loss(_dev(X, F32), spec, A=None if A is None else _dev(A, F32),
                           Dm=None if Dm is None else _dev(Dm, F32), slices=slices)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("source", ["gram", "matrix"])
def test_default_and_unit_weights_keep_the_bits_of_the_old_entry_point(source):
    A, X, D = _grid_case(257, 70, 3)
    src = dict(A=A) if source == "gram" else dict(Dm=D.astype(np.float32))
    weighted, plain = _spec("L_WEIGHTED_QUADRATIC", weighted=True), _spec("L_HUBER", (3.0,))
    for slices in (1, 3):
        # p = 2 is the expression of the default weights
        assert _equal(_run(X, weighted, _power(2.0), slices=slices, raw=True, **src), _old(X, weighted, slices=slices, **src))
        # p = 0 is exactly 1, and so is a matrix of ones (its diagonal is never used)
        old = _old(X, plain, slices=slices, **src)
        assert _equal(_run(X, plain, _power(0.0), slices=slices, raw=True, **src), old)
        ones = np.ones((257, 257), dtype=np.float32)
        assert _equal(_run(X, plain, _matrix(ones), 257 * 256 // 2, slices=slices, raw=True, **src), old)


# ---------------------------------------------------------------- 4. missing pairs
def _poisoned(D, W):
    """D as float32 with NaN and +inf, alternating, wherever W == 0 (the diagonal included)."""
    Dm = D.astype(np.float32).copy()
    gone = np.argwhere(W == 0)
    Dm[gone[::2, 0], gone[::2, 1]] = np.nan
    Dm[gone[1::2, 0], gone[1::2, 1]] = np.inf
    return Dm


def test_unknown_deviations_of_missing_pairs_never_count():
    A, X, D = _grid_case(193, 37, 2)
    W = _sym_weights(193, 11)
    Dm = _poisoned(D, W)
    assert np.isnan(Dm).sum() > 1000 and np.isinf(Dm).sum() > 1000
    for name in ("L_QUADRATIC", "L_ABSOLUTE"):
        want, pairs = _oracle_square(X, D, W, name)
        for slices in (1, 3):
            _compare("poisoned %s slices=%d" % (name, slices), _run(X, _spec(name), _matrix(W), pairs, Dm=Dm, slices=slices),
                     want)


def test_a_whole_tile_of_zero_weights_and_a_row_with_one_pair_in_the_last_tile():
    A, X, D = _grid_case(193, 37, 2)
    W = _sym_weights(193, 11).copy()
    W[0:64, 64:128] = 0.0                                        # tile (0, 1) and its mirror image
    W[64:128, 0:64] = 0.0
    W[5, :] = 0.0                                                # row 5 keeps the pair (5, 192) alone: the last,
    W[:, 5] = 0.0                                                # partial tile of its row
    W[5, 192] = W[192, 5] = 2.0
    assert ((W > 0).sum(1) >= 1).all() and (W[5] > 0).sum() == 1
    want, pairs = _oracle_square(X, D, W, "L_QUADRATIC")
    Dm = _poisoned(D, W)
    got = _run(X, _spec("L_QUADRATIC"), _matrix(W), pairs, Dm=Dm, slices=3)
    _compare("empty tile, matrix", got, want)
    _compare("empty tile, gram", _run(X, _spec("L_QUADRATIC"), _matrix(W), pairs, A=A), want)
    # the row with one pair: its loss is that pair's
    one = 2.0 * (np.linalg.norm(X[5].astype(np.float64) - X[192]) - D[5, 192]) ** 2
    assert abs(got[2][5] - one) <= 1e-5 * max(one, want[2].mean())


# ---------------------------------------------------------------- 5. rectangular and list forms
def _rect_weights(n_q, n_c, seed):
    rng = np.random.default_rng(seed)
    W = rng.choice(np.asarray(VALUES, dtype=np.float32), size=(n_q, n_c))
    W[np.arange(n_q), rng.integers(0, n_c, n_q)] = 2.0          # every query row keeps a pair
    return W.astype(np.float32)


@pytest.mark.parametrize("n_q,n_c,nf,d,slices", [(1, 193, 37, 2, 1), (193, 1, 37, 2, 1), (193, 257, 37, 1, 0),
                                                 (193, 257, 37, 1, 3), (257, 193, 70, 8, 40)])
def test_rectangular_matrix_weights(n_q, n_c, nf, d, slices):
    Q, C, XQ, XC, D = _cross_case(n_q, n_c, nf, d)
    W = _rect_weights(n_q, n_c, n_q + n_c)
    label = "%dx%d d=%d slices=%d" % (n_q, n_c, d, slices)
    for kind in ("L_QUADRATIC", "L_WEIGHTED_QUADRATIC"):
        want, pairs = _oracle_cross(XQ, XC, D, W, kind)
        spec = _spec(kind, weighted=_is_weighted(kind))
        _compare_cross("W cross gram %s %s" % (kind, label), _run_cross(XQ, XC, spec, _matrix(W), pairs, Q=Q, C=C, slices=slices),
                       want)
        Dm = _poisoned(D, W)
        _compare_cross("W cross matrix %s %s" % (kind, label), _run_cross(XQ, XC, spec, _matrix(W), pairs, Dm=Dm, slices=slices),
                       want)


def test_rectangular_power_weights():
    Q, C, XQ, XC, D = _cross_case(193, 257, 37, 2)
    assert D.min() >= 1.0
    for p in (1.0, 2.5):
        want, pairs = _oracle_cross(XQ, XC, D, D ** -p, "L_WEIGHTED_QUADRATIC", continuous=True)
        assert pairs == 193 * 257
        _compare_cross("cross p=%g" % p, _run_cross(XQ, XC, _spec("L_QUADRATIC"), _power(p), Q=Q, C=C, slices=3), want)


@pytest.mark.parametrize("form", ["power", "matrix"])
@pytest.mark.parametrize("source", ["gram", "matrix"])
def test_the_list_form_has_the_bits_of_the_rectangular_call(form, source):
    from pymde_amd import rows as rows_mod
    Q, C, XQ, XC, D = _cross_case(193, 257, 37, 2)
    W = _rect_weights(193, 257, 5)
    weights, pairs = (_power(1.0), None) if form == "power" else (_matrix(W), int((W > 0).sum()))
    src = dict(Q=Q, C=C) if source == "gram" else dict(Dm=_poisoned(D, W) if form == "matrix" else D.astype(np.float32))
    spec = _spec("L_HUBER", (3.0,))
    listed = torch.as_tensor(np.random.default_rng(9).permutation(193)[:101].astype(np.int32)).to(DEV)
    for slices in (1, 3):
        full = _run_cross(XQ, XC, spec, weights, pairs, slices=slices, raw=True, **src)
        row_loss = torch.full((193,), -7.0, dtype=torch.float64, device=DEV)
        row_grad = torch.full((193, 2), -7.0, dtype=F32, device=DEV)
        rows_mod.pair_loss_cross_rows(_dev(XQ, F32), _dev(XC, F32), spec, row_loss, row_grad, rows=listed,
                                      slices=slices, weights=weights, **{k: _dev(v, F32) for k, v in src.items()})
        torch.cuda.synchronize()
        idx = listed.long()
        assert torch.equal(row_loss[idx], full[2][idx])
        rest = torch.ones(193, dtype=torch.bool, device=DEV)
        rest[idx] = False
        assert (row_loss[rest] == -7).all() and (row_grad[rest] == -7).all()
        # row_grad = G / n_c where the rectangular call has G / pairs
        scale = (193.0 * 257.0 if pairs is None else float(pairs)) / 257.0
        np.testing.assert_allclose(row_grad[idx].cpu().numpy(), full[1][idx].cpu().numpy() * scale, rtol=1e-6, atol=0)


# ---------------------------------------------------------------- 6. determinism, arguments, the checking kernel
def test_two_runs_give_the_same_bits():
    A, X, D = _grid_case(257, 70, 3)
    W = _sym_weights(257, 7 * 257 + 3)
    pairs = int(np.triu(W > 0, 1).sum())
    for weights, n_pairs in ((_matrix(W), pairs), (_power(2.5), None)):
        for slices in (1, 3):
            for src in (dict(A=A), dict(Dm=D.astype(np.float32))):
                first = _run(X, _spec("L_QUADRATIC"), weights, n_pairs, slices=slices, raw=True, **src)
                again = _run(X, _spec("L_QUADRATIC"), weights, n_pairs, slices=slices, raw=True, **src)
                assert _equal(first, again)


def test_invalid_weight_arguments_launch_nothing():
    from pymde_amd import _lib
    from pymde_amd.functions.function import KIND
    lib = _lib.load()
    n, nf, d = 100, 5, 2
    A = _dev(np.random.default_rng(0).standard_normal((n, nf)).astype(np.float32))
    Wm = _dev(np.ones((n, n), dtype=np.float32))
    X = _dev(np.random.default_rng(1).standard_normal((n, d)).astype(np.float32))
    loss = torch.full((1,), -7.0, dtype=torch.float64, device=DEV)
    grad = torch.full((n, d), -7.0, dtype=F32, device=DEV)
    rows = torch.full((n,), -7.0, dtype=torch.float64, device=DEV)
    work = torch.full((1 << 20,), 0x5A, dtype=torch.uint8, device=DEV)
    listed = torch.arange(n, dtype=torch.int32, device=DEV)
    p, st, quad = _lib.ptr, _lib.stream_ptr(), KIND["L_QUADRATIC"]
    all_pairs = 0.5 * n * (n - 1)
    inf, nan = float("inf"), float("nan")

    def square(source=1, p_=1.0, W_=None, pairs=all_pairs, d_=d):
        return lib.mde_pair_loss_weighted(n, nf, p(A), 0, None, 1.0, d_, p(X), quad, 0.0, 0.0, 0.0, 1, source, p_, p(W_),
                                          pairs, p(loss), p(grad), p(rows), p(work), st)

    def cross(source=1, p_=1.0, W_=None, pairs=float(n * n)):
        return lib.mde_pair_loss_cross_weighted(n, n, nf, p(A), p(A), 0, None, 1.0, d, p(X), p(X), quad, 0.0, 0.0, 0.0,
                                                1, source, p_, p(W_), pairs, p(loss), p(grad), p(rows), p(work), st)

    def listc(source=1, p_=1.0, W_=None):
        return lib.mde_pair_loss_cross_rows_weighted(n, n, nf, p(A), p(A), 0, None, 1.0, d, p(X), p(X), quad, 0.0, 0.0,
                                                     0.0, 1, n, p(listed), source, p_, p(W_), p(rows), p(grad), p(work),
                                                     st)
    bad = []
    for call in (square, cross, listc):
        bad += [call(source=1, W_=Wm),              # both sources given
                call(source=0, W_=Wm), call(source=2, W_=None), call(source=3), call(source=-1),
                call(p_=-1.0), call(p_=inf), call(p_=nan)]
    for call in (square, cross):
        bad += [call(pairs=0.0), call(pairs=-3.0), call(pairs=inf), call(pairs=nan)]
    bad += [square(d_=9)]                           # and whatever the old entry point refuses
    assert bad == [_lib.MDE_E_INVALID] * len(bad)
    assert "mde_pair_loss_weighted" in _lib.last_error()
    torch.cuda.synchronize()
    assert (loss == -7).all() and (grad == -7).all() and (rows == -7).all() and (work == 0x5A).all()
    ok = [square(), square(source=2, W_=Wm), square(source=0), cross(), cross(source=2, W_=Wm), listc(),
          listc(source=2, W_=Wm)]
    assert ok == [_lib.MDE_OK] * len(ok)
    torch.cuda.synchronize()
    assert torch.isfinite(loss).all() and torch.isfinite(grad).all() and (rows >= 0).all()


def _check_numpy(W, Dm, square):
    W64 = W.astype(np.float64)
    n_q, n_c = W.shape
    off = ~np.eye(n_q, dtype=bool) if square else np.ones(W.shape, dtype=bool)
    fin = np.isfinite(W)
    with np.errstate(invalid="ignore"):
        kept = off & (W > 0)
        counts = [int((off & ~fin).sum()), int((off & (W < 0)).sum()),
                  int(np.triu(kept, 1).sum()) if square else int(kept.sum()), int((kept.sum(1) == 0).sum()), 0]
        tops = [0.0, 0.0, 0.0, 0.0]
        if Dm is not None:
            d_ok = np.isfinite(Dm) & (Dm >= 0)
            counts[4] = int((kept & ~d_ok).sum())
        if square:
            diff = np.abs(W64 - W64.T)
            tops[0] = float(diff[off & fin & np.isfinite(diff)].max(initial=0.0))
            tops[1] = float(np.abs(W64)[off & fin].max(initial=0.0))
            if Dm is not None:
                dd = np.abs(Dm.astype(np.float64) - Dm.astype(np.float64).T)
                tops[2] = float(dd[kept & d_ok & np.isfinite(dd)].max(initial=0.0))
                tops[3] = float(Dm[kept & d_ok].max(initial=0.0))
    return counts, tops, kept.sum(1).astype(np.int32)


def _check_gpu(W, Dm, square):
    from pymde_amd import dense
    s = dense.weight_stats(_dev(W, F32), None if Dm is None else _dev(Dm, F32), square)
    return ([s.nonfinite, s.negative, s.kept, s.empty_rows, s.bad_deviations],
            [s.asymmetry, s.largest, s.deviation_asymmetry, s.largest_deviation], s.row_kept.cpu().numpy())


def _same_check(W, Dm, square):
    counts, tops, row_kept = _check_gpu(W, Dm, square)
    wcounts, wtops, wrows = _check_numpy(W, Dm, square)
    assert counts == wcounts
    assert np.asarray(tops, dtype=np.float32).tolist() == np.asarray(wtops, dtype=np.float32).tolist()
    assert (row_kept == wrows).all()
    return counts, tops


def test_the_checking_kernel_against_numpy():
    _, _, D = _grid_case(193, 37, 2)
    W = _sym_weights(193, 11)
    Dm = _poisoned(D, W)
    counts, tops = _same_check(W, Dm, True)
    assert counts[:2] == [0, 0] and counts[3:] == [0, 0] and tops[0] == 0.0 and tops[1] == 3.0 and tops[2] == 0.0
    _same_check(W, None, True)
    # one poisoned entry of each kind, each away from the diagonal
    for value, slot in ((np.nan, 0), (np.inf, 0), (-np.inf, 0), (-1.0, 1)):
        V = W.copy()
        V[70, 3] = value
        assert _same_check(V, Dm, True)[0][slot] >= 1
    V = W.copy()
    V[70, 3] = V[3, 70] + 0.25                                   # asymmetric
    assert _same_check(V, Dm, True)[1][0] == 0.25
    V = W.copy()
    V[100, :] = 0.0                                              # a row without a pair (and its column: symmetric)
    V[:, 100] = 0.0
    assert _same_check(V, Dm, True)[0][3] == 1
    for value in (np.nan, np.inf, -2.0):                         # a kept pair whose deviation is unknown
        i, j = np.argwhere(np.triu(W, 1) > 0)[17]
        E = Dm.copy()
        E[i, j] = value
        assert _same_check(W, E, True)[0][4] == 1
    E = Dm.copy()
    i, j = np.argwhere(np.triu(W, 1) > 0)[17]
    E[i, j] += 0.5                                               # the deviations of a kept pair disagree
    assert _same_check(W, E, True)[1][2] == 0.5
    V = W.copy()
    np.fill_diagonal(V, np.nan)                                  # the diagonal of a square W is ignored
    assert _same_check(V, Dm, True)[0] == counts
    # rectangular: every entry is a pair, 257 x 193 and a single row
    _, _, _, _, Dr = _cross_case(257, 193, 70, 8)
    Wr = _rect_weights(257, 193, 1)
    Wr[200, :] = 0.0
    rcounts, _ = _same_check(Wr, _poisoned(Dr, Wr), False)
    assert rcounts[2] == int((Wr > 0).sum()) and rcounts[3] == 1 and rcounts[4] == 0
    _same_check(Wr[:1].copy(), None, False)

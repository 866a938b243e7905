"""``mde_pair_sqdist_apply`` (csrc/mde_pair_apply.hip) against float64 on the same float32 inputs.

Bounds.  The matrix source squares a float32 entry exactly in double and adds ``n_c`` products by fma in a fixed
order: at most ``n_c + 8`` roundings of ``2^-53`` each on the way to an output (the columns of a thread, the four
threads of a row, the slices), and the float64 reference carries as many: ``2 (n_c + 8) 2^-53 sum_j S |V|``.  The Gram
sources add the tile's own error: a float32 squared distance in the expanded form is within ``EPS(nf) (|x|^2 + |y|^2)``
of float64, ``EPS(nf) = (nf + 2) 2^-24`` (the bound of tests/test_gpu_landmarks.py), summed against ``|V|``; mode 1
propagates it through the square, ``|(d2 + e)^2 - d2^2| / 4 <= (2 d2 e + e^2) / 4``.  Every test prints its worst
error / bound; observed on an MI355X over all cases: 0.30 (mode 0), 0.07 (mode 1), 0.09 (matrix).
"""
import ctypes
import itertools

import numpy as np
import pytest
import torch

from pymde_amd import _lib, classical

import _classical_reference as ref

pytestmark = pytest.mark.gpu

SHAPES = [(1, 2), (63, 65), (64, 64), (130, 257)]
RANKS = [1, 3, 8, 9, 18, 32]          # every padded width (8, 16, 32) and its edge
FEATURES = [1, 5, 33, 64]
SOURCES = ["gram0", "gram1", "matrix"]
SLICES = [1, 3, 0, 7]                 # 7 exceeds the column tiles of every shape here: empty slices
U53 = 2.0 ** -53


def EPS(nf):
    return (nf + 2) * 2.0 ** -24


def _inputs(n_q, n_c, nf, r, source, seed=0):
    """float32 inputs of one case: ``(Q, C, Dm, V)`` as numpy arrays (the unused source is None)."""
    rng = np.random.default_rng([seed, n_q, n_c, nf, r])
    V = rng.standard_normal((n_c, r)).astype(np.float32)
    if source == "matrix":
        return None, None, (np.abs(rng.standard_normal((n_q, n_c))) * 3.0).astype(np.float32), V
    Q, C = rng.standard_normal((n_q, nf)) + 0.5, rng.standard_normal((n_c, nf)) + 0.5
    if source == "gram1":
        Q, C = ref.unit_rows(Q), ref.unit_rows(C)
    return Q.astype(np.float32), C.astype(np.float32), None, V


def _reference(Q, C, Dm, V, source, skip=False):
    """``(S V, bound)`` in float64: the product and the entrywise error the kernel may have."""
    V64 = V.astype(np.float64)
    if source == "matrix":
        S = Dm.astype(np.float64) ** 2
        err = np.zeros_like(S)
    else:
        Q64, C64 = Q.astype(np.float64), C.astype(np.float64)
        d2 = ref.d2_rows(Q64, C64)
        e = EPS(Q.shape[1]) * ((Q64 ** 2).sum(1)[:, None] + (C64 ** 2).sum(1)[None, :])
        S, err = (d2, e) if source == "gram0" else ((0.5 * d2) ** 2, 0.25 * (2.0 * d2 * e + e * e))
    if skip:
        S, err = S.copy(), err.copy()
        np.fill_diagonal(S, 0.0)
        np.fill_diagonal(err, 0.0)
    bound = err @ np.abs(V64) + 2.0 * (V.shape[0] + 8) * U53 * ((S + err) @ np.abs(V64))
    return S @ V64, bound


def _device(*arrays):
    return [None if a is None else torch.as_tensor(a).cuda().contiguous() for a in arrays]


def _apply(Q, C, Dm, V, source, slices, skip=False):
    return classical.sqdist_apply(V, Q=Q, C=C, mode=1 if source == "gram1" else 0, Dm=Dm, skip_diagonal=skip,
                                  slices=slices)


def _check(got, want, bound, what):
    err = np.abs(got.cpu().numpy() - want)
    ratio = float((err / np.maximum(bound, 1e-300)).max())
    print("%s: worst error / bound %.3g (largest error %.3g)" % (what, ratio, float(err.max())))
    assert np.all(err <= bound), what


CASES = [(shape, source, r, FEATURES[i % 4])
         for i, (shape, source, r) in enumerate(itertools.product(SHAPES, SOURCES, RANKS))]


@pytest.mark.parametrize("shape,source,r,nf", CASES)
def test_against_float64(shape, source, r, nf):
    n_q, n_c = shape
    host = _inputs(n_q, n_c, nf, r, source)
    want, bound = _reference(*host, source)
    dev = _device(*host)
    for slices in SLICES:
        got = _apply(*dev, source, slices)
        assert got.dtype == torch.float64 and tuple(got.shape) == (n_q, r)
        _check(got, want, bound, "%s %dx%d nf=%d r=%d slices=%d" % (source, n_q, n_c, nf, r, slices))


@pytest.mark.parametrize("source", SOURCES)
@pytest.mark.parametrize("nf", FEATURES)
def test_every_feature_count_on_every_source(source, nf):
    """(the cases above pair each rank with one feature count; here every count meets every source at r = 18)"""
    host = _inputs(130, 257, nf, 18, source, seed=1)
    want, bound = _reference(*host, source)
    _check(_apply(*_device(*host), source, 3), want, bound, "%s nf=%d" % (source, nf))


@pytest.mark.parametrize("n", [64, 130])
def test_skip_diagonal_is_by_index(n):
    # a matrix whose diagonal holds 7.0: with skip_diagonal it never counts, without it it is an ordinary entry
    _, _, Dm, V = _inputs(n, n, 1, 9, "matrix", seed=2)
    np.fill_diagonal(Dm, 7.0)
    dev = _device(None, None, Dm, V)
    want, bound = _reference(None, None, Dm, V, "matrix", skip=True)
    for slices in SLICES:
        _check(_apply(*dev, "matrix", slices, skip=True), want, bound, "matrix diagonal 7, n=%d, skipped" % n)
    want_all, bound_all = _reference(None, None, Dm, V, "matrix")
    assert np.abs(want_all - want - 49.0 * V.astype(np.float64)).max() <= 1e-9
    _check(_apply(*dev, "matrix", 1), want_all, bound_all, "matrix diagonal 7, n=%d, counted" % n)
    # Gram rows with a duplicated row: the pair (5, 17) is an ordinary pair, only j == i is left out
    for source in ("gram0", "gram1"):
        Q, _, _, V = _inputs(n, n, 33, 9, source, seed=3)
        Q[17] = Q[5]
        want, bound = _reference(Q, Q, None, V, source, skip=True)
        dev = _device(Q, Q, None, V)
        for slices in (1, 3):
            _check(_apply(*dev, source, slices, skip=True), want, bound, "%s duplicated row, n=%d" % (source, n))
    # two rows far from the origin: d2(i, i) is rounding noise of the order of the bound, d2(0, 1) = d2(1, 0) = 5 is
    # the only pair of either row
    far = np.full((2, 5), 1000.0, dtype=np.float32)
    far[1] += 1.0
    got = _apply(*_device(far, far, None, np.ones((2, 1), np.float32)), "gram0", 1, skip=True)
    assert abs(float(got[0, 0]) - 5.0) <= EPS(5) * 2 * 5.01e6 and torch.equal(got[0], got[1])


@pytest.mark.parametrize("source", SOURCES)
def test_same_bits_on_every_run_and_for_every_block_mate(source):
    host = _inputs(130, 257, 33, 18, source, seed=4)
    Q, C, Dm, V = _device(*host)
    for slices in (1, 3):
        full = _apply(Q, C, Dm, V, source, slices)
        assert torch.equal(full, _apply(Q, C, Dm, V, source, slices))
        # rows 0 .. 63 computed alone, at the same slice count
        alone = _apply(None if Q is None else Q[:64].contiguous(), C, None if Dm is None else Dm[:64].contiguous(), V,
                       source, slices)
        assert torch.equal(alone, full[:64])
        # ... and one row alone
        one = _apply(None if Q is None else Q[70:71].contiguous(), C, None if Dm is None else Dm[70:71].contiguous(),
                     V, source, slices)
        assert torch.equal(one, full[70:71])


def test_refused_arguments():
    lib = _lib.load()
    n_q, n_c, nf, r = 8, 8, 4, 3
    Q = torch.zeros((n_q, nf), device="cuda")
    Dm = torch.zeros((n_q, n_c), device="cuda")
    V = torch.zeros((n_c, r), device="cuda")
    out = torch.full((n_q, r), -1.0, dtype=torch.float64, device="cuda")
    work = torch.empty(1 << 16, dtype=torch.uint8, device="cuda")
    p, stream = _lib.ptr, _lib.stream_ptr(torch.device("cuda", 0))
    good = dict(n_q=n_q, n_c=n_c, nf=nf, Q=p(Q), C=p(Q), mode=0, Dm=None, skip=1, r=r, V=p(V), slices=1, out=p(out),
                work=p(work))

    def call(**changed):
        a = dict(good, **changed)
        return lib.mde_pair_sqdist_apply(a["n_q"], a["n_c"], a["nf"], a["Q"], a["C"], a["mode"], a["Dm"], a["skip"],
                                         a["r"], a["V"], a["slices"], a["out"], a["work"], stream)

    refused = [dict(r=0), dict(r=33), dict(Dm=p(Dm)), dict(Q=None, C=None), dict(C=None), dict(Q=None),
               dict(n_q=7), dict(V=None), dict(out=None), dict(work=None), dict(n_q=0, skip=0), dict(n_c=0, skip=0),
               dict(n_q=1 << 31, skip=0), dict(n_c=1 << 31, skip=0), dict(mode=2), dict(mode=-1), dict(nf=0),
               dict(slices=-1), dict(slices=65536)]
    for changed in refused:
        assert call(**changed) == _lib.MDE_E_INVALID, changed
        assert "mde_pair_sqdist_apply" in _lib.last_error()
    torch.cuda.synchronize()
    assert bool((out == -1.0).all())                       # nothing was launched
    assert call() == _lib.MDE_OK and call(Q=None, C=None, Dm=p(Dm)) == _lib.MDE_OK
    torch.cuda.synchronize()
    assert bool((out == 0.0).all())
    for sizes in ((0, 8, 3, 1), (8, 0, 3, 1), (8, 8, 0, 1), (8, 8, 33, 1), (8, 8, 3, -1), (1 << 31, 8, 3, 1)):
        assert lib.mde_pair_sqdist_apply_work_bytes(*sizes) == _lib.MDE_E_INVALID, sizes
    assert lib.mde_pair_sqdist_apply_work_bytes(130, 257, 18, 1) == 4 * (130 + 257)
    assert lib.mde_pair_sqdist_apply_work_bytes(130, 257, 18, 3) == 3 * 130 * 18 * 8 + 4 * (130 + 257)
    assert isinstance(ctypes.c_int64(lib.mde_pair_sqdist_apply_work_bytes(130, 257, 18, 0)).value, int)

"""``classical.triangulate`` and the triangulated start of ``DensePlacement`` / ``LandmarkMDE`` on the GPU.

Bound of a triangulated coordinate against the float64 formula on the same float32 inputs, with ``P = pinv(L)^T``
and ``c = deviation_scale^2``: the kernel's error in a squared deviation, ``EPS(nf) (|q|^2 + |c|^2)`` for the Gram
source (``EPS(nf) = (nf + 2) 2^-24``, tests/test_gpu_landmarks.py) and none for a matrix, summed against ``|P|``;
the rounding of ``P`` to float32, ``2^-24 sum_j delta |P_j|``; both times ``c / 2``; and the rounding of the result
to float32.  Its floor is the float64 figure of tests/test_classical_host.py for deviations rounded to float32
(3e-8 at this scale).  Against the TRUE images the formula's own distance to them on those inputs is added.
Observed on an MI355X: 2.1e-7 to 4.3e-7 against the formula, 0.03 (Gram) to 0.33 (matrix) of the bound.
"""
import numpy as np
import pytest
import torch

import pymde_amd
from pymde_amd import classical, quality
from pymde_amd.functions import losses

import _classical_reference as ref

pytestmark = pytest.mark.gpu

U24 = 2.0 ** -24


def EPS(nf):
    return (nf + 2) * U24


def _r3_case(scale=1.0):
    """130 old and 70 new rows of R^3 in 20 features (float32), the old rows' embedding -- rotated, shifted, scaled by
    ``scale`` -- as float32, and the new rows' true images."""
    P_old, P_new = ref.points(130, 3, seed=2), ref.points(70, 3, seed=3)
    iso, R, shift = ref.isometry(3, 20, seed=4), ref.rotation(3, seed=5), np.array([1.0, -2.0, 0.5])
    C, Q = (P_old @ iso).astype(np.float32), (P_new @ iso).astype(np.float32)
    return Q, C, (scale * P_old @ R + shift).astype(np.float32), scale * P_new @ R + shift


@pytest.mark.parametrize("scale", [1.0, 2.5])
@pytest.mark.parametrize("source", ["gram", "matrix"])
def test_new_rows_come_back_at_their_true_images(source, scale):
    Q, C, X_old, want = _r3_case(scale)
    Q64, C64 = Q.astype(np.float64), C.astype(np.float64)
    if source == "gram":
        delta = ref.d2_rows(Q64, C64)
        kernel_error = EPS(20) * ((Q64 ** 2).sum(1)[:, None] + (C64 ** 2).sum(1)[None, :])
        got = classical.triangulate(torch.as_tensor(X_old).cuda(), Q=torch.as_tensor(Q).cuda(),
                                    C=torch.as_tensor(C).cuda(), deviation_scale=scale)
    else:
        Dm = np.sqrt(ref.d2_rows(Q64, C64)).astype(np.float32)
        delta = Dm.astype(np.float64) ** 2
        kernel_error = np.zeros_like(delta)
        got = classical.triangulate(torch.as_tensor(X_old).cuda(), Dm=torch.as_tensor(Dm).cuda(),
                                    deviation_scale=scale)
    formula, P = ref.triangulate(X_old.astype(np.float64), scale ** 2 * delta)
    bound = 0.5 * scale ** 2 * ((kernel_error + U24 * delta) @ np.abs(P)) + 2.0 * U24 * np.abs(formula)
    own = float(np.abs(formula - want).max())
    got = got.double().cpu().numpy()
    err, true_err = np.abs(got - formula), float(np.abs(got - want).max())
    print("%s, scale %g: against the float64 formula %.3g (worst error / bound %.3g), against the true images %.3g "
          "(the formula's own %.3g)" % (source, scale, err.max(), (err / bound).max(), true_err, own))
    assert got.shape == (70, 3) and np.all(err <= bound)
    assert true_err <= bound.max() + own


def test_collinear_embedded_rows_give_finite_output():
    t = np.linspace(-2.0, 2.0, 40)
    X_old = np.stack([t, np.full(40, 3.0)], 1).astype(np.float32)              # on a line in the plane
    new = np.array([[0.25, 3.0], [5.0, 3.0], [0.0, 4.0]])
    Dm = np.sqrt(ref.d2_rows(new, X_old.astype(np.float64))).astype(np.float32)
    got = classical.triangulate(torch.as_tensor(X_old).cuda(), Dm=torch.as_tensor(Dm).cuda()).cpu().numpy()
    assert np.all(np.isfinite(got))
    # along the line the position is found; across it (the null direction) every row stays at the mean's
    assert np.abs(got[:, 0] - np.array([0.25, 5.0, 0.0])).max() <= 1e-5
    assert np.abs(got[:, 1] - 3.0).max() <= 1e-5


def test_placement_started_by_triangulation():
    Q, C, X_old, want = _r3_case()
    place = pymde_amd.DensePlacement.weighted(C, X_old, Q, weights=None, loss=losses.Quadratic, init="triangulation")
    plain = pymde_amd.DensePlacement(C, X_old, Q, loss=losses.Quadratic)
    assert place.init == "triangulation" and plain.init == "neighbors"
    tri, near = place.initialization(), plain.initialization()
    assert torch.equal(tri, plain.initialization("triangulation")) and torch.equal(tri, place.initialization(None))
    assert np.abs(tri.double().cpu().numpy() - want).max() <= 1e-5
    v_tri, v_near = float(plain.average_distortion(tri)), float(plain.average_distortion(near))
    print("average distortion of the start: triangulation %.3g, neighbors %.3g" % (v_tri, v_near))
    assert v_tri < v_near
    place.embed(solver="rows")
    status = place.row_status.cpu().numpy()
    print("rows solver from the triangulated start: %d sweeps, %d of %d rows converged"
          % (place.solve_stats.iterations, int((status == 1).sum()), status.size))
    assert np.all(status == 1)
    plain.init = "triangulation"                                               # the attribute is the default method
    assert torch.equal(plain.initialization(), tri)
    with pytest.raises(ValueError, match="method"):
        plain.initialization("classical")
    # a weight matrix that leaves out pairs has no triangulated start
    W = np.ones((70, 130), dtype=np.float32)
    W[4, 7] = 0.0
    with pytest.raises(ValueError, match="every"):
        pymde_amd.DensePlacement.weighted(C, X_old, Q, weights=W, init="triangulation")
    with pytest.raises(ValueError, match="every"):
        pymde_amd.DensePlacement.weighted(C, X_old, Q, weights=W).initialization("triangulation")


def test_landmark_start_is_an_exact_copy():
    data = (ref.points(400, 2, seed=6) @ ref.isometry(2, 30, seed=7)).astype(np.float32)
    mde = pymde_amd.LandmarkMDE(data, landmarks=64, loss=losses.Quadratic, seed=0, init="classical")
    X0 = mde.initialization()
    score = float(quality.stress(data, X0, scale=1.0))
    print("stress at scale 1 of the landmark start, before any iteration: %.3g" % score)
    assert tuple(X0.shape) == (400, 2) and score <= 1e-3
    assert mde.landmark_problem.init == "classical"
    X = mde.embed(max_iter=5)
    assert mde.placement.init == "triangulation"
    assert float(quality.stress(data, X, scale=1.0)) <= 1e-3
    # the default start of both stages is what it was
    assert pymde_amd.LandmarkMDE(data, landmarks=64, seed=0).landmark_problem.init == "random"

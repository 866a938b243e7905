"""Classical scaling without a device: the float64 reference (tests/_classical_reference.py) against itself and
against closed forms, the defaults of the new keywords, and the argument errors that are raised before any device
work.

The float64 figures of the reference alone, n = 300, 10 oversamples (``test_replay_reaches_the_exact_solution``):
relative eigenvalue error <= 1e-15 and largest principal sine <= 2e-8 at 4 iterations on the planted rows
(eigenvalues 2.1e5, 9.3e4, 2.8e4 | 83), the squared cosine distance of the shifted rows (105, 63, 25 | 2.5, negative
eigenvalues down to -18.6) and the 300-cycle at d = 2 (sine 1.3e-8); at 2 iterations the cycle gives 5e-10 and 2.2e-5.
Triangulation of 50 rows against 200 in R^3: 2e-15, and 3.3e-8 once delta is rounded to float32.
"""
import inspect

import numpy as np
import pytest
import torch

import pymde_amd
from pymde_amd import classical, dense

import _classical_reference as ref


def test_points_in_r3_are_recovered_up_to_rotation():
    P = ref.points(120, 3, seed=1)
    X, lam, negative, evals = ref.classical_exact(ref.S_from_matrix(ref.pair_distances(P)), 3)
    assert not negative and lam.min() > 0
    assert np.abs(ref.pair_distances(X) - ref.pair_distances(P)).max() <= 1e-12
    assert ref.gram_gap(X, P - P.mean(0)) <= 1e-13
    assert np.abs(X.mean(0)).max() <= 1e-13
    # the other eigenvalues vanish, and the trace is sum S / (2 n)
    assert np.abs(np.sort(evals)[:-3]).max() <= 1e-10 * lam[0]
    assert abs(evals.sum() - ref.S_from_matrix(ref.pair_distances(P)).sum() / 240.0) <= 1e-10 * lam[0]


def test_cycle_is_a_circle():
    n = 300
    S = ref.S_from_matrix(ref.cycle_matrix(n))
    X, lam, negative, evals = ref.classical_exact(S, 2)
    assert abs(lam[0] - lam[1]) <= 1e-10 * lam[0]          # a double eigenvalue: compare distances, not vectors
    radius = np.linalg.norm(X, axis=1)
    assert np.abs(radius / radius[0] - 1.0).max() <= 1e-10
    angle = 2.0 * np.pi * np.arange(n) / n
    circle = radius[0] * np.stack([np.cos(angle), np.sin(angle)], 1)
    assert ref.gram_gap(X, circle) <= 1e-10
    assert evals.min() < -0.1 * lam[0]                     # graph distances are not Euclidean: B is indefinite


def test_apply_B_is_the_double_centred_product():
    S = ref.S_from_rows(ref.planted_rows(60, 10).astype(np.float64))
    V = ref.points(60, 5, seed=3)
    assert np.abs(ref.apply_B(S, V) - ref.B_matrix(S) @ V).max() <= 1e-12 * np.abs(S).max() * 60


@pytest.mark.parametrize("case,n_iter,eig_tol,sine_tol", [("planted", 4, 1e-14, 2e-8), ("cosine", 4, 1e-14, 2e-8),
                                                          ("cycle", 4, 1e-14, 5e-8), ("cycle", 2, 1e-8, 1e-4)])
def test_replay_reaches_the_exact_solution(case, n_iter, eig_tol, sine_tol):
    n = 300
    if case == "planted":
        S, d = ref.S_from_rows(ref.planted_rows(n).astype(np.float64)), 3
    elif case == "cosine":
        S, d = ref.S_from_rows(ref.unit_rows(ref.planted_cosine_rows(n)), 1), 3
    else:
        S, d = ref.S_from_matrix(ref.cycle_matrix(n)), 2
    omega = np.random.default_rng(7).standard_normal((n, d + 10))
    Xe, le, _, evals = ref.classical_exact(S, d)
    Xr, lr, _, _ = ref.replay(S, omega, d, n_iter)
    eig_err, sine = np.abs(lr - le).max() / le[0], ref.principal_sines(Xe, Xr).max()
    print("%s, %d iterations: eigenvalues %s | %.3g, smallest %.3g; relative eigenvalue error %.3g, largest sine %.3g"
          % (case, n_iter, le, np.sort(evals)[::-1][d], evals.min(), eig_err, sine))
    assert eig_err <= eig_tol and sine <= sine_tol
    if case == "cosine":
        assert evals.min() < -0.1 * le[0]


def test_triangulation_is_exact_for_euclidean_deviations():
    P_old, P_new = ref.points(200, 3, seed=2), ref.points(50, 3, seed=3)
    R, shift = ref.rotation(3, seed=4), np.array([1.0, -2.0, 0.5])
    delta = ref.d2_rows(P_new, P_old)
    got, P = ref.triangulate(P_old @ R + shift, delta)
    assert np.abs(got - (P_new @ R + shift)).max() <= 2e-14
    rounded, _ = ref.triangulate(P_old @ R + shift, delta.astype(np.float32).astype(np.float64))
    err, bound = np.abs(rounded - (P_new @ R + shift)).max(), (2.0 ** -24 * 0.5 * delta @ np.abs(P)).max()
    print("delta rounded to float32: %.3g (bound %.3g)" % (err, bound))
    assert err <= bound
    # embedded rows on a line in the plane: finite, and the null direction stays at the mean's
    line = np.stack([np.linspace(-1, 1, 20), np.full(20, 3.0)], 1)
    got, _ = ref.triangulate(line, ref.d2_rows(np.array([[0.25, 3.0]]), line))
    assert np.all(np.isfinite(got)) and np.abs(got - np.array([[0.25, 3.0]])).max() <= 1e-12


# ------------------------------------------------------------------------------------------------------ the surface
def test_signature_defaults():
    assert inspect.signature(pymde_amd.DenseMDE.__init__).parameters["init"].default == "random"
    assert list(inspect.signature(pymde_amd.DenseMDE.__init__).parameters)[-1] == "init"
    assert inspect.signature(pymde_amd.LandmarkMDE.__init__).parameters["init"].default == "random"
    assert inspect.signature(pymde_amd.preserve_distances).parameters["init"].default == "random"
    weighted = inspect.signature(pymde_amd.DensePlacement.weighted).parameters["init"]
    assert weighted.default == "neighbors" and weighted.kind is inspect.Parameter.KEYWORD_ONLY
    assert inspect.signature(pymde_amd.DensePlacement.initialization).parameters["method"].default is None
    assert "init" not in inspect.signature(pymde_amd.DensePlacement.__init__).parameters
    sig = inspect.signature(pymde_amd.classical_mds)
    assert list(sig.parameters) == ["data", "embedding_dim", "distance_matrix", "metric", "deviation_scale",
                                    "n_oversamples", "n_iter", "seed", "test_matrix", "device"]
    assert [sig.parameters[p].default for p in ("embedding_dim", "metric", "deviation_scale", "n_oversamples",
                                                "n_iter", "seed")] == [2, "euclidean", 1.0, 10, 4, 0]
    assert pymde_amd.classical_mds is classical.classical_mds
    assert callable(pymde_amd.DenseMDE.classical_initialization) and callable(pymde_amd.LandmarkMDE.initialization)


def test_errors_that_need_no_device():
    data = np.random.default_rng(0).standard_normal((40, 6)).astype(np.float32)
    D = np.abs(data @ data.T)
    with pytest.raises(ValueError, match="exactly one"):
        pymde_amd.classical_mds()
    with pytest.raises(ValueError, match="exactly one"):
        pymde_amd.classical_mds(data, distance_matrix=D)
    for bad in (0, 9):
        with pytest.raises(ValueError, match="embedding_dim"):
            pymde_amd.classical_mds(distance_matrix=D, embedding_dim=bad)
    with pytest.raises(ValueError, match="n_oversamples"):
        pymde_amd.classical_mds(distance_matrix=D, embedding_dim=8, n_oversamples=25)       # 33 > 32
    with pytest.raises(ValueError, match="n_oversamples"):
        pymde_amd.classical_mds(distance_matrix=D[:10, :10], embedding_dim=2, n_oversamples=8)   # 10 > n - 1
    with pytest.raises(ValueError, match="square"):
        pymde_amd.classical_mds(distance_matrix=D[:10])
    with pytest.raises(ValueError, match="manhattan"):
        pymde_amd.classical_mds(data, metric="manhattan")
    with pytest.raises(ValueError, match="deviation_scale"):
        pymde_amd.classical_mds(data, deviation_scale=0.0)
    assert classical.check_arguments(300, 3) == (3, 13) and classical.check_arguments(12, 2, 9) == (2, 11)
    # the problems
    with pytest.raises(ValueError, match="init"):
        pymde_amd.DenseMDE(data, init="spectral")
    anchored = pymde_amd.Anchored(torch.tensor([0, 1]), torch.zeros(2, 2))
    with pytest.raises(ValueError, match="Anchored"):
        pymde_amd.DenseMDE(data, constraint=anchored, init="classical")
    with pytest.raises(ValueError, match="init"):
        pymde_amd.LandmarkMDE(data, 10, init="pca")
    with pytest.raises(ValueError, match="init"):
        pymde_amd.preserve_distances(data, init="classical")            # the edge-list path
    with pytest.raises(ValueError, match="init"):
        pymde_amd.preserve_distances(data, dense=True, init="neighbors")
    with pytest.raises(ValueError, match="init"):
        pymde_amd.DensePlacement.weighted(data, np.zeros((40, 2), np.float32), data[:5], weights=None, init="classical")
    assert dense.check_init("classical") == "classical"
    assert dense.check_init("triangulation", dense.PLACEMENT_INITS) == "triangulation"
    # triangulate: the source and the shape of X_old
    X_old = torch.zeros(6, 2)
    with pytest.raises(ValueError, match="exactly one source"):
        classical.triangulate(X_old)
    with pytest.raises(ValueError, match="exactly one source"):
        classical.triangulate(X_old, Q=torch.zeros(3, 4), C=torch.zeros(6, 4), Dm=torch.zeros(3, 6))
    with pytest.raises(ValueError, match="one embedding vector"):
        classical.triangulate(X_old, Dm=torch.zeros(3, 5))
    with pytest.raises(ValueError, match="X_old"):
        classical.triangulate(torch.zeros(6, 9), Dm=torch.zeros(3, 6))

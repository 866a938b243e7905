"""``pymde_amd.classical_mds`` and the classical start of ``DenseMDE`` on the GPU, against the float64 reference
(tests/_classical_reference.py) on the inputs as the device holds them.

Tolerances.  The device runs the float64 replay's iteration with its blocks rounded to float32 between the steps:
a perturbation of ``B`` on the iterated subspace of the order ``E = (r + 2) 2^-24 lambda_1`` (r columns, and the
float32 deviations themselves).  Eigenvalues move by at most ``E``; the Gram matrix ``X X^T`` of the kept part moves
by at most ``E (1 + 2 lambda_1 / gap)``, ``gap`` the distance from the last kept eigenvalue to the first dropped one
(Davis-Kahan for the kept invariant subspace).  Against the EXACT solution the replay's own distance to it, which
the reference alone shows on that input, is added (tests/test_classical_host.py: at most 3e-8 of the largest Gram
entry, on the cycle).  Every test prints what it observed beside the bound.

Observed on an MI355X (n = 300, r = d + 10), device against the float64 replay from the same start block: eigenvalues
within 4.4e-8 (planted), 3.0e-8 (cosine), 3.4e-8 (cycle) of lambda_1, bound (r + 2) 2^-24 = 8.9e-7: a margin of 20;
Gram matrices within 2.3e-3 (planted, bound 3.0), 4.0e-7 (cosine, bound 9.8e-4), 2.0e-3 (cycle, bound 1.9): the
Davis-Kahan factor is a worst case, the margin is 500 and more.  Against the exact solution: cosine eigenvalues
within 1.4e-6 (bound 9.4e-5), 150 points of R^3 squared distances within 6.3e-6 (bound 2.1e-3).
"""
import functools

import numpy as np
import pytest
import scipy.sparse
import torch

import pymde_amd
from pymde_amd import quality
from pymde_amd.functions import losses

import _classical_reference as ref

pytestmark = pytest.mark.gpu

DEVICE = "cuda"


def eig_bound(lam1, r):
    return (r + 2) * 2.0 ** -24 * lam1


def gram_bound(lam1, gap, r):
    return eig_bound(lam1, r) * (1.0 + 2.0 * lam1 / gap)


def _gram_error(X, Y):
    return float(np.abs(X @ X.T - Y @ Y.T).max())


@functools.lru_cache(maxsize=None)
def _cosine_case():
    """The shifted planted rows under the cosine distance: the prepared rows read back from the device, their S, the
    exact solution at d = 3 and all eigenvalues."""
    data = ref.planted_cosine_rows(300)
    A = quality._self_rows(torch.as_tensor(data), "cosine", torch.device(DEVICE, 0), "data").cpu().numpy()
    S = ref.S_from_rows(A.astype(np.float64), 1)
    return data, S, ref.classical_exact(S, 3)


def test_distance_matrix_of_points_in_r3():
    P = ref.points(150, 3, seed=1)
    D = ref.pair_distances(P).astype(np.float32)
    fit = pymde_amd.classical_mds(distance_matrix=D, embedding_dim=3)
    X = fit.X.double().cpu().numpy()
    Xe, le, _, evals = ref.classical_exact(ref.S_from_matrix(D), 3)
    lam = fit.eigenvalues.cpu().numpy()
    bound = gram_bound(le[0], le[2] - np.sort(evals)[::-1][3], 13)
    err = _gram_error(X, Xe)
    d2_err = float(np.abs(ref.d2_rows(X, X) - D.astype(np.float64) ** 2).max())
    print("R^3: eigenvalue error %.3g (bound %.3g), Gram error %.3g (bound %.3g), squared distances %.3g (bound %.3g)"
          % (np.abs(lam - le).max(), eig_bound(le[0], 13), err, bound, d2_err, 4 * bound))
    assert fit.X.dtype == torch.float32 and fit.X.is_cuda and fit.eigenvalues.dtype == torch.float64
    assert np.abs(lam - le).max() <= eig_bound(le[0], 13) and np.all(np.diff(lam) <= 0)
    assert err <= bound and d2_err <= 4 * bound
    assert np.abs(X.mean(0)).max() <= 1e-6 * np.abs(X).max()
    assert abs(float(fit.total) - evals.sum()) <= 1e-6 * evals.sum() and not fit.negative
    # the sign rule: the entry of largest magnitude of every column is positive
    assert np.all(X[np.abs(X).argmax(0), np.arange(3)] > 0)
    # deviation_scale multiplies the configuration
    scaled = pymde_amd.classical_mds(distance_matrix=D, embedding_dim=3, deviation_scale=2.5)
    assert _gram_error(scaled.X.double().cpu().numpy(), 2.5 * Xe) <= 6.25 * bound
    assert np.abs(scaled.eigenvalues.cpu().numpy() - 6.25 * le).max() <= 6.25 * eig_bound(le[0], 13)


def test_cosine_against_the_exact_solution():
    data, S, (Xe, le, negative, evals) = _cosine_case()
    fit = pymde_amd.classical_mds(data, 3, metric="cosine")
    X, lam = fit.X.double().cpu().numpy(), fit.eigenvalues.cpu().numpy()
    Xr = ref.replay(S, np.random.default_rng(7).standard_normal((300, 13)), 3)[0]
    replay_gap = _gram_error(Xr, Xe)
    bound = gram_bound(le[0], le[2] - np.sort(evals)[::-1][3], 13) + replay_gap
    err = _gram_error(X, Xe)
    print("cosine: eigenvalues %s (exact %s), error %.3g (bound %.3g); Gram error %.3g (bound %.3g, the replay's own "
          "%.3g); smallest eigenvalue of B %.3g" % (lam, le, np.abs(lam - le).max(), eig_bound(le[0], 13), err, bound,
                                                    replay_gap, evals.min()))
    assert np.abs(lam - le).max() <= eig_bound(le[0], 13)
    assert err <= bound
    assert abs(float(fit.total) - evals.sum()) <= 1e-6 * np.abs(evals).sum()
    assert evals.min() < 0 and not negative and not fit.negative      # B is indefinite; the three kept are positive


def test_negative_is_set_when_a_kept_eigenvalue_is_clipped():
    """At d = 8 without oversampling the block of 8 holds the eigenvalues of largest magnitude, the negative ones
    among them: five of the kept eight are clipped, as in the float64 replay from the same start block."""
    data, S, _ = _cosine_case()
    omega = np.random.default_rng(8).standard_normal((300, 8)).astype(np.float32)
    _, lr, negative, _ = ref.replay(S, omega.astype(np.float64), 8)
    fit = pymde_amd.classical_mds(data, 8, metric="cosine", n_oversamples=0, test_matrix=omega)
    lam = fit.eigenvalues.cpu().numpy()
    print("d = 8, r = 8: device %s, replay %s" % (lam, lr))
    assert negative and fit.negative
    assert (lam == 0).any() and (lr == 0).any() and np.all(lam[:3] > 0)
    assert bool((fit.X[:, torch.as_tensor(lam == 0)] == 0).all())
    assert np.abs(lam[:3] - lr[:3]).max() <= eig_bound(lr[0], 8)


def test_cycle_is_a_circle():
    n = 300
    D = ref.cycle_matrix(n)
    fit = pymde_amd.classical_mds(distance_matrix=D, embedding_dim=2)
    X, lam = fit.X.double().cpu().numpy(), fit.eigenvalues.cpu().numpy()
    S = ref.S_from_matrix(D)
    Xe, le, _, evals = ref.classical_exact(S, 2)
    Xr, lr, _, _ = ref.replay(S, np.random.default_rng(7).standard_normal((n, 12)), 2)
    replay_gap = _gram_error(Xr, Xe)
    bound = gram_bound(le[0], le[1] - np.sort(evals)[::-1][2], 12) + replay_gap
    err = _gram_error(X, Xe)            # the top eigenvalue is double: Gram matrices, never eigenvectors
    radius = np.linalg.norm(X, axis=1)
    print("cycle: eigenvalues %s (exact %.9g twice); Gram error %.3g (bound %.3g, the replay's own %.3g); radius "
          "%.6g +- %.3g" % (lam, le[0], err, bound, replay_gap, radius.mean(), np.abs(radius - radius.mean()).max()))
    assert np.abs(lam - le).max() <= eig_bound(le[0], 12) + np.abs(lr - le).max()
    assert err <= bound
    # |r_i^2 - R^2| = |G_ii - G_ii exact|
    assert np.abs(radius ** 2 - le[0] * 2.0 / n).max() <= bound
    assert evals.min() < 0 and not fit.negative


def test_euclidean_data_are_the_principal_component_scores():
    data = torch.as_tensor(ref.planted_rows(300))
    fit = pymde_amd.classical_mds(data, 3)
    pc = pymde_amd.preprocess.principal_components(data, 3)
    assert torch.equal(fit.X, pc.scores)
    assert torch.equal(fit.eigenvalues, pc.singular_values ** 2) and not fit.negative
    le = ref.classical_exact(ref.S_from_rows(data.double().numpy()), 3)[1]
    assert np.abs(fit.eigenvalues.cpu().numpy() - le).max() <= 1e-5 * le[0]
    assert abs(float(fit.total) - ref.S_from_rows(data.double().numpy()).sum() / 600.0) <= 1e-5 * float(fit.total)
    # sparse rows take the randomized route, with the same seed
    sp = scipy.sparse.random(300, 50, density=0.2, random_state=3, dtype=np.float32, format="csr")
    fit = pymde_amd.classical_mds(sp, 2, seed=5)
    assert torch.equal(fit.X, pymde_amd.preprocess.principal_components(sp, 2, seed=5).scores)


@pytest.mark.parametrize("case", ["planted", "cosine", "cycle"])
def test_test_matrix_makes_the_device_follow_the_replay(case):
    n = 300
    if case == "cycle":
        source, d = dict(distance_matrix=ref.cycle_matrix(n)), 2
        S = ref.S_from_matrix(source["distance_matrix"])
    elif case == "cosine":
        data, S, _ = _cosine_case()
        source, d = dict(data=data, metric="cosine"), 3
    else:
        # (Euclidean deviations through the walk: as a matrix of distances, since Euclidean rows take the PCA route)
        D = ref.pair_distances(ref.planted_rows(n).astype(np.float64)).astype(np.float32)
        source, d, S = dict(distance_matrix=D), 3, ref.S_from_matrix(D)
    r = d + 10
    omega = np.random.default_rng(11).standard_normal((n, r)).astype(np.float32)
    Xr, lr, _, _ = ref.replay(S, omega.astype(np.float64), d)
    fit = pymde_amd.classical_mds(embedding_dim=d, test_matrix=omega, **source)
    again = pymde_amd.classical_mds(embedding_dim=d, test_matrix=torch.as_tensor(omega), **source)
    assert torch.equal(fit.X, again.X) and torch.equal(fit.eigenvalues, again.eigenvalues)
    X, lam = fit.X.double().cpu().numpy(), fit.eigenvalues.cpu().numpy()
    evals = np.sort(np.linalg.eigvalsh(ref.B_matrix(S)))[::-1]
    bound = gram_bound(lr[0], lr[d - 1] - evals[d], r)
    err = _gram_error(X, Xr)
    print("%s: device against the float64 replay: eigenvalues %.3g of lambda_1 (bound %.3g), Gram %.3g (bound %.3g)"
          % (case, np.abs(lam - lr).max() / lr[0], eig_bound(1.0, r), err, bound))
    assert np.abs(lam - lr).max() <= eig_bound(lr[0], r)
    assert err <= bound
    with pytest.raises(ValueError, match="test_matrix"):
        pymde_amd.classical_mds(embedding_dim=d, test_matrix=omega[:, :5], **source)


def test_rank_one_input_gives_a_zero_column():
    t = np.sort(ref.points(120, 1, seed=5)[:, 0])
    D = np.abs(t[:, None] - t[None, :]).astype(np.float32)
    fit = pymde_amd.classical_mds(distance_matrix=D, embedding_dim=2)
    lam = fit.eigenvalues.cpu().numpy()
    assert lam[0] > 0 and lam[1] == 0.0 and not fit.negative
    assert bool((fit.X[:, 1] == 0).all()) and bool(torch.isfinite(fit.X).all())
    x = fit.X[:, 0].double().cpu().numpy()
    want = t - t.mean()
    assert np.abs(x * np.sign(x[-1] * want[-1]) - want).max() <= 1e-5 * np.abs(want).max()


# ------------------------------------------------------------------------------------------------ the start of DenseMDE
def _r3_problem(**keywords):
    P = ref.points(150, 3, seed=1)
    D = ref.pair_distances(P).astype(np.float32)
    return pymde_amd.DenseMDE(distance_matrix=D, embedding_dim=3, loss=losses.Quadratic, **keywords), D


def test_classical_start_of_an_exact_configuration():
    mde, D = _r3_problem(init="classical")
    X0 = mde.classical_initialization()
    value, scale = float(mde.average_distortion(X0)), float((D.astype(np.float64) ** 2).sum() / (150 * 149))
    print("average distortion of the classical start %.3g = %.3g of the mean D^2" % (value, value / scale))
    assert tuple(X0.shape) == (150, 3) and X0.dtype == torch.float32
    assert value <= 1e-6 * scale
    mde.embed()
    print("embed() from it: %d iterations, value %.3g" % (mde.solve_stats.iterations, mde.value))
    assert mde.solve_stats.iterations <= 10 and mde.value <= 1e-6 * scale
    # a random start needs the unfolding the classical one skips
    pymde_amd.seed(0)
    random, _ = _r3_problem()
    assert random.init == "random" and float(random.average_distortion(
        random.constraint.initialization(150, 3, random.device))) > 0.1 * scale


def test_classical_start_satisfies_standardized():
    mde, _ = _r3_problem(init="classical", constraint=pymde_amd.Standardized())
    X0 = mde.classical_initialization().double()
    assert float(X0.mean(0).abs().max()) <= 1e-5
    assert float((X0.t() @ X0 / 150 - torch.eye(3, dtype=torch.float64, device=X0.device)).abs().max()) <= 1e-4
    # a flat column is lifted off the saddle before the projection: points on a plane, embedded in R^3
    P = np.concatenate([ref.points(100, 2, seed=6), np.zeros((100, 1))], 1)
    flat = pymde_amd.DenseMDE(distance_matrix=ref.pair_distances(P).astype(np.float32), embedding_dim=3,
                              loss=losses.Quadratic, init="classical")
    X0 = flat.classical_initialization()
    assert bool(torch.isfinite(X0).all()) and float(X0[:, 2].abs().max()) > 0
    assert float(X0[:, 2].abs().max()) <= 1e-2 * float(X0[:, 0].abs().max())


def test_random_init_is_the_constraints_own_draw():
    mde, _ = _r3_problem()
    pymde_amd.seed(0)
    X_default = mde.embed(max_iter=3).clone()
    pymde_amd.seed(0)
    start = mde.constraint.initialization(150, 3, mde.device)
    assert torch.equal(mde.embed(start, max_iter=3), X_default)
    explicit, _ = _r3_problem(init="random")
    pymde_amd.seed(0)
    assert torch.equal(explicit.embed(max_iter=3), X_default)


def test_classical_init_needs_every_pair():
    D = ref.pair_distances(ref.points(30, 2, seed=2)).astype(np.float32)
    W = np.ones((30, 30), dtype=np.float32)
    W[3, 9] = W[9, 3] = 0.0
    with pytest.raises(ValueError, match="every pair"):
        pymde_amd.DenseMDE(distance_matrix=D, weights=W, init="classical")
    # power weights are ignored by the start and used by the solve
    mde = pymde_amd.DenseMDE(distance_matrix=D, loss=losses.Quadratic, weights=1.0, init="classical")
    plain = pymde_amd.DenseMDE(distance_matrix=D, loss=losses.Quadratic, init="classical")
    assert torch.equal(mde.classical_initialization(), plain.classical_initialization())
    # the recipe hands `init` on
    data = ref.planted_rows(80, 12)
    assert pymde_amd.preserve_distances(data, dense=True, init="classical").init == "classical"
    assert pymde_amd.preserve_distances(data, landmarks=20, init="classical", seed=0).landmark_problem.init == \
        "classical"

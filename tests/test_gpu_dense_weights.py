"""The ``weights=`` of the dense problems on the GPU (pymde_amd.dense): Sammon mapping, masked
problems, ``DensePlacement.weighted(weights=...)`` under both solvers, ``LandmarkMDE(weights=p)`` and
``DenseMDE.from_graph``, each against the edge-list ``MDE`` over the same pairs with the same weights (the edge-list path is the yardstick: its
kernels are checked against the oracle elsewhere).  Tolerances: LOSS_RTOL and assert_grad_close of tests/conftest.py;
the embed() bounds are those of tests/test_gpu_dense_mde.py and tests/test_gpu_rows_place.py."""
import functools
import math

import numpy as np
import pytest
import torch

from conftest import LOSS_RTOL
from test_gpu_dense_mde import _compare, _value_and_grad

pytestmark = pytest.mark.gpu
DEV = "cuda"
N, NF = 150, 20
N_OLD, N_NEW = 120, 70
_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _data():
    """(data [N, NF] float32, X [N, 2] float32, D float64 [N, N] of the float32 rows, a symmetric bool mask that keeps
    about 70 % of the pairs and at least one per row)."""
    def make():
        rng = np.random.default_rng(41)
        data = rng.standard_normal((N, NF)) * rng.uniform(0.5, 2.0, NF)
        data = (data - data.mean(0)).astype(np.float32)
        X = rng.standard_normal((N, 2)) * 3.0
        D = np.sqrt(((data[:, None, :].astype(np.float64) - data[None, :, :]) ** 2).sum(-1))
        U = np.triu(rng.random((N, N)) < 0.7, 1)
        mask = U | U.T
        assert (mask.sum(1) >= 1).all()
        return data, (X - X.mean(0)).astype(np.float32), D, mask
    return _cached("data", make)


def _edge_problem(n, pairs, deviations, loss, weights=None, constraint=None):
    """The edge-list MDE over `pairs` [m, 2] with float32 deviations (and per-edge weights for a weighted loss)."""
    import pymde_amd
    edges = torch.as_tensor(np.asarray(pairs, dtype=np.int64)).to(DEV)
    dev = torch.as_tensor(np.asarray(deviations, dtype=np.float32)).to(DEV)
    f = loss(dev) if weights is None else loss(dev, torch.as_tensor(np.asarray(weights, dtype=np.float32)).to(DEV))
    return pymde_amd.MDE(n, 2, edges, f, constraint=constraint)


def _pairs_of(mask):
    iu, ju = np.triu_indices(mask.shape[0], 1)
    sel = mask[iu, ju]
    return np.stack([iu[sel], ju[sel]], 1)


# ---------------------------------------------------------------- 1. Sammon mapping
@pytest.mark.parametrize("form", ["matrix", "power"])
def test_sammon_mapping_is_the_weighted_quadratic_of_the_edge_list(form):
    import pymde_amd
    data, X, D, _ = _data()
    pairs = _pairs_of(np.ones((N, N), dtype=bool))
    dev = D[pairs[:, 0], pairs[:, 1]]
    edge = _edge_problem(N, pairs, dev, pymde_amd.losses.WeightedQuadratic, weights=1.0 / dev)
    with np.errstate(divide="ignore"):
        weights = np.where(np.eye(N, dtype=bool), 0.0, 1.0 / D).astype(np.float32) if form == "matrix" else 1
    dense = pymde_amd.DenseMDE(data, loss=pymde_amd.losses.Quadratic, weights=weights)
    assert dense.p == N * (N - 1) // 2 == int(edge.p)
    _compare("Sammon, %s form, data" % form, _value_and_grad(dense, X), _value_and_grad(edge, X))
    dense = pymde_amd.DenseMDE(distance_matrix=D, loss=pymde_amd.losses.Quadratic, weights=weights)
    _compare("Sammon, %s form, distance matrix" % form, _value_and_grad(dense, X), _value_and_grad(edge, X))
    # the weighted loss takes the weight in place of its default 1 / D^2
    dense = pymde_amd.DenseMDE(data, loss=pymde_amd.losses.WeightedQuadratic, weights=weights)
    _compare("WeightedQuadratic, %s form" % form, _value_and_grad(dense, X), _value_and_grad(edge, X))


# ---------------------------------------------------------------- 2. a masked problem
@pytest.mark.parametrize("loss", ["Absolute", "Quadratic", "Huber"])
def test_masked_problem_equals_the_edge_list_problem_over_the_kept_pairs(loss):
    import pymde_amd
    data, X, D, mask = _data()
    pairs = _pairs_of(mask)
    L = getattr(pymde_amd.losses, loss)
    if loss == "Huber":
        L = functools.partial(L, threshold=3.0)                  # both branches: |E - D| is of the order of 5
    edge = _edge_problem(N, pairs, D[pairs[:, 0], pairs[:, 1]], L)
    Dm = np.where(mask, D, np.nan)                               # unknown where the pair is missing
    np.fill_diagonal(Dm, 0.0)
    for label, dense in (("data", pymde_amd.DenseMDE(data, loss=L, weights=mask)),
                         ("distance matrix", pymde_amd.DenseMDE(distance_matrix=Dm, loss=L,
                                                                weights=torch.as_tensor(mask.astype(np.float64))))):
        assert dense.p == len(pairs) == int(edge.p) and dense.n_all_pairs == N * (N - 1) // 2
        assert "of %d" % dense.n_all_pairs in str(dense) and str(dense.p) in str(dense)
        _compare("masked %s, %s" % (loss, label), _value_and_grad(dense, X), _value_and_grad(edge, X))
    # item_distortions: the edge-list per-edge distortions averaged per item
    per_edge = edge.distortions(torch.as_tensor(X).to(DEV)).double().cpu().numpy()
    sums = np.zeros(N)
    np.add.at(sums, pairs[:, 0], per_edge)
    np.add.at(sums, pairs[:, 1], per_edge)
    want = sums / mask.sum(1)
    items = dense.item_distortions(torch.as_tensor(X))
    assert items.dtype == torch.float32 and items.shape == (N,)
    worst = float(np.abs(items.double().cpu().numpy() - want).max() / want.mean())
    print("item_distortions: worst error %.3g of the mean item (bound %.3g)" % (worst, LOSS_RTOL))
    assert worst <= LOSS_RTOL


def test_embed_of_a_masked_problem_reaches_what_the_edge_list_problem_reaches():
    import pymde_amd
    rng = np.random.default_rng(42)
    data = rng.standard_normal((N, 2)) * np.array([3.0, 1.0])
    data = (data - data.mean(0)).astype(np.float32)
    D = np.sqrt(((data[:, None, :].astype(np.float64) - data[None, :, :]) ** 2).sum(-1))
    U = np.triu(rng.random((N, N)) < 0.7, 1)                     # 30 % of the pairs are missing
    mask = U | U.T
    assert (mask.sum(1) >= 1).all() and 0.25 < 1.0 - mask.sum() / (N * (N - 1.0)) < 0.35
    pairs = _pairs_of(mask)
    start = data + (0.1 * data.std() * rng.standard_normal((N, 2))).astype(np.float32)
    start = torch.as_tensor(start - start.mean(0)).to(DEV)
    kwargs = dict(eps=1e-6, max_iter=200)
    quadratic = pymde_amd.losses.Quadratic
    edge = _edge_problem(N, pairs, D[pairs[:, 0], pairs[:, 1]], quadratic, constraint=pymde_amd.Centered())
    edge.embed(X=start.clone(), **kwargs)
    dense = pymde_amd.DenseMDE(data, loss=quadratic, constraint=pymde_amd.Centered(), weights=mask)
    initial = float(dense.average_distortion(start))
    X = dense.embed(X=start.clone(), **kwargs)
    print("initial value %.6g; final value dense %.6g in %d iterations, edge list %.6g in %d iterations"
          % (initial, dense.value, dense.solve_stats.iterations, edge.value, edge.solve_stats.iterations))
    assert dense.solve_stats.iterations > 0
    assert dense.value <= 1.05 * edge.value + 1e-6 * initial
    assert abs(float(dense.average_distortion()) - dense.value) <= 1e-4 * initial
    again = pymde_amd.DenseMDE(data, loss=quadratic, constraint=pymde_amd.Centered(), weights=mask)
    assert torch.equal(again.embed(X=start.clone(), **kwargs), X) and again.value == dense.value


def test_every_value_error_of_the_validation():
    import pymde_amd
    data, _, D, mask = _data()
    W = mask.astype(np.float32)

    def bad(match, matrix, **kwargs):
        with pytest.raises(ValueError, match=match):
            pymde_amd.DenseMDE(kwargs.pop("data", data), weights=matrix, **kwargs)
    bad("shape", W[:, :-1])
    bad("shape", W[:-1, :-1])
    V = W.copy(); V[3, 70] = np.nan
    bad("not finite", V)
    V = W.copy(); V[3, 70] = np.inf
    bad("not finite", V)
    V = W.copy(); V[3, 70] = -1.0
    bad("non-negative", V)
    V = W.copy(); V[3, 70] = V[70, 3] + 0.5
    bad("not symmetric", V)
    V = W.copy(); V[9, :] = 0.0; V[:, 9] = 0.0
    bad("without a pair", V)
    i, j = _pairs_of(mask)[5]
    for value in (np.nan, np.inf, -1.0):
        E = D.copy(); E[i, j] = E[j, i] = value
        bad("`distance_matrix` is NaN, infinite or negative", W, data=None, distance_matrix=E)
    E = D.copy(); E[i, j] += 1.0
    bad("`distance_matrix` is not symmetric on the pairs", W, data=None, distance_matrix=E)
    # the same entries under a zero weight are nobody's business
    E = D.copy()
    E[~mask] = np.nan
    assert pymde_amd.DenseMDE(distance_matrix=E, weights=W).p == int(np.triu(mask, 1).sum())
    # a tiny asymmetry (a float32 product of two roundings) passes, by the rule of SYMMETRY_RTOL
    V = W.copy(); V[3, 70] = V[70, 3] = 1.0; V[3, 70] += 5e-6
    assert pymde_amd.DenseMDE(data, weights=V).p >= int(np.triu(mask, 1).sum())
    # without weights a distance matrix is still checked whole, with the messages it had
    with pytest.raises(ValueError, match="`distance_matrix` is not finite"):
        pymde_amd.DenseMDE(distance_matrix=E)
    with pytest.raises(ValueError, match="`distance_matrix` is not finite"):
        pymde_amd.DenseMDE(distance_matrix=E, weights=1)
    # the rectangular problem: shape, a row without a pair, an unknown kept deviation; no symmetry is asked for
    X_old = torch.zeros((N_OLD, 2))
    R = np.ones((N_NEW, N_OLD), dtype=np.float32)
    Dr = D[:N_NEW, :N_OLD].copy()
    with pytest.raises(ValueError, match="shape"):
        pymde_amd.DensePlacement.weighted(None, X_old, None, distance_matrix=Dr, weights=R.T)
    V = R.copy(); V[4, :] = 0.0
    with pytest.raises(ValueError, match="without a pair"):
        pymde_amd.DensePlacement.weighted(None, X_old, None, distance_matrix=Dr, weights=V)
    E = Dr.copy(); E[4, 7] = np.nan
    with pytest.raises(ValueError, match="NaN, infinite or negative"):
        pymde_amd.DensePlacement.weighted(None, X_old, None, distance_matrix=E, weights=R)
    V = R.copy(); V[4, 7] = 0.0
    assert pymde_amd.DensePlacement.weighted(None, X_old, None, distance_matrix=E, weights=V).p == N_NEW * N_OLD - 1


# ---------------------------------------------------------------- 3. DensePlacement.weighted(weights=...)
def _placement_data():
    def make():
        rng = np.random.default_rng(43)
        rows = rng.standard_normal((N_OLD + N_NEW, NF)) * rng.uniform(0.5, 2.0, NF)
        rows = (rows - rows[:N_OLD].mean(0)).astype(np.float32)
        X = (rng.standard_normal((N_OLD + N_NEW, 2)) * 3.0).astype(np.float32)
        D = np.sqrt(((rows[N_OLD:, None, :].astype(np.float64) - rows[None, :N_OLD, :]) ** 2).sum(-1))
        mask = rng.random((N_NEW, N_OLD)) < 0.7
        mask[np.arange(N_NEW), rng.integers(0, N_OLD, N_NEW)] = True
        return rows[:N_OLD], rows[N_OLD:], X[:N_OLD], X[N_OLD:], D, mask
    return _cached("placement", make)


def _bipartite(mask):
    i, j = np.nonzero(mask)
    return np.stack([j, N_OLD + i], 1), i, j


def _edge_value_and_grad(edge, X_old, X_new):
    Xg = torch.as_tensor(np.concatenate([X_old, X_new])).to(DEV).requires_grad_(True)
    value = edge.average_distortion(Xg)
    value.backward()
    return float(value.detach()), Xg.grad.cpu().numpy()[N_OLD:]


def test_placement_with_both_forms_equals_the_bipartite_edge_list_problem():
    import pymde_amd
    data, new, X_old, X_new, D, mask = _placement_data()
    losses = pymde_amd.losses
    # the power form: Sammon's weights over every (new, old) pair
    pairs, i, j = _bipartite(np.ones_like(mask))
    edge = _edge_problem(N_OLD + N_NEW, pairs, D[i, j], losses.WeightedQuadratic, weights=1.0 / D[i, j])
    place = pymde_amd.DensePlacement.weighted(data, X_old, new, loss=losses.Quadratic, weights=1)
    assert place.p == N_NEW * N_OLD
    _compare("placement, weights=1", _value_and_grad(place, X_new), _edge_value_and_grad(edge, X_old, X_new))
    # the matrix form: continuous weights with zeros, from data and from a matrix with unknown entries
    rng = np.random.default_rng(44)
    W = (mask * rng.uniform(0.2, 3.0, mask.shape)).astype(np.float32)
    pairs, i, j = _bipartite(mask)
    edge = _edge_problem(N_OLD + N_NEW, pairs, D[i, j], losses.WeightedQuadratic, weights=W[i, j])
    weighted = pymde_amd.DensePlacement.weighted
    for label, place in (("data", weighted(data, X_old, new, loss=losses.Quadratic, weights=W)),
                         ("distance matrix", weighted(None, X_old, None, loss=losses.Quadratic,
                                                      distance_matrix=np.where(mask, D, np.inf), weights=W))):
        assert place.p == int(mask.sum()) == int(edge.p) and "of %d" % (N_NEW * N_OLD) in str(place)
        _compare("placement, weight matrix, %s" % label, _value_and_grad(place, X_new),
                 _edge_value_and_grad(edge, X_old, X_new))
    items = place.item_distortions(torch.as_tensor(X_new)).double().cpu().numpy()
    value = float(place.average_distortion(torch.as_tensor(X_new).to(DEV)))
    assert abs((items * mask.sum(1)).sum() - place.p * value) <= LOSS_RTOL * place.p * value
    assert torch.isfinite(place.initialization()).all()


def test_rows_solver_on_a_masked_placement_reports_the_joint_problems_value():
    import pymde_amd
    rng = np.random.default_rng(45)
    rows = rng.standard_normal((N_OLD + N_NEW, 2)) * np.array([3.0, 1.0])
    rows = (rows - rows[:N_OLD].mean(0)).astype(np.float32)
    data, new = rows[:N_OLD], rows[N_OLD:]
    mask = rng.random((N_NEW, N_OLD)) < 0.7
    mask[:, :3] = True                                           # three known distances fix a position in the plane
    # noisy dissimilarities: the minimum is not zero, so a wrong rescaling of the reported value shows
    D = np.sqrt(((new[:, None, :].astype(np.float64) - data[None, :, :]) ** 2).sum(-1))
    D = D * rng.uniform(0.9, 1.1, D.shape)
    X_old = torch.as_tensor(data).to(DEV)
    start = torch.as_tensor(new + (0.1 * rows.std() * rng.standard_normal((N_NEW, 2))).astype(np.float32)).to(DEV)
    kwargs = dict(eps=1e-6, max_iter=200)
    quadratic = pymde_amd.losses.Quadratic

    def problem():
        return pymde_amd.DensePlacement.weighted(None, X_old, None, loss=quadratic, weights=mask,
                                                 distance_matrix=np.where(mask, D, np.nan))
    joint = problem()
    initial = float(joint.average_distortion(start))
    joint.embed(X=start.clone(), **kwargs)
    place = problem()
    X = place.embed(X=start.clone(), solver="rows", **kwargs)
    stats = place.solve_stats
    at_X = float(place.average_distortion(X))
    print("initial %.6g; joint %.6g in %d iterations; rows %.6g in %d sweeps (average_distortion(X) %.6g), residual "
          "norm %.3g against %.3g" % (initial, joint.value, joint.solve_stats.iterations, place.value, stats.iterations,
                                      at_X, place.residual_norm, joint.residual_norm))
    assert place.p == int(mask.sum()) < N_NEW * N_OLD
    assert joint.value > 1e-3 * initial                          # the minimum is not zero
    assert place.value <= 1.05 * joint.value + 1e-6 * initial
    assert abs(place.value - at_X) <= 1e-4 * at_X                # what catches a wrong rescaling
    assert place.value == stats.average_distortions[-1] and place.residual_norm == stats.residual_norms[-1]
    # the residual norm is the Frobenius norm of the joint gradient G / p, as for the unmasked placement: checked two
    # sweeps in, where the gradient is far from zero and GRAD_RTOL of itself means something
    short = problem()
    Xs = short.embed(X=start.clone(), solver="rows", eps=1e-6, max_iter=2)
    Xg = Xs.clone().requires_grad_(True)
    short.average_distortion(Xg).backward()
    want = float(Xg.grad.double().square().sum().sqrt())
    print("residual norm after two sweeps %.6g against |G / p|_F %.6g" % (short.residual_norm, want))
    assert abs(short.residual_norm - want) <= 1e-4 * want
    assert abs(short.value - float(short.average_distortion(Xs))) <= 1e-4 * short.value


# ---------------------------------------------------------------- 4. landmarks
def test_landmarks_carry_the_weight_through_both_stages():
    import pymde_amd
    from pymde_amd import dense as dense_mod
    data, start, _, _ = _data()
    quadratic = pymde_amd.losses.Quadratic
    kwargs = dict(X=torch.as_tensor(start), eps=1e-5, max_iter=30)
    direct = pymde_amd.LandmarkMDE(data, 60, loss=quadratic, seed=3, weights=1)
    recipe = pymde_amd.preserve_distances(data, landmarks=60, loss=quadratic, seed=3, weights=1)
    plain = pymde_amd.preserve_distances(data, landmarks=60, loss=quadratic, seed=3)
    for problem in (direct, recipe, plain):
        problem.embed(**kwargs)
    assert torch.equal(direct.X, recipe.X) and torch.equal(direct.landmarks, plain.landmarks)
    for problem in (direct, recipe):
        for stage in (problem.landmark_problem, problem.placement):
            assert stage._weights == dense_mod.Weights(dense_mod.W_POWER, 1.0, None)
    assert plain.landmark_problem._weights is None and plain.placement._weights is None
    # the landmark stage's value is that of a DenseMDE(weights=1) over the same rows
    rows = data[direct.landmarks.numpy()]
    same = pymde_amd.DenseMDE(rows, loss=quadratic, weights=1)
    X_l = direct.X[direct.landmarks.to(DEV)]
    got = float(direct.landmark_problem.average_distortion(direct.landmark_problem.X))
    assert got == float(same.average_distortion(direct.landmark_problem.X))
    unweighted = float(plain.landmark_problem.average_distortion(direct.landmark_problem.X))
    assert abs(unweighted - got) > 0.05 * got                    # the weight matters
    assert X_l.shape == (60, 2)
    # the placement's too: against the bipartite DensePlacement with weights=1
    other = pymde_amd.DensePlacement.weighted(rows, direct.landmark_problem.X, data[direct.placed.numpy()],
                                              loss=quadratic, weights=1)
    assert float(other.average_distortion(direct.placement.X)) == float(direct.placement.average_distortion())
    # dense=True takes it as well, with Standardized's rescaling as it was
    std = pymde_amd.preserve_distances(data, dense=True, loss=quadratic, constraint=pymde_amd.Standardized(), weights=1)
    ref = pymde_amd.preserve_distances(data, dense=True, loss=quadratic, constraint=pymde_amd.Standardized())
    assert std.deviation_scale == ref.deviation_scale != 1.0 and std._weights.p == 1.0


# ---------------------------------------------------------------- 5. from_graph
def _two_cycles(a=40, b=60):
    e = [(i, (i + 1) % a) for i in range(a)] + [(a + i, a + (i + 1) % b) for i in range(b)]
    return np.asarray(e, dtype=np.int64)


def test_from_graph_keeps_the_pairs_a_path_joins():
    import pymde_amd
    cycles = _two_cycles()
    n = 100
    graph = pymde_amd.Graph.from_edges(torch.as_tensor(cycles), n_items=n)
    rng = np.random.default_rng(46)
    X = (8.0 * rng.standard_normal((n, 2))).astype(np.float32)
    for loss in (pymde_amd.losses.Absolute, pymde_amd.losses.Quadratic):
        edge = pymde_amd.preserve_distances(graph, max_distances=1e9, loss=loss)
        dense = pymde_amd.DenseMDE.from_graph(graph, loss=loss)
        assert dense.p == math.comb(40, 2) + math.comb(60, 2) == int(edge.p)
        _compare("two cycles, %s" % loss.__name__, _value_and_grad(dense, X), _value_and_grad(edge, X))
    # max_length keeps the pairs within 5 steps: 5 per node and side
    capped = pymde_amd.DenseMDE.from_graph(graph, max_length=5)
    assert capped.p == 100 * 5
    W = capped._weights.W.cpu().numpy()
    gap = np.abs(np.arange(n)[:, None] - np.arange(n)[None, :])
    steps = np.full((n, n), np.inf)
    steps[:40, :40] = np.minimum(gap[:40, :40], 40 - gap[:40, :40])
    steps[40:, 40:] = np.minimum(gap[40:, 40:], 60 - gap[40:, 40:])
    assert np.array_equal(W > 0, (steps >= 1) & (steps <= 5))
    assert np.array_equal(capped._Dm.cpu().numpy()[W > 0], steps[W > 0].astype(np.float32))
    # an isolated node has no position
    lonely = pymde_amd.Graph.from_edges(torch.as_tensor(cycles), n_items=n + 1)
    with pytest.raises(ValueError, match="without a pair"):
        pymde_amd.DenseMDE.from_graph(lonely)
    with pytest.raises(ValueError, match="Graph"):
        pymde_amd.DenseMDE.from_graph(cycles)

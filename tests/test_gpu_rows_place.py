"""DensePlacement.embed(solver="rows") and LandmarkMDE.embed(placement_solver="rows") on the GPU: the per-row solver
reaches what the joint solver reaches with fewer evaluations, every row reaches what scipy's float64 BFGS reaches on
that row alone (``tests/_rows_reference.py``), Absolute terminates by stalling, and a solve is reproducible."""
import functools

import numpy as np
import pytest
import torch

import _rows_reference as ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
N_OLD, N_NEW = 300, 150

_CACHE = {}


def _seed31():
    """The seed-31 inputs at d = 2 and scipy's per-row minima (computed once per loss)."""
    if "inputs" not in _CACHE:
        _CACHE["inputs"] = ref.seed31_problem(2)
    return _CACHE["inputs"]


def _scipy(loss_name):
    if loss_name not in _CACHE:
        _, _, X_old, start, D = _seed31()
        loss = {"Quadratic": ref.quadratic, "Huber": ref.huber(1.0)}[loss_name]
        _CACHE[loss_name] = ref.scipy_row_minima(ref.row_objective(loss, X_old, D), start)
    return _CACHE[loss_name]


def test_rows_reach_what_the_joint_solver_reaches_with_fewer_evaluations():
    """The planar exact-embedding setting of test_embed_reaches_what_the_anchored_edge_list_problem_reaches."""
    import pymde_amd
    rng = np.random.default_rng(22)
    rows = rng.standard_normal((N_OLD + N_NEW, 2)) * np.array([3.0, 1.0])
    rows = (rows - rows[:N_OLD].mean(0)).astype(np.float32)
    data, new = rows[:N_OLD], rows[N_OLD:]
    X_old = torch.as_tensor(data).to(DEV)                       # the true coordinates
    kept = X_old.clone()
    start = torch.as_tensor(new + (0.1 * rows.std() * rng.standard_normal((N_NEW, 2))).astype(np.float32)).to(DEV)
    kwargs = dict(eps=1e-6, max_iter=200)
    quadratic = pymde_amd.losses.Quadratic
    joint = pymde_amd.DensePlacement(data, X_old, new, loss=quadratic)
    initial = float(joint.average_distortion(start))
    joint.embed(X=start.clone(), **kwargs)
    place = pymde_amd.DensePlacement(data, X_old, new, loss=quadratic)
    assert place.row_status is None
    X = place.embed(X=start.clone(), solver="rows", **kwargs)
    stats = place.solve_stats
    error = float((X - torch.as_tensor(new).to(DEV)).abs().max())
    print("initial %.6g; joint %.6g in %d iterations, %d evaluations; rows %.6g in %d sweeps, %.2f evaluations, "
          "status counts %s; worst coordinate error %.3g"
          % (initial, joint.value, joint.solve_stats.iterations, joint.solve_stats.evaluations, place.value,
             stats.iterations, stats.evaluations, torch.bincount(place.row_status, minlength=3).tolist(), error))
    assert X is place.X and X.shape == (N_NEW, 2) and X.is_cuda and X.dtype == torch.float32
    assert place.value <= 1.05 * joint.value + 1e-6 * initial
    assert error <= 1e-3
    assert place.row_status.dtype == torch.int32 and place.row_status.shape == (N_NEW,)
    assert int((place.row_status == 0).sum()) == 0
    assert stats.evaluations < joint.solve_stats.evaluations
    assert stats.iterations == len(stats.average_distortions) == len(stats.residual_norms) == len(
        stats.step_size_percents) == len(stats.times) > 0
    assert place.value == stats.average_distortions[-1] and place.residual_norm == stats.residual_norms[-1]
    assert abs(float(place.average_distortion()) - place.value) <= 1e-4 * initial
    both = place.embedding()
    assert torch.equal(both[:N_OLD], kept) and torch.equal(both[N_OLD:], X) and torch.equal(X_old, kept)
    # snapshots are honoured
    again = pymde_amd.DensePlacement(data, X_old, new, loss=quadratic)
    again.embed(X=start.clone(), solver="rows", snapshot_every=5, **kwargs)
    assert len(again.solve_stats.snapshots) == (again.solve_stats.iterations + 4) // 5
    assert torch.equal(again.solve_stats.snapshots[0], start.cpu())


@pytest.mark.parametrize("source", ["data", "distance_matrix"])
@pytest.mark.parametrize("loss_name", ["Quadratic", "Huber"])
def test_every_row_reaches_scipys_minimum_for_that_row(loss_name, source):
    import pymde_amd
    old, new, X_old, start, D = _seed31()
    best, first = _scipy(loss_name)
    loss = {"Quadratic": pymde_amd.losses.Quadratic,
            "Huber": functools.partial(pymde_amd.losses.Huber, threshold=1.0)}[loss_name]
    if source == "data":
        place = pymde_amd.DensePlacement(old, X_old, new, loss=loss)
    else:
        place = pymde_amd.DensePlacement(None, X_old, None, loss=loss, distance_matrix=D)
    place.embed(X=torch.as_tensor(start).to(DEV), solver="rows", eps=1e-5, max_iter=300)
    items = place.item_distortions().double().cpu().numpy()
    excess = (items - best) / first
    print("%s from %s: %d sweeps, %.2f evaluations, status counts %s, worst excess over scipy %.3g of the starting "
          "value (bound 1e-4)" % (loss_name, source, place.solve_stats.iterations, place.solve_stats.evaluations,
                                  torch.bincount(place.row_status, minlength=3).tolist(), excess.max()))
    assert int((place.row_status == 0).sum()) == 0
    assert (items <= best + 1e-4 * first).all()


def test_absolute_terminates_by_stalling():
    import pymde_amd
    old, new, X_old, start, _ = _seed31()
    first = torch.as_tensor(start).to(DEV)
    joint = pymde_amd.DensePlacement(old, X_old, new, loss=pymde_amd.losses.Absolute)
    joint.embed(X=first.clone(), eps=1e-5, max_iter=300)
    place = pymde_amd.DensePlacement(old, X_old, new, loss=pymde_amd.losses.Absolute)
    place.embed(X=first.clone(), solver="rows", eps=1e-5, max_iter=300)
    print("Absolute: rows %.8g in %d sweeps, %.2f evaluations, status counts %s; joint %.8g in %d iterations"
          % (place.value, place.solve_stats.iterations, place.solve_stats.evaluations,
             torch.bincount(place.row_status, minlength=3).tolist(), joint.value, joint.solve_stats.iterations))
    assert place.solve_stats.iterations <= 300
    assert bool((place.row_status == 2).all())
    assert place.value <= 1.05 * joint.value


def test_two_solves_from_the_same_start_give_the_same_bits():
    import pymde_amd
    old, new, X_old, start, _ = _seed31()
    results = []
    for _ in range(2):
        place = pymde_amd.DensePlacement(old, X_old, new, loss=pymde_amd.losses.Quadratic)
        place.embed(X=torch.as_tensor(start).to(DEV), solver="rows", eps=1e-5, max_iter=300)
        results.append((place.X.clone(), place.row_status.clone(), place.value, place.solve_stats.evaluations))
    assert torch.equal(results[0][0], results[1][0]) and torch.equal(results[0][1], results[1][1])
    assert results[0][2:] == results[1][2:]


def test_landmarks_with_the_per_row_placement_reach_the_stress_of_the_full_problem():
    """The n = 600, m = 150 setting of test_landmarks_reach_the_stress_of_the_full_problem."""
    import pymde_amd
    from pymde_amd import quality
    n, m = 600, 150
    rng = np.random.default_rng(23)
    coords = rng.standard_normal((n, 2)) * np.array([3.0, 1.0])
    coords = coords - coords.mean(0)
    basis = np.linalg.qr(rng.standard_normal((5, 2)))[0]
    data = (coords @ basis.T).astype(np.float32)
    start = torch.as_tensor((coords + 0.1 * coords.std() * rng.standard_normal((n, 2))).astype(np.float32)).to(DEV)
    kwargs = dict(eps=1e-6, max_iter=200)
    quadratic = pymde_amd.losses.Quadratic
    landmark = pymde_amd.preserve_distances(data, landmarks=m, seed=0, loss=quadratic)
    X = landmark.embed(X=start.clone(), placement_solver="rows", **kwargs)
    full = pymde_amd.DenseMDE(data, loss=quadratic)
    X_full = full.embed(X=start.clone(), **kwargs)
    s_full = quality.stress(data, X_full, scale=1.0)
    s_landmark = quality.stress(data, X, scale=1.0)
    print("stress at scale 1: full dense problem %.6g, %d landmarks with per-row placement %.6g (%d sweeps, %.2f "
          "evaluations)" % (s_full, m, s_landmark, landmark.solve_stats.placement.iterations,
                            landmark.solve_stats.placement.evaluations))
    assert s_landmark <= s_full + 1e-3
    assert landmark.placement.row_status is not None and landmark.placement.row_status.shape == (n - m,)
    assert landmark.landmark_problem.solve_stats.evaluations is not None     # the landmark stage ran the joint solver

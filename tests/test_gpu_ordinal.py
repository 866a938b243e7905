"""pymde_amd.OrdinalMDE on the GPU against the float64 reference of tests/_ordinal_reference.py: disparities with and
without ties, recovery of a configuration from monotonically distorted distances where the metric solution fits
the distortion, invariance under a monotone transformation, the history, the errors and the recipe."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _ordinal_reference as ref  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _points(n=60):
    return np.random.default_rng(0).uniform(-1.0, 1.0, (n, 2))


def _all_pairs(P):
    i, j = np.triu_indices(len(P), 1)
    edges = np.stack([i, j], 1)
    return edges, np.sqrt(((P[i] - P[j]) ** 2).sum(1))


def _problem(edges, deviations, n, **kw):
    import pymde_amd
    return pymde_amd.OrdinalMDE(n, 2, torch.as_tensor(edges, device=DEV), torch.as_tensor(deviations, device=DEV),
                                **kw)


@pytest.mark.parametrize("ties", [False, True])
def test_disparities_match_reference(ties):
    import pymde_amd
    pymde_amd.seed(0)
    P = _points()
    edges, D = _all_pairs(P)
    dev = np.ceil(8.0 * D) if ties else D ** 3
    mde = _problem(edges, dev, 60)
    assert (mde.n_groups < len(dev)) == ties
    X = torch.randn(60, 2, device=DEV)
    got = mde.disparities(X)
    assert got.dtype == torch.float32 and tuple(got.shape) == (len(dev),)
    dist = mde.problem.distances(X).detach().cpu().numpy()          # the device's own float32 distances
    want = ref.disparities(dev, dist)
    err = np.abs(got.cpu().numpy().astype(np.float64) - want).max()
    print("ties", ties, "err", err, "allowed", 2.0 ** -22 * dist.max())
    assert err <= 2.0 ** -22 * dist.max()
    if ties:
        g = got.cpu().numpy()
        for value in np.unique(dev):
            assert np.unique(g[dev == value].view(np.int32)).size == 1
    assert mde.stress(X) == pytest.approx(ref.stress1(dist, want), rel=1e-5)
    d_rank, dist_rank, fit_rank = mde.shepard(X)
    assert np.all(np.diff(d_rank.cpu().numpy()) >= 0) and np.all(np.diff(fit_rank.cpu().numpy()) >= 0)
    assert np.array_equal(np.sort(dist_rank.cpu().numpy()), np.sort(dist))


@functools.lru_cache(maxsize=None)
def _recovered(name):
    """The metric and the ordinal solution of a recovery problem, computed once."""
    import pymde_amd
    from scipy.spatial import procrustes
    pymde_amd.seed(0)
    P, edges, D, dev = ref.recovery_problem(name)
    n = len(P)
    e = torch.as_tensor(edges, device=DEV)
    d0 = torch.as_tensor(dev / np.sqrt((dev ** 2).mean()), dtype=torch.float32, device=DEV)
    metric = pymde_amd.MDE(n, 2, e, pymde_amd.losses.Quadratic(d0))
    X_metric = metric.embed()
    mde = _problem(edges, dev, n)
    stress_metric = mde.stress(X_metric)
    X = mde.embed()
    return {"mde": mde, "stress_metric": stress_metric, "stress": mde.stress_,
            "procrustes_metric": procrustes(P, X_metric.cpu().numpy().astype(np.float64))[2],
            "procrustes": procrustes(P, X.cpu().numpy().astype(np.float64))[2], "X": X}


@pytest.mark.parametrize("name", ref.RECOVERY)
def test_recovery(name):
    r = _recovered(name)
    print(name, "stress-1 %.3e -> %.3e, procrustes %.3e -> %.3e, rounds %d" % (
        r["stress_metric"], r["stress"], r["procrustes_metric"], r["procrustes"], r["mde"].rounds_))
    assert r["stress"] <= r["stress_metric"] / 20.0
    assert r["procrustes"] <= r["procrustes_metric"] / 20.0
    mde = r["mde"]
    assert mde.stress_ == pytest.approx(mde.stress(), rel=1e-6)
    assert torch.equal(mde.disparities_, mde.disparities())
    assert mde.solve_stats is mde.problem.solve_stats and mde.rounds_ == len(mde.stress_history) - 1


def test_invariance_under_a_monotone_transformation():
    import pymde_amd
    pymde_amd.seed(0)
    P = _points()
    edges, D = _all_pairs(P)
    D = np.round(D, 2)                                   # ties, identical by construction in D and D^3
    X = torch.randn(60, 2, device=DEV)
    a = _problem(edges, D, 60).disparities(X)
    b = _problem(edges, D ** 3, 60).disparities(X)
    assert torch.equal(a, b)


def test_history_and_determinism():
    mde = _recovered("cube")["mde"]
    assert mde.stress_history[-1] <= mde.stress_history[0]
    assert len(mde.stress_history) >= 2
    X0 = torch.randn(60, 2, device=DEV)
    X0 -= X0.mean(0)
    first = mde.embed(X0, rounds=4).clone()
    history = list(mde.stress_history)
    second = mde.embed(X0, rounds=4)
    assert torch.equal(first, second) and history == mde.stress_history
    assert mde.stress_history[-1] <= mde.stress_history[0]


def test_errors():
    import pymde_amd
    P = _points(10)
    edges, D = _all_pairs(P)
    with pytest.raises(ValueError):
        _problem(edges, D, 10, loss=pymde_amd.losses.WeightedQuadratic)
    with pytest.raises(ValueError):
        _problem(edges, D, 10, constraint=pymde_amd.Anchored(torch.tensor([0, 1]), torch.zeros(2, 2)))
    for bad in (np.nan, np.inf):
        Z = D.copy()
        Z[3] = bad
        with pytest.raises(ValueError):
            _problem(edges, Z, 10)
    with pytest.raises(ValueError):
        _problem(edges, D, 10).disparities()


def test_recipe():
    import pymde_amd
    pymde_amd.seed(0)
    data = np.random.default_rng(3).standard_normal((80, 5)).astype(np.float32)
    mde = pymde_amd.preserve_distances(data, loss=pymde_amd.losses.Quadratic, ordinal=True)
    assert isinstance(mde, pymde_amd.OrdinalMDE) and int(mde.edges.shape[0]) == 80 * 79 // 2
    X = mde.embed(rounds=3)
    assert tuple(X.shape) == (80, 2) and bool(torch.isfinite(X).all())
    assert mde.stress_history[-1] <= mde.stress_history[0]
    std = pymde_amd.preserve_distances(data, loss=pymde_amd.losses.Quadratic, ordinal=True,
                                       constraint=pymde_amd.Standardized())
    assert std.length == pytest.approx(float(pymde_amd.Standardized().natural_length(80, 2)))
    with pytest.raises(ValueError):
        pymde_amd.preserve_distances(data, ordinal=True, dense=True)
    with pytest.raises(ValueError):
        pymde_amd.preserve_distances(data, ordinal=True, landmarks=20)
    with pytest.raises(ValueError):
        pymde_amd.preserve_distances(data, ordinal=True,
                                     constraint=pymde_amd.Anchored(torch.tensor([0, 1]), torch.zeros(2, 2)))
    plain = pymde_amd.preserve_distances(data, ordinal=False)
    assert isinstance(plain, pymde_amd.MDE)

"""The float64 reference of tests/_ordinal_reference.py against scipy and scikit-learn, its optimality check, its
tie groups, and the choice of the recovery problems of tests/test_gpu_ordinal.py (no GPU)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _ordinal_reference as ref  # noqa: E402

SIZES = (1, 2, 3, 64, 257, 1000)


def _weights(kind, p, seed):
    rng = np.random.default_rng(seed)
    if kind == "none":
        return None
    if kind == "integers":
        return rng.integers(1, 17, p).astype(np.float64)
    return rng.uniform(1e-3, 1e3, p)


@pytest.mark.parametrize("weights", ["none", "integers", "wide"])
@pytest.mark.parametrize("name", ref.PATTERNS)
def test_pava_matches_scipy_and_sklearn(name, weights):
    from scipy.optimize import isotonic_regression
    for p in SIZES:
        y = ref.pattern(name, p, seed=p).astype(np.float64)
        w = _weights(weights, p, seed=p + 1)
        got = ref.pava(y, w)
        scale = max(np.abs(y).max(), 1.0)
        want = isotonic_regression(y, weights=w).x
        assert np.abs(got - want).max() <= 1e-12 * scale, (name, p)
        assert np.all(np.diff(got) >= 0)
    sk = pytest.importorskip("sklearn.isotonic")
    for p in SIZES:
        y = ref.pattern(name, p, seed=p).astype(np.float64)
        w = _weights(weights, p, seed=p + 1)
        want = sk.isotonic_regression(y, sample_weight=w)
        assert np.abs(ref.pava(y, w) - want).max() <= 1e-12 * max(np.abs(y).max(), 1.0), (name, p)


@pytest.mark.parametrize("name", ref.PATTERNS)
def test_kkt_violation(name):
    p = 300
    y = ref.pattern(name, p, seed=3).astype(np.float64)
    w = _weights("integers", p, seed=4)
    out = ref.pava(y, w)
    viol, weight = ref.kkt_violation(y, w, out)
    assert viol <= 1e-9 * max(np.abs(y).max(), 1.0) * w.sum()
    assert weight > 0
    # a wrongly pooled copy: the first two blocks (or the two halves of the only block) forced to one value
    starts = np.flatnonzero(np.concatenate([[True], out[1:] != out[:-1]]))
    wrong = out.copy()
    if len(starts) > 1:
        end = starts[2] if len(starts) > 2 else p
        wrong[:end] = np.average(y[:end], weights=w[:end])
        # pooling two blocks of different means leaves a prefix of the new run below its value
        assert ref.kkt_violation(y, w, wrong)[0] > 1e-6 * np.abs(y).max()
    else:
        wrong[:p // 2] -= 0.5            # still nondecreasing, no longer the weighted mean
        assert ref.kkt_violation(y, w, wrong)[0] > 0.1
    assert ref.kkt_violation([0.0, 1.0], None, [1.0, 0.0]) == (np.inf, 0.0)


def test_tie_groups_by_hand():
    dev = np.array([3.0, 1.0, 2.0, 1.0, 3.0, 3.0, 0.5])
    order, group, sizes = ref.tie_groups(dev)
    assert order.tolist() == [6, 1, 3, 2, 0, 4, 5]          # stable: equal deviations keep their edge order
    assert group.tolist() == [0, 1, 1, 2, 3, 3, 3]
    assert sizes.tolist() == [1, 2, 1, 3]
    # the tied edges 1 and 3 share their mean distance, which then pools with edge 2; so do edges 0, 4 and 5
    dist = np.array([5.0, 2.0, 3.0, 4.0, 6.0, 7.0, 1.0])
    got = ref.disparities(dev, dist)
    assert np.allclose(got, [6.0, 3.0, 3.0, 3.0, 6.0, 6.0, 1.0])
    assert ref.stress1(dist, got) == pytest.approx(np.sqrt(((dist - got) ** 2).sum() / (dist ** 2).sum()))
    order, group, sizes = ref.tie_groups(np.array([2.0, 1.0, 3.0]))
    assert group.tolist() == [0, 1, 2] and sizes.tolist() == [1, 1, 1]


@pytest.mark.parametrize("name", ref.RECOVERY)
def test_replay_recovers_the_configuration(name):
    """Pins the choice of inputs, not the device: on each recovery problem the float64 alternation ends at no more
    than 1 / 100 of the metric start's ordinal stress."""
    from scipy.spatial import procrustes
    P, edges, D, dev = ref.recovery_problem(name)
    n = len(P)
    X0 = np.random.default_rng(1).standard_normal((n, 2))
    X, history, X_metric = ref.replay(edges, dev, n, 2, X0, rounds=30, inner_iter=15)
    print(name, "stress", history[0], "->", history[-1], "procrustes", procrustes(P, X_metric)[2], "->",
          procrustes(P, X)[2])
    assert history[-1] <= history[0] / 100.0

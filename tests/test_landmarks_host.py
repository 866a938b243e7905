"""Landmark selection without a device: the refusals of ``pymde_amd.landmarks.select`` and of the recipes that use
it come before any device is required, the new keywords default to the uniform draw, and the numpy replay
(tests/_landmarks_reference.py) the kernels are held to gives the known answers on hand-made cases."""
import inspect

import numpy as np
import pytest
import torch

import pymde_amd
from pymde_amd import landmarks

import _landmarks_reference as ref


@pytest.fixture(autouse=True)
def no_device(monkeypatch):
    """Any attempt to pick a device fails the test: the refusals below must come first."""
    def refuse(*args, **kwargs):
        raise AssertionError("a device was required before the arguments were checked")
    monkeypatch.setattr(pymde_amd.util, "require_cuda_device", refuse)


DATA = np.arange(40, dtype=np.float32).reshape(10, 4)


def test_exported():
    assert pymde_amd.landmarks is landmarks
    assert landmarks.LandmarkSelection._fields == ("indices", "radius", "nearest", "distance")


@pytest.mark.parametrize("method", ["nearest", "uniform", "", None, 3])
def test_unknown_method(method):
    with pytest.raises(ValueError, match="method"):
        landmarks.select(DATA, 3, method=method)


def test_method_aliases():
    assert landmarks.resolve_method("k-means++") == landmarks.resolve_method("kmeans++") == "kmeans++"
    assert landmarks.resolve_method("Farthest") == "farthest"
    assert landmarks.resolve_selection("uniform") == "uniform"
    with pytest.raises(ValueError, match="selection"):
        landmarks.resolve_selection("random")


@pytest.mark.parametrize("metric", ["manhattan", "l1", "cityblock"])
def test_manhattan_refused(metric):
    with pytest.raises(ValueError, match="manhattan"):
        landmarks.select(DATA, 3, metric=metric)


def test_unknown_metric():
    with pytest.raises(ValueError):
        landmarks.select(DATA, 3, metric="chebyshev")


class _Graph:
    """What ``preprocess._is_graph`` takes for a ``Graph`` (building a real one needs a device)."""
    edges, n_items = None, 10


def test_graph_refused():
    with pytest.raises(ValueError, match="Graph"):
        landmarks.select(_Graph(), 2)
    with pytest.raises(ValueError, match="Graph"):
        pymde_amd.preserve_distances(_Graph(), landmarks=4, landmark_selection="farthest")


@pytest.mark.parametrize("m", [0, -1, 11, 2.5, True])
def test_m_outside_range(m):
    with pytest.raises(ValueError, match="`m`"):
        landmarks.select(DATA, m)


@pytest.mark.parametrize("start", [-1, 10, 1.5, True])
def test_start_outside_range(start):
    with pytest.raises(ValueError, match="`start`"):
        landmarks.select(DATA, 3, start=start)


def test_not_a_matrix():
    with pytest.raises(ValueError):
        landmarks.select(np.zeros(5, dtype=np.float32), 2)


def test_landmark_selection_needs_landmarks():
    for dense in (False, True):
        with pytest.raises(ValueError, match="landmark_selection"):
            pymde_amd.preserve_distances(DATA, landmark_selection="farthest", dense=dense)


def test_unknown_selection_in_the_recipes():
    with pytest.raises(ValueError, match="selection"):
        pymde_amd.preserve_distances(DATA, landmarks=4, landmark_selection="maxmin")
    with pytest.raises(ValueError, match="selection"):
        pymde_amd.LandmarkMDE(DATA, 4, selection="maxmin")
    # and the landmark path's own refusals still come without a device under the new selections
    with pytest.raises(ValueError, match="'euclidean', 'cosine' and 'correlation'"):
        pymde_amd.preserve_distances(DATA, landmarks=4, landmark_selection="farthest", metric="manhattan")
    with pytest.raises(ValueError, match="landmarks"):
        pymde_amd.preserve_distances(DATA, landmarks=10, landmark_selection="kmeans++")


def test_signatures_default_to_uniform():
    assert inspect.signature(pymde_amd.LandmarkMDE.__init__).parameters["selection"].default == "uniform"
    assert inspect.signature(pymde_amd.preserve_distances).parameters["landmark_selection"].default == "uniform"
    sig = inspect.signature(landmarks.select)
    assert list(sig.parameters) == ["data", "m", "method", "metric", "start", "seed", "device"]
    assert sig.parameters["method"].default == "farthest" and sig.parameters["metric"].default == "euclidean"
    assert all(sig.parameters[p].default is None for p in ("start", "seed", "device"))


# ---------------------------------------------------------------- the reference on hand-made cases
def test_reference_four_points_on_a_line():
    X = np.array([[0.0], [1.0], [3.0], [10.0]])
    idx, radius2, nearest, mind2 = ref.select(X, 4, ref.FARTHEST, 0)
    assert idx.tolist() == [0, 3, 2, 1]
    assert radius2.tolist() == [np.inf, 100.0, 9.0, 1.0]
    assert nearest.tolist() == [0, 3, 2, 1] and mind2.tolist() == [0.0] * 4
    idx, radius2, nearest, mind2 = ref.select(X, 2, ref.FARTHEST, 1)
    assert idx.tolist() == [1, 3] and radius2.tolist() == [np.inf, 81.0]
    assert nearest.tolist() == [0, 0, 0, 1] and mind2.tolist() == [1.0, 0.0, 4.0, 0.0]
    # an equal maximum goes to the smaller row, an equal distance to the earlier landmark
    X = np.array([[0.0], [2.0], [-2.0], [1.0]])
    idx, radius2, nearest, _ = ref.select(X, 3, ref.FARTHEST, 0)
    assert idx.tolist() == [0, 1, 2] and radius2.tolist() == [np.inf, 4.0, 4.0]
    assert nearest.tolist() == [0, 1, 2, 0]


@pytest.mark.parametrize("method", [ref.FARTHEST, ref.KMEANSPP])
def test_reference_duplicates_give_distinct_rows(method):
    base = np.array([[0.0, 0.0], [3.0, 0.0], [0.0, 4.0]])
    X = base[[0, 1, 2, 0, 1, 2, 0]]
    idx, radius2, nearest, mind2 = ref.select(X, 6, method, 3, seed=5)
    assert len(set(idx.tolist())) == 6
    assert sorted(map(tuple, X[idx[:3]].tolist())) == sorted(map(tuple, base.tolist()))
    assert radius2[3:].tolist() == [0.0, 0.0, 0.0]
    # with nothing but duplicates left the smallest unselected row is next
    assert idx[3] == min(set(range(7)) - set(idx[:3].tolist()))
    assert mind2.tolist() == [0.0] * 7
    # a duplicate keeps the landmark that came first
    assert all(nearest[r] < 3 for r in range(7))


def test_reference_draws():
    assert ref.splitmix64(0) == 0xE220A8397B1DCDAF       # the published first output of SplitMix64 from state 0
    assert ref.uniform01(0, 1) == 0.36818951565166946
    assert ref.uniform01(0, 1) == (ref.splitmix64(ref.splitmix64(1)) >> 11) / 2.0 ** 53
    assert ref.uniform01(7, 3) != ref.uniform01(8, 3) and 0.0 <= ref.uniform01(2 ** 64 - 1, 2 ** 40) < 1.0


def test_reference_kmeanspp_follows_the_prefix_sum():
    mind2 = np.array([1.0, -1.0, 2.0, 0.0, 5.0])       # total 8: prefixes 1, 1, 3, 3, 8
    for u, want in [(0.0, 0), (0.124, 0), (0.125, 2), (0.3, 2), (0.375, 4), (0.99, 4)]:
        assert ref.choose(mind2, ref.KMEANSPP, u)[0] == want, u
    assert ref.choose(np.array([-1.0, 0.0, -1.0, 0.0]), ref.KMEANSPP, 0.7)[0] == 1
    assert ref.choose(np.array([-1.0, 0.0, 3.0, 3.0]), ref.FARTHEST)[0] == 2


def test_reference_covers_the_far_group():
    X = ref.blobs_with_far_group(1037, 50)
    idx, _, _, mind2 = ref.select(X, 64, ref.FARTHEST, 17)
    assert (idx < 5).any()
    uniform = np.random.default_rng(0).permutation(1037)[:64]
    uniform = uniform[uniform >= 5]                    # (a draw that misses the far group, as most do)
    assert 9.0 * mind2.max() < ref.covering_radius2(X, uniform)

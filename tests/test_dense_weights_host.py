"""What the ``weights=`` of the dense problems decides without a device (pymde_amd.dense): the
parsing of the argument, the shape errors (raised before any device is asked for), the refusals of a weight matrix
where landmark MDS draws the rows, and the refusals that were there before."""
import functools

import numpy as np
import pytest
import torch

from pymde_amd import dense, losses, recipes


def test_a_number_is_the_power_form_and_a_matrix_the_matrix_form():
    assert dense.parse_weights(None) is dense.NO_WEIGHTS and dense.NO_WEIGHTS.source == dense.W_NONE
    for value in (0, 1, 2, 2.5, np.float32(1.0), np.float64(0.5), np.int64(2), np.asarray(1.5), torch.tensor(1.0)):
        w = dense.parse_weights(value)
        assert w.source == dense.W_POWER and w.p == float(value) and w.W is None
    for matrix in (np.ones((4, 4), dtype=np.float32), np.ones((4, 4), dtype=bool), np.ones((4, 4), dtype=np.int64),
                   torch.ones((4, 4)), torch.ones((4, 4), dtype=torch.bool), torch.ones((4, 4), dtype=torch.float64)):
        w = dense.parse_weights(matrix, (4, 4))
        assert w.source == dense.W_MATRIX and w.W is matrix
    assert dense.parse_weights(np.ones((3, 5)), (3, 5)).source == dense.W_MATRIX


@pytest.mark.parametrize("value", [True, False, np.bool_(True), -1, -0.5, float("nan"), float("inf"), "1", b"1", "sammon",
                                   [[1.0, 0.0], [0.0, 1.0]], (1.0,), 1j, np.asarray(True), torch.tensor(True)])
def test_what_is_neither_is_refused(value):
    with pytest.raises(ValueError, match="weights"):
        dense.parse_weights(value, (2, 2))


def test_a_matrix_of_the_wrong_shape_or_type_is_refused():
    for matrix in (np.ones((4, 5)), np.ones((5, 4)), np.ones(4), np.ones((4, 4, 1)), torch.ones((3, 4))):
        with pytest.raises(ValueError, match="shape"):
            dense.parse_weights(matrix, (4, 4))
    with pytest.raises(ValueError, match="dtype"):
        dense.parse_weights(np.ones((4, 4), dtype=np.complex64), (4, 4))
    with pytest.raises(ValueError, match="dtype"):
        dense.parse_weights(np.full((4, 4), "a"), (4, 4))


def test_shape_errors_come_before_any_device_work(monkeypatch):
    """No device may be asked for on the way to a shape error."""
    from pymde_amd import util

    def no_device(*args, **kwargs):
        raise AssertionError("a device was asked for")
    monkeypatch.setattr(util, "require_cuda_device", no_device)
    monkeypatch.setattr(util, "get_default_device", no_device)
    data = np.random.default_rng(0).standard_normal((10, 3)).astype(np.float32)
    with pytest.raises(ValueError, match=r"shape \(10, 10\)"):
        dense.DenseMDE(data, weights=np.ones((10, 9)))
    with pytest.raises(ValueError, match=r"shape \(10, 10\)"):
        dense.DenseMDE(distance_matrix=np.ones((10, 10)), weights=np.ones((9, 9)))
    with pytest.raises(ValueError, match="weights"):
        dense.DenseMDE(data, weights=True)
    with pytest.raises(ValueError, match="weights"):
        dense.DenseMDE(data, weights=-1.0)
    X_old = np.zeros((10, 2), dtype=np.float32)
    new = data[:4]
    with pytest.raises(ValueError, match=r"shape \(4, 10\)"):
        dense.DensePlacement.weighted(data, X_old, new, weights=np.ones((10, 4)))
    with pytest.raises(ValueError, match=r"shape \(4, 10\)"):
        dense.DensePlacement.weighted(None, X_old, None, distance_matrix=np.ones((4, 10)), weights=np.ones((4, 4)))
    with pytest.raises(ValueError, match="weights"):
        dense.DensePlacement.weighted(data, X_old, new, weights="1")
    # the constructor itself keeps the parameters it had: the weights of a placement go through `weighted`
    import inspect
    assert "weights" not in inspect.signature(dense.DensePlacement.__init__).parameters
    assert inspect.signature(dense.DensePlacement.weighted).parameters["weights"].kind is inspect.Parameter.KEYWORD_ONLY
    with pytest.raises(TypeError):
        dense.DensePlacement(data, X_old, new, weights=1)


def test_landmarks_and_the_recipe_take_the_power_form_only(monkeypatch):
    from pymde_amd import util

    def no_device(*args, **kwargs):
        raise AssertionError("a device was asked for")
    monkeypatch.setattr(util, "require_cuda_device", no_device)
    monkeypatch.setattr(util, "get_default_device", no_device)
    data = np.random.default_rng(1).standard_normal((12, 3)).astype(np.float32)
    W = np.ones((12, 12), dtype=np.float32)
    with pytest.raises(ValueError, match="weight matrix"):
        dense.LandmarkMDE(data, 5, weights=W)
    with pytest.raises(ValueError, match="weight matrix"):
        recipes.preserve_distances(data, landmarks=5, weights=W)
    with pytest.raises(ValueError, match="weight matrix"):
        recipes.preserve_distances(data, dense=True, weights=W)
    for value in (True, -1.0, float("nan"), "1"):
        with pytest.raises(ValueError, match="weights"):
            dense.LandmarkMDE(data, 5, weights=value)
        with pytest.raises(ValueError, match="weights"):
            recipes.preserve_distances(data, dense=True, weights=value)
    # the edge-list problem is weighed through its loss
    with pytest.raises(ValueError, match="dense=True or landmarks"):
        recipes.preserve_distances(data, weights=1)


def test_the_refusals_that_were_there_stay():
    dev = torch.ones(1)
    with pytest.raises(ValueError, match="weights of its own"):
        dense.loss_spec(lambda d: losses.WeightedQuadratic(d, 3.0 * torch.ones_like(d)))
    with pytest.raises(ValueError, match="weights of its own"):
        dense.loss_spec(functools.partial(losses.WeightedQuadratic, weights=2.0 * dev))
    assert dense.loss_spec(losses.WeightedQuadratic).weighted and not dense.loss_spec(losses.Quadratic).weighted

    class _Graph:
        """What preprocess._is_graph recognises, without a device."""
        edges, n_items = None, 10
    g = _Graph()
    for kwargs in (dict(dense=True), dict(landmarks=3), dict(dense=True, weights=1)):
        with pytest.raises(ValueError, match="Graph"):
            recipes.preserve_distances(g, **kwargs)
    with pytest.raises(ValueError, match="Graph"):
        dense.DenseMDE(g)
    with pytest.raises(ValueError, match="Graph"):
        dense.DenseMDE.from_graph(np.ones((3, 3)))

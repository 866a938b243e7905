"""pymde_amd.DensePlacement, pymde_amd.LandmarkMDE and preserve_distances(landmarks=...): what is refused, and that it is
refused on the host -- every case here is a ValueError raised before a device is asked for, so the file runs without
one."""
import numpy as np
import pytest
import torch


def _inputs(n_old=12, n_new=5, nf=4, d=2):
    rng = np.random.default_rng(0)
    return (rng.standard_normal((n_old, nf)).astype(np.float32), rng.standard_normal((n_old, d)).astype(np.float32),
            rng.standard_normal((n_new, nf)).astype(np.float32))


class _Graph:
    """What preprocess._is_graph recognises, without a device behind it."""
    edges, n_items = None, 12


def test_public_names():
    import pymde_amd
    from pymde_amd import dense
    assert pymde_amd.DensePlacement is dense.DensePlacement
    assert pymde_amd.LandmarkMDE is dense.LandmarkMDE
    assert hasattr(dense, "_pair_loss_cross")
    import inspect
    assert "landmarks" in inspect.signature(pymde_amd.preserve_distances).parameters
    assert list(inspect.signature(dense.DensePlacement.__init__).parameters)[1:] == [
        "data", "X", "new_data", "loss", "metric", "deviation_scale", "distance_matrix", "device"]


def test_exactly_one_source():
    import pymde_amd
    data, X, new = _inputs()
    D = np.ones((5, 12), dtype=np.float32)
    with pytest.raises(ValueError, match="exactly one source"):
        pymde_amd.DensePlacement(data, X, new, distance_matrix=D)
    with pytest.raises(ValueError, match="exactly one source"):
        pymde_amd.DensePlacement(None, X, None)
    with pytest.raises(ValueError, match="together"):
        pymde_amd.DensePlacement(data, X, None)
    with pytest.raises(ValueError, match="together"):
        pymde_amd.DensePlacement(None, X, new)


def test_the_embedding_of_the_old_rows():
    import pymde_amd
    data, X, new = _inputs()
    with pytest.raises(ValueError, match="one embedding vector per row of `data`"):
        pymde_amd.DensePlacement(data, X[:11], new)
    with pytest.raises(ValueError, match=r"\[1, 8\]"):
        pymde_amd.DensePlacement(data, np.zeros((12, 0), dtype=np.float32), new)
    with pytest.raises(ValueError, match=r"\[1, 8\]"):
        pymde_amd.DensePlacement(data, np.zeros((12, 9), dtype=np.float32), new)
    with pytest.raises(ValueError, match=r"`X` must be the embedding"):
        pymde_amd.DensePlacement(data, np.zeros(12, dtype=np.float32), new)


def test_the_rows_to_place():
    import pymde_amd
    data, X, new = _inputs()
    with pytest.raises(ValueError, match="features"):
        pymde_amd.DensePlacement(data, X, new[:, :3])
    with pytest.raises(ValueError, match="at least one row"):
        pymde_amd.DensePlacement(data, X, new[:0])
    with pytest.raises(ValueError, match="at least one row"):
        pymde_amd.DensePlacement(None, X, None, distance_matrix=np.ones((0, 12), dtype=np.float32))


def test_manhattan_and_graphs_are_refused():
    import pymde_amd
    data, X, new = _inputs()
    with pytest.raises(ValueError, match="no Gram tile"):
        pymde_amd.DensePlacement(data, X, new, metric="manhattan")
    graph = _Graph()
    with pytest.raises(ValueError, match="Graph"):
        pymde_amd.DensePlacement(graph, X, new)
    with pytest.raises(ValueError, match="Graph"):
        pymde_amd.DensePlacement(data, X, graph)
    with pytest.raises(ValueError, match="Graph"):
        pymde_amd.preserve_distances(graph, landmarks=2)
    with pytest.raises(ValueError, match="no Gram tile"):
        pymde_amd.preserve_distances(data, landmarks=4, metric="manhattan")


def test_the_loss_and_the_scale():
    import pymde_amd
    data, X, new = _inputs()
    with pytest.raises(ValueError, match="penalty"):
        pymde_amd.DensePlacement(data, X, new, loss=pymde_amd.penalties.Log1p)
    with pytest.raises(ValueError, match="penalty"):
        pymde_amd.preserve_distances(data, landmarks=4, loss=pymde_amd.penalties.Log1p)
    for scale in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="deviation_scale"):
            pymde_amd.DensePlacement(data, X, new, deviation_scale=scale)


def test_the_shape_of_the_distance_matrix():
    import pymde_amd
    _, X, _ = _inputs()
    for shape in ((12, 5), (5, 11), (12,), (5, 12, 1)):
        with pytest.raises(ValueError, match="rectangular"):
            pymde_amd.DensePlacement(None, X, None, distance_matrix=np.ones(shape, dtype=np.float32))
    with pytest.raises(ValueError, match="rectangular"):
        pymde_amd.DensePlacement(None, X, None, distance_matrix=[[1.0] * 12] * 5)


def test_landmarks_lie_in_2_n():
    import pymde_amd
    data, _, _ = _inputs()
    for m in (-1, 0, 1, 12, 13, 2.5, True):
        with pytest.raises(ValueError, match="landmarks"):
            pymde_amd.preserve_distances(data, landmarks=m)
    with pytest.raises(ValueError, match="landmarks"):
        pymde_amd.LandmarkMDE(data, 12)


def test_landmarks_take_no_constraint_but_centered():
    import pymde_amd
    data, X, _ = _inputs()
    with pytest.raises(ValueError, match="placed rows are unconstrained"):
        pymde_amd.preserve_distances(data, landmarks=4, constraint=pymde_amd.Standardized())
    anchored = pymde_amd.Anchored(torch.tensor([0, 1]), torch.as_tensor(X[:2]))
    with pytest.raises(ValueError, match="placed rows are unconstrained"):
        pymde_amd.preserve_distances(data, landmarks=4, constraint=anchored)
    with pytest.raises(ValueError, match=r"\[1, 8\]"):
        pymde_amd.preserve_distances(data, landmarks=4, embedding_dim=9)

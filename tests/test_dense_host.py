"""Host side of the dense MDE problems (pymde_amd/dense.py): how a loss callable is resolved, and the argument errors
that are raised before any device is required.  No GPU needed."""
import functools

import numpy as np
import pytest
import torch

from pymde_amd import dense, losses, penalties, recipes
from pymde_amd.functions.function import KIND


# ---------------------------------------------------------------- loss_spec
@pytest.mark.parametrize("make,kind,scalars,weighted", [
    (losses.Quadratic, "L_QUADRATIC", (0.0, 0.0, 0.0), False),
    (losses.WeightedQuadratic, "L_WEIGHTED_QUADRATIC", (0.0, 0.0, 0.0), True),
    (losses.Cubic, "L_CUBIC", (0.0, 0.0, 0.0), False),
    (losses.Absolute, "L_ABSOLUTE", (0.0, 0.0, 0.0), False),
    (losses.Logistic, "L_LOGISTIC", (0.0, 0.0, 0.0), False),
    (losses.Fractional, "L_FRACTIONAL", (0.0, 0.0, 0.0), False),
    (losses.SoftFractional, "L_SOFT_FRACTIONAL", (10.0, 0.0, 0.0), False),
    (functools.partial(losses.SoftFractional, gamma=2.5), "L_SOFT_FRACTIONAL", (2.5, 0.0, 0.0), False),
    (functools.partial(losses.Huber, threshold=0.75), "L_HUBER", (0.75, 0.0, 0.0), False),
    (functools.partial(losses.Power, exponent=1.5), "L_POWER", (1.5, 0.0, 0.0), False),
    (functools.partial(losses.Power, exponent=torch.tensor(2.5)), "L_POWER", (2.5, 0.0, 0.0), False),
    (lambda deviations: losses.Huber(deviations, 2.0), "L_HUBER", (2.0, 0.0, 0.0), False),
])
def test_loss_spec(make, kind, scalars, weighted):
    spec = dense.loss_spec(make)
    assert isinstance(spec, dense.LossSpec)
    assert spec == (KIND[kind], scalars, weighted)
    assert spec.kind == KIND[kind] and spec.scalars == scalars and spec.weighted is weighted


def test_loss_spec_covers_every_public_loss():
    public = [v for k, v in vars(losses).items()
              if isinstance(v, type) and issubclass(v, losses._Loss) and not k.startswith("_")]
    assert len(public) == 9
    for cls in public:
        make = {losses.Huber: functools.partial(cls, threshold=1.0),
                losses.Power: functools.partial(cls, exponent=2.0)}.get(cls, cls)
        assert dense.loss_spec(make).kind == KIND[cls._kind]


@pytest.mark.parametrize("bad,word", [
    (penalties.Log1p, "penalty"),
    (penalties.Quadratic, "penalty"),
    (functools.partial(penalties.Huber, threshold=1.0), "penalty"),
    (lambda deviations: deviations * 2.0, "_hip_spec"),
    (lambda deviations: None, "_hip_spec"),
    (functools.partial(losses.WeightedQuadratic, weights=torch.ones(1)), "weights of its own"),
    (functools.partial(losses.WeightedQuadratic, weights=3.0), "weights of its own"),
    (lambda deviations: losses.WeightedQuadratic(deviations, 1.0 / deviations), "weights of its own"),
    (losses.Quadratic(torch.ones(3)), "not a callable of the deviations"),
    (None, "not a callable of the deviations"),
])
def test_loss_spec_refuses(bad, word):
    with pytest.raises(ValueError, match=word) as info:
        dense.loss_spec(bad)
    assert "pymde_amd.losses" in str(info.value) and "default weights" in str(info.value)     # what is accepted


# ---------------------------------------------------------------- DenseMDE: errors before any device
def test_dense_mde_argument_errors():
    data = np.zeros((10, 4), dtype=np.float32)
    square = np.zeros((10, 10), dtype=np.float32)
    with pytest.raises(ValueError, match="exactly one of `data` and `distance_matrix`"):
        dense.DenseMDE()
    with pytest.raises(ValueError, match="exactly one of `data` and `distance_matrix`"):
        dense.DenseMDE(data, distance_matrix=square)
    with pytest.raises(ValueError, match=r"square matrix \[n, n\]"):
        dense.DenseMDE(distance_matrix=np.zeros((10, 9), dtype=np.float32))
    with pytest.raises(ValueError, match=r"square matrix \[n, n\]"):
        dense.DenseMDE(distance_matrix=np.zeros(10, dtype=np.float32))
    for dim in (9, 0, -1):
        with pytest.raises(ValueError, match=r"embedding_dim must lie in \[1, 8\]"):
            dense.DenseMDE(data, embedding_dim=dim)
        with pytest.raises(ValueError, match=r"embedding_dim must lie in \[1, 8\]"):
            dense.DenseMDE(distance_matrix=square, embedding_dim=dim)
    with pytest.raises(ValueError, match="penalty"):
        dense.DenseMDE(data, loss=penalties.Log1p)
    for scale in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="deviation_scale"):
            dense.DenseMDE(data, deviation_scale=scale)
    with pytest.raises(ValueError, match="'euclidean', 'cosine' and 'correlation'"):
        dense.DenseMDE(data, metric="manhattan")
    with pytest.raises(ValueError, match="unknown metric"):
        dense.DenseMDE(data, metric="chebyshev")
    with pytest.raises(ValueError, match="matrix"):
        dense.DenseMDE(np.zeros(10, dtype=np.float32))
    with pytest.raises(ValueError, match="at least two items"):
        dense.DenseMDE(distance_matrix=np.zeros((1, 1), dtype=np.float32))


class _Graph:
    edges, n_items = None, 10


def test_preserve_distances_dense_argument_errors():
    data = np.zeros((10, 4), dtype=np.float32)
    with pytest.raises(ValueError, match="Graph"):
        recipes.preserve_distances(_Graph(), dense=True)
    with pytest.raises(ValueError, match="Graph"):
        dense.DenseMDE(_Graph())
    for name in ("manhattan", "l1", "cityblock"):
        with pytest.raises(ValueError, match="'euclidean', 'cosine' and 'correlation'"):
            recipes.preserve_distances(data, dense=True, metric=name)
    with pytest.raises(ValueError, match="penalty"):
        recipes.preserve_distances(data, dense=True, loss=penalties.Log1p)
    with pytest.raises(ValueError, match=r"embedding_dim must lie in \[1, 8\]"):
        recipes.preserve_distances(data, dense=True, embedding_dim=9)


def test_the_public_names():
    import pymde_amd
    assert pymde_amd.DenseMDE is dense.DenseMDE
    assert dense.MAX_DIM == 8

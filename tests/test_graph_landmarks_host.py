"""Landmark MDS on graphs without a device: the argument errors of ``landmarks.select_graph``,
``LandmarkMDE.from_graph``, ``graph.distances_from`` and ``preserve_geodesics`` come before any device is required,
and the entry points that refuse a ``Graph`` refuse it as they did."""
import inspect

import numpy as np
import pytest
import torch

import pymde_amd
from pymde_amd import graph as G
from pymde_amd import landmarks, losses, preprocess


@pytest.fixture(autouse=True)
def no_device(monkeypatch):
    """Any attempt to pick a device fails the test: the refusals below must come first."""
    def refuse(*args, **kwargs):
        raise AssertionError("a device was required before the arguments were checked")
    monkeypatch.setattr(pymde_amd.util, "require_cuda_device", refuse)


def ring(n=10):
    """A ``Graph`` as its own constructors leave it, on the CPU (building its plan would need a device)."""
    edges = torch.stack([torch.arange(n - 1), torch.arange(1, n)], dim=1)
    return G.Graph._from_unique_edges(edges, torch.ones(n - 1), n)


DATA = np.arange(40, dtype=np.float32).reshape(10, 4)


def test_exported():
    assert pymde_amd.preserve_geodesics is pymde_amd.recipes.preserve_geodesics
    assert callable(G.distances_from) and callable(landmarks.select_graph) and callable(preprocess.neighbor_graph)
    names = list(inspect.signature(pymde_amd.LandmarkMDE.from_graph).parameters)
    assert names == ["graph", "landmarks", "embedding_dim", "loss", "constraint", "seed", "selection", "init",
                     "max_length", "weights"]
    defaults = inspect.signature(pymde_amd.preserve_geodesics).parameters
    assert defaults["loss"].default is losses.Quadratic and defaults["landmark_selection"].default == "farthest"
    assert defaults["n_neighbors"].default == 15 and defaults["landmarks"].default is None
    assert defaults["init"].default is None


@pytest.mark.parametrize("m", [0, 11, -1, 2.5, True])
def test_select_graph_m_out_of_range(m):
    with pytest.raises(ValueError, match="`m`"):
        landmarks.select_graph(ring(), m)


def test_select_graph_other_arguments():
    with pytest.raises(ValueError, match="Graph"):
        landmarks.select_graph(DATA, 3)
    for start in (-1, 10, 1.5):
        with pytest.raises(ValueError, match="start"):
            landmarks.select_graph(ring(), 3, start=start)


@pytest.mark.parametrize("m", [1, 10, 11, 2.5])
def test_from_graph_landmarks_out_of_range(m):
    with pytest.raises(ValueError, match="landmarks"):
        pymde_amd.LandmarkMDE.from_graph(ring(), m)


def test_from_graph_arguments():
    with pytest.raises(ValueError, match="kmeans"):
        pymde_amd.LandmarkMDE.from_graph(ring(), 4, selection="kmeans++")
    with pytest.raises(ValueError, match="selection"):
        pymde_amd.LandmarkMDE.from_graph(ring(), 4, selection="nearest")
    with pytest.raises(ValueError, match="Graph"):
        pymde_amd.LandmarkMDE.from_graph(DATA, 4)
    with pytest.raises(ValueError, match="power form"):
        pymde_amd.LandmarkMDE.from_graph(ring(), 4, weights=np.ones((10, 4)))
    with pytest.raises(ValueError, match="init"):
        pymde_amd.LandmarkMDE.from_graph(ring(), 4, init="spectral")
    with pytest.raises(ValueError, match="init"):
        pymde_amd.LandmarkMDE.from_graph(ring(), 4, init=None)
    with pytest.raises(ValueError, match="embedding_dim"):
        pymde_amd.LandmarkMDE.from_graph(ring(), 4, embedding_dim=9)
    with pytest.raises(ValueError, match="constraint"):
        pymde_amd.LandmarkMDE.from_graph(ring(), 4, constraint=pymde_amd.Standardized())


def test_distances_from_arguments():
    with pytest.raises(ValueError, match="Graph"):
        G.distances_from(DATA, [0])
    for bad in ([], [10], [-1], [0.5]):
        with pytest.raises(ValueError, match="sources"):
            G.distances_from(ring(), bad)
    negative = G.Graph._from_unique_edges(ring().edges, -torch.ones(9), 10)
    with pytest.raises(ValueError, match="non-negative"):
        G.distances_from(negative, [0])
    with pytest.raises(ValueError, match="non-negative"):
        G.distances_from(G.Graph._from_unique_edges(ring().edges, torch.full((9,), float("nan")), 10), [0])


def test_preserve_geodesics_arguments():
    with pytest.raises(ValueError, match="kmeans"):
        pymde_amd.preserve_geodesics(DATA, landmark_selection="kmeans++")
    with pytest.raises(ValueError, match="landmarks"):
        pymde_amd.preserve_geodesics(DATA, landmarks=10)
    with pytest.raises(ValueError, match="landmarks"):
        pymde_amd.preserve_geodesics(ring(), landmarks=10)
    with pytest.raises(ValueError, match="init"):
        pymde_amd.preserve_geodesics(DATA, init="spectral")
    with pytest.raises(ValueError, match="metric"):
        pymde_amd.preserve_geodesics(ring(), metric="cosine")
    with pytest.raises(ValueError, match="data matrix"):
        preprocess.neighbor_graph(ring(), 3)


def test_the_refusals_of_a_graph_stand():
    g = ring()
    with pytest.raises(ValueError):
        landmarks.select(g, 3)
    with pytest.raises(ValueError):
        pymde_amd.LandmarkMDE(g, 4)
    with pytest.raises(ValueError):
        pymde_amd.DenseMDE(g)
    with pytest.raises(ValueError):
        pymde_amd.DensePlacement(g, torch.zeros(10, 2), g)
    with pytest.raises(ValueError):
        pymde_amd.preserve_distances(g, landmarks=4)

"""Landmark MDS on graphs: ``landmarks.select_graph``, ``LandmarkMDE.from_graph``, ``preprocess.neighbor_graph`` and
``preserve_geodesics`` on top of ``graph.distances_from``.  The selection is held to a numpy replay over scipy's
float64 lengths (exact, the lengths being multiples of 2^-6); exact configurations (a path, a complete Euclidean
graph) must come back with the stress bound of an exact copy (tests/test_gpu_triangulate.py); Isomap is held to
scikit-learn's."""
import numpy as np
import pytest
import torch

import pymde_amd
from pymde_amd import classical, landmarks, losses, preprocess, quality
from pymde_amd import graph as G

import _graph_sssp_reference as ref

pytestmark = pytest.mark.gpu


def build(n, edges, lengths):
    return G.Graph.from_edges(torch.as_tensor(edges), torch.as_tensor(lengths), n_items=n)


# ---------------------------------------------------------------------------------------------- select_graph
@pytest.mark.parametrize("name", ["random", "cycle"])
def test_select_graph_equals_the_replay(name):
    n, edges, lengths = ref.random_graph() if name == "random" else ref.cycle()
    comp = ref.components(n, edges)
    c = len(set(comp))
    m = c + 6 if name == "random" else 12
    D = ref.distances_from(n, edges, lengths, np.arange(n))
    want = ref.farthest(D, m, start=7)
    got = landmarks.select_graph(build(n, edges, lengths), m, start=7)
    indices, radius = got.indices.cpu().numpy(), got.radius.cpu().numpy().astype(np.float64)
    assert got.indices.dtype == torch.int64 and got.nearest.dtype == torch.int64
    assert np.array_equal(indices, want[0]) and len(set(indices)) == m
    assert np.array_equal(radius, want[1]) and np.isinf(radius[0])
    assert np.array_equal(got.nearest.cpu().numpy(), want[2])
    assert np.array_equal(got.distance.cpu().numpy().astype(np.float64), want[3])
    assert (radius[2:] <= radius[1:-1]).all()         # (inf, ..., inf, then finite and falling)
    assert len(set(comp[indices[:c]])) == c          # every component before any gets a second landmark
    assert float(got.distance.max()) == want[3].max()
    # the draw of the first node: the same seed gives the same nodes
    a = landmarks.select_graph(build(n, edges, lengths), 3, seed=11)
    b = landmarks.select_graph(build(n, edges, lengths), 3, seed=11)
    assert torch.equal(a.indices, b.indices)


# ---------------------------------------------------------------------------------------------- exact configurations
def test_a_path_comes_back_as_a_line():
    n, edges, lengths = ref.path_graph()
    t = np.concatenate([[0.0], np.cumsum(lengths.astype(np.float64))]).astype(np.float32)
    mde = pymde_amd.LandmarkMDE.from_graph(build(n, edges, lengths), 48, embedding_dim=1, loss=losses.Quadratic,
                                           selection="farthest", init="classical", seed=0)
    assert isinstance(mde, pymde_amd.LandmarkMDE) and mde.metric is None and mde.selection == "farthest"
    assert mde.landmark_radius is not None and len(mde.landmarks) == 48 and len(mde.placed) == n - 48
    X0 = mde.initialization()
    score = float(quality.stress(t[:, None], X0, scale=1.0))
    print("stress at scale 1 of the start on a path: %.3g" % score)
    assert tuple(X0.shape) == (n, 1) and score <= 1e-3
    X = mde.embed(max_iter=5)
    assert mde.placement.init == "triangulation" and mde.X is X
    assert float(quality.stress(t[:, None], X, scale=1.0)) <= 1e-3


def test_a_complete_euclidean_graph():
    # 150 points in convex position (on an ellipse): no three are nearly collinear.  Among random points a few
    # triangles in ten thousand are so flat that fl(a) + fl(b), rounded, falls one ulp BELOW fl(c) -- the rounded
    # lengths then break the triangle inequality and the shortest path really is the detour.  Checked here on the
    # host, in float32: no two-hop detour undercuts an edge, and by the monotonicity of the rounded sum no longer one
    # does either.
    rng = np.random.default_rng(8)
    n = 150
    theta = 2.0 * np.pi * (np.arange(n) + 0.5 * rng.uniform(size=n)) / n
    P = np.stack([2.0 * np.cos(theta), np.sin(theta)], axis=1)
    full = np.sqrt(((P[:, None] - P[None]) ** 2).sum(2)).astype(np.float32)
    for k in range(n):
        via = full[:, k][:, None] + full[k][None, :]
        via[k, :] = via[:, k] = np.inf
        assert not (via < full).any()
    i, j = np.triu_indices(n, 1)
    lengths = full[i, j]
    g = build(n, np.stack([i, j], axis=1), lengths)
    D = G.distances_from(g, np.arange(n)).cpu().numpy()
    # so no detour is shorter than the edge, and the edge lengths come back bit for bit
    assert np.array_equal(D[i, j].view(np.int32), lengths.view(np.int32))
    assert np.array_equal(D[j, i].view(np.int32), lengths.view(np.int32)) and (np.diag(D) == 0).all()
    mde = pymde_amd.LandmarkMDE.from_graph(g, 32, embedding_dim=2, loss=losses.Quadratic, selection="farthest",
                                           init="classical", seed=0)
    data = P.astype(np.float32)
    assert float(quality.stress(data, mde.initialization(), scale=1.0)) <= 1e-3
    assert float(quality.stress(data, mde.embed(max_iter=5), scale=1.0)) <= 1e-3


# ---------------------------------------------------------------------------------------------- missing pairs
def test_two_components_leave_pairs_out():
    n, edges, lengths = ref.two_cycles(60)
    g = build(n, edges, lengths)
    comp = ref.components(n, edges)
    mde = pymde_amd.LandmarkMDE.from_graph(g, 16, selection="farthest", seed=0)
    assert mde.init == "random"
    X = mde.embed(max_iter=20)
    assert tuple(X.shape) == (n, 2) and bool(torch.isfinite(X).all())
    at, placed = mde.landmarks.numpy(), mde.placed.numpy()
    assert len(set(comp[at])) == 2
    reach = comp[placed][:, None] == comp[at][None, :]
    assert np.array_equal(mde.placement._weights.W.cpu().numpy(), reach.astype(np.float32))
    assert mde.placement.p == int(reach.sum())
    block = comp[at][:, None] == comp[at][None, :]
    assert mde.landmark_problem.p == (int(block.sum()) - 16) // 2
    with pytest.raises(ValueError, match="every"):
        pymde_amd.LandmarkMDE.from_graph(g, 16, selection="farthest", init="classical", seed=0)
    with pytest.raises(ValueError, match="missing pairs"):
        pymde_amd.LandmarkMDE.from_graph(g, 16, selection="farthest", weights=1.0, seed=0)
    # a connected graph builds no weight matrix
    n1, e1, l1 = ref.cycle()
    whole = pymde_amd.LandmarkMDE.from_graph(build(n1, e1, l1), 16, seed=0)
    assert whole._W is None and whole.landmark_problem._weights is None


@pytest.mark.parametrize("selection", ["uniform", "farthest"])
def test_a_node_joined_to_no_landmark(selection):
    n, edges, lengths = ref.two_cycles(60, extra=1)
    with pytest.raises(ValueError, match="1 of the 121 nodes"):
        pymde_amd.LandmarkMDE.from_graph(build(n, edges, lengths), 30, selection=selection, seed=0)


# ---------------------------------------------------------------------------------------------- Isomap
def rolled_strip(n=400, seed=12):
    rng = np.random.default_rng(seed)
    t = 1.5 * np.pi * (1.0 + 1.2 * rng.uniform(size=n))
    return np.stack([t * np.cos(t), 12.0 * rng.uniform(size=n), t * np.sin(t)], axis=1).astype(np.float32)


def _procrustes_difference(A, B):
    """|A Q - B|_F / |B|_F at the best orthogonal Q, both centred (float64)."""
    A, B = A - A.mean(0), B - B.mean(0)
    U, _, Vt = np.linalg.svd(A.T @ B)
    return np.linalg.norm(A @ (U @ Vt) - B) / np.linalg.norm(B)


def test_isomap_against_scikit_learn():
    from scipy.sparse.csgraph import connected_components
    from sklearn.manifold import Isomap
    from sklearn.neighbors import kneighbors_graph
    data = rolled_strip()
    n = len(data)
    knn = kneighbors_graph(data, 10, mode="distance")
    assert connected_components(knn, directed=False)[0] == 1
    dense = Isomap(n_neighbors=10, n_components=2, eigen_solver="dense").fit_transform(data).astype(np.float64)
    arpack = Isomap(n_neighbors=10, n_components=2, eigen_solver="arpack").fit_transform(data).astype(np.float64)
    own = _procrustes_difference(arpack, dense)
    # measured on an MI355X (profiles/r25_graph_landmarks.txt): scikit-learn's dense against its arpack solver
    # 2.42e-07, this package against scikit-learn 2.69e-06; the bound is ten times the former, or 1e-4, whichever is
    # larger
    bound = max(10.0 * own, 1e-4)
    g = preprocess.neighbor_graph(data, 10)
    D = G.distances_from(g, np.arange(n))
    fit = classical.classical_mds(distance_matrix=D)
    got = _procrustes_difference(fit.X.cpu().numpy().astype(np.float64), dense)
    print("Isomap: scikit-learn dense against arpack %.3g, this package against scikit-learn %.3g (bound %.3g)"
          % (own, got, bound))
    assert got <= bound


# ---------------------------------------------------------------------------------------------- the front door
def test_neighbor_graph():
    rng = np.random.default_rng(13)
    data = rng.standard_normal((400, 32)).astype(np.float32)
    g = preprocess.neighbor_graph(data, 10)
    edges, _ = preprocess.k_nearest_neighbors(data, 10)
    assert isinstance(g, G.Graph) and g.n_items == 400
    assert torch.equal(g.edges, edges)
    e = g.edges.cpu().numpy()
    x = data.astype(np.float64)
    want = np.sqrt(((x[e[:, 0]] - x[e[:, 1]]) ** 2).sum(1))
    error = np.abs(g.distances.cpu().numpy().astype(np.float64) - want) / want
    print("neighbor_graph: largest relative error of a length %.3g (bound %.3g)" % (error.max(), 32 * 2.0 ** -23))
    assert error.max() <= 32 * 2.0 ** -23
    with pytest.raises(ValueError, match="data matrix"):
        preprocess.neighbor_graph(g, 10)


def test_preserve_geodesics():
    data = rolled_strip()
    mde = pymde_amd.preserve_geodesics(data, n_neighbors=10, landmarks=40, seed=0)
    assert isinstance(mde, pymde_amd.LandmarkMDE) and mde.init == "classical" and mde.selection == "farthest"
    X = mde.embed(max_iter=10)
    assert tuple(X.shape) == (400, 2) and bool(torch.isfinite(X).all())
    g = preprocess.neighbor_graph(data, 10)
    again = pymde_amd.preserve_geodesics(g, landmarks=40, seed=0)
    assert torch.equal(again.landmarks, mde.landmarks)
    X2 = again.embed(max_iter=10)
    assert tuple(X2.shape) == (400, 2) and bool(torch.isfinite(X2).all())
    # landmarks=None: min(1000, n // 2); a disconnected graph starts at random
    n, edges, lengths = ref.two_cycles(60)
    split = pymde_amd.preserve_geodesics(build(n, edges, lengths), seed=0)
    assert len(split.landmarks) == 60 and split.init == "random"

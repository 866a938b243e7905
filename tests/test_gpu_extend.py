"""``extend_embedding``: new points placed into an existing embedding through an ``Anchored`` problem whose
attractive edges come from the query-against-corpus search.  Structure of the problem, the solve, where
the new points land, and the variants."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
N_OLD, N_NEW, CLUSTERS = 2000, 203, 4
# the default n_neighbors: the preserve_neighbors rule on n_old -- 1 % of all pairs as edges, within [5, 15]
K = int(max(min(15, (N_OLD * (N_OLD - 1) / 2) * 0.01 / N_OLD), 5))
assert K == 9


@pytest.fixture(scope="module")
def blobs():
    """Four unit-variance Gaussian clusters in 10-d with centres 50 apart; their embedding ``X`` is four
    unit-variance 2-D blobs at the corners of a square of side 50.  Read-only."""
    rng = np.random.default_rng(0)
    centres = np.zeros((CLUSTERS, 10))
    centres[np.arange(CLUSTERS), np.arange(CLUSTERS)] = 50.0 / np.sqrt(2.0)       # |c_i - c_j| = 50
    corners = np.array([[0.0, 0.0], [50.0, 0.0], [0.0, 50.0], [50.0, 50.0]])
    old_labels = np.arange(N_OLD) % CLUSTERS
    new_labels = rng.integers(0, CLUSTERS, N_NEW)
    data = (centres[old_labels] + rng.standard_normal((N_OLD, 10))).astype(np.float32)
    new = (centres[new_labels] + rng.standard_normal((N_NEW, 10))).astype(np.float32)
    X = (corners[old_labels] + rng.standard_normal((N_OLD, 2))).astype(np.float32)
    return {"data": torch.tensor(data, device=DEV), "new": torch.tensor(new, device=DEV),
            "X": torch.tensor(X, device=DEV), "old_labels": old_labels, "new_labels": new_labels}


@pytest.fixture(scope="module")
def problem(blobs):
    import pymde_amd
    return pymde_amd.extend_embedding(blobs["data"], blobs["X"], blobs["new"], seed=0)


def _rows(t):
    return set(map(tuple, t.cpu().numpy().tolist()))


# ---------------------------------------------------------------- structure
def test_edges_touch_a_new_item_and_are_distinct(problem):
    e = problem.edges
    assert int(problem.n_items) == N_OLD + N_NEW and int(problem.embedding_dim) == 2
    assert bool((e >= N_OLD).any(1).all())
    assert bool((e >= 0).all()) and bool((e < N_OLD + N_NEW).all())
    assert bool((e[:, 0] < e[:, 1]).all())
    assert len(_rows(e)) == e.shape[0]


def test_attractive_edges_are_the_cross_neighbours(problem, blobs):
    from pymde_amd import preprocess
    idx, dist = preprocess.cross_nearest_neighbors(blobs["new"], blobs["data"], K)
    assert bool((idx >= 0).all())
    want = {(int(c), N_OLD + q) for q, row in enumerate(idx.cpu().numpy()) for c in row}
    w = problem.distortion_function.weights
    attractive = problem.edges[w > 0]
    assert attractive.shape[0] == N_NEW * K and _rows(attractive) == want
    assert bool((w[w > 0] == 1).all())


def test_repulsive_edges(problem):
    w = problem.distortion_function.weights
    attractive, repulsive = problem.edges[w > 0], problem.edges[w < 0]
    assert int((w == 0).sum()) == 0 and bool((w[w < 0] == -1).all())
    assert repulsive.shape[0] == int(1 * attractive.shape[0])
    assert not (_rows(repulsive) & _rows(attractive))
    assert bool((repulsive[:, 0] != repulsive[:, 1]).all())
    assert bool((repulsive[:, 0] >= N_OLD).any()), "pairs of two new items are drawn as well"


def test_repulsive_fraction_and_seed(problem, blobs):
    import pymde_amd
    again = pymde_amd.extend_embedding(blobs["data"], blobs["X"], blobs["new"], seed=0)
    assert torch.equal(again.edges, problem.edges)
    assert torch.equal(again.distortion_function.weights, problem.distortion_function.weights)
    assert torch.equal(again._X_init, problem._X_init)
    other = pymde_amd.extend_embedding(blobs["data"], blobs["X"], blobs["new"], seed=1, repulsive_fraction=0.37,
                                       n_neighbors=7)
    w = other.distortion_function.weights
    assert int((w > 0).sum()) == N_NEW * 7 and int((w < 0).sum()) == int(0.37 * N_NEW * 7)
    assert len(_rows(other.edges)) == other.edges.shape[0]
    assert not _rows(other.edges[w < 0]) <= _rows(problem.edges)


def test_start_is_the_neighbour_mean(problem, blobs):
    from pymde_amd import preprocess
    X0 = problem._X_init
    assert X0.shape == (N_OLD + N_NEW, 2) and X0.dtype == torch.float32
    assert torch.equal(X0[:N_OLD], blobs["X"])
    assert bool((problem.distances(X0) > 0).all())            # no zero-length edge: the start was not perturbed
    idx, _ = preprocess.cross_nearest_neighbors(blobs["new"], blobs["data"], K)
    X64 = blobs["X"].double().cpu().numpy()
    want = X64[idx.cpu().numpy()].mean(1)
    # a float32 sum of at most 15 terms of size <= max|X| and one division: 16 roundings of 2^-24 each
    atol = 16 * 2.0 ** -24 * np.abs(X64).max()
    np.testing.assert_allclose(X0[N_OLD:].double().cpu().numpy(), want, rtol=0, atol=atol)


# ---------------------------------------------------------------- solve and placement
@pytest.fixture(scope="module")
def solved(problem):
    start = float(problem.average_distortion(problem._X_init))
    problem.embed()
    return problem, start


def test_solve_keeps_the_old_rows_and_lowers_the_distortion(solved, blobs):
    mde, start = solved
    assert torch.equal(mde.X[:N_OLD], blobs["X"])
    assert bool(torch.isfinite(mde.X[N_OLD:]).all())
    final = float(mde.average_distortion(mde.X))
    print("average distortion: %.6f at the start, %.6f after embed()" % (start, final))
    assert final <= start


def test_new_points_land_in_their_own_cluster(solved, blobs):
    mde, _ = solved
    X = blobs["X"].double().cpu().numpy()
    centroids = np.stack([X[blobs["old_labels"] == c].mean(0) for c in range(CLUSTERS)])
    Z = mde.X[N_OLD:].double().cpu().numpy()
    d = np.linalg.norm(Z[:, None, :] - centroids[None, :, :], axis=2)
    nearest = d.argmin(1)
    wrong = np.nonzero(nearest != blobs["new_labels"])[0]
    print("largest distance of a new point to its own centroid: %.3f"
          % d[np.arange(N_NEW), blobs["new_labels"]].max())
    assert wrong.size == 0, wrong


# ---------------------------------------------------------------- variants
def test_without_repulsion(blobs):
    import pymde_amd
    mde = pymde_amd.extend_embedding(blobs["data"], blobs["X"], blobs["new"], repulsive_penalty=None, seed=0)
    assert mde.edges.shape[0] == N_NEW * K
    assert isinstance(mde.distortion_function, pymde_amd.penalties.Log1p)
    mde.embed(max_iter=30)
    assert torch.equal(mde.X[:N_OLD], blobs["X"]) and bool(torch.isfinite(mde.X).all())


def test_a_new_point_without_neighbour_raises_with_the_count(blobs):
    import pymde_amd
    from pymde_amd import preprocess
    _, nearest = preprocess.cross_nearest_neighbors(blobs["new"], blobs["data"], 1)
    srt = np.sort(nearest[:, 0].double().cpu().numpy())
    assert srt[-3] - srt[-4] > 1e-4                               # the bound sits in a gap float32 resolves
    md = 0.5 * (srt[-4] + srt[-3])                                # three new points have nothing within it
    with pytest.raises(ValueError, match=r"\b3 of the 203 new points"):
        pymde_amd.extend_embedding(blobs["data"], blobs["X"], blobs["new"], max_distance=float(md), seed=0)
    mde = pymde_amd.extend_embedding(blobs["data"], blobs["X"], blobs["new"], max_distance=float(srt[-1]) + 1.0,
                                     seed=0)
    w = mde.distortion_function.weights
    assert 0 < int((w > 0).sum()) <= N_NEW * K


def test_cosine_builds(blobs):
    import pymde_amd
    from pymde_amd import preprocess
    mde = pymde_amd.extend_embedding(blobs["data"], blobs["X"], blobs["new"], metric="cosine", seed=0)
    idx, _ = preprocess.cross_nearest_neighbors(blobs["new"], blobs["data"], K, metric="cosine")
    want = {(int(c), N_OLD + q) for q, row in enumerate(idx.cpu().numpy()) for c in row}
    w = mde.distortion_function.weights
    assert _rows(mde.edges[w > 0]) == want
    with pytest.raises(ValueError, match="Manhattan"):
        pymde_amd.extend_embedding(blobs["data"], blobs["X"], blobs["new"], metric="manhattan")

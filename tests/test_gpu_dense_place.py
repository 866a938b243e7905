"""pymde_amd.DensePlacement and preserve_distances(landmarks=...) on the GPU: the rectangular dense problem equals the
edge-list problem over the same bipartite pairs (the edge-list path is the yardstick: its kernels are checked against
the oracle elsewhere), from data matrices and from a rectangular distance matrix; its embed() reaches what the
Anchored edge-list problem reaches and leaves the embedded rows alone; landmark MDS reaches the stress of the full
dense problem on data that can be embedded exactly.
Tolerances: LOSS_RTOL and assert_grad_close of tests/conftest.py."""
import numpy as np
import pytest
import torch

from conftest import GRAD_ATOL_REL, GRAD_RTOL, LOSS_RTOL, assert_grad_close

pytestmark = pytest.mark.gpu
DEV = "cuda"
N_OLD, N_NEW, NF = 300, 150, 20


# ---------------------------------------------------------------- helpers
_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _data():
    """(data [N_OLD, NF], new_data [N_NEW, NF], X_old [N_OLD, 2], X_new [N_NEW, 2]) float32; the data are centred at
    the mean of the old rows."""
    def make():
        rng = np.random.default_rng(21)
        rows = rng.standard_normal((N_OLD + N_NEW, NF)) * rng.uniform(0.5, 2.0, NF)
        rows = (rows - rows[:N_OLD].mean(0)).astype(np.float32)
        X = (rng.standard_normal((N_OLD + N_NEW, 2)) * 3.0).astype(np.float32)
        return rows[:N_OLD], rows[N_OLD:], X[:N_OLD], X[N_OLD:]
    return _cached("data", make)


def _distances64(new, old):
    new, old = new.astype(np.float64), old.astype(np.float64)
    return np.sqrt(((new[:, None, :] - old[None, :, :]) ** 2).sum(-1))


def _cosine64(new, old):
    new, old = new.astype(np.float64), old.astype(np.float64)
    new = new / np.linalg.norm(new, axis=1, keepdims=True)
    old = old / np.linalg.norm(old, axis=1, keepdims=True)
    return 1.0 - new @ old.T


def _edge_problem(D, loss, X_old=None):
    """The edge-list MDE over the bipartite pairs {(j, N_OLD + i)} with the deviations D [n_new, n_old] (float64,
    rounded once to float32); Anchored at X_old when given."""
    import pymde_amd
    n_new, n_old = D.shape
    i, j = np.divmod(np.arange(n_new * n_old, dtype=np.int64), n_old)
    edges = torch.as_tensor(np.stack([j, n_old + i], 1)).to(DEV)
    deviations = torch.as_tensor(D[i, j].astype(np.float32)).to(DEV)
    constraint = None
    if X_old is not None:
        constraint = pymde_amd.Anchored(torch.arange(n_old, device=DEV), torch.as_tensor(X_old).to(DEV))
    return pymde_amd.MDE(n_old + n_new, 2, edges, loss(deviations), constraint=constraint)


def _edge_value_and_grad(edge, X_old, X_new):
    Xg = torch.as_tensor(np.concatenate([X_old, X_new])).to(DEV).requires_grad_(True)
    value = edge.average_distortion(Xg)
    value.backward()
    return float(value.detach()), Xg.grad.cpu().numpy()[X_old.shape[0]:]


def _value_and_grad(problem, X):
    Xg = torch.as_tensor(X).to(DEV).clone().requires_grad_(True)
    value = problem.average_distortion(Xg)
    assert value.dim() == 0 and value.dtype == torch.float32
    value.backward()
    return float(value.detach()), Xg.grad.cpu().numpy()


def _compare(label, got, want):
    """Prints the worst error of the value and the gradient next to each bound, then asserts."""
    (value, grad), (wvalue, wgrad) = got, want
    e_value = abs(value - wvalue) / abs(wvalue)
    allow = GRAD_ATOL_REL * float(np.abs(wgrad).max()) + GRAD_RTOL * np.abs(wgrad.astype(np.float64))
    e_grad = float((np.abs(grad.astype(np.float64) - wgrad) / allow).max())
    print("%s: value %.8g against %.8g, rel. error %.3g (bound %.3g); gradient error %.3g of its allowance (rtol %.3g, "
          "atol %.3g max|g|)" % (label, value, wvalue, e_value, LOSS_RTOL, e_grad, GRAD_RTOL, GRAD_ATOL_REL))
    assert e_value <= LOSS_RTOL
    assert_grad_close(grad, wgrad)


# ---------------------------------------------------------------- 1. the edge-list problem over the bipartite pairs
@pytest.mark.parametrize("loss", ["Absolute", "Quadratic", "WeightedQuadratic"])
def test_placement_equals_the_edge_list_problem(loss):
    import pymde_amd
    data, new, X_old, X_new = _data()
    L = getattr(pymde_amd.losses, loss)
    D = _cached("D", lambda: _distances64(new, data))
    place = pymde_amd.DensePlacement(data, X_old, new, loss=L)
    assert place.n_items == N_NEW and place.p == N_NEW * N_OLD and place.embedding_dim == 2
    assert place.metric == "euclidean" and place.X is None and place.value is None
    _compare(loss, _value_and_grad(place, X_new), _edge_value_and_grad(_edge_problem(D, L), X_old, X_new))


def test_cosine():
    import pymde_amd
    data, new, X_old, X_new = _data()
    data, new = data + 0.5, new + 0.5
    X_old, X_new = X_old * 0.1, X_new * 0.1                     # cosine distances lie in [0, 2]
    place = pymde_amd.DensePlacement(data, X_old, new, metric="cosine")
    assert place.metric == "cosine"
    edge = _edge_problem(_cosine64(new, data), pymde_amd.losses.Absolute)
    _compare("cosine", _value_and_grad(place, X_new), _edge_value_and_grad(edge, X_old, X_new))


def test_distance_matrix_gives_the_result_of_data():
    import pymde_amd
    data, new, X_old, X_new = _data()
    D = _cached("D", lambda: _distances64(new, data))
    for loss in (pymde_amd.losses.Absolute, pymde_amd.losses.Quadratic):
        from_data = pymde_amd.DensePlacement(data, X_old, new, loss=loss)
        from_matrix = pymde_amd.DensePlacement(None, X_old, None, loss=loss, distance_matrix=D)
        assert from_matrix.n_items == N_NEW and from_matrix.p == N_NEW * N_OLD and from_matrix.metric is None
        _compare("distance_matrix %s" % loss.__name__, _value_and_grad(from_matrix, X_new),
                 _value_and_grad(from_data, X_new))
    as_tensor = pymde_amd.DensePlacement(None, torch.as_tensor(X_old).to(DEV), None, loss=pymde_amd.losses.Quadratic,
                                         distance_matrix=torch.as_tensor(D).to(DEV))
    assert _value_and_grad(as_tensor, X_new)[0] == _value_and_grad(from_matrix, X_new)[0]


def test_distance_matrix_is_checked_on_the_gpu():
    import pymde_amd
    X_old = np.arange(10.0, dtype=np.float32).reshape(5, 2)
    D = np.abs(np.subtract.outer(np.arange(3.0), np.arange(5.0)))           # rectangular, and not symmetric
    pymde_amd.DensePlacement(None, X_old, None, distance_matrix=D)
    for poison, word in ((np.nan, "finite"), (np.inf, "finite"), (-1.0, "non-negative")):
        bad = D.copy()
        bad[1, 3] = poison
        with pytest.raises(ValueError, match=word):
            pymde_amd.DensePlacement(None, X_old, None, distance_matrix=bad)
    data = np.ones((5, 3), dtype=np.float32)
    bad = np.ones((3, 3), dtype=np.float32)
    bad[2, 1] = np.nan
    with pytest.raises(ValueError, match="new_data"):
        pymde_amd.DensePlacement(data, X_old, bad)
    with pytest.raises(ValueError, match="`data`"):
        pymde_amd.DensePlacement(bad[[0, 1, 2, 0, 1]], X_old, data[:3])


def test_item_distortions():
    import pymde_amd
    data, new, X_old, X_new = _data()
    place = pymde_amd.DensePlacement(data, X_old, new, loss=pymde_amd.losses.Absolute)
    value = float(place.average_distortion(torch.as_tensor(X_new).to(DEV)))
    items = place.item_distortions(torch.as_tensor(X_new))
    assert items.dtype == torch.float32 and items.is_cuda and items.shape == (N_NEW,)
    total, want = float(items.double().sum()) * N_OLD, place.p * value
    print("item_distortions sum * n_old %.8g against p * value %.8g (bound %.3g)" % (total, want, LOSS_RTOL))
    assert abs(total - want) <= LOSS_RTOL * want
    with pytest.raises(ValueError, match="embed"):
        place.item_distortions()


# ---------------------------------------------------------------- 2. embed()
def test_embed_reaches_what_the_anchored_edge_list_problem_reaches():
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
    edge = _edge_problem(_distances64(new, data), quadratic, X_old=data)
    place = pymde_amd.DensePlacement(data, X_old, new, loss=quadratic)
    initial = float(place.average_distortion(start))
    edge.embed(X=torch.cat([X_old, start]), **kwargs)
    assert place.X is None and place.solve_stats is None and place.value is None and place.residual_norm is None
    X = place.embed(X=start.clone(), **kwargs)
    print("initial value %.6g; final value placement %.6g in %d iterations, anchored edge list %.6g in %d iterations"
          % (initial, place.value, place.solve_stats.iterations, edge.value, edge.solve_stats.iterations))
    assert X is place.X and X.shape == (N_NEW, 2) and X.is_cuda and X.dtype == torch.float32
    assert place.solve_stats is not None and place.solve_stats.iterations > 0
    assert place.value is not None and place.residual_norm is not None
    assert place.value <= 1.05 * edge.value + 1e-6 * initial
    both = place.embedding()
    assert both.shape == (N_OLD + N_NEW, 2) and torch.equal(both[:N_OLD], kept) and torch.equal(both[N_OLD:], X)
    assert torch.equal(X_old, kept)                             # the caller's tensor is as it was
    assert abs(float(place.average_distortion()) - place.value) <= 1e-4 * initial     # X=None: the stored rows
    # the default start: the mean of the d + 1 = 3 nearest embedded rows
    again = pymde_amd.DensePlacement(data, X_old, new, loss=quadratic)
    first = again.initialization()
    assert first.shape == (N_NEW, 2) and bool(torch.isfinite(first).all())
    at_default = float(again.average_distortion(first))
    again.embed(**kwargs)
    print("default start: value %.6g, after embed() %.6g" % (at_default, again.value))
    assert again.value < at_default and again.value < initial
    # from either source it is the mean of the three nearest embedded rows
    D = _distances64(new, data)
    want = data.astype(np.float64)[np.argsort(D, 1, kind="stable")[:, :3]].mean(1)
    from_matrix = pymde_amd.DensePlacement(None, X_old, None, loss=quadratic, distance_matrix=D)
    for got in (first, from_matrix.initialization()):
        np.testing.assert_allclose(got.cpu().numpy(), want, rtol=1e-5, atol=1e-5)


# ---------------------------------------------------------------- 3. landmark MDS
def test_landmarks_reach_the_stress_of_the_full_problem():
    import pymde_amd
    from pymde_amd import quality
    n, m = 600, 150
    rng = np.random.default_rng(23)
    coords = rng.standard_normal((n, 2)) * np.array([3.0, 1.0])
    coords = coords - coords.mean(0)
    basis = np.linalg.qr(rng.standard_normal((5, 2)))[0]        # orthonormal columns: the rows are exactly planar
    data = (coords @ basis.T).astype(np.float32)
    start = torch.as_tensor((coords + 0.1 * coords.std() * rng.standard_normal((n, 2))).astype(np.float32)).to(DEV)
    kwargs = dict(eps=1e-6, max_iter=200)
    quadratic = pymde_amd.losses.Quadratic
    landmark = pymde_amd.preserve_distances(data, landmarks=m, seed=0, loss=quadratic)
    assert isinstance(landmark, pymde_amd.LandmarkMDE) and landmark.X is None and landmark.placement is None
    assert landmark.landmarks.dtype == torch.int64 and landmark.landmarks.shape == (m,)
    assert len(set(landmark.landmarks.tolist())) == m
    assert torch.equal(landmark.landmarks, pymde_amd.preserve_distances(data, landmarks=m, seed=0).landmarks)
    assert not torch.equal(landmark.landmarks, pymde_amd.preserve_distances(data, landmarks=m, seed=1).landmarks)
    X = landmark.embed(X=start.clone(), **kwargs)
    full = pymde_amd.DenseMDE(data, loss=quadratic)
    X_full = full.embed(X=start.clone(), **kwargs)
    s_full = quality.stress(data, X_full, scale=1.0)
    s_landmark = quality.stress(data, X, scale=1.0)
    print("stress at scale 1: full dense problem %.6g (%d iterations), %d landmarks %.6g (%d + %d iterations); start %.6g"
          % (s_full, full.solve_stats.iterations, m, s_landmark, landmark.solve_stats.landmarks.iterations,
             landmark.solve_stats.placement.iterations, quality.stress(data, start, scale=1.0)))
    assert s_landmark <= s_full + 1e-3
    assert X is landmark.X and X.shape == (n, 2) and X.is_cuda and X.dtype == torch.float32
    scale = float(X.abs().max())
    assert float(X.double().mean(0).abs().max()) <= 1e-5 * scale
    shift = X[landmark.landmarks.to(DEV)] - landmark.landmark_problem.X
    assert float((shift - shift[0]).abs().max()) <= 4.0 * 2.0 ** -23 * scale     # one constant row, to float32 rounding
    assert landmark.landmark_problem.n_items == m and landmark.placement.n_items == n - m
    assert landmark.placement.n_old == m and landmark.value == landmark.placement.value
    assert landmark.solve_stats.landmarks is landmark.landmark_problem.solve_stats
    assert landmark.solve_stats.placement is landmark.placement.solve_stats
    # the default start runs too
    assert pymde_amd.preserve_distances(data, landmarks=m, seed=0, loss=quadratic).embed(max_iter=20).shape == (n, 2)

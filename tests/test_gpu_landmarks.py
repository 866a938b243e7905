"""Landmark selection on the GPU (csrc/mde_landmarks.hip, pymde_amd.landmarks): the exact sequence of the numpy
replay on integer data, float64 replays along the kernel's own choices on real-valued data, duplicates, determinism
(runs, seeds, start, grid), the metrics, sparse input, coverage against the uniform draw, and the landmark recipe end
to end under the three selections.

Tolerances.  A float32 squared distance of nf features in difference form carries a relative error of at most about
``(nf + 2) 2^-24`` (one rounding per difference, doubled by the square, and nf - 1 additions): ``EPS(nf)`` below.  The
farthest point is therefore within ``2 EPS`` of the float64 maximum, the k-means++ target within ``2 EPS total`` of the
chosen row's float64 prefix interval, and distances agree with float64 to ``EPS``.

Stress at scale 1 of the 600 x 30 end-to-end case (Quadratic loss, 150 landmarks, at most 100 iterations per stage),
as ``test_end_to_end`` prints it: 0.955103 for the start, then uniform 0.212109, farthest 0.211856, kmeans++ 0.229724.
No order among the three is asserted."""
import numpy as np
import pytest
import torch

import pymde_amd
from pymde_amd import landmarks, metrics, quality

import _landmarks_reference as ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
METHODS = [ref.FARTHEST, ref.KMEANSPP]


def EPS(nf):
    return (nf + 2) * 2.0 ** -24


def _prepared(data):
    """The float32 rows the Euclidean selection runs on (``quality._self_rows``), as float64 on the host."""
    rows = quality._self_rows(torch.as_tensor(data), metrics.EUCLIDEAN, torch.device(DEV), "data")
    return rows.cpu().numpy().astype(np.float64)


def _integers(n, nf, seed=0):
    return np.random.default_rng(seed).integers(0, 4, (n, nf)).astype(np.float32)


# ---------------------------------------------------------------- exact sequence on integer data
@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("n,nf", [(3001, 20), (130, 3), (1037, 1),
                                  # and one shape for every other number of lanes that share a row
                                  (260, 6), (515, 8), (300, 16), (515, 100), (200, 256), (150, 1030)])
def test_exact_sequence_on_integer_data(n, nf, method):
    data = _integers(n, nf)
    m = 64
    want_idx, want_r2, want_near, want_d2 = ref.select(data, m, method, 0, seed=11)
    got = landmarks.select(data, m, method=method, start=0, seed=11)
    assert got.indices.dtype == torch.int64 and got.nearest.dtype == torch.int64
    assert got.radius.dtype == torch.float32 and got.distance.dtype == torch.float32
    assert all(t.is_cuda for t in got)
    assert got.indices.cpu().tolist() == want_idx.tolist()
    assert got.nearest.cpu().tolist() == want_near.tolist()
    # every squared distance is a small integer: exact in float32, and the root is the same operation on both sides
    assert torch.equal(got.radius, torch.as_tensor(want_r2.astype(np.float32)).to(DEV).sqrt())
    assert torch.equal(got.distance, torch.as_tensor(want_d2.astype(np.float32)).to(DEV).sqrt())
    assert float(got.radius[0]) == float("inf")


def test_one_landmark_and_one_row():
    data = _integers(50, 5, seed=2)
    for method in METHODS:
        got = landmarks.select(data, 1, method=method, start=9, seed=0)
        assert got.indices.tolist() == [9] and got.radius.tolist() == [float("inf")]
        assert got.nearest.tolist() == [0] * 50
        want = torch.as_tensor(ref.d2_to(data.astype(np.float64), 9).astype(np.float32)).to(DEV).sqrt()
        assert torch.equal(got.distance, want)
        one = landmarks.select(data[:1], 1, method=method, seed=4)
        assert one.indices.tolist() == [0] and one.distance.tolist() == [0.0] and one.nearest.tolist() == [0]


# ---------------------------------------------------------------- real-valued data
REAL_CASES = [(1037, 50, 64), (300, 784, 32), (1037, 3, 64), (257, 130, 32), (130, 3, 130)]


@pytest.fixture(scope="module")
def real_data():
    return {(n, nf): ref.blobs_with_far_group(n, nf, seed=n + nf) for n, nf, _ in REAL_CASES}


def _check_final_state(X64, got, nf):
    """``distance`` and ``nearest`` against the float64 state along the same choices, up to ties within EPS."""
    idx = got.indices.cpu().numpy()
    *_, (m, mind2, _) = ref.replay(X64, idx)
    d2_gpu = got.distance.cpu().numpy().astype(np.float64) ** 2
    scale = np.maximum(mind2, 1e-300)
    assert np.all(np.abs(d2_gpu - mind2) <= 2.0 * EPS(nf) * scale + 1e-30), float(np.abs(d2_gpu / scale - 1).max())
    assert np.all(d2_gpu[idx] == 0.0)
    near = got.nearest.cpu().numpy()
    assert near.min() >= 0 and near.max() < m
    diff = X64 - X64[idx[near]]
    to_named = np.einsum("ij,ij->i", diff, diff)
    assert np.all(to_named <= mind2 * (1.0 + 2.0 * EPS(nf)) + 1e-30)


@pytest.mark.parametrize("n,nf,m", REAL_CASES)
def test_farthest_follows_the_float64_maximum(real_data, n, nf, m):
    data = real_data[(n, nf)]
    X64 = _prepared(data)
    got = landmarks.select(data, m, method="farthest", start=7, seed=0)
    idx = got.indices.cpu().numpy()
    assert idx[0] == 7 and len(set(idx.tolist())) == m
    radius = got.radius.cpu().numpy().astype(np.float64)
    assert radius[0] == np.inf and np.all(np.diff(radius[1:]) <= 0.0)
    worst = 0.0
    for step in ref.replay(X64, idx):
        if step[0] == m:
            break
        t, mind2 = step
        worst = max(worst, 1.0 - mind2[idx[t]] / mind2.max())
        assert mind2[idx[t]] >= mind2.max() * (1.0 - 2.0 * EPS(nf)), (t, worst)
        assert abs(radius[t] ** 2 - mind2[idx[t]]) <= 2.0 * EPS(nf) * mind2[idx[t]]
    print("farthest %d x %d, m = %d: largest shortfall to the float64 maximum %.3g (bound %.3g)"
          % (n, nf, m, worst, 2.0 * EPS(nf)))
    _check_final_state(X64, got, nf)


@pytest.mark.parametrize("n,nf,m", REAL_CASES)
def test_kmeanspp_follows_the_float64_prefix_sum(real_data, n, nf, m):
    data = real_data[(n, nf)]
    X64 = _prepared(data)
    seed = 5
    got = landmarks.select(data, m, method="kmeans++", start=7, seed=seed)
    idx = got.indices.cpu().numpy()
    assert idx[0] == 7 and len(set(idx.tolist())) == m
    worst = 0.0
    for step in ref.replay(X64, idx):
        if step[0] == m:
            break
        t, mind2 = step
        j = idx[t]
        assert mind2[j] >= 0.0                                   # (never a marked row)
        prefix = np.cumsum(np.where(mind2 > 0.0, mind2, 0.0))
        total = prefix[-1]
        if total > 0.0:
            target = ref.uniform01(seed, t) * total
            lo = prefix[j - 1] if j > 0 else 0.0
            slack = 2.0 * EPS(nf) * total
            worst = max(worst, (lo - target) / total, (target - prefix[j]) / total)
            assert lo - slack <= target <= prefix[j] + slack, (t, j, worst)
            assert mind2[j] > 0.0
    print("kmeans++ %d x %d, m = %d: the target left the chosen row's float64 interval by at most %.3g of the total "
          "(bound %.3g)" % (n, nf, m, max(worst, 0.0), 2.0 * EPS(nf)))
    _check_final_state(X64, got, nf)


def test_many_features_stage_the_landmark_in_chunks():
    """20 000 features: the landmark row passes through LDS in several chunks; integer data, so exact."""
    data = _integers(70, 20000, seed=3)
    for method in METHODS:
        want_idx, want_r2, want_near, _ = ref.select(data, 6, method, 2, seed=1)
        got = landmarks.select(data, 6, method=method, start=2, seed=1)
        assert got.indices.cpu().tolist() == want_idx.tolist()
        assert got.nearest.cpu().tolist() == want_near.tolist()
        assert torch.equal(got.radius, torch.as_tensor(want_r2.astype(np.float32)).to(DEV).sqrt())


# ---------------------------------------------------------------- duplicates
@pytest.mark.parametrize("method", METHODS)
def test_duplicates_give_distinct_rows(method):
    rng = np.random.default_rng(4)
    base = rng.standard_normal((5, 7)).astype(np.float32) * 3.0
    data = base[rng.permutation(np.repeat(np.arange(5), 8))]
    got = landmarks.select(data, 12, method=method, start=0, seed=2)
    idx = got.indices.cpu().numpy()
    assert len(set(idx.tolist())) == 12
    first = {tuple(data[i].tolist()) for i in idx[:5]}
    assert first == {tuple(b.tolist()) for b in base}
    radius = got.radius.cpu().numpy()
    assert np.all(radius[1:5] > 0.0) and np.all(radius[5:] == 0.0)
    assert np.all(got.distance.cpu().numpy() == 0.0)
    # a duplicate keeps the landmark that came first, and the smallest unselected row is taken when only
    # duplicates are left
    assert int(got.nearest.max()) < 5
    for t in range(5, 12):
        assert idx[t] == min(set(range(40)) - set(idx[:t].tolist()))


# ---------------------------------------------------------------- determinism
def _equal(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


def test_runs_seeds_and_start(real_data):
    data = real_data[(1037, 50)]
    for method in METHODS:
        a = landmarks.select(data, 64, method=method, seed=3)
        assert _equal(a, landmarks.select(data, 64, method=method, seed=3))
        assert int(a.indices[0]) == int(quality._sample_rows(1037, 1, 3)[0])
        b = landmarks.select(data, 64, method=method, seed=3, start=500)
        assert int(b.indices[0]) == 500 and int(b.nearest[500]) == 0
    k3 = landmarks.select(data, 64, method="kmeans++", seed=3, start=0)
    k4 = landmarks.select(data, 64, method="kmeans++", seed=4, start=0)
    assert k3.indices.tolist() != k4.indices.tolist()
    # the farthest point does not draw: from one start every seed gives the same list
    f3 = landmarks.select(data, 64, method="farthest", seed=3, start=0)
    assert _equal(f3, landmarks.select(data, 64, method="farthest", seed=4, start=0))
    assert _equal(k3, landmarks.select(torch.as_tensor(data).to(DEV), 64, method="kmeans++", seed=3, start=0))


@pytest.mark.parametrize("n,nf", [(5003, 16), (1037, 50), (300, 784)])
def test_results_do_not_depend_on_the_grid(monkeypatch, n, nf):
    data = ref.blobs_with_far_group(n, nf, seed=1)
    for method in METHODS:
        monkeypatch.delenv("MDE_LANDMARK_BLOCKS", raising=False)
        a = landmarks.select(data, 40, method=method, seed=9, start=1)
        for blocks in (1, 3, 7, 100000):
            monkeypatch.setenv("MDE_LANDMARK_BLOCKS", str(blocks))
            assert _equal(a, landmarks.select(data, 40, method=method, seed=9, start=1)), (method, blocks)


# ---------------------------------------------------------------- metrics, sparse input
@pytest.mark.parametrize("metric", ["cosine", "correlation"])
@pytest.mark.parametrize("method", METHODS)
def test_cosine_and_correlation_select_on_the_unit_rows(metric, method):
    rng = np.random.default_rng(8)
    data = (4.0 * rng.standard_normal((6, 30))[rng.integers(0, 6, 257)] + rng.standard_normal((257, 30)))
    data = torch.as_tensor((data - data.mean(0)).astype(np.float32)).to(DEV)
    unit = metrics.normalized_rows(data, metrics.resolve(metric))
    assert metrics.translated_rows(unit)[1] is None      # (centred data: the Euclidean path takes the unit rows as is)
    got = landmarks.select(data, 32, method=method, metric=metric, seed=6, start=3)
    euclid = landmarks.select(unit, 32, method=method, seed=6, start=3)
    assert torch.equal(got.indices, euclid.indices) and torch.equal(got.nearest, euclid.nearest)
    idx, radius2, mind2, nearest = landmarks._select_rows(unit, 32, method, 3, 6)
    assert torch.equal(got.distance, mind2 * 0.5) and torch.equal(got.radius, radius2 * 0.5)
    # and that is the metric's own distance 1 - cos to the named landmark
    cos = (unit.double() * unit.double()[got.indices[got.nearest]]).sum(1)
    assert float((got.distance.double() - (1.0 - cos)).abs().max()) <= 4.0 * EPS(30)


def test_sparse_input_equals_its_dense_copy():
    data = _integers(400, 24, seed=5)
    data[data < 2] = 0.0
    dense = torch.as_tensor(data)
    for method in METHODS:
        a = landmarks.select(dense, 20, method=method, seed=1, start=0)
        assert _equal(a, landmarks.select(dense.to_sparse(), 20, method=method, seed=1, start=0))
        assert _equal(a, landmarks.select(dense.to_sparse_csr(), 20, method=method, seed=1, start=0))


def test_rows_that_cannot_be_prepared_raise():
    data = ref.blobs_with_far_group(50, 4)
    bad = data.copy()
    bad[7, 2] = np.nan
    with pytest.raises(ValueError, match="row 7"):
        landmarks.select(bad, 5)
    zero = data.copy()
    zero[9] = 0.0
    with pytest.raises(ValueError):
        landmarks.select(zero, 5, metric="cosine")


def test_c_entry_refuses_bad_sizes():
    from pymde_amd import _lib
    lib = _lib.load()
    assert lib.mde_select_landmarks_work_bytes(10, 4, 11) == _lib.MDE_E_INVALID
    assert lib.mde_select_landmarks_work_bytes(10, 0, 2) == _lib.MDE_E_INVALID
    assert lib.mde_select_landmarks_work_bytes(2 ** 31, 4, 2) == _lib.MDE_E_TOO_LARGE
    assert lib.mde_select_landmarks_work_bytes(10, 4, 10) > 0
    rows = torch.zeros((10, 4), device=DEV)
    out_i, out_f = torch.zeros(10, dtype=torch.int32, device=DEV), torch.zeros(10, device=DEV)
    work = torch.zeros(4096, dtype=torch.uint8, device=DEV)
    for n, m, method, start in [(10, 11, 0, 0), (10, 0, 0, 0), (10, 3, 2, 0), (10, 3, 0, 10), (10, 3, 0, -1)]:
        rc = lib.mde_select_landmarks(n, 4, _lib.ptr(rows), m, method, start, 0, _lib.ptr(out_i), _lib.ptr(out_f),
                                      _lib.ptr(out_f), _lib.ptr(out_i), _lib.ptr(work), _lib.stream_ptr())
        assert rc == _lib.MDE_E_INVALID and "mde_select_landmarks" in _lib.last_error()


# ---------------------------------------------------------------- coverage
@pytest.mark.parametrize("n,nf,m", [(1037, 50, 64), (600, 30, 150)])
def test_farthest_covers_what_a_uniform_draw_misses(n, nf, m):
    data = ref.blobs_with_far_group(n, nf)
    for seed in range(5):
        got = landmarks.select(data, m, method="farthest", seed=seed)
        covering = float(got.distance.max())
        uniform = np.sqrt(ref.covering_radius2(data, quality._sample_rows(n, m, seed).numpy()))
        print("%d x %d, m = %d, seed %d: covering radius %.4g farthest, %.4g uniform" % (n, nf, m, seed, covering,
                                                                                         uniform))
        assert covering < uniform
        assert bool((got.indices < 5).any())
        assert covering <= float(got.radius[-1])       # (radius[t] is the covering radius of the first t landmarks)


# ---------------------------------------------------------------- end to end
def test_end_to_end():
    n, m = 600, 150
    data = ref.blobs_with_far_group(n, 30)
    start = torch.as_tensor(np.random.default_rng(1).standard_normal((n, 2)).astype(np.float32)).to(DEV)
    s_start = quality.stress(data, start, scale=1.0)
    stresses = {}
    for selection in ("uniform", "farthest", "kmeans++"):
        problem = pymde_amd.preserve_distances(data, landmarks=m, landmark_selection=selection, seed=0,
                                               loss=pymde_amd.losses.Quadratic)
        assert isinstance(problem, pymde_amd.LandmarkMDE) and problem.selection == selection
        X = problem.embed(X=start.clone(), eps=1e-5, max_iter=100)
        assert X.shape == (n, 2) and X.dtype == torch.float32 and X.is_cuda
        assert float(X.double().mean(0).abs().max()) <= 1e-5 * float(X.abs().max())
        assert problem.landmarks.dtype == torch.int64 and not problem.landmarks.is_cuda
        assert problem.landmarks.shape == (m,) and len(set(problem.landmarks.tolist())) == m
        if selection == "uniform":
            assert problem.landmark_radius is None
            assert torch.equal(problem.landmarks, quality._sample_rows(n, m, 0))
        else:
            chosen = landmarks.select(data, m, method=selection, seed=0)
            assert torch.equal(problem.landmarks, chosen.indices.cpu())
            assert isinstance(problem.landmark_radius, float)
            assert problem.landmark_radius == float(chosen.distance.max()) > 0.0
        stresses[selection] = quality.stress(data, X, scale=1.0)
        assert stresses[selection] < s_start
    print("stress at scale 1, 600 x 30, 150 landmarks: start %.6g, uniform %.6g, farthest %.6g, kmeans++ %.6g"
          % (s_start, stresses["uniform"], stresses["farthest"], stresses["kmeans++"]))
    # the keyword reaches LandmarkMDE directly as well
    direct = pymde_amd.LandmarkMDE(data, m, loss=pymde_amd.losses.Quadratic, seed=0, selection="k-means++")
    assert direct.selection == "kmeans++"
    assert torch.equal(direct.landmarks, landmarks.select(data, m, method="kmeans++", seed=0).indices.cpu())

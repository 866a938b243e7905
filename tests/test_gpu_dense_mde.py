"""pymde_amd.DenseMDE and preserve_distances(dense=True) on the GPU: the dense problem equals the edge-list problem
over all pairs (the edge-list path is the yardstick: its kernels are checked against the oracle elsewhere), from a
data matrix and from a distance matrix, and its embed() minimises what quality.stress measures.
Tolerances: LOSS_RTOL and assert_grad_close of tests/conftest.py."""
import numpy as np
import pytest
import torch

from conftest import GRAD_ATOL_REL, GRAD_RTOL, LOSS_RTOL, assert_grad_close

pytestmark = pytest.mark.gpu
DEV = "cuda"
N, NF = 150, 20


# ---------------------------------------------------------------- helpers
_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _data():
    def make():
        rng = np.random.default_rng(11)
        data = rng.standard_normal((N, NF)) * rng.uniform(0.5, 2.0, NF)
        X = rng.standard_normal((N, 2)) * 3.0
        return (data - data.mean(0)).astype(np.float32), (X - X.mean(0)).astype(np.float32)
    return _cached("data", make)


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


def _constraint(name):
    import pymde_amd
    return pymde_amd.Centered() if name == "Centered" else pymde_amd.Standardized()


# ---------------------------------------------------------------- 1. the edge-list problem over all pairs
@pytest.mark.parametrize("constraint", ["Centered", "Standardized"])
@pytest.mark.parametrize("loss", ["Absolute", "Quadratic", "WeightedQuadratic"])
def test_dense_equals_the_edge_list_problem(loss, constraint):
    import pymde_amd
    data, X = _data()
    L = getattr(pymde_amd.losses, loss)
    edge = pymde_amd.preserve_distances(data, max_distances=1e9, loss=L, constraint=_constraint(constraint))
    assert int(edge.p) == N * (N - 1) // 2
    dense = pymde_amd.preserve_distances(data, dense=True, loss=L, constraint=_constraint(constraint))
    assert isinstance(dense, pymde_amd.DenseMDE) and dense.p == N * (N - 1) // 2
    assert dense.n_items == N and dense.embedding_dim == 2 and dense.constraint.name() == constraint.lower()
    if constraint == "Standardized":
        assert dense.deviation_scale != 1.0                     # the rms rescaling is what this case checks
    else:
        assert dense.deviation_scale == 1.0
    _compare("%s %s" % (loss, constraint), _value_and_grad(dense, X), _value_and_grad(edge, X))


def test_cosine():
    import pymde_amd
    data, X = _data()
    data = data + 0.5
    X = X * 0.1                                                 # cosine distances lie in [0, 2]
    edge = pymde_amd.preserve_distances(data, max_distances=1e9, metric="cosine")
    dense = pymde_amd.preserve_distances(data, dense=True, metric="cosine")
    assert dense.metric == "cosine"
    _compare("cosine", _value_and_grad(dense, X), _value_and_grad(edge, X))


def test_distance_matrix_gives_the_result_of_data():
    import pymde_amd
    data, X = _data()
    d64 = data.astype(np.float64)
    D = np.sqrt(((d64[:, None, :] - d64[None, :, :]) ** 2).sum(-1))
    for loss in (pymde_amd.losses.Absolute, pymde_amd.losses.Quadratic):
        from_data = pymde_amd.DenseMDE(data, loss=loss)
        from_matrix = pymde_amd.DenseMDE(distance_matrix=D, loss=loss)
        assert from_matrix.n_items == N and from_matrix.metric is None
        _compare("distance_matrix %s" % loss.__name__, _value_and_grad(from_matrix, X), _value_and_grad(from_data, X))
    as_tensor = pymde_amd.DenseMDE(distance_matrix=torch.as_tensor(D).to(DEV), loss=pymde_amd.losses.Quadratic)
    assert _value_and_grad(as_tensor, X)[0] == _value_and_grad(from_matrix, X)[0]


def test_distance_matrix_is_checked_on_the_gpu():
    import pymde_amd
    D = np.abs(np.subtract.outer(np.arange(5.0), np.arange(5.0)))
    pymde_amd.DenseMDE(distance_matrix=D)
    for poison, word in ((np.nan, "finite"), (np.inf, "finite"), (-1.0, "non-negative")):
        bad = D.copy()
        bad[1, 3] = bad[3, 1] = poison
        with pytest.raises(ValueError, match=word):
            pymde_amd.DenseMDE(distance_matrix=bad)
    bad = D.copy()
    bad[1, 3] = 2.5
    with pytest.raises(ValueError, match="symmetric"):
        pymde_amd.DenseMDE(distance_matrix=bad)
    bad = D.copy()
    np.fill_diagonal(bad, np.nan)                               # the check reads the whole matrix (the kernel never
    with pytest.raises(ValueError, match="finite"):             # uses the diagonal)
        pymde_amd.DenseMDE(distance_matrix=bad)


def test_grad_output_scales_the_gradient():
    import pymde_amd
    data, X = _data()
    dense = pymde_amd.DenseMDE(data, loss=pymde_amd.losses.Quadratic)
    value, grad = _value_and_grad(dense, X)
    Xg = torch.as_tensor(X).to(DEV).requires_grad_(True)
    (3.0 * dense.average_distortion(Xg)).backward()
    assert np.array_equal(Xg.grad.cpu().numpy(), 3.0 * grad)
    # float64 embeddings are cast, and the gradient flows back through the cast
    X64 = torch.as_tensor(X, dtype=torch.float64).to(DEV).requires_grad_(True)
    v64 = dense.average_distortion(X64)
    v64.backward()
    assert float(v64) == value and X64.grad.dtype == torch.float64
    assert np.array_equal(X64.grad.cpu().numpy().astype(np.float32), grad)


def test_item_distortions():
    import pymde_amd
    data, X = _data()
    dense = pymde_amd.DenseMDE(data, loss=pymde_amd.losses.Absolute)
    value = float(dense.average_distortion(torch.as_tensor(X).to(DEV)))
    items = dense.item_distortions(torch.as_tensor(X))
    assert items.dtype == torch.float32 and items.is_cuda and items.shape == (N,)
    total, want = float(items.double().sum()), 2.0 * dense.p * value / (N - 1)
    print("item_distortions sum %.8g against %.8g (bound %.3g)" % (total, want, LOSS_RTOL))
    assert abs(total - want) <= LOSS_RTOL * want
    with pytest.raises(ValueError, match="embed"):
        dense.item_distortions()


# ---------------------------------------------------------------- 2. embed()
def test_embed_reaches_what_the_edge_list_problem_reaches():
    import pymde_amd
    from pymde_amd import quality
    rng = np.random.default_rng(12)
    data = rng.standard_normal((N, 2)) * np.array([3.0, 1.0])
    data = (data - data.mean(0)).astype(np.float32)
    start = data + (0.1 * data.std() * rng.standard_normal((N, 2))).astype(np.float32)
    start = torch.as_tensor(start - start.mean(0)).to(DEV)
    kwargs = dict(eps=1e-6, max_iter=200)
    edge = pymde_amd.preserve_distances(data, max_distances=1e9, loss=pymde_amd.losses.Quadratic,
                                        constraint=pymde_amd.Centered())
    dense = pymde_amd.preserve_distances(data, dense=True, loss=pymde_amd.losses.Quadratic,
                                         constraint=pymde_amd.Centered())
    initial = float(dense.average_distortion(start))
    stress_before = quality.stress(data, start, scale=1.0)
    edge.embed(X=start.clone(), **kwargs)
    assert dense.X is None and dense.solve_stats is None and dense.value is None and dense.residual_norm is None
    X = dense.embed(X=start.clone(), **kwargs)
    print("initial value %.6g; final value dense %.6g in %d iterations, edge list %.6g in %d iterations"
          % (initial, dense.value, dense.solve_stats.iterations, edge.value, edge.solve_stats.iterations))
    assert X is dense.X and X.shape == (N, 2) and X.is_cuda and X.dtype == torch.float32
    assert dense.solve_stats is not None and dense.solve_stats.iterations > 0
    assert dense.value is not None and dense.residual_norm is not None
    assert dense.value <= 1.05 * edge.value + 1e-6 * initial
    stress_after = quality.stress(data, X, scale=1.0)
    print("stress at scale 1: %.6g before, %.6g after" % (stress_before, stress_after))
    assert stress_after < stress_before
    assert abs(float(dense.average_distortion()) - dense.value) <= 1e-4 * initial     # X=None: the stored embedding


# ---------------------------------------------------------------- 3. config 1 in small
def test_cycle_graph_through_a_distance_matrix():
    """All-pairs shortest paths of a 300-node cycle as a distance_matrix, against the graph recipe's edge-list problem
    over the same pairs.  The graph recipe's deviations are integers, so they are exact."""
    import pymde_amd
    n = 300
    idx = np.arange(n)
    gap = np.abs(idx[:, None] - idx[None, :])
    D = np.minimum(gap, n - gap).astype(np.float64)
    cycle = torch.as_tensor(np.stack([idx, (idx + 1) % n], 1))
    rng = np.random.default_rng(13)
    X = (40.0 * rng.standard_normal((n, 2))).astype(np.float32)
    for loss in (pymde_amd.losses.Absolute, pymde_amd.losses.Quadratic):
        edge = pymde_amd.preserve_distances(pymde_amd.Graph.from_edges(cycle), max_distances=1e9, loss=loss)
        assert int(edge.p) == n * (n - 1) // 2
        # joined by the sorted edge list: the edge-list problem holds the entries of D
        e = edge.edges.cpu().numpy()
        order = np.lexsort((e[:, 1], e[:, 0]))
        iu, ju = np.triu_indices(n, 1)
        assert np.array_equal(e[order], np.stack([iu, ju], 1))
        assert np.array_equal(edge.distortion_function.deviations.cpu().numpy()[order], D[iu, ju].astype(np.float32))
        dense = pymde_amd.DenseMDE(distance_matrix=D, loss=loss)
        _compare("cycle %s" % loss.__name__, _value_and_grad(dense, X), _value_and_grad(edge, X))

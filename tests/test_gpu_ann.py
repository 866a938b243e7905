"""Approximate k-NN by the inverted-file search (csrc/mde_ann.hip, pymde_amd/ann.py): full probing equals
the exact kernel bit for bit, recall on clustered data at the defaults, determinism, the small-input and
max_distance contracts, adverse shapes, input forms, the recipes and the C entries' argument checks."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _mixture(n, nf, classes=10, seed=0):
    """Classes with means ~ N(0, 9 I), each a random 10-12 dimensional linear patch, plus N(0, 0.25 I) noise."""
    g = torch.Generator(device=DEV)
    g.manual_seed(seed)
    labels = torch.randint(0, classes, (n,), generator=g, device=DEV)
    means = 3.0 * torch.randn(classes, nf, generator=g, device=DEV)
    X = means[labels] + 0.5 * torch.randn(n, nf, generator=g, device=DEV)
    for c in range(classes):
        dim = 10 + c % 3
        basis = torch.randn(dim, nf, generator=g, device=DEV)
        rows = (labels == c).nonzero()[:, 0]
        X[rows] += torch.randn(rows.shape[0], dim, generator=g, device=DEV) @ basis
    return X.contiguous(), labels


def _uniform(n, nf, seed=0):
    g = torch.Generator(device=DEV)
    g.manual_seed(seed)
    return torch.rand(n, nf, generator=g, device=DEV)


def _knn(data, k, **kw):
    from pymde_amd import preprocess
    e, w = preprocess.k_nearest_neighbors(data, k, **kw)
    return e.cpu().numpy(), w.cpu().numpy()


def _ann_lists(X, k, **kw):
    from pymde_amd import ann
    with torch.cuda.device(X.device):
        return ann.knn_lists(X, k, **kw)


def _check_lists(X, idx, d2, rows=None, rtol=1e-5):
    """Every listed (id, d2) is real against float64, no row lists itself or a neighbour twice, -1 slots
    only at the end of a row."""
    n, k = idx.shape
    rows = torch.arange(n, device=X.device) if rows is None else rows
    Xd = X.double()
    for s in range(0, rows.shape[0], 2048):
        r = rows[s:s + 2048]
        ii, dd = idx[r].long(), d2[r].double()
        valid = ii >= 0
        assert bool((valid[:, 1:] <= valid[:, :-1]).all())           # -1 slots trail
        assert not bool((ii == r[:, None]).any())
        srt = torch.sort(torch.where(valid, ii, -1 - torch.arange(k, device=X.device)), 1).values
        assert not bool((srt[:, 1:] == srt[:, :-1]).any())           # no neighbour twice
        true = (Xd[r][:, None, :] - Xd[ii.clamp(min=0)]).pow(2).sum(2)
        scale = Xd[r].pow(2).sum(1, keepdim=True) + Xd[ii.clamp(min=0)].pow(2).sum(2)
        err = (dd - true).abs()
        # |x|^2 + |y|^2 - 2 x.y in f32: rounding relative to the norms, beside the rtol on d2 itself
        assert bool(((err <= rtol * true + 2e-6 * scale) | ~valid).all()), float(err[valid].max())
        assert bool((dd[:, 1:] >= dd[:, :-1])[valid[:, 1:]].all())


# ---------------------------------------------------------------- 1. full probing is the exact search
@pytest.mark.parametrize("nf", [1, 3, 50, 784])
def test_full_probe_equals_exact(nf):
    from pymde_amd import preprocess
    n = 20000 + 37
    X = _uniform(n, nf, seed=nf)
    for k in (1, 15, 64):
        e, w = _knn(X, k)
        ea, wa = _knn(X, k, approximate=True, n_probe=10 ** 6)
        np.testing.assert_array_equal(ea, e)
        np.testing.assert_array_equal(wa, w)
        idx, d2 = preprocess._dense_knn_lists(X, k)
        idx_a, d2_a = _ann_lists(X, k, n_probe=10 ** 6)
        assert torch.equal(d2_a, d2)
        assert torch.equal(idx_a, idx)


# ---------------------------------------------------------------- 2. recall on clustered data, defaults
@pytest.mark.parametrize("nf", [64, 784])
def test_recall_at_defaults_on_mixture(nf):
    from pymde_amd import preprocess
    n, k = 200000, 15
    X, _ = _mixture(n, nf, seed=nf)
    truth, _ = preprocess._dense_knn_lists(X, k)
    idx, d2 = _ann_lists(X, k)
    hit = (truth[:, :, None] == idx[:, None, :]).any(2)
    recall = float(hit.float().mean())
    assert recall >= 0.95, recall
    est = preprocess._estimated_recall(X, idx, k)
    assert abs(est - recall) < 0.03, (est, recall)
    assert bool((idx >= 0).all())
    g = torch.Generator(device=DEV)
    g.manual_seed(1)
    _check_lists(X, idx, d2, rows=torch.randperm(n, generator=g, device=DEV)[:20000])


# ---------------------------------------------------------------- 3. determinism
def test_same_seed_same_graph():
    X, _ = _mixture(60000, 32, seed=3)
    e1, w1 = _knn(X, 15, approximate=True, n_probe=4, seed=7)
    e2, w2 = _knn(X, 15, approximate=True, n_probe=4, seed=7)
    np.testing.assert_array_equal(e1, e2)
    np.testing.assert_array_equal(w1, w2)
    i1, d1 = _ann_lists(X, 15, n_probe=4, seed=7)
    i2, d2 = _ann_lists(X, 15, n_probe=4, seed=7)
    assert torch.equal(i1, i2) and torch.equal(d1, d2)


# ---------------------------------------------------------------- 4. small inputs take the exact kernel
def test_small_input_is_exact():
    X, _ = _mixture(5000, 20, seed=4)
    e, w = _knn(X, 15)
    ea, wa = _knn(X, 15, approximate=True, n_probe=1)
    np.testing.assert_array_equal(ea, e)
    np.testing.assert_array_equal(wa, w)


# ---------------------------------------------------------------- 5. max_distance
def test_max_distance():
    from pymde_amd import preprocess
    X, _ = _mixture(30000, 48, seed=5)
    idx, d2 = _ann_lists(X, 10)
    md = float(d2[:, 4].median().sqrt())
    e, w = preprocess.k_nearest_neighbors(X, 10, max_distance=md, approximate=True)
    full, _ = preprocess.k_nearest_neighbors(X, 10, approximate=True)
    assert 0 < e.shape[0] < full.shape[0]
    Xd = X.double()
    length = (Xd[e[:, 0]] - Xd[e[:, 1]]).norm(dim=1)
    # the cut is taken on the f32 squared distances, as on the exact path: rounding is the only slack
    assert float(length.max()) <= md * (1 + 1e-4), (float(length.max()), md)


# ---------------------------------------------------------------- 6. adverse shapes
def _valid_graph(e, w, n):
    assert e.ndim == 2 and e.shape[1] == 2
    assert (e[:, 0] < e[:, 1]).all() and (e >= 0).all() and (e < n).all()
    assert set(np.unique(w).tolist()) <= {1.0, 2.0}


def test_adverse_one_giant_list():
    X = _uniform(20000, 16, seed=6)
    X[:6000] = X[6000]                                   # 30 % of the rows identical (with row 6000)
    idx, d2 = _ann_lists(X, 15)
    _check_lists(X, idx, d2)
    dup = idx[:6001]
    assert bool((dup >= 0).all())
    e, w = _knn(X, 15, approximate=True)
    _valid_graph(e, w, 20000)


def test_adverse_all_rows_identical():
    X = torch.full((12000, 8), 0.25, device=DEV)
    idx, d2 = _ann_lists(X, 15)
    assert bool((idx >= 0).all()) and bool((idx != torch.arange(12000, device=DEV)[:, None]).all())
    assert float(d2.max()) <= 1e-5
    e, w = _knn(X, 15, approximate=True)
    _valid_graph(e, w, 12000)


def test_adverse_tiny_lists_leave_empty_slots():
    n = 10000
    X = _uniform(n, 6, seed=8)
    idx, d2 = _ann_lists(X, 15, n_lists=n // 2, n_probe=1)
    assert bool((idx < 0).any())
    _check_lists(X, idx, d2)
    e, w = _knn(X, 15, approximate=True, n_lists=n // 2, n_probe=1)
    _valid_graph(e, w, n)


def test_adverse_one_feature():
    X = _uniform(20000, 1, seed=9)
    idx, d2 = _ann_lists(X, 15)
    _check_lists(X, idx, d2, rtol=1e-4)
    e, w = _knn(X, 15, approximate=True)
    _valid_graph(e, w, 20000)


# ---------------------------------------------------------------- 7. inputs
def test_sparse_input_equals_dense_copy():
    A = sp.random(12000, 300, density=0.1, format="csr", random_state=10, dtype=np.float32)
    e, w = _knn(A, 12, approximate=True, n_probe=4)
    ed, wd = _knn(torch.tensor(A.toarray(), device=DEV), 12, approximate=True, n_probe=4)
    np.testing.assert_array_equal(e, ed)
    np.testing.assert_array_equal(w, wd)


def test_invalid_inputs():
    import pymde_amd
    from pymde_amd import _lib, preprocess
    X = _uniform(12000, 4, seed=11)
    g = pymde_amd.Graph(sp.csr_matrix(np.array([[0, 1, 0], [1, 0, 1], [0, 1, 0]], dtype=np.float32)))
    with pytest.raises(ValueError):
        preprocess.k_nearest_neighbors(g, 1, approximate=True)
    for kw in ({"n_probe": 0}, {"n_lists": 0}, {"n_lists": -1}):
        with pytest.raises(ValueError):
            preprocess.k_nearest_neighbors(X, 5, approximate=True, **kw)
        with pytest.raises(ValueError):
            preprocess.k_nearest_neighbors(X[:100], 5, approximate=True, **kw)
    with pytest.raises(_lib.MdeHipError):
        preprocess.k_nearest_neighbors(X, 65)
    with pytest.raises(_lib.MdeHipError):
        preprocess.k_nearest_neighbors(X, 65, approximate=True)
    with pytest.raises(ValueError):
        pymde_amd.preserve_neighbors(g, approximate_neighbors=True)


# ---------------------------------------------------------------- 8. recipes
def test_preserve_neighbors_approximate():
    import pymde_amd
    n, classes = 30000, 10
    X, labels = _mixture(n, 32, classes=classes, seed=12)
    labels = labels.cpu().numpy()
    torch.manual_seed(0)
    mde = pymde_amd.preserve_neighbors(X, embedding_dim=2, constraint=pymde_amd.Standardized(), seed=0,
                                       approximate_neighbors=True)
    assert set(np.unique(mde.distortion_function.weights.cpu().numpy()).tolist()) <= {-1.0, 1.0, 2.0}
    Z = mde.embed(max_iter=100).cpu().numpy()
    np.testing.assert_allclose(Z.T @ Z / n, np.eye(2), atol=1e-3)
    cent = np.stack([Z[labels == c].mean(0) for c in range(classes)])
    within = np.mean([np.linalg.norm(Z[labels == c] - cent[c], axis=1).mean() for c in range(classes)])
    between = np.linalg.norm(cent[:, None] - cent[None], axis=2)[np.triu_indices(classes, 1)].mean()
    assert between > 3 * within, (between, within)
    lap = pymde_amd.laplacian_embedding(X, approximate_neighbors={"n_lists": 100, "n_probe": 8})
    assert lap.edges.shape[0] > 0


def test_recipe_keyword_off_is_unchanged():
    import pymde_amd
    X, _ = _mixture(15000, 16, seed=13)
    torch.manual_seed(0)
    a = pymde_amd.preserve_neighbors(X, seed=0)
    torch.manual_seed(0)
    b = pymde_amd.preserve_neighbors(X, seed=0, approximate_neighbors=False)
    assert torch.equal(a.edges, b.edges)
    assert torch.equal(a.distortion_function.weights, b.distortion_function.weights)
    assert type(a.constraint) is type(b.constraint) and a.n_items == b.n_items


# ---------------------------------------------------------------- 9. the C entries' argument checks
def _scan_args(**over):
    """A valid mde_ann_search call on 100 rows (two lists of 40 / 60), with some arguments replaced."""
    from pymde_amd import _lib
    n, nf = 100, 5
    X = torch.rand(n, nf, device=DEV)
    sqn = X.pow(2).sum(1).contiguous()
    a = dict(nf=nf, k=3, flags=3, n_q=n, Q=X, q_sqn=sqn, n_qpos=n,
             q_map=torch.arange(n, dtype=torch.int32, device=DEV), n_b=n, B=X, b_sqn=sqn, n_bpos=n,
             b_map=torch.arange(n, dtype=torch.int32, device=DEV), n_lists=2,
             offsets=torch.tensor([0, 40, 100], dtype=torch.int64, device=DEV), n_probe=2,
             probe=torch.tensor([[0, 1], [1, 0]], dtype=torch.int32, device=DEV), n_tiles=2,
             tiles=torch.tensor([[0, 40, 0], [40, 100, 1]], dtype=torch.int64, device=DEV),
             idx=torch.full((n, 3), -7, dtype=torch.int32, device=DEV),
             d2=torch.full((n, 3), -7.0, device=DEV))
    a.update(over)
    p = lambda t: _lib.ptr(t) if isinstance(t, torch.Tensor) else t
    args = [a["nf"], a["k"], a["flags"], a["n_q"], p(a["Q"]), p(a["q_sqn"]), a["n_qpos"], p(a["q_map"]), a["n_b"],
            p(a["B"]), p(a["b_sqn"]), a["n_bpos"], p(a["b_map"]), a["n_lists"], p(a["offsets"]), a["n_probe"],
            p(a["probe"]), a["n_tiles"], p(a["tiles"]), p(a["idx"]), p(a["d2"]), _lib.stream_ptr()]
    return args, a


def test_c_entries_reject_invalid_arguments():
    from pymde_amd import _lib
    lib = _lib.load()
    args, a = _scan_args()
    assert lib.mde_ann_search(*args) == _lib.MDE_OK
    torch.cuda.synchronize()
    assert bool((a["idx"] >= 0).all())
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=DEV)
    i64 = lambda v: torch.tensor(v, dtype=torch.int64, device=DEV)
    bad = {
        "null Q": {"Q": None}, "null sqn": {"b_sqn": None}, "null offsets": {"offsets": None},
        "null probe": {"probe": None}, "null tiles": {"tiles": None}, "null idx": {"idx": None},
        "null d2": {"d2": None}, "k = 0": {"k": 0}, "k = 65": {"k": 65}, "nf = 0": {"nf": 0},
        "unknown flag": {"flags": 4},
        "offsets decrease": {"offsets": i64([0, 60, 40])},
        "offsets past the positions": {"offsets": i64([0, 40, 101])},
        "negative offset": {"offsets": i64([-1, 40, 100])},
        "probe id past n_lists": {"probe": i32([[0, 2], [1, 0]])},
        "negative probe id": {"probe": i32([[0, -1], [1, 0]])},
        "tile of 65 rows": {"tiles": i64([[0, 65, 0]]), "n_tiles": 1},
        "empty tile": {"tiles": i64([[5, 5, 0]]), "n_tiles": 1},
        "tile past the positions": {"tiles": i64([[90, 101, 0]]), "n_tiles": 1},
        "tile list past n_lists": {"tiles": i64([[0, 10, 2]]), "n_tiles": 1},
        "query map out of range": {"q_map": i32(list(range(99)) + [100])},
        "base map negative": {"b_map": i32([-1] + list(range(1, 100)))},
        "positions beyond rows without a map": {"q_map": None, "n_qpos": 101},
    }
    for what, over in bad.items():
        args, a = _scan_args(**over)
        rc = lib.mde_ann_search(*args)
        torch.cuda.synchronize()
        assert rc == _lib.MDE_E_INVALID, what
        for out in (a["idx"], a["d2"]):
            if out is not None:
                assert bool((out == -7).all()), what                   # nothing launched
    X = torch.rand(50, 4, device=DEV)
    cent = torch.full((3, 4), -7.0, device=DEV)
    members = torch.arange(50, dtype=torch.int32, device=DEV)
    ok = lib.mde_ann_centroids(50, 4, _lib.ptr(X), 50, _lib.ptr(members), 3, _lib.ptr(i64([0, 10, 10, 50])),
                               _lib.ptr(cent), _lib.stream_ptr())
    torch.cuda.synchronize()
    assert ok == _lib.MDE_OK
    torch.testing.assert_close(cent[0], X[:10].mean(0))
    assert bool((cent[1] == -7.0).all())                                # an empty list keeps its centroid
    for what, (mem, off) in {"member out of range": (i32([0] * 49 + [50]), i64([0, 10, 10, 50])),
                             "offsets decrease": (members, i64([0, 20, 10, 50])),
                             "offsets past the members": (members, i64([0, 10, 10, 51]))}.items():
        cent.fill_(-7.0)
        rc = lib.mde_ann_centroids(50, 4, _lib.ptr(X), 50, _lib.ptr(mem), 3, _lib.ptr(off), _lib.ptr(cent),
                                   _lib.stream_ptr())
        torch.cuda.synchronize()
        assert rc == _lib.MDE_E_INVALID, what
        assert bool((cent == -7.0).all()), what
    assert lib.mde_ann_centroids(50, 4, None, 50, _lib.ptr(members), 3, _lib.ptr(i64([0, 10, 10, 50])),
                                 _lib.ptr(cent), _lib.stream_ptr()) == _lib.MDE_E_INVALID

"""The bfloat16-shortlist k-NN search (``mde_knn_bf16``, ``precision="bfloat16"``) on the GPU.

Where test_knn_bf16_host.py's emulation shows that the shortlist keeps every true neighbour with 8 places to
spare, the result must be the float32 search's: the same ids and the same d2 bits.  Elsewhere (k = 64, one
feature, tiny corpora) the lists must be valid: ascending, no self, no duplicate, and every d2 the float32
distance of its pair.

The shortlist kernel's tile is 128 query rows x 128 candidates, parked in halves of 64; its feature chunk is 32
bfloat16 (two K steps of 16 of the MFMA): the geometry cases sit on both sides of each."""
import numpy as np
import pytest
import torch
from scipy.spatial.distance import cdist

import _knn_bf16_cases as cases
from pymde_amd import preprocess, recipes

pytestmark = pytest.mark.gpu
DEV = "cuda"
TILE, KSTEP = 128, 16
RTOL, STOL = 1e-5, 2e-6      # the float32 tolerance of tests/test_gpu_euclidean_accuracy.py


def _dev(X):
    return torch.tensor(np.asarray(X), device=DEV)


def _bits(d2):
    return d2.contiguous().view(torch.int32)


def _self_lists(X, k, n_candidates=None, slices=0):
    """(float32 lists, bfloat16 lists) of the self-join of X on the rows the float32 search runs on."""
    rows, mu, _ = preprocess._bf16_rows(_dev(X))
    k = min(k, rows.shape[0] - 1)
    return (preprocess._dense_knn_lists(rows, k),
            preprocess._dense_knn_lists_bf16(rows, k, n_candidates, mu, slices))


def _cross_lists(Q, C, k, n_candidates=None, slices=0):
    C_rows, mu, shift = preprocess._bf16_rows(_dev(C))
    Q_rows = _dev(Q) if shift is None else preprocess._metrics.subtract_columns(_dev(Q), shift)
    return (preprocess._cross_knn_lists(Q_rows, C_rows, k),
            preprocess._cross_knn_lists_bf16(Q_rows, C_rows, k, n_candidates, mu, slices))


def _assert_same(f32, bf16, label):
    assert torch.equal(bf16[0], f32[0]), label
    assert torch.equal(_bits(bf16[1]), _bits(f32[1])), label


def _assert_valid(idx, d2, Q, C, self_join, label):
    """Rows ascend by (d2, index), no id twice, no self, empty slots (-1 / FLT_MAX) only at the end and only
    when the corpus runs out; every d2 within the float32 tolerance (1e-5 of d2 + 2e-6 of the two squared norms the
    kernel saw) of the float64 distance of its pair."""
    n_q, k = idx.shape
    n_c = C.shape[0]
    idx, d2 = idx.cpu().numpy().astype(np.int64), d2.cpu().numpy().astype(np.float64)
    full = min(k, n_c - (1 if self_join else 0))
    assert (idx[:, :full] >= 0).all() and (idx[:, :full] < n_c).all(), label
    assert (idx[:, full:] == -1).all() and (d2[:, full:] == np.finfo(np.float32).max).all(), label
    if self_join:
        assert not (idx == np.arange(n_q)[:, None]).any(), label
    if full == 0:
        return
    srt = np.sort(idx[:, :full], 1)
    assert not (srt[:, 1:] == srt[:, :-1]).any(), label
    d, i = d2[:, :full], idx[:, :full]
    assert ((d[:, 1:] > d[:, :-1]) | ((d[:, 1:] == d[:, :-1]) & (i[:, 1:] > i[:, :-1]))).all(), label
    # the float32 error is relative to the norms of the rows the kernel searched: minus the grid means of the
    # corpus where metrics.translation_pays, as given otherwise (tests/test_gpu_cross_knn.py's scale)
    Q64, C64 = np.asarray(Q, dtype=np.float64), np.asarray(C, dtype=np.float64)
    mean, var = torch.tensor(C64.mean(0)), torch.tensor(C64.var(0))
    shift = preprocess._metrics.grid_means(mean, var).numpy() if preprocess._metrics.translation_pays(mean, var) else 0.0
    true = np.take_along_axis(cdist(Q64, C64, "sqeuclidean"), i, 1)
    scale = ((Q64 - shift) ** 2).sum(1)[:, None] + ((C64 - shift) ** 2).sum(1)[i]
    assert (np.abs(d - true) <= RTOL * true + STOL * scale).all(), label


# ---------------------------------------------------------------- 1. the float32 result where the shortlist suffices
@pytest.mark.parametrize("kind", cases.GENERATORS)
@pytest.mark.parametrize("n, nf, k", cases.SELF_SHAPES)
def test_self_join_equals_float32(kind, n, nf, k):
    X = cases.make(kind, n, nf)
    f32, bf16 = _self_lists(X, k)
    _assert_same(f32, bf16, (kind, n, nf, k))
    e, w = preprocess.k_nearest_neighbors(_dev(X), k)
    eb, wb = preprocess.k_nearest_neighbors(_dev(X), k, precision="bfloat16")
    assert torch.equal(eb, e) and torch.equal(wb, w)


@pytest.mark.parametrize("n_q, n_c, nf, k", cases.CROSS_SHAPES)
def test_cross_search_equals_float32(n_q, n_c, nf, k):
    Q, C = cases.cross_pair("mixture", n_q, n_c, nf)
    f32, bf16 = _cross_lists(Q, C, k)
    _assert_same(f32, bf16, (n_q, n_c, nf, k))
    idx, dist = preprocess.cross_nearest_neighbors(_dev(Q), _dev(C), k)
    idx_b, dist_b = preprocess.cross_nearest_neighbors(_dev(Q), _dev(C), k, precision="bf16")
    assert torch.equal(idx_b, idx) and torch.equal(_bits(dist_b), _bits(dist))


# ---------------------------------------------------------------- 2. k = 64: no margin
def test_k64_recall_and_validity():
    X = cases.make("gauss", 1500, 100)
    (idx, d2), (idx_b, d2_b) = _self_lists(X, 64, n_candidates=64)
    hit = (idx_b[:, :, None] == idx[:, None, :])                  # [n, 64 bf16, 64 f32]
    recall = float(hit.any(2).float().mean())
    print("k = 64, n_candidates = 64 on gauss 1500 x 100: recall %.4f" % recall)
    assert recall >= 0.99
    where = hit.nonzero()
    assert torch.equal(_bits(d2_b)[where[:, 0], where[:, 1]], _bits(d2)[where[:, 0], where[:, 2]])
    _assert_valid(idx_b, d2_b, X, X, True, "k64")


# ---------------------------------------------------------------- 3. geometry edges of the 128 x 128 tile
EDGE_N = (1, TILE - 1, TILE, TILE + 1, 2 * TILE + 1)
EDGE_NF = (1, 7, KSTEP - 1, KSTEP + 1, 31, 33, 784)


def _edge_case(n_q, n_c, nf, k, self_join):
    if self_join:
        X = cases.make("mixture", n_c, nf)
        Q = C = X
        f32, bf16 = _self_lists(X, k)
    else:
        Q, C = cases.cross_pair("mixture", n_q, n_c, nf)
        f32, bf16 = _cross_lists(Q, C, k)
    label = (n_q, n_c, nf, k, self_join)
    _assert_valid(bf16[0], bf16[1], Q, C, self_join, label)
    if cases.shortlist_is_safe(Q, C, k, self_join):
        _assert_same(f32, bf16, label)
    return f32, bf16


@pytest.mark.parametrize("n_q", EDGE_N)
def test_cross_tile_edges(n_q):
    for n_c in EDGE_N:          # n_c = 1 < k: 14 empty slots
        _edge_case(n_q, n_c, 7, 15, False)


@pytest.mark.parametrize("n", (2, 10) + EDGE_N[1:])
def test_self_join_tile_edges(n):
    _edge_case(n, n, 7, 15, True)      # n = 2, 10: fewer than k other rows


@pytest.mark.parametrize("nf", EDGE_NF)
def test_feature_edges(nf):
    _edge_case(TILE + 1, 2 * TILE + 1, nf, 15, False)
    _edge_case(2 * TILE + 1, 2 * TILE + 1, nf, 15, True)


def test_short_corpus_leaves_empty_slots():
    Q, C = cases.cross_pair("gauss", 70, 9, 20)
    f32, bf16 = _cross_lists(Q, C, 15)
    _assert_same(f32, bf16, "9 rows")
    assert bool((bf16[0][:, 9:] == -1).all()) and bool((bf16[0][:, :9] >= 0).all())
    idx, dist = preprocess.cross_nearest_neighbors(_dev(Q), _dev(C), 15, precision="bfloat16")
    assert bool((idx[:, 9:] == -1).all()) and bool(torch.isinf(dist[:, 9:]).all())


# ---------------------------------------------------------------- 4. the corpus split
@pytest.mark.parametrize("n_q, n_c, nf", [(65, 1037, 50), (70, 20000, 50)])
def test_result_does_not_depend_on_the_split(n_q, n_c, nf):
    Q, C = cases.cross_pair("mixture", n_q, n_c, nf)
    ref = _cross_lists(Q, C, 15, slices=1)[1]
    for slices in (1, 3, 7, 0):
        got = _cross_lists(Q, C, 15, slices=slices)[1]
        assert torch.equal(got[0], ref[0]) and torch.equal(_bits(got[1]), _bits(ref[1])), slices
    # the shortlist itself (n_candidates = k: the re-rank only reorders it) is the same for every split
    short = [_cross_lists(Q, C, 31, n_candidates=31, slices=s)[1] for s in (1, 3, 7, 0, 0)]
    for got in short[1:]:
        assert torch.equal(got[0], short[0][0]) and torch.equal(_bits(got[1]), _bits(short[0][1]))


# ---------------------------------------------------------------- 5. metrics and recipes
@pytest.mark.parametrize("metric", ["cosine", "correlation"])
def test_cosine_and_correlation_equal_float32(metric):
    X = _dev(cases.make("mixture", 1037, 50))
    i32, v32, _ = preprocess._metric_knn_lists(X, 15, metric)
    ib, vb, _ = preprocess._metric_knn_lists(X, 15, metric, precision="bfloat16")
    assert torch.equal(ib, i32) and torch.equal(_bits(vb), _bits(v32))
    e, w = preprocess.k_nearest_neighbors(X, 15, metric=metric)
    eb, wb = preprocess.k_nearest_neighbors(X, 15, metric=metric, precision="bfloat16")
    assert torch.equal(eb, e) and torch.equal(wb, w)


def test_max_distance_is_honoured():
    X = _dev(cases.make("mixture", 1037, 50))
    _, d2 = preprocess._dense_knn_lists(X, 15)
    radius = float(d2[:, 7].median().sqrt())          # cuts the lists of about half the rows
    e, w = preprocess.k_nearest_neighbors(X, 15, max_distance=radius)
    eb, wb = preprocess.k_nearest_neighbors(X, 15, max_distance=radius, precision="bfloat16")
    full = preprocess.k_nearest_neighbors(X, 15, precision="bfloat16")[0]
    assert 0 < e.shape[0] < full.shape[0]
    assert torch.equal(eb, e) and torch.equal(wb, w)


def test_recipes_build_the_same_edges():
    X = cases.make("mixture", 1037, 50)
    a = recipes.preserve_neighbors(_dev(X), n_neighbors=15, init="random", seed=3)
    b = recipes.preserve_neighbors(_dev(X), n_neighbors=15, init="random", seed=3, neighbor_precision="bfloat16")
    assert torch.equal(a.edges, b.edges)
    lap_a = recipes.laplacian_embedding(_dev(X), n_neighbors=15, init="random")
    lap_b = recipes.laplacian_embedding(_dev(X), n_neighbors=15, init="random", neighbor_precision="bf16")
    assert torch.equal(lap_a.edges, lap_b.edges)
    new, old = cases.cross_pair("mixture", 65, 1037, 50)
    emb = torch.randn(1037, 2, generator=torch.Generator().manual_seed(0))
    c = recipes.extend_embedding(_dev(old), emb, _dev(new), n_neighbors=15, seed=5)
    d = recipes.extend_embedding(_dev(old), emb, _dev(new), n_neighbors=15, seed=5, neighbor_precision="bfloat16")
    assert torch.equal(c.edges, d.edges)


def test_sparse_input_is_densified_and_served():
    import scipy.sparse as sp
    X = cases.make("ints", 1037, 50) * (cases.make("uniform", 1037, 50) < 0.3)
    A = sp.csr_matrix(X)
    e, w = preprocess.k_nearest_neighbors(A, 15, device=DEV)
    eb, wb = preprocess.k_nearest_neighbors(A, 15, device=DEV, precision="bfloat16")
    assert torch.equal(eb, e) and torch.equal(wb, w)


def test_sparse_input_that_stays_sparse_is_refused(monkeypatch):
    import scipy.sparse as sp
    A = sp.csr_matrix(cases.make("ints", 130, 3) + 1)      # no all-zero row: cosine is defined for every row
    monkeypatch.setattr(preprocess, "_densify_sparse_knn", lambda *a: False)
    for metric in ("euclidean", "cosine"):
        with pytest.raises(ValueError, match="does not fit"):
            preprocess.k_nearest_neighbors(A, 5, device=DEV, metric=metric, precision="bfloat16")


def test_c_abi_argument_errors():
    from pymde_amd import _lib
    lib = _lib.load()
    assert lib.mde_knn_bf16_work_bytes(10, 10, 4, 5, 4, 0) == _lib.MDE_E_INVALID        # n_cand < k
    assert lib.mde_knn_bf16_work_bytes(10, 10, 4, 5, 65, 0) == _lib.MDE_E_INVALID       # n_cand > 64
    assert "1 <= k <= n_cand <= 64" in _lib.last_error()
    assert lib.mde_knn_bf16_work_bytes(10, 10, 4, 5, 21, 1) > 0

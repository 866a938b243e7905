"""The neighbour-of-neighbour pass on the GPU (csrc/mde_ann_refine.hip, pymde_amd.ann.refine_lists): equal to
the numpy restatement bit for bit, exact lists a fixed point, entries only move earlier and recall rises at
scale, the public path, and the C entries' argument checks."""
import numpy as np
import pytest
import torch

import _ann_refine_reference as ref

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _mixture(n, nf, classes=10, seed=0):
    """The mixture of tests/test_gpu_ann.py: class means ~ N(0, 9 I), a 10-12 dimensional linear patch each."""
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
    return X.contiguous()


def _check_lists(X, idx, d2, rtol=1e-5):
    """Every listed (id, d2) is real against float64, no row lists itself or a neighbour twice, -1 slots only
    at the end of a row, distances ascending (the rule of test_gpu_ann._check_lists)."""
    n, k = idx.shape
    Xd = X.double()
    for s in range(0, n, 2048):
        r = torch.arange(s, min(n, s + 2048), device=X.device)
        ii, dd = idx[r].long(), d2[r].double()
        valid = ii >= 0
        assert bool((valid[:, 1:] <= valid[:, :-1]).all())
        assert not bool((ii == r[:, None]).any())
        srt = torch.sort(torch.where(valid, ii, -1 - torch.arange(k, device=X.device)), 1).values
        assert not bool((srt[:, 1:] == srt[:, :-1]).any())
        true = (Xd[r][:, None, :] - Xd[ii.clamp(min=0)]).pow(2).sum(2)
        scale = Xd[r].pow(2).sum(1, keepdim=True) + Xd[ii.clamp(min=0)].pow(2).sum(2)
        err = (dd - true).abs()
        assert bool(((err <= rtol * true + 2e-6 * scale) | ~valid).all()), float(err[valid].max())
        assert bool((dd[:, 1:] >= dd[:, :-1])[valid[:, 1:]].all())


def _pair_table(X):
    """float32 [n, n]: the squared distance the searches give every pair, through ``mde_knn_ranks``' d2_out in
    chunks of 64 listed rows (the diagonal, not a pair of a self-join, comes out FLT_MAX)."""
    from pymde_amd import _lib
    lib = _lib.load()
    n, nf = X.shape
    T = torch.empty((n, n), dtype=torch.float32, device=X.device)
    work = _lib.work_buffer(lib.mde_knn_ranks_work_bytes, n, n, 64, 0, device=X.device)
    ranks = torch.empty((n, 64), dtype=torch.int32, device=X.device)
    d2 = torch.empty((n, 64), dtype=torch.float32, device=X.device)
    for c0 in range(0, n, 64):
        cols = torch.arange(c0, c0 + 64, dtype=torch.int32, device=X.device)
        listed = torch.where(cols < n, cols, torch.full_like(cols, -1)).repeat(n, 1).contiguous()
        _lib.check(lib.mde_knn_ranks(n, n, nf, _lib.ptr(X), _lib.ptr(X), 1, 64, _lib.ptr(listed), 0,
                                     _lib.ptr(ranks), _lib.ptr(d2), _lib.ptr(work), _lib.stream_ptr(X.device)))
        T[:, c0:c0 + 64] = d2[:, :min(64, n - c0)]
    return T.cpu().numpy()


def _spoiled_lists(X, k, seed):
    """The exact lists with a seeded third of the entries replaced by random rows (self entries and repeats
    among them: ``order_lists`` has to drop those)."""
    from pymde_amd import preprocess
    n = X.shape[0]
    g = torch.Generator(device=DEV)
    g.manual_seed(seed)
    idx, _ = preprocess._dense_knn_lists(X, k)
    spoil = torch.rand(idx.shape, generator=g, device=DEV) < 1.0 / 3.0
    rand = torch.randint(0, n, idx.shape, generator=g, device=DEV, dtype=torch.int32)
    return torch.where(spoil, rand, idx).contiguous()


def _assert_pass_equals_reference(X, idx, d2, table, what):
    from pymde_amd import ann
    got_i, got_d, changed = ann.refine_lists(X, idx, d2)
    want_i, want_d, want_changed = ref.refine_pass(idx.cpu().numpy(), d2.cpu().numpy(), lambda i, c: table[i, c])
    np.testing.assert_array_equal(got_i.cpu().numpy(), want_i, err_msg=what)
    np.testing.assert_array_equal(got_d.cpu().numpy().view(np.int32), want_d.view(np.int32), err_msg=what)
    assert changed == [want_changed], what
    return got_i, got_d


# ---------------------------------------------------------------- 1. the pass equals the restatement, bit for bit
@pytest.mark.parametrize("k", [1, 15, 64])
@pytest.mark.parametrize("nf", [1, 33, 784])
def test_pass_equals_reference_bit_for_bit(nf, k):
    from pymde_amd import ann
    n = 301                                            # the last workgroup holds one row
    g = torch.Generator(device=DEV)
    g.manual_seed(100 * nf + k)
    real = torch.randn(n, nf, generator=g, device=DEV).contiguous()
    whole = torch.randint(0, 4, (n, nf), generator=g, device=DEV).float().contiguous()   # distances tie exactly
    for name, X in (("real", real), ("integer", whole)):
        table = _pair_table(X)
        raw = _spoiled_lists(X, k, seed=k)
        idx, d2 = ann.order_lists(X, raw)
        _check_lists(X, idx, d2)
        got_i, got_d = _assert_pass_equals_reference(X, idx, d2, table, name)
        assert k == 1 or not torch.equal(got_i, idx)   # the spoiled lists do improve
        # the d2=None path is the same thing from the raw indices
        raw_i, raw_d, _ = ann.refine_lists(X, raw)
        assert torch.equal(raw_i, got_i) and torch.equal(raw_d.view(torch.int32), got_d.view(torch.int32))
        # rows with trailing -1 slots, one row of only -1
        cut_i, cut_d = idx.clone(), d2.clone()
        keep = torch.randint(0, k + 1, (n,), generator=g, device=DEV)
        keep[17] = 0
        gone = torch.arange(k, device=DEV)[None, :] >= keep[:, None]
        cut_i[gone] = -1
        cut_d[gone] = float(ref.FLT_MAX)
        _assert_pass_equals_reference(X, cut_i, cut_d, table, name + ", short rows")


# ---------------------------------------------------------------- 2. exact lists are a fixed point
def test_exact_lists_are_a_fixed_point():
    from pymde_amd import ann, preprocess
    n, k = 10037, 15
    X = _mixture(n, 24, seed=2)
    idx, d2 = preprocess._dense_knn_lists(X, k)
    new_i, new_d, changed = ann.refine_lists(X, idx, d2)
    assert changed == [0]
    assert torch.equal(new_i, idx) and torch.equal(new_d.view(torch.int32), d2.view(torch.int32))
    with torch.cuda.device(X.device):
        full_i, full_d = ann.knn_lists(X, k, n_probe=10 ** 6, n_refine=1)
    assert torch.equal(full_i, idx) and torch.equal(full_d.view(torch.int32), d2.view(torch.int32))


# ---------------------------------------------------------------- 3. monotone and valid at scale
def test_monotone_valid_and_recall_rises_at_scale():
    from pymde_amd import ann, preprocess
    n, k = 20000, 15
    X = _mixture(n, 32)
    truth, _ = preprocess._dense_knn_lists(X, k)
    lists, recall = [], []
    with torch.cuda.device(X.device):
        for n_refine in (0, 1, 2):
            stats = {}
            idx, d2 = ann.knn_lists(X, k, n_probe=2, n_refine=n_refine, timings=stats)
            again_i, again_d = ann.knn_lists(X, k, n_probe=2, n_refine=n_refine)
            assert torch.equal(idx, again_i) and torch.equal(d2.view(torch.int32), again_d.view(torch.int32))
            _check_lists(X, idx, d2)
            lists.append((idx, d2))
            recall.append(float((truth[:, :, None] == idx[:, None, :]).any(2).float().mean()))
            if n_refine:
                assert len(stats["refine_changed"]) == len(stats["refine_evaluated"]) <= n_refine
                assert stats["refine"] > 0.0 and stats["refine_changed"][0] > 0
                print("n_refine", n_refine, "changed", stats["refine_changed"], "distances per row",
                      [e / n for e in stats["refine_evaluated"]])
    print("recall@15 at n_probe=2 with 0, 1, 2 passes:", recall)
    for (i0, d0), (i1, d1) in zip(lists[:-1], lists[1:]):
        e0 = torch.where(i0 < 0, torch.full_like(i0, 2 ** 31 - 1), i0)
        e1 = torch.where(i1 < 0, torch.full_like(i1, 2 ** 31 - 1), i1)
        assert not bool(((d1 > d0) | ((d1 == d0) & (e1 > e0))).any())
    assert recall[1] > recall[0]
    assert recall[2] >= recall[1]


# ---------------------------------------------------------------- 4. the public path
def test_public_path():
    import pymde_amd
    from pymde_amd import ann, metrics, preprocess
    n, k = 12000, 15
    X = _mixture(n, 20, seed=4)
    e, w = preprocess.k_nearest_neighbors(X, k, approximate=True, n_probe=2, n_refine=1)
    rows, _ = metrics.translated_rows(X)
    with torch.cuda.device(X.device):
        idx, d2 = ann.knn_lists(rows, k, n_probe=2, n_refine=1)
        plain, _ = ann.knn_lists(rows, k, n_probe=2)
    assert not torch.equal(plain, idx)
    want_e, want_w = preprocess._neighbor_lists_to_graph(n, k, idx, d2, None, X.device)
    assert torch.equal(e, want_e) and torch.equal(w, want_w)
    ec, wc = preprocess.k_nearest_neighbors(X, k, approximate=True, n_probe=2, n_refine=1, metric="cosine")
    assert ec.shape[0] > 0 and set(np.unique(wc.cpu().numpy()).tolist()) <= {1.0, 2.0}
    for bad in (True, 1.5, -1):
        with pytest.raises(ValueError, match="n_refine"):
            preprocess.k_nearest_neighbors(X, k, approximate=True, n_refine=bad)
    with pytest.raises(ValueError, match="n_refine"):
        preprocess.k_nearest_neighbors(X, k, n_refine=1)
    small = X[:5000].contiguous()
    es, ws = preprocess.k_nearest_neighbors(small, k)
    ea, wa = preprocess.k_nearest_neighbors(small, k, approximate=True, n_probe=1, n_refine=2)
    assert torch.equal(ea, es) and torch.equal(wa, ws)
    torch.manual_seed(0)
    mde = pymde_amd.preserve_neighbors(X, embedding_dim=2, seed=0,
                                       approximate_neighbors={"n_probe": 2, "n_refine": 1})
    Z = mde.embed(max_iter=20)
    assert Z.shape == (n, 2) and bool(torch.isfinite(Z).all())


# ---------------------------------------------------------------- 5. the C entries' argument checks
def test_c_entries_reject_invalid_arguments():
    from pymde_amd import _lib, ann
    lib = _lib.load()
    n, nf, k = 100, 5, 3
    X = torch.rand(n, nf, device=DEV)
    idx, d2 = ann.order_lists(X, torch.randint(0, n, (n, k), device=DEV, dtype=torch.int32))
    a = dict(n=n, nf=nf, X=X, sqn=ann._row_sqnorm(X), k=k, idx=idx, d2=d2, rev=ann.reverse_lists(idx, d2),
             idx_out=torch.full((n, k), -7, dtype=torch.int32, device=DEV), d2_out=torch.full((n, k), -7.0, device=DEV),
             changed=torch.full((1,), -7, dtype=torch.int32, device=DEV),
             work=torch.zeros(16, dtype=torch.uint8, device=DEV))
    order = ["n", "nf", "X", "sqn", "k", "idx", "d2", "rev", "idx_out", "d2_out", "changed", "work"]

    def call(**over):
        b = dict(a, **over)
        rc = lib.mde_knn_refine(*[_lib.ptr(b[key]) if isinstance(b[key], torch.Tensor) else b[key] for key in order],
                                _lib.stream_ptr())
        torch.cuda.synchronize()
        return rc

    bad = {"k = 0": {"k": 0}, "k = 65": {"k": 65}, "n = 0": {"n": 0}, "n = 2^31": {"n": 2 ** 31}, "nf = 0": {"nf": 0},
           "outputs are the inputs": {"idx_out": idx}}
    bad.update({"null " + key: {key: None} for key in order if isinstance(a[key], torch.Tensor)})
    for what, over in bad.items():
        assert call(**over) == _lib.MDE_E_INVALID, what
        assert "mde_knn_refine" in _lib.last_error()
        for out in (a["idx_out"], a["d2_out"], a["changed"]):
            assert bool((out == -7).all()), what                     # nothing launched
    assert lib.mde_knn_refine_work_bytes(n, 0) == _lib.MDE_E_INVALID
    assert lib.mde_knn_refine_work_bytes(n, 65) == _lib.MDE_E_INVALID
    assert lib.mde_knn_refine_work_bytes(0, k) == _lib.MDE_E_INVALID
    assert lib.mde_knn_refine_work_bytes(2 ** 31, k) == _lib.MDE_E_INVALID
    assert lib.mde_knn_refine_work_bytes(n, k) >= 8
    assert call() == _lib.MDE_OK
    assert bool((a["idx_out"] >= -1).all()) and int(a["changed"].item()) >= 0

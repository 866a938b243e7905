"""Queries against a corpus on packed rows: mde_bits_knn through the C ABI at every slice count, and
preprocess.cross_nearest_neighbors on two BitMatrix arguments, against tests/_binary_reference.py."""
import functools

import numpy as np
import pytest
import torch

import _binary_reference as ref
from pymde_amd import _lib, binary, preprocess

pytestmark = pytest.mark.gpu

NF = 200
NQS = [1, 64, 100]
NCS = [1, 63, 1000, 4101]
FLT_MAX = np.float32(3.402823466e+38)


@functools.lru_cache(maxsize=None)
def _corpus(n_c):
    C = ref.make_bits(n_c, NF, 0.1, seed=1)
    return C, binary.pack(C)


@functools.lru_cache(maxsize=None)
def _queries(n_q):
    Q = ref.make_bits(n_q, NF, 0.1, seed=2, clear=(0,))
    C = _corpus(4101)[0]
    if n_q > 7:
        Q[7] = C[11]                       # a query equal to corpus row 11 (where the corpus has one)
    return Q, binary.pack(Q)


def _call(q, c, k, slices, self_join=0, kind=None, nw=None, nf=None, null=None, n_q=None):
    """mde_bits_knn as the C ABI takes it: (rc, idx int32 [n_q, k], dist float32 [n_q, k]) with the outputs
    pre-filled, so that a refused call is seen to have written nothing."""
    lib = _lib.load()
    dev = c.device
    n_q = q.shape[0] if n_q is None else n_q
    idx = torch.full((n_q, max(k, 1)), -7, dtype=torch.int32, device=dev)
    dist = torch.full((n_q, max(k, 1)), -7.0, dtype=torch.float32, device=dev)
    nbytes = int(lib.mde_bits_knn_work_bytes(n_q, c.shape[0], k, slices))
    work = torch.empty(max(nbytes, 8), dtype=torch.uint8, device=dev)
    args = [n_q, c.shape[0], int(c.words.shape[1]) if nw is None else nw, c.n_features if nf is None else nf,
            _lib.ptr(q.words), _lib.ptr(q.counts), _lib.ptr(c.words), _lib.ptr(c.counts), self_join,
            c.kind if kind is None else kind, k, slices, _lib.ptr(idx), _lib.ptr(dist), _lib.ptr(work),
            _lib.stream_ptr(dev)]
    if null is not None:
        args[null] = None
    rc = lib.mde_bits_knn(*args)
    torch.cuda.synchronize()
    return rc, idx.cpu().numpy(), dist.cpu().numpy(), nbytes


@pytest.mark.parametrize("distance", ["jaccard", "hamming"])
@pytest.mark.parametrize("n_c", NCS)
@pytest.mark.parametrize("n_q", NQS)
def test_every_slice_count_gives_the_reference(n_q, n_c, distance):
    (Q, q), (C, c) = _queries(n_q), _corpus(n_c)
    q, c = q.with_distance(distance), c.with_distance(distance)
    k = 15
    want_idx, want_val = ref.cross_lists(Q, C, k, distance)
    want_val = np.where(want_idx < 0, FLT_MAX, want_val).astype(np.float32)
    for slices in (1, 2, 5, 0):
        rc, idx, dist, _ = _call(q, c, k, slices)
        assert rc == _lib.MDE_OK, _lib.last_error()
        assert np.array_equal(idx, want_idx), slices
        assert np.array_equal(dist.view(np.uint32), want_val.view(np.uint32)), slices
    # k above n_c: -1 / +inf through the Python entry
    idx, dist = preprocess.cross_nearest_neighbors(q, c, k)
    assert idx.dtype == torch.int64 and dist.dtype == torch.float32
    idx, dist = idx.cpu().numpy(), dist.cpu().numpy()
    assert np.array_equal(idx, want_idx)
    assert np.array_equal(np.isinf(dist), want_idx < 0) and (n_c >= k or np.isinf(dist[:, n_c:]).all())
    assert np.array_equal(dist[want_idx >= 0], want_val[want_idx >= 0])


def test_k_64_and_many_slices():
    (Q, q), (C, c) = _queries(100), _corpus(4101)
    want_idx, want_val = ref.cross_lists(Q, C, 64, "jaccard")
    for slices in (1, 7, 65):              # 65 slices of one tile each: the last one holds 5 rows
        rc, idx, dist, _ = _call(q, c, 64, slices)
        assert rc == _lib.MDE_OK
        assert np.array_equal(idx, want_idx) and np.array_equal(dist.view(np.uint32), want_val.view(np.uint32))
    rc, idx, dist, _ = _call(q, c, 64, 100)        # more slices than tiles: the empty ones add nothing
    assert rc == _lib.MDE_OK and np.array_equal(idx, want_idx)


def test_a_query_equal_to_corpus_rows_lists_them_at_zero_smallest_index_first():
    C = ref.make_bits(300, NF, 0.1, seed=3)
    C[250] = C[40]
    C[120] = C[40]
    q, c = binary.pack(C[40:41]), binary.pack(C)
    for distance in ("jaccard", "hamming"):
        idx, dist = preprocess.cross_nearest_neighbors(q.with_distance(distance), c.with_distance(distance), 4)
        assert idx[0, :3].tolist() == [40, 120, 250] and dist[0, :3].tolist() == [0.0, 0.0, 0.0]
        assert float(dist[0, 3]) > 0.0


def test_max_distance_and_the_self_join_through_the_abi():
    (Q, q), (C, c) = _queries(100), _corpus(1000)
    want_idx, want_val = ref.cross_lists(Q, C, 15, "jaccard")
    cut = float(np.median(want_val))
    idx, dist = preprocess.cross_nearest_neighbors(q, c, 15, max_distance=cut)
    keep = want_val <= cut
    assert np.array_equal(idx.cpu().numpy(), np.where(keep, want_idx, -1))
    assert np.array_equal(dist.cpu().numpy(), np.where(keep, want_val, np.float32(np.inf)))
    # self = 1 with slices: the self-join's lists for every slice count
    sidx, sval = ref.knn_lists(C, 15, "jaccard")
    for slices in (1, 3, 0):
        rc, idx, dist, _ = _call(c, c, 15, slices, self_join=1)
        assert rc == _lib.MDE_OK
        assert np.array_equal(idx, sidx) and np.array_equal(dist.view(np.uint32), sval.view(np.uint32))


def test_mismatched_bitmatrices_are_a_value_error():
    c = _corpus(63)[1]
    other = binary.pack(ref.make_bits(10, NF + 1, 0.1))
    with pytest.raises(ValueError, match="features"):
        preprocess.cross_nearest_neighbors(other, c, 3)
    with pytest.raises(ValueError, match="hamming"):
        preprocess.cross_nearest_neighbors(c.with_distance("hamming"), c, 3)
    with pytest.raises(ValueError, match="BitMatrix"):
        preprocess.cross_nearest_neighbors(np.zeros((4, NF), np.float32), c, 3)


def test_argument_errors_are_invalid_and_launch_nothing():
    (Q, q), (C, c) = _queries(64), _corpus(63)
    nw = int(c.words.shape[1])

    def refused(**kw):
        rc, idx, dist, _ = _call(q, c, kw.pop("k", 5), kw.pop("slices", 1), **kw)
        assert rc == _lib.MDE_E_INVALID and _lib.last_error().startswith("mde_bits_knn")
        assert (idx == -7).all() and (dist == -7.0).all()

    refused(k=65)
    refused(k=0)
    for pointer in (4, 5, 6, 7, 12, 13, 14):
        refused(null=pointer)
    refused(self_join=1)                              # n_q != n_c (and Q != C)
    refused(nw=nw + 1)
    refused(nw=nw - 1)
    refused(nf=NF + 32)                               # ceil(nf / 32) no longer nw
    refused(nf=2 ** 24, nw=2 ** 19)
    refused(nf=0, nw=0)
    refused(kind=2)
    refused(slices=-1)
    refused(slices=65536)
    lib = _lib.load()
    assert lib.mde_bits_knn_work_bytes(64, 63, 65, 1) == _lib.MDE_E_INVALID
    assert lib.mde_bits_knn_work_bytes(64, 63, 0, 1) == _lib.MDE_E_INVALID
    assert lib.mde_bits_knn_work_bytes(0, 63, 5, 1) == _lib.MDE_E_INVALID
    assert lib.mde_bits_knn_work_bytes(2 ** 31, 63, 5, 1) == _lib.MDE_E_INVALID
    assert lib.mde_bits_knn_work_bytes(64, 63, 5, 4) == 8 * 4 * 64 * 5

"""The bfloat16 k-NN search (``precision="bfloat16"``), the part that needs no GPU: the argument errors, the
default shortlist length, and a CPU emulation of the bfloat16 shortlist on the inputs of
test_gpu_knn_bf16.py -- that test may only demand the float32 result where this one shows that the shortlist
holds every true neighbour with places to spare."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

import _knn_bf16_cases as cases
from pymde_amd import preprocess, recipes

X = np.zeros((40, 3), dtype=np.float32)


def test_default_n_candidates_rule():
    f = preprocess.default_n_candidates
    assert [f(k) for k in (1, 5, 15, 16, 17, 32, 48, 49, 64)] == [17, 21, 31, 32, 34, 64, 64, 64, 64]
    assert f(15, available=1000) == 31 and f(15, available=20) == 20      # capped by the rows there are,
    assert f(15, available=15) == 15 and f(15, available=3) == 15         # never below k
    assert preprocess.MAX_CANDIDATES == 64


def test_precision_names():
    assert preprocess.resolve_precision("float32") == "float32"
    assert preprocess.resolve_precision("bf16") == preprocess.resolve_precision(" BFloat16 ") == "bfloat16"
    for bad in ("float16", "fp64", None, 16):
        with pytest.raises(ValueError, match="unknown precision"):
            preprocess.resolve_precision(bad)


@pytest.mark.parametrize("kwargs, message", [
    (dict(precision="half"), "unknown precision"),
    (dict(precision="bfloat16", metric="manhattan"), "no Manhattan search"),
    (dict(precision="bf16", approximate=True), "approximate=True"),
    (dict(n_candidates=31), "n_candidates is the shortlist length"),
    (dict(precision="bf16", n_candidates=14), r"n_candidates must lie in \[k, 64\]"),
    (dict(precision="bf16", n_candidates=65), r"n_candidates must lie in \[k, 64\]"),
])
def test_k_nearest_neighbors_argument_errors_need_no_device(kwargs, message):
    with pytest.raises(ValueError, match=message):
        preprocess.k_nearest_neighbors(X, 15, **kwargs)


def test_graph_input_is_refused():
    class g:                                   # quacks like a Graph; never touched: the precision is checked first
        edges, n_items = None, 4
    with pytest.raises(ValueError, match="a Graph has its own"):
        preprocess.k_nearest_neighbors(g, 2, precision="bfloat16")
    with pytest.raises(ValueError, match="a Graph has its own"):
        preprocess.cross_nearest_neighbors(g, X, 2, precision="bfloat16")


@pytest.mark.parametrize("kwargs, message", [
    (dict(precision="half"), "unknown precision"),
    (dict(precision="bf16", metric="l1"), "no Manhattan search"),
    (dict(n_candidates=31), "n_candidates is the shortlist length"),
    (dict(precision="bf16", n_candidates=3), r"n_candidates must lie in \[k, 64\]"),
    (dict(precision="bf16", n_candidates=100), r"n_candidates must lie in \[k, 64\]"),
])
def test_cross_nearest_neighbors_argument_errors_need_no_device(kwargs, message):
    with pytest.raises(ValueError, match=message):
        preprocess.cross_nearest_neighbors(X[:5], X, 5, **kwargs)


def test_recipes_argument_errors_need_no_device():
    with pytest.raises(ValueError, match="unknown precision"):
        recipes.preserve_neighbors(X, neighbor_precision="double")
    with pytest.raises(ValueError, match="no Manhattan search"):
        recipes.preserve_neighbors(X, neighbor_precision="bf16", metric="manhattan")
    with pytest.raises(ValueError, match="approximate=True"):
        recipes.laplacian_embedding(X, neighbor_precision="bf16", approximate_neighbors=True)
    with pytest.raises(ValueError, match="unknown precision"):
        recipes.extend_embedding(X, torch.zeros(40, 2), X[:3], neighbor_precision="double")


def test_sparse_message_names_the_way_out():
    msg = preprocess._BF16_SPARSE_DOES_NOT_FIT.format(n=10, nf=20)
    assert "does not fit" in msg and "10 x 20" in msg and "precision='float32'" in msg
    assert sp.issparse(sp.csr_matrix(X))


# ---------------------------------------------------------------- the shortlist emulation
@pytest.mark.parametrize("kind", cases.GENERATORS)
@pytest.mark.parametrize("n, nf, k", cases.SELF_SHAPES)
def test_emulated_shortlist_keeps_every_true_neighbour_self(kind, n, nf, k):
    data = cases.make(kind, n, nf)
    n_cand = preprocess.default_n_candidates(k, n - 1)
    worst = cases.worst_place(data, data, k, True)
    print("%s %d x %d k=%d: worst shortlist place %d of %d" % (kind, n, nf, k, worst, n_cand))
    assert worst <= n_cand - cases.MARGIN
    assert cases.shortlist_is_safe(data, data, k, True)


@pytest.mark.parametrize("n_q, n_c, nf, k", cases.CROSS_SHAPES)
def test_emulated_shortlist_keeps_every_true_neighbour_cross(n_q, n_c, nf, k):
    Q, C = cases.cross_pair("mixture", n_q, n_c, nf)
    n_cand = preprocess.default_n_candidates(k, n_c)
    worst = cases.worst_place(Q, C, k, False)
    print("mixture %d x %d x %d k=%d: worst shortlist place %d of %d" % (n_q, n_c, nf, k, worst, n_cand))
    assert worst <= n_cand - cases.MARGIN


def test_emulation_of_integer_data_is_exact():
    """Small integers minus their grid means are bfloat16 numbers: the shortlist ranks by the true distances
    and a true neighbour never leaves the first k places, ties included."""
    data = cases.make("ints", 1037, 50)
    Qb, Cb = cases.bf16_points(data, data)
    assert np.array_equal(Qb, Cb)
    assert np.array_equal(Qb - Qb[0], data.astype(np.float64) - data[0].astype(np.float64))
    assert cases.worst_place(data, data, 15, True) <= 15

"""The exact k-NN entry points (mde_knn, mde_knn_cross, mde_knn_l1) reproduce recorded results bit for bit.

tests/golden/knn_bits.npz holds the inputs and the raw (idx, d2 / dist) outputs recorded by
tests/golden/make_knn_bits.py before the three Gram-tile kernels were moved onto one shared tile
(csrc/mde_knn_tile.h).  The dot products keep their feature order, so every squared distance keeps its bits;
the shapes cover each tile edge: row block, column tile, feature chunk, a list shorter than k, slice boundary.
"""
import importlib.util
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, load_golden

pytestmark = pytest.mark.gpu
DEV = "cuda"

_spec = importlib.util.spec_from_file_location("make_knn_bits", os.path.join(GOLDEN, "make_knn_bits.py"))
bits = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(bits)


@pytest.fixture(scope="module")
def golden():
    return load_golden("knn_bits")


def _assert_same_bits(got, want):
    (idx, d), (idx_w, d_w) = got, want
    assert idx.dtype == np.int32 and d.dtype == np.float32 and idx_w.dtype == np.int32 and d_w.dtype == np.float32
    assert np.array_equal(idx, idx_w)
    assert np.array_equal(d.view(np.uint32), d_w.view(np.uint32))


@pytest.mark.parametrize("name", list(bits.KNN_CASES))
def test_knn_bits(golden, name):
    from pymde_amd import _lib
    n, nf, k = bits.KNN_CASES[name]
    X = golden[name + "__X"]
    assert X.shape == (n, nf)
    want = golden[name + "__idx"], golden[name + "__d2"]
    assert want[0].shape == (n, k)
    if n <= k:                                                # fewer rows than k: the tail is empty
        assert (want[0][:, n - 1:] == -1).all() and (want[1][:, n - 1:] == np.float32(3.402823466e+38)).all()
    _assert_same_bits(bits.run_knn(_lib, torch.tensor(X, device=DEV), k), want)


@pytest.mark.parametrize("slices", bits.CROSS_CASE[5])
def test_knn_cross_bits(golden, slices):
    from pymde_amd import _lib
    name, n_q, n_c, nf, k, _ = bits.CROSS_CASE
    Q, C = golden[name + "__Q"], golden[name + "__C"]
    assert Q.shape == (n_q, nf) and C.shape == (n_c, nf)
    want = golden["%s__s%d__idx" % (name, slices)], golden["%s__s%d__d2" % (name, slices)]
    _assert_same_bits(bits.run_cross(_lib, torch.tensor(Q, device=DEV), torch.tensor(C, device=DEV), k, slices),
                      want)


def test_knn_l1_bits(golden):
    from pymde_amd import _lib
    name, n, nf, k = bits.L1_CASE
    X = golden["knn_n130_nf33_k15__X"]
    assert X.shape == (n, nf)
    _assert_same_bits(bits.run_l1(_lib, torch.tensor(X, device=DEV), k), (golden[name + "__idx"], golden[name + "__d"]))

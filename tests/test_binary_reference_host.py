"""tests/_binary_reference.py against scipy.spatial.distance.cdist: the reference the GPU tests compare with
bit for bit is itself within one float32 rounding of scipy's float64 Jaccard and Hamming distances."""
import numpy as np
import pytest
from scipy.spatial.distance import cdist

import _binary_reference as ref

SHAPES = [(1037, 50, 0.3), (257, 2048, 0.05), (130, 3, 0.5), (300, 33, 0.5), (65, 1025, 0.5)]
# one float32 rounding of a value in [0, 1] is at most 2^-25; scipy's own float64 rounding is far below the slack
BOUND = 2.0 ** -24


@pytest.mark.parametrize("distance", ["jaccard", "hamming"])
@pytest.mark.parametrize("n,nf,p", SHAPES)
def test_reference_agrees_with_scipy(n, nf, p, distance):
    B = ref.make_bits(n, nf, p)
    got = ref.cross_distances(B, B, distance)
    want = cdist(B, B, distance)
    assert got.dtype == np.float32
    err = float(np.abs(got.astype(np.float64) - want).max())
    print(f"{distance} {n} x {nf}: max |reference - scipy| = {err:.3e}, "
          f"mismatches against float32(scipy): {int((got != want.astype(np.float32)).sum())}")
    assert err <= BOUND


@pytest.mark.parametrize("distance", ["jaccard", "hamming"])
def test_empty_rows(distance):
    B = np.zeros((3, 40), dtype=bool)
    B[2, ::3] = True
    D = ref.cross_distances(B, B, distance)
    assert D[0, 1] == 0.0 and D[0, 0] == 0.0
    if distance == "jaccard":
        assert D[0, 2] == 1.0 and D[2, 1] == 1.0
    else:
        assert D[0, 2] == np.float32(14) / np.float32(40)


def test_lists_are_ordered_by_value_then_index_and_exclude_self():
    B = ref.make_bits(130, 3, 0.5)
    idx, val = ref.knn_lists(B, 15, "jaccard")
    assert not (idx == np.arange(130)[:, None]).any()
    assert (np.diff(val, axis=1) >= 0).all()
    ties = np.diff(val, axis=1) == 0
    assert ties.any() and (np.diff(idx, axis=1)[ties] > 0).all()
    assert 5 in idx[3] and val[3][list(idx[3]).index(5)] == 0.0
    cidx, cval = ref.cross_lists(B[:4], B[:2], 5, "hamming")
    assert (cidx[:, 2:] == -1).all() and np.isinf(cval[:, 2:]).all() and (cidx[:, :2] >= 0).all()

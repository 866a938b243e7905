"""Host side of the query-against-corpus k-NN search (``mde_knn_cross``, csrc/mde_knn.hip): arguments are
refused before any launch and the scratch size follows the slice count.  The library loads without a GPU,
and none of these calls reaches one."""
import ctypes

import pytest

from pymde_amd import _lib

FAKE = ctypes.c_void_p(0x1000)      # a non-null pointer that is never dereferenced: the checks come first


def _cross(n_q=10, n_c=100, nf=8, Q=FAKE, C=FAKE, k=5, slices=1, idx=FAKE, d2=FAKE, work=FAKE):
    return _lib.load().mde_knn_cross(n_q, n_c, nf, Q, C, k, slices, idx, d2, work, None)


@pytest.mark.parametrize("kw", [{"k": 0}, {"k": 65}, {"k": -1}, {"n_c": 0}, {"n_q": 0}, {"nf": 0}, {"slices": -1},
                                {"slices": 65536}, {"Q": None}, {"C": None}, {"idx": None}, {"d2": None},
                                {"work": None}])
def test_invalid_arguments_are_refused_before_any_launch(kw):
    assert _cross(**kw) == _lib.MDE_E_INVALID
    assert "mde_knn_cross" in _lib.last_error()


def test_work_bytes():
    wb = _lib.load().mde_knn_cross_work_bytes
    n_q, n_c, k = 1000, 50000, 15
    assert wb(n_q, n_c, k, 1) == 4 * (n_q + n_c)                       # the row norms of Q and C alone
    sizes = [wb(n_q, n_c, k, s) for s in (1, 2, 3, 7, 64)]
    assert sizes == sorted(set(sizes))                                  # strictly growing with the slice count
    assert wb(n_q, n_c, k, 7) == 4 * (n_q + n_c) + 8 * 7 * n_q * k      # plus [slices, n_q, k] of (d2, idx)
    assert wb(3, 2 ** 31 - 1, 64, 65535) > 2 ** 32                      # 64-bit sizes
    for bad in ((0, n_c, k, 1), (n_q, 0, k, 1), (n_q, n_c, 0, 1), (n_q, n_c, 65, 1), (n_q, n_c, k, -1),
                (n_q, n_c, k, 65536)):
        assert wb(*bad) == _lib.MDE_E_INVALID

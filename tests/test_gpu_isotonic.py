"""pymde_amd.isotonic on the GPU (csrc/mde_isotonic.hip) against the float64 pool-adjacent-violators of
tests/_ordinal_reference.py: the accuracy bound of include/mde_hip.h, exact monotonicity, the optimality conditions
tested from the output alone, and equal bits on two runs -- over sizes around the leaf of the merge tree (odd node
counts on several levels, ten levels at the top) and the patterns that send a tangent to either end."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _ordinal_reference as ref  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _sizes():
    from pymde_amd import isotonic
    L = isotonic.leaf()
    return (1, 2, 3, 63, 64, 65, L - 1, L, L + 1, 2 * L + 1, 3 * L, 100003, 2 ** 20 + 1)


def _check(y, w, what):
    from pymde_amd import isotonic
    wt = None if w is None else torch.as_tensor(w, device=DEV)
    out = isotonic.regression(torch.as_tensor(y, device=DEV), wt)
    again = isotonic.regression(y, w)                      # the numpy door, a fresh work buffer
    assert out.dtype == torch.float32 and out.is_cuda and tuple(out.shape) == y.shape
    assert torch.equal(out, again), what
    got = out.cpu().numpy()
    w64 = None if w is None else w.astype(np.float64)
    want = ref.isotonic(y.astype(np.float64), w64)
    tol = ref.bound(y, w64)
    err = np.abs(got.astype(np.float64) - want).max()
    viol, weight = ref.kkt_violation(y, w64, got)
    print(what, "err %.3e bound %.3e kkt %.3e allowed %.3e" % (err, tol, viol, tol * max(weight, 0.0)))
    assert np.all(got[1:] >= got[:-1]), what
    assert err <= tol, (what, err, tol)
    assert viol <= tol * weight, (what, viol, tol * weight)


@pytest.mark.parametrize("weights", ["none", "integers"])
@pytest.mark.parametrize("name", ref.PATTERNS)
def test_regression(name, weights):
    for p in _sizes():
        y = ref.pattern(name, p, seed=p % 1000)
        w = None
        if weights == "integers":
            w = np.random.default_rng(p + 7).integers(1, 17, p).astype(np.float32)
        _check(y, w, "%s p=%d weights=%s" % (name, p, weights))


def test_wide_weights():
    rng = np.random.default_rng(5)
    y = ref.pattern("noisy_ramp", 4096, seed=11)
    w = rng.uniform(1e-3, 1e3, 4096).astype(np.float32)
    _check(y, w, "noisy_ramp p=4096 weights in [1e-3, 1e3]")
    _check(ref.pattern("normal", 4096, seed=12), w, "normal p=4096 weights in [1e-3, 1e3]")


def test_decreasing_and_empty():
    from pymde_amd import isotonic
    y = ref.pattern("noisy_ramp", 3000, seed=2)
    down = isotonic.regression(-y, increasing=False)
    assert torch.equal(down, -isotonic.regression(y))
    assert np.all(np.diff(down.cpu().numpy()) <= 0)
    empty = isotonic.regression(np.zeros(0, np.float32))
    assert empty.numel() == 0 and empty.dtype == torch.float32 and empty.is_cuda
    assert isotonic.regression(torch.zeros(0, device=DEV), torch.zeros(0, device=DEV)).numel() == 0


def test_errors():
    from pymde_amd import isotonic
    y = np.arange(5, dtype=np.float32)
    for bad in (np.nan, np.inf, -np.inf):
        z = y.copy()
        z[3] = bad
        with pytest.raises(ValueError):
            isotonic.regression(z)
    for bad in (np.nan, np.inf, 0.0, -1.0):
        w = np.ones(5, np.float32)
        w[2] = bad
        with pytest.raises(ValueError):
            isotonic.regression(y, w)
    with pytest.raises(ValueError):
        isotonic.regression(y, np.ones(4, np.float32))
    with pytest.raises(ValueError):
        isotonic.regression(np.zeros((3, 2), np.float32))
    with pytest.raises(ValueError):
        isotonic.regression(y, np.ones((5, 1), np.float32))
    # the unchecked door still refuses buffers that the kernels would overrun
    z = torch.zeros(5000, device=DEV)
    with pytest.raises(ValueError):
        isotonic.run(z, None, torch.empty_like(z), isotonic.work_buffer(10, DEV))
    with pytest.raises(ValueError):
        isotonic.run(z, None, torch.empty(4999, device=DEV), isotonic.work_buffer(5000, DEV))

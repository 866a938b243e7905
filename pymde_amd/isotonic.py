"""Weighted isotonic regression on the GPU (``csrc/mde_isotonic.hip``).

``regression(y, weights)`` is the nondecreasing sequence that minimises ``sum_i w_i (y_i - out_i)^2``: the monotone
least-squares fit that ordinal MDS (``pymde_amd.ordinal``) takes once per round over every edge.  The kernels build
the lower convex hull of the cumulative-sum diagram by a merge tree, so the depth of the computation does not
depend on the data; sums are in double and in a fixed order, and the result has the same bits on every run.
"""
import numpy as np
import torch

from pymde_amd import _lib
from pymde_amd import util


def leaf():
    """Points per leaf of the merge tree (tests place their sizes around it)."""
    return int(_lib.load().mde_isotonic_leaf())


def work_buffer(p, device):
    """The uint8 work buffer ``run`` needs for ``p`` values."""
    return _lib.work_buffer(_lib.load().mde_isotonic_work_bytes, int(p), device=device)


def run(y, weights, out, work):
    """``mde_isotonic`` on float32 device vectors that the caller has checked (``weights`` may be None: all ones);
    asynchronous on the current stream.  Returns ``out``."""
    p = int(y.numel())
    if int(out.numel()) != p or (weights is not None and int(weights.numel()) != p):
        raise ValueError(f"`y` has {p} values, `out` {int(out.numel())}"
                         + ("" if weights is None else f" and `weights` {int(weights.numel())}"))
    if p:
        need = int(_lib.load().mde_isotonic_work_bytes(p))
        if work.dtype != torch.uint8 or int(work.numel()) < need:
            raise ValueError(f"the work buffer holds {int(work.numel())} bytes of {work.dtype}; {p} values need "
                             f"{need} bytes of uint8 (isotonic.work_buffer)")
        with torch.cuda.device(y.device):
            _lib.check(_lib.load().mde_isotonic(p, _lib.ptr(y), _lib.ptr(weights), _lib.ptr(out), _lib.ptr(work),
                                                _lib.stream_ptr(y.device)))
    return out


def _vector(values, name, device):
    if isinstance(values, np.ndarray):
        values = torch.from_numpy(np.ascontiguousarray(values))
    elif not isinstance(values, torch.Tensor):
        values = torch.as_tensor(values)
    if values.dim() != 1:
        raise ValueError(f"`{name}` must have one dimension (got shape {tuple(values.shape)})")
    return values.detach().to(device=device, dtype=torch.float32).contiguous()


def regression(y, weights=None, *, increasing=True):
    """The isotonic regression of ``y`` (a numpy array or torch tensor of one dimension) under positive
    ``weights`` (default: all ones), as a float32 tensor on the GPU (the device of ``y`` when it is there, else
    the default device).  The input is taken as float32.  ``increasing=False`` fits a nonincreasing sequence.

    The result is exactly monotone and within ``2^-23 max|y| + 2^-47 sum(w |y|) / min(w)`` of the exact fit.
    ``ValueError`` for a non-finite ``y``, a non-finite or non-positive weight, a length mismatch and more than one
    dimension."""
    if isinstance(y, torch.Tensor) and y.is_cuda:
        device = y.device
    else:
        device = util.get_default_device()
    device = util.require_cuda_device(device)
    y = _vector(y, "y", device)
    if weights is not None:
        weights = _vector(weights, "weights", device)
        if weights.numel() != y.numel():
            raise ValueError(f"`weights` has {weights.numel()} entries, `y` has {y.numel()}")
    p = int(y.numel())
    out = torch.empty(p, dtype=torch.float32, device=device)
    if p == 0:
        return out
    if not bool(torch.isfinite(y).all()):
        raise ValueError("`y` must be finite")
    if weights is not None and not bool((torch.isfinite(weights) & (weights > 0)).all()):
        raise ValueError("`weights` must be finite and positive")
    if not increasing:
        y = -y
    run(y, weights, out, work_buffer(p, device))
    return out if increasing else out.neg_()

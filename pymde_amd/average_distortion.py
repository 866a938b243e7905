"""The average-distortion operator on the HIP kernels.

Host-side mirror of the reference's ``pymde/average_distortion.py``
[ref: average_distortion.py:38-129]:

  * ``EdgePlan``        -- owns an ``mde_plan`` (symmetrised incidence CSR built once per edge
                           list on the device; replaces the ``_lhs/_rhs`` gather indices,
                           problem.py:163-170).
  * ``Binding``         -- a distortion function bound to a plan: per-edge parameters permuted
                           into plan order once, plus the ``mde_func`` descriptor.
  * ``_AverageDistortion`` (autograd.Function) -- E(X) and dE/dX in ONE kernel launch for
                           built-in functions; for arbitrary callables the reference's
                           three-stage structure (distances -> torch autograd on f ->
                           scatter) with HIP kernels for the first and last stage.
  * ``_Norm``           -- distances with the reference's sub-gradient convention at 0.

No stage has a CPU or PyTorch fallback.
"""
import ctypes

import torch

from pymde_amd import _lib
from pymde_amd import util


def _check_X(X, n=None, d=None):
    if not isinstance(X, torch.Tensor) or X.dim() != 2:
        raise ValueError("the embedding must be a 2-D tensor")
    if X.dtype != torch.float32:
        raise ValueError(
            "pymde_amd computes in float32; got an embedding of dtype %s (MDE.embed and "
            "MDE.average_distortion cast float64 inputs with a warning; the kernels themselves do not)" % X.dtype)
    util.require_cuda_device(X.device)
    if n is not None and X.shape[0] != n:
        raise ValueError("embedding has %d rows, the problem has %d items" % (X.shape[0], n))


class EdgePlan(object):
    """Device-resident edge plan (see include/mde_hip.h `mde_plan`)."""

    def __init__(self, n_items, edges, row_lo=0, row_hi=None):
        lib = _lib.load()
        device = util.require_cuda_device(edges.device)
        if edges.dtype != torch.int64 or edges.dim() != 2 or edges.shape[1] != 2:
            raise ValueError("edges must be an int64 tensor of shape (p, 2)")
        self.device = device
        self.n = int(n_items)
        self.p = int(edges.shape[0])
        self.edges = edges.contiguous()
        self.row_lo = int(row_lo)
        self.row_hi = self.n if row_hi is None else int(row_hi)
        handle = ctypes.c_void_p()
        with torch.cuda.device(device):
            rc = lib.mde_plan_create(self.n, self.p, _lib.ptr(self.edges), self.row_lo, self.row_hi,
                                     _lib.stream_ptr(device), ctypes.byref(handle))
        if rc == _lib.MDE_E_SELF_EDGE:
            offending = torch.where(self.edges[:, 0] == self.edges[:, 1])[0]
            raise ValueError(
                "The edge list must not contain self edges; the "
                "following rows were found to be self edges: ", offending.cpu().numpy())
        if rc == _lib.MDE_E_RANGE:
            raise ValueError("edges reference items outside [0, n_items): " + _lib.last_error())
        _lib.check(rc)
        self._handle = handle
        self.half_edges = int(lib.mde_plan_half_edges(handle))

    @property
    def handle(self):
        return self._handle

    @property
    def is_full(self):
        return self.row_lo == 0 and self.row_hi == self.n

    def expand(self, per_edge, layout=0):
        """Permute a per-edge array [p] into plan order (layout 0: CSR, 1: LDS ring)."""
        lib = _lib.load()
        t = per_edge.detach().to(device=self.device, dtype=torch.float32).contiguous().reshape(-1)
        if t.numel() != self.p:
            raise ValueError(
                "distortion function has %d parameters but the problem has %d edges"
                % (t.numel(), self.p))
        size = int(lib.mde_plan_layout_half_edges(self._handle, int(layout)))
        out = torch.empty(max(size, 1), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(lib.mde_plan_expand_layout(self._handle, int(layout), _lib.ptr(t),
                                                  _lib.ptr(out), _lib.stream_ptr(self.device)))
        return out

    def expand_codebook(self, per_edge, spec=None):
        """Layout 1 only: the codebook form of a per-edge array with at most 7 distinct values
        (``mde_plan_expand_codebook``), or None when it does not apply.  With the function's ``spec``
        (``mde_plan_expand_codebook_for``) the result is ``(stream or None, a0_scalar code)``: 2, or 4 for the pair
        codebook of one or two values under a function that allows it."""
        lib = _lib.load()
        t = per_edge.detach().to(device=self.device, dtype=torch.float32).contiguous().reshape(-1)
        if t.numel() != self.p:
            return None if spec is None else (None, 0)
        size = int(lib.mde_plan_layout_half_edges(self._handle, 1))
        out = torch.empty(max(size, 1), dtype=torch.float32, device=self.device)
        nv, form = ctypes.c_int32(0), ctypes.c_int32(0)
        with torch.cuda.device(self.device):
            if spec is None:
                _lib.check(lib.mde_plan_expand_codebook(self._handle, _lib.ptr(t), _lib.ptr(out),
                                                        ctypes.byref(nv), _lib.stream_ptr(self.device)))
                return out if nv.value > 0 else None
            f = spec.to_struct(out, None)   # (kind, kind_neg and the scalars are what is read)
            _lib.check(lib.mde_plan_expand_codebook_for(self._handle, ctypes.byref(f), _lib.ptr(t), _lib.ptr(out),
                                                        ctypes.byref(nv), ctypes.byref(form),
                                                        _lib.stream_ptr(self.device)))
        return (out, form.value) if nv.value > 0 else (None, 0)

    def expand_bytes(self, per_edge):
        """Layout 1 only: the byte-index form of a per-edge array with at most 255 distinct values
        (``mde_plan_expand_bytes``), or None when it does not apply."""
        lib = _lib.load()
        t = per_edge.detach().to(device=self.device, dtype=torch.float32).contiguous().reshape(-1)
        if t.numel() != self.p:
            return None
        size = int(lib.mde_plan_layout_half_edges(self._handle, 1))
        out = torch.empty(max(size, 1), dtype=torch.float32, device=self.device)
        nv = ctypes.c_int32(0)
        with torch.cuda.device(self.device):
            _lib.check(lib.mde_plan_expand_bytes(self._handle, _lib.ptr(t), _lib.ptr(out),
                                                 ctypes.byref(nv), _lib.stream_ptr(self.device)))
        return out if nv.value > 0 else None

    def ring_info(self):
        """The LDS-ring layout of the plan as a dict (``mde_plan_ring_info``, ``mde_plan_ring_loss_balance``); ``built``
        is False before the first evaluation at a dimension that takes it.  ``loss_band``: width in vertices of the bands
        between which the rule for who adds an edge's loss term flips (0: the smaller endpoint does); ``class_blocks``:
        blocks of four wave iterations in which no / every / some entries add their term; ``loss_share_min`` /
        ``loss_share_max``: smallest and largest fraction of a workgroup's entries that add their term."""
        lib = _lib.load()
        info = (ctypes.c_int64 * 16)()
        _lib.check(lib.mde_plan_ring_info(self._handle, info))
        names = ("built", "d", "rows_per_block", "row_blocks", "col_groups", "chunks", "ring_slots", "iterations",
                 "ring_half_edges", "padded_entries", "permuted", "hub_rows", "hub_half_edges", "hub_segments", "loss_band")
        out = {k: int(info[i]) for i, k in enumerate(names)}
        out["built"], out["permuted"] = bool(out["built"]), bool(out["permuted"])
        bal = (ctypes.c_double * 8)()
        _lib.check(lib.mde_plan_ring_loss_balance(self._handle, bal))
        out["class_blocks"] = tuple(int(bal[i]) for i in (1, 2, 3))
        out["loss_share_min"], out["loss_share_max"] = float(bal[4]), float(bal[5])
        return out

    def ring_check(self):
        """Device check of the LDS-ring layout (``mde_plan_ring_check``).  Lane-stable pairs: ``split`` entries whose
        row the other iteration of their pair holds on another lane (always 0), ``shared`` rows held by both
        iterations of a pair, ``pairs`` checked.  Loss terms (layouts whose rows are not permuted): ``loss_bad`` edges
        whose term is not added exactly once (always 0), ``loss_flag_bad`` entries whose flag in the packed word
        disagrees with the rule (always 0), ``loss_edges`` edges with both entries in this plan."""
        lib = _lib.load()
        out = (ctypes.c_int64 * 8)()
        with torch.cuda.device(self.device):
            _lib.check(lib.mde_plan_ring_check(self._handle, out, _lib.stream_ptr(self.device)))
        return {"split": int(out[0]), "shared": int(out[1]), "pairs": int(out[2]), "loss_bad": int(out[3]),
                "loss_flag_bad": int(out[4]), "loss_edges": int(out[5])}

    def row_order(self, mode=1):
        """Build (mode 1: keep if it helps, 2: keep regardless) or drop (0) the breadth-first processing order of the
        rows that the general-d kernel walks (``mde_plan_row_order``); returns a dict with ``in_use``, the mean distance
        between the positions of an edge's two ends before and after, and the number of levels.  Evaluations at
        d = 128 / 256 / 512 call it with mode 1 by themselves; results never depend on it."""
        lib = _lib.load()
        info = (ctypes.c_double * 4)()
        with torch.cuda.device(self.device):
            _lib.check(lib.mde_plan_row_order(self._handle, int(mode), _lib.stream_ptr(self.device), info))
        return {"in_use": bool(info[0]), "mean_distance_before": float(info[1]),
                "mean_distance_after": float(info[2]), "levels": int(info[3])}

    def csr(self):
        """(rowptr, nbr, eid) as int32 tensors (copies; for tests and debugging)."""
        lib = _lib.load()
        nloc = self.row_hi - self.row_lo
        rowptr = torch.empty(nloc + 1, dtype=torch.int32, device=self.device)
        nbr = torch.empty(max(self.half_edges, 1), dtype=torch.int32, device=self.device)
        eid = torch.empty(max(self.half_edges, 1), dtype=torch.int32, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(lib.mde_plan_export(self._handle, _lib.ptr(rowptr), _lib.ptr(nbr),
                                           _lib.ptr(eid), _lib.stream_ptr(self.device)))
        return rowptr, nbr[:self.half_edges], eid[:self.half_edges]

    def __del__(self):
        h = getattr(self, "_handle", None)
        if h is not None and h.value:
            try:
                _lib.load().mde_plan_destroy(h)
            except Exception:
                pass
            self._handle = None


class Binding(object):
    """A distortion function bound to an EdgePlan."""

    def __init__(self, plan, function):
        self.plan = plan
        self.function = function
        self.spec = function._hip_spec() if hasattr(function, "_hip_spec") else None
        self._struct = None
        self._keep = None
        self._key = None
        self.codebook = False
        self.byte_stream = False
        self.stream_kind = None

    @property
    def fused(self):
        return self.spec is not None

    def _param_key(self, spec):
        return tuple((a.data_ptr(), a._version, a.numel(), str(a.device)) for a in spec.arrays()) + (
            spec.kind, spec.kind_neg, spec.scalars, spec.scalars_neg)

    def struct(self, d):
        """The ``mde_func`` for the fused kernel at embedding dimension ``d`` (arrays in the
        layout the plan prefers for that d), rebuilt when the function's parameters change."""
        lib = _lib.load()
        spec = self.function._hip_spec()
        key = self._param_key(spec) + (int(d),)
        if self._struct is None or key != self._key:
            plan = self.plan
            with torch.cuda.device(plan.device):
                # (which function the layout decision is for: the close calls of mid-size problems depend on it)
                _lib.check(lib.mde_plan_function_hint(plan.handle, int(spec.kind), int(spec.kind_neg)))
                layout = lib.mde_plan_layout(plan.handle, int(d), _lib.stream_ptr(plan.device))
            if layout < 0:
                _lib.check(layout)

            def prep(a):
                if a is None:
                    return None
                if a.numel() == 1:
                    return a.detach().to(device=plan.device, dtype=torch.float32).reshape(1).contiguous()
                return plan.expand(a, layout)
            # few distinct first parameters (k-NN weights): 4-byte codebook stream instead of 8 bytes
            # (one or two values under a function whose coinciding entries add zero: the pair codebook, a0_scalar 4)
            a0, codebook_form = None, 0
            if layout == 1 and spec.a0 is not None and spec.a0.numel() > 1:
                a0, codebook_form = plan.expand_codebook(spec.a0, spec)
            self.codebook = a0 is not None
            # ... up to 255: one index byte per entry beside the packed words, 5 bytes (hop-count deviations)
            self.byte_stream = False
            if a0 is None and layout == 1 and spec.a0 is not None and spec.a0.numel() > 1:
                a0 = plan.expand_bytes(spec.a0)
                self.byte_stream = a0 is not None
            if a0 is None:
                a0 = prep(spec.a0)
            a1 = prep(spec.a1)
            # the per-edge arrays in the caller's edge order as well: hub rows the ring layout peels off to the CSR hub
            # kernel read their parameters through the plan's edge ids (mde_func.e0 / e1)
            def edge_order(a):
                if a is None or a.numel() == 1:
                    return None
                return a.detach().to(device=plan.device, dtype=torch.float32).contiguous().reshape(-1)
            e0, e1 = (edge_order(spec.a0), edge_order(spec.a1)) if layout == 1 else (None, None)
            self._keep = (a0, a1, e0, e1)
            self._struct = spec.to_struct(a0, a1)
            self._struct.e0 = e0.data_ptr() if e0 is not None else None
            self._struct.e1 = e1.data_ptr() if e1 is not None else None
            if self.codebook:
                self._struct.a0_scalar = codebook_form
            elif self.byte_stream:
                self._struct.a0_scalar = 3
            self.stream_kind = ("codebook" if self.codebook else "byte index" if self.byte_stream else
                                "scalar" if (spec.a0 is not None and spec.a0.numel() == 1) else "fp32")
            self._struct.layout = layout
            self._key = key
            self.spec = spec
        return self._struct


def fused_evaluate(binding, X, grad_out, loss_out, grad_scale=1.0):
    """Enqueue the fused kernel: writes the plan's rows of ``grad_out`` (may be None) and the
    plan's share of E(X) into ``loss_out`` (1-element float32 tensor)."""
    lib = _lib.load()
    plan = binding.plan
    f = binding.struct(X.shape[1])
    if X.data_ptr() & 15:
        X = X.clone()  # (a view into a larger tensor: the kernels read rows with 16-byte loads)
    with torch.cuda.device(plan.device):
        _lib.check(lib.mde_average_distortion(
            plan.handle, _lib.ptr(X), X.shape[1], ctypes.byref(f), float(grad_scale),
            _lib.ptr(grad_out), _lib.ptr(loss_out), _lib.stream_ptr(plan.device)))


class _AverageDistortion(torch.autograd.Function):
    """E(X) = mean_k f_k(||x_i - x_j||) [ref: average_distortion.py:62-106]."""

    @staticmethod
    def forward(ctx, X, binding):
        plan = binding.plan
        _check_X(X, plan.n)
        if not plan.is_full:
            raise ValueError("use pymde_amd.distributed for sharded plans")
        Xc = X.detach().contiguous()
        loss = torch.empty(1, dtype=torch.float32, device=X.device)
        need_grad = X.requires_grad
        if binding.fused:
            grad = torch.empty_like(Xc) if need_grad else None
            fused_evaluate(binding, Xc, grad, loss)
        else:
            grad, value = _unfused(binding, Xc, need_grad)
            loss = value.reshape(1)
        if need_grad:
            ctx.save_for_backward(grad)
        return loss.reshape(())

    @staticmethod
    def backward(ctx, grad_output):
        (grad,) = ctx.saved_tensors
        return grad * grad_output, None


def _unfused(binding, X, need_grad):
    """Arbitrary callable f: HIP distances -> torch autograd through f -> HIP scatter
    (the reference's own structure, average_distortion.py:68-105)."""
    lib = _lib.load()
    plan = binding.plan
    f = binding.function
    n, d = X.shape
    dist = torch.empty(plan.p, dtype=torch.float32, device=X.device)
    with torch.cuda.device(plan.device):
        _lib.check(lib.mde_distances(n, plan.p, _lib.ptr(plan.edges), _lib.ptr(X), d, _lib.ptr(dist),
                                     _lib.stream_ptr(plan.device)))
    if not need_grad:
        with torch.no_grad():
            return None, f(dist).mean().to(torch.float32)
    with torch.enable_grad():
        norms = dist.detach().requires_grad_(True)
        distortion = f(norms).mean()
        (gnorm,) = torch.autograd.grad(distortion, norms)
    gnorm = gnorm.to(torch.float32).contiguous()
    grad = torch.empty_like(X)
    with torch.cuda.device(plan.device):
        _lib.check(lib.mde_scatter(plan.handle, _lib.ptr(X), d, _lib.ptr(gnorm), _lib.ptr(dist), 1.0,
                                   _lib.ptr(grad), _lib.stream_ptr(plan.device)))
    return grad, distortion.detach().to(torch.float32)


def average_distortion(X, binding):
    return _AverageDistortion.apply(X, binding)


class _Norm(torch.autograd.Function):
    """Embedding distances per edge; backward x g / ||x|| with NaN -> 0
    [ref: average_distortion.py:38-55, problem.py:246-283]."""

    @staticmethod
    def forward(ctx, X, plan):
        _check_X(X, plan.n)
        lib = _lib.load()
        Xc = X.detach().contiguous()
        n, d = Xc.shape
        dist = torch.empty(plan.p, dtype=torch.float32, device=X.device)
        with torch.cuda.device(plan.device):
            _lib.check(lib.mde_distances(n, plan.p, _lib.ptr(plan.edges), _lib.ptr(Xc), d,
                                         _lib.ptr(dist), _lib.stream_ptr(plan.device)))
        ctx.plan = plan
        ctx.save_for_backward(Xc)
        return dist

    @staticmethod
    def backward(ctx, grad_output):
        (Xc,) = ctx.saved_tensors
        plan = ctx.plan
        lib = _lib.load()
        gout = grad_output.detach().to(torch.float32).contiguous()
        grad = torch.empty_like(Xc)
        with torch.cuda.device(plan.device):
            _lib.check(lib.mde_distances_backward(plan.handle, _lib.ptr(Xc), Xc.shape[1],
                                                  _lib.ptr(gout), _lib.ptr(grad),
                                                  _lib.stream_ptr(plan.device)))
        return grad, None


def distances(X, plan):
    return _Norm.apply(X, plan)


def differences(X, plan):
    """X[i] - X[j] for every edge (i, j), shape (p, d)."""
    _check_X(X, plan.n)
    lib = _lib.load()
    Xc = X.detach().contiguous()
    n, d = Xc.shape
    out = torch.empty((plan.p, d), dtype=torch.float32, device=X.device)
    with torch.cuda.device(plan.device):
        _lib.check(lib.mde_differences(n, plan.p, _lib.ptr(plan.edges), _lib.ptr(Xc), d,
                                       _lib.ptr(out), _lib.stream_ptr(plan.device)))
    return out


# ---------------------------------------------------------------- reference-signature shim
_PLAN_CACHE = {}


def _gather_indices(idx, m):
    """Kept for signature compatibility with the reference (average_distortion.py:58-59)."""
    return idx[:, None].expand(idx.shape[0], m)


def _average_distortion(X, f, lhs, rhs):
    """Drop-in for the reference's ``_average_distortion(X, f, lhs, rhs)`` seam
    (average_distortion.py:109): lhs/rhs are the (expanded) endpoint index tensors."""
    li = lhs[:, 0] if lhs.dim() == 2 else lhs
    ri = rhs[:, 0] if rhs.dim() == 2 else rhs
    # keyed on what the index tensors ARE (storage address, offset, strides, length, in-place
    # version), not on the Python objects: a caller that slices edges[:, 0] / edges[:, 1] afresh on
    # every call gets the same plan back.  The entry keeps the storages and f alive, so an address
    # cannot be reused while it is cached.
    def ident(t):
        return (t.untyped_storage().data_ptr(), t.storage_offset(), tuple(t.stride()), tuple(t.shape), t._version,
                str(t.dtype), str(t.device))
    key = (ident(lhs), ident(rhs), X.shape[0], str(X.device), id(f))
    hit = _PLAN_CACHE.get(key)
    if hit is not None and hit[3] is not f:
        hit = None
    if hit is None:
        edges = torch.stack([li, ri], dim=1).to(device=X.device, dtype=torch.int64).contiguous()
        binding = Binding(EdgePlan(X.shape[0], edges), f)
        if len(_PLAN_CACHE) > 8:
            _PLAN_CACHE.clear()
        hit = _PLAN_CACHE[key] = (binding, lhs.untyped_storage(), rhs.untyped_storage(), f)
    return _AverageDistortion.apply(X, hit[0])

"""Every distortion function, edge by edge, against float64 on each kernel that instantiates
mde_functions.h.  Needs an MI355X.

The probe graph is a matching: probe k joins vertices 2k and 2k + 1, X[2k] = 0 and X[2k + 1] = d_k e_axis,
and neither vertex has another edge.  So mde.distortions(X)[k] is f(d_k) and grad[2k, axis] = -(f'/d)_k d_k / p:
every probe's f and f'/d is read off on its own and judged by the rule of tests/_functions_reference.py
(hull of the float64 reference over d (1 +- 2^-22), the kernel tolerances LOSS_RTOL / GRAD_RTOL relative, an
absolute term only where the reference's own float32 formula cancels).  test_functions_reference_host.py shows
that the C oracle passes the same rule at the same probes, so a failure here is a finding about a kernel.
"""
import numpy as np
import pytest
import torch

import _functions_reference as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
CASES = R.cases()
IDS = [c.id for c in CASES]


def _function(c, a0, a1=None):
    """The pymde_amd function object of a case with per-edge parameters a0 / a1 (numpy float32)."""
    import pymde_amd
    pen, los = pymde_amd.penalties, pymde_amd.losses
    penalties = {
        "LINEAR": lambda w, s: pen.Linear(w), "QUADRATIC": lambda w, s: pen.Quadratic(w),
        "CUBIC": lambda w, s: pen.Cubic(w), "POWER": lambda w, s: pen.Power(w, s[0]),
        "HUBER": lambda w, s: pen.Huber(w, s[0]), "LOGISTIC": lambda w, s: pen.Logistic(w, s[0], s[1]),
        "SIGMOID": lambda w, s: pen.Sigmoid(w, s[0], s[1]), "HINGE": lambda w, s: pen.Hinge(w, s[0], s[1]),
        "LOG1P": lambda w, s: pen.Log1p(w, s[0]), "LOG": lambda w, s: pen.Log(w, s[0]),
        "INVPOWER": lambda w, s: pen.InvPower(w, s[0]), "LOGRATIO": lambda w, s: pen.LogRatio(w, s[0]),
        "DEADZONE_QUADRATIC": lambda w, s: pen._DeadzoneQuadratic(w, s[0]),
        "DEADZONE_CUBIC": lambda w, s: pen._DeadzoneCubic(w, s[0]),
        "CLIPPED_QUADRATIC": lambda w, s: pen._ClippedQuadratic(w, s[0]),
    }
    t0 = torch.tensor(a0, device=DEV)
    t1 = None if a1 is None else torch.tensor(a1, device=DEV)
    s, sn = c.scalars, c.scalars_neg
    if c.kind_neg != "NONE":
        return pen.PushAndPull(t0, lambda w: penalties[c.kind](w, s), lambda w: penalties[c.kind_neg](w, sn))
    if c.kind in penalties:
        return penalties[c.kind](t0, s)
    losses = {
        "L_QUADRATIC": lambda: los.Quadratic(t0), "L_WEIGHTED_QUADRATIC": lambda: los.WeightedQuadratic(t0, t1),
        "L_HUBER": lambda: los.Huber(t0, s[0]), "L_CUBIC": lambda: los.Cubic(t0),
        "L_POWER": lambda: los.Power(t0, s[0]), "L_WEIGHTED_POWER": lambda: los._WeightedPower(t0, s[0], t1),
        "L_ABSOLUTE": lambda: los.Absolute(t0), "L_LOGISTIC": lambda: los.Logistic(t0),
        "L_FRACTIONAL": lambda: los.Fractional(t0), "L_SOFT_FRACTIONAL": lambda: los.SoftFractional(t0, s[0]),
        "L_CLIPPED_QUADRATIC": lambda: los._ClippedQuadratic(t0, s[0]), "L_LOG1P": lambda: los._Log1p(t0, s[0]),
    }
    return losses[c.kind]()


def _evaluate(c, dim, edges, X, a0, a1):
    import pymde_amd
    mde = pymde_amd.MDE(X.shape[0], dim, torch.tensor(edges, device=DEV), _function(c, a0, a1))
    Xt = torch.tensor(X, device=DEV, requires_grad=True)
    E = mde.average_distortion(Xt)
    E.backward()
    return mde, float(E.detach()), Xt.grad.cpu().numpy()


def _check_probe_rows(c, grad, axis, p):
    """f'/d of every probe by the rule; the partner row is the negative to 2 ulp; the other coordinates are zero."""
    P = c.d.size
    b = R.bounds(c)["g"]
    g = c.g_from_grad(grad, axis, p)
    assert R.passes(g, b).all(), R.describe_failures(c, "f'/d", g, b)
    rows = grad[:2 * P]
    lo, hi = rows[0::2, axis], rows[1::2, axis]
    assert (np.abs(lo + hi) <= 2.0 * np.spacing(np.abs(lo))).all()
    assert not np.delete(rows, axis, axis=1).any()


def _check_loss(E, ref_f, bound):
    """|E - mean(ref)| <= mean of the per-edge bounds (which bounds the summed error) + 2^-19 mean|ref| (float32
    accumulation of up to 2^19 terms)."""
    print("loss %.9g reference %.9g allowed %.3g" % (E, ref_f.mean(), bound.mean() + 2.0 ** -19 * np.abs(ref_f).mean()))
    assert abs(E - ref_f.mean()) <= bound.mean() + 2.0 ** -19 * np.abs(ref_f).mean()


def _probes_only(c, dim):
    """Evaluate the case on its matching graph alone and check loss and gradient; returns the MDE."""
    axis = dim - 1
    edges, X = c.matching(dim, axis)
    mde, E, grad = _evaluate(c, dim, edges, X, c.a0, c.a1)
    bf = R.bounds(c)["f"]
    _check_loss(E, bf[0], R.per_edge_bound(bf))
    _check_probe_rows(c, grad, axis, c.d.size)
    return mde


def _native_loaded():
    assert "libmde_hip.so" in open("/proc/self/maps").read()


# ------------------------------------------------------------------------------------ 1. distortions()
@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_distortions_per_edge(c):
    """mde.distortions(X): the element-wise evaluator (mde_distortions, the run-time functor)."""
    import pymde_amd
    edges, X = c.matching(2, 1)
    f = _function(c, c.a0, c.a1)
    assert f._hip_spec() is not None                       # the device evaluator, not a torch expression
    mde = pymde_amd.MDE(X.shape[0], 2, torch.tensor(edges, device=DEV), f)
    got = mde.distortions(torch.tensor(X, device=DEV)).cpu().numpy()
    _native_loaded()
    assert got.dtype == np.float32 and got.shape == c.d.shape
    b = R.bounds(c)["f"]
    assert R.passes(got, b).all(), R.describe_failures(c, "f", got, b)


# ------------------------------------------------------------------------------------ 2. CSR kernels, d = 2 and 3
# MDE_PANEL=0 keeps the LDS-ring kernel away.  MDE_FLAT=0 is the row-per-group kernel (k_fused_small), MDE_FLAT=1 the
# edge-balanced one (k_fused_flat; also what an unset MDE_FLAT gives on a graph this sparse).  Quadratic, Log1p(1.5),
# the losses Quadratic / Absolute / Huber and the two PushAndPull pairs have compile-time functors here
# (dispatch_fused); every other case runs FnRuntime.
@pytest.mark.parametrize("c", CASES, ids=IDS)
@pytest.mark.parametrize("dim,flat", [(2, "0"), (3, "0"), (2, "1")])
def test_csr_kernels(monkeypatch, dim, flat, c):
    monkeypatch.setenv("MDE_PANEL", "0")
    monkeypatch.setenv("MDE_FLAT", flat)
    mde = _probes_only(c, dim)
    b = mde._binding()
    assert b.fused and b.struct(dim).layout == 0 and not b.codebook
    _native_loaded()


# ------------------------------------------------------------------------------------ 3. wide kernels, d = 8
# The probe axis is the last coordinate (the second float4 of a row).  Default: the pipelined k_fused_wide4p;
# MDE_WIDE_P=0: the 16-byte form of k_fused_wide.  Log1p(1.5) is FnSingle<LOG1P, 2> here, everything else FnRuntime.
@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_wide_kernel(monkeypatch, c):
    monkeypatch.delenv("MDE_WIDE_P", raising=False)
    mde = _probes_only(c, 8)
    assert mde._binding().fused and mde._binding().struct(8).layout == 0


@pytest.mark.parametrize("id", ["LOG1P-e1p5", "LOG-e0p7"])
def test_wide_kernel_without_the_pipeline(monkeypatch, id):
    monkeypatch.setenv("MDE_WIDE_P", "0")
    mde = _probes_only(R.case(id), 8)
    assert mde._binding().fused and mde._binding().struct(8).layout == 0


# ------------------------------------------------------------------------------------ 4. the LDS-ring kernel
# One case per functor of the mde_ring_k_*.hip units.
RING_IDS = [
    "LOG1P-e1p5", "LOG1P-e1", "LOG1P-e2", "LOG1P-e0p7",                      # mde_ring_k_log1p: classes 2, 1, 3, run-time
    "LOG-e1", "LOG-e2", "LINEAR", "QUADRATIC", "CUBIC", "HUBER",             # mde_ring_k_penalty (Log: classes 1 and 3)
    "POWER-e1p5", "POWER-e0p5", "POWER-e2p5", "INVPOWER-e1", "INVPOWER-e2p5",  # mde_ring_k_penalty2
    "LOGRATIO-e2", "LOGRATIO-e0p7", "LOGISTIC", "SIGMOID", "HINGE",
    "PUSHPULL-LOG1P-e1p5-LOG-e1", "PUSHPULL-LOG1P-e1p5-LOGRATIO-e2",         # mde_ring_k_pushpull
    "L_QUADRATIC", "L_WEIGHTED_QUADRATIC", "L_ABSOLUTE", "L_HUBER",          # mde_ring_k_loss
    "L_CUBIC", "L_POWER-e1p5", "L_LOGISTIC", "L_FRACTIONAL", "L_SOFT_FRACTIONAL",  # mde_ring_k_loss2
    "DEADZONE_QUADRATIC", "PUSHPULL-LOG1P-e2-LOG-e1p5",                      # mde_ring_k_runtime
]
# The layout builder takes the probes-only graph (layout 1 at d = 2 and 3), but the probes have two to four
# distinct parameter values, which is the codebook stream.  For the fp32 stream the probes go in front of a random
# background graph on vertices of its own, with continuous parameters; the smallest background tried, 1000
# vertices and 4000 edges, gives layout == 1 as well (so did 2000 / 20000, 8000 / 100000 and 30000 / 400000).
RING_BACKGROUND = (1000, 4000)


_BACKGROUND = {}


def _background(dim):
    """Random graph, positions and parameter draws of the background, made once per dimension."""
    if dim not in _BACKGROUND:
        n, p = RING_BACKGROUND
        rng = np.random.default_rng(500 + dim)
        i = rng.integers(0, n, p)
        j = (i + 1 + rng.integers(0, n - 1, p)) % n
        key = np.unique(np.minimum(i, j).astype(np.int64) * n + np.maximum(i, j))
        edges = np.stack([key // n, key % n], 1)
        X = (rng.standard_normal((n, dim)) * 1.5).astype(np.float32)
        diff = X[edges[:, 0]].astype(np.float64) - X[edges[:, 1]].astype(np.float64)
        _BACKGROUND[dim] = dict(edges=edges, X=X, dist=np.sqrt((diff ** 2).sum(1)), u=rng.random(len(edges)),
                                v=rng.random(len(edges)), negative=rng.random(len(edges)) < 0.3)
    return _BACKGROUND[dim]


@pytest.mark.parametrize("id", RING_IDS)
@pytest.mark.parametrize("dim", [2, 3])
def test_ring_kernel(monkeypatch, dim, id):
    """The fp32 parameter stream: probes in front of the background, whose parameters are continuous draws.  The
    probes are judged edge by edge; the background enters through the loss only (float64 on its float32 coordinates)."""
    monkeypatch.setenv("MDE_PANEL", "1")
    c, bg, axis = R.case(id), _background(dim), dim - 1
    pe, pX = c.matching(dim, axis)
    edges = np.concatenate([pe, bg["edges"] + 2 * c.d.size])
    X = np.concatenate([pX, bg["X"]])
    lo, hi = np.abs(c.a0).min() * 0.8, np.abs(c.a0).max() * 1.1           # weights 0.3 .. 1.65, deviations 0.2 .. 0.41
    b0 = (lo + (hi - lo) * bg["u"]).astype(np.float32)
    if (c.a0 < 0).all():
        b0 = -b0
    elif (c.a0 < 0).any():
        b0 = np.where(bg["negative"], -b0, b0)
    b1 = None if c.a1 is None else (0.3 + 1.3 * bg["v"]).astype(np.float32)
    a0 = np.concatenate([c.a0, b0])
    a1 = None if c.a1 is None else np.concatenate([c.a1, b1])
    mde, E, grad = _evaluate(c, dim, edges, X, a0, a1)
    b = mde._binding()
    assert b.fused and b.struct(dim).layout == 1 and b.stream_kind == "fp32", (b.stream_kind, mde._plan.ring_info())
    _check_probe_rows(c, grad, axis, len(edges))
    bf, bb = R.bounds(c)["f"], R.bounds_at(c, bg["dist"], b0, b1)["f"]
    _check_loss(E, np.concatenate([bf[0], bb[0]]), np.concatenate([R.per_edge_bound(bf), R.per_edge_bound(bb)]))


W = R.WEIGHTS
CODEBOOK_CASES = [R.case("LOG1P-e1p5"),                                    # two values
                  R.merged_pushpull("PUSHPULL-LOG1P-e1p5-LOG-e1-w++-", (W[0], W[1], -W[0])),   # three values each; between
                  R.merged_pushpull("PUSHPULL-LOG1P-e1p5-LOG-e1-w+--", (W[0], -W[0], -W[1]))]  # them, both weights of both signs


@pytest.mark.parametrize("c", CODEBOOK_CASES, ids=[c.id for c in CODEBOOK_CASES])
@pytest.mark.parametrize("dim", [2, 3])
def test_ring_kernel_codebook_stream(monkeypatch, dim, c):
    """At most three distinct parameter values (the probes-only graph): the codebook stream, where the kFiniteG
    functors -- Log1p(1.5) and the merged PushAndPull -- skip the NaN / Inf fix-up of f'/d."""
    monkeypatch.setenv("MDE_PANEL", "1")
    assert np.unique(c.a0).size <= 3
    mde = _probes_only(c, dim)
    b = mde._binding()
    assert b.fused and b.struct(dim).layout == 1 and b.codebook and b.stream_kind == "codebook"


# ------------------------------------------------------------------------------------ 5. f of the fused kernels, one edge at a time
# The fused kernels return f only inside the mean, where an error on one short edge vanishes, and distortions() runs
# the run-time functor.  Log1p(1.5) and the merged PushAndPull spell their own f (the CSR functors in mde_functions.h,
# Log1p(1.5) once more inside the ring kernel): with every weight but one set to zero the other edges add exact
# zeros, so p E is that one edge's f.
@pytest.mark.parametrize("id", ["LOG1P-e1p5", "PUSHPULL-LOG1P-e1p5-LOG-e1", "PUSHPULL-LOG1P-e1p5-LOGRATIO-e2"])
@pytest.mark.parametrize("panel", ["0", "1"])
def test_fused_f_one_edge_at_a_time(monkeypatch, panel, id):
    """Every fourth probe of the global sweep and k = 0, 1, 8, 16, 23 of the local ones, per weight; d = 2, the
    row-per-group CSR kernel (MDE_PANEL=0) and the ring kernel (MDE_PANEL=1, codebook stream: two values)."""
    import pymde_amd
    monkeypatch.setenv("MDE_PANEL", panel)
    monkeypatch.setenv("MDE_FLAT", "0")
    c = R.case(id)
    edges, X = c.matching(2, 1)
    thin = ((c.local_k == 0) & (c.sweep_k % 4 == 0)) | np.isin(np.abs(c.local_k), (1, 8, 16, 23)) | c.at_special
    mde = pymde_amd.MDE(X.shape[0], 2, torch.tensor(edges, device=DEV), _function(c, c.a0))
    f = mde.distortion_function            # (the MDE's own: it copies a function whose buffers sit on two devices)
    Xt = torch.tensor(X, device=DEV)
    bf = R.bounds(c)["f"]
    got = bf[0].copy()
    for k in np.flatnonzero(thin):
        f.weights.zero_()
        f.weights[k] = float(c.a0[k])
        got[k] = float(mde.average_distortion(Xt)) * c.d.size
    b = mde._binding()
    assert b.fused and b.struct(2).layout == int(panel) and b.codebook == (panel == "1")
    assert thin.sum() >= 64 and R.passes(got, bf).all(), R.describe_failures(c, "f", got, bf)

"""A float64 reference of every distortion function, a generator of probe distances and the rule
that decides whether a float32 value is acceptable.  Shared by test_functions_reference_host.py
(no GPU) and test_gpu_function_sweeps.py.  Needs numpy only (mpmath for `f_mp`).

The reference is written from the definitions in the docstrings of the reference's
`pymde/functions/penalties.py` and `losses.py`, in forms without cancellation (log1p, expm1,
logaddexp), with the reference's conventions: sign(0) = 0, a tie of max / min splits the
sub-gradient 1/2, Huber switches at a strict `<`, pow(x, 0) has zero gradient.  It restates neither
the device code nor the C oracle.

Parameters and scalars are float32 values (what the kernels receive), held in float64.
"""
import functools

import numpy as np

from conftest import GRAD_RTOL, LOSS_RTOL

# ------------------------------------------------------------------------------------ arithmetic
# One body of formulas, two arithmetics: float64 arrays (numpy) and mpmath numbers (the derivative
# check of the host test).  `where` evaluates both branches in either.


class _NP(object):
    log, log1p, exp, expm1, abs, sign = np.log, np.log1p, np.exp, np.expm1, np.abs, np.sign
    power, where, maximum = np.power, np.where, np.maximum
    log2 = float(np.log(2.0))


def _mp_arith():
    import mpmath

    class _MP(object):
        log, log1p, exp, expm1, abs, sign = (mpmath.log, mpmath.log1p, mpmath.exp, mpmath.expm1,
                                             abs, mpmath.sign)
        power = mpmath.power
        log2 = mpmath.log(2)

        @staticmethod
        def where(c, a, b):
            return a if c else b

        @staticmethod
        def maximum(a, b):
            return a if a >= b else b
    return _MP


def _pow(M, x, e):
    """x^e; an integer-valued e is repeated multiplication (so a negative x is fine), 0 -> 1."""
    if e == 0.0:
        return x * 0 + 1
    if e == int(e):
        return x ** int(e)
    return M.power(x, e)


def _dpow(M, x, e):
    """d/dx x^e = e x^(e-1), defined as 0 for e = 0 (torch.pow's backward)."""
    if e == 0.0:
        return x * 0
    return e * _pow(M, x, e - 1.0)


def _softplus(M, z):
    return M.maximum(z, z * 0) + M.log1p(M.exp(-M.abs(z)))


def _sigmoid(M, z):
    t = M.exp(-M.abs(z))
    return M.where(z >= 0, 1 / (1 + t), t / (1 + t))


def _eval_kind(M, kind, d, a0, a1, s):
    """(f(d), f'(d)) of one kind; a0 = weight (penalties) or deviation (losses), a1 = the weight of
    the weighted losses, s = the kind's scalars."""
    s = tuple(s) + (0.0, 0.0, 0.0)
    s0, s1 = s[0], s[1]
    zero = d * 0
    # ------------------------------------------------------------ penalties  f = w p(d)
    if kind == "LINEAR":                       # p = d
        return a0 * d, a0 + zero
    if kind == "QUADRATIC":                    # p = d^2
        return a0 * d * d, 2 * a0 * d
    if kind == "CUBIC":                        # p = d^3
        return a0 * d * d * d, 3 * a0 * d * d
    if kind == "POWER":                        # p = d^e
        return a0 * _pow(M, d, s0), a0 * _dpow(M, d, s0)
    if kind == "HUBER":                        # p = d^2 / 2 below the threshold, t (d - t / 2) from it on
        lt = d < s0
        return (M.where(lt, a0 * d * d / 2, a0 * s0 * (d - s0 / 2)),
                M.where(lt, a0 * d, a0 * s0 + zero))
    if kind == "LOGISTIC":                     # p = log(1 + exp(alpha (d - threshold)))
        z = s1 * (d - s0)
        return a0 * _softplus(M, z), a0 * s1 * _sigmoid(M, z)
    if kind == "SIGMOID":                      # p = sigmoid(alpha (d - threshold));  1 - sigmoid(z) = sigmoid(-z)
        z = s1 * (d - s0)
        return a0 * _sigmoid(M, z), a0 * s1 * _sigmoid(M, z) * _sigmoid(M, -z)
    if kind == "HINGE":                        # f = max(0, w (d - (threshold - sign(w) sigma)))
        v = a0 * (d - (s0 - M.sign(a0) * s1))
        return (M.where(v > 0, v, zero),
                M.where(v > 0, a0 + zero, M.where(v == 0, a0 / 2 + zero, zero)))
    if kind == "LOG1P":                        # p = log(1 + d^e)
        pe = _pow(M, d, s0)
        return a0 * M.log1p(pe), a0 * _dpow(M, d, s0) / (1 + pe)
    if kind == "LOG":                          # p = log(1 - exp(-d^e))
        u = _pow(M, d, s0)
        p = M.where(u > M.log2, M.log1p(-M.exp(-u)), M.log(-M.expm1(-u)))
        return a0 * p, a0 * _dpow(M, d, s0) * M.exp(-u) / (-M.expm1(-u))
    if kind == "INVPOWER":                     # f = |w| / d^e
        pe = _pow(M, d, s0)
        return M.abs(a0) / pe, -M.abs(a0) * s0 / (pe * d)
    if kind == "LOGRATIO":                     # p = log(d^e / (1 + d^e)) = -log(1 + d^-e)
        pe = _pow(M, d, s0)
        return -a0 * M.log1p(1 / pe), a0 * s0 / (d * (1 + pe))
    if kind == "DEADZONE_QUADRATIC":           # 0 below the threshold, d^2 from it on
        lt = d < s0
        return M.where(lt, zero, a0 * d * d), M.where(lt, zero, 2 * a0 * d)
    if kind == "DEADZONE_CUBIC":
        lt = d < s0
        return M.where(lt, zero, a0 * d * d * d), M.where(lt, zero, 3 * a0 * d * d)
    if kind == "CLIPPED_QUADRATIC":            # p = min(d^2, (threshold + 1)^2)
        q, c = d * d, (s0 + 1) * (s0 + 1)
        return (a0 * M.where(q < c, q, c + zero),
                M.where(q < c, 2 * a0 * d, M.where(q == c, a0 * d, zero)))
    # ------------------------------------------------------------ losses  f = l(d, delta)
    r = d - a0
    ar, sg = M.abs(r), M.sign(r)
    if kind == "L_QUADRATIC":                  # (d - delta)^2
        return r * r, 2 * r
    if kind == "L_WEIGHTED_QUADRATIC":         # w (d - delta)^2
        return a1 * r * r, 2 * a1 * r
    if kind == "L_CLIPPED_QUADRATIC":          # min((d - delta)^2, (threshold + 1)^2)
        q, c = r * r, (s0 + 1) * (s0 + 1)
        return (M.where(q < c, q, c + zero),
                M.where(q < c, 2 * r, M.where(q == c, r, zero)))
    if kind == "L_HUBER":                      # |r|^2 below the threshold, t (2 |r| - t) from it on
        lt = ar < s0
        return (M.where(lt, r * r, s0 * (2 * ar - s0)),
                M.where(lt, 2 * r, 2 * s0 * sg))
    if kind == "L_CUBIC":                      # |d - delta|^3
        return ar * ar * ar, 3 * r * r * sg
    if kind == "L_POWER":                      # |d - delta|^e
        return _pow(M, ar, s0), _dpow(M, ar, s0) * sg
    if kind == "L_WEIGHTED_POWER":
        return a1 * _pow(M, ar, s0), a1 * _dpow(M, ar, s0) * sg
    if kind == "L_ABSOLUTE":
        return ar, sg + zero
    if kind == "L_LOGISTIC":                   # log(1 + exp(|d - delta|))
        return _softplus(M, ar), _sigmoid(M, ar) * sg
    if kind == "L_FRACTIONAL":                 # max(delta / d, d / delta) - 1
        g1, g2 = -a0 / (d * d), 1 / a0 + zero
        return (M.where(r > 0, r / a0, -r / d),
                M.where(r > 0, g2, M.where(r < 0, g1, (g1 + g2) / 2)))
    if kind == "L_SOFT_FRACTIONAL":            # (1/gamma) log((exp(gamma delta/d) + exp(gamma d/delta)) / (2 exp(gamma)))
        q1, q2 = s0 * a0 / d, s0 * d / a0
        lse = M.maximum(q1, q2) + M.log1p(M.exp(-M.abs(q1 - q2)))     # logaddexp(q1, q2)
        return ((lse - (M.log2 + s0)) / s0,
                _sigmoid(M, q1 - q2) * (-a0 / (d * d)) + _sigmoid(M, q2 - q1) / a0)
    if kind == "L_LOG1P":                      # log(1 + (d - delta)^e), e an integer
        pe = _pow(M, r, s0)
        return M.log1p(pe), _dpow(M, r, s0) / (1 + pe)
    raise KeyError(kind)


KINDS = ("LINEAR", "QUADRATIC", "CUBIC", "POWER", "HUBER", "LOGISTIC", "SIGMOID", "HINGE", "LOG1P", "LOG",
         "INVPOWER", "LOGRATIO", "DEADZONE_QUADRATIC", "DEADZONE_CUBIC", "CLIPPED_QUADRATIC", "L_QUADRATIC",
         "L_WEIGHTED_QUADRATIC", "L_HUBER", "L_CUBIC", "L_POWER", "L_WEIGHTED_POWER", "L_ABSOLUTE", "L_LOGISTIC",
         "L_FRACTIONAL", "L_SOFT_FRACTIONAL", "L_CLIPPED_QUADRATIC", "L_LOG1P")
WEIGHTED = ("L_WEIGHTED_QUADRATIC", "L_WEIGHTED_POWER")


def _branch(a0):
    """PushAndPull: True where the weight is attractive (zero counts as attractive)."""
    return np.asarray(a0) >= 0


def ref(kind, d, a0, a1=None, scalars=(), kind_neg=None, scalars_neg=()):
    """(f, f'/d) in float64 at the distances d (any float array) for per-edge parameters a0 / a1.
    With `kind_neg` the function is PushAndPull(kind, kind_neg), chosen by the sign of a0."""
    d = np.asarray(d, dtype=np.float64)
    a0 = np.broadcast_to(np.asarray(a0, dtype=np.float64), d.shape)
    a1 = None if a1 is None else np.broadcast_to(np.asarray(a1, dtype=np.float64), d.shape)
    with np.errstate(all="ignore"):
        f, fp = _eval_kind(_NP, kind, d, a0, a1, scalars)
        if kind_neg not in (None, "NONE"):
            fn, fpn = _eval_kind(_NP, kind_neg, d, a0, a1, scalars_neg)
            att = _branch(a0)
            f, fp = np.where(att, f, fn), np.where(att, fp, fpn)
        return f + 0.0 * d, fp / d


def f_mp(kind, d, a0, a1=None, scalars=(), kind_neg=None, scalars_neg=()):
    """f at ONE distance in mpmath's current precision (d may be an mpf; parameters are floats)."""
    import mpmath
    M = _mp_arith()
    if kind_neg not in (None, "NONE") and not a0 >= 0:
        kind, scalars = kind_neg, scalars_neg
    a1 = None if a1 is None else mpmath.mpf(float(a1))
    return _eval_kind(M, kind, mpmath.mpf(d), mpmath.mpf(float(a0)), a1, tuple(float(x) for x in scalars))[0]


# ------------------------------------------------------------------------------------ probes
def _f32(x):
    return float(np.float32(x))


EXPONENTS = tuple(_f32(e) for e in (1.0, 1.5, 2.0, 3.0, 0.5, 2.5, 0.7))   # classes 1, 2, 3, 4, 5 and two run-time values
WEIGHTS = (_f32(1.5), _f32(0.37))
DEVIATIONS = (_f32(0.25), _f32(0.37))
_EXPONENT_KINDS = ("POWER", "LOG1P", "LOG", "INVPOWER", "LOGRATIO", "L_POWER", "L_WEIGHTED_POWER", "L_LOG1P")
# scalars of the kinds without an exponent: Logistic, Sigmoid, Hinge and SoftFractional as the ring-kernel test of
# every public function has them; thresholds of the rest chosen so that both delta - t and delta + t are distances
SCALARS = {
    "HUBER": (0.5,), "LOGISTIC": (0.5, 3.0), "SIGMOID": (1.0, 2.0), "HINGE": (1.0, 0.5),
    "DEADZONE_QUADRATIC": (0.75,), "DEADZONE_CUBIC": (0.75,), "CLIPPED_QUADRATIC": (0.5,),
    "L_HUBER": (0.125,), "L_SOFT_FRACTIONAL": (10.0,), "L_CLIPPED_QUADRATIC": (-0.875,),
}


def global_sweep():
    """2^(k/4), k = -80 .. 48: 2^-20 .. 4096 in 129 float32 values."""
    return (2.0 ** (GLOBAL_K / 4.0)).astype(np.float32)


def local_sweep(c):
    """c and c (1 +- 2^-k), k = 1 .. 23, as float32 values."""
    k = LOCAL_K.astype(np.float64)
    return (c * (1.0 + np.sign(k) * 2.0 ** -np.abs(k))).astype(np.float32)


GLOBAL_K = np.arange(-80, 49)
LOCAL_K = np.concatenate([[0], -np.arange(1, 24), np.arange(1, 24)])    # 0: the point itself


def special_points(kind, scalars, a0):
    """The distances around which one kind is probed closely: the deviation of a loss, thresholds, and the points at
    which the device code switches between two forms of the same function."""
    s = tuple(scalars) + (0.0, 0.0)
    pts = []
    if kind.startswith("L_"):
        pts.append(a0)
    if kind in ("HUBER", "LOGISTIC", "SIGMOID", "DEADZONE_QUADRATIC", "DEADZONE_CUBIC"):
        pts.append(s[0])
    if kind == "HINGE":                       # the threshold and the kink of either sign of the weight
        pts += [s[0], s[0] - s[1], s[0] + s[1]]
    if kind == "CLIPPED_QUADRATIC":
        pts.append(s[0] + 1.0)
    if kind == "L_HUBER":
        pts += [a0 - s[0], a0 + s[0]]
    if kind == "L_CLIPPED_QUADRATIC":
        pts += [a0 - (s[0] + 1.0), a0 + (s[0] + 1.0)]
    if kind == "LOG":                         # series / direct 1 - exp(-u) at u = 1/16; log1p(-em) / log(A) at u = 1
        pts += [0.0625 ** (1.0 / s[0]), 1.0]
    return [p for p in pts if p > 0]


class Case(object):
    """One problem: a function (kind, scalars, maybe a repulsive kind) and per-probe arrays d, a0, a1 (float32).
    `at_special` marks the probes that sit on a special point itself (kinks and jumps); `sweep_k` is the k of a
    probe of the global sweep and `local_k` the signed k of a probe of a local sweep (0 elsewhere)."""

    def __init__(self, id, kind, scalars, a0_values, a1_values=(None,), kind_neg="NONE", scalars_neg=(), extra=()):
        self.id, self.kind, self.kind_neg = id, kind, kind_neg
        self.scalars = tuple(_f32(x) for x in scalars)
        self.scalars_neg = tuple(_f32(x) for x in scalars_neg)
        ds, a0s, a1s, sp, gk, lk = [], [], [], [], [], []
        for v0 in a0_values:
            for v1 in a1_values:
                k, sc = (kind, self.scalars) if (kind_neg == "NONE" or v0 >= 0) else (kind_neg, self.scalars_neg)
                pts = [_f32(c) for c in special_points(k, sc, v0) + list(extra)]
                d = np.concatenate([global_sweep()] + [local_sweep(c) for c in pts])
                at = np.isin(d, np.array(pts, dtype=np.float32))
                g = np.concatenate([GLOBAL_K] + [np.zeros(LOCAL_K.size, dtype=np.int64)] * len(pts))
                l = np.concatenate([np.zeros(GLOBAL_K.size, dtype=np.int64)] + [LOCAL_K] * len(pts))
                keep = np.ones(d.size, dtype=bool)
                if k in ("L_POWER", "L_WEIGHTED_POWER") and sc[0] < 1.0:
                    # e < 1 at d = delta: e 0^(e-1) sign(0) = inf x 0, no derivative in the reference either
                    keep = d != np.float32(v0)
                d, at, g, l = d[keep], at[keep], g[keep], l[keep]
                ds.append(d)
                sp.append(at)
                gk.append(g)
                lk.append(l)
                a0s.append(np.full(d.size, v0, dtype=np.float32))
                a1s.append(None if v1 is None else np.full(d.size, v1, dtype=np.float32))
        self.d = np.concatenate(ds)
        self.at_special = np.concatenate(sp)
        self.sweep_k, self.local_k = np.concatenate(gk), np.concatenate(lk)
        self.a0 = np.concatenate(a0s)
        self.a1 = None if a1s[0] is None else np.concatenate(a1s)
        assert self.d.dtype == np.float32 and (self.d > 0).all()

    def __repr__(self):
        return self.id

    def ref(self, d=None, a0=None, a1=None):
        return ref(self.kind, self.d if d is None else d, self.a0 if a0 is None else a0,
                   self.a1 if a1 is None else a1, self.scalars, self.kind_neg, self.scalars_neg)

    def branch_kind(self, a0=None):
        """The kind that evaluates each probe (PushAndPull: by the sign of the weight)."""
        a0 = self.a0 if a0 is None else a0
        if self.kind_neg == "NONE":
            return np.full(np.shape(a0), self.kind, dtype=object)
        return np.where(_branch(a0), self.kind, self.kind_neg).astype(object)

    def oracle_func(self):
        from oracle import oracle
        return oracle.func(self.kind, self.a0, self.a1, self.scalars, self.kind_neg, self.scalars_neg)


    def matching(self, dim, axis):
        """The probe graph: probe k joins vertices 2k and 2k + 1, X[2k] = 0 and X[2k + 1] = d_k e_axis."""
        P = self.d.size
        edges = np.stack([2 * np.arange(P), 2 * np.arange(P) + 1], 1).astype(np.int64)
        X = np.zeros((2 * P, dim), dtype=np.float32)
        X[1::2, axis] = self.d
        return edges, X

    def g_from_grad(self, grad, axis, p):
        """f'/d per probe from the gradient of the average over p edges: grad[2k, axis] = -(f'/d)_k d_k / p."""
        P = self.d.size
        return -np.asarray(grad, dtype=np.float64)[0:2 * P:2, axis] * float(p) / self.d.astype(np.float64)


def _tag(e):
    return ("%g" % e).replace(".", "p")


def merged_pushpull(id, weights):
    """PushAndPull(Log1p 1.5, Log 1), the pair with one merged instruction stream: it switches its series at d = 1/16
    and its log1p correction at d = 1."""
    return Case(id, "LOG1P", (1.5,), weights, kind_neg="LOG", scalars_neg=(1.0,), extra=(0.0625, 1.0))


@functools.lru_cache(maxsize=None)
def cases():
    """Every (kind, exponent) problem of the sweep, PushAndPull last.  The parameters are per edge, so the sweeps of
    both values of every parameter (weights 1.5 and 0.37, deviations 0.25 and 0.37) share one problem."""
    out = []
    for kind in KINDS:
        a0 = DEVIATIONS if kind.startswith("L_") else WEIGHTS
        if kind == "INVPOWER":       # |w| / d^e: the constructor takes negative weights only
            a0 = tuple(-w for w in WEIGHTS)
        a1 = WEIGHTS if kind in WEIGHTED else (None,)
        if kind == "L_LOG1P":        # exponents 2 and 3, delta = 0.25: 1 + r^e >= 1 - 0.25^3 stays above 0.98
            out += [Case("L_LOG1P-e%s" % _tag(e), kind, (e,), (DEVIATIONS[0],)) for e in (2.0, 3.0)]
        elif kind in _EXPONENT_KINDS:
            out += [Case("%s-e%s" % (kind, _tag(e)), kind, (e,), a0, a1) for e in EXPONENTS]
        else:
            out.append(Case(kind, kind, SCALARS.get(kind, ()), a0, a1))
    both = WEIGHTS + tuple(-w for w in WEIGHTS)
    out.append(merged_pushpull("PUSHPULL-LOG1P-e1p5-LOG-e1", both))
    out.append(Case("PUSHPULL-LOG1P-e1p5-LOGRATIO-e2", "LOG1P", (1.5,), both, kind_neg="LOGRATIO", scalars_neg=(2.0,)))
    out.append(Case("PUSHPULL-LOG1P-e2-LOG-e1p5", "LOG1P", (2.0,), both, kind_neg="LOG", scalars_neg=(1.5,)))  # unmerged
    for c in out:
        for arr in bounds(c)["raw"]:
            assert np.isfinite(arr).all() and (np.abs(arr) <= FLT_MAX).all(), c.id   # no dropped probes
    return tuple(out)


def case(id):
    return {c.id: c for c in cases()}[id]


# ------------------------------------------------------------------------------------ acceptance
U = 2.0 ** -22           # two float32 ulps of d: ss = fl(d d) and a square root good to one ulp
FLOOR = 2.0 ** -100      # flushed denormals
EPS = 2.0 ** -24
A_UNITS = 8.0            # the absolute term is A_UNITS x EPS x S
FLT_MAX = float(np.finfo(np.float32).max)


def _ratio(d, a0):
    return np.maximum(a0 / d, d / a0)


# S of the absolute term A = 8 x 2^-24 x S, per kind and output; None: A = 0.  It applies where the reference's own
# float32 formula subtracts O(1) quantities: log(1 - exp(-u)) and log(pe / (1 + pe)) near 0, log(1 + r^e), q - 1 and
# logsumexp - (log 2 + gamma), and the 1 - sigmoid of the Sigmoid's derivative.
# The two numbers are what the C oracle needs beyond RTOL |R| + hull, in units of 2^-24 S, as measured by
# test_functions_reference_host.py::test_oracle_passes_the_rule (0 where A = 0: it passes without).
#   kind: (S for f, S for f'/d, the oracle's need for f, for f'/d)
S_TABLE = {
    "LINEAR": (None, None, 0.0, 0.0),
    "QUADRATIC": (None, None, 0.0, 0.0),
    "CUBIC": (None, None, 0.0, 0.0),
    "POWER": (None, None, 0.0, 0.0),
    "HUBER": (None, None, 0.0, 0.0),
    "LOGISTIC": (None, None, 0.0, 0.0),
    "SIGMOID": (None, lambda d, a0, a1, s: np.abs(a0 * s[1]) / d, 0.0, 0.68),
    "HINGE": (None, None, 0.0, 0.0),
    "LOG1P": (None, None, 0.0, 0.0),
    "LOG": (lambda d, a0, a1, s: np.abs(a0), None, 0.47, 0.0),
    "INVPOWER": (None, None, 0.0, 0.0),
    "LOGRATIO": (lambda d, a0, a1, s: np.abs(a0), None, 1.23, 0.0),
    "DEADZONE_QUADRATIC": (None, None, 0.0, 0.0),
    "DEADZONE_CUBIC": (None, None, 0.0, 0.0),
    "CLIPPED_QUADRATIC": (None, None, 0.0, 0.0),
    "L_QUADRATIC": (None, None, 0.0, 0.0),
    "L_WEIGHTED_QUADRATIC": (None, None, 0.0, 0.0),
    "L_HUBER": (None, None, 0.0, 0.0),
    "L_CUBIC": (None, None, 0.0, 0.0),
    "L_POWER": (None, None, 0.0, 0.0),
    "L_WEIGHTED_POWER": (None, None, 0.0, 0.0),
    "L_ABSOLUTE": (None, None, 0.0, 0.0),
    "L_LOGISTIC": (None, None, 0.0, 0.0),
    "L_FRACTIONAL": (lambda d, a0, a1, s: _ratio(d, a0), None, 0.0, 0.0),
    "L_SOFT_FRACTIONAL": (lambda d, a0, a1, s: 1.0 + _ratio(d, a0), None, 0.81, 0.0),
    "L_CLIPPED_QUADRATIC": (None, None, 0.0, 0.0),
    "L_LOG1P": (lambda d, a0, a1, s: np.ones_like(d), None, 1.00, 0.0),
}
assert set(S_TABLE) == set(KINDS)


def scale_S(c, out, d=None, a0=None, a1=None):
    """S per probe for output `out` (0: f, 1: f'/d); 0 where the kind has no absolute term."""
    d = np.asarray(c.d if d is None else d, dtype=np.float64)
    a0 = np.asarray(c.a0 if a0 is None else a0, dtype=np.float64)
    a1 = c.a1 if a1 is None else a1
    S = np.zeros(d.shape)
    kinds = c.branch_kind(a0)
    for kind, sc in ((c.kind, c.scalars), (c.kind_neg, c.scalars_neg)):
        fn = S_TABLE[kind][out] if kind != "NONE" else None
        if fn is not None:
            S = np.where(kinds == kind, fn(d, a0, a1, sc + (0.0, 0.0)), S)
    return S


def bounds_at(c, d, a0, a1=None):
    """The rule at arbitrary float32 distances / parameters of the function of case `c`: a dict with, per output
    ("f", "g" = f'/d), the tuple (R(d), lo, hi, tol, S): a value v passes when lo - tol <= v <= hi + tol.  [lo, hi] is
    the hull of R at d (1 - U), d, d (1 + U); tol = RTOL |R(d)| + 8 x 2^-24 x S + 2^-100."""
    d = np.asarray(d, dtype=np.float64)
    three = [c.ref(x, a0, a1) for x in (d * (1.0 - U), d, d * (1.0 + U))]
    out = {"raw": [t[k] for t in three for k in (0, 1)]}
    for k, (name, rtol) in enumerate((("f", LOSS_RTOL), ("g", GRAD_RTOL))):
        vals = np.stack([t[k] for t in three])
        S = scale_S(c, k, d, a0, a1)
        out[name] = (vals[1], vals.min(0), vals.max(0), rtol * np.abs(vals[1]) + A_UNITS * EPS * S + FLOOR, S)
    return out


_BOUNDS = {}


def bounds(c):
    """bounds_at for the case's own probes, computed once."""
    if c.id not in _BOUNDS:
        _BOUNDS[c.id] = bounds_at(c, c.d, c.a0, c.a1)
    return _BOUNDS[c.id]


def passes(got, b):
    """Boolean per probe: got within [lo - tol, hi + tol] (b = one output of bounds())."""
    R, lo, hi, tol, _ = b
    got = np.asarray(got, dtype=np.float64)
    return (got >= lo - tol) & (got <= hi + tol)


def per_edge_bound(b):
    """How far a passing value can be from R(d): the hull's reach plus tol."""
    R, lo, hi, tol, _ = b
    return np.maximum(hi - R, R - lo) + tol


def need(got, b, rtol):
    """What `got` needs beyond RTOL |R| + hull + 2^-100, in units of 2^-24 S (inf where S = 0 and it needs any)."""
    R, lo, hi, tol, S = b
    got = np.asarray(got, dtype=np.float64)
    base = rtol * np.abs(R) + FLOOR
    excess = np.maximum(np.maximum(lo - base - got, got - hi - base), 0.0)
    excess = np.where(np.isnan(got), np.inf, excess)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(excess > 0, excess / (EPS * S), 0.0)


def describe_failures(c, name, got, b, limit=8):
    """A few failing probes as text: distance, parameters, value, reference, hull and tolerance."""
    R, lo, hi, tol, _ = b
    got = np.asarray(got, dtype=np.float64)
    bad = np.flatnonzero(~passes(got, b))
    rel = np.abs(got[bad] - R[bad]) / np.maximum(np.abs(R[bad]), 1e-300)
    lines = ["%s %s: %d of %d probes fail" % (c.id, name, bad.size, got.size)]
    for i in bad[np.argsort(-rel)][:limit]:
        lines.append("  d=%.9g a0=%.9g got=%.9g ref=%.9g hull=[%.9g, %.9g] tol=%.3g" %
                     (c.d[i], c.a0[i], got[i], R[i], lo[i], hi[i], tol[i]))
    return "\n".join(lines)

"""The float64 reference of tests/_functions_reference.py checked without a GPU: against the
reference's golden distortions, its derivative against a 50-digit central difference of its own f,
and the C oracle (float32 libm) against the acceptance rule -- so that a probe that fails on the
device and passes here is a finding about the kernel, not about the rule."""
import functools

import numpy as np
import pytest

import _functions_reference as R
from conftest import GRAD_RTOL, LOSS_RTOL
from oracle import oracle

CASES = R.cases()
IDS = [c.id for c in CASES]


def test_probe_generator_covers_every_kind_and_exponent_class():
    assert {c.kind for c in CASES if c.kind_neg == "NONE"} == set(R.KINDS) and len(R.KINDS) == 27
    for kind in ("POWER", "LOG1P", "LOG", "INVPOWER", "LOGRATIO", "L_POWER", "L_WEIGHTED_POWER"):
        assert sorted(c.scalars[0] for c in CASES if c.kind == kind and c.kind_neg == "NONE") == sorted(R.EXPONENTS)
    g = R.global_sweep()
    assert g.size == 129 and g[0] == np.float32(2.0 ** -20) and g[-1] == 4096.0
    c = R.case("L_HUBER")                      # delta, delta - t, delta + t per deviation, 47 probes around each
    assert c.d.size == 2 * (129 + 3 * 47) and c.at_special.sum() >= 6
    assert set(np.unique(c.a0)) == {np.float32(0.25), np.float32(0.37)}
    c = R.case("PUSHPULL-LOG1P-e1p5-LOG-e1")
    assert (c.a0 < 0).any() and (c.a0 > 0).any() and np.isin(np.float32([0.0625, 1.0]), c.d).all()
    c = R.case("LOG-e2")                       # u = d^2 = 1/16 and 1
    assert np.isin(np.float32([0.25, 1.0]), c.d).all()


def test_reference_against_the_golden_distortions(golden_functions):
    g = golden_functions
    edges = g["edges"]
    for name in g["names"]:
        name = str(name)
        a1 = g[name + "__a1"] if (name + "__a1") in g.files else None
        for tag in ("d1", "d2", "d3", "d8", "zero"):
            X = (g["X_zero"] if tag == "zero" else g["X_" + tag]).astype(np.float64)
            dist = np.sqrt(((X[edges[:, 0]] - X[edges[:, 1]]) ** 2).sum(1))
            want = g["%s__%s__distortions" % (name, tag)]
            ok = np.isfinite(want) & (dist > 0)
            assert ok.sum() >= 0.9 * want.size
            f, _ = R.ref(str(g[name + "__kind"]), dist, g[name + "__a0"], a1,
                         tuple(np.float32(g[name + "__scalars"]).astype(np.float64)),
                         str(g[name + "__kind_neg"]), tuple(np.float32(g[name + "__scalars_neg"]).astype(np.float64)))
            np.testing.assert_allclose(f[ok], want[ok], rtol=2e-5, atol=1e-6, err_msg=str((name, tag)))


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_reference_derivative_against_a_central_difference(c):
    """f' of the reference against (f(d + h) - f(d - h)) / 2h of the reference's own f, evaluated by mpmath at 50
    digits with h = 1e-20 d, on every eighth probe of the global sweep and k = 1, 5, .. 21 of the local ones; the
    special points themselves (kinks, jumps) are left out."""
    import mpmath
    thin = ((c.local_k == 0) & (c.sweep_k % 8 == 0) & ~c.at_special) | (np.abs(c.local_k) % 4 == 1) & (np.abs(c.local_k) < 22)
    thin &= ~c.at_special
    idx = np.flatnonzero(thin)
    assert idx.size >= 17
    _, g = c.ref()
    with mpmath.workprec(170):                 # 50 digits
        for i in idx:
            d = mpmath.mpf(float(c.d[i]))
            h = d * mpmath.mpf(10) ** -20
            a1 = None if c.a1 is None else c.a1[i]
            args = (c.a0[i], a1, c.scalars, c.kind_neg, c.scalars_neg)
            fd = (R.f_mp(c.kind, d + h, *args) - R.f_mp(c.kind, d - h, *args)) / (2 * h)
            # (50 digits of f, O(1 + |f|) inside, divided by 2h = 2e-20 d: the difference itself is good to 1e-29 (1 + |f|) / d)
            f0 = abs(float(R.f_mp(c.kind, d, *args)))
            got = g[i] * float(c.d[i])
            assert got == pytest.approx(float(fd), rel=1e-9, abs=1e-28 * (1.0 + f0) / float(d)), (c.id, float(d), float(c.a0[i]))


# Probes at which the ORACLE is excused from the rule (the kernels are not): kind: (which probes, why -- from the
# oracle's own formula, at most this fraction of a case's probes).  The Logistic loss beyond |d - delta| = 80 is the
# one known in advance (every probe of the global sweep from 2^6.5 on); any further entry may cover 5 % at the most.
ORACLE_EXCEPTIONS = {
    "L_LOGISTIC": (lambda d, a0: np.abs(d - a0) > 80.0,
                   "logf(1 + expf(r)): expf(r) overflows for r > 88, as the reference's float32 does", 0.15),
}


@functools.lru_cache(maxsize=None)
def _oracle_run(id):
    """The oracle on the matching graph of one case: per-probe f (oracle.distortions), the mean, per-probe f'/d read off
    the gradient (oracle.average_distortion), the excused probes."""
    c = R.case(id)
    edges, X = c.matching(2, 0)
    fd = c.oracle_func()
    with np.errstate(all="ignore"):
        dist = oracle.distances(edges, X)
        assert np.array_equal(dist, c.d)
        f = oracle.distortions(dist, fd).astype(np.float64)
        E, grad = oracle.average_distortion(edges, X, fd)
    g = c.g_from_grad(grad, 0, c.d.size)
    assert np.array_equal(grad[1::2], -grad[0::2]) and not grad[:, 1].any()
    excused = np.zeros(c.d.size, dtype=bool)
    kinds = c.branch_kind()
    for kind, (where, _, most) in ORACLE_EXCEPTIONS.items():
        this = (kinds == kind) & where(c.d.astype(np.float64), c.a0.astype(np.float64))
        assert this.mean() <= most and (most <= 0.05 or kind == "L_LOGISTIC")
        excused |= this
    return f, E, g, excused


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_oracle_passes_the_rule(c):
    f, E, g, excused = _oracle_run(c.id)
    b = R.bounds(c)
    for name, got in (("f", f), ("f'/d", g)):
        bb = b["f" if name == "f" else "g"]
        ok = R.passes(got, bb) | excused
        assert ok.all(), R.describe_failures(c, name, np.where(excused, bb[0], got), bb)
    # the mean, as the device test asks it of average_distortion
    keep = ~excused
    if keep.all():
        R0 = b["f"][0]
        assert abs(E - R0.mean()) <= R.per_edge_bound(b["f"]).mean() + 2.0 ** -19 * np.abs(R0).mean()


def _oracle_need():
    """What the oracle needs beyond RTOL |R| + hull + 2^-100, in units of 2^-24 S, per kind and output."""
    out = {k: [0.0, 0.0] for k in R.KINDS}
    for c in CASES:
        f, _, g, excused = _oracle_run(c.id)
        b = R.bounds(c)
        kinds = c.branch_kind()
        for k, (got, name, rtol) in enumerate(((f, "f", LOSS_RTOL), (g, "g", GRAD_RTOL))):
            nd = np.where(excused, 0.0, R.need(got, b[name], rtol))
            for kind in set(kinds):
                out[kind][k] = max(out[kind][k], float(nd[kinds == kind].max()))
    return out


def test_oracle_need_of_the_absolute_term():
    """The one constant of the rule that is not derived is the 8 of A = 8 x 2^-24 x S.  The oracle (libm, nearly
    correctly rounded) must need at most 2 of those units at every kind -- the other 6 are for the kernels' 1-ulp
    v_rcp / v_exp / v_log -- and nothing where S_TABLE has no absolute term.  S_TABLE records the figures."""
    need = _oracle_need()
    print("\noracle's need in units of 2^-24 S (f, f'/d):")
    for kind in R.KINDS:
        print("  %-22s %.2f %.2f" % (kind, need[kind][0], need[kind][1]))
    for kind in R.KINDS:
        Sf, Sg, nf, ng = R.S_TABLE[kind]
        for S, recorded, measured in ((Sf, nf, need[kind][0]), (Sg, ng, need[kind][1])):
            assert measured <= 2.0, (kind, measured)
            assert recorded <= 2.0 and (S is not None or recorded == 0.0), kind
            assert measured <= recorded + 0.25, (kind, measured, recorded)   # the table is kept up to date


def test_rule_rejects_a_log1p_without_its_correction():
    """The rule has teeth: float32 log(fl(1 + u)) for log1p(u) -- the rounding-error correction dropped -- is off by
    up to 2^-24 / u relative and fails below u ~ 1e-2, while an honest float32 log1p passes everywhere."""
    c = R.case("LOG1P-e1p5")
    pe = (c.d.astype(np.float64) ** 1.5).astype(np.float32)
    naive = c.a0 * np.log(np.float32(1.0) + pe)
    honest = c.a0 * np.log1p(pe)
    assert naive.dtype == np.float32 and honest.dtype == np.float32
    b = R.bounds(c)["f"]
    assert R.passes(honest, b).all()
    bad = ~R.passes(naive, b)
    assert bad.sum() > 50 and (pe[bad] < 0.05).all()

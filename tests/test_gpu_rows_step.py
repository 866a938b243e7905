"""mde_rows_init / mde_rows_step on the GPU against the float64 mirror with the kernel's float32 state
(``tests/_rows_reference.py``), on hand-made states that reach every branch of the update with a clear margin."""
import numpy as np
import pytest
import torch

import _rows_reference as ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
N = 130                 # two full waves and a partial one
N_C = 7                 # f = row_loss / N_C
EPS = 1e-5
RTOL = 1e-5             # float32 rounding of the mirror's values
BRANCHES = ["update", "skip", "converge", "same", "small_twice", "small_once", "interpolate", "clamp_low",
            "clamp_high", "not_finite", "floor", "reset", "inactive"]


def _state(d):
    """A float32 mirror state of N rows, the evaluation (f_t, g_t) at its trial points, and each row's branch."""
    rng = np.random.default_rng(50 + d)
    branch = np.array([BRANCHES[i % len(BRANCHES)] for i in range(N)])
    x = rng.standard_normal((N, d)).astype(np.float32)
    g = rng.standard_normal((N, d)).astype(np.float32)
    A = rng.standard_normal((N, d, d)) * 0.3
    H = (A @ A.transpose(0, 2, 1) + np.eye(d)).astype(np.float32)
    H = ((H + H.transpose(0, 2, 1)) / 2).astype(np.float32)
    t = rng.uniform(0.2, 1.0, N).astype(np.float32)
    f = rng.uniform(5.0, 15.0, N)
    fresh = (np.arange(N) // len(BRANCHES)) % 2
    small = np.zeros(N, dtype=np.int32)
    status = np.zeros(N, dtype=np.int32)
    reset = branch == "reset"
    H[reset] = -H[reset]                                        # no descent direction can come of it
    p = -np.einsum("nab,nb->na", H.astype(np.float64), g.astype(np.float64)).astype(np.float32)
    p[reset] = -g[reset]
    t[branch == "floor"] = 1e-12
    f[np.isin(branch, ["small_twice", "small_once"])] = 1e10    # a decrease of a few units is below 1e-7 |f| = 1e3
    small[branch == "small_twice"] = 1
    small[(branch == "update") & (fresh == 1)] = 1              # a large decrease resets the counter
    inactive = np.nonzero(branch == "inactive")[0]
    status[inactive] = np.where(np.arange(len(inactive)) % 2 == 0, ref.CONVERGED, ref.STALLED)
    x_trial = (x.astype(np.float64) + t.astype(np.float64)[:, None] * p.astype(np.float64)).astype(np.float32)
    x_trial[branch == "same"] = x[branch == "same"]
    x_trial[inactive] = rng.standard_normal((len(inactive), d)).astype(np.float32)   # to be overwritten with x
    state = ref.State(x, f, g, H, p, t, status, fresh, small, x_trial, np.float32)

    # ---- the evaluation at the trial points
    gp = (g.astype(np.float64) * p.astype(np.float64)).sum(1)                # < 0
    tgp = t.astype(np.float64) * gp
    s = x_trial.astype(np.float64) - x.astype(np.float64)
    f_t = f + 0.5 * tgp                                                       # accepted: far below f + 1e-4 t g.p
    M = rng.standard_normal((N, d, d)) * 0.3
    M = M @ M.transpose(0, 2, 1) + np.eye(d)
    g_t = (g.astype(np.float64) + np.einsum("nab,nb->na", M, s)).astype(np.float32)      # s.y = s.M s > 0
    negative = np.isin(branch, ["skip", "reset"])
    g_t[negative] = (g.astype(np.float64) - 0.5 * s)[negative].astype(np.float32)        # s.y = -|s|^2 / 2 < 0
    conv = branch == "converge"
    g_t[conv] = (1e-7 * rng.standard_normal((int(conv.sum()), d))).astype(np.float32)    # |g_t| << eps
    g_t[branch == "same"] = (g[branch == "same"] * 0.5).astype(np.float32)
    for name, alpha in (("interpolate", 1.0), ("clamp_low", 20.0), ("clamp_high", -0.5e-4)):
        rows = branch == name                                   # f_t - f = alpha (-g.p t): t / (2 (1 + alpha))
        f_t[rows] = (f - alpha * tgp)[rows]
    f_t[branch == "floor"] = (f - 1.0 * tgp)[branch == "floor"]
    bad = np.nonzero(branch == "not_finite")[0]
    f_t[bad[0::3]] = np.inf
    f_t[bad[1::3]] = np.nan
    g_t[bad[2::3], 0] = np.nan                                  # a good value with a gradient that is not finite
    f_t[inactive] = np.nan                                      # never read
    return state, f_t, g_t, branch


class _Device(object):
    """The mirror state on the GPU, in the layout of the kernels."""

    def __init__(self, state):
        up = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a).astype(dt)).to(DEV)
        self.x, self.g, self.H, self.p, self.t, self.x_trial = (
            up(a, np.float32) for a in (state.x, state.g, state.H, state.p, state.t, state.x_trial))
        self.f = up(state.f, np.float64)
        self.flags = up(state.status | (state.fresh << 2) | (state.small << 3), np.int32)
        self.counts = torch.full((3,), -1, dtype=torch.int64, device=DEV)

    def arrays(self):
        return dict(x=self.x, f=self.f, g=self.g, H=self.H, p=self.p, t=self.t, flags=self.flags,
                    x_trial=self.x_trial)

    def host(self):
        return {k: v.cpu().numpy() for k, v in self.arrays().items()}


def _step(dev, d, f_t, g_t):
    from pymde_amd import _lib
    row_loss = torch.as_tensor(f_t * N_C).to(DEV)
    row_grad = torch.as_tensor(g_t).to(DEV)
    a = dev.arrays()
    _lib.check(_lib.load().mde_rows_step(N, d, N_C, EPS, *[_lib.ptr(a[k]) for k in
                                                             ("x", "f", "g", "H", "p", "t", "flags", "x_trial")],
                                         _lib.ptr(row_loss), _lib.ptr(row_grad), _lib.ptr(dev.counts),
                                         _lib.stream_ptr(torch.device(DEV))))
    torch.cuda.synchronize()


@pytest.mark.parametrize("d", [1, 2, 3, 5, 8])
def test_step_follows_the_mirror_in_every_branch(d):
    state, f_t, g_t, branch = _state(d)
    dev = _Device(state)
    before = dev.host()
    _step(dev, d, f_t, g_t)
    got = dev.host()
    want = ref.step(state.copy(), (f_t * N_C) / N_C, g_t, EPS)
    # the hand-made states reach the branches they were made for
    expect = {"update": ref.ACTIVE, "skip": ref.ACTIVE, "converge": ref.CONVERGED, "same": ref.STALLED,
              "small_twice": ref.STALLED, "small_once": ref.ACTIVE, "interpolate": ref.ACTIVE,
              "clamp_low": ref.ACTIVE, "clamp_high": ref.ACTIVE, "not_finite": ref.ACTIVE, "floor": ref.STALLED,
              "reset": ref.ACTIVE}
    for name, status in expect.items():
        rows = branch == name
        assert (want.status[rows] == status).all(), name
    t0 = state.t.astype(np.float64)
    for name, factor in (("interpolate", 0.25), ("clamp_low", 0.1), ("clamp_high", 0.5), ("not_finite", 0.5)):
        np.testing.assert_allclose(want.t[branch == name], (factor * t0)[branch == name], rtol=1e-6)
    assert (want.fresh[branch == "reset"] == 1).all() and (want.fresh[branch == "update"] == 0).all()
    assert (want.small[branch == "small_once"] == 1).all() and (want.small[branch == "update"] == 0).all()
    assert (want.x[branch == "interpolate"] == state.x[branch == "interpolate"]).all()        # rejected: x stays
    # exact: status, fresh bit, counter, counts, and what is adopted
    assert (got["flags"] == (want.status | (want.fresh << 2) | (want.small << 3))).all()
    assert dev.counts.tolist() == want.counts()
    assert (got["x"] == want.x).all() and (got["g"] == want.g).all() and (got["f"] == want.f).all()
    # to float32 rounding of the mirror's values
    for key in ("t", "H", "p", "x_trial"):
        w = getattr(want, key)
        w64 = w.astype(np.float64)
        worst = float((np.abs(got[key].astype(np.float64) - w64) / np.maximum(np.abs(w64), 1e-300)).max())
        print("d=%d %s: worst rel. difference from the mirror %.3g (bound %.3g)" % (d, key, worst, RTOL))
        np.testing.assert_allclose(got[key], w, rtol=RTOL, atol=0, equal_nan=False)
    # the state of the inactive rows, bit for bit; their trial point is x
    rows = branch == "inactive"
    for key in ("x", "f", "g", "H", "p", "t", "flags"):
        assert got[key][rows].tobytes() == before[key][rows].tobytes(), key
    assert got["x_trial"][rows].tobytes() == before["x"][rows].tobytes()


@pytest.mark.parametrize("d", [1, 3, 8])
def test_init_follows_the_mirror(d):
    from pymde_amd import _lib
    rng = np.random.default_rng(60 + d)
    x = rng.standard_normal((N, d)).astype(np.float32)
    g = (rng.standard_normal((N, d)) * np.where(np.arange(N) % 2, 0.05, 5.0)[:, None]).astype(np.float32)
    g[::5] = (1e-7 * rng.standard_normal((len(g[::5]), d))).astype(np.float32)      # converged at the start
    row_loss = rng.uniform(1.0, 9.0, N)
    row_loss[3] = np.inf                                                            # a row that cannot be worked on
    want = ref.init(x, row_loss / N_C, g, EPS, np.float32)
    dev = _Device(ref.State(*(np.zeros_like(a) for a in (want.x, want.f, want.g, want.H, want.p, want.t)),
                            want.status * 0, want.fresh * 0, want.small * 0, np.zeros_like(want.x), np.float32))
    dev.x.copy_(torch.as_tensor(x))
    a = dev.arrays()
    row_loss_dev, row_grad_dev = torch.as_tensor(row_loss).to(DEV), torch.as_tensor(g).to(DEV)
    _lib.check(_lib.load().mde_rows_init(N, d, N_C, EPS, _lib.ptr(a["x"]), _lib.ptr(row_loss_dev),
                                         _lib.ptr(row_grad_dev),
                                         *[_lib.ptr(a[k]) for k in ("f", "g", "H", "p", "t", "flags", "x_trial")],
                                         _lib.ptr(dev.counts), _lib.stream_ptr(torch.device(DEV))))
    torch.cuda.synchronize()
    got = dev.host()
    assert sorted(set(want.status)) == [ref.ACTIVE, ref.CONVERGED, ref.STALLED]
    assert (got["flags"] == (want.status | 4)).all() and dev.counts.tolist() == want.counts()
    for key in ("x", "f", "g", "H", "p"):
        assert (got[key] == getattr(want, key)).all(), key
    np.testing.assert_allclose(got["t"], want.t, rtol=RTOL, atol=0)
    np.testing.assert_allclose(got["x_trial"], want.x_trial, rtol=RTOL, atol=0)

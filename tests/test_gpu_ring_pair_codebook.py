"""The pair codebook of the LDS-ring kernel (csrc/mde_ring_kernel.h, PS 3; include/mde_hip.h, a0_scalar = 4): a per-edge
array of one or two distinct values under a function whose coinciding entries add zero (Log1p, exponents 1, 1.5, 2)
streams as the 4-byte codebook does, but the kernel selects the value with bit 0 of the packed word between two
registers instead of reading an 8-entry table from LDS.  Padding lanes select a real weight in this form; their
column is their own dummy row, so they add exact zeros.  MDE_CODEBOOK_PAIR=0 sends the same arrays through the LDS
table: the selected values are the same floats, so the gradient must agree BITWISE and the loss exactly.

Shape: that of tests/test_gpu_ring_loss_band.py -- n = 16384, out-degree 24, bench.make_workload, MDE_PANEL=1
MDE_RING_ROWS=512 MDE_RING_Q=2 -- and out-degree 3 for streams of part-filled iterations.  Tolerances
against the float64 oracle: those of tests/test_gpu_configs.py for a forced ring layout (loss 1e-5 relative,
assert_grad_close)."""
import os

import pytest
import torch

from conftest import assert_grad_close
from oracle import oracle

pytestmark = pytest.mark.gpu
DEV = "cuda"
N = 16384
LAYOUT_ENV = {"MDE_PANEL": "1", "MDE_RING_ROWS": "512", "MDE_RING_Q": "2"}
KNOBS = ("MDE_PANEL", "MDE_RING_ROWS", "MDE_RING_Q", "MDE_RING_LOSS_BAND", "MDE_RING_HUB", "MDE_RING_PERMUTE",
         "MDE_CODEBOOK_PAIR", "MDE_CODEBOOK")


class _Env(object):
    """The knobs of one case, restored afterwards (the library reads them when it builds a layout or a stream)."""

    def __init__(self, **extra):
        self.want = dict(LAYOUT_ENV, **extra)

    def __enter__(self):
        self.saved = {k: os.environ.get(k) for k in KNOBS}
        for k in KNOBS:
            os.environ.pop(k, None)
        os.environ.update(self.want)

    def __exit__(self, *exc):
        for k, v in self.saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def _evaluate(edges, function, X, runs=1, lo=0, hi=None):
    """`runs` evaluations on a fresh plan: the buffers ([n * d] gradient | loss), the binding and the plan's layout."""
    from pymde_amd.average_distortion import Binding, EdgePlan, fused_evaluate
    n, d = X.shape
    plan = EdgePlan(n, edges, lo, n if hi is None else hi)
    b = Binding(plan, function)
    bufs = []
    for _ in range(runs):
        buf = torch.zeros(n * d + 1, device=X.device)
        fused_evaluate(b, X, buf[:n * d].view(n, d), buf[n * d:])
        bufs.append(buf)
    st = b.struct(d)
    assert st.layout == 1, "the LDS-ring layout should have been chosen"
    return {"bufs": bufs, "form": int(st.a0_scalar), "codebook": b.codebook, "stream_kind": b.stream_kind,
            "info": plan.ring_info()}


_WORKLOADS = {}


def _workload(deg, d):
    import bench
    if (deg, d) not in _WORKLOADS:
        _WORKLOADS[(deg, d)] = bench.make_workload(torch.device(DEV, 0), n=N, deg=deg, d=d)
    return _WORKLOADS[(deg, d)]


def _both_forms(edges, function, X, env=None, ranges=((0, None),)):
    """The problem with the pair codebook allowed (three evaluations) and with MDE_CODEBOOK_PAIR=0 (one); over several
    vertex-range plans the buffers are the sums of the plans' (every plan owns its rows and its share of the loss)."""
    out = {}
    for name, extra, runs in (("pair", {}, 3), ("table", {"MDE_CODEBOOK_PAIR": "0"}, 1)):
        with _Env(**dict(env or {}, **extra)):
            parts = [_evaluate(edges, function, X, runs=runs, lo=lo, hi=hi) for lo, hi in ranges]
        out[name] = dict(parts[0], bufs=[sum(p["bufs"][r] for p in parts) for r in range(runs)], parts=parts)
    return out


def _check_pair_against_table_and_oracle(res, edges, X, fd):
    n, d = X.shape
    for part in res["pair"]["parts"]:
        assert part["form"] == 4 and part["codebook"] and part["stream_kind"] == "codebook", part
    for part in res["table"]["parts"]:
        assert part["form"] == 2 and part["codebook"] and part["stream_kind"] == "codebook", part
    pair, table = res["pair"]["bufs"], res["table"]["bufs"][0]
    print("loss pair", float(pair[0][n * d]), "table", float(table[n * d]), "stream entries", res["pair"]["info"]["padded_entries"],
          "of them half-edges", res["pair"]["info"]["ring_half_edges"], "iterations", res["pair"]["info"]["iterations"])
    for pp, pt in zip(res["pair"]["parts"], res["table"]["parts"]):   # plan by plan: the very same bits
        assert torch.equal(pp["bufs"][0][:n * d], pt["bufs"][0][:n * d]), "the gradients of the two forms differ bitwise"
        assert float(pp["bufs"][0][n * d]) == float(pt["bufs"][0][n * d]), "the losses of the two forms differ"
        for other in pp["bufs"][1:]:
            assert torch.equal(other, pp["bufs"][0]), "two evaluations differ bitwise"
    assert bool(torch.isfinite(pair[0]).all())
    wE, wgrad = oracle.average_distortion(edges.cpu().numpy(), X.cpu().numpy(), fd)
    print("oracle", wE)
    assert float(pair[0][n * d]) == pytest.approx(wE, rel=1e-5)
    assert_grad_close(pair[0][:n * d].view(n, d).cpu().numpy(), wgrad)


@pytest.mark.parametrize("name", ["d2_two_values", "d2_all_ones", "d3_two_values", "d2_exponent_1", "d2_exponent_2"])
def test_pair_codebook_equals_the_lds_table_bitwise_and_agrees_with_the_oracle(name):
    import pymde_amd
    d = 3 if name.startswith("d3") else 2
    exponent = {"d2_exponent_1": 1.0, "d2_exponent_2": 2.0}.get(name, 1.5)
    edges, w, X = _workload(24, d)
    if name == "d2_all_ones":
        w = torch.ones_like(w)   # (a full array, not the one broadcast scalar)
    res = _both_forms(edges, pymde_amd.penalties.Log1p(w, exponent), X)
    assert res["pair"]["info"]["d"] == d and not res["pair"]["info"]["permuted"], res["pair"]["info"]
    _check_pair_against_table_and_oracle(res, edges, X, oracle.func("LOG1P", w.cpu().numpy(), None, (exponent,)))


@pytest.mark.parametrize("name", ["dealt_rows", "vertex_range"])
def test_streams_of_part_filled_iterations(name):
    """Out-degree 3: 6 half-edges per row, so most wave iterations are part-filled and every padding lane selects a
    real weight.  A padding column that is not the lane's own (zero) row, or a second table entry that is not finite,
    shows here.  Once with the rows dealt to the blocks (MDE_RING_PERMUTE=1), once on a vertex-range plan [n/4, 3n/4)
    -- checked against the oracle together with the two plans that own the other rows."""
    import pymde_amd
    edges, w, X = _workload(3, 2)
    if name == "dealt_rows":
        res = _both_forms(edges, pymde_amd.penalties.Log1p(w), X, env={"MDE_RING_PERMUTE": "1"})
        assert res["pair"]["info"]["permuted"], res["pair"]["info"]
    else:
        res = _both_forms(edges, pymde_amd.penalties.Log1p(w), X, ranges=((N // 4, 3 * N // 4), (0, N // 4), (3 * N // 4, N)))
    info = res["pair"]["info"]
    # ("padded_entries" is the length of the padded streams: the rest of it are padding lanes)
    assert info["padded_entries"] - info["ring_half_edges"] >= info["iterations"], info   # (a lane per iteration at least)
    _check_pair_against_table_and_oracle(res, edges, X, oracle.func("LOG1P", w.cpu().numpy(), None, (1.5,)))


def test_three_values_keep_the_lds_table():
    import pymde_amd
    edges, w, X = _workload(24, 2)
    gen = torch.Generator(device=w.device)
    gen.manual_seed(2)
    w3 = 1.0 + torch.randint(0, 3, w.shape, device=w.device, generator=gen).to(torch.float32)
    assert sorted(torch.unique(w3).tolist()) == [1.0, 2.0, 3.0]
    res = _both_forms(edges, pymde_amd.penalties.Log1p(w3), X)
    n, d = X.shape
    for k in ("pair", "table"):
        assert res[k]["form"] == 2 and res[k]["stream_kind"] == "codebook", res[k]
    assert torch.equal(res["pair"]["bufs"][0], res["table"]["bufs"][0])
    wE, wgrad = oracle.average_distortion(edges.cpu().numpy(), X.cpu().numpy(), oracle.func("LOG1P", w3.cpu().numpy(), None, (1.5,)))
    assert float(res["pair"]["bufs"][0][n * d]) == pytest.approx(wE, rel=1e-5)
    assert_grad_close(res["pair"]["bufs"][0][:n * d].view(n, d).cpu().numpy(), wgrad)


def test_a_function_without_the_trait_keeps_the_lds_table():
    """Log: w log(1 - exp(-d)) is -Inf x w at d = 0 -- a padding lane with a real weight would add it.  Two values,
    yet the stream stays in the LDS-table form, whose padding lanes carry weight 0."""
    import pymde_amd
    edges, w, X = _workload(24, 2)
    wn = -w
    with _Env():
        res = _evaluate(edges, pymde_amd.penalties.Log(wn), X)
    n, d = X.shape
    assert res["form"] == 2 and res["codebook"] and res["stream_kind"] == "codebook", res
    wE, wgrad = oracle.average_distortion(edges.cpu().numpy(), X.cpu().numpy(), oracle.func("LOG", wn.cpu().numpy(), None, (1.0,)))
    assert float(res["bufs"][0][n * d]) == pytest.approx(wE, rel=1e-5)
    assert_grad_close(res["bufs"][0][:n * d].view(n, d).cpu().numpy(), wgrad)

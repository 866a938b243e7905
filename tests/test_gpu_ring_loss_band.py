"""Who adds an edge's loss term in the LDS-ring layout (csrc/mde_ring.h, ring_counts).  Every edge has one entry per
endpoint; one of them adds the term.  "The smaller vertex" puts all the loss arithmetic on one corner of the (row
block, column group) grid; at d = 2, on full plans whose rows are not permuted, the rule flips between bands of
``loss_band`` vertices instead, so that every workgroup adds about half of its entries' terms.  The gradient does not
depend on the rule at all, the loss only by its order of summation.

Shape: n = 16384, out-degree 24, uniform-random edges built like bench.make_workload, Log1p with weights {1, 2};
MDE_PANEL=1 MDE_RING_ROWS=512 MDE_RING_Q=2 gives 32 row blocks x 2 column groups = 64 workgroups of 16 chunks.
Case A: the default band (1024 vertices, 16 bands: nearly every block of four iterations crosses a band's edge and
tests per lane); case B: MDE_RING_LOSS_BAND=8 row blocks (4 bands: whole blocks that add all or none); band 0: the
old rule.  Tolerances: those of tests/test_gpu_configs.py for a forced ring layout (loss 1e-5 relative,
assert_grad_close)."""
import os

import numpy as np
import pytest
import torch

from conftest import assert_grad_close
from oracle import oracle

pytestmark = pytest.mark.gpu
DEV = "cuda"
N, DEG = 16384, 24
LAYOUT_ENV = {"MDE_PANEL": "1", "MDE_RING_ROWS": "512", "MDE_RING_Q": "2"}
KNOBS = ("MDE_PANEL", "MDE_RING_ROWS", "MDE_RING_Q", "MDE_RING_LOSS_BAND", "MDE_RING_HUB", "MDE_RING_PERMUTE")


class _Env(object):
    """The layout knobs of one case, restored afterwards (the library reads them when it builds a layout)."""

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


def _evaluate(edges, w, X, runs=1, lo=0, hi=None):
    """`runs` evaluations on a fresh plan: the buffers ([n * d] gradient | loss) and the plan."""
    import pymde_amd
    from pymde_amd.average_distortion import Binding, EdgePlan, fused_evaluate
    n, d = X.shape
    plan = EdgePlan(n, edges, lo, n if hi is None else hi)
    b = Binding(plan, pymde_amd.penalties.Log1p(w))
    bufs = []
    for _ in range(runs):
        buf = torch.zeros(n * d + 1, device=X.device)
        fused_evaluate(b, X, buf[:n * d].view(n, d), buf[n * d:])
        bufs.append(buf)
    assert b.struct(d).layout == 1, "the LDS-ring layout should have been chosen"
    return bufs, plan


def _oracle(edges, w, X):
    return oracle.average_distortion(edges.cpu().numpy(), X.cpu().numpy(), oracle.func("LOG1P", w.cpu().numpy(), None, (1.5,)))


@pytest.fixture(scope="module")
def workload():
    import bench
    dev = torch.device(DEV, 0)
    edges, w, X = bench.make_workload(dev, n=N, deg=DEG, d=2)
    wE, wgrad = _oracle(edges, w, X)
    return {"edges": edges, "w": w, "X": X, "loss": wE, "grad": wgrad}


@pytest.fixture(scope="module")
def cases(workload):
    """Cases A, B and band 0 on the same problem: three evaluations each, the layout's description and its check."""
    out = {}
    for name, extra in (("A", {}), ("B", {"MDE_RING_LOSS_BAND": "8"}), ("0", {"MDE_RING_LOSS_BAND": "0"})):
        with _Env(**extra):
            bufs, plan = _evaluate(workload["edges"], workload["w"], workload["X"], runs=3)
            out[name] = {"bufs": bufs, "info": plan.ring_info(), "check": plan.ring_check()}
    return out


def test_layout_geometry_and_bands(cases):
    for name, band in (("A", 1024), ("B", 8 * 512), ("0", 0)):
        info = cases[name]["info"]
        assert (info["d"], info["rows_per_block"], info["row_blocks"], info["col_groups"], info["chunks"]) == (2, 512, 32, 2, 32), info
        assert not info["permuted"] and info["hub_rows"] == 0, info
        assert info["loss_band"] == band, (name, info)


def test_all_three_loss_classes_occur(cases):
    a, b = cases["A"]["info"]["class_blocks"], cases["B"]["info"]["class_blocks"]
    print("class blocks (none, all, per lane): A", a, "B", b, "band 0", cases["0"]["info"]["class_blocks"])
    assert b[0] > 0 and b[1] > 0, b                 # whole blocks that add none / all of their terms
    assert a[2] > 0, a                              # ... and the per-lane test
    assert all(a[c] + b[c] > 0 for c in range(3))
    assert 2 * a[2] > sum(a), a                     # (case A: most blocks cross a band's edge)


@pytest.mark.parametrize("name", ["A", "B", "0"])
def test_every_edge_adds_its_loss_term_exactly_once(cases, workload, name):
    chk, info = cases[name]["check"], cases[name]["info"]
    assert chk["pairs"] == info["iterations"] // 2 and chk["split"] == 0, chk
    assert chk["loss_edges"] == workload["edges"].shape[0], chk     # every edge has both entries in a full plan
    assert chk["loss_bad"] == 0 and chk["loss_flag_bad"] == 0, chk


@pytest.mark.parametrize("name", ["A", "B", "0"])
def test_loss_and_gradient_against_oracle_and_bitwise_repeatable(cases, workload, name):
    bufs = cases[name]["bufs"]
    n, d = workload["X"].shape
    print("loss", name, float(bufs[0][n * d]), "oracle", workload["loss"])
    assert float(bufs[0][n * d]) == pytest.approx(workload["loss"], rel=1e-5)
    assert_grad_close(bufs[0][:n * d].view(n, d).cpu().numpy(), workload["grad"])
    for other in bufs[1:]:
        assert torch.equal(other, bufs[0]), "two evaluations differ bitwise"


def test_gradient_does_not_depend_on_the_rule(cases, workload):
    n, d = workload["X"].shape
    for name in ("A", "B"):
        assert torch.equal(cases[name]["bufs"][0][:n * d], cases["0"]["bufs"][0][:n * d]), name


def test_bands_even_out_the_workgroups_loss_shares(cases):
    spread = {k: v["info"]["loss_share_max"] - v["info"]["loss_share_min"] for k, v in cases.items()}
    print("loss share spread over the workgroups:", spread)
    assert 0.0 <= cases["A"]["info"]["loss_share_min"] <= cases["A"]["info"]["loss_share_max"] <= 1.0
    assert spread["A"] < spread["0"], spread


def test_hub_row_uses_the_same_rule(workload):
    """One hub of degree n / 4, peeled off to the hub kernel: its half-edges' twins sit in the ring streams, and both
    sides must agree on who adds the term (default band)."""
    edges, w, X = workload["edges"], workload["w"], workload["X"]
    gen = torch.Generator(device=edges.device)
    gen.manual_seed(1)
    p, h, hub = edges.shape[0], N // 4, N // 3
    other = torch.randperm(N - 1, device=edges.device, generator=gen)[:h]
    other += (other >= hub).to(torch.int64)
    idx = torch.randperm(p, device=edges.device, generator=gen)[:h]
    e2 = edges.clone()
    e2[idx, 0] = torch.minimum(other, torch.full_like(other, hub))
    e2[idx, 1] = torch.maximum(other, torch.full_like(other, hub))
    with _Env(MDE_RING_HUB="1000", MDE_RING_PERMUTE="0"):
        bufs, plan = _evaluate(e2, w, X)
        info, chk = plan.ring_info(), plan.ring_check()
    assert info["hub_rows"] == 1 and not info["permuted"] and info["loss_band"] == 1024, info
    assert chk["loss_bad"] == 0 and chk["loss_flag_bad"] == 0 and chk["loss_edges"] == p, chk
    wE, wgrad = _oracle(e2, w, X)
    n, d = X.shape
    assert float(bufs[0][n * d]) == pytest.approx(wE, rel=1e-5)
    assert_grad_close(bufs[0][:n * d].view(n, d).cpu().numpy(), wgrad)


def test_sharded_plans_keep_the_old_rule(workload, cases):
    """The ranks of a sharded problem choose their block heights independently: no bands across plans."""
    edges, w, X = workload["edges"], workload["w"], workload["X"]
    n, d = X.shape
    total = torch.zeros(n * d + 1, device=X.device)
    with _Env():
        for lo, hi in ((0, N // 2), (N // 2, N)):
            bufs, plan = _evaluate(edges, w, X, lo=lo, hi=hi)
            info, chk = plan.ring_info(), plan.ring_check()
            assert info["built"] and info["loss_band"] == 0, info
            assert chk["loss_bad"] == 0 and chk["loss_flag_bad"] == 0, chk
            total += bufs[0]
    assert float(total[n * d]) == pytest.approx(float(cases["A"]["bufs"][0][n * d]), rel=1e-5)   # the unsharded plan's
    assert float(total[n * d]) == pytest.approx(workload["loss"], rel=1e-5)
    assert_grad_close(total[:n * d].view(n, d).cpu().numpy(), workload["grad"])


def test_d3_keeps_the_old_rule():
    import bench
    dev = torch.device(DEV, 0)
    edges, w, X = bench.make_workload(dev, n=N, deg=DEG, d=3)
    with _Env():
        bufs, plan = _evaluate(edges, w, X)
        info, chk = plan.ring_info(), plan.ring_check()
    assert info["built"] and info["d"] == 3 and info["loss_band"] == 0, info
    assert chk["loss_bad"] == 0 and chk["loss_edges"] == edges.shape[0], chk
    wE, wgrad = _oracle(edges, w, X)
    assert float(bufs[0][N * 3]) == pytest.approx(wE, rel=1e-5)
    assert_grad_close(bufs[0][:N * 3].view(N, 3).cpu().numpy(), wgrad)

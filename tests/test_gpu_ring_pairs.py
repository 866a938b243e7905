"""Lane-stable pairs of the LDS-ring layout: the kernel (csrc/mde_ring_kernel.h) reads both accumulators of a pair of
wave iterations before it writes either, and forwards a row the two iterations share in a register -- which is only
right when the layout holds every such row on ONE lane in both iterations (k_ring_pack).  Each case builds a layout
the way an evaluation does and checks every pair of it on the device (mde_plan_ring_check)."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _layout(n, deg, d, graph="uniform", force=False, monkeypatch=None):
    import bench
    import pymde_amd
    from pymde_amd.average_distortion import Binding, EdgePlan, fused_evaluate
    if force:
        monkeypatch.setenv("MDE_PANEL", "1")
    dev = torch.device(DEV, 0)
    edges, w, X = bench.make_workload(dev, n=n, deg=deg, d=d, graph=graph)
    f = pymde_amd.penalties.Log1p(w)
    b = Binding(EdgePlan(n, edges), f)
    buf = torch.zeros(n * d + 1, device=dev)
    fused_evaluate(b, X, buf[:n * d].view(n, d), buf[n * d:])
    assert b.struct(d).layout == 1, "the LDS-ring layout should have been chosen"
    assert torch.isfinite(buf).all()
    return b.plan


@pytest.mark.parametrize("case", ["uniform", "d3", "hub", "powerlaw", "d1", "d4"])
def test_ring_layout_keeps_a_pairs_shared_rows_on_one_lane(case, monkeypatch):
    if case == "uniform":
        plan = _layout(1_000_000, 50, 2)
    elif case == "d3":
        plan = _layout(1_000_000, 50, 3)
    elif case == "hub":
        plan = _layout(1_000_000, 50, 2, graph="hub")
    elif case == "powerlaw":
        plan = _layout(1_000_000, 50, 2, graph="powerlaw")
    else:
        plan = _layout(200_000, 20, int(case[1]), force=True, monkeypatch=monkeypatch)
    info = plan.ring_info()
    if case == "hub":
        assert info["hub_rows"] == 1
    if case == "powerlaw":
        assert info["permuted"] and info["hub_rows"] > 10
    chk = plan.ring_check()
    assert chk["pairs"] == info["iterations"] // 2
    assert chk["shared"] > 0, chk   # (the check saw rows that both iterations of a pair hold)
    assert chk["split"] == 0, chk

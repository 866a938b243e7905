"""BASELINE.json configs at (or near) full size: oracle comparison where the oracle finishes in
seconds, size-independent properties otherwise (translation invariance of E, zero row-sum of the
gradient, constraint residuals, monotone solver progress, sharding = unsharded)."""
import os

import numpy as np
import pytest
import torch

from conftest import assert_grad_close
from oracle import oracle

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _knn_like_graph(rng, n, k):
    """k out-neighbours per item within a window (kNN-graph-like locality), undirected, unique."""
    src = np.repeat(np.arange(n), k)
    off = rng.integers(1, 200, n * k)
    dst = (src + off) % n
    lo, hi = np.minimum(src, dst), np.maximum(src, dst)
    key = np.unique(lo.astype(np.int64) * n + hi)
    return np.stack([key // n, key % n], 1)


def test_config2_mnist_like_preserve_neighbors_problem():
    """configs[1]: n = 70k, k = 15 kNN + as many repulsive edges, PushAndPull(Log1p, LogRatio), d = 2,
    Standardized (synthetic stand-in: MNIST is not available offline)."""
    import pymde_amd
    pen = pymde_amd.penalties
    rng = np.random.default_rng(0)
    n = 70000
    att = _knn_like_graph(rng, n, 15)
    i = rng.integers(0, n, len(att))
    j = (i + 1 + rng.integers(0, n - 1, len(att))) % n
    rep = np.stack([np.minimum(i, j), np.maximum(i, j)], 1)
    edges = np.concatenate([att, rep])
    w = np.concatenate([1.0 + (rng.random(len(att)) < 0.3), -np.ones(len(rep))]).astype(np.float32)
    f = pen.PushAndPull(torch.tensor(w, device=DEV), pen.Log1p, pen.LogRatio)
    mde = pymde_amd.MDE(n, 2, torch.tensor(edges, device=DEV), f, constraint=pymde_amd.Standardized())
    torch.manual_seed(0)
    X0 = pymde_amd.Standardized().initialization(n, 2, device=DEV)
    Xt = X0.clone().requires_grad_(True)
    E = mde.average_distortion(Xt)
    E.backward()
    wE, wgrad = oracle.average_distortion(edges, X0.cpu().numpy(),
                                          oracle.func("LOG1P", w, None, (1.5,), "LOGRATIO", (2.0,)))
    assert float(E) == pytest.approx(wE, rel=1e-5)
    assert_grad_close(Xt.grad.cpu().numpy(), wgrad)
    mde.embed(X=X0, max_iter=40)
    Es = np.array(mde.solve_stats.average_distortions)
    assert (np.diff(Es) <= 1e-6 * np.abs(Es[:-1])).all() and Es[-1] < Es[0]
    X = mde.X.double().cpu().numpy()
    np.testing.assert_allclose(X.T @ X / n, np.eye(2), atol=5e-5)
    np.testing.assert_allclose(X.mean(0), 0, atol=1e-5)


def test_config3_sparse_graph_distances_huber():
    """configs[2]: n ~ 40k, sampled graph distances, Huber loss, d = 2 (synthetic stand-in for the
    Google Scholar graph: pairs with ring-lattice hop distances)."""
    import pymde_amd
    rng = np.random.default_rng(1)
    n, p = 40000, 3_000_000
    i = rng.integers(0, n, p)
    j = (i + 1 + rng.integers(0, n - 1, p)) % n
    key = np.unique(np.minimum(i, j).astype(np.int64) * n + np.maximum(i, j))
    edges = np.stack([key // n, key % n], 1)
    hop = np.abs(edges[:, 0] - edges[:, 1])
    dev = (np.minimum(hop, n - hop) / 500.0 + 1.0).astype(np.float32)
    f = pymde_amd.losses.Huber(torch.tensor(dev, device=DEV), 1.0)
    mde = pymde_amd.MDE(n, 2, torch.tensor(edges, device=DEV), f)
    torch.manual_seed(0)
    X0 = pymde_amd.Centered().initialization(n, 2, device=DEV) * 10
    Xt = X0.clone().requires_grad_(True)
    E = mde.average_distortion(Xt)
    E.backward()
    wE, wgrad = oracle.average_distortion(edges, X0.cpu().numpy(), oracle.func("L_HUBER", dev, None, (1.0,)))
    assert float(E) == pytest.approx(wE, rel=1e-5)
    assert_grad_close(Xt.grad.cpu().numpy(), wgrad)
    mde.embed(X=X0, max_iter=30)
    Es = np.array(mde.solve_stats.average_distortions)
    assert Es[-1] < 0.5 * Es[0] and abs(float(mde.X.mean())) < 1e-4


def test_config3_dense_pairs_take_the_ring_kernel():
    """configs[2] at the density of bench.py --config 3 (40k nodes, tens of millions of sampled pairs):
    the table fits L2, but with this many half-edges the LDS-ring kernel is chosen anyway -- tall row
    blocks x column groups, entries ordered by column inside a chunk -- and reproduces the oracle;
    integer hop counts travel as a codebook when there are few enough of them."""
    import pymde_amd
    rng = np.random.default_rng(5)
    n, p = 40000, 12_000_000
    i = rng.integers(0, n, p)
    j = (i + 1 + rng.integers(0, n - 1, p)) % n
    key = np.unique(np.minimum(i, j).astype(np.int64) * n + np.maximum(i, j))
    edges = np.stack([key // n, key % n], 1)
    X0 = (rng.standard_normal((n, 2)) * 3).astype(np.float32)
    for ndist in (5, 40):
        dev = (1.0 + rng.integers(0, ndist, len(edges))).astype(np.float32)
        f = pymde_amd.losses.Huber(torch.tensor(dev, device=DEV), 1.0)
        mde = pymde_amd.MDE(n, 2, torch.tensor(edges, device=DEV), f)
        Xt = torch.tensor(X0, device=DEV, requires_grad=True)
        E = mde.average_distortion(Xt)
        E.backward()
        st = mde._binding().struct(2)
        assert st.layout == 1, "dense pairs: the ring layout should have been chosen"
        wE, wgrad = oracle.average_distortion(edges, X0, oracle.func("L_HUBER", dev, None, (1.0,)))
        assert float(E) == pytest.approx(wE, rel=1e-5)
        assert_grad_close(Xt.grad.cpu().numpy(), wgrad)
        mde2 = pymde_amd.MDE(n, 2, torch.tensor(edges, device=DEV), f)
        Xt2 = torch.tensor(X0, device=DEV, requires_grad=True)
        E2 = mde2.average_distortion(Xt2)
        E2.backward()
        assert torch.equal(Xt2.grad, Xt.grad) and torch.equal(E2.detach(), E.detach())


def test_config4_full_size_against_oracle_and_invariants():
    """configs[3], the headline: n = 1M, |E| = 50M, d = 2, Log1p -- the LDS column-panel kernel
    against the OpenMP oracle on the full problem, plus invariants."""
    import bench
    import pymde_amd
    from pymde_amd import distributed
    from pymde_amd.average_distortion import Binding, EdgePlan, fused_evaluate
    dev = torch.device(DEV, 0)
    edges, w, X = bench.make_workload(dev)
    n, d, p = X.shape[0], 2, edges.shape[0]
    f = pymde_amd.penalties.Log1p(w)
    binding = Binding(EdgePlan(n, edges), f)
    buf = torch.zeros(n * d + 1, device=dev)
    fused_evaluate(binding, X, buf[:n * d].view(n, d), buf[n * d:])
    assert binding.struct(d).layout == 1  # the panel kernel is what runs at this size
    wE, wgrad = oracle.average_distortion(edges.cpu().numpy(), X.cpu().numpy(),
                                          oracle.func("LOG1P", w.cpu().numpy(), None, (1.5,)))
    assert float(buf[n * d]) == pytest.approx(wE, rel=1e-5)
    assert_grad_close(buf[:n * d].view(n, d).cpu().numpy(), wgrad)
    # translation invariance and zero net force
    buf2 = torch.zeros_like(buf)
    fused_evaluate(binding, X + torch.tensor([3.0, -2.0], device=dev), buf2[:n * d].view(n, d), buf2[n * d:])
    assert float(buf2[n * d]) == pytest.approx(float(buf[n * d]), rel=1e-5)
    assert buf[:n * d].view(n, d).double().sum(0).abs().max().item() < 1e-9 * n
    # bitwise reproducible; 4-way vertex-range sharding reproduces the unsharded gradient bitwise
    buf3 = torch.zeros_like(buf)
    fused_evaluate(binding, X, buf3[:n * d].view(n, d), buf3[n * d:])
    assert torch.equal(buf3, buf)
    bounds = distributed.shard_bounds(n, edges, 4)
    total = torch.zeros_like(buf)
    for r in range(4):
        lo, hi = distributed.shard_range(bounds, r)
        part = torch.zeros_like(buf)
        fused_evaluate(Binding(EdgePlan(n, edges, lo, hi), f), X, part[:n * d].view(n, d), part[n * d:])
        total += part
    np.testing.assert_allclose(total[:n * d].cpu().numpy(), buf[:n * d].cpu().numpy(), rtol=1e-5, atol=1e-12)
    assert float(total[n * d]) == pytest.approx(float(buf[n * d]), rel=1e-6)
    # ... and the 4-way sharded ring result against the ORACLE at the kernel tolerances
    assert float(total[n * d]) == pytest.approx(wE, rel=1e-5)
    assert_grad_close(total[:n * d].view(n, d).cpu().numpy(), wgrad)


def test_config4b_pushpull_full_size_against_oracle():
    """SURVEY 8d config 4b at full size: n = 1M, |E| = 50M, d = 2, PushAndPull(Log1p, Log) with the
    last third of the edges repulsive (w = -1) -- the LDS-ring kernel (compile-time functor pair,
    codebook stream of three values) against the OpenMP oracle, unsharded and as an 8-way shard."""
    import bench
    import pymde_amd
    from pymde_amd import distributed
    from pymde_amd.average_distortion import Binding, EdgePlan, fused_evaluate
    dev = torch.device(DEV, 0)
    edges, w, X = bench.make_workload(dev)
    n, d, p = X.shape[0], 2, edges.shape[0]
    w = w.clone()
    w[(2 * p) // 3:] = -1.0
    pen = pymde_amd.penalties
    f = pen.PushAndPull(w, pen.Log1p, pen.Log)
    binding = Binding(EdgePlan(n, edges), f)
    buf = torch.zeros(n * d + 1, device=dev)
    fused_evaluate(binding, X, buf[:n * d].view(n, d), buf[n * d:])
    assert binding.struct(d).layout == 1 and binding.codebook
    wE, wgrad = oracle.average_distortion(edges.cpu().numpy(), X.cpu().numpy(),
                                          oracle.func("LOG1P", w.cpu().numpy(), None, (1.5,), "LOG", (1.0,)))
    assert float(buf[n * d]) == pytest.approx(wE, rel=1e-5)
    assert_grad_close(buf[:n * d].view(n, d).cpu().numpy(), wgrad)
    bounds = distributed.shard_bounds(n, edges, 8)
    total = torch.zeros_like(buf)
    for r in range(8):
        lo, hi = distributed.shard_range(bounds, r)
        part = torch.zeros_like(buf)
        fused_evaluate(Binding(EdgePlan(n, edges, lo, hi), f), X, part[:n * d].view(n, d), part[n * d:])
        total += part
    assert float(total[n * d]) == pytest.approx(wE, rel=1e-5)
    assert_grad_close(total[:n * d].view(n, d).cpu().numpy(), wgrad)


def test_config4_d3_codebook_and_fp32_streams_full_size_against_oracle():
    """50M edges through the two parameter streams of the LDS-ring kernel the headline test does not take:
    d = 3 with PushAndPull weights {1, 2, -1} (the codebook in the two spare bits of the packed word at d = 3;
    n = 250k, out-degree 200 -- at n = 1M and d = 3 a pair of wave iterations does not fit the chunk window
    and the CSR kernel runs), and the config-4 graph at d = 2 with continuous weights (4 bytes per half-edge
    next to the packed word, NaN / Inf fix-up in the kernel) -- both against the OpenMP oracle."""
    import bench
    import pymde_amd
    from pymde_amd.average_distortion import Binding, EdgePlan, fused_evaluate
    dev = torch.device(DEV, 0)
    pen = pymde_amd.penalties
    # d = 3, three distinct weights
    edges3, w3, X3 = bench.make_workload(dev, n=250000, deg=200, d=3)
    n3, p3 = X3.shape[0], edges3.shape[0]
    w3 = w3.clone()
    w3[(2 * p3) // 3:] = -1.0
    b3 = Binding(EdgePlan(n3, edges3), pen.PushAndPull(w3, pen.Log1p, pen.Log))
    buf = torch.zeros(n3 * 3 + 1, device=dev)
    fused_evaluate(b3, X3, buf[:n3 * 3].view(n3, 3), buf[n3 * 3:])
    assert b3.struct(3).layout == 1 and b3.codebook
    wE, wgrad = oracle.average_distortion(edges3.cpu().numpy(), X3.cpu().numpy(),
                                          oracle.func("LOG1P", w3.cpu().numpy(), None, (1.5,), "LOG", (1.0,)))
    assert float(buf[n3 * 3]) == pytest.approx(wE, rel=1e-5)
    assert_grad_close(buf[:n3 * 3].view(n3, 3).cpu().numpy(), wgrad)
    del b3, buf, edges3, w3, X3
    # d = 2, continuous weights: no codebook
    edges, w, X2 = bench.make_workload(dev)
    n, p = X2.shape[0], edges.shape[0]
    plan = EdgePlan(n, edges)
    e_np = edges.cpu().numpy()
    g = torch.Generator(device=dev).manual_seed(5)
    wc = torch.rand(p, device=dev, generator=g) * 1.5 + 0.25
    b2 = Binding(plan, pen.Log1p(wc))
    buf = torch.zeros(n * 2 + 1, device=dev)
    fused_evaluate(b2, X2, buf[:n * 2].view(n, 2), buf[n * 2:])
    assert b2.struct(2).layout == 1 and not b2.codebook
    wE, wgrad = oracle.average_distortion(e_np, X2.cpu().numpy(), oracle.func("LOG1P", wc.cpu().numpy(), None, (1.5,)))
    assert float(buf[n * 2]) == pytest.approx(wE, rel=1e-5)
    assert_grad_close(buf[:n * 2].view(n, 2).cpu().numpy(), wgrad)


def test_config5_high_dim_standardized():
    """configs[4]: n = 500k, |E| = 20M, d = 128, Standardized (f32 MFMA Gram + projection).
    The gradient is checked against the oracle on an edge sub-sample; the full-size evaluation
    through invariants."""
    import pymde_amd
    from pymde_amd.average_distortion import Binding, EdgePlan, fused_evaluate
    dev = torch.device(DEV, 0)
    n, d, deg = 500_000, 128, 40
    gen = torch.Generator(device=dev)
    gen.manual_seed(0)
    src = torch.arange(n, device=dev).repeat_interleave(deg)
    dst = torch.randint(0, n - 1, (n * deg,), device=dev, generator=gen)
    dst += (dst >= src).long()
    edges = torch.stack([torch.minimum(src, dst), torch.maximum(src, dst)], 1).contiguous()
    w = 1.0 + (torch.rand(n * deg, device=dev, generator=gen) < 0.3).float()
    std = pymde_amd.Standardized()
    torch.manual_seed(0)
    X = std.initialization(n, d, device=dev)
    G = (X.double().T @ X.double() / n).cpu().numpy()
    np.testing.assert_allclose(G, np.eye(d), atol=5e-5)            # MFMA Gram + Newton-Schulz retraction
    assert X.mean(0).abs().max().item() < 1e-5
    # full-size fused evaluation (20M edges, 2 KB of gathers per edge)
    f = pymde_amd.penalties.Quadratic(w)
    binding = Binding(EdgePlan(n, edges), f)
    buf = torch.zeros(n * d + 1, device=dev)
    grad = buf[:n * d].view(n, d)
    fused_evaluate(binding, X, grad, buf[n * d:])
    E = float(buf[n * d])
    # Quadratic: E = (1/p) sum w ||x_i - x_j||^2 = (2/p) tr(X^T L X); grad = (2/p) L X, so <grad, X> = 2 E
    assert float((grad.double() * X.double()).sum()) == pytest.approx(2 * E, rel=1e-4)
    assert grad.double().sum(0).abs().max().item() < 1e-7 * n
    # tangent projection is orthogonal to the constraint normal space: X^T Z_t symmetric-part = 0
    Zt = std.project_onto_tangent_space(X, grad.clone(), inplace=True)
    A = (Zt.double().T @ X.double() / n).cpu().numpy()
    assert np.abs(A).max() < 1e-6 * max(1.0, float(grad.abs().max()) * n ** 0.5)
    # oracle on a sub-sample of 200k edges over the first 50k vertices
    m = 50_000
    sel = ((edges[:, 0] < m) & (edges[:, 1] < m)).nonzero().squeeze(1)[:200_000]
    es, ws = edges[sel].contiguous(), w[sel].contiguous()
    Xs = X[:m].contiguous()
    bs = Binding(EdgePlan(m, es), pymde_amd.penalties.Log1p(ws))
    out = torch.zeros(m * d + 1, device=dev)
    fused_evaluate(bs, Xs, out[:m * d].view(m, d), out[m * d:])
    wE, wgrad = oracle.average_distortion(es.cpu().numpy(), Xs.cpu().numpy(),
                                          oracle.func("LOG1P", ws.cpu().numpy(), None, (1.5,)))
    assert float(out[m * d]) == pytest.approx(wE, rel=1e-5)
    assert_grad_close(out[:m * d].view(m, d).cpu().numpy(), wgrad)


def test_config5_full_size_against_oracle():
    """configs[4] at FULL size against the oracle: n = 500k, |E| = 20M, d = 128, Quadratic and Log1p
    (the OpenMP oracle on 8 threads keeps 8 x 512 MB of per-thread gradient accumulators)."""
    import pymde_amd
    from pymde_amd.average_distortion import Binding, EdgePlan, fused_evaluate
    dev = torch.device(DEV, 0)
    n, d, deg = 500_000, 128, 40
    gen = torch.Generator(device=dev)
    gen.manual_seed(0)
    src = torch.arange(n, device=dev).repeat_interleave(deg)
    dst = torch.randint(0, n - 1, (n * deg,), device=dev, generator=gen)
    dst += (dst >= src).long()
    edges = torch.stack([torch.minimum(src, dst), torch.maximum(src, dst)], 1).contiguous()
    w = 1.0 + (torch.rand(n * deg, device=dev, generator=gen) < 0.3).float()
    torch.manual_seed(0)
    X = pymde_amd.Standardized().initialization(n, d, device=dev)
    plan = EdgePlan(n, edges)
    e_np, w_np, X_np = edges.cpu().numpy(), w.cpu().numpy(), X.cpu().numpy()
    L = oracle.lib()
    L.oracle_set_num_threads(min(8, L.oracle_num_threads()))
    buf = torch.zeros(n * d + 1, device=dev)
    for name, f, scal in (("QUADRATIC", pymde_amd.penalties.Quadratic(w), ()), ("LOG1P", pymde_amd.penalties.Log1p(w), (1.5,))):
        buf.zero_()
        fused_evaluate(Binding(plan, f), X, buf[:n * d].view(n, d), buf[n * d:])
        wE, wgrad = oracle.average_distortion(e_np, X_np, oracle.func(name, w_np, None, scal))
        assert float(buf[n * d]) == pytest.approx(wE, rel=1e-5), name
        assert_grad_close(buf[:n * d].view(n, d).cpu().numpy(), wgrad)


def test_config5_size_band_graph_renumbered_against_oracle(monkeypatch):
    """configs[4]'s shape on a graph WITH locality that the numbering hides: n = 500k, d = 128, neighbours within 100
    rows of a hidden order, vertices renumbered at random.  The plan adopts a breadth-first processing order on its
    first evaluation (`mde_plan_row_order`); the gradient equals the one computed without any order BIT FOR BIT, three
    evaluations agree bitwise, and both agree with the oracle at full size (~16.5M edges)."""
    import pymde_amd
    from pymde_amd.average_distortion import Binding, EdgePlan, fused_evaluate
    dev = torch.device(DEV, 0)
    n, d, deg, window = 500_000, 128, 40, 100
    gen = torch.Generator(device=dev)
    gen.manual_seed(0)
    src = torch.arange(n, device=dev).repeat_interleave(deg)
    dst = (src + torch.randint(1, window + 1, (n * deg,), device=dev, generator=gen)) % n
    perm = torch.randperm(n, device=dev, generator=gen)
    e = perm[torch.stack([src, dst], 1)]
    edges = torch.unique(torch.stack([e.min(1).values, e.max(1).values], 1), dim=0).contiguous()
    p = edges.shape[0]
    w = 1.0 + (torch.rand(p, device=dev, generator=gen) < 0.3).float()
    torch.manual_seed(0)
    X = pymde_amd.Standardized().initialization(n, d, device=dev)
    f = pymde_amd.penalties.Log1p(w)

    def run(plan):
        buf = torch.zeros(n * d + 1, device=dev)
        fused_evaluate(Binding(plan, f), X, buf[:n * d].view(n, d), buf[n * d:])
        return buf

    monkeypatch.setenv("MDE_ROW_ORDER", "0")
    plain = EdgePlan(n, edges)
    ref = run(plain)
    assert not plain.row_order(0)["in_use"]
    monkeypatch.delenv("MDE_ROW_ORDER")
    plan = EdgePlan(n, edges)
    outs = [run(plan) for _ in range(3)]
    info = plan.row_order(1)
    assert info["in_use"] and info["mean_distance_after"] < 4 * window and info["mean_distance_before"] > n / 10
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
    assert torch.equal(outs[0][:n * d], ref[:n * d])
    L = oracle.lib()
    L.oracle_set_num_threads(min(8, L.oracle_num_threads()))
    wE, wgrad = oracle.average_distortion(edges.cpu().numpy(), X.cpu().numpy(),
                                          oracle.func("LOG1P", w.cpu().numpy(), None, (1.5,)))
    for out in (outs[0], ref):
        assert float(out[n * d]) == pytest.approx(wE, rel=1e-5)
    assert_grad_close(outs[0][:n * d].view(n, d).cpu().numpy(), wgrad)


def test_mid_size_problems_ask_the_cost_model():
    """Between the MNIST-sized problems and the benchmark shape (table in L2, fewer than 16 M half-edges) the layout is
    chosen by the cost model with both kernels' fixed costs and the FUNCTION's cost on the ring kernel priced (round 6;
    rounds 3-5 kept the CSR kernels there without asking): n = 100k at out-degree 50 with Log1p takes the LDS-ring
    layout, the same graph at out-degree 20 with PushAndPull (1.3 x per iteration on the ring) stays on the CSR
    kernels, a 20k-item problem stays there whatever the function -- and every one of them agrees with the oracle."""
    import bench
    import pymde_amd
    from pymde_amd.average_distortion import Binding, EdgePlan, fused_evaluate
    dev = torch.device(DEV, 0)
    pen = pymde_amd.penalties
    cases = [(100_000, 50, "log1p", True), (100_000, 20, "pushpull", False), (20_000, 20, "log1p", False),
             (150_000, 20, "log1p", True)]
    for n, deg, fname, want_ring in cases:
        for d in (2, 3):
            edges, w, X = bench.make_workload(dev, n=n, deg=deg, d=d)
            p = edges.shape[0]
            if fname == "pushpull":
                w = w.clone()
                w[(2 * p) // 3:] = -1.0
                f = pen.PushAndPull(w, pen.Log1p, pen.Log)
                fd = oracle.func("LOG1P", w.cpu().numpy(), None, (1.5,), "LOG", (1.0,))
            else:
                f = pen.Log1p(w)
                fd = oracle.func("LOG1P", w.cpu().numpy(), None, (1.5,))
            plan = EdgePlan(n, edges)
            b = Binding(plan, f)
            buf = torch.zeros(n * d + 1, device=dev)
            fused_evaluate(b, X, buf[:n * d].view(n, d), buf[n * d:])
            assert plan.ring_info()["built"] == want_ring, (n, deg, fname, d)
            assert (int(b.struct(d).layout) == 1) == want_ring
            wE, wgrad = oracle.average_distortion(edges.cpu().numpy(), X.cpu().numpy(), fd)
            assert float(buf[n * d]) == pytest.approx(wE, rel=1e-5), (n, deg, fname, d)
            assert_grad_close(buf[:n * d].view(n, d).cpu().numpy(), wgrad)


def test_links_near_the_diagonal_keep_the_csr_kernels():
    """A graph whose links stay near the diagonal of the vertex order (2/3 of them inside clusters of 1000 consecutive
    items: data sorted by class) serialises the ring kernel's consumer waves -- every wave's entries sit in the chunks
    of its own rows' clusters.  The layout builder measures how evenly the waves advance along the column sweep
    (k_ring_sweep_balance) and auto mode keeps the CSR kernels (round 6: 1.28 ms on the ring against 0.66 at n = 1M,
    0.22 against 0.05 at n = 100k); the same graph under a random renumbering of its vertices is as good as uniform
    and takes the ring.  Both against the oracle; the forced ring layout on the cluster graph as well."""
    import bench
    import pymde_amd
    from pymde_amd.average_distortion import Binding, EdgePlan, fused_evaluate
    dev = torch.device(DEV, 0)
    n, deg, d = 300_000, 50, 2
    edges, w, X = bench.make_workload(dev, n=n, deg=deg, d=d, graph="clusters")
    f = pymde_amd.penalties.PushAndPull(w, pymde_amd.penalties.Log1p, pymde_amd.penalties.Log)
    fd = oracle.func("LOG1P", w.cpu().numpy(), None, (1.5,), "LOG", (1.0,))
    gen = torch.Generator(device=dev)
    gen.manual_seed(1)
    perm = torch.randperm(n, device=dev, generator=gen)
    e2 = perm[edges]
    e2 = torch.stack([e2.min(1).values, e2.max(1).values], 1).contiguous()
    L = oracle.lib()
    L.oracle_set_num_threads(min(8, L.oracle_num_threads()))
    for name, e, want_ring, env in (("as given", edges, False, None), ("renumbered", e2, True, None), ("ring forced", edges, True, "1")):
        if env is not None:
            os.environ["MDE_PANEL"] = env
        try:
            plan = EdgePlan(n, e)
            b = Binding(plan, f)
            buf = torch.zeros(n * d + 1, device=dev)
            fused_evaluate(b, X, buf[:n * d].view(n, d), buf[n * d:])
        finally:
            os.environ.pop("MDE_PANEL", None)
        assert plan.ring_info()["built"] == want_ring, name
        wE, wgrad = oracle.average_distortion(e.cpu().numpy(), X.cpu().numpy(), fd)
        assert float(buf[n * d]) == pytest.approx(wE, rel=1e-5), name
        assert_grad_close(buf[:n * d].view(n, d).cpu().numpy(), wgrad)


def _ring_full_size_case(n, deg, d, make_f, oracle_func, runs=3, graph="uniform"):
    """>= 5e7 half-edge entries through the LDS-ring kernel: against the OpenMP oracle at the kernel
    tolerances, `runs` evaluations bitwise equal (a race in the ring protocol shows up as a few rows that
    differ from run to run -- the round-4 d = 3 race was invisible below ~1e7 entries)."""
    import bench
    from pymde_amd.average_distortion import Binding, EdgePlan, fused_evaluate
    dev = torch.device(DEV, 0)
    edges, w, X = bench.make_workload(dev, n=n, deg=deg, d=d, graph=graph)
    p = edges.shape[0]
    assert 2 * p >= 5 * 10 ** 7
    f, fd = make_f(w, p, dev), None
    b = Binding(EdgePlan(n, edges), f)
    bufs = []
    for _ in range(runs):
        buf = torch.zeros(n * d + 1, device=dev)
        fused_evaluate(b, X, buf[:n * d].view(n, d), buf[n * d:])
        bufs.append(buf)
    assert b.struct(d).layout == 1, "the LDS-ring layout should have been chosen"
    for other in bufs[1:]:
        assert torch.equal(other, bufs[0]), "two evaluations differ bitwise"
    fd = oracle_func(f, w.cpu().numpy())
    wE, wgrad = oracle.average_distortion(edges.cpu().numpy(), X.cpu().numpy(), fd)
    assert float(bufs[0][n * d]) == pytest.approx(wE, rel=1e-5)
    assert_grad_close(bufs[0][:n * d].view(n, d).cpu().numpy(), wgrad)
    return b


@pytest.mark.parametrize("ndist,d", [(40, 2), (200, 2), (255, 3)])
def test_byte_index_parameter_stream_full_size(ndist, d):
    """The byte-index parameter stream (round 5; <= 255 distinct per-edge parameters: 5 bytes per half-edge, the
    value table in the 1 KB behind the kernel's ring) on the ring kernel at full size: losses.Huber with `ndist`
    distinct integer deviations -- what preserve_distances on a graph produces [ref: pymde/recipes.py:194-215,
    losses.py:101-125] -- on the config-4 graph (d = 2: 50M edges) and at d = 3 (25M edges), against the oracle,
    three evaluations bitwise equal; 256 distinct values fall back to the fp32 stream with the same result."""
    import pymde_amd
    los = pymde_amd.losses
    n, deg = (1_000_000, 50) if d == 2 else (250_000, 100)
    holder = {}

    def mk(w, p, dev):
        g = torch.Generator(device=dev).manual_seed(7)
        holder["dev"] = 1.0 + torch.randint(0, ndist, (p,), device=dev, generator=g).float()
        return los.Huber(holder["dev"], 1.0)
    b = _ring_full_size_case(n, deg, d, mk, lambda f, w: oracle.func("L_HUBER", holder["dev"].cpu().numpy(), None, (1.0,)))
    assert b.byte_stream and not b.codebook and b.stream_kind == "byte index"
    if d == 3:
        # one value more than the table holds: the fp32 stream, same numbers
        def mk2(w, p, dev):
            g = torch.Generator(device=dev).manual_seed(7)
            holder["dev"] = 1.0 + torch.randint(0, 256, (p,), device=dev, generator=g).float()
            return los.Huber(holder["dev"], 1.0)
        b2 = _ring_full_size_case(n, deg, d, mk2, lambda f, w: oracle.func("L_HUBER", holder["dev"].cpu().numpy(), None, (1.0,)),
                                  runs=1)
        assert not b2.byte_stream and not b2.codebook and b2.stream_kind == "fp32"


@pytest.mark.parametrize("case", ["pen_huber_d3", "pen_quadratic_d3", "loss_huber_d3", "log1p_fp32_d3",
                                  "runtime_logistic_d1", "runtime_power_d4", "pen_cubic_scalar_d2"])
def test_ring_units_full_size_against_oracle_and_bitwise(case):
    """Every translation unit that instantiates the ring kernel (mde_ring_k_*.hip) at full size, in the
    dimensions and parameter forms the headline tests do not take: the penalty unit and the loss unit at
    d = 3 (codebook streams), the Log1p unit's fp32 stream at d = 3, the run-time functor at d = 1 and
    d = 4 (fp32 streams), and a scalar-parameter form at d = 2.  25M edges = 5e7 entries each."""
    import pymde_amd
    pen, los = pymde_amd.penalties, pymde_amd.losses
    n, deg = 250_000, 100

    def cont(w, p, dev, lo=0.25, hi=1.75, seed=11):
        g = torch.Generator(device=dev).manual_seed(seed)
        return torch.rand(p, device=dev, generator=g) * (hi - lo) + lo

    if case == "pen_huber_d3":
        b = _ring_full_size_case(n, deg, 3, lambda w, p, dev: pen.Huber(w, 0.5),
                                 lambda f, w: oracle.func("HUBER", w, None, (0.5,)))
        assert b.codebook
    elif case == "pen_quadratic_d3":
        b = _ring_full_size_case(n, deg, 3, lambda w, p, dev: pen.Quadratic(w),
                                 lambda f, w: oracle.func("QUADRATIC", w))
        assert b.codebook
    elif case == "loss_huber_d3":
        # deviations {1, 2}: the loss unit's codebook stream at d = 3
        b = _ring_full_size_case(n, deg, 3, lambda w, p, dev: los.Huber(w, 1.0),
                                 lambda f, w: oracle.func("L_HUBER", w, None, (1.0,)))
        assert b.codebook
    elif case == "log1p_fp32_d3":
        holder = {}

        def mk(w, p, dev):
            holder["w"] = cont(w, p, dev)
            return pen.Log1p(holder["w"])
        b = _ring_full_size_case(n, deg, 3, mk, lambda f, w: oracle.func("LOG1P", holder["w"].cpu().numpy(), None, (1.5,)))
        assert not b.codebook
    elif case == "runtime_logistic_d1":
        holder = {}

        def mk(w, p, dev):
            holder["w"] = cont(w, p, dev)
            return pen.Logistic(holder["w"], 0.5, 3.0)
        b = _ring_full_size_case(n, deg, 1, mk, lambda f, w: oracle.func("LOGISTIC", holder["w"].cpu().numpy(), None, (0.5, 3.0)))
        assert not b.codebook
    elif case == "runtime_power_d4":
        holder = {}

        def mk(w, p, dev):
            holder["w"] = cont(w, p, dev)
            return pen.Power(holder["w"], 2.5)
        b = _ring_full_size_case(n, deg, 4, mk, lambda f, w: oracle.func("POWER", holder["w"].cpu().numpy(), None, (2.5,)))
        assert not b.codebook
    else:
        # one scalar weight for every edge (the LIN = false form: padding lanes are masked)
        _ring_full_size_case(n, deg, 2, lambda w, p, dev: pen.Cubic(torch.tensor([1.5], device=dev)),
                             lambda f, w: oracle.func("CUBIC", np.array([1.5], np.float32)))


@pytest.mark.parametrize("case", ["d3_n1m", "n2m", "hub", "powerlaw", "powerlaw_d3_pushpull"])
def test_ring_beyond_the_old_feasibility_rule_full_size(case):
    """Round 6: the regimes the ring layout's feasibility rule of rounds 3-5 sent to the CSR kernels (>= 1.1 ms per
    1e8 half-edges) now run on the ring kernel in AUTO mode -- each at full size against the OpenMP oracle, three
    evaluations bitwise equal:
      d3_n1m    d = 3 at n = 1M, 50M edges (22 entries per consumer wave and chunk against the old threshold of 32)
      n2m       n = 2M at out-degree 50, 100M edges (25 against 32): half-filled wave iterations
      hub       the config-4 graph with one vertex of degree 5e5: the hub row is peeled off to k_hub_rows
      powerlaw  preferential attachment at n = 1M, 50M edges (degrees fall along the vertex order, hubs of
                thousands of half-edges): hubs peeled, row blocks dealt by degree (every entry adds f / 2)
      powerlaw_d3_pushpull  the same graph at d = 3 with PushAndPull weights {1, 2, -1}."""
    import pymde_amd
    pen = pymde_amd.penalties
    log1p = (lambda w, p, dev: pen.Log1p(w), lambda f, w: oracle.func("LOG1P", w, None, (1.5,)))
    if case == "d3_n1m":
        b = _ring_full_size_case(1_000_000, 50, 3, *log1p)
        info = b.plan.ring_info()
        assert not info["permuted"] and info["hub_rows"] == 0
    elif case == "n2m":
        b = _ring_full_size_case(2_000_000, 50, 2, *log1p)
        info = b.plan.ring_info()
        assert info["row_blocks"] == 256 and not info["permuted"] and info["hub_rows"] == 0
    elif case == "hub":
        b = _ring_full_size_case(1_000_000, 50, 2, *log1p, graph="hub")
        info = b.plan.ring_info()
        assert info["hub_rows"] == 1 and info["hub_half_edges"] >= 500_000 and not info["permuted"]
    elif case == "powerlaw":
        b = _ring_full_size_case(1_000_000, 50, 2, *log1p, graph="powerlaw")
        info = b.plan.ring_info()
        assert info["hub_rows"] > 10 and info["permuted"]
    else:
        holder = {}

        def mk(w, p, dev):
            holder["w"] = w.clone()
            holder["w"][(2 * p) // 3:] = -1.0
            return pen.PushAndPull(holder["w"], pen.Log1p, pen.Log)
        b = _ring_full_size_case(1_000_000, 50, 3, mk,
                                 lambda f, w: oracle.func("LOG1P", holder["w"].cpu().numpy(), None, (1.5,), "LOG", (1.0,)),
                                 graph="powerlaw")
        info = b.plan.ring_info()
        assert info["hub_rows"] > 10 and info["permuted"] and b.codebook


def test_config4_survey_seed_tensors_loss_and_gradient_against_oracle():
    """SURVEY 8d's config 4a EXACTLY as the survey writes it (bench.py --survey-seed: numpy default_rng(0) edges and
    weights, torch.manual_seed(0) CPU randn X -- the tensors a reference-side run of the recipe builds): loss AND
    gradient of the HIP path against the oracle on all 50M edges (round 5's --survey-seed record compared the loss)."""
    import bench
    import pymde_amd
    from pymde_amd.average_distortion import Binding, EdgePlan, fused_evaluate
    dev = torch.device(DEV, 0)
    edges, w, X = bench.make_workload_survey(dev)
    n, d = X.shape
    b = Binding(EdgePlan(n, edges), pymde_amd.penalties.Log1p(w))
    buf = torch.zeros(n * d + 1, device=dev)
    fused_evaluate(b, X, buf[:n * d].view(n, d), buf[n * d:])
    assert b.struct(d).layout == 1 and b.codebook
    wE, wgrad = oracle.average_distortion(edges.cpu().numpy(), X.cpu().numpy(), oracle.func("LOG1P", w.cpu().numpy(), None, (1.5,)))
    assert float(buf[n * d]) == pytest.approx(wE, rel=1e-5)
    assert_grad_close(buf[:n * d].view(n, d).cpu().numpy(), wgrad)


def test_ring_layout_fuzz_against_the_csr_kernels():
    """Random problems (n = 2k .. 600k, out-degree 3 .. 120, d = 1 .. 4, uniform / preferential-attachment / planted-cluster /
    hub graphs, five kinds of function incl. continuous weights) through the ring layout forced, the ring layout with
    the round-5 row map, and auto mode, against the CSR kernels on the same tensors: no fault, every evaluation
    reproducible, gradient and loss equal to rounding (tools/r6_ring_fuzz.py; round 6 found an unseen stream overflow
    of the layout builder this way)."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("MDE_PANEL", "MDE_RING_ASSIGN")}
    out = subprocess.run([sys.executable, os.path.join(root, "tools", "r6_ring_fuzz.py"), "24", "7"], env=env,
                         capture_output=True, text=True, timeout=900)
    assert out.returncode == 0 and "ok, worst" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]


def test_bench_plain_run_times_its_steps_and_dumps_what_they_computed(tmp_path):
    """`bench.py --steps K` without --full: one timed region of exactly K steps, the headline fields only, and
    --dump-outputs writes the last step's gradient and loss -- equal to the oracle's on the same seeded inputs."""
    import json
    import subprocess
    import sys
    import bench
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    n = 20000
    out = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                          "--n", str(n), "--dump-outputs", str(tmp_path)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    rec = json.loads(lines[0])
    assert rec["steps"] == 3 and rec["blocks"] == 1 and len(rec["ms_per_step_blocks"]) == 1
    assert rec["ms_per_step"] > 0 and rec["unit"] == "edges/s/iter" and rec["higher_is_better"] is True
    assert rec["dtype"] == "f32" and "roofline" not in rec and "cpu_baseline" not in rec
    grad, loss = np.load(tmp_path / "grad.npy"), np.load(tmp_path / "loss.npy")
    assert grad.dtype == np.float32 and grad.shape == (n, 2) and loss.dtype == np.float32 and loss.shape == (1,)
    edges, w, X = bench.make_workload(torch.device(DEV, 0), n=n)
    wE, wgrad = oracle.average_distortion(edges.cpu().numpy(), X.cpu().numpy(), oracle.func("LOG1P", w.cpu().numpy(), None, (1.5,)))
    assert float(loss[0]) == pytest.approx(wE, rel=1e-5)
    assert_grad_close(grad, wgrad)

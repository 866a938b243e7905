"""Isotonic regression (csrc/mde_isotonic.hip) and ordinal MDS (pymde_amd.ordinal) at user sizes.

    python tools/ordinal_scale.py [--sizes 1000000,12500000,50000000] [--runs 5] [--rows 5000] [--no-embed]

Per size p, medians (min - max) of --runs synchronised calls after one warm-up: ``mde_isotonic`` (through
``isotonic.run``, the work buffer allocated once) on an already nondecreasing sequence (p blocks: nothing
shrinks, the compaction's worst case), iid noise (one block) and a noisy ramp; beside it on the same length
``torch.sort`` of the noise, a float64 ``torch.cumsum``, one ``average_distortion`` evaluation (forward and
backward) of a ``Quadratic`` problem with p random edges, and ``scipy.optimize.isotonic_regression`` of the noisy
ramp on the host.  The regression and the evaluation are called alternately.

Then one round of ``OrdinalMDE`` over all pairs of --rows rows of the mixture of tools/mnist_like.py (10 centres
~ N(0, 4 I) in R^784, unit noise) with deviations D^3, split into its stages, and ``OrdinalMDE.embed()`` end to
end."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pymde_amd  # noqa: E402
from pymde_amd import isotonic  # noqa: E402

DEV = "cuda"


def wall(fn, *a, **kw):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn(*a, **kw)
    torch.cuda.synchronize()
    return out, time.perf_counter() - t


def timed(fn, runs):
    fn()
    return [wall(fn)[1] for _ in range(runs)]


def ms(times):
    return "%9.3f ms (%.3f - %.3f)" % (1e3 * statistics.median(times), 1e3 * min(times), 1e3 * max(times))


def regression_rows(p, runs):
    g = torch.Generator(device=DEV)
    g.manual_seed(p)
    noise = torch.randn(p, generator=g, device=DEV)
    inputs = {"nondecreasing": torch.arange(p, device=DEV, dtype=torch.float32) / p,
              "iid noise": noise,
              "noisy ramp": torch.arange(p, device=DEV, dtype=torch.float32) + 3.0 * noise}
    work = isotonic.work_buffer(p, DEV)
    out = torch.empty(p, dtype=torch.float32, device=DEV)
    n = max(int(2.5 * p ** 0.5), 1000)
    e = pymde_amd.preprocess.sample_edges(n, p, seed=0, device=DEV)
    mde = pymde_amd.MDE(n, 2, e, pymde_amd.losses.Quadratic(torch.rand(p, device=DEV) + 0.5))
    X = torch.randn(n, 2, device=DEV, requires_grad=True)

    def evaluate():
        X.grad = None
        mde.average_distortion(X).backward()
    print("p = %d (work buffer %.1f MB; the Quadratic problem has n = %d)" % (p, work.numel() / 1e6, n), flush=True)
    evaluate()
    for name, y in inputs.items():
        isotonic.run(y, None, out, work)
        t_iso, t_eval = [], []
        for _ in range(runs):                       # alternately
            t_iso.append(wall(isotonic.run, y, None, out, work)[1])
            t_eval.append(wall(evaluate)[1])
        blocks = int(torch.unique_consecutive(out).numel())
        print("  mde_isotonic, %-14s %s   %d blocks | average_distortion fwd+bwd %s" % (
            name + ":", ms(t_iso), blocks, ms(t_eval)), flush=True)
    print("  torch.sort (noise):          %s" % ms(timed(lambda: torch.sort(noise), runs)))
    wide = noise.double()
    print("  torch.cumsum (float64):      %s" % ms(timed(lambda: torch.cumsum(wide, 0), runs)), flush=True)
    from scipy.optimize import isotonic_regression
    host = inputs["noisy ramp"].cpu().numpy().astype(np.float64)
    times = []
    for _ in range(3 if p <= 20_000_000 else 1):
        t = time.perf_counter()
        isotonic_regression(host)
        times.append(time.perf_counter() - t)
    print("  scipy isotonic_regression on the host (noisy ramp, float64, %d runs): %s" % (len(times), ms(times)),
          flush=True)


def mixture(n, nf=784):
    rng = np.random.default_rng(0)
    centers = rng.standard_normal((10, nf)) * 2.0
    labels = rng.integers(0, 10, n)
    return torch.tensor((centers[labels] + rng.standard_normal((n, nf))).astype(np.float32), device=DEV)


def ordinal_rows(rows, runs, embed):
    pymde_amd.seed(0)
    data = mixture(rows)
    graph = pymde_amd.recipes.distances(data)
    deviations = graph.distances.double() ** 3
    mde, t_build = wall(pymde_amd.OrdinalMDE, rows, 2, graph.edges, deviations)
    p = int(graph.edges.shape[0])
    print("OrdinalMDE over all %d pairs of %d rows, deviations D^3: %d distinct (construction with the sort %.2f s)"
          % (p, rows, mde.n_groups, t_build), flush=True)
    inner = mde.problem.distortion_function
    X = mde.problem.embed(max_iter=30)
    d = mde._distances(X)
    ranked = d[mde._order]
    values = mde._group_means(ranked)
    regressed = mde._regress(values)
    fit = mde._expand(regressed)
    scaled = fit / float(fit.double().pow(2).mean().sqrt())
    Xg = X.clone().requires_grad_(True)

    def evaluate():
        Xg.grad = None
        mde.problem.average_distortion(Xg).backward()

    def write_back():
        inner.deviations.copy_(scaled)
        evaluate()
    print("  distances:                                   %s" % ms(timed(lambda: mde._distances(X), runs)))
    print("  gather into rank order:                      %s" % ms(timed(lambda: d[mde._order], runs)))
    print("  means of the %9d tie groups:            %s" % (
        mde.n_groups, ms(timed(lambda: mde._group_means(ranked), runs))))
    print("  regression over the groups:                  %s" % ms(timed(lambda: mde._regress(values), runs)))
    print("  groups to edges, back to edge order:         %s" % ms(timed(lambda: mde._expand(regressed), runs)))
    print("  stress-1 (two float64 sums, one read-back):  %s" % ms(timed(lambda: mde._stress(d, fit), runs)))
    t_write, t_plain = [], []
    write_back()
    for _ in range(runs):                           # alternately
        t_write.append(wall(write_back)[1])
        t_plain.append(wall(evaluate)[1])
    print("  deviations.copy_ + first evaluation:         %s" % ms(t_write))
    print("  an evaluation with the stream in place:      %s" % ms(t_plain))
    times = []
    for _ in range(runs):
        inner.deviations.copy_(scaled)
        times.append(wall(mde.problem.embed, X, max_iter=15)[1])
    print("  inner embed(X, max_iter=15) (%d iterations):  %s" % (mde.problem.solve_stats.iterations, ms(times)),
          flush=True)
    if embed:
        for rep in range(2):
            pymde_amd.seed(0)
            _, t = wall(mde.embed)
            print("  embed() end to end, run %d: %.2f s, %d rounds after the metric start, stress-1 %.4g -> %.4g" % (
                rep, t, mde.rounds_, mde.stress_history[0], mde.stress_))
        from scipy.stats import spearmanr
        pick = torch.randperm(p, device=DEV)[:200000]
        true = graph.distances[pick].cpu().numpy()
        rho_metric = spearmanr(true, mde.problem.distances(X)[pick].cpu().numpy())[0]
        rho = spearmanr(true, mde.problem.distances(mde.X)[pick].cpu().numpy())[0]
        print("  Spearman of embedding and data distances on 200 000 pairs: after 30 metric iterations %.4f, "
              "after embed() %.4f" % (rho_metric, rho), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1000000,12500000,50000000")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--rows", type=int, default=5000)
    ap.add_argument("--no-embed", action="store_true")
    args = ap.parse_args()
    print("device: %s, leaf %d points" % (torch.cuda.get_device_name(0), isotonic.leaf()))
    for p in [int(s) for s in args.sizes.split(",") if s]:
        regression_rows(p, args.runs)
        torch.cuda.empty_cache()
    if args.rows:
        ordinal_rows(args.rows, args.runs, not args.no_embed)


if __name__ == "__main__":
    main()

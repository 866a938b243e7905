"""Dense MDE problems (pymde_amd.DenseMDE, mde_pair_loss) at user sizes: the time of one evaluation of the loss and
gradient over all pairs, beside parent-commit code on the same matrices in the same run.

    python tools/dense_mde_scale.py [--gram 20000x64,20000x784,70000x784] [--matrix 5000,20000] [--cycle 5000]
                                    [--out profiles/r15_dense_mde.txt]

Every figure is a warm-up call and then the median of three calls timed with a device synchronise on both sides, in
one process.

  Gram source     the stand-in of tools/mnist_like.py (a 10-component Gaussian mixture, centres N(0, 4 I), unit noise)
                  in R^nf, drawn on the GPU; the embedding is a random projection to two dimensions.
                  mde_pair_loss (kernels alone: the row norms, the walk, the fold, the total; losses.Quadratic and
                  losses.Absolute) beside mde_pair_moments on the same prepared rows and the same embedding:
                  pair_moments runs two Gram tiles per step (data and embedding) where pair_loss runs one and forms
                  the embedding distance from differences.  DenseMDE.average_distortion + backward is the public call.
  matrix source   the float32 [n, n] matrix of the same distances, read once per evaluation; at the first size beside
                  the edge-list MDE over all_edges(n) (MDE.average_distortion + backward, and the plan's build time).
  cycle           BASELINE config 1: a cycle graph, all pairs, losses.Quadratic, embed(max_iter=50) from the same start,
                  as the graph recipe's edge-list problem and as a DenseMDE over the matrix of hop counts.
No time is asserted anywhere."""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, calls=3):
    fn()                                    # warm-up
    times = []
    for _ in range(calls):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t)
    return sorted(times)[len(times) // 2], times


def mnist_like(n, nf, dev, components=10):
    g = torch.Generator(device=dev)
    g.manual_seed(n + nf)
    centres = 2.0 * torch.randn(components, nf, generator=g, device=dev)
    labels = torch.randint(0, components, (n,), generator=g, device=dev)
    data = torch.randn(n, nf, generator=g, device=dev)
    data += centres[labels]
    return data.contiguous()


def embedding_of(data, seed):
    g = torch.Generator(device=data.device)
    g.manual_seed(seed)
    X = data @ torch.randn(data.shape[1], 2, generator=g, device=data.device)
    return (X - X.mean(0)).contiguous()


def value_and_backward(problem, X):
    Xg = X.detach().clone().requires_grad_(True)
    problem.average_distortion(Xg).backward()
    return Xg.grad


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gram", default="20000x64,20000x784,70000x784")
    ap.add_argument("--matrix", default="5000,20000")
    ap.add_argument("--cycle", type=int, default=5000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import pymde_amd
    from pymde_amd import dense, losses, metrics, quality
    dev = torch.device("cuda", 0)
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    def line(name, med, times, base=None, note=""):
        ratio = "  = %.2f x %s" % (med / base[1], base[0]) if base else ""
        say("  %-52s %.6f %s%s%s" % (name, med, [round(t, 6) for t in times], ratio, note))

    quad, absolute = dense.loss_spec(losses.Quadratic), dense.loss_spec(losses.Absolute)
    say("tools/dense_mde_scale.py on %s; seconds, median of three calls after a warm-up [the three]"
        % torch.cuda.get_device_name(dev))
    with torch.cuda.device(dev):
        for shape in [v for v in args.gram.split(",") if v]:
            n, nf = (int(v) for v in shape.split("x"))
            data = mnist_like(n, nf, dev)
            X = embedding_of(data, n)
            A = metrics.translated_rows(data)[0]
            say("")
            say("Gram source: %d x %d mixture, embedding %d x 2 (%.3g ordered pairs)" % (n, nf, n, n * (n - 1.0)))
            mom = timed(lambda: quality._pair_moments(A, X))
            line("mde_pair_moments (two Gram tiles; parent commit)", *mom)
            base = ("mde_pair_moments", mom[0])
            for name, spec in (("Quadratic", quad), ("Absolute", absolute)):
                med, times = timed(lambda: dense._pair_loss(X, spec, A=A))
                line("mde_pair_loss %s (kernels alone)" % name, med, times, base,
                     "  (%.1f TF/s of Gram)" % (2.0 * n * n * nf / med / 1e12))
            problem = pymde_amd.DenseMDE(data, loss=losses.Quadratic)
            med, times = timed(lambda: value_and_backward(problem, X))
            line("DenseMDE.average_distortion + backward, Quadratic", med, times, base)
            del data, X, A, problem
            torch.cuda.empty_cache()
        first = True
        for n in [int(v) for v in args.matrix.split(",") if v]:
            data = mnist_like(n, 64, dev)
            X = embedding_of(data, n)
            Dm = torch.cdist(data.double(), data.double()).float().contiguous()
            Dm = (0.5 * (Dm + Dm.T)).contiguous()
            Dm.fill_diagonal_(0.0)
            say("")
            say("matrix source: %d x %d float32 distances (%.3g GB), embedding %d x 2" % (n, n, 4e-9 * n * n, n))
            base = None
            if first:
                t = time.perf_counter()
                edges = pymde_amd.all_edges(n).to(dev)
                deviations = Dm[edges[:, 0], edges[:, 1]].contiguous()
                mde = pymde_amd.MDE(n, 2, edges, losses.Quadratic(deviations))
                value_and_backward(mde, X)
                torch.cuda.synchronize()
                say("  edge-list MDE over all_edges(%d): %d edges (%.3g GB of edges), built and first evaluated in %.3f s"
                    % (n, edges.shape[0], 16e-9 * edges.shape[0], time.perf_counter() - t))
                med, times = timed(lambda: value_and_backward(mde, X))
                line("MDE.average_distortion + backward, Quadratic", med, times)
                base = ("edge-list MDE", med)
                del mde, edges, deviations
            for name, spec in (("Quadratic", quad), ("Absolute", absolute)):
                med, times = timed(lambda: dense._pair_loss(X, spec, Dm=Dm))
                line("mde_pair_loss %s (kernels alone)" % name, med, times, base,
                     "  (%.0f GB/s of the matrix)" % (4e-9 * n * n / med))
            problem = pymde_amd.DenseMDE(distance_matrix=Dm, loss=losses.Quadratic)
            med, times = timed(lambda: value_and_backward(problem, X))
            line("DenseMDE.average_distortion + backward, Quadratic", med, times, base)
            first = False
            del data, X, Dm, problem
            torch.cuda.empty_cache()
        if args.cycle:
            n = args.cycle
            idx = np.arange(n)
            say("")
            say("cycle (BASELINE config 1): %d nodes, all %d pairs, losses.Quadratic, embed(max_iter=50), one start"
                % (n, n * (n - 1) // 2))
            start = pymde_amd.Centered().initialization(n, 2, dev)
            start = (start * (n / 8.0)).contiguous()            # at the scale of the hop counts
            t = time.perf_counter()
            graph = pymde_amd.Graph.from_edges(torch.as_tensor(np.stack([idx, (idx + 1) % n], 1)))
            edge = pymde_amd.preserve_distances(graph, max_distances=1e9, loss=losses.Quadratic)
            torch.cuda.synchronize()
            t_edge_build = time.perf_counter() - t
            t = time.perf_counter()
            gap = np.abs(idx[:, None] - idx[None, :])
            problem = pymde_amd.DenseMDE(distance_matrix=np.minimum(gap, n - gap).astype(np.float32),
                                         loss=losses.Quadratic)
            torch.cuda.synchronize()
            t_dense_build = time.perf_counter() - t
            for name, p, built in (("edge list (graph recipe)", edge, t_edge_build),
                                   ("DenseMDE(distance_matrix)", problem, t_dense_build)):
                p.embed(X=start.clone(), max_iter=3)            # warm-up
                torch.cuda.synchronize()
                t = time.perf_counter()
                p.embed(X=start.clone(), max_iter=50)
                torch.cuda.synchronize()
                t = time.perf_counter() - t
                s = p.solve_stats
                evals = s.evaluations or s.iterations
                say("  %-28s built in %.3f s; embed %.3f s, %d iterations, %d evaluations (%.2f ms per evaluation), "
                    "value %.6g" % (name, built, t, s.iterations, evals, 1e3 * t / max(evals, 1), p.value))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

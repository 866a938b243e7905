"""Placement into a dense embedding (pymde_amd.DensePlacement, mde_pair_loss_cross) and landmark MDS
(preserve_distances(landmarks=m)) at user sizes.

    python tools/dense_place_scale.py [--walk 20000x784,20000x64] [--evals 1000000x20000,100000x5000]
                                      [--landmark 1000000x20000] [--full 70000] [--max-iter 60] [--reps 5]
                                      [--limit 600] [--out profiles/r16_dense_place.txt]

Every step is a child process under its own time limit (--limit seconds); the first step that fails or runs past its
limit stops the run.  The data are the stand-in of tools/mnist_like.py (a 10-component Gaussian mixture, centres
N(0, 4 I), unit noise) in R^nf, drawn on the GPU; embeddings are random projections to two dimensions.

  walk      the rectangular walk against the square walk at equal ordered-pair counts: mde_pair_loss_cross of n query
            rows against n OTHER corpus rows beside mde_pair_loss of n rows (kernels alone, losses.Quadratic, d = 2,
            automatic slices), alternating, the median (min - max) of --reps calls after a warm-up, each timed with a
            device synchronise on both sides.  The square walk skips n diagonal pairs of n^2.
  evals     one evaluation of mde_pair_loss_cross at a landmark shape, n_q rows against n_c landmarks, 784 features.
  landmark  preserve_distances(data, landmarks=m, loss=Quadratic, seed=0).embed(max_iter=--max-iter) on n x 784: the
            wall time of the construction, of each stage's solve and of the whole, and
            quality.stress(data, X, scale=1.0, sample=2000) of the result.
  full      the full DenseMDE(loss=Quadratic).embed(max_iter=--max-iter) on n x 784 and the same stress, for comparison.
No time is asserted anywhere."""
import argparse
import os
import subprocess
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
NF = 784


def mnist_like(n, nf, dev, seed=0, components=10):
    """n rows of the mixture, drawn in blocks (the centres depend on nf and `components` alone)."""
    g = torch.Generator(device=dev)
    g.manual_seed(nf)
    centres = 2.0 * torch.randn(components, nf, generator=g, device=dev)
    g.manual_seed(1000003 * (seed + 1) + n)
    data = torch.empty((n, nf), device=dev)
    for lo in range(0, n, 100000):
        block = data[lo:lo + 100000]
        torch.randn(block.shape, generator=g, device=dev, out=block)
        block += centres[torch.randint(0, components, (block.shape[0],), generator=g, device=dev)]
    return data


def projection(data, seed):
    g = torch.Generator(device=data.device)
    g.manual_seed(seed)
    return (data @ torch.randn(data.shape[1], 2, generator=g, device=data.device)).contiguous()


def clock(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t


def summary(times):
    times = sorted(times)
    return "%.6f (%.6f - %.6f)" % (times[len(times) // 2], times[0], times[-1])


def step_walk(n, nf, reps):
    from pymde_amd import dense, losses, metrics
    dev = torch.device("cuda", 0)
    spec = dense.loss_spec(losses.Quadratic)
    A, mu = metrics.translated_rows(mnist_like(n, nf, dev, seed=0))
    B = mnist_like(n, nf, dev, seed=1)
    if mu is not None:
        B = metrics.subtract_columns(B, mu)
    XA, XB = projection(A, 1), projection(B, 1)
    square = lambda: dense._pair_loss(XA, spec, A=A)                       # noqa: E731
    cross = lambda: dense._pair_loss_cross(XB, XA, spec, Q=B, C=A)         # noqa: E731
    square(), cross()
    t_square, t_cross = [], []
    for _ in range(reps):
        t_square.append(clock(square))
        t_cross.append(clock(cross))
    med = lambda t: sorted(t)[len(t) // 2]                                 # noqa: E731
    print("  %d x %d features, d = 2, Quadratic, %d alternating calls; seconds, median (min - max)" % (n, nf, reps))
    print("    mde_pair_loss        %d rows            %s" % (n, summary(t_square)))
    print("    mde_pair_loss_cross  %d x %d rows    %s  = %.3f x the square walk  (%.1f TF/s of Gram)"
          % (n, n, summary(t_cross), med(t_cross) / med(t_square), 2.0 * n * n * nf / med(t_cross) / 1e12))


def step_eval(n_q, n_c, reps):
    from pymde_amd import _lib, dense, losses, metrics
    dev = torch.device("cuda", 0)
    spec = dense.loss_spec(losses.Quadratic)
    C, mu = metrics.translated_rows(mnist_like(n_c, NF, dev, seed=0))
    Q = mnist_like(n_q, NF, dev, seed=1)
    if mu is not None:
        Q = metrics.subtract_columns(Q, mu)
    XQ, XC = projection(Q, 1), projection(C, 1)
    work = dense._work_cross(_lib.load(), n_q, n_c, 2, 0, dev)
    run = lambda: dense._pair_loss_cross(XQ, XC, spec, Q=Q, C=C, work=work)           # noqa: E731
    run()
    times = [clock(run) for _ in range(reps)]
    med = sorted(times)[len(times) // 2]
    print("  mde_pair_loss_cross %d x %d rows, %d features, d = 2 (%.3g pairs): %s s  (%.1f TF/s of Gram; work %.1f MB)"
          % (n_q, n_c, NF, float(n_q) * n_c, summary(times), 2.0 * n_q * n_c * NF / med / 1e12, work.numel() / 1e6))


def step_landmark(n, m, max_iter):
    import pymde_amd
    from pymde_amd import losses, quality
    dev = torch.device("cuda", 0)
    data = mnist_like(n, NF, dev)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    problem = pymde_amd.preserve_distances(data, landmarks=m, seed=0, loss=losses.Quadratic)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    X = problem.embed(max_iter=max_iter)
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    stats = problem.solve_stats
    stress = quality.stress(data, X, scale=1.0, sample=2000)
    torch.cuda.synchronize()
    t3 = time.perf_counter()
    print("  preserve_distances(landmarks=%d) on %d x %d, Quadratic, embed(max_iter=%d):" % (m, n, NF, max_iter))
    print("    construction (the draw, the landmark rows, their preparation)   %.3f s" % (t1 - t0))
    for name, s, p in (("landmark stage: DenseMDE of %d rows" % m, stats.landmarks, problem.landmark_problem),
                       ("placement stage: %d rows against %d" % (n - m, m), stats.placement, problem.placement)):
        print("    %-60s solve %.3f s, %d iterations, %d evaluations, value %.6g"
              % (name, s.solve_time, s.iterations, s.evaluations or s.iterations, p.value))
    print("    embed() as a whole (both solves, the rows of the placement, its start, the scatter)   %.3f s" % (t2 - t1))
    print("    quality.stress(data, X, scale=1.0, sample=2000) = %.6f   (%.3f s)" % (stress, t3 - t2))


def step_full(n, max_iter):
    import pymde_amd
    from pymde_amd import losses, quality
    dev = torch.device("cuda", 0)
    data = mnist_like(n, NF, dev)
    problem = pymde_amd.DenseMDE(data, loss=losses.Quadratic)
    t = clock(lambda: problem.embed(max_iter=max_iter))
    s = problem.solve_stats
    stress = quality.stress(data, problem.X, scale=1.0, sample=2000)
    print("  DenseMDE on %d x %d, Quadratic, embed(max_iter=%d): %.3f s, %d iterations, %d evaluations, value %.6g; "
          "quality.stress(scale=1.0, sample=2000) = %.6f"
          % (n, NF, max_iter, t, s.iterations, s.evaluations or s.iterations, problem.value, stress))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--walk", default="20000x784,20000x64")
    ap.add_argument("--evals", default="1000000x20000,100000x5000")
    ap.add_argument("--landmark", default="1000000x20000")
    ap.add_argument("--full", default="70000")
    ap.add_argument("--max-iter", type=int, default=60)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--limit", type=int, default=600, help="seconds per step")
    ap.add_argument("--out", default=None)
    ap.add_argument("--step", default=None, help=argparse.SUPPRESS)      # kind:a:b
    a = ap.parse_args()
    if a.step:
        kind, x, y = a.step.split(":")
        with torch.cuda.device(0):
            if kind == "walk":
                step_walk(int(x), int(y), a.reps)
            elif kind == "eval":
                step_eval(int(x), int(y), a.reps)
            elif kind == "landmark":
                step_landmark(int(x), int(y), a.max_iter)
            else:
                step_full(int(x), a.max_iter)
        return 0
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def finish(code):
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")
        return code

    def pairs(text):
        return [tuple(int(v) for v in item.split("x")) for item in text.split(",") if item]

    steps = [("walk", n, nf) for n, nf in pairs(a.walk)] + [("eval", q, c) for q, c in pairs(a.evals)]
    steps += [("landmark", n, m) for n, m in pairs(a.landmark)] + [("full", int(n), 0) for n in a.full.split(",") if n]
    say("tools/dense_place_scale.py; every step a process of its own under a limit of %d s" % a.limit)
    last = None
    for kind, x, y in steps:
        if kind != last:
            say("")
            say("## %s" % kind)
            last = kind
        cmd = [sys.executable, os.path.abspath(__file__), "--step", "%s:%d:%d" % (kind, x, y), "--reps", str(a.reps),
               "--max-iter", str(a.max_iter)]
        try:
            p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=a.limit)
        except subprocess.TimeoutExpired:
            say("step %s:%d:%d ran past its limit of %d s: stopping" % (kind, x, y, a.limit))
            return finish(1)
        for line in p.stdout.decode(errors="replace").splitlines():
            say(line)
        if p.returncode != 0:
            say("step %s:%d:%d exited with status %d: stopping" % (kind, x, y, p.returncode))
            return finish(1)
    return finish(0)


if __name__ == "__main__":
    sys.exit(main())

"""Classical scaling and triangulation (pymde_amd.classical, csrc/mde_pair_apply.hip) at user sizes.

    python tools/classical_scale.py [--apply 20000x784,20000x64,20000x0] [--mds 20000x784:cosine,20000x64:cosine,20000x0]
                                    [--dense 20000x784] [--landmark 1000000x20000] [--unchanged 20000x784]
                                    [--r 18] [--reps 5] [--max-iter 60] [--limit 600]
                                    [--out profiles/r22_classical_mds.txt]

Every step is a child process under its own time limit (--limit seconds); the first step that fails or runs past its
limit stops the run.  Rows: the mixture of tools/mnist_like.py, drawn on the GPU as tools/dense_place_scale.py draws
it; "n x 0" is the n x n matrix of the Euclidean distances of n x 64 rows.  Times are medians (min - max) of --reps
calls after a warm-up, each with a device synchronise on both sides.

  apply      one mde_pair_sqdist_apply with --r columns beside the kernels of quality.pair_moments on the same rows
             (the embedding side: a 2-D projection), in alternating calls; for a matrix, beside mde_pair_loss on it.
  mds        classical_mds end to end (preparation and checks included) on rows under a metric, or on the matrix.
  dense      DenseMDE(rows, Quadratic).embed(max_iter) from init="random" and from init="classical": iterations,
             evaluations, seconds, quality.stress(scale=1.0, sample=2000); and the stress of the classical start.
  landmark   preserve_distances(rows, landmarks=m, placement_solver="rows") with and without init="classical".
  unchanged  mde_pair_loss, mde_pair_loss_cross and mde_pair_moments on the rows, in alternating calls.
No number is asserted anywhere."""
import argparse
import os
import subprocess
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from dense_place_scale import clock, mnist_like, projection  # noqa: E402


def ms(times):
    times = sorted(1e3 * t for t in times)
    return "%.3f (%.3f - %.3f) ms" % (times[len(times) // 2], times[0], times[-1])


def alternate(runs, reps):
    """``reps`` rounds of every callable of ``runs`` in turn, after one warm-up round: a list of times per callable."""
    for run in runs:
        run()
    times = [[] for _ in runs]
    for _ in range(reps):
        for t, run in zip(times, runs):
            t.append(clock(run))
    return times


def matrix_of(n, dev):
    return torch.cdist(*(2 * [mnist_like(n, 64, dev)])).contiguous()


def step_apply(n, nf, r, reps):
    from pymde_amd import _lib, classical, dense, losses, metrics, quality
    dev = torch.device("cuda", 0)
    V = torch.randn((n, r), device=dev)
    lib = _lib.load()
    work = _lib.work_buffer(lib.mde_pair_sqdist_apply_work_bytes, n, n, r, 0, device=dev)
    if nf:
        A = metrics.translated_rows(mnist_like(n, nf, dev))[0]
        X = projection(A, 1)
        ours = lambda: classical.sqdist_apply(V, Q=A, C=A, skip_diagonal=True, work=work)          # noqa: E731
        theirs = lambda: quality._pair_moments(A, X)                                               # noqa: E731
        name = "quality._pair_moments (two Gram tiles per step)"
    else:
        Dm = matrix_of(n, dev)
        X = torch.randn((n, 2), device=dev)
        spec = dense.loss_spec(losses.Quadratic)
        loss_work = dense._work(lib, n, 2, 0, dev)
        ours = lambda: classical.sqdist_apply(V, Dm=Dm, skip_diagonal=True, work=work)             # noqa: E731
        theirs = lambda: dense._pair_loss(X, spec, Dm=Dm, work=loss_work)                          # noqa: E731
        name = "mde_pair_loss on the matrix, d = 2"
    t_ours, t_theirs = alternate([ours, theirs], reps)
    print("  %d x %s, r = %d; %d alternating calls after a warm-up, median (min - max)"
          % (n, nf or "%d matrix" % n, r, reps))
    print("    mde_pair_sqdist_apply            %s" % ms(t_ours))
    print("    %s   %s" % (name, ms(t_theirs)))


def step_mds(n, nf, metric, reps):
    import pymde_amd
    dev = torch.device("cuda", 0)
    source = dict(data=mnist_like(n, nf, dev), metric=metric) if nf else dict(distance_matrix=matrix_of(n, dev))
    run = lambda: pymde_amd.classical_mds(embedding_dim=2, **source)                               # noqa: E731
    fit = run()
    times = [clock(run) for _ in range(reps)]
    print("  classical_mds(%d x %s%s, 2) end to end, n_iter = 4, 10 oversamples: %s; eigenvalues %s of a trace of %.6g, "
          "negative %s" % (n, nf or "%d matrix" % n, ", " + metric if nf else "", ms(times),
                           ["%.6g" % v for v in fit.eigenvalues.tolist()], float(fit.total), fit.negative))


def step_dense(n, nf, max_iter):
    import pymde_amd
    from pymde_amd import losses, quality
    dev = torch.device("cuda", 0)
    data = mnist_like(n, nf, dev)
    for init in ("random", "classical"):
        pymde_amd.seed(0)
        problem = pymde_amd.DenseMDE(data, loss=losses.Quadratic, init=init)
        t = clock(lambda: problem.embed(max_iter=max_iter))
        s = problem.solve_stats
        stress = quality.stress(data, problem.X, scale=1.0, sample=2000)
        print("  DenseMDE(%d x %d, Quadratic, init=%r).embed(max_iter=%d): %.3f s (the start included), %d iterations, "
              "%s evaluations, value %.6g; quality.stress(scale=1.0, sample=2000) = %.6f"
              % (n, nf, init, max_iter, t, s.iterations, getattr(s, "evaluations", None) or s.iterations,
                 problem.value, stress))
        if init == "classical":
            start = [clock(problem.classical_initialization) for _ in range(3)]
            X0 = problem.classical_initialization()
            print("    the classical start alone: %s; its stress %.6f"
                  % (ms(start), quality.stress(data, X0, scale=1.0, sample=2000)))


def step_landmark(n, m, max_iter):
    import pymde_amd
    from pymde_amd import losses, quality
    dev = torch.device("cuda", 0)
    data = mnist_like(n, 784, dev)
    for init in ("random", "classical"):
        pymde_amd.seed(0)
        problem = pymde_amd.preserve_distances(data, landmarks=m, seed=0, loss=losses.Quadratic, init=init)
        if init == "classical":
            t = clock(lambda: problem.initialization())
            print("    LandmarkMDE.initialization(): %.3f s; stress of that start %.6f"
                  % (t, quality.stress(data, problem.initialization(), scale=1.0, sample=2000)))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        X = problem.embed(max_iter=max_iter, placement_solver="rows")
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        sl, sp = problem.solve_stats.landmarks, problem.solve_stats.placement
        status = problem.placement.row_status
        print("  preserve_distances(%d x 784, landmarks=%d, init=%r).embed(max_iter=%d, placement_solver='rows'): "
              "%.3f s; landmarks %d iterations in %.3f s; placement %d sweeps, %.2f full evaluations, %.3f s, %d "
              "converged / %d stalled / %d active rows; quality.stress(scale=1.0, sample=2000) = %.6f"
              % (n, m, init, max_iter, t1 - t0, sl.iterations, sl.solve_time, sp.iterations, sp.evaluations,
                 sp.solve_time, int((status == 1).sum()), int((status == 2).sum()), int((status == 0).sum()),
                 quality.stress(data, X, scale=1.0, sample=2000)))


def step_unchanged(n, nf, reps):
    from pymde_amd import _lib, dense, losses, metrics, quality
    dev = torch.device("cuda", 0)
    spec = dense.loss_spec(losses.Quadratic)
    A = metrics.translated_rows(mnist_like(n, nf, dev))[0]
    X = projection(A, 1)
    lib = _lib.load()
    w_sq, w_cr = dense._work(lib, n, 2, 0, dev), dense._work_cross(lib, n, n, 2, 0, dev)
    runs = [lambda: dense._pair_loss(X, spec, A=A, work=w_sq),
            lambda: dense._pair_loss_cross(X, X, spec, Q=A, C=A, work=w_cr),
            lambda: quality._pair_moments(A, X)]
    times = alternate(runs, reps)
    print("  %d x %d; %d alternating calls after a warm-up, median (min - max)" % (n, nf, reps))
    for name, t in zip(("mde_pair_loss", "mde_pair_loss_cross", "mde_pair_moments"), times):
        print("    %-22s %s" % (name, ms(t)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--apply", default="20000x784,20000x64,20000x0")
    ap.add_argument("--mds", default="20000x784:cosine,20000x64:cosine,20000x0")
    ap.add_argument("--dense", default="20000x784")
    ap.add_argument("--landmark", default="1000000x20000")
    ap.add_argument("--unchanged", default="20000x784")
    ap.add_argument("--r", type=int, default=18)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--max-iter", type=int, default=60)
    ap.add_argument("--landmark-max-iter", type=int, default=300)
    ap.add_argument("--limit", type=int, default=600, help="seconds per step")
    ap.add_argument("--out", default=None)
    ap.add_argument("--step", default=None, help=argparse.SUPPRESS)      # kind:a:b[:metric]
    a = ap.parse_args()
    if a.step:
        kind, n, second, metric = (a.step.split(":") + ["euclidean"])[:4]
        n, second = int(n), int(second)
        with torch.cuda.device(0):
            if kind == "apply":
                step_apply(n, second, a.r, a.reps)
            elif kind == "mds":
                step_mds(n, second, metric, a.reps)
            elif kind == "dense":
                step_dense(n, second, a.max_iter)
            elif kind == "landmark":
                step_landmark(n, second, a.landmark_max_iter)
            else:
                step_unchanged(n, second, a.reps)
        return 0
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
        if a.out:                                   # (kept current: a run that is cut short leaves what it measured)
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    steps = []
    for kind, text in (("apply", a.apply), ("mds", a.mds), ("dense", a.dense), ("landmark", a.landmark),
                       ("unchanged", a.unchanged)):
        for item in text.split(","):
            if item:
                shape, _, metric = item.partition(":")
                steps.append(":".join([kind] + shape.split("x") + ([metric] if metric else [])))
    say("tools/classical_scale.py; every step a process of its own under a limit of %d s" % a.limit)
    for step in steps:
        say("")
        say("## %s" % step)
        cmd = [sys.executable, os.path.abspath(__file__), "--step", step, "--r", str(a.r), "--reps", str(a.reps),
               "--max-iter", str(a.max_iter), "--landmark-max-iter", str(a.landmark_max_iter)]
        try:
            p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=a.limit)
        except subprocess.TimeoutExpired:
            say("step %s ran past its limit of %d s: stopping" % (step, a.limit))
            return 1
        for line in p.stdout.decode(errors="replace").splitlines():
            say(line)
        if p.returncode != 0:                       # (warnings on stderr are not part of the record; a failure's are)
            for line in p.stderr.decode(errors="replace").splitlines():
                say(line)
            say("step %s exited with status %d: stopping" % (step, p.returncode))
            return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())

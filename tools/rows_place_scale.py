"""The per-row placement solver (pymde_amd.rows) beside the joint solver at user sizes.

    python tools/rows_place_scale.py [--walk 20000x784] [--landmark 1000000x20000] [--solvers rows,joint]
                                     [--rows-max-iter 300] [--joint-max-iter 60] [--eps 1e-5] [--reps 5]
                                     [--limit 600] [--out profiles/r17_rows_place.txt]

Every step is a child process under its own time limit (--limit seconds); the first step that fails or runs past its
limit stops the run.  Data and helpers are those of tools/dense_place_scale.py.

  walk      mde_pair_loss_cross_rows(rows=NULL) beside mde_pair_loss_cross, n query rows against n OTHER corpus rows
            (kernels alone, losses.Quadratic, d = 2, automatic slices), alternating, the median (min - max) of --reps
            calls after a warm-up, each timed with a device synchronise on both sides.
  landmark  preserve_distances(data, landmarks=m, loss=Quadratic, seed=0) on n x 784, once per solver of the placement
            stage: embed(placement_solver="rows", eps=--eps, max_iter=--rows-max-iter) and the unchanged joint solver
            at embed(max_iter=--joint-max-iter): wall time, sweeps / iterations, full-evaluation equivalents, the
            status counts, the final value, and quality.stress(data, X, scale=1.0, sample=2000).
No time is asserted anywhere."""
import argparse
import os
import subprocess
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from dense_place_scale import NF, clock, mnist_like, projection, summary  # noqa: E402


def step_walk(n, nf, reps):
    from pymde_amd import _lib, dense, losses, metrics, rows
    dev = torch.device("cuda", 0)
    spec = dense.loss_spec(losses.Quadratic)
    A, mu = metrics.translated_rows(mnist_like(n, nf, dev, seed=0))
    B = mnist_like(n, nf, dev, seed=1)
    if mu is not None:
        B = metrics.subtract_columns(B, mu)
    XA, XB = projection(A, 1), projection(B, 1)
    row_loss = torch.empty(n, dtype=torch.float64, device=dev)
    row_grad = torch.empty((n, 2), dtype=torch.float32, device=dev)
    work = rows.work_cross_rows(_lib.load(), n, n, 2, 0, dev)
    work_cross = dense._work_cross(_lib.load(), n, n, 2, 0, dev)
    cross = lambda: dense._pair_loss_cross(XB, XA, spec, Q=B, C=A, work=work_cross)                       # noqa: E731
    listed = lambda: rows.pair_loss_cross_rows(XB, XA, spec, row_loss, row_grad, Q=B, C=A, work=work)     # noqa: E731
    want = cross()[2]
    listed()
    same = bool(torch.equal(want, row_loss))
    t_cross, t_rows = [], []
    for _ in range(reps):
        t_cross.append(clock(cross))
        t_rows.append(clock(listed))
    med = lambda t: sorted(t)[len(t) // 2]                                 # noqa: E731
    print("  %d x %d rows, %d features, d = 2, Quadratic, %d alternating calls; seconds, median (min - max)"
          % (n, n, nf, reps))
    print("    mde_pair_loss_cross                  %s" % summary(t_cross))
    print("    mde_pair_loss_cross_rows(rows=NULL)  %s  = %.3f x; row_loss bit-equal: %s"
          % (summary(t_rows), med(t_rows) / med(t_cross), same))


def step_landmark(n, m, solver, max_iter, eps):
    import pymde_amd
    from pymde_amd import losses, quality
    dev = torch.device("cuda", 0)
    data = mnist_like(n, NF, dev)
    problem = pymde_amd.preserve_distances(data, landmarks=m, seed=0, loss=losses.Quadratic)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    if solver == "rows":
        X = problem.embed(placement_solver="rows", eps=eps, max_iter=max_iter)
    else:
        X = problem.embed(max_iter=max_iter)
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    stats, place = problem.solve_stats, problem.placement
    stress = quality.stress(data, X, scale=1.0, sample=2000)
    print("  preserve_distances(landmarks=%d) on %d x %d, Quadratic, placement solver %r, max_iter=%d%s:"
          % (m, n, NF, solver, max_iter, ", eps=%g" % eps if solver == "rows" else ""))
    print("    landmark stage: solve %.3f s, %d iterations, %d evaluations, value %.6g"
          % (stats.landmarks.solve_time, stats.landmarks.iterations, stats.landmarks.evaluations,
             problem.landmark_problem.value))
    print("    placement stage (%d rows against %d): solve %.3f s, %d %s, %.2f full evaluations, value %.6g, "
          "residual norm %.3g" % (n - m, m, stats.placement.solve_time, stats.placement.iterations,
                                  "sweeps" if solver == "rows" else "iterations", stats.placement.evaluations,
                                  place.value, place.residual_norm))
    if solver == "rows":
        counts = torch.bincount(place.row_status, minlength=3).tolist()
        print("    rows by status: active %d, converged %d, stalled %d" % tuple(counts))
        print("    sweeps after which 50 %% / 90 %% / 99 %% of the solve's wall time had passed: %s"
              % " / ".join(str(v) for v in time_quantiles(stats.placement)))
    print("    embed() as a whole %.3f s; quality.stress(data, X, scale=1.0, sample=2000) = %.6f" % (t2 - t1, stress))


def time_quantiles(stats):
    """The sweeps at which 50 %, 90 % and 99 % of the solve's wall time had passed (the late sweeps evaluate few rows)."""
    total = stats.times[-1] if stats.times else 0.0
    out = []
    for share in (0.5, 0.9, 0.99):
        out.append(next((i + 1 for i, t in enumerate(stats.times) if t >= share * total), len(stats.times)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--walk", default="20000x784")
    ap.add_argument("--landmark", default="1000000x20000")
    ap.add_argument("--solvers", default="rows,joint")
    ap.add_argument("--rows-max-iter", type=int, default=300)
    ap.add_argument("--joint-max-iter", type=int, default=60)
    ap.add_argument("--eps", type=float, default=1e-5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--limit", type=int, default=600, help="seconds per step")
    ap.add_argument("--out", default=None)
    ap.add_argument("--step", default=None, help=argparse.SUPPRESS)      # kind:a:b[:solver]
    a = ap.parse_args()
    if a.step:
        kind, x, y, solver = (a.step.split(":") + [""])[:4]
        with torch.cuda.device(0):
            if kind == "walk":
                step_walk(int(x), int(y), a.reps)
            else:
                step_landmark(int(x), int(y), solver, a.rows_max_iter if solver == "rows" else a.joint_max_iter, a.eps)
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

    steps = ["walk:%d:%d" % p for p in pairs(a.walk)]
    steps += ["landmark:%d:%d:%s" % (n, m, s) for n, m in pairs(a.landmark) for s in a.solvers.split(",") if s]
    say("tools/rows_place_scale.py; every step a process of its own under a limit of %d s" % a.limit)
    for step in steps:
        say("")
        say("## %s" % step)
        cmd = [sys.executable, os.path.abspath(__file__), "--step", step, "--reps", str(a.reps), "--eps", str(a.eps),
               "--rows-max-iter", str(a.rows_max_iter), "--joint-max-iter", str(a.joint_max_iter)]
        try:
            p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=a.limit)
        except subprocess.TimeoutExpired:
            say("step %s ran past its limit of %d s: stopping" % (step, a.limit))
            return finish(1)
        for line in p.stdout.decode(errors="replace").splitlines():
            say(line)
        if p.returncode != 0:
            say("step %s exited with status %d: stopping" % (step, p.returncode))
            return finish(1)
    return finish(0)


if __name__ == "__main__":
    sys.exit(main())

"""Landmark selection on the GPU (pymde_amd.landmarks) at user sizes.

    python tools/landmark_select_scale.py [--shapes 200000x784,1000000x64,1000000x784] [--m 1000] [--reps 5]
                                          [--stress 1000000x20000] [--max-iter 300] [--eps 1e-5] [--limit 600]
                                          [--out profiles/r20_landmark_selection.txt]

Every step is a child process under its own time limit (--limit seconds); the first step that fails or runs past its
limit stops the run.  Data: the mixture of tools/mnist_like.py as tools/dense_place_scale.py draws it on the GPU.

  select  per shape and method ("farthest", "kmeans++"), m landmarks: the wall time of mde_select_landmarks alone (on
          the prepared rows) and of landmarks.select as a whole (with the preparation of the rows), the median
          (min - max) of --reps calls after a warm-up, each with a device synchronise on both sides; the update
          kernel's achieved rate n * nf * 4 * m / time beside the 8 TB/s of the data sheet; and the covering radius
          (the largest distance from a row to its nearest landmark) of the two selections and of the uniform draw
          quality._sample_rows(n, m, 0).
  stress  preserve_distances(data, landmarks=m, landmark_selection=s, loss=Quadratic, seed=0) on n x 784 for the three
          selections, embed(placement_solver="rows", eps=--eps, max_iter=--max-iter): the time to build the problem
          (the selection is in it), of embed(), the covering radius and quality.stress(data, X, scale=1.0,
          sample=2000).
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
from dense_place_scale import NF, clock, mnist_like, summary  # noqa: E402

SPEC_BYTES_PER_S = 8.0e12


def covering_radius(data, rows):
    """The largest Euclidean distance from a row of ``data`` to its nearest row among ``rows`` (float32, in blocks)."""
    L = data[rows.to(data.device)]
    worst = 0.0
    for r0 in range(0, data.shape[0], 1 << 16):
        d = torch.cdist(data[r0:r0 + (1 << 16)], L, compute_mode="donot_use_mm_for_euclid_dist")
        worst = max(worst, float(d.min(dim=1).values.max()))
    return worst


def step_select(n, nf, m, reps):
    from pymde_amd import landmarks, metrics, quality
    dev = torch.device("cuda", 0)
    data = mnist_like(n, nf, dev)
    rows = quality._self_rows(data, metrics.EUCLIDEAN, dev, "data")
    print("  %d x %d, m = %d, %d calls after a warm-up; seconds, median (min - max)" % (n, nf, m, reps))
    for method in ("farthest", "kmeans++"):
        kernels = lambda: landmarks._select_rows(rows, m, method, 0, 0)                          # noqa: E731
        whole = lambda: landmarks.select(data, m, method=method, start=0, seed=0)               # noqa: E731
        kernels()
        t_k = [clock(kernels) for _ in range(reps)]
        whole()
        t_w = [clock(whole) for _ in range(reps)]
        med = sorted(t_k)[len(t_k) // 2]
        rate = n * nf * 4.0 * m / med
        chosen = whole()
        print("    %-9s mde_select_landmarks %s = %.1f us per landmark, %.2f TB/s (%.0f %% of 8 TB/s); "
              "landmarks.select %s; covering radius %.4f"
              % (method, summary(t_k), 1e6 * med / m, rate / 1e12, 100.0 * rate / SPEC_BYTES_PER_S, summary(t_w),
                 float(chosen.distance.max())))
    print("    uniform   quality._sample_rows(n, m, 0): covering radius %.4f"
          % covering_radius(rows, quality._sample_rows(n, m, 0)))


def step_stress(n, m, selection, max_iter, eps):
    import pymde_amd
    from pymde_amd import losses, quality
    dev = torch.device("cuda", 0)
    data = mnist_like(n, NF, dev)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    problem = pymde_amd.preserve_distances(data, landmarks=m, landmark_selection=selection, seed=0,
                                           loss=losses.Quadratic)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    X = problem.embed(placement_solver="rows", eps=eps, max_iter=max_iter)
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    radius = problem.landmark_radius
    if radius is None:
        radius = covering_radius(data, problem.landmarks)
    stress = quality.stress(data, X, scale=1.0, sample=2000)
    print("  preserve_distances(landmarks=%d, landmark_selection=%r) on %d x %d, Quadratic, placement solver 'rows', "
          "max_iter=%d, eps=%g:" % (m, selection, n, NF, max_iter, eps))
    print("    building the problem %.3f s (the selection is in it), embed() %.3f s; covering radius %.4f; "
          "quality.stress(data, X, scale=1.0, sample=2000) = %.6f" % (t1 - t0, t2 - t1, radius, stress))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="200000x784,1000000x64,1000000x784")
    ap.add_argument("--m", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--stress", default="1000000x20000")
    ap.add_argument("--max-iter", type=int, default=300)
    ap.add_argument("--eps", type=float, default=1e-5)
    ap.add_argument("--limit", type=int, default=600, help="seconds per step")
    ap.add_argument("--out", default=None)
    ap.add_argument("--step", default=None, help=argparse.SUPPRESS)      # kind:a:b[:selection]
    a = ap.parse_args()
    if a.step:
        kind, x, y, selection = (a.step.split(":") + [""])[:4]
        with torch.cuda.device(0):
            if kind == "select":
                step_select(int(x), int(y), a.m, a.reps)
            else:
                step_stress(int(x), int(y), selection, a.max_iter, a.eps)
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

    steps = ["select:%d:%d" % p for p in pairs(a.shapes)]
    steps += ["stress:%d:%d:%s" % (n, m, s) for n, m in pairs(a.stress) for s in ("uniform", "farthest", "kmeans++")]
    say("tools/landmark_select_scale.py; every step a process of its own under a limit of %d s" % a.limit)
    for step in steps:
        say("")
        say("## %s" % step)
        cmd = [sys.executable, os.path.abspath(__file__), "--step", step, "--m", str(a.m), "--reps", str(a.reps),
               "--max-iter", str(a.max_iter), "--eps", str(a.eps)]
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

"""Per-pair weights in the dense walk at user sizes: what the weight variants cost beside the
unweighted call, and that the existing entry points cost what they did.

    python tools/dense_weights_scale.py [--old 20000x784] [--weighted 20000x784] [--embed 20000] [--max-iter 60]
                                        [--reps 5] [--limit 600] [--tree PATH [--tree-label TEXT]]
                                        [--out profiles/r18_dense_weights.txt]

Every step is a child process under its own time limit (--limit seconds); the first step that fails or runs past its
limit stops the run.  Data and helpers are those of tools/dense_place_scale.py.  d = 2, losses.Quadratic, automatic
slices, kernels alone through the thin wrappers; a figure is the median (min - max) of --reps calls after a warm-up,
each timed with a device synchronise on both sides, the calls of a step alternating.

  old       mde_pair_loss from the Gram source (n x nf) and from the matrix source (n x n): the entry points that were
            there before the weights.  With --tree PATH the step imports pymde_amd from that checkout (built there)
            instead of this one, and runs before and after this one's: the parent commit beside this build.
  weighted  beside the unweighted call of the same build and shape: p = 1, p = 2.5, a weight matrix (uniform in
            [0.5, 1.5]) and a half-empty one (every other pair missing, at random) with the Gram source; the unweighted
            call and a weight matrix with the matrix source, which reads twice the bytes per pair.
  embed     DenseMDE(data, loss=Quadratic).embed(max_iter=--max-iter) beside the same with weights=1 (Sammon mapping):
            wall time, iterations, evaluations, value, quality.stress(data, X, scale=1.0, sample=2000).
No time is asserted anywhere."""
import argparse
import os
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from dense_place_scale import NF, clock, mnist_like, projection, summary  # noqa: E402


def _median(times):
    return sorted(times)[len(times) // 2]


def _alternate(calls, reps):
    """{name: [seconds] * reps} of the named calls, run in turn `reps` times after one warm-up each."""
    for fn in calls.values():
        fn()
    times = {name: [] for name in calls}
    for _ in range(reps):
        for name, fn in calls.items():
            times[name].append(clock(fn))
    return times


def _inputs(n, nf, dev):
    from pymde_amd import metrics
    A = metrics.translated_rows(mnist_like(n, nf, dev, seed=0))[0]
    return A, projection(A, 1)


def step_old(n, nf, reps):
    from pymde_amd import _lib, dense, losses
    dev = torch.device("cuda", 0)
    spec = dense.loss_spec(losses.Quadratic)
    A, X = _inputs(n, nf, dev)
    Dm = torch.cdist(A, A).contiguous()
    work = dense._work(_lib.load(), n, 2, 0, dev)
    times = _alternate({"gram": lambda: dense._pair_loss(X, spec, A=A, work=work),
                        "matrix": lambda: dense._pair_loss(X, spec, Dm=Dm, work=work)}, reps)
    print("  mde_pair_loss, %d rows, d = 2, Quadratic, %d alternating calls; seconds, median (min - max)" % (n, reps))
    print("    Gram source, %d features   %s" % (nf, summary(times["gram"])))
    print("    matrix source [n, n]        %s" % summary(times["matrix"]))


def step_weighted(n, nf, reps):
    from pymde_amd import _lib, dense, losses
    dev = torch.device("cuda", 0)
    spec = dense.loss_spec(losses.Quadratic)
    A, X = _inputs(n, nf, dev)
    work = dense._work(_lib.load(), n, 2, 0, dev)
    g = torch.Generator(device=dev)
    g.manual_seed(5)
    U = torch.triu(0.5 + torch.rand((n, n), generator=g, device=dev), 1)
    W = (U + U.T).contiguous()
    del U
    H = torch.triu((torch.rand((n, n), generator=g, device=dev) < 0.5).to(torch.float32), 1)
    H = (H + H.T).contiguous()
    full, half = dense.weight_stats(W), dense.weight_stats(H)
    assert full.kept == n * (n - 1) // 2 and full.empty_rows == 0 and half.empty_rows == 0
    t_check = [clock(lambda: dense.weight_stats(W)) for _ in range(reps)]
    wm = lambda M: dense.Weights(dense.W_MATRIX, 0.0, M)                    # noqa: E731
    wp = lambda p: dense.Weights(dense.W_POWER, p, None)                    # noqa: E731
    gram = lambda weights=None, pairs=None: dense._pair_loss(X, spec, A=A, work=work, weights=weights,   # noqa: E731
                                                             pairs=pairs)
    times = _alternate({"none": gram, "p1": lambda: gram(wp(1.0)), "p2.5": lambda: gram(wp(2.5)),
                        "W": lambda: gram(wm(W), full.kept), "half": lambda: gram(wm(H), half.kept)}, reps)
    base = _median(times["none"])
    print("  %d x %d, d = 2, Quadratic, %d alternating calls; seconds, median (min - max), and the ratio to the "
          "unweighted call" % (n, nf, reps))
    print("  Gram source")
    for name, label in (("none", "mde_pair_loss (no weights)"), ("p1", "weights D^-1"), ("p2.5", "weights D^-2.5 (powf)"),
                        ("W", "weight matrix, every pair kept"), ("half", "weight matrix, %.1f %% of the pairs kept"
                                                                  % (100.0 * half.kept / full.kept))):
        print("    %-42s %s  %.3f x" % (label, summary(times[name]), _median(times[name]) / base))
    del H
    Dm = torch.cdist(A, A).contiguous()
    matrix = lambda weights=None, pairs=None: dense._pair_loss(X, spec, Dm=Dm, work=work, weights=weights,  # noqa: E731
                                                               pairs=pairs)
    times = _alternate({"none": matrix, "p1": lambda: matrix(wp(1.0)), "W": lambda: matrix(wm(W), full.kept)}, reps)
    base = _median(times["none"])
    print("  matrix source [n, n]")
    for name, label in (("none", "mde_pair_loss (no weights)"), ("p1", "weights D^-1"),
                        ("W", "weight matrix (a second [n, n] read)")):
        print("    %-42s %s  %.3f x" % (label, summary(times[name]), _median(times[name]) / base))
    print("  mde_pair_weights_check of the [n, n] weight matrix: %s (%.0f GB/s of W and its mirror image)"
          % (summary(t_check), 2 * 4.0 * n * n / _median(t_check) / 1e9))


def step_embed(n, max_iter):
    import pymde_amd
    from pymde_amd import losses, quality
    dev = torch.device("cuda", 0)
    data = mnist_like(n, NF, dev)
    print("  DenseMDE(data %d x %d, loss=Quadratic).embed(max_iter=%d)" % (n, NF, max_iter))
    for weights in (None, 1):
        problem = pymde_amd.DenseMDE(data, loss=losses.Quadratic, weights=weights)
        torch.manual_seed(0)
        t = clock(lambda: problem.embed(max_iter=max_iter))
        s = problem.solve_stats
        stress = quality.stress(data, problem.X, scale=1.0, sample=2000)
        print("    weights=%-4s %.3f s, %d iterations, %s evaluations, value %.6g, residual norm %.3g; "
              "quality.stress(scale=1.0, sample=2000) = %.6f"
              % (weights, t, s.iterations, s.evaluations, problem.value, problem.residual_norm, stress))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--old", default="20000x784")
    ap.add_argument("--weighted", default="20000x784")
    ap.add_argument("--embed", default="20000")
    ap.add_argument("--max-iter", type=int, default=60)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--limit", type=int, default=600, help="seconds per step")
    ap.add_argument("--tree", default=None, help="a second, built checkout whose `old` step runs around this one's")
    ap.add_argument("--tree-label", default="the checkout of --tree", help="what the record calls it")
    ap.add_argument("--out", default=None)
    ap.add_argument("--step", default=None, help=argparse.SUPPRESS)      # kind:a:b
    ap.add_argument("--package", default=ROOT, help=argparse.SUPPRESS)   # the checkout a step imports pymde_amd from
    a = ap.parse_args()
    if a.step:
        sys.path.insert(0, os.path.abspath(a.package))
        import pymde_amd
        assert os.path.dirname(os.path.dirname(os.path.abspath(pymde_amd.__file__))) == os.path.abspath(a.package)
        kind, x, y = (a.step.split(":") + ["0"])[:3]
        with torch.cuda.device(0):
            if kind == "old":
                step_old(int(x), int(y), a.reps)
            elif kind == "weighted":
                step_weighted(int(x), int(y), a.reps)
            else:
                step_embed(int(x), a.max_iter)
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

    steps = []
    for p in pairs(a.old):
        here = ("old:%d:%d" % p, ROOT, "this build")
        there = ("old:%d:%d" % p, a.tree, a.tree_label)
        steps += [there, here, there, here] if a.tree else [here]
    steps += [("weighted:%d:%d" % p, ROOT, "this build") for p in pairs(a.weighted)]
    steps += [("embed:%d" % int(n), ROOT, "this build") for n in a.embed.split(",") if n]
    say("tools/dense_weights_scale.py; every step a process of its own under a limit of %d s" % a.limit)
    for step, package, label in steps:
        say("")
        say("## %s (%s)" % (step, label))
        cmd = [sys.executable, os.path.abspath(__file__), "--step", step, "--package", package, "--reps", str(a.reps),
               "--max-iter", str(a.max_iter)]
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

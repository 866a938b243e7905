"""An embedding scored against a distance matrix or a Graph (csrc/mde_matrix_quality.hip) at user
sizes.

    python tools/graph_quality_scale.py [--square 20000] [--tall 1000000x1000] [--graph 1000000x64] [--m 1000] [--k 15]
                                        [--unchanged 20000] [--variant path/to/another/libmde_hip.so] [--reps 5]
                                        [--limit 600] [--out profiles/r26_graph_quality.txt]

Every step is a child process under its own time limit (--limit seconds); the first step that fails or runs past its
limit stops the run.  Times are medians (min - max) of --reps calls after a warm-up, a device synchronise on both
sides of every call; where several things are compared their calls alternate.  d = 2 throughout.  Bytes/s are
4 n m / time, the matrix read once, beside the 8 TB/s peak the README uses.

  square     an n x n matrix of uniform random dissimilarities (1 % of them inf), items = None: mde_matrix_moments,
             mde_matrix_histogram (64 bins) and mde_pair_loss (Quadratic) from the same matrix, the nearest walk the
             library had; mde_matrix_ranks with k = 15 and k = 64 (random lists).
  tall       the same kernels (no mde_pair_loss: it takes square matrices) on n x m with m random items.
  graph      the neighbour graph of tools/graph_landmarks_scale.py (n x nf rows, --k neighbours): graph_stress and
             graph_trustworthiness with sample = --m against a random 2-D projection, beside the graph.distances_from
             call of the same sources that both contain.
  unchanged  (with --variant) mde_pair_moments and mde_pair_loss from n x 784 data rows, this tree's library against
             the library named, in child processes that alternate.
No number is asserted anywhere."""
import argparse
import ctypes
import os
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from dense_place_scale import NF, clock, mnist_like, projection, summary  # noqa: E402

PEAK = 8.0e12


def median(times):
    return sorted(times)[len(times) // 2]


def alternate(calls, reps):
    """``calls``: name -> callable.  One warm-up each, then --reps rounds in which the calls alternate."""
    for fn in calls.values():
        fn()
    times = {name: [] for name in calls}
    for _ in range(reps):
        for name, fn in calls.items():
            times[name].append(clock(fn))
    return times


def report(times, nbytes):
    for name, t in times.items():
        rate = nbytes / median(t)
        print("  %-34s %s s   %.2f TB/s = %.0f %% of 8 TB/s" % (name, summary(t), rate / 1e12, 100.0 * rate / PEAK))


def step_walk(n, m, reps, k_list=(15, 64)):
    from pymde_amd import dense, losses, quality
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev)
    g.manual_seed(n + m)
    Dm = torch.rand((n, m), generator=g, device=dev) * 9.0 + 0.5
    Dm[torch.rand((n, m), generator=g, device=dev) < 0.01] = float("inf")
    X = torch.randn((n, 2), generator=g, device=dev)
    square = n == m
    items = None if square else torch.randint(0, n, (m,), generator=g, device=dev, dtype=torch.int32)
    counts = torch.zeros((64, 64), dtype=torch.int64, device=dev)
    calls = {
        "mde_matrix_moments": lambda: quality._matrix_moments(Dm, X, items),
        "mde_matrix_histogram, 64 bins": lambda: quality._matrix_histogram(Dm, X, items, 64, (0.0, 9.5), (0.0, 8.0),
                                                                           counts),
    }
    if square:
        Df = torch.where(torch.isfinite(Dm), Dm, torch.full_like(Dm, 3.0))   # mde_pair_loss expects finite entries
        spec = dense.loss_spec(losses.Quadratic)
        calls["mde_pair_loss from the matrix"] = lambda: dense._pair_loss(X, spec, Dm=Df)
    for k in k_list:
        idx = torch.randint(0, n, (m, k), generator=g, device=dev, dtype=torch.int32)
        calls["mde_matrix_ranks, k = %d" % k] = (lambda idx=idx: quality._matrix_ranks(Dm, idx, items))
    print("  %d x %d float32 (%.2f GB), d = 2, items %s" % (n, m, 4.0 * n * m / 1e9, "None" if square else "random"))
    times = alternate(calls, reps)
    report(times, 4.0 * n * m)
    if square:
        print("  ratio of the medians, mde_matrix_moments / mde_pair_loss: %.2f" % (
            median(times["mde_matrix_moments"]) / median(times["mde_pair_loss from the matrix"])))


def step_graph(n, nf, m, k, reps):
    from graph_landmarks_scale import neighbour_graph
    from pymde_amd import graph as G
    from pymde_amd import quality
    dev = torch.device("cuda", 0)
    data, g = neighbour_graph(n, nf, k, dev)
    X = projection(data, 1)
    sources = quality._sample_rows(n, m, 0).to(dev)
    calls = {
        "graph.distances_from, the same %d sources" % m: lambda: G.distances_from(g, sources),
        "graph_stress(sample=%d)" % m: lambda: quality.graph_stress(g, X, sample=m),
        "graph_trustworthiness(sample=%d)" % m: lambda: quality.graph_trustworthiness(g, X, k, sample=m),
    }
    times = alternate(calls, reps)
    for name, t in times.items():
        print("  %-44s %s s" % (name, summary(t)))
    mom = quality.graph_moments(g, X, sample=m)
    print("  batches of %d sources; %d pairs counted, %d missing (no path); stress %.4f, trustworthiness %.4f"
          % (quality._batch_columns(n), mom.count, mom.missing, quality.graph_stress(g, X, sample=m),
             quality.graph_trustworthiness(g, X, k, sample=m)))


def step_unchanged(n):
    """One warm-up and three timed calls of each unchanged entry point, with whatever library PYMDE_AMD_LIB_VARIANT
    names (a library from before this unit lacks its symbols: they are not bound then)."""
    from pymde_amd import _lib
    variant = os.environ.get("PYMDE_AMD_LIB_VARIANT")
    if variant:
        other = ctypes.CDLL(variant)
        for name in [s for s in _lib.SYMBOLS if not hasattr(other, s)]:
            del _lib.SYMBOLS[name]
    from pymde_amd import dense, losses, metrics, quality
    dev = torch.device("cuda", 0)
    A, _ = metrics.translated_rows(mnist_like(n, NF, dev, seed=0))
    X = projection(A, 1)
    spec = dense.loss_spec(losses.Quadratic)
    moments = lambda: quality._pair_moments(A, X)                        # noqa: E731
    loss = lambda: dense._pair_loss(X, spec, A=A)                        # noqa: E731
    moments(), loss()
    print("TIMES %.6f %.6f" % (min(clock(moments) for _ in range(3)), min(clock(loss) for _ in range(3))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--square", type=int, default=20000)
    ap.add_argument("--tall", default="1000000x1000")
    ap.add_argument("--graph", default="1000000x64")
    ap.add_argument("--unchanged", type=int, default=20000)
    ap.add_argument("--m", type=int, default=1000)
    ap.add_argument("--k", type=int, default=15)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--variant", default=None, help="another build of libmde_hip.so to time the unchanged entry points against")
    ap.add_argument("--limit", type=int, default=600, help="seconds per step")
    ap.add_argument("--out", default=None)
    ap.add_argument("--step", default=None, help=argparse.SUPPRESS)      # kind:n[:m]
    a = ap.parse_args()
    if a.step:
        kind, x, y = (a.step.split(":") + ["0", "0"])[:3]
        with torch.cuda.device(0):
            if kind == "walk":
                step_walk(int(x), int(y), a.reps)
            elif kind == "graph":
                step_graph(int(x), int(y), a.m, a.k, a.reps)
            else:
                step_unchanged(int(x))
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

    def child(step, env=None):
        cmd = [sys.executable, os.path.abspath(__file__), "--step", step, "--m", str(a.m), "--k", str(a.k), "--reps",
               str(a.reps)]
        try:
            p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=a.limit, env=env)
        except subprocess.TimeoutExpired:
            say("step %s ran past its limit of %d s: stopping" % (step, a.limit))
            return None
        text = p.stdout.decode(errors="replace").splitlines()
        if p.returncode != 0:
            for line in text:
                say(line)
            say("step %s exited with status %d: stopping" % (step, p.returncode))
            return None
        return text

    say("tools/graph_quality_scale.py; every step a process of its own under a limit of %d s; medians (min - max) of %d "
        "calls that alternate" % (a.limit, a.reps))
    steps = []
    if a.square:
        steps.append("walk:%d:%d" % (a.square, a.square))
    steps += ["walk:%s" % s.replace("x", ":") for s in a.tall.split(",") if s]
    steps += ["graph:%s" % s.replace("x", ":") for s in a.graph.split(",") if s]
    for step in steps:
        say("")
        say("## %s" % step)
        text = child(step)
        if text is None:
            return finish(1)
        for line in text:
            say(line)
    if a.variant and a.unchanged:
        say("")
        say("## unchanged:%d x %d -- this tree's library and %s, child processes that alternate (the least of three "
            "calls in each)" % (a.unchanged, NF, a.variant))
        times = {"tree": [], "variant": []}
        for _ in range(a.reps):
            for which in ("tree", "variant"):
                env = dict(os.environ)
                env.pop("PYMDE_AMD_LIB_VARIANT", None)
                if which == "variant":
                    env["PYMDE_AMD_LIB_VARIANT"] = os.path.abspath(a.variant)
                text = child("unchanged:%d" % a.unchanged, env)
                if text is None:
                    return finish(1)
                row = [line for line in text if line.startswith("TIMES ")][-1].split()
                times[which].append((float(row[1]), float(row[2])))
        for col, name in ((0, "mde_pair_moments"), (1, "mde_pair_loss (Quadratic)")):
            say("  %-28s this tree %s s | the other library %s s" % (
                name, summary([t[col] for t in times["tree"]]), summary([t[col] for t in times["variant"]])))
    return finish(0)


if __name__ == "__main__":
    sys.exit(main())

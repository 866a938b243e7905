"""Shortest paths from chosen sources and landmark MDS on graphs (csrc/mde_graph_sssp.hip) at user
sizes.

    python tools/graph_landmarks_scale.py [--compare 20000] [--scale 1000000x64] [--end 1000000x64] [--m 1000] [--k 15]
                                          [--reps 5] [--components 10] [--variant path/to/another/libmde_hip.so]
                                          [--limit 600]
                                          [--out profiles/r25_graph_landmarks.txt]

Every step is a child process under its own time limit (--limit seconds); the first step that fails or runs past its
limit stops the run.  Data: the mixture of tools/mnist_like.py as tools/dense_place_scale.py draws it on the GPU, with
--components centres (10, the default, falls into as many components under k = 15; 1 is one connected cloud); the
graph is preprocess.neighbor_graph(data, k) (lengths = distances), searched exactly below 100 000 rows and with
approximate=True from there on.  Times are medians (min - max) of --reps calls after a warm-up with a device
synchronise on both sides; where two things are compared their calls alternate.

  compare    n rows x 784: graph.distances_from(g, arange(n)) against graph.shortest_paths(g, retain_fraction=1e-6):
             both solve n single-source problems over the same adjacency (the latter row-major, consecutive sources,
             with an emit pass that keeps next to nothing), and the ratio of the two.
  unchanged  (with --variant) graph.shortest_paths and the shortest-path k-NN (mde_graph_knn) at the size of --compare,
             this tree's library against the library named, in child processes that alternate.
  scale      n x nf, m random sources: the time, the sweeps, 4 m half-edges sweeps / time (what relaxing every tile in
             every sweep would read, beside the 5-6 TB/s of gathered rows) and the share of tiles skipped.
  end        preserve_geodesics(data, n_neighbors=k, landmarks=m, seed=0).embed(placement_solver="rows"): the build
             time (k-NN graph, farthest-point selection, the m-source solve), the solve time and landmark_radius.
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

EXACT_BELOW = 100000
COMPONENTS = 10          # centres of the mixture (--components)


def neighbour_graph(n, nf, k, dev):
    from pymde_amd import preprocess
    data = mnist_like(n, nf, dev, components=COMPONENTS)
    search = {} if n < EXACT_BELOW else {"approximate": True}
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    g = preprocess.neighbor_graph(data, k, **search)
    torch.cuda.synchronize()
    t = time.perf_counter() - t0
    print("  %d x %d, k = %d%s: %d edges, neighbor_graph %.3f s" % (
        n, nf, k, ", approximate=True" if search else "", g.n_edges, t))
    return data, g


def step_compare(n, k, reps):
    from pymde_amd import graph as G
    dev = torch.device("cuda", 0)
    _, g = neighbour_graph(n, NF, k, dev)
    sources = torch.arange(n, device=dev)
    new = lambda: G.distances_from(g, sources)                          # noqa: E731
    old = lambda: G.shortest_paths(g, retain_fraction=1e-6)             # noqa: E731
    new(), old()
    t_new, t_old = [], []
    for _ in range(reps):
        t_new.append(clock(new))
        t_old.append(clock(old))
    stats = G.last_distances_stats()
    med = lambda t: sorted(t)[len(t) // 2]                              # noqa: E731
    print("  distances_from(g, arange(n))               %s s; %d sweeps, %.1f %% of the tiles skipped, %d heavy nodes"
          % (summary(t_new), stats["sweeps"],
             100.0 * (1.0 - stats["tiles_relaxed"] / float(stats["sweeps"] * stats["tiles_per_sweep"])),
             stats["heavy_nodes"]))
    print("  shortest_paths(g, retain_fraction=1e-6)    %s s" % summary(t_old))
    print("  ratio of the medians (shortest_paths / distances_from): %.2f" % (med(t_old) / med(t_new)))


def step_unchanged(n, k):
    """One warm-up and one timed call of each entry point, with whatever library PYMDE_AMD_LIB_VARIANT names."""
    from pymde_amd import graph as G
    dev = torch.device("cuda", 0)
    _, g = neighbour_graph(n, NF, k, dev)
    paths = lambda: G.shortest_paths(g, retain_fraction=1e-6)           # noqa: E731
    knn = lambda: G._neighbor_lists(g, k, graph_distances=True)         # noqa: E731
    paths(), knn()
    print("TIMES %.6f %.6f" % (clock(paths), clock(knn)))


def step_scale(n, nf, m, k, reps):
    from pymde_amd import graph as G
    dev = torch.device("cuda", 0)
    _, g = neighbour_graph(n, nf, k, dev)
    gen = torch.Generator(device="cpu")
    gen.manual_seed(0)
    sources = torch.randperm(n, generator=gen)[:m].to(dev)
    run = lambda: G.distances_from(g, sources)                          # noqa: E731
    D = run()
    joined = float(torch.isfinite(D).float().mean())
    del D
    times = [clock(run) for _ in range(reps)]
    stats = G.last_distances_stats()
    med = sorted(times)[len(times) // 2]
    half_edges = 2 * g.n_edges
    print("  distances_from, m = %d random sources: %s s; %d sweeps; 4 m half-edges sweeps / time = %.2f TB/s; "
          "%.1f %% of the tiles skipped (%d of %d relaxed); %d heavy nodes; %.1f %% of the pairs joined"
          % (m, summary(times), stats["sweeps"], 4.0 * m * half_edges * stats["sweeps"] / med / 1e12,
             100.0 * (1.0 - stats["tiles_relaxed"] / float(stats["sweeps"] * stats["tiles_per_sweep"])),
             stats["tiles_relaxed"], stats["sweeps"] * stats["tiles_per_sweep"], stats["heavy_nodes"], 100.0 * joined))


def step_end(n, nf, m, k, max_iter, eps):
    import pymde_amd
    dev = torch.device("cuda", 0)
    data = mnist_like(n, nf, dev, components=COMPONENTS)
    search = {} if n < EXACT_BELOW else {"approximate": True}
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    problem = pymde_amd.preserve_geodesics(data, n_neighbors=k, landmarks=m, seed=0, **search)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    X = problem.embed(placement_solver="rows", eps=eps, max_iter=max_iter)
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    print("  preserve_geodesics(%d x %d, n_neighbors=%d, landmarks=%d%s), init=%r, embed(placement_solver='rows', "
          "max_iter=%d, eps=%g):" % (n, nf, k, m, ", approximate=True" if search else "", problem.init, max_iter, eps))
    print("    building the problem %.3f s, embed() %.3f s; landmark_radius %.4f; value %.6g; finite: %s"
          % (t1 - t0, t2 - t1, problem.landmark_radius, problem.value, bool(torch.isfinite(X).all())))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--compare", type=int, default=20000)
    ap.add_argument("--scale", default="1000000x64")
    ap.add_argument("--end", default="1000000x64")
    ap.add_argument("--m", type=int, default=1000)
    ap.add_argument("--k", type=int, default=15)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--max-iter", type=int, default=300)
    ap.add_argument("--eps", type=float, default=1e-5)
    ap.add_argument("--components", type=int, default=10, help="centres of the mixture the rows are drawn from")
    ap.add_argument("--variant", default=None, help="another build of libmde_hip.so to time the unchanged entry points against")
    ap.add_argument("--limit", type=int, default=600, help="seconds per step")
    ap.add_argument("--out", default=None)
    ap.add_argument("--step", default=None, help=argparse.SUPPRESS)      # kind:n[:nf]
    a = ap.parse_args()
    global COMPONENTS
    COMPONENTS = a.components
    if a.step:
        kind, x, y = (a.step.split(":") + ["0", "0"])[:3]
        with torch.cuda.device(0):
            if kind == "compare":
                step_compare(int(x), a.k, a.reps)
            elif kind == "unchanged":
                step_unchanged(int(x), a.k)
            elif kind == "scale":
                step_scale(int(x), int(y), a.m, a.k, a.reps)
            else:
                step_end(int(x), int(y), a.m, a.k, a.max_iter, a.eps)
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
               str(a.reps), "--max-iter", str(a.max_iter), "--eps", str(a.eps), "--components", str(a.components)]
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

    say("tools/graph_landmarks_scale.py; every step a process of its own under a limit of %d s; rows from %d centres"
        % (a.limit, a.components))
    steps = []
    if a.compare:
        steps.append("compare:%d" % a.compare)
    steps += ["scale:%s" % s.replace("x", ":") for s in a.scale.split(",") if s]
    steps += ["end:%s" % s.replace("x", ":") for s in a.end.split(",") if s]
    for step in steps:
        say("")
        say("## %s" % step)
        text = child(step)
        if text is None:
            return finish(1)
        for line in text:
            say(line)
    if a.variant and a.compare:
        say("")
        say("## unchanged:%d -- this tree's library and %s, child processes that alternate" % (a.compare, a.variant))
        times = {"tree": [], "variant": []}
        for _ in range(a.reps):
            for which in ("tree", "variant"):
                env = dict(os.environ)
                env.pop("PYMDE_AMD_LIB_VARIANT", None)
                if which == "variant":
                    env["PYMDE_AMD_LIB_VARIANT"] = os.path.abspath(a.variant)
                text = child("unchanged:%d" % a.compare, env)
                if text is None:
                    return finish(1)
                row = [line for line in text if line.startswith("TIMES ")][-1].split()
                times[which].append((float(row[1]), float(row[2])))
        for col, name in ((0, "graph.shortest_paths(retain_fraction=1e-6)"), (1, "mde_graph_knn, shortest-path metric")):
            say("  %-44s this tree %s s | the other library %s s" % (
                name, summary([t[col] for t in times["tree"]]), summary([t[col] for t in times["variant"]])))
    return finish(0)


if __name__ == "__main__":
    sys.exit(main())

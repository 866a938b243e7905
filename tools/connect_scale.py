"""Connected components, nearest pairs between groups and connect= (csrc/mde_graph_components.hip,
csrc/mde_group_nearest.hip) at user sizes.

    python tools/connect_scale.py [--n 1000000] [--wide 200000x784] [--k 15] [--m 1000] [--reps 5] [--limit 900]
                                  [--skip-end] [--variant path/to/the/parent/libmde_hip.so]
                                  [--out profiles/r27_connect.txt]

Every step is a child process under its own time limit (--limit seconds); the first step that fails or runs past its
limit stops the run.  Data: the mixture of tools/mnist_like.py as tools/dense_place_scale.py draws it on the GPU (10
centres: the 15-NN graph falls into as many components; 1 centre: one connected cloud).  Times are medians (min - max)
of --reps synchronised calls after a warm-up; where two things are compared their calls alternate.

  components  graph.connected_components beside a single-source graph.distances_from on the same graph and beside
              scipy.sparse.csgraph.connected_components on the host (its CSR built beforehand), with rounds, launches
              and hooks: on the k-NN graph of n x 64 rows of the mixture, on a connected cloud, and on a path of n
              nodes under a random renumbering.
  pairs       preprocess._group_nearest_table with the component labels beside the exact search mde_knn of the same
              rows, and the share of (query block, candidate block) tiles the labels skip: on n x 64 and on --wide, rows
              in the order drawn, sorted by component, and in random order.
  end         preserve_geodesics(n x 64, landmarks=m, connect=True) beside the same call without connect: build time,
              embed(placement_solver="rows") time and quality.graph_stress(sample=1000) of both.
  unchanged   (with --variant) mde_knn, mde_knn_cross and mde_graph_distances_from, this tree's library against the
              library named, through ctypes on each library alone, in child processes that alternate.
No number is asserted anywhere."""
import argparse
import ctypes
import os
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from dense_place_scale import clock, mnist_like, summary  # noqa: E402

EXACT_BELOW = 100000


def neighbour_graph(data, k):
    from pymde_amd import preprocess
    search = {} if int(data.shape[0]) < EXACT_BELOW else {"approximate": True}
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    g = preprocess.neighbor_graph(data, k, **search)
    torch.cuda.synchronize()
    t = time.perf_counter() - t0
    print("  %d x %d, k = %d%s: %d edges, neighbor_graph %.3f s" % (
        data.shape[0], data.shape[1], k, ", approximate=True" if search else "", g.n_edges, t))
    return g


def step_components(kind, n, k, reps):
    import scipy.sparse as sp
    from scipy.sparse.csgraph import connected_components as scipy_components
    from pymde_amd import graph as G
    dev = torch.device("cuda", 0)
    if kind == "path":
        order = torch.randperm(n, generator=torch.Generator().manual_seed(0))
        e = torch.stack([order[:-1], order[1:]], dim=1)
        g = G.Graph.from_edges(e.to(dev), n_items=n)
        print("  a path of %d nodes under a random renumbering" % n)
    else:
        g = neighbour_graph(mnist_like(n, 64, dev, components=10 if kind == "mixture" else 1), k)
    g.plan()
    source = torch.zeros(1, dtype=torch.int64, device=dev)
    edges = g.edges.cpu().numpy()
    A = sp.coo_matrix((np.ones(len(edges)), (edges[:, 0], edges[:, 1])), shape=(n, n)).tocsr()
    ours = lambda: G.connected_components(g)                            # noqa: E731
    sssp = lambda: G.distances_from(g, source)                          # noqa: E731
    count, labels = ours()
    want_count, want = scipy_components(A, directed=False)
    same = count == want_count and bool((labels.cpu().numpy() == want).all())
    sssp()
    t_ours, t_sssp, t_host = [], [], []
    for _ in range(reps):
        t_ours.append(clock(ours))
        stats = G.last_components_stats()
        t_sssp.append(clock(sssp))
        t0 = time.perf_counter()
        scipy_components(A, directed=False)
        t_host.append(time.perf_counter() - t0)
    print("  %d components (labels equal scipy's: %s); %d rounds, %d launches, %d hooks" % (
        count, same, stats["rounds"], stats["launches"], stats["hooks"]))
    print("  connected_components                        %s s" % summary(t_ours))
    print("  distances_from, one source (%3d sweeps)      %s s" % (G.last_distances_stats()["sweeps"], summary(t_sssp)))
    print("  scipy connected_components on the host      %s s" % summary(t_host))


def skipped_share(labels, groups):
    """The share of (query block, candidate block) pairs of 64 x 64 rows that the label rule leaves out."""
    blocks = (torch.bincount(labels, minlength=groups).double() + 63).div(64).floor()
    total = float(blocks.sum()) ** 2
    above = blocks.flip(0).cumsum(0).flip(0) - blocks                   # blocks of a larger label
    return 1.0 - float((blocks * above).sum()) / total


def step_pairs(n, nf, k, reps):
    from pymde_amd import graph as G
    from pymde_amd import metrics, preprocess
    dev = torch.device("cuda", 0)
    data = mnist_like(n, nf, dev, components=10)
    count, labels = G.connected_components(neighbour_graph(data, k))
    print("  %d components; sizes %s" % (count, sorted(torch.bincount(labels).tolist(), reverse=True)[:12]))
    if count < 2:
        print("  one component: nothing to measure between")
        return
    rows, _ = metrics.translated_rows(data)
    del data
    exact = lambda X: (lambda: preprocess._dense_knn_lists(X, k))       # noqa: E731
    orders = {"as drawn": torch.arange(n, device=dev), "sorted by component": torch.argsort(labels, stable=True),
              "random order": torch.randperm(n, generator=torch.Generator().manual_seed(1)).to(dev)}
    reference = None
    for name, order in orders.items():
        X, lab = rows[order].contiguous(), labels[order].contiguous()
        walk = lambda: preprocess._group_nearest_table(X, lab, count)   # noqa: E731
        knn = exact(X)
        d2, _ = walk()
        knn()
        if reference is None:
            reference = d2
        t_walk, t_knn = [], []
        for _ in range(reps):
            t_walk.append(clock(walk))
            t_knn.append(clock(knn))
        med = lambda t: sorted(t)[len(t) // 2]                          # noqa: E731
        print("  rows %-20s group walk %s s | mde_knn (k = %d) %s s | ratio %.2f | %.1f %% of the tiles skipped | "
              "table equal to the first order's: %s" % (name, summary(t_walk), k, summary(t_knn),
                                                      med(t_knn) / med(t_walk), 100.0 * skipped_share(lab, count),
                                                      bool(torch.equal(d2, reference))))
        del X, lab


def step_end(n, m, k, connect, max_iter, eps):
    import pymde_amd
    from pymde_amd import quality
    dev = torch.device("cuda", 0)
    data = mnist_like(n, 64, dev, components=10)
    search = {} if n < EXACT_BELOW else {"approximate": True}
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    problem = pymde_amd.preserve_geodesics(data, n_neighbors=k, landmarks=m, seed=0, connect=bool(connect), **search)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    X = problem.embed(placement_solver="rows", eps=eps, max_iter=max_iter)
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    graph = problem.connection.graph if connect else pymde_amd.preprocess.neighbor_graph(data, k, **search)
    stress = float(quality.graph_stress(graph, X, sample=1000))
    moments = quality.graph_moments(graph, X, sample=1000)
    print("  preserve_geodesics(%d x 64, n_neighbors=%d, landmarks=%d, connect=%s%s): init=%r" % (
        n, k, m, bool(connect), ", approximate=True" if search else "", problem.init))
    if connect:
        print("    %d components joined by %d bridges" % (problem.connection.n_components,
                                                           int(problem.connection.bridges.shape[0])))
    print("    building the problem %.3f s, embed(placement_solver='rows') %.3f s; graph_stress(sample=1000) on %s "
          "graph %.4f with %d of the sampled pairs missing" % (t1 - t0, t2 - t1, "the connected" if connect else "its own",
                                                             stress, int(moments.missing)))


def step_unchanged(n, k):
    """One warm-up and one timed call of each unchanged entry point through ctypes on the library that
    CONNECT_SCALE_LIBRARY names (this tree's when unset), bound without the rest of the table: the parent's library
    lacks the entry points this change adds, so ``_lib.load`` (and ``PYMDE_AMD_LIB_VARIANT``) cannot bind it."""
    from pymde_amd import _lib
    path = os.environ.get("CONNECT_SCALE_LIBRARY") or _lib.LIB_PATH
    lib = ctypes.CDLL(path)
    for name in ("mde_knn", "mde_knn_cross", "mde_knn_cross_work_bytes", "mde_plan_create", "mde_plan_destroy",
                 "mde_graph_distances_from"):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = _lib.SYMBOLS[name]
    dev = torch.device("cuda", 0)
    stream = _lib.stream_ptr(dev)
    data = mnist_like(n, 64, dev, components=10)
    idx = torch.empty((n, k), dtype=torch.int32, device=dev)
    d2 = torch.empty((n, k), dtype=torch.float32, device=dev)
    sqn = torch.empty(n, dtype=torch.float32, device=dev)
    n_q = min(n, 4096)
    work = torch.empty(int(lib.mde_knn_cross_work_bytes(n_q, n, k, 0)), dtype=torch.uint8, device=dev)
    knn = lambda: lib.mde_knn(n, 64, _lib.ptr(data), k, _lib.ptr(idx), _lib.ptr(d2), _lib.ptr(sqn), stream)  # noqa: E731
    cross = lambda: lib.mde_knn_cross(n_q, n, 64, _lib.ptr(data), _lib.ptr(data), k, 0, _lib.ptr(idx), _lib.ptr(d2),  # noqa: E731
                                      _lib.ptr(work), stream)
    assert knn() == 0
    i = torch.arange(n, device=dev).unsqueeze(1).expand(n, k).reshape(-1)
    j = idx.reshape(-1).to(torch.int64)
    key = torch.unique(torch.minimum(i, j) * n + torch.maximum(i, j))
    edges = torch.stack([key // n, key % n], dim=1).contiguous()
    handle = ctypes.c_void_p()
    assert lib.mde_plan_create(n, int(edges.shape[0]), _lib.ptr(edges), 0, n, stream, ctypes.byref(handle)) == 0
    sources = torch.arange(0, n, max(1, n // 64), device=dev)[:64].contiguous()
    out = torch.empty((n, int(sources.numel())), dtype=torch.float32, device=dev)
    sssp = lambda: lib.mde_graph_distances_from(handle, None, 0.0, int(sources.numel()), _lib.ptr(sources),  # noqa: E731
                                                _lib.ptr(out), stream)
    assert cross() == 0 and sssp() == 0
    print("TIMES %.6f %.6f %.6f" % (clock(knn), clock(cross), clock(sssp)))
    lib.mde_plan_destroy(handle)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1000000)
    ap.add_argument("--wide", default="200000x784")
    ap.add_argument("--k", type=int, default=15)
    ap.add_argument("--m", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--max-iter", type=int, default=300)
    ap.add_argument("--eps", type=float, default=1e-5)
    ap.add_argument("--unchanged-n", type=int, default=100000, help="rows of the unchanged-kernel comparison")
    ap.add_argument("--skip-end", action="store_true")
    ap.add_argument("--variant", default=None, help="the parent commit's libmde_hip.so, to time the unchanged kernels against")
    ap.add_argument("--limit", type=int, default=900, help="seconds per step")
    ap.add_argument("--out", default=None)
    ap.add_argument("--step", default=None, help=argparse.SUPPRESS)      # kind:a[:b[:c]]
    a = ap.parse_args()
    if a.step:
        part = a.step.split(":")
        with torch.cuda.device(0):
            if part[0] == "components":
                step_components(part[1], int(part[2]), a.k, a.reps)
            elif part[0] == "pairs":
                step_pairs(int(part[1]), int(part[2]), a.k, a.reps)
            elif part[0] == "end":
                step_end(int(part[1]), a.m, a.k, int(part[2]), a.max_iter, a.eps)
            else:
                step_unchanged(int(part[1]), a.k)
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
               str(a.reps), "--max-iter", str(a.max_iter), "--eps", str(a.eps)]
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

    say("tools/connect_scale.py; every step a process of its own under a limit of %d s; seconds, median (min - max) of "
        "%d calls" % (a.limit, a.reps))
    steps = ["components:%s:%d" % (kind, a.n) for kind in ("mixture", "cloud", "path")]
    steps += ["pairs:%d:64" % a.n] + ["pairs:%s" % s.replace("x", ":") for s in a.wide.split(",") if s]
    if not a.skip_end:
        steps += ["end:%d:0" % a.n, "end:%d:1" % a.n]
    for step in steps:
        say("")
        say("## %s" % step)
        text = child(step)
        if text is None:
            return finish(1)
        for line in text:
            say(line)
    if a.variant:
        say("")
        say("## unchanged:%d -- mde_knn, mde_knn_cross (4096 queries), mde_graph_distances_from (64 sources); this "
            "tree's library and %s, child processes that alternate" % (a.unchanged_n, a.variant))
        times = {"tree": [], "variant": []}
        for _ in range(a.reps):
            for which in ("tree", "variant"):
                env = dict(os.environ)
                env.pop("CONNECT_SCALE_LIBRARY", None)
                if which == "variant":
                    env["CONNECT_SCALE_LIBRARY"] = os.path.abspath(a.variant)
                text = child("unchanged:%d" % a.unchanged_n, env)
                if text is None:
                    return finish(1)
                row = [line for line in text if line.startswith("TIMES ")][-1].split()
                times[which].append(tuple(float(v) for v in row[1:4]))
        for col, name in enumerate(("mde_knn", "mde_knn_cross", "mde_graph_distances_from")):
            say("  %-28s this tree %s s | the other library %s s" % (
                name, summary([t[col] for t in times["tree"]]), summary([t[col] for t in times["variant"]])))
    return finish(0)


if __name__ == "__main__":
    sys.exit(main())

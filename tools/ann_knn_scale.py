"""Approximate (inverted-file) k-NN against the exact kernel at user sizes, k = 15, default knobs.

    python tools/ann_knn_scale.py [--shapes 200000x64,200000x784,1000000x64,1000000x784,4000000x64]
                                  [--exact-max 1000000] [--embed 1000000x784 | --embed none]
    (a shape NxFpP runs n_probe = P instead of the default, without the exact search)

Data: the class mixture the defaults were calibrated on -- 10 classes, means ~ N(0, 9 I), each class a
random 10-12 dimensional linear patch, plus N(0, 0.25 I) noise -- generated on the GPU from a seed.
Per shape: wall time of k_nearest_neighbors exact (mde_knn lists + the graph; skipped above --exact-max
items) and approximate, the approximate search split into k-means / assignment / probe lists / scan
(synchronised stages), the sampled recall@15 (1 000 rows, as verbose=True logs it) and, where the exact
lists exist, the recall over every row; the scan's useful rate (candidate pairs x n_features x 2 over the
scan stage) beside mde_knn's (n^2 x n_features x 2 over the exact lists).  --embed times
preserve_neighbors(approximate_neighbors=True) stage by stage and embed() on the mixture."""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pymde_amd import ann, preprocess  # noqa: E402

K = 15


def mixture(n, nf, classes=10, seed=0, dev="cuda"):
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    labels = torch.randint(0, classes, (n,), generator=g, device=dev)
    means = 3.0 * torch.randn(classes, nf, generator=g, device=dev)
    X = means[labels] + 0.5 * torch.randn(n, nf, generator=g, device=dev)
    for c in range(classes):
        dim = 10 + c % 3
        basis = torch.randn(dim, nf, generator=g, device=dev)
        rows = (labels == c).nonzero()[:, 0]
        for r0 in range(0, rows.shape[0], 1 << 20):
            r = rows[r0:r0 + (1 << 20)]
            X[r] += torch.randn(r.shape[0], dim, generator=g, device=dev) @ basis
    return X.contiguous()


def timed(fn, *a, **kw):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn(*a, **kw)
    torch.cuda.synchronize()
    return out, time.perf_counter() - t


def full_recall(truth, idx):
    hits = 0
    for r0 in range(0, truth.shape[0], 1 << 18):
        t, a = truth[r0:r0 + (1 << 18)], idx[r0:r0 + (1 << 18)]
        hits += int((t[:, :, None] == a[:, None, :]).any(2).sum())
    return hits / float(truth.numel())


def shape_row(n, nf, exact_max, n_probe=None):
    X = mixture(n, nf, seed=n + nf)
    dev = X.device
    row = {"n": n, "nf": nf}
    stages = {}
    with torch.cuda.device(dev):
        idx, _ = ann.knn_lists(X, K, n_probe=n_probe, timings=stages)
        (edges, _), t_graph = timed(preprocess._neighbor_lists_to_graph, n, K, idx, None, None, dev)
        _, row["approx_s"] = timed(preprocess.k_nearest_neighbors, X, K, approximate=True, n_probe=n_probe)
        row["recall_sampled"] = preprocess._estimated_recall(X, idx, K)
        if n <= exact_max:
            (truth, _), t_lists = timed(preprocess._dense_knn_lists, X, K)
            _, t_egraph = timed(preprocess._neighbor_lists_to_graph, n, K, truth, None, None, dev)
            row["exact_s"] = t_lists + t_egraph
            row["exact_rate"] = 2.0 * n * n * nf / t_lists / 1e12
            row["recall_full"] = full_recall(truth, idx)
            del truth
    for s in ("kmeans", "assign", "probe", "scan"):
        row[s] = stages[s]
    row["graph_s"] = t_graph
    row["pairs_frac"] = stages["candidate_pairs"] / float(n) ** 2
    row["scan_rate"] = 2.0 * stages["candidate_pairs"] * nf / stages["scan"] / 1e12
    row["imbalance"] = stages["imbalance"]
    row["tiles"] = stages["tiles"]
    sizes = stages["list_sizes"]
    row["lists"] = "%d (%d..%d)" % (stages["n_lists"], int(sizes.min()), int(sizes.max()))
    return row


def embed_stages(n, nf):
    """preserve_neighbors(approximate_neighbors=True) with its stages timed (wrapped, synchronised)."""
    import pymde_amd
    from pymde_amd import quadratic
    X = mixture(n, nf, seed=n + nf)
    spent = {}

    def wrap(mod, name, label):
        fn = getattr(mod, name)

        def timed_fn(*a, **kw):
            out, t = timed(fn, *a, **kw)
            spent[label] = spent.get(label, 0.0) + t
            return out
        setattr(mod, name, timed_fn)
        return mod, name, fn

    saved = [wrap(preprocess, "k_nearest_neighbors", "knn"), wrap(quadratic, "spectral", "spectral"),
             wrap(preprocess, "sample_edges", "repulsive")]
    try:
        mde, t_build = timed(pymde_amd.preserve_neighbors, X, embedding_dim=2, seed=0, approximate_neighbors=True)
    finally:
        for mod, name, fn in saved:
            setattr(mod, name, fn)
    _, t_embed = timed(mde.embed)
    other = t_build - sum(spent.values())
    return ("preserve_neighbors(%d x %d, approximate_neighbors=True): build %.2f s = k-NN %.2f + spectral "
            "init %.2f + repulsive edges %.2f + other %.2f; embed() %.2f s (%d edges)"
            % (n, nf, t_build, spent.get("knn", 0), spent.get("spectral", 0), spent.get("repulsive", 0), other,
               t_embed, mde.edges.shape[0]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="200000x64,200000x784,1000000x64,1000000x784,4000000x64")
    ap.add_argument("--exact-max", type=int, default=1000000)
    ap.add_argument("--embed", default="1000000x784")
    args = ap.parse_args()
    with torch.cuda.device(0):
        ann.knn_lists(mixture(20000, 64), K)                  # warm-up: code objects, torch kernels
        preprocess._dense_knn_lists(mixture(20000, 64), K)
    print("approximate k-NN (IVF, default n_lists = round(sqrt(n)), n_probe = 32) against exact, k = %d; "
          "times in s" % K)
    print("%8s %4s %8s %8s %7s %7s %7s %7s %7s %6s %7s %7s %7s %8s %6s %5s  %s"
          % ("n", "nf", "exact", "approx", "speedup", "kmeans", "assign", "probe", "scan", "pairs", "recall",
             "rec_all", "scanTF", "exactTF", "tiles", "imbal", "lists (min..max size)"), flush=True)
    for s in args.shapes.split(","):
        s, _, probe = s.partition("p")                     # NxF or NxFpP: n_probe = P instead of the default
        n, nf = (int(v) for v in s.split("x"))
        r = shape_row(n, nf, 0 if probe else args.exact_max, int(probe) if probe else None)   # exact once
        ex = r.get("exact_s")
        print("%s%8d %4d %8s %8.3f %7s %7.3f %7.3f %7.3f %7.3f %6.3f %7.3f %7s %7.1f %8s %6d %5.2f  %s"
              % ("p=%-3s" % probe if probe else "", n, nf, "%.3f" % ex if ex else "-", r["approx_s"],
                 "%.1f" % (ex / r["approx_s"]) if ex else "-",
                 r["kmeans"], r["assign"], r["probe"], r["scan"], r["pairs_frac"], r["recall_sampled"],
                 "%.3f" % r["recall_full"] if ex else "-", r["scan_rate"],
                 "%.1f" % r["exact_rate"] if ex else "-", r["tiles"], r["imbalance"], r["lists"]), flush=True)
        torch.cuda.empty_cache()
    if args.embed != "none":
        n, nf = (int(v) for v in args.embed.split("x"))
        print(embed_stages(n, nf), flush=True)


if __name__ == "__main__":
    main()

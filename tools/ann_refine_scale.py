"""The neighbour-of-neighbour refinement of the approximate k-NN (ann.refine_lists) at user sizes, k = 15.

    python tools/ann_refine_scale.py [--shapes 200000x784,1000000x64,1000000x784] [--data patches,isotropic]
                                     [--runs 5] [--parent-ann PATH]

Data: ``patches`` is the class mixture of tests/test_gpu_ann.py (10 classes, means ~ N(0, 9 I), each a random
10-12 dimensional linear patch, plus N(0, 0.25 I) noise); ``isotropic`` is the mixture of tools/mnist_like.py
(10 centres ~ N(0, 4 I), unit isotropic noise), drawn on the GPU.  Per shape and data set, for n_refine in
{0, 1, 2} at the default knobs and for n_probe = 64 unrefined: the wall time of ann.knn_lists and of its scan
and refine laps (medians of --runs synchronised runs after one warm-up), the recall@15 over all rows against
the exact lists, the rows each pass changed and the distances it evaluated per row.  --parent-ann names another
ann.py (the previous commit's) whose knn_lists is timed alternately with this one's at n_refine = 0: both launch
the same kernels of the same library."""
import argparse
import importlib.util
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pymde_amd import ann, preprocess  # noqa: E402
from ann_knn_scale import full_recall, mixture  # noqa: E402

K = 15


def isotropic(n, nf, seed=0, dev="cuda"):
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    centers = 2.0 * torch.randn(10, nf, generator=g, device=dev)
    labels = torch.randint(0, 10, (n,), generator=g, device=dev)
    X = centers[labels]
    for r0 in range(0, n, 1 << 18):
        X[r0:r0 + (1 << 18)] += torch.randn(min(1 << 18, n - r0), nf, generator=g, device=dev)
    return X.contiguous()


def wall(fn, *a, **kw):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn(*a, **kw)
    torch.cuda.synchronize()
    return out, time.perf_counter() - t


def config_row(X, truth, runs, **kw):
    n = X.shape[0]
    ann.knn_lists(X, K, **kw)                                       # warm-up
    total, scan, refine = [], [], []
    for _ in range(runs):
        stats = {}
        (idx, _), t = wall(ann.knn_lists, X, K, timings=stats, **kw)
        total.append(t)
        scan.append(stats["scan"])
        refine.append(stats.get("refine", 0.0))
    med = statistics.median
    changed = stats.get("refine_changed", [])
    per_row = ["%.1f" % (e / n) for e in stats.get("refine_evaluated", [])]
    return ("%8.3f %8.3f %8.3f %7.3f %8.4f  %-18s %s"
            % (med(total), med(scan), med(refine), med(refine) / med(scan), full_recall(truth, idx),
               ",".join(str(c) for c in changed) or "-", ",".join(per_row) or "-"))


def against_parent(X, path, runs):
    spec = importlib.util.spec_from_file_location("parent_ann", path)
    parent = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(parent)
    ann.knn_lists(X, K)
    parent.knn_lists(X, K)
    here, there = [], []
    for _ in range(runs):
        there.append(wall(parent.knn_lists, X, K)[1])
        here.append(wall(ann.knn_lists, X, K, n_refine=0)[1])
    return ("  n_refine=0 against the parent's knn_lists, alternately: %.3f s (%.3f..%.3f) against %.3f s (%.3f..%.3f)"
            % (statistics.median(here), min(here), max(here), statistics.median(there), min(there), max(there)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="200000x784,1000000x64,1000000x784")
    ap.add_argument("--data", default="patches,isotropic")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--parent-ann", default=None)
    args = ap.parse_args()
    print("refinement of the approximate k-NN, k = %d, default n_lists = round(sqrt(n)), n_probe = 32 unless given; "
          "times in s, medians of %d runs" % (K, args.runs), flush=True)
    with torch.cuda.device(0):
        for shape in args.shapes.split(","):
            n, nf = (int(v) for v in shape.split("x"))
            for data in args.data.split(","):
                X = mixture(n, nf, seed=n + nf) if data == "patches" else isotropic(n, nf, seed=n + nf)
                (truth, _), t_exact = wall(preprocess._dense_knn_lists, X, K)
                print("%d x %d, %s (exact lists %.2f s)" % (n, nf, data, t_exact), flush=True)
                print("  %-22s %8s %8s %8s %7s %8s  %-18s %s" % ("", "total", "scan", "refine", "ref/scan", "recall",
                                                                 "rows changed", "distances per row"), flush=True)
                for label, kw in (("n_refine=0", {}), ("n_refine=1", {"n_refine": 1}), ("n_refine=2", {"n_refine": 2}),
                                  ("n_probe=64", {"n_probe": 64})):
                    print("  %-22s %s" % (label, config_row(X, truth, args.runs, **kw)), flush=True)
                if args.parent_ann:
                    print(against_parent(X, args.parent_ann, args.runs), flush=True)
                del X, truth
                torch.cuda.empty_cache()


if __name__ == "__main__":
    main()

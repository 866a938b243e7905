"""The affinity kernels (pymde_amd.affinity, csrc/mde_affinity.hip) at user sizes, beside the 1 / 2 path.

    python tools/affinity_scale.py [--shapes 200000x64x15,1000000x64x15,1000000x64x64] [--runs 5]
                                   [--recipe 1000000x64]

Data: the mixture of tools/mnist_like.py (10 centres ~ N(0, 4 I), unit isotropic noise), drawn on the GPU.  Per
shape n x features x k, on the exact Euclidean lists: the wall time of mde_knn_calibrate (both kinds, through
affinity.calibrate), of mde_knn_symmetrize (both rules, through affinity.symmetrize) and of
preprocess._neighbor_lists_to_graph -- the unchanged path that turns the same lists into the 1 / 2 graph -- as
medians (min - max) of --runs synchronised calls after one warm-up, the symmetrisation and the 1 / 2 path called
alternately.  --recipe: the graph stage alone (k_nearest_neighbors beside neighbor_affinities) and one build of
preserve_neighbors(weights="perplexity") beside the same call without the keyword, each twice ("" skips it); what
the build adds beyond the graph stage is spent downstream, in the spectral start and the layout of the edge
kernel, which take arbitrary float32 weights in place of the two values 1 and 2."""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pymde_amd  # noqa: E402
from pymde_amd import affinity, preprocess  # noqa: E402


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


def ms(times):
    return "%8.2f ms (%.2f - %.2f)" % (1e3 * statistics.median(times), 1e3 * min(times), 1e3 * max(times))


def shape_rows(n, nf, k, runs):
    X = isotropic(n, nf, seed=n + nf)
    (idx, d2, _, root, scale), t_lists = wall(preprocess._neighbor_lists, X, k)
    del X
    print("%d x %d, k = %d (exact lists %.2f s)" % (n, nf, k, t_lists), flush=True)
    calibrations = {}
    for kind in ("perplexity", "umap"):
        affinity.calibrate(idx, d2, kind, root=root, scale=scale)                     # warm-up
        times = []
        for _ in range(runs):
            calibrations[kind], t = wall(affinity.calibrate, idx, d2, kind, root=root, scale=scale)
            times.append(t)
        print("  calibrate %-28s %s" % (kind, ms(times)), flush=True)
    for kind, rule in (("perplexity", "mean"), ("umap", "union")):
        cal = calibrations[kind]
        affinity.symmetrize(cal.idx, cal.conditionals, rule)
        preprocess._neighbor_lists_to_graph(n, k, idx, d2, None, idx.device)
        ours, theirs = [], []
        for _ in range(runs):
            (edges, _), t = wall(affinity.symmetrize, cal.idx, cal.conditionals, rule)
            ours.append(t)
            (edges12, _), t = wall(preprocess._neighbor_lists_to_graph, n, k, idx, d2, None, idx.device)
            theirs.append(t)
        assert torch.equal(edges, edges12)
        ratio = statistics.median(ours) / statistics.median(theirs)
        print("  symmetrize %-27s %s   %d edges" % (rule, ms(ours), edges.shape[0]), flush=True)
        print("  _neighbor_lists_to_graph (1 / 2)       %s   ratio %.2f" % (ms(theirs), ratio), flush=True)
    torch.cuda.empty_cache()


def recipe_rows(n, nf):
    X = isotropic(n, nf, seed=n + nf)
    for _ in range(2):                                                              # (the first pair warms up)
        _, t12 = wall(preprocess.k_nearest_neighbors, X, 15)
        _, taff = wall(affinity.neighbor_affinities, X, 15)
        print("  graph stage alone at k = 15: k_nearest_neighbors %.2f s, neighbor_affinities %.2f s" % (t12, taff),
              flush=True)
    for weights in (None, "perplexity", None, "perplexity"):                       # (the first pair warms up)
        pymde_amd.seed(0)
        mde, t = wall(pymde_amd.preserve_neighbors, X, seed=0, weights=weights)
        print("  preserve_neighbors(%d x %d, weights=%r): %.2f s, %d edges" % (n, nf, weights, t, int(mde.p)),
              flush=True)
        del mde
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="200000x64x15,1000000x64x15,1000000x64x64")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--recipe", default="1000000x64")
    args = ap.parse_args()
    print("affinity kernels beside the 1 / 2 path; medians (min - max) of %d synchronised calls" % args.runs, flush=True)
    with torch.cuda.device(0):
        for shape in [s for s in args.shapes.split(",") if s]:
            n, nf, k = (int(v) for v in shape.split("x"))
            shape_rows(n, nf, k, args.runs)
        if args.recipe:
            n, nf = (int(v) for v in args.recipe.split("x"))
            recipe_rows(n, nf)


if __name__ == "__main__":
    main()

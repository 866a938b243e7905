"""The embedding quality scores (pymde_amd.quality, mde_knn_ranks) at user sizes, beside the exact k-NN search.

    python tools/quality_scale.py [--shapes 70000x784:uniform,200000x784:mixture] [--out profiles/r13_quality.txt]

For every shape n x nf (data as in tools/bf16_knn_scale.py) and a 2-D embedding of the same rows (a random linear
projection to two dimensions: a stand-in, the timings do not depend on what it shows) one
process measures, each as a warm-up call and then the median of three calls timed with a device synchronise on
both sides:

  mde_knn            the exact search at k = 15 in data space (nf features) and in embedding space (nf = 2): the
                     same Gram pass as a rank pass, so the yardstick
  mde_knn_ranks      the rank kernels alone (thresholds, count, fold; automatic slices) for lists of m = 15 and
                     m = 64 in both spaces, and the ratio to mde_knn in the same space
  trustworthiness,   through pymde_amd.quality at n_neighbors = 15 (column statistics, the search of one space,
  continuity         the rank pass in the other, one read-back)

The lines go to stdout and, with --out, to that file.  No time is asserted anywhere."""
import argparse
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

K = 15


def timed(fn, calls=3):
    fn()                                    # warm-up
    times = []
    for _ in range(calls):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t)
    return sorted(times)[len(times) // 2], times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="70000x784:uniform,200000x784:mixture")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from bf16_knn_scale import make
    from pymde_amd import preprocess, quality
    dev = torch.device("cuda", 0)
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    say("tools/quality_scale.py on %s; seconds, median of three calls after a warm-up [the three]"
        % torch.cuda.get_device_name(dev))
    with torch.cuda.device(dev):
        for shape in args.shapes.split(","):
            dims, kind = shape.split(":")
            n, nf = (int(v) for v in dims.split("x"))
            data = make(kind, n, nf, dev)
            g = torch.Generator(device=dev)
            g.manual_seed(n)
            X = (data @ torch.randn(nf, 2, generator=g, device=dev)).contiguous()
            X = (X - X.mean(0)).contiguous()
            say("")
            say("%d x %d %s, embedding %d x 2" % (n, nf, kind, n))
            lists = {}
            for name, rows in (("data", data), ("embedding", X)):
                med, times = timed(lambda: preprocess._dense_knn_lists(rows, K))
                say("  mde_knn k=15, %-9s space (nf = %3d)  %.4f %s" % (name, rows.shape[1], med,
                                                                         [round(t, 4) for t in times]))
                lists[name] = (rows, med)
            for m in (15, 64):
                idx = {"data": preprocess._dense_knn_lists(X, m)[0], "embedding": preprocess._dense_knn_lists(data, m)[0]}
                for name in ("data", "embedding"):
                    rows, knn_med = lists[name]
                    med, times = timed(lambda: quality._ranks(rows, rows, idx[name], True))
                    tflops = 2.0 * n * n * rows.shape[1] / med / 1e12
                    say("  mde_knn_ranks m=%2d, %-9s space     %.4f %s  = %.2f x mde_knn  (%.1f TF/s of Gram)"
                        % (m, name, med, [round(t, 4) for t in times], med / knn_med, tflops))
            for name, score in (("trustworthiness", quality.trustworthiness), ("continuity", quality.continuity)):
                value = [None]

                def run():
                    value[0] = score(data, X, n_neighbors=K)
                med, times = timed(run)
                say("  quality.%-15s k=15           %.4f %s  value %.6f" % (name, med, [round(t, 4) for t in times],
                                                                           value[0]))
            del data, X, lists, idx
            torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

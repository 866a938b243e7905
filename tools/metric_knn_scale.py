"""k-NN (k = 15) under the four metrics on dense data, all in one process.

    python tools/metric_knn_scale.py [--shapes 70000x784,200000x128] [--reps 5] [--metrics euclidean,cosine]
                                     [--out profiles/r08_metric_knn.txt]

Data: uniform (0, 1] float32 generated on the GPU from a seed.  Per shape and metric: the median wall time
of ``preprocess.k_nearest_neighbors`` (lists + graph) over --reps synchronised calls after one warm-up call
of every metric, and the time of the neighbour lists alone (Euclidean: the column statistics, the
translation to the column means where the rule of DESIGN section 6 asks for it -- it does on this data -- and
``mde_knn``).  Cosine and correlation are reported beside Euclidean with the difference and the time two passes
over the data take at the 6 TB/s HBM rate of profiles/r03_streamprobe.txt; Manhattan beside its VALU floor,
n^2 nf element pairs x 2 operations over 256 CUs x 4 SIMDs x lanes per clock at 2.4 GHz (16 lanes as the
issue derives it, and the 32 of the SIMD-32 issue rate)."""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pymde_amd import metrics, preprocess  # noqa: E402

K = 15
HBM = 6.0e12


def timed(fn, reps):
    times = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t)
    return statistics.median(times), min(times), max(times)


def lists(X, metric):
    if metric == metrics.EUCLIDEAN:
        return preprocess._euclidean_knn_lists(X, K)
    return preprocess._metric_knn_lists(X, K, metric)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="70000x784,200000x128")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--metrics", default=",".join(metrics.METRICS))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    chosen = [metrics.resolve(m) for m in a.metrics.split(",")]
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    g = torch.Generator(device="cuda")
    g.manual_seed(0)
    warm = torch.rand(4000, 100, generator=g, device="cuda")
    for m in chosen:
        preprocess.k_nearest_neighbors(warm, K, metric=m)
    say("k-NN at k = %d under the four metrics, one process; seconds, median of %d (min - max)" % (K, a.reps))
    for shape in a.shapes.split(","):
        n, nf = (int(v) for v in shape.split("x"))
        X = (torch.rand(n, nf, generator=g, device="cuda") * 0.999 + 0.001).contiguous()
        for m in chosen:                                # warm every metric at this shape
            preprocess.k_nearest_neighbors(X, K, metric=m)
        graph, only = {}, {}
        say("## %d x %d" % (n, nf))
        say("%-12s %28s %28s" % ("metric", "k_nearest_neighbors", "neighbour lists alone"))
        for m in chosen:
            graph[m] = timed(lambda: preprocess.k_nearest_neighbors(X, K, metric=m), a.reps)
            only[m] = timed(lambda: lists(X, m), a.reps)
            say("%-12s %10.4f (%.4f - %.4f) %10.4f (%.4f - %.4f)" % ((m,) + graph[m] + only[m]))
        passes = 2.0 * 4.0 * n * nf / HBM
        for m in (metrics.COSINE, metrics.CORRELATION):
            if m not in chosen or metrics.EUCLIDEAN not in chosen:
                continue
            say("%s - euclidean: %+.4f s (lists alone); one read and one write of the data at 6 TB/s: %.5f s"
                % (m, only[m][0] - only[metrics.EUCLIDEAN][0], passes))
        pairs = float(n) * n * nf
        for lanes in (16, 32) if metrics.MANHATTAN in chosen else ():
            floor = pairs * 2.0 / (256 * 4 * lanes * 2.4e9)
            say("manhattan lists %.4f s against the VALU floor at %d lanes per SIMD and clock %.4f s: %.2fx"
                % (only[metrics.MANHATTAN][0], lanes, floor, only[metrics.MANHATTAN][0] / floor))
        del X
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

"""The global embedding scores (pymde_amd.quality: stress, distance_correlation, shepard_histogram; mde_pair_moments,
mde_pair_histogram) at user sizes, beside the exact k-NN search of the same matrix in the same run.

    python tools/global_quality_scale.py [--full 70000,200000] [--sampled 1000000] [--sample 2000]
                                         [--out profiles/r14_global_quality.txt]

The data are the stand-in of tools/mnist_like.py -- a 10-component Gaussian mixture in R^784, centres N(0, 4 I), unit
noise -- drawn on the GPU from a seeded generator, and the embedding is a random linear projection of the same rows to
two dimensions (a stand-in: the timings do not depend on what it shows).  Every figure is a warm-up call and then the
median of three calls timed with a device synchronise on both sides, in one process.

  mde_knn              the exact self-join at k = 15 on the data: the same Gram pass, so the yardstick
  mde_pair_moments     the kernels alone on the prepared rows (row norms, walk, fold, totals; automatic slices)
  stress, distance_    the public calls end to end (column statistics, the moments pass, one read-back)
  correlation
  mde_pair_histogram   the kernels alone at 64 x 64 bins, three times: over [0, max D] x [0, max E] ("spread": the
                       mixture's distances fill the range), over a range 64 times as wide, which puts every pair
                       into bin (0, 0) ("one bin": the worst same-address contention of the LDS atomics), and the
                       spread range on a single Gaussian blob, whose data distances concentrate in a few bins
  shepard_histogram    the public call end to end with range=None (a moments pass, then the histogram pass)

--sampled: the same calls with sample= query rows against all rows of a larger matrix; the yardstick there is the
query-against-corpus search of the same queries (mde_knn_cross).  No time is asserted anywhere."""
import argparse
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

K = 15
NF = 784
BINS = 64


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


def mnist_like(n, dev, components=10):
    g = torch.Generator(device=dev)
    g.manual_seed(n)
    centres = 2.0 * torch.randn(components, NF, generator=g, device=dev)
    labels = torch.randint(0, components, (n,), generator=g, device=dev)
    data = torch.randn(n, NF, generator=g, device=dev)
    data += centres[labels]
    return data.contiguous()


def embedding_of(data, seed):
    g = torch.Generator(device=data.device)
    g.manual_seed(seed)
    X = data @ torch.randn(data.shape[1], 2, generator=g, device=data.device)
    return (X - X.mean(0)).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--full", default="70000,200000")
    ap.add_argument("--sampled", default="1000000")
    ap.add_argument("--sample", type=int, default=2000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from pymde_amd import metrics, preprocess, quality
    dev = torch.device("cuda", 0)
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    def line(name, med, times, base=None, note=""):
        ratio = "  = %.2f x %s" % (med / base[1], base[0]) if base else ""
        say("  %-44s %.4f %s%s%s" % (name, med, [round(t, 4) for t in times], ratio, note))

    def histogram_lines(A, B, q, base, label):
        top = quality._pair_moments(A, B, q_rows=q)[2][5:7].cpu().tolist()
        spread = ((0.0, top[0]), (0.0, top[1]))
        wide = ((0.0, BINS * top[0]), (0.0, BINS * top[1]))
        for name, rng in (("spread", spread), ("one bin", wide)):
            counts = [None]

            def run():
                counts[0] = quality._pair_histogram(A, B, BINS, rng[0], rng[1], q_rows=q)
            med, times = timed(run)
            c = counts[0]
            line("mde_pair_histogram 64x64, %s, %s" % (label, name), med, times, base,
                 "  (%d bins hold pairs, the fullest %.1f %%)" % (int((c > 0).sum()), 100.0 * float(c.max()) / float(c.sum())))

    say("tools/global_quality_scale.py on %s; seconds, median of three calls after a warm-up [the three]"
        % torch.cuda.get_device_name(dev))
    with torch.cuda.device(dev):
        for n in [int(v) for v in args.full.split(",") if v]:
            data = mnist_like(n, dev)
            X = embedding_of(data, n)
            A = metrics.translated_rows(data)[0]
            B = metrics.translated_rows(X)[0]
            say("")
            say("%d x %d mixture, embedding %d x 2, every row a query (%.3g ordered pairs)" % (n, NF, n, n * (n - 1.0)))
            knn = timed(lambda: preprocess._dense_knn_lists(A, K))
            line("mde_knn k=15 (the exact search of the data)", *knn)
            base = ("mde_knn", knn[0])
            med, times = timed(lambda: quality._pair_moments(A, B))
            line("mde_pair_moments (kernels alone)", med, times, base,
                 "  (%.1f TF/s of Gram)" % (2.0 * n * n * (NF + 2) / med / 1e12))
            value = [None]
            for name, score in (("stress", quality.stress), ("distance_correlation", quality.distance_correlation)):
                def run():
                    value[0] = score(data, X)
                med, times = timed(run)
                line("quality.%s" % name, med, times, base, "  value %.6f" % value[0])
            histogram_lines(A, B, None, base, "mixture")
            blob = torch.randn(n, NF, device=dev)
            histogram_lines(blob, embedding_of(blob, n + 1), None, base, "one blob")
            del blob

            def run():
                value[0] = quality.shepard_histogram(data, X)[3]
            med, times = timed(run)
            line("quality.shepard_histogram range=None", med, times, base, "  counted %d" % value[0])
            del data, X, A, B
            torch.cuda.empty_cache()
        for n in [int(v) for v in args.sampled.split(",") if v]:
            m = args.sample
            data = mnist_like(n, dev)
            X = embedding_of(data, n)
            A = metrics.translated_rows(data)[0]
            B = metrics.translated_rows(X)[0]
            q = quality._sample_rows(n, m, 0).to(device=dev, dtype=torch.int32)
            say("")
            say("%d x %d mixture, embedding %d x 2, sample=%d query rows (%.3g ordered pairs)"
                % (n, NF, n, m, m * (n - 1.0)))
            Q = A[q.long()].contiguous()
            knn = timed(lambda: preprocess._cross_knn_lists(Q, A, K))
            line("mde_knn_cross k=15 (the same queries)", *knn)
            base = ("mde_knn_cross", knn[0])
            med, times = timed(lambda: quality._pair_moments(A, B, q_rows=q))
            line("mde_pair_moments (kernels alone)", med, times, base,
                 "  (%.1f TF/s of Gram)" % (2.0 * m * n * (NF + 2) / med / 1e12))
            value = [None]
            for name, score in (("stress", quality.stress), ("distance_correlation", quality.distance_correlation)):
                def run():
                    value[0] = score(data, X, sample=m)
                med, times = timed(run)
                line("quality.%s sample=%d" % (name, m), med, times, base, "  value %.6f" % value[0])
            histogram_lines(A, B, q, base, "mixture")

            def run():
                value[0] = quality.shepard_histogram(data, X, sample=m)[3]
            med, times = timed(run)
            line("quality.shepard_histogram sample=%d" % m, med, times, base, "  counted %d" % value[0])
            del data, X, A, B, Q
            torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

"""Query-against-corpus k-NN (``mde_knn_cross``) at user sizes, k = 15, nf = 784.

    python tools/cross_knn_scale.py [--shapes 1000x1000000,10000x1000000,100000x1000000] [--reps 5]
                                    [--limit 300] [--out profiles/r09_cross_knn.txt]

Per shape (n_q x n_c) two steps, each a child process of its own under a time limit of --limit seconds; the
first step that fails or runs out of time ends the script.
  * cross: ``mde_knn_cross`` with automatic slices and with ``slices=1``, alternating, --reps synchronised
    calls each after one warm-up call of both; median (min - max) seconds, the slice count the automatic rule
    picked, the useful rate 2 n_q n_c nf / time, and whether the two results are bit-identical.
  * stacked: the self-join ``mde_knn`` on the n_c + n_q stacked rows, the only way to the same lists without
    the cross search; one synchronised call after a warm-up at a small size (the call is tens of seconds).
Data: uniform [0, 1) float32 generated on the GPU from a seed.  Times are host clocks around synchronised
calls; they include the scratch allocation of the Python wrappers."""
import argparse
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K, NF = 15, 784


def _data(n_q, n_c):
    import torch
    g = torch.Generator(device="cuda")
    g.manual_seed(n_q + n_c)
    C = torch.rand(n_c, NF, generator=g, device="cuda")
    Q = torch.rand(n_q, NF, generator=g, device="cuda")
    return Q, C


def _clock(fn):
    import torch
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t, out


def step_cross(n_q, n_c, reps):
    import torch
    sys.path.insert(0, ROOT)
    from pymde_amd import _lib, preprocess
    Q, C = _data(n_q, n_c)
    lib = _lib.load()
    norms = 4 * (n_q + n_c)
    picked = (int(lib.mde_knn_cross_work_bytes(n_q, n_c, K, 0)) - norms) // (8 * n_q * K) or 1
    _, auto = _clock(lambda: preprocess._cross_knn_lists(Q, C, K, 0))
    _, one = _clock(lambda: preprocess._cross_knn_lists(Q, C, K, 1))
    same = torch.equal(auto[0], one[0]) and torch.equal(auto[1], one[1])
    times = {0: [], 1: []}
    for _ in range(reps):
        for s in (0, 1):
            times[s].append(_clock(lambda: preprocess._cross_knn_lists(Q, C, K, s))[0])
    flop = 2.0 * n_q * n_c * NF
    for s, name in ((0, "automatic (%d slices)" % picked), (1, "slices=1")):
        med = statistics.median(times[s])
        print("cross %-24s %9.4f (%.4f - %.4f) s  %6.1f TFLOP/s useful" % (name, med, min(times[s]), max(times[s]),
                                                                        flop / med / 1e12))
    print("automatic / slices=1: %.2fx; results bit-identical: %s"
          % (statistics.median(times[0]) / statistics.median(times[1]), same))
    print("RESULT auto %.6f" % statistics.median(times[0]))


def step_stacked(n_q, n_c):
    import torch
    sys.path.insert(0, ROOT)
    from pymde_amd import preprocess
    Q, C = _data(n_q, n_c)
    preprocess._dense_knn_lists(C[:4096].contiguous(), K)          # code load and first-launch costs
    X = torch.cat([C, Q])
    del Q, C
    t, _ = _clock(lambda: preprocess._dense_knn_lists(X, K))
    print("stacked self-join mde_knn on %d rows %9.4f s  %6.1f TFLOP/s" % (X.shape[0], t,
                                                                        2.0 * X.shape[0] ** 2 * NF / t / 1e12))
    print("RESULT stacked %.6f" % t)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="1000x1000000,10000x1000000,100000x1000000")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--limit", type=int, default=300, help="seconds per step")
    ap.add_argument("--out", default=None)
    ap.add_argument("--step", default=None, help=argparse.SUPPRESS)      # cross:n_q:n_c or stacked:n_q:n_c
    a = ap.parse_args()
    if a.step:
        kind, n_q, n_c = a.step.split(":")
        if kind == "cross":
            step_cross(int(n_q), int(n_c), a.reps)
        else:
            step_stacked(int(n_q), int(n_c))
        return 0
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def finish(code):
        if a.out:
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")
        return code

    say("query-against-corpus k-NN, k = %d, nf = %d; seconds, median of %d (min - max)" % (K, NF, a.reps))
    for shape in a.shapes.split(","):
        n_q, n_c = (int(v) for v in shape.split("x"))
        say("## n_q = %d, n_c = %d" % (n_q, n_c))
        result = {}
        for kind in ("cross", "stacked"):
            cmd = [sys.executable, os.path.abspath(__file__), "--step", "%s:%d:%d" % (kind, n_q, n_c), "--reps",
                   str(a.reps)]
            try:
                p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=a.limit)
            except subprocess.TimeoutExpired:
                say("step %s ran past its limit of %d s: stopping" % (kind, a.limit))
                return finish(1)
            for line in p.stdout.decode(errors="replace").splitlines():
                if line.startswith("RESULT "):
                    _, key, value = line.split()
                    result[key] = float(value)
                else:
                    say(line)
            if p.returncode != 0:
                say("step %s exited with status %d: stopping" % (kind, p.returncode))
                return finish(1)
        say("stacked self-join / cross search (automatic slices): %.1fx" % (result["stacked"] / result["auto"]))
    return finish(0)


if __name__ == "__main__":
    sys.exit(main())

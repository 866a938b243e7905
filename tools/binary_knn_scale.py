"""The Jaccard / Hamming k-NN search on bit-packed rows (k = 15) beside the float32 Euclidean search of the same
bits, and the unchanged float32 kernels beside the parent commit's build.

    python tools/binary_knn_scale.py [--part self|cross|parent|precheck|all] [--reps 5] [--parent-lib PATH]
                                     [--variant-lib PATH] [--float-limit-gb 40]
                                     [--out profiles/r28_binary_knn.txt]

Every step -- each self-join shape, the cross search, the parent comparison, the pre-check comparison -- runs as a
child process under a time limit of its own (``--step`` is what a child is started with); after a step that
fails or runs out of time no further step is started.

Data: random bits of density 1/8 (the AND of three random words) generated on the GPU from a seed and handed over
as ``np.packbits`` bytes (``binary.from_packbits``).  Random bits have no neighbourhoods: the distances of a row
concentrate, so a tile offers the merge more candidates than clustered fingerprints would.

self:   200k x 2048, 1M x 2048 and 1M x 166 bits: ``binary.knn_lists`` (``mde_bits_knn``, self-join) under both
        distances, and ``preprocess._dense_knn_lists`` (``mde_knn``) on the unpacked 0/1 float32 matrix where that
        matrix is at most --float-limit-gb; on 0/1 data the squared Euclidean distance is the Hamming count, so
        the two rank alike.  Alternating calls, medians of --reps with min and max, every call synchronised.
cross:  10k queries against 1M x 2048 bits with automatic slices and with slices = 1.
parent: ``mde_knn`` and ``mde_knn_l1`` at 70k x 784 from this build and from --parent-lib (a build of the parent
        commit), each library bound alone through ctypes, alternating.
precheck: ``mde_bits_knn`` (self-join, Jaccard) at 200k x 2048 and 1M x 166 bits from this build and from
        --variant-lib, a build of csrc/mde_bits.hip with -DBITS_PRECHECK=0 (every merge thread scans its row of
        every tile), bound the same way: what the flag test before the merge is worth.

The share of the VALU peak is n_q n_c nw 2 instructions per lane (one AND and one popcount-add per word pair) over
256 CUs x 4 SIMDs x lanes per clock at 2.4 GHz, at 16 lanes (a wave's instruction over four clocks) and at the 32
of the SIMD-32 issue rate, as tools/metric_knn_scale.py reports Manhattan.  Lines are appended to --out as they
are measured."""
import argparse
import ctypes
import os
import statistics
import subprocess
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pymde_amd import _lib, binary, preprocess  # noqa: E402

K = 15
SELF_SHAPES = [(200000, 2048), (1000000, 2048), (1000000, 166)]
CROSS_SHAPE = (10000, 1000000, 2048)
PARENT_SHAPE = (70000, 784)
PRECHECK_SHAPES = [(200000, 2048), (1000000, 166)]
# the steps of every part and the seconds a child process gets for each (start-up included)
STEPS = {"self": [("self:0", 240), ("self:1", 900), ("self:2", 300)], "cross": [("cross", 240)],
         "parent": [("parent", 240)], "precheck": [("precheck", 300)]}


def timed_alternating(fns, reps):
    """{name: (median, min, max)} of ``reps`` synchronised calls of every function, taken in turn."""
    times = {name: [] for name in fns}
    for rep in range(reps):
        for name, fn in fns.items():
            torch.cuda.synchronize()
            t = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times[name].append(time.perf_counter() - t)
        print("  (round %d of %d timed)" % (rep + 1, reps), file=sys.stderr, flush=True)
    return {name: (statistics.median(v), min(v), max(v)) for name, v in times.items()}


def random_bits(n, nf, generator, distance="jaccard"):
    nb = (nf + 7) // 8
    packed = torch.randint(0, 256, (n, nb), generator=generator, device="cuda", dtype=torch.uint8)
    for _ in range(2):
        packed &= torch.randint(0, 256, (n, nb), generator=generator, device="cuda", dtype=torch.uint8)
    if nf % 8:
        packed[:, -1] &= (1 << (nf % 8)) - 1
    return binary.from_packbits(packed, nf, distance, bitorder="little")


def valu_share(n_q, n_c, nw, seconds, lanes):
    return float(n_q) * n_c * nw * 2.0 / (256 * 4 * lanes * 2.4e9) / seconds


def fmt(t):
    return "%9.4f (%.4f - %.4f)" % t


def part_self(say, reps, float_limit_gb, which):
    g = torch.Generator(device="cuda")
    g.manual_seed(which)
    for n, nf in SELF_SHAPES[which:which + 1]:
        bits = random_bits(n, nf, g)
        nw = int(bits.words.shape[1])
        ham = bits.with_distance("hamming")
        fns = {"jaccard": lambda: binary.knn_lists(bits, bits, K, self_join=True),
               "hamming": lambda: binary.knn_lists(ham, ham, K, self_join=True)}
        float_bytes = 4.0 * n * nf
        X = None
        if float_bytes <= float_limit_gb * 1e9:
            X = torch.empty((n, nf), dtype=torch.float32, device="cuda")
            for r0 in range(0, n, 65536):
                part = binary.BitMatrix(bits.words[r0:r0 + 65536], bits.counts[r0:r0 + 65536], nf)
                X[r0:r0 + 65536] = part.unpack()
            fns["float32 euclidean"] = lambda: preprocess._dense_knn_lists(X, K)
        say("## self-join %d x %d bits (%d words per row): packed %.3f GB, float32 %.3f GB"
            % (n, nf, nw, 4.0 * n * nw / 1e9, float_bytes / 1e9))
        for fn in fns.values():                         # one warm-up call of every search at this shape
            fn()
        got = timed_alternating(fns, reps)
        for name, t in got.items():
            say("%-18s %s s" % (name, fmt(t)))
        for name in ("jaccard", "hamming"):
            say("%s: %.1f %% of the VALU peak at 16 lanes per SIMD and clock, %.1f %% at 32"
                % (name, 100 * valu_share(n, n, nw, got[name][0], 16), 100 * valu_share(n, n, nw, got[name][0], 32)))
        if X is not None:
            idx_h, _ = binary.knn_lists(ham, ham, K, self_join=True)
            idx_f, _ = preprocess._dense_knn_lists(X, K)
            same = float((idx_h[:4096] == idx_f[:4096]).float().mean())
            say("float32 euclidean / hamming: %.2fx (time); memory 32.0x; lists equal in %.4f of the first 4096 rows' "
                "entries (0/1 data: d2 is the Hamming count, exact in float32)"
                % (got["float32 euclidean"][0] / got["hamming"][0], same))
        else:
            say("float32 euclidean: not run (the float32 matrix is above --float-limit-gb %.0f)" % float_limit_gb)
        del X, bits, ham, fns
        torch.cuda.empty_cache()


def part_cross(say, reps):
    g = torch.Generator(device="cuda")
    g.manual_seed(1)
    n_q, n_c, nf = CROSS_SHAPE
    q, c = random_bits(n_q, nf, g), random_bits(n_c, nf, g)
    nw = int(c.words.shape[1])
    fns = {"automatic slices": lambda: binary.knn_lists(q, c, K, slices=0),
           "slices = 1": lambda: binary.knn_lists(q, c, K, slices=1)}
    say("## cross search: %d queries against %d x %d bits" % (n_q, n_c, nf))
    a, b = fns["automatic slices"](), fns["slices = 1"]()
    say("the two results are identical: %s" % bool(torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])))
    got = timed_alternating(fns, reps)
    for name, t in got.items():
        say("%-18s %s s; %.1f %% of the VALU peak at 16 lanes, %.1f %% at 32"
            % (name, fmt(t), 100 * valu_share(n_q, n_c, nw, t[0], 16), 100 * valu_share(n_q, n_c, nw, t[0], 32)))


def _bind(path, names=("mde_knn", "mde_knn_l1")):
    lib = ctypes.CDLL(path)
    for name in names:
        res, args = _lib.SYMBOLS[name]
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    return lib


def part_parent(say, reps, parent_lib):
    n, nf = PARENT_SHAPE
    say("## the unchanged kernels at %d x %d, k = %d: this build beside the parent commit's" % (n, nf, K))
    if not parent_lib or not os.path.exists(parent_lib):
        say("not run: no --parent-lib (a build of the parent commit's libmde_hip.so) was given")
        return
    g = torch.Generator(device="cuda")
    g.manual_seed(2)
    X = torch.rand(n, nf, generator=g, device="cuda")
    idx = torch.empty((n, K), dtype=torch.int32, device="cuda")
    val = torch.empty((n, K), dtype=torch.float32, device="cuda")
    sqn = torch.empty(n, dtype=torch.float32, device="cuda")
    libs = {"this build": _bind(_lib.LIB_PATH), "parent": _bind(parent_lib)}
    stream = _lib.stream_ptr(X.device)

    def knn(lib):
        _lib.check(lib.mde_knn(n, nf, _lib.ptr(X), K, _lib.ptr(idx), _lib.ptr(val), _lib.ptr(sqn), stream))

    def l1(lib):
        _lib.check(lib.mde_knn_l1(n, nf, _lib.ptr(X), K, _lib.ptr(idx), _lib.ptr(val), stream))

    for kernel, call in (("mde_knn", knn), ("mde_knn_l1", l1)):
        out = {}
        for name, lib in libs.items():
            call(lib)
            torch.cuda.synchronize()
            out[name] = (idx.clone(), val.clone())
        same = torch.equal(out["this build"][0], out["parent"][0]) and torch.equal(out["this build"][1],
                                                                                   out["parent"][1])
        got = timed_alternating({name: (lambda lib=lib: call(lib)) for name, lib in libs.items()}, reps)
        for name, t in got.items():
            say("%-12s %-12s %s s" % (kernel, name, fmt(t)))
        lo, hi = got["parent"][1], got["parent"][2]
        med = got["this build"][0]
        where = "lies inside" if lo <= med <= hi else ("lies BELOW (faster than)" if med < lo else
                                                       "LIES ABOVE (slower than)")
        say("%s: outputs bit-identical: %s; this build's median %.6f s %s the parent's min-to-max spread "
            "%.6f - %.6f s" % (kernel, same, med, where, lo, hi))


def part_precheck(say, reps, variant_lib):
    say("## the flag test before the merge: this build beside a build with -DBITS_PRECHECK=0, self-join, Jaccard, "
        "k = %d" % K)
    if not variant_lib or not os.path.exists(variant_lib):
        say("not run: no --variant-lib (a build of csrc/mde_bits.hip with -DBITS_PRECHECK=0) was given")
        return
    names = ("mde_bits_knn", "mde_bits_knn_work_bytes")
    libs = {"with the test": _bind(_lib.LIB_PATH, names), "every row scanned": _bind(variant_lib, names)}
    g = torch.Generator(device="cuda")
    g.manual_seed(3)
    for n, nf in PRECHECK_SHAPES:
        bits = random_bits(n, nf, g)
        nw = int(bits.words.shape[1])
        idx = torch.empty((n, K), dtype=torch.int32, device="cuda")
        val = torch.empty((n, K), dtype=torch.float32, device="cuda")
        work = torch.empty(max(int(libs["with the test"].mde_bits_knn_work_bytes(n, n, K, 1)), 8), dtype=torch.uint8,
                           device="cuda")
        stream = _lib.stream_ptr(idx.device)

        def call(lib):
            _lib.check(lib.mde_bits_knn(n, n, nw, nf, _lib.ptr(bits.words), _lib.ptr(bits.counts),
                                        _lib.ptr(bits.words), _lib.ptr(bits.counts), 1, bits.kind, K, 1, _lib.ptr(idx),
                                        _lib.ptr(val), _lib.ptr(work), stream))

        out = {}
        for name, lib in libs.items():                  # the warm-up call of either build, and its result
            call(lib)
            torch.cuda.synchronize()
            out[name] = (idx.clone(), val.clone())
        a, b = out["with the test"], out["every row scanned"]
        got = timed_alternating({name: (lambda lib=lib: call(lib)) for name, lib in libs.items()}, reps)
        say("%d x %d bits (%d words per row); outputs bit-identical: %s"
            % (n, nf, nw, bool(torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]))))
        for name, t in got.items():
            say("%-18s %s s" % (name, fmt(t)))
        say("every row scanned / with the test: %.3fx" % (got["every row scanned"][0] / got["with the test"][0]))
        del bits, idx, val, work
        torch.cuda.empty_cache()


def run_step(step, a, say):
    _lib.require_gpu()
    if step.startswith("self:"):
        part_self(say, a.reps, a.float_limit_gb, int(step[5:]))
    elif step == "cross":
        part_cross(say, a.reps)
    elif step == "parent":
        part_parent(say, a.reps, a.parent_lib)
    elif step == "precheck":
        part_precheck(say, a.reps, a.variant_lib)
    else:
        raise SystemExit("unknown step %r" % step)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", default="all", choices=sorted(STEPS) + ["all"])
    ap.add_argument("--step", default=None, help="run one step in this process (what a child is started with)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--variant-lib", default=None)
    ap.add_argument("--float-limit-gb", type=float, default=40.0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    def say(s):
        print(s, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(s + "\n")

    if a.step is not None:
        run_step(a.step, a, say)
        return
    say("# binary k-NN at k = %d; seconds, median of %d alternating synchronised calls (min - max); every step a "
        "child process under its own time limit" % (K, a.reps))
    parts = ["self", "cross", "parent", "precheck"] if a.part == "all" else [a.part]
    passed = ["--reps", str(a.reps), "--float-limit-gb", str(a.float_limit_gb)]
    for flag, value in (("--parent-lib", a.parent_lib), ("--variant-lib", a.variant_lib), ("--out", a.out)):
        if value:
            passed += [flag, value]
    for step, limit in (s for p in parts for s in STEPS[p]):
        try:
            rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", step] + passed,
                                timeout=limit).returncode
        except subprocess.TimeoutExpired:
            rc = None
        if rc != 0:
            say("step %s did not complete (%s); no further step is started"
                % (step, "time limit of %d s" % limit if rc is None else "exit code %d" % rc))
            raise SystemExit(1)


if __name__ == "__main__":
    main()

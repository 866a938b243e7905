"""Sparse k-NN (k = 15) at user sizes: the sparse kernel, densify + the dense kernel (where the dense copy
is at most --dense-max-gb) and what the dispatcher picks; mde_sparse_distances on sampled pairs.

    python tools/sparse_knn_scale.py [--cases mnist,scrna,text,counts] [--pairs 5e7] [--dense-max-gb 16]

Inputs are generated on the GPU from a seed: every row draws round(density * nf) column ids (duplicates
merged), values are counts in [1, 5] (MNIST-like: uniform in (0, 1]).  Times are wall-clock around
synchronised calls, best of --reps after one warm-up call of every path at a small size."""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pymde_amd import _lib, preprocess, sparse  # noqa: E402

CASES = {
    "mnist": ("MNIST-like", 70000, 784, 0.19),
    "scrna": ("scRNA-like counts", 100000, 20000, 0.05),
    "text": ("text-like", 100000, 100000, 0.001),
    "counts": ("larger counts", 400000, 20000, 0.02),
}


def make_csr(n, nf, density, seed, unit=False, dev="cuda"):
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    m = max(1, int(round(density * nf)))
    keys = []
    for r0 in range(0, n, 20000):               # in slices: the key sort stays small
        r1 = min(n, r0 + 20000)
        cols = torch.randint(0, nf, (r1 - r0, m), generator=g, device=dev)
        rows = torch.arange(r0, r1, device=dev)[:, None]
        keys.append(torch.unique(rows * nf + cols))
    keys = torch.cat(keys)
    rows, cols = keys // nf, keys % nf
    if unit:
        vals = torch.rand(keys.shape[0], generator=g, device=dev) * 0.999 + 0.001
    else:
        vals = torch.randint(1, 6, (keys.shape[0],), generator=g, device=dev).float()
    indptr = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    torch.cumsum(torch.bincount(rows, minlength=n), 0, out=indptr[1:])
    return sparse.DeviceCSR(indptr, cols.to(torch.int32).contiguous(), vals.contiguous(), (n, nf))


def timed(fn, reps):
    best = float("inf")
    out = None
    for _ in range(reps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        best = min(best, time.perf_counter() - t)
    return best, out


def sparse_distances(csr, edges):
    lib = _lib.load()
    out = torch.empty(edges.shape[0], dtype=torch.float32, device=csr.device)
    _lib.check(lib.mde_sparse_distances(csr.n, csr.n_features, csr.nnz, _lib.ptr(csr.indptr), _lib.ptr(csr.indices),
                                        _lib.ptr(csr.values), edges.shape[0], _lib.ptr(edges), _lib.ptr(out),
                                        _lib.stream_ptr(csr.device)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="mnist,scrna,text,counts")
    ap.add_argument("--k", type=int, default=15)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--pairs", type=float, default=5e7)
    ap.add_argument("--dense-max-gb", type=float, default=16.0)
    a = ap.parse_args()
    k = a.k
    warm = make_csr(3000, 2000, 0.05, 1)
    preprocess._sparse_knn_lists(warm, k)
    preprocess._dense_knn_lists(warm.to_dense(), k)
    torch.cuda.synchronize()
    print("sparse k-NN, k = %d; times in s (best of %d)" % (k, a.reps))
    print("%-18s %7s %7s %8s %11s %9s %9s %9s %8s %10s" % ("input", "n", "nf", "density", "nnz", "sparse",
                                                           "dense", "picked", "pick/best", "sparse TFMA/s"))
    for key in a.cases.split(","):
        name, n, nf, density = CASES[key]
        csr = make_csr(n, nf, density, 7, unit=(key == "mnist"))
        ts, (idx_s, d2_s) = timed(lambda: preprocess._sparse_knn_lists(csr, k), a.reps)
        td = None
        if 4.0 * n * nf <= a.dense_max_gb * 2 ** 30:
            td, (idx_d, d2_d) = timed(lambda: preprocess._dense_knn_lists(csr.to_dense(), k), 1)
            if key != "mnist":     # integer data: both paths exact
                assert torch.equal(idx_s, idx_d) and torch.equal(d2_s, d2_d), key
            del idx_d, d2_d
        densify = preprocess._densify_sparse_knn(n, nf, csr.nnz, csr.device)
        picked = td if densify else ts
        best = min(x for x in (ts, td) if x is not None)
        fma = float(n) * csr.nnz           # query x stored-entry products the sparse kernel makes
        print("%-18s %7d %7d %8.4f %11d %9.3f %9s %9s %8.3f %10.2f" % (
            name, n, nf, csr.nnz / (n * float(nf)), csr.nnz, ts, "%.3f" % td if td is not None else "not run",
            "dense" if densify else "sparse", picked / best if picked is not None else float("nan"),
            fma / ts / 1e12), flush=True)
        if key == "scrna" and a.pairs > 0:
            edges = preprocess.sample_edges(n, int(a.pairs), seed=0)
            tp, out = timed(lambda: sparse_distances(csr, edges), a.reps)
            print("mde_sparse_distances, %s, %d pairs: %.3f s (%.1f M pairs/s), mean %.3f" % (
                name, edges.shape[0], tp, edges.shape[0] / tp / 1e6, float(out.mean())), flush=True)
            del edges, out
        del csr, idx_s, d2_s
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()

"""Record the raw outputs of the exact k-NN C entry points (mde_knn, mde_knn_cross, mde_knn_l1) on the GPU.

    python tests/golden/make_knn_bits.py

writes ``knn_bits.npz`` next to this file: for every case the float32 inputs and the (idx int32, d2 / dist
float32) arrays exactly as the entry point left them.  tests/test_gpu_knn_bits.py holds later builds to
these bits, so the file is regenerated only when a change of the arithmetic is intended -- run this at the
commit whose results are the reference, never at the commit under test.

The shapes are the smallest at which each edge of the 64 x 64 tile can go wrong: two full row blocks plus two
ragged rows, a ragged column tile, feature counts of less than a chunk, a chunk + 1 and three chunks with
the last ragged, fewer rows than k, and corpus slices of which some are empty.
"""
import os

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "knn_bits.npz")
MAX_BYTES = 256 * 1024

# mde_knn: name -> (n, nf, k); the seed of a case is its position
KNN_CASES = {"knn_n130_nf1_k64": (130, 1, 64), "knn_n130_nf33_k15": (130, 33, 15),
             "knn_n130_nf70_k1": (130, 70, 1), "knn_n5_nf8_k15": (5, 8, 15)}
CROSS_CASE = ("cross_q65_c130_nf50_k15", 65, 130, 50, 15, (1, 7))
L1_CASE = ("l1_n130_nf33_k15", 130, 33, 15)


def _data(seed, *shape):
    return (np.random.default_rng(seed).standard_normal(shape) + 0.5).astype(np.float32)


def run_knn(lib_mod, X, k):
    lib = lib_mod.load()
    n, nf = X.shape
    idx = torch.full((n, k), -7, dtype=torch.int32, device=X.device)
    d2 = torch.full((n, k), -7.0, dtype=torch.float32, device=X.device)
    work = torch.empty(n, dtype=torch.float32, device=X.device)
    lib_mod.check(lib.mde_knn(n, nf, lib_mod.ptr(X), k, lib_mod.ptr(idx), lib_mod.ptr(d2), lib_mod.ptr(work),
                              lib_mod.stream_ptr(X.device)))
    torch.cuda.synchronize()
    return idx.cpu().numpy(), d2.cpu().numpy()


def run_l1(lib_mod, X, k):
    lib = lib_mod.load()
    n, nf = X.shape
    idx = torch.full((n, k), -7, dtype=torch.int32, device=X.device)
    d = torch.full((n, k), -7.0, dtype=torch.float32, device=X.device)
    lib_mod.check(lib.mde_knn_l1(n, nf, lib_mod.ptr(X), k, lib_mod.ptr(idx), lib_mod.ptr(d),
                                 lib_mod.stream_ptr(X.device)))
    torch.cuda.synchronize()
    return idx.cpu().numpy(), d.cpu().numpy()


def run_cross(lib_mod, Q, C, k, slices):
    lib = lib_mod.load()
    n_q, n_c, nf = Q.shape[0], C.shape[0], C.shape[1]
    idx = torch.full((n_q, k), -7, dtype=torch.int32, device=Q.device)
    d2 = torch.full((n_q, k), -7.0, dtype=torch.float32, device=Q.device)
    work = torch.empty(lib.mde_knn_cross_work_bytes(n_q, n_c, k, slices), dtype=torch.uint8, device=Q.device)
    lib_mod.check(lib.mde_knn_cross(n_q, n_c, nf, lib_mod.ptr(Q), lib_mod.ptr(C), k, slices, lib_mod.ptr(idx),
                                    lib_mod.ptr(d2), lib_mod.ptr(work), lib_mod.stream_ptr(Q.device)))
    torch.cuda.synchronize()
    return idx.cpu().numpy(), d2.cpu().numpy()


def main():
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    from pymde_amd import _lib
    dev = torch.device("cuda", 0)
    out = {}
    for seed, (name, (n, nf, k)) in enumerate(KNN_CASES.items()):
        X = _data(seed, n, nf)
        out[name + "__X"] = X
        out[name + "__idx"], out[name + "__d2"] = run_knn(_lib, torch.tensor(X, device=dev), k)
    name, n_q, n_c, nf, k, slice_counts = CROSS_CASE
    Q, C = _data(10, n_q, nf), _data(11, n_c, nf)
    out[name + "__Q"], out[name + "__C"] = Q, C
    for s in slice_counts:
        out["%s__s%d__idx" % (name, s)], out["%s__s%d__d2" % (name, s)] = run_cross(
            _lib, torch.tensor(Q, device=dev), torch.tensor(C, device=dev), k, s)
    name, n, nf, k = L1_CASE
    X = out["knn_n130_nf33_k15__X"]                      # the Manhattan case shares the Euclidean case's input
    out[name + "__idx"], out[name + "__d"] = run_l1(_lib, torch.tensor(X, device=dev), k)
    np.savez_compressed(OUT, **out)
    size = os.path.getsize(OUT)
    assert size < MAX_BYTES, size
    print("wrote %s: %d arrays, %d bytes" % (OUT, len(out), size))


if __name__ == "__main__":
    main()

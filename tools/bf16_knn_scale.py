"""The bfloat16-shortlist k-NN search (mde_knn_bf16) against the float32 search at user sizes, k = 15.

    python tools/bf16_knn_scale.py --shape self:70000x784:uniform --mode f32 [--lib /path/to/libmde_hip.so]
    python tools/bf16_knn_scale.py --shape cross:10000x1000000x784:mixture --mode bf16 [--recall]

One process measures one shape in one mode and prints one JSON line: a warm-up call, then three calls timed
with a device synchronise on both sides (seconds, and their median), the CRC32 of the raw idx and d2 bytes and
the useful rate 2 n_q n_c nf / median.  profiles/r12_bf16_knn.txt runs fresh processes, alternating.

The calls go through ctypes straight to the C ABI (mde_knn / mde_knn_cross / mde_knn_bf16), so that --lib can
name an older build of libmde_hip.so -- one without mde_knn_bf16 -- as the float32 baseline.  What is timed is
the search alone: the column statistics both precisions need at the Python level are taken before.
  --mode f32   mde_knn (self) or mde_knn_cross (cross, automatic slices) on the rows as given
  --mode bf16  mde_knn_bf16 with the default shortlist (31 at k = 15), bf16 copies centred at the grid means
  --recall     (bf16) also runs the float32 search of the same library and reports the recall over all rows
               and whether every shared pair has the same d2 bits

Data: `uniform` (0, 1] as tools/metric_knn_scale.py, `mixture` the class mixture of tools/ann_knn_scale.py;
cross queries are corpus rows + N(0, 0.01 I)."""
import argparse
import ctypes
import json
import os
import sys
import time
import zlib

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

K = 15
c_i32, c_i64, c_vp = ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p


def make(kind, n, nf, dev):
    if kind == "uniform":
        g = torch.Generator(device=dev)
        g.manual_seed(n + nf)
        return (1.0 - torch.rand(n, nf, generator=g, device=dev)).contiguous()
    from ann_knn_scale import mixture
    return mixture(n, nf, seed=n + nf, dev=dev)


def ptr(t):
    return None if t is None else c_vp(t.data_ptr())


class Lib:
    def __init__(self, path):
        self.lib = ctypes.CDLL(path)
        self.lib.mde_knn.argtypes = [c_i64, c_i32, c_vp, c_i32, c_vp, c_vp, c_vp, c_vp]
        self.lib.mde_knn_cross_work_bytes.restype = c_i64
        self.lib.mde_knn_cross_work_bytes.argtypes = [c_i64, c_i64, c_i32, c_i32]
        self.lib.mde_knn_cross.argtypes = [c_i64, c_i64, c_i32, c_vp, c_vp, c_i32, c_i32, c_vp, c_vp, c_vp, c_vp]
        if hasattr(self.lib, "mde_knn_bf16"):
            self.lib.mde_knn_bf16_work_bytes.restype = c_i64
            self.lib.mde_knn_bf16_work_bytes.argtypes = [c_i64, c_i64, c_i32, c_i32, c_i32, c_i32]
            self.lib.mde_knn_bf16.argtypes = [c_i64, c_i64, c_i32, c_vp, c_vp, c_vp, c_i32, c_i32, c_i32, c_i32,
                                              c_vp, c_vp, c_vp, c_vp]

    def search(self, mode, Q, C, self_join, mu=None, n_cand=None):
        n_q, n_c, nf = Q.shape[0], C.shape[0], C.shape[1]
        dev = C.device
        idx = torch.empty((n_q, K), dtype=torch.int32, device=dev)
        d2 = torch.empty((n_q, K), dtype=torch.float32, device=dev)
        stream = c_vp(torch.cuda.current_stream(dev).cuda_stream)
        if mode == "bf16":
            nbytes = self.lib.mde_knn_bf16_work_bytes(n_q, n_c, nf, K, n_cand, 0)
            assert nbytes > 0, nbytes
            work = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            rc = self.lib.mde_knn_bf16(n_q, n_c, nf, ptr(Q), ptr(C), ptr(mu), int(self_join), K, n_cand, 0, ptr(idx),
                                       ptr(d2), ptr(work), stream)
        elif self_join:
            work = torch.empty(n_c, dtype=torch.float32, device=dev)
            rc = self.lib.mde_knn(n_c, nf, ptr(C), K, ptr(idx), ptr(d2), ptr(work), stream)
        else:
            nbytes = self.lib.mde_knn_cross_work_bytes(n_q, n_c, K, 0)
            assert nbytes > 0, nbytes
            work = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            rc = self.lib.mde_knn_cross(n_q, n_c, nf, ptr(Q), ptr(C), K, 0, ptr(idx), ptr(d2), ptr(work), stream)
        assert rc == 0, rc
        return idx, d2


def crc(t):
    return "%08x" % zlib.crc32(t.cpu().numpy().tobytes())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", required=True, help="self:NxF:kind or cross:QxNxF:kind")
    ap.add_argument("--mode", choices=("f32", "bf16"), required=True)
    ap.add_argument("--lib", default=os.path.join(ROOT, "pymde_amd", "libmde_hip.so"))
    ap.add_argument("--recall", action="store_true")
    ap.add_argument("--calls", type=int, default=3)
    args = ap.parse_args()
    what, dims, kind = args.shape.split(":")
    dims = [int(v) for v in dims.split("x")]
    dev = torch.device("cuda", 0)
    lib = Lib(args.lib)
    with torch.cuda.device(dev):
        if what == "self":
            n_q = n_c = dims[0]
            C = make(kind, dims[0], dims[1], dev)
            Q = C
        else:
            n_q, n_c = dims[0], dims[1]
            C = make(kind, n_c, dims[2], dev)
            g = torch.Generator(device=dev)
            g.manual_seed(n_q)
            pick = torch.randint(0, n_c, (n_q,), generator=g, device=dev)
            Q = (C[pick] + 0.1 * torch.randn(n_q, dims[2], generator=g, device=dev)).contiguous()
        nf = C.shape[1]
        mu, n_cand = None, None
        if args.mode == "bf16":
            from pymde_amd import preprocess
            mu = preprocess._bf16_mu(C)
            n_cand = preprocess.default_n_candidates(K, n_c - (what == "self"))
        lib.search(args.mode, Q, C, what == "self", mu, n_cand)            # warm-up
        times = []
        for _ in range(args.calls):
            torch.cuda.synchronize()
            t = time.perf_counter()
            idx, d2 = lib.search(args.mode, Q, C, what == "self", mu, n_cand)
            torch.cuda.synchronize()
            times.append(time.perf_counter() - t)
        med = sorted(times)[len(times) // 2]
        row = {"shape": args.shape, "mode": args.mode, "lib": os.path.basename(os.path.dirname(args.lib)) + "/" +
               os.path.basename(args.lib), "times": [round(t, 5) for t in times], "median": round(med, 5),
               "tflops": round(2.0 * n_q * n_c * nf / med / 1e12, 1), "crc_idx": crc(idx), "crc_d2": crc(d2)}
        if args.mode == "bf16":
            row["n_cand"] = n_cand
        if args.recall and args.mode == "bf16":
            ref_idx, ref_d2 = lib.search("f32", Q, C, what == "self")
            hits, same_bits = 0, True
            for r0 in range(0, n_q, 1 << 16):
                a, b = idx[r0:r0 + (1 << 16)], ref_idx[r0:r0 + (1 << 16)]
                hit = a[:, :, None] == b[:, None, :]
                hits += int(hit.any(2).sum())
                w = hit.nonzero()
                da = d2[r0:r0 + (1 << 16)].view(torch.int32)[w[:, 0], w[:, 1]]
                db = ref_d2[r0:r0 + (1 << 16)].view(torch.int32)[w[:, 0], w[:, 2]]
                same_bits = same_bits and bool(torch.equal(da, db))
            row["recall_all_rows"] = hits / float(n_q * K)
            row["rows_identical"] = int((idx == ref_idx).all(1).sum())
            row["shared_pairs_same_d2_bits"] = same_bits
            row["f32_crc_idx"], row["f32_crc_d2"] = crc(ref_idx), crc(ref_d2)
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()

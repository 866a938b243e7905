"""One line per plan describing the LDS-ring layout the library builds for it, from the Python entry points only:
ring_info(), ring_check(), hashes of the edge-id order (expand of 1..p in layout 1, padding included), of the codebook
words (d = 2, 3), of the byte-index stream of a 40-value array, and of loss and gradient of one fp32-stream function.
Run it with two builds of the library (PYMDE_AMD_LIB_VARIANT=<path> selects one) and compare the outputs: a change
that only moves code must leave every line as it was.

    python tools/ring_layout_digest.py [--only SUBSTRING] > digest.txt
"""
import argparse
import hashlib
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pymde_amd  # noqa: E402
from pymde_amd.average_distortion import Binding, EdgePlan, fused_evaluate  # noqa: E402

DEV = torch.device("cuda", 0)
KNOBS = ("MDE_PANEL", "MDE_RING_HUB", "MDE_RING_PERMUTE", "MDE_RING_ASSIGN", "MDE_RING_LOSS_BAND")


def sha(t):
    return hashlib.sha1(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()[:12]


def skewed_graph(rng, n, p, hubs):
    """tests/test_gpu_kernels.py::_skewed_graph: degrees fall along the vertex order, plus a few hub vertices."""
    i = np.minimum((n * rng.random(p) ** 3).astype(np.int64), n - 1)
    j = (i + 1 + rng.integers(0, n - 1, p)) % n
    for v, deg in hubs:
        sel = rng.choice(p, deg, replace=False)
        i[sel] = v
        j[sel] = (v + 1 + rng.choice(n - 1, deg, replace=False)) % n
    key = np.unique(np.minimum(i, j).astype(np.int64) * n + np.maximum(i, j))
    return np.stack([key // n, key % n], 1)


def dense_graph(rng):
    """the graph of test_ring_layout_peeled_and_dealt_rows_on_a_dense_graph (the by-column path of the builder)"""
    n, p = 3000, 2_000_000
    i = np.minimum((n * rng.random(p) ** 1.5).astype(np.int64), n - 1)
    j = (i + 1 + rng.integers(0, n - 1, p)) % n
    key = np.unique(np.minimum(i, j).astype(np.int64) * n + np.maximum(i, j))
    return n, np.stack([key // n, key % n], 1)


def uniform_graph(rng, n, p):
    i = rng.integers(0, n, p)
    j = (i + 1 + rng.integers(0, n - 1, p)) % n
    key = np.unique(np.minimum(i, j).astype(np.int64) * n + np.maximum(i, j))
    return np.stack([key // n, key % n], 1)


def digest(name, n, edges, d, env, row_lo=0, row_hi=None):
    for k in KNOBS:
        os.environ.pop(k, None)
    os.environ.update(env)
    rng = np.random.default_rng(1234)
    p = len(edges)
    et = torch.tensor(edges, device=DEV)
    X = torch.tensor((rng.standard_normal((n, d)) * 1.5).astype(np.float32), device=DEV)
    wc = np.where(rng.random(p) < 0.3, -rng.uniform(0.5, 1.5, p), rng.uniform(0.5, 2.0, p)).astype(np.float32)
    w40 = (1.0 + rng.integers(0, 40, p)).astype(np.float32)
    pen = pymde_amd.penalties
    plan = EdgePlan(n, et, row_lo, row_hi)
    b = Binding(plan, pen.PushAndPull(torch.tensor(wc, device=DEV), pen.Log1p, pen.Log))
    buf = torch.zeros(n * d + 1, device=DEV)
    fused_evaluate(b, X, buf[:n * d].view(n, d), buf[n * d:])
    torch.cuda.synchronize()
    info = plan.ring_info()
    parts = [name, "d=%d" % d, "layout=%d" % b.struct(d).layout, "stream=%s" % b.stream_kind,
             " ".join("%s=%s" % (k, info[k]) for k in sorted(info))]
    if info["built"]:
        chk = plan.ring_check()
        parts.append(" ".join("%s=%d" % (k, chk[k]) for k in sorted(chk)))
        H = info["padded_entries"]
        order = plan.expand(torch.arange(1, p + 1, dtype=torch.float32, device=DEV), layout=1)
        parts.append("eid=%s" % sha(order[:H]))
        if d in (2, 3):
            cb = plan.expand_codebook(torch.ones(p, device=DEV))
            parts.append("codebook=%s" % (sha(cb[:H + 8].view(torch.int32)) if cb is not None else "none"))
        by = plan.expand_bytes(torch.tensor(w40, device=DEV))
        parts.append("bytes=%s" % (sha(by[:H // 4 + 256].view(torch.int32)) if by is not None else "none"))
    parts.append("loss=%s grad=%s" % (sha(buf[n * d:]), sha(buf[:n * d])))
    print(" | ".join(parts), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="", help="run the cases whose name contains this")
    args = ap.parse_args()
    n = 40000
    skew = skewed_graph(np.random.default_rng(100), n, 500000, [(7, 20000), (n // 2, 3000), (n - 3, 900)])
    unif = uniform_graph(np.random.default_rng(101), n, 500000)
    nd, dense = dense_graph(np.random.default_rng(9))
    on = {"MDE_PANEL": "1"}
    cases = []
    for d in (1, 2, 3, 4):
        cases.append(("skewed default", n, skew, d, on))
        cases.append(("skewed peel", n, skew, d, dict(on, MDE_RING_HUB="300")))
        cases.append(("skewed deal", n, skew, d, dict(on, MDE_RING_PERMUTE="1")))
        cases.append(("skewed peel+deal", n, skew, d, dict(on, MDE_RING_HUB="300", MDE_RING_PERMUTE="1")))
    cases.append(("dense by-column", nd, dense, 2, dict(on, MDE_RING_HUB="1500", MDE_RING_PERMUTE="1")))
    cases.append(("uniform default", n, unif, 2, on))
    cases.append(("uniform greedy assign", n, unif, 2, dict(on, MDE_RING_ASSIGN="1")))
    cases.append(("uniform loss band 0", n, unif, 2, dict(on, MDE_RING_LOSS_BAND="0")))
    bounds = [0, n // 5, n // 2, n]
    for r in range(3):
        cases.append(("skewed shard %d of 3" % r, n, skew, 2, dict(on, MDE_RING_HUB="300"), bounds[r], bounds[r + 1]))
    # a degree-20000 vertex that stays in the ring: its stream overflows the single-pass region, count-then-fill
    cases.append(("hub kept in the ring", n, skew, 2, dict(on, MDE_RING_HUB="0", MDE_RING_PERMUTE="0")))
    for c in cases:
        if args.only in c[0]:
            digest(*c)


if __name__ == "__main__":
    main()

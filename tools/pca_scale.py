"""Sparse principal components (pymde_amd.pca, csrc/mde_spmm.hip) at user sizes.

    python tools/pca_scale.py [--shapes 100000x20000x0.05,400000x20000x0.02] [--baseline 100000x20000x0.05,...]
                              [--r 60] [--m 50] [--reps 5] [--overlap 70000x784] [--limit 600]
                              [--out profiles/r21_sparse_pca.txt]

Every step is a child process under its own time limit (--limit seconds); the first step that fails or runs past its
limit stops the run.  Sparse data: a random CSR drawn on the GPU (per row, density * nf column ids drawn with
replacement and de-duplicated; standard normal values), handed to the library as a torch sparse CSR tensor.

  spmm     per shape: one mde_csr_spmm call on the CSR and one on its transpose with B of --r columns, u and v given;
           the median (min - max) of --reps calls after a warm-up, each with a device synchronise on both sides, in ms
           and as 4 r nnz / time (the bytes of B gathered); and DeviceCSR.transpose() itself.
  pca      per shape: preprocess.principal_components(data, --m) end to end (conversion, validation, transpose, the
           2 n_iter + 3 products and the orthonormalisations), the same statistics.
  recipe   per shape: ONE call of preserve_neighbors(data, n_components=--m, seed=0), and for the --baseline shapes
           one call of preserve_neighbors(data, seed=0) on the same data beside it.
  overlap  quality.neighbor_overlap(data, scores, 15) of the lists in the reduced space against the lists in the full
           space, on the mixture of tools/mnist_like.py (drawn on the GPU as tools/dense_place_scale.py draws it: ten
           isotropic blobs, so neighbours inside a blob are decided by noise in all nf dimensions), and on the same
           mixture in 20 latent dimensions mapped into nf with a little isotropic noise, where the lists of the
           noise-free rows are known and both searches are scored against them.
No number is asserted anywhere."""
import argparse
import os
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from dense_place_scale import clock, mnist_like, summary  # noqa: E402


def random_csr(n, nf, density, dev, seed=0):
    from pymde_amd import sparse
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    per_row = max(int(round(density * nf)), 1)
    cols = torch.sort(torch.randint(0, nf, (n, per_row), generator=g, device=dev), dim=1).values
    keep = torch.ones_like(cols, dtype=torch.bool)
    keep[:, 1:] = cols[:, 1:] != cols[:, :-1]
    indptr = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    torch.cumsum(keep.sum(1), 0, out=indptr[1:])
    indices = cols[keep].to(torch.int32).contiguous()
    values = torch.randn(indices.shape[0], generator=g, device=dev)
    return sparse.DeviceCSR(indptr, indices, values, (n, nf))


def as_tensor(csr):
    return torch.sparse_csr_tensor(csr.indptr, csr.indices.to(torch.int64), csr.values, csr.shape)


def ms(times):
    times = sorted(1e3 * t for t in times)
    return "%.3f (%.3f - %.3f) ms" % (times[len(times) // 2], times[0], times[-1])


def step_spmm(n, nf, density, r, reps):
    from pymde_amd import sparse
    dev = torch.device("cuda", 0)
    csr = random_csr(n, nf, density, dev).validate()
    print("  %d x %d, %d stored entries (density %.4f), r = %d, segment %d; %d calls after a warm-up, median "
          "(min - max)" % (n, nf, csr.nnz, csr.density, r, sparse.spmm_segment(), reps))
    t_t = [clock(csr.transpose) for _ in range(max(reps // 2, 1) + 1)][1:]
    print("    DeviceCSR.transpose()            %s" % ms(t_t))
    for name, mat in (("CSR", csr), ("transpose", csr.transpose().validate())):
        B = torch.randn((mat.n_features, r), device=dev)
        u, v = torch.randn(mat.n, device=dev), torch.randn(r, device=dev, dtype=torch.float64)
        work = sparse.spmm_work(mat, r)
        run = lambda: sparse.spmm(mat, B, u, v, work)                                           # noqa: E731
        run()
        times = [clock(run) for _ in range(reps)]
        med = sorted(times)[len(times) // 2]
        lengths = (mat.indptr[1:] - mat.indptr[:-1])
        print("    mde_csr_spmm on the %-10s %s = %.2f TB/s of B rows gathered (4 r nnz / time); rows of %d .. %d "
              "entries" % (name, ms(times), 4.0 * r * mat.nnz / med / 1e12, int(lengths.min()), int(lengths.max())))


def step_pca(n, nf, density, m, reps):
    from pymde_amd import preprocess
    dev = torch.device("cuda", 0)
    data = as_tensor(random_csr(n, nf, density, dev))
    run = lambda: preprocess.principal_components(data, m)                                       # noqa: E731
    run()
    times = [clock(run) for _ in range(reps)]
    print("  principal_components(%d x %d at %.3f, %d) end to end, n_iter = 4, 10 oversamples: %s s"
          % (n, nf, density, m, summary(times)))


def step_recipe(n, nf, density, m):
    import pymde_amd
    dev = torch.device("cuda", 0)
    data = as_tensor(random_csr(n, nf, density, dev))
    kw = {"n_components": m} if m else {}
    t = clock(lambda: pymde_amd.preserve_neighbors(data, seed=0, **kw))
    print("  preserve_neighbors(%d x %d at %.3f, seed=0%s): %.3f s to build the problem (one call)"
          % (n, nf, density, ", n_components=%d" % m if m else "", t))


def step_overlap(n, nf, m):
    from pymde_amd import preprocess, quality
    dev = torch.device("cuda", 0)
    data = mnist_like(n, nf, dev)
    fit = preprocess.principal_components(data, m)
    ratio = float(fit.explained_variance.sum() / fit.total_variance)
    overlap = quality.neighbor_overlap(data, fit.scores, 15)
    print("  mixture of tools/mnist_like.py, %d x %d, %d components (dense route): explained variance ratio %.4f; "
          "quality.neighbor_overlap(data, scores, 15) = %.4f" % (n, nf, m, ratio, overlap))
    # the same mixture in 20 latent dimensions, mapped into nf by a random matrix, plus isotropic noise of 0.05
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    latent = mnist_like(n, 20, dev)
    clean = latent @ (torch.randn((20, nf), generator=g, device=dev) / 20.0 ** 0.5)
    data = clean + 0.05 * torch.randn((n, nf), generator=g, device=dev)
    fit = preprocess.principal_components(data, m)
    ratio = float(fit.explained_variance.sum() / fit.total_variance)
    print("  that mixture in 20 latent dimensions mapped into %d by a random matrix, plus N(0, 0.05^2) noise, %d "
          "components: explained variance ratio %.4f; neighbor_overlap(data, scores, 15) = %.4f; against the lists of "
          "the noise-free rows: full space %.4f, reduced space %.4f"
          % (nf, m, ratio, quality.neighbor_overlap(data, fit.scores, 15), quality.neighbor_overlap(clean, data, 15),
             quality.neighbor_overlap(clean, fit.scores, 15)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="100000x20000x0.05,400000x20000x0.02")
    ap.add_argument("--baseline", default="100000x20000x0.05,400000x20000x0.02")
    ap.add_argument("--r", type=int, default=60)
    ap.add_argument("--m", type=int, default=50)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--overlap", default="70000x784")
    ap.add_argument("--limit", type=int, default=600, help="seconds per step")
    ap.add_argument("--out", default=None)
    ap.add_argument("--step", default=None, help=argparse.SUPPRESS)      # kind:n:nf:density
    a = ap.parse_args()
    if a.step:
        kind, n, nf, density = (a.step.split(":") + ["0"])[:4]
        n, nf, density = int(n), int(nf), float(density)
        with torch.cuda.device(0):
            if kind == "spmm":
                step_spmm(n, nf, density, a.r, a.reps)
            elif kind == "pca":
                step_pca(n, nf, density, a.m, a.reps)
            elif kind == "recipe":
                step_recipe(n, nf, density, a.m)
            elif kind == "baseline":
                step_recipe(n, nf, density, 0)
            else:
                step_overlap(n, nf, a.m)
        return 0
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
        if a.out:                                   # (kept current: a run that is cut short leaves what it measured)
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    def triples(text):
        return [tuple(item.split("x")) for item in text.split(",") if item]

    shapes, baseline = triples(a.shapes), triples(a.baseline)
    steps = ["%s:%s:%s:%s" % ((kind,) + s) for kind in ("spmm", "pca") for s in shapes]
    steps += ["overlap:%s:%s" % s for s in triples(a.overlap)]
    for s in shapes:
        steps.append("recipe:%s:%s:%s" % s)
        if s in baseline:
            steps.append("baseline:%s:%s:%s" % s)
    say("tools/pca_scale.py; every step a process of its own under a limit of %d s" % a.limit)
    for step in steps:
        say("")
        say("## %s" % step)
        cmd = [sys.executable, os.path.abspath(__file__), "--step", step, "--r", str(a.r), "--m", str(a.m),
               "--reps", str(a.reps)]
        try:
            p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=a.limit)
        except subprocess.TimeoutExpired:
            say("step %s ran past its limit of %d s: stopping" % (step, a.limit))
            return 1
        for line in p.stdout.decode(errors="replace").splitlines():
            say(line)
        if p.returncode != 0:                       # (warnings on stderr are not part of the record; a failure's are)
            for line in p.stderr.decode(errors="replace").splitlines():
                say(line)
            say("step %s exited with status %d: stopping" % (step, p.returncode))
            return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())

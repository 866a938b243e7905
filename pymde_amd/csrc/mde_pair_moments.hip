// mde_pair_moments.hip -- sums over ALL pairs of the distances in two spaces: what Kruskal's
// stress, the correlation of the pairwise distances and the Shepard histogram of pymde_amd.quality are computed
// from, in O(n) memory.
//
// A [n, nfa] (the prepared data rows) and B [n, nfb] (the embedding) have the same rows.  For every query row
// i = q_rows[r] and every corpus row j != i (by index: a duplicate of row i elsewhere counts)
//   D = dist_A(i, j),  E = dist_B(i, j),  dist = sqrtf(d2) (mode 0) or 0.5f d2 (mode 1: the cosine / correlation
//   distance of unit rows, the units the searches return),  d2 = fmaxf(|x|^2 + |y|^2 - 2 x.y, 0)
// with d2 the Gram tile's own expression (mde_knn_tile.h), bit for bit the squared distance of the k-NN kernels.
//
//   k_pair_walk<HIST>     the grid of k_knn_rank: workgroup (x, y) owns 64 queries and the corpus columns of slice y.
//                         Per 64-column tile it runs the Gram tile twice (A, then B) and parks both tiles of squared
//                         distances (sD and a second [64][65] block); thread t owns tile row t & 63 and the 16 columns
//                         16 (t >> 6) ... of both parked tiles.
//       HIST = false      five double accumulators (sum D, E, D^2, E^2, D E; products formed in double from the
//                         float32 D and E) and two float maxima per thread; the four threads of a row are combined in
//                         thread order at the end.  Fixed order, no floating-point atomics: for a given slice count
//                         the sums are the same bits on every run, and a row's sums do not depend on which queries
//                         share its block.
//       HIST = true       every counted pair increments a bins x bins uint32 block in LDS (LDS integer atomics), which
//                         is flushed once with 64-bit integer global atomics: integers, so any slice count gives the
//                         same counts.
//   k_pair_fold           adds the per-slice row sums in slice order (maxima: the largest)
//   k_pair_totals         one workgroup reduces the rows to totals[8] in a fixed order
#include "mde_pair.h"

#define PAIR_MAX_BINS 64
// A workgroup's uint32 bin counts 64 pairs per corpus column: a slice holds at most this many column tiles
#define PAIR_HIST_MAX_TILES ((int64_t)1 << 19)

template <bool HIST>
__global__ __launch_bounds__(MDE_BLOCK) void k_pair_walk(int n, int n_q, int nfa, int nfb, int mode_a, int mode_b,
                                                         int64_t slice_cols, const float* __restrict__ A,
                                                         const float* __restrict__ B, const float* __restrict__ an,
                                                         const float* __restrict__ bn,
                                                         const int32_t* __restrict__ q_rows,
                                                         double* __restrict__ sums_out, float* __restrict__ max_out,
                                                         int bins, float a_lo, float a_hi, float a_scale, float b_lo,
                                                         float b_hi, float b_scale,
                                                         unsigned long long* __restrict__ counts) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const knn_tile_lds s = knn_tile_carve(lds, 0, PAIR_TILE);
  float* sE = s.extra;                                          // [KNN_BM][KNN_BN + 1]
  unsigned int* hist = reinterpret_cast<unsigned int*>(s.bestd);  // [bins][bins], HIST only
  __shared__ int sQ[KNN_BM];                                    // the corpus index of every query of the block, -1: none
  const int tid = threadIdx.x, r = tid & 63, w = tid >> 6;
  const int64_t row0 = (int64_t)blockIdx.x * KNN_BM;
  const int64_t lo = (int64_t)blockIdx.y * slice_cols;
  const int64_t c_lo = lo < n ? lo : n, c_hi = lo + slice_cols < n ? lo + slice_cols : n;
  if (tid < KNN_BM) {
    const int64_t gr = row0 + tid;
    sQ[tid] = gr < n_q ? (q_rows ? q_rows[gr] : (int)gr) : -1;
  }
  if (HIST)
    for (int i = tid; i < bins * bins; i += MDE_BLOCK) hist[i] = 0u;
  const float* arow[KNN_STG];
  const float* brow[KNN_STG];
  bool qok[KNN_STG];
#pragma unroll
  for (int q = 0; q < KNN_STG; ++q) {
    const int64_t gr = row0 + (tid >> 5) + 8 * q;
    qok[q] = gr < n_q;
    const int64_t qi = qok[q] ? (q_rows ? (int64_t)q_rows[gr] : gr) : 0;
    arow[q] = A + qi * nfa;
    brow[q] = B + qi * nfb;
  }
  __syncthreads();                                              // sQ, hist
  double sd = 0.0, se = 0.0, sdd = 0.0, see = 0.0, sde = 0.0;
  float md = 0.0f, me = 0.0f;
  for (int64_t col0 = c_lo; col0 < c_hi; col0 += KNN_BN) {
    const float* acol[KNN_STG];
    const float* bcol[KNN_STG];
    bool cok[KNN_STG];
#pragma unroll
    for (int q = 0; q < KNN_STG; ++q) {
      const int64_t gc = col0 + (tid >> 5) + 8 * q;
      cok[q] = gc < n;
      const int64_t cj = cok[q] ? gc : n - 1;
      acol[q] = A + cj * nfa;
      bcol[q] = B + cj * nfb;
    }
    auto keep = [&](int rr, int cc) { return sQ[rr] >= 0 && col0 + cc < n && (int64_t)sQ[rr] != col0 + cc; };
    // the parks follow the barriers of their knn_gram_tile: every thread is past the walk of the last tile by then
    {
      const f32x16 acc = knn_gram_tile(s.sA, s.sB, nfa, arow, qok, acol, cok);
      knn_park_tile(s.sD, acc, keep, [&](int rr) { return an[sQ[rr]]; }, [&](int cc) { return an[col0 + cc]; });
    }
    {
      const f32x16 acc = knn_gram_tile(s.sA, s.sB, nfb, brow, qok, bcol, cok);
      knn_park_tile(sE, acc, keep, [&](int rr) { return bn[sQ[rr]]; }, [&](int cc) { return bn[col0 + cc]; });
    }
    __syncthreads();
    // the 64 lanes of a wave read 64 rows at stride 65: conflict-free
    const float* pd = s.sD + r * (KNN_BN + 1) + w * PAIR_COLS;
    const float* pe = sE + r * (KNN_BN + 1) + w * PAIR_COLS;
#pragma unroll 4
    for (int cc = 0; cc < PAIR_COLS; ++cc) {
      const float d2a = pd[cc], d2b = pe[cc];
      const bool have = d2a != PAIR_FLT_MAX;                    // what keep() refused is parked as FLT_MAX
      const float D = have ? pair_dist(d2a, mode_a) : 0.0f;
      const float E = have ? pair_dist(d2b, mode_b) : 0.0f;
      if (HIST) {
        if (have && D >= a_lo && D <= a_hi && E >= b_lo && E <= b_hi) {
          int bd = (int)((D - a_lo) * a_scale), be = (int)((E - b_lo) * b_scale);
          bd = bd < bins - 1 ? bd : bins - 1;
          be = be < bins - 1 ? be : bins - 1;
          atomicAdd(&hist[bd * bins + be], 1u);
        }
      } else {
        const double Dd = (double)D, Ed = (double)E;            // a pair that does not count adds 0.0: no change
        sd += Dd;
        se += Ed;
        sdd = fma(Dd, Dd, sdd);
        see = fma(Ed, Ed, see);
        sde = fma(Dd, Ed, sde);
        md = fmaxf(md, D);
        me = fmaxf(me, E);
      }
    }
  }
  __syncthreads();                                              // the last walk is over: sD is free, hist is complete
  if (HIST) {
    for (int i = tid; i < bins * bins; i += MDE_BLOCK) {
      const unsigned int v = hist[i];
      if (v) atomicAdd(counts + i, (unsigned long long)v);
    }
  } else {
    double* cs = reinterpret_cast<double*>(s.sD);               // [4][KNN_BM][5]; sD starts at a multiple of 8 bytes
    float* cm = sE;                                             // [4][KNN_BM][2]
    double* mine = cs + ((size_t)w * KNN_BM + r) * 5;
    mine[0] = sd;
    mine[1] = se;
    mine[2] = sdd;
    mine[3] = see;
    mine[4] = sde;
    cm[(w * KNN_BM + r) * 2 + 0] = md;
    cm[(w * KNN_BM + r) * 2 + 1] = me;
    __syncthreads();
    // thread (row, v) adds value v of the row's four threads in thread order
    for (int i = tid; i < KNN_BM * 5; i += MDE_BLOCK) {
      const int rr = i / 5, v = i - 5 * rr;
      if (row0 + rr < n_q) {
        double t = cs[((size_t)0 * KNN_BM + rr) * 5 + v];
#pragma unroll
        for (int u = 1; u < 4; ++u) t += cs[((size_t)u * KNN_BM + rr) * 5 + v];
        sums_out[((int64_t)blockIdx.y * n_q + row0 + rr) * 5 + v] = t;
      }
    }
    if (tid < KNN_BM * 2) {
      const int rr = tid >> 1, v = tid & 1;
      if (row0 + rr < n_q) {
        float t = cm[(0 * KNN_BM + rr) * 2 + v];
#pragma unroll
        for (int u = 1; u < 4; ++u) t = fmaxf(t, cm[(u * KNN_BM + rr) * 2 + v]);
        max_out[((int64_t)blockIdx.y * n_q + row0 + rr) * 2 + v] = t;
      }
    }
  }
}

// row_sums[i] = the sum over the slices, in slice order, of part_sums[y][i]; row_max the largest of part_max[y][i].
__global__ __launch_bounds__(MDE_BLOCK) void k_pair_fold(int64_t n_q, int slices, const double* __restrict__ part_sums,
                                                         const float* __restrict__ part_max,
                                                         double* __restrict__ row_sums, float* __restrict__ row_max) {
  const int64_t total = n_q * 7;                                // 5 sums and 2 maxima per row
  for (int64_t i = (int64_t)blockIdx.x * MDE_BLOCK + threadIdx.x; i < total; i += (int64_t)gridDim.x * MDE_BLOCK) {
    if (i < n_q * 5) {
      double t = 0.0;
      for (int y = 0; y < slices; ++y) t += part_sums[(int64_t)y * n_q * 5 + i];
      row_sums[i] = t;
    } else {
      const int64_t k = i - n_q * 5;
      float t = 0.0f;
      for (int y = 0; y < slices; ++y) t = fmaxf(t, part_max[(int64_t)y * n_q * 2 + k]);
      row_max[k] = t;
    }
  }
}

// One workgroup: thread t adds the rows t, t + 256, ... in row order, thread v < 7 then adds (takes the largest
// of) the 256 threads' value v in thread order.  totals = sum D, E, D^2, E^2, D E, max D, max E, the pair count.
__global__ __launch_bounds__(MDE_BLOCK) void k_pair_totals(int64_t n_q, double pairs,
                                                           const double* __restrict__ row_sums,
                                                           const float* __restrict__ row_max,
                                                           double* __restrict__ totals) {
  __shared__ double part[MDE_BLOCK][7];
  double t[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int64_t i = threadIdx.x; i < n_q; i += MDE_BLOCK) {
#pragma unroll
    for (int v = 0; v < 5; ++v) t[v] += row_sums[i * 5 + v];
#pragma unroll
    for (int v = 0; v < 2; ++v) {
      const double m = (double)row_max[i * 2 + v];
      t[5 + v] = m > t[5 + v] ? m : t[5 + v];
    }
  }
#pragma unroll
  for (int v = 0; v < 7; ++v) part[threadIdx.x][v] = t[v];
  __syncthreads();
  if (threadIdx.x < 7) {
    const int v = threadIdx.x;
    double a = part[0][v];
    for (int u = 1; u < MDE_BLOCK; ++u) a = v < 5 ? a + part[u][v] : (part[u][v] > a ? part[u][v] : a);
    totals[v] = a;
  }
  if (threadIdx.x == 7) totals[7] = pairs;
}

// work: [s, n_q, 5] doubles (s > 1) | the row norms of A and B, [n] floats each | [s, n_q, 2] floats (s > 1)
extern "C" int64_t mde_pair_moments_work_bytes(int64_t n, int64_t n_q, int32_t slices) {
  if (!pair_args_ok(n, n_q, slices)) {
    mde_set_error("mde_pair_moments_work_bytes: invalid arguments (2 <= n < 2^31, 1 <= n_q < 2^31, 0 <= slices <= %d)",
                  CROSS_MAX_SLICES);
    return MDE_E_INVALID;
  }
  const int64_t s = cross_resolve_slices(n_q, n, slices);
  if (s < 0) return s;
  int64_t bytes = 4 * 2 * n;
  if (s > 1) bytes += s * n_q * (5 * 8 + 2 * 4);
  return bytes;
}

struct pair_hist_args {
  int32_t bins;
  float a_lo, a_hi, b_lo, b_hi;
  int64_t* counts;
};

static int pair_run(const char* who, int64_t n, int32_t nfa, const float* A, int32_t mode_a, int32_t nfb,
                    const float* B, int32_t mode_b, int64_t n_q, const int32_t* q_rows, int32_t slices,
                    double* row_sums, float* row_max, double* totals, const pair_hist_args* h, void* work,
                    void* stream) {
  const bool hist_ok = !h || (h->bins >= 1 && h->bins <= PAIR_MAX_BINS && h->a_hi > h->a_lo && h->b_hi > h->b_lo &&
                              h->counts);
  if (!pair_args_ok(n, n_q, slices) || nfa <= 0 || nfb <= 0 || (mode_a != 0 && mode_a != 1) ||
      (mode_b != 0 && mode_b != 1) || !A || !B || !work || (!q_rows && n_q != n) || !hist_ok ||
      (!h && (!row_sums || !row_max || !totals))) {
    mde_set_error("%s: invalid arguments (2 <= n < 2^31, 1 <= n_q < 2^31 and n_q == n without q_rows, nfa, nfb >= 1, "
                  "modes 0 / 1, 0 <= slices <= %d, non-null A / B / outputs / work%s)", who, CROSS_MAX_SLICES,
                  h ? "; 1 <= bins <= 64, a_hi > a_lo, b_hi > b_lo" : "");
    return MDE_E_INVALID;
  }
  int64_t s = cross_resolve_slices(n_q, n, slices);
  if (s < 0) return (int)s;
  const int64_t tiles = (n + KNN_BN - 1) / KNN_BN;
  if (h && (tiles + s - 1) / s > PAIR_HIST_MAX_TILES) s = (tiles + PAIR_HIST_MAX_TILES - 1) / PAIR_HIST_MAX_TILES;
  hipStream_t st = mde_stream(stream);
  double* part_sums = static_cast<double*>(work);
  float* an = reinterpret_cast<float*>(part_sums + (!h && s > 1 ? s * n_q * 5 : 0));
  float* bn = an + n;
  float* part_max = bn + n;
  int rc = mde_row_sqnorm(n, nfa, A, an, stream);
  if (rc == MDE_OK) rc = mde_row_sqnorm(n, nfb, B, bn, stream);
  if (rc != MDE_OK) return rc;
  const int64_t slice_cols = ((tiles + s - 1) / s) * KNN_BN;     // whole tiles; the last slices may be short or empty
  const dim3 grid((unsigned)((n_q + KNN_BM - 1) / KNN_BM), (unsigned)s);
  if (h) {
    const size_t lds = knn_tile_lds_bytes(0, PAIR_TILE + h->bins * h->bins);
    rc = knn_raise_lds_limit<k_pair_walk<true>>((int)knn_tile_lds_bytes(0, PAIR_TILE + PAIR_MAX_BINS * PAIR_MAX_BINS));
    if (rc != MDE_OK) return rc;
    hipLaunchKernelGGL(k_pair_walk<true>, grid, dim3(MDE_BLOCK), lds, st, (int)n, (int)n_q, nfa, nfb, mode_a, mode_b,
                       slice_cols, A, B, an, bn, q_rows, (double*)nullptr, (float*)nullptr, h->bins, h->a_lo, h->a_hi,
                       (float)h->bins / (h->a_hi - h->a_lo), h->b_lo, h->b_hi, (float)h->bins / (h->b_hi - h->b_lo),
                       reinterpret_cast<unsigned long long*>(h->counts));
    MDE_LAUNCH_CHECK();
    return MDE_OK;
  }
  hipLaunchKernelGGL(k_pair_walk<false>, grid, dim3(MDE_BLOCK), knn_tile_lds_bytes(0, PAIR_TILE), st, (int)n, (int)n_q,
                     nfa, nfb, mode_a, mode_b, slice_cols, A, B, an, bn, q_rows, s > 1 ? part_sums : row_sums,
                     s > 1 ? part_max : row_max, 0, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, (unsigned long long*)nullptr);
  MDE_LAUNCH_CHECK();
  if (s > 1) {
    hipLaunchKernelGGL(k_pair_fold, dim3(mde_grid(n_q * 7, MDE_BLOCK, 4096)), dim3(MDE_BLOCK), 0, st, n_q, (int)s,
                       part_sums, part_max, row_sums, row_max);
    MDE_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(k_pair_totals, dim3(1), dim3(MDE_BLOCK), 0, st, n_q, (double)n_q * (double)(n - 1), row_sums,
                     row_max, totals);
  MDE_LAUNCH_CHECK();
  return MDE_OK;
}

extern "C" int mde_pair_moments(int64_t n, int32_t nfa, const float* A, int32_t mode_a, int32_t nfb, const float* B,
                                int32_t mode_b, int64_t n_q, const int32_t* q_rows, int32_t slices, double* row_sums,
                                float* row_max, double* totals, void* work, void* stream) {
  return pair_run("mde_pair_moments", n, nfa, A, mode_a, nfb, B, mode_b, n_q, q_rows, slices, row_sums, row_max,
                  totals, nullptr, work, stream);
}

extern "C" int mde_pair_histogram(int64_t n, int32_t nfa, const float* A, int32_t mode_a, int32_t nfb, const float* B,
                                  int32_t mode_b, int64_t n_q, const int32_t* q_rows, int32_t slices, int32_t bins,
                                  float a_lo, float a_hi, float b_lo, float b_hi, int64_t* counts, void* work,
                                  void* stream) {
  const pair_hist_args h = {bins, a_lo, a_hi, b_lo, b_hi, counts};
  return pair_run("mde_pair_histogram", n, nfa, A, mode_a, nfb, B, mode_b, n_q, q_rows, slices, nullptr, nullptr,
                  nullptr, &h, work, stream);
}

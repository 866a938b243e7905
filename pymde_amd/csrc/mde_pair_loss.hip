// mde_pair_loss.hip -- the loss and the gradient of a DENSE MDE problem: a loss of pymde_amd.losses
// over ALL n (n - 1) / 2 pairs without an edge list, what pymde_amd.DenseMDE minimises, in O(n) memory beside D.
//
// For every row i and every row j != i (by index: a duplicate of row i elsewhere counts)
//   E = |x_i - x_j| from the differences (never |x|^2 + |y|^2 - 2 x.y: the gradient multiplies f'(E) / E by x_i - x_j,
//       and the expansion cancels for close points, exactly where f'(E) / E is large),
//   D = d_scale * the original deviation of the pair, from one of two sources:
//       Gram     the 64x64 Gram tile of the prepared data rows A [n, nf] (mde_knn_tile.h), parked as squared distances,
//                through pair_dist(d2, mode): bit for bit the D of mde_pair_moments;
//       matrix   a 64x64 tile of a row-major float32 [n, n] matrix, parked in the same LDS block (a wave reads whole
//                256-byte row segments; 64-bit offsets);
//   (l, gd) = mde_eval_rt(kind, E^2, a0 = D, a1 = 1 / D^2, scalars), gd = l'(E) / E under the reference's
//       NaN / Inf -> 1 rule (mde_fix_g),
//   row_loss[i] = sum_j l,  G[i, :] = sum_j gd (x_i - x_j),  loss = sum_i row_loss[i] / (2 P),  grad = G / P,
//   P = n (n - 1) / 2: MDE(n, d, all_edges(n), loss(deviations)).average_distortion and its gradient.
//
//   k_pair_loss_walk   the grid of k_pair_walk: workgroup (x, y) owns 64 rows and the column tiles of slice y.  Per
//                      tile the D side is parked in sD and the 64 column rows of X are staged as [64][DC] floats
//                      (DC = d padded with zeros to 1, 2, 3 or 8); thread t owns tile row t & 63, kept in registers,
//                      and the 16 columns 16 (t >> 6) ...: the lanes of a wave read the same staged column (a
//                      broadcast) and 64 rows of sD at stride 65 (conflict-free).  1 + DC double accumulators per
//                      thread, every product formed in double from its float32 terms; the four threads of a row are
//                      combined in thread order.  No floating-point atomics.
//   k_pair_loss_fold   adds the per-slice partials in slice order: row_loss, and grad = G / P rounded once
//   k_pair_loss_total  one workgroup reduces row_loss to the loss in a fixed order
// For a given slice count the loss, the gradient and row_loss are the same bits on every run.
//
// mde_pair_loss_cross is the RECTANGULAR form, what pymde_amd.DensePlacement minimises: the rows
// are n_q free query rows (Q, XQ), the columns n_c fixed corpus rows (C, XC), D comes from the Gram tile of Q against
// C or from an [n_q, n_c] matrix, and nothing is "self".  The same kernels: k_pair_loss_walk takes the rows and the
// columns from two sets of pointers and drops the row != col test at compile time (SELF = false); the fold divides
// by P = n_q n_c and the total by 1 P instead of 2 P, since every pair is in one row.  No gradient for XC.
//
// mde_pair_loss_cross_rows is the rectangular walk over a LIST of query rows, what the per-row
// placement solver (mde_rows.hip) evaluates once its first rows have finished: workgroup x owns the list entries
// 64 x ..., reads Q, the row norms, XQ and the Dm row through the list (ROWS = true, a compile-time variant of
// k_pair_loss_walk), and k_pair_loss_fold_rows writes row_loss and row_grad = G / n_c at the rows' own indices.
#include <math.h>

#include "mde_pair.h"
#include "mde_functions.h"

#define PAIR_LOSS_MAX_D 8
#define PAIR_LOSS_XS (KNN_BN * PAIR_LOSS_MAX_D)   // floats of the staged column rows of X: 2 KB

// ROWS (mde_pair_loss_cross_rows): the workgroup's 64 rows are the list entries 64 x ... of `rows` (NULL: the rows
// themselves), n_q is the length of the list, and the partials are indexed by list position.  Without ROWS `rows`
// is not read and the code is what it was.
template <int DC, bool MATRIX, bool SELF, bool ROWS = false>
__global__ __launch_bounds__(MDE_BLOCK) void k_pair_loss_walk(int n_q, int n_c, int nf, int d, int mode,
                                                              int64_t slice_cols, const float* __restrict__ Q,
                                                              const float* __restrict__ qn,
                                                              const float* __restrict__ C,
                                                              const float* __restrict__ cn,
                                                              const float* __restrict__ Dm,
                                                              const float* __restrict__ XQ,
                                                              const float* __restrict__ XC, int kind, int weighted,
                                                              MdeScalars S, float d_scale,
                                                              double* __restrict__ part,
                                                              const int32_t* __restrict__ rows) {
  static_assert(!(SELF && ROWS), "the row list belongs to the rectangular walk");
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const knn_tile_lds s = knn_tile_carve(lds, 0, PAIR_TILE + PAIR_LOSS_XS + (ROWS ? KNN_BM : 0));
  float* sX = s.extra + PAIR_TILE;                              // [KNN_BN][DC]
  const int tid = threadIdx.x, r = tid & 63, w = tid >> 6;
  const int64_t row0 = (int64_t)blockIdx.x * KNN_BM;
  int* sRow = reinterpret_cast<int*>(sX + PAIR_LOSS_XS);        // [KNN_BM] the rows of the list entries (ROWS)
  if constexpr (ROWS) {
    if (tid < KNN_BM) sRow[tid] = row0 + tid < n_q ? (rows ? rows[row0 + tid] : (int)(row0 + tid)) : 0;
    __syncthreads();
  }
  // the row behind tile row rr: any readable row where the list has ended
  auto row_of = [&](int rr) -> int64_t { return ROWS ? (int64_t)sRow[rr] : row0 + rr; };
  const int64_t lo = (int64_t)blockIdx.y * slice_cols;
  const int64_t c_lo = lo < n_c ? lo : n_c, c_hi = lo + slice_cols < n_c ? lo + slice_cols : n_c;
  float xi[DC];                                                 // the thread's own row
#pragma unroll
  for (int k = 0; k < DC; ++k) xi[k] = (row0 + r < n_q && k < d) ? XQ[row_of(r) * d + k] : 0.0f;
  const float* arow[KNN_STG];
  bool qok[KNN_STG];
  if constexpr (!MATRIX) {
#pragma unroll
    for (int q = 0; q < KNN_STG; ++q) {
      const int64_t gr = row0 + (tid >> 5) + 8 * q;
      qok[q] = gr < n_q;
      arow[q] = Q + (qok[q] ? (ROWS ? row_of((tid >> 5) + 8 * q) : gr) : 0) * nf;
    }
  }
  double sl = 0.0, sg[DC];
#pragma unroll
  for (int k = 0; k < DC; ++k) sg[k] = 0.0;
  for (int64_t col0 = c_lo; col0 < c_hi; col0 += KNN_BN) {
    auto keep = [&](int rr, int cc) {
      return row0 + rr < n_q && col0 + cc < n_c && (!SELF || row0 + rr != col0 + cc);
    };
    if constexpr (MATRIX) {
      // wave w takes the tile rows w, w + 4, ...: all sixteen loads go out from clamped addresses before the first is
      // used, and what the tile does not have (or the diagonal of the square walk) is replaced when the registers are
      // parked
      const int lane = tid & 63;
      const int64_t gc = col0 + lane < n_c ? col0 + lane : n_c - 1;
      float v[KNN_BM / 4];
#pragma unroll
      for (int q = 0; q < KNN_BM / 4; ++q) {
        const int64_t gr = ROWS ? row_of(w + 4 * q) : (row0 + w + 4 * q < n_q ? row0 + w + 4 * q : n_q - 1);
        v[q] = Dm[gr * (int64_t)n_c + gc];
      }
      __syncthreads();                                          // the walk of the last tile is over
#pragma unroll
      for (int q = 0; q < KNN_BM / 4; ++q)
        s.sD[(w + 4 * q) * (KNN_BN + 1) + lane] = keep(w + 4 * q, lane) ? v[q] : PAIR_FLT_MAX;
    } else {
      const float* acol[KNN_STG];
      bool cok[KNN_STG];
#pragma unroll
      for (int q = 0; q < KNN_STG; ++q) {
        const int64_t gc = col0 + (tid >> 5) + 8 * q;
        cok[q] = gc < n_c;
        acol[q] = C + (cok[q] ? gc : n_c - 1) * nf;
      }
      // the park follows the barriers of knn_gram_tile: every thread is past the walk of the last tile by then
      const f32x16 acc = knn_gram_tile(s.sA, s.sB, nf, arow, qok, acol, cok);
      knn_park_tile(s.sD, acc, keep, [&](int rr) { return qn[row_of(rr)]; }, [&](int cc) { return cn[col0 + cc]; });
    }
    for (int i = tid; i < KNN_BN * DC; i += MDE_BLOCK) {
      const int c = i / DC, k = i - c * DC;
      sX[i] = (col0 + c < n_c && k < d) ? XC[(col0 + c) * d + k] : 0.0f;
    }
    __syncthreads();
    const float* pd = s.sD + r * (KNN_BN + 1) + w * PAIR_COLS;
    const float* px = sX + w * PAIR_COLS * DC;
#pragma unroll 4
    for (int cc = 0; cc < PAIR_COLS; ++cc) {
      const float v = pd[cc];
      if (v != PAIR_FLT_MAX) {                                  // what keep() refused is parked as FLT_MAX
        const float D = (MATRIX ? v : pair_dist(v, mode)) * d_scale;
        float diff[DC], ss = 0.0f;
#pragma unroll
        for (int k = 0; k < DC; ++k) {
          diff[k] = xi[k] - px[cc * DC + k];
          ss = fmaf(diff[k], diff[k], ss);
        }
        const float a1 = weighted ? 1.0f / (D * D) : 0.0f;      // the losses' default weights
        float f, gd;
        mde_eval_rt(kind, ss, D, a1, S, f, gd);
        gd = mde_fix_g(gd);
        sl += (double)f;
#pragma unroll
        for (int k = 0; k < DC; ++k) sg[k] = fma((double)gd, (double)diff[k], sg[k]);
      }
    }
  }
  __syncthreads();                                              // the last walk is over: sD and the tile after it are free
  constexpr int NV = 1 + DC;
  double* cs = reinterpret_cast<double*>(s.sD);                 // [4][KNN_BM][NV]; sD starts at a multiple of 8 bytes
  double* mine = cs + ((size_t)w * KNN_BM + r) * NV;
  mine[0] = sl;
#pragma unroll
  for (int k = 0; k < DC; ++k) mine[1 + k] = sg[k];
  __syncthreads();
  // thread (row, v) adds value v of the row's four threads in thread order
  for (int i = tid; i < KNN_BM * NV; i += MDE_BLOCK) {
    const int rr = i / NV, v = i - NV * rr;
    if (row0 + rr < n_q && v <= d) {
      double t = cs[((size_t)0 * KNN_BM + rr) * NV + v];
#pragma unroll
      for (int u = 1; u < 4; ++u) t += cs[((size_t)u * KNN_BM + rr) * NV + v];
      part[((int64_t)blockIdx.y * n_q + row0 + rr) * (1 + d) + v] = t;
    }
  }
}
static_assert(4 * KNN_BM * (1 + PAIR_LOSS_MAX_D) * sizeof(double) <= 2 * PAIR_TILE * sizeof(float),
              "the row partials must fit in the parked tile and the tile after it");

// row_loss[i] and grad[i, :] = G[i, :] / pairs from the per-slice partials [slices, n, 1 + d], added in slice order
// (n rows: the rows of the square problem, the query rows of the rectangular one).
__global__ __launch_bounds__(MDE_BLOCK) void k_pair_loss_fold(int64_t n, int d, int slices, double pairs,
                                                              const double* __restrict__ part,
                                                              double* __restrict__ row_loss,
                                                              float* __restrict__ grad) {
  const int64_t total = n * (1 + d);
  for (int64_t i = (int64_t)blockIdx.x * MDE_BLOCK + threadIdx.x; i < total; i += (int64_t)gridDim.x * MDE_BLOCK) {
    double t = 0.0;
    for (int y = 0; y < slices; ++y) t += part[(int64_t)y * total + i];
    const int64_t row = i / (1 + d);
    const int v = (int)(i - row * (1 + d));
    if (v == 0)
      row_loss[row] = t;
    else
      grad[row * d + v - 1] = (float)(t / pairs);
  }
}

// The fold of mde_pair_loss_cross_rows: the partials [slices, n_rows, 1 + d] are indexed by list position, the
// outputs by the row itself; row_grad = G / n_c, so a row's result does not depend on the list it came in.
__global__ __launch_bounds__(MDE_BLOCK) void k_pair_loss_fold_rows(int64_t n_rows, int d, int slices, double n_c,
                                                                   const double* __restrict__ part,
                                                                   const int32_t* __restrict__ rows,
                                                                   double* __restrict__ row_loss,
                                                                   float* __restrict__ row_grad) {
  const int64_t total = n_rows * (1 + d);
  for (int64_t i = (int64_t)blockIdx.x * MDE_BLOCK + threadIdx.x; i < total; i += (int64_t)gridDim.x * MDE_BLOCK) {
    double t = 0.0;
    for (int y = 0; y < slices; ++y) t += part[(int64_t)y * total + i];
    const int64_t pos = i / (1 + d);
    const int v = (int)(i - pos * (1 + d));
    const int64_t row = rows ? (int64_t)rows[pos] : pos;
    if (v == 0)
      row_loss[row] = t;
    else
      row_grad[row * d + v - 1] = (float)(t / n_c);
  }
}

// One workgroup: thread t adds the rows t, t + 256, ... in row order, thread 0 then adds the 256 threads' sums in
// thread order.  loss = sum_i row_loss[i] / (factor * pairs): factor 2 for the square problem, where every pair is in
// two rows, 1 for the rectangular one.
__global__ __launch_bounds__(MDE_BLOCK) void k_pair_loss_total(int64_t n, double pairs, double factor,
                                                               const double* __restrict__ row_loss,
                                                               double* __restrict__ loss) {
  __shared__ double sums[MDE_BLOCK];
  double t = 0.0;
  for (int64_t i = threadIdx.x; i < n; i += MDE_BLOCK) t += row_loss[i];
  sums[threadIdx.x] = t;
  __syncthreads();
  if (threadIdx.x == 0) {
    double a = sums[0];
    for (int u = 1; u < MDE_BLOCK; ++u) a += sums[u];
    loss[0] = a / (factor * pairs);
  }
}

static bool pair_loss_kind_ok(int32_t kind) { return kind >= MDE_F_L_QUADRATIC && kind <= MDE_F_L_LOG1P; }
static bool pair_loss_args_ok(int64_t n, int32_t d, int32_t slices) {
  return pair_args_ok(n, n, slices) && d >= 1 && d <= PAIR_LOSS_MAX_D;
}
static bool pair_loss_cross_args_ok(int64_t n_q, int64_t n_c, int32_t d, int32_t slices) {
  return n_q >= 1 && n_q < ((int64_t)1 << 31) && n_c >= 1 && n_c < ((int64_t)1 << 31) && slices >= 0 &&
         slices <= CROSS_MAX_SLICES && d >= 1 && d <= PAIR_LOSS_MAX_D;
}

// work: [s, n, 1 + d] doubles | the row norms of A, [n] floats (the Gram source; the room is there for either source)
extern "C" int64_t mde_pair_loss_work_bytes(int64_t n, int32_t d, int32_t slices) {
  if (!pair_loss_args_ok(n, d, slices)) {
    mde_set_error("mde_pair_loss_work_bytes: invalid arguments (2 <= n < 2^31, 1 <= d <= %d, 0 <= slices <= %d)",
                  PAIR_LOSS_MAX_D, CROSS_MAX_SLICES);
    return MDE_E_INVALID;
  }
  const int64_t s = cross_resolve_slices(n, n, slices);
  if (s < 0) return s;
  return s * n * (1 + d) * 8 + 4 * n;
}

// work: [s, n_q, 1 + d] doubles | the row norms of Q, [n_q] floats | the row norms of C, [n_c] floats
extern "C" int64_t mde_pair_loss_cross_work_bytes(int64_t n_q, int64_t n_c, int32_t d, int32_t slices) {
  if (!pair_loss_cross_args_ok(n_q, n_c, d, slices)) {
    mde_set_error("mde_pair_loss_cross_work_bytes: invalid arguments (1 <= n_q, n_c < 2^31, 1 <= d <= %d, 0 <= slices "
                  "<= %d)", PAIR_LOSS_MAX_D, CROSS_MAX_SLICES);
    return MDE_E_INVALID;
  }
  const int64_t s = cross_resolve_slices(n_q, n_c, slices);
  if (s < 0) return s;
  return s * n_q * (1 + d) * 8 + 4 * (n_q + n_c);
}

template <int DC, bool SELF, bool ROWS>
static void pair_loss_launch_dc(bool matrix, dim3 grid, hipStream_t st, int n_q, int n_c, int nf, int d, int mode,
                                int64_t slice_cols, const float* Q, const float* qn, const float* C, const float* cn,
                                const float* Dm, const float* XQ, const float* XC, int kind, MdeScalars S,
                                float d_scale, double* part, const int32_t* rows) {
  const size_t lds = knn_tile_lds_bytes(0, PAIR_TILE + PAIR_LOSS_XS + (ROWS ? KNN_BM : 0));
  const int weighted = kind == MDE_F_L_WEIGHTED_QUADRATIC || kind == MDE_F_L_WEIGHTED_POWER;
  if (matrix)
    hipLaunchKernelGGL((k_pair_loss_walk<DC, true, SELF, ROWS>), grid, dim3(MDE_BLOCK), lds, st, n_q, n_c, nf, d, mode,
                       slice_cols, Q, qn, C, cn, Dm, XQ, XC, kind, weighted, S, d_scale, part, rows);
  else
    hipLaunchKernelGGL((k_pair_loss_walk<DC, false, SELF, ROWS>), grid, dim3(MDE_BLOCK), lds, st, n_q, n_c, nf, d, mode,
                       slice_cols, Q, qn, C, cn, Dm, XQ, XC, kind, weighted, S, d_scale, part, rows);
}

// The walk of either problem on checked arguments: n_q rows (ROWS: list entries, the rows of `rows`) against the n_c
// columns in s slices; part [s, n_q, 1 + d]; qn / cn are read by the Gram source only.
template <bool SELF, bool ROWS>
static int pair_loss_walk(int64_t n_q, int64_t n_c, int32_t nf, const float* Q, const float* qn, const float* C,
                          const float* cn, int32_t mode, const float* Dm, float d_scale, int32_t d, const float* XQ,
                          const float* XC, int32_t kind, MdeScalars S, int64_t s, double* part, const int32_t* rows,
                          hipStream_t st) {
  const int64_t tiles = (n_c + KNN_BN - 1) / KNN_BN;
  const int64_t slice_cols = ((tiles + s - 1) / s) * KNN_BN;     // whole tiles; the last slices may be short or empty
  const dim3 grid((unsigned)((n_q + KNN_BM - 1) / KNN_BM), (unsigned)s);
  const bool matrix = Dm != nullptr;
  if (d == 1)
    pair_loss_launch_dc<1, SELF, ROWS>(matrix, grid, st, (int)n_q, (int)n_c, nf, d, mode, slice_cols, Q, qn, C, cn,
                                       Dm, XQ, XC, kind, S, d_scale, part, rows);
  else if (d == 2)
    pair_loss_launch_dc<2, SELF, ROWS>(matrix, grid, st, (int)n_q, (int)n_c, nf, d, mode, slice_cols, Q, qn, C, cn,
                                       Dm, XQ, XC, kind, S, d_scale, part, rows);
  else if (d == 3)
    pair_loss_launch_dc<3, SELF, ROWS>(matrix, grid, st, (int)n_q, (int)n_c, nf, d, mode, slice_cols, Q, qn, C, cn,
                                       Dm, XQ, XC, kind, S, d_scale, part, rows);
  else
    pair_loss_launch_dc<PAIR_LOSS_MAX_D, SELF, ROWS>(matrix, grid, st, (int)n_q, (int)n_c, nf, d, mode, slice_cols, Q,
                                                     qn, C, cn, Dm, XQ, XC, kind, S, d_scale, part, rows);
  MDE_LAUNCH_CHECK();
  return MDE_OK;
}

// The walk, the fold and the total of either problem on checked arguments: SELF is the square problem (rows and
// columns are the same items, the diagonal is left out, every pair is in two rows), !SELF the rectangular one.
template <bool SELF>
static int pair_loss_run(int64_t n_q, int64_t n_c, int32_t nf, const float* Q, const float* qn, const float* C,
                         const float* cn, int32_t mode, const float* Dm, float d_scale, int32_t d, const float* XQ,
                         const float* XC, int32_t kind, MdeScalars S, int64_t s, double pairs, double* loss,
                         float* grad, double* row_loss, double* part, hipStream_t st) {
  const int rc = pair_loss_walk<SELF, false>(n_q, n_c, nf, Q, qn, C, cn, mode, Dm, d_scale, d, XQ, XC, kind, S, s,
                                             part, nullptr, st);
  if (rc != MDE_OK) return rc;
  hipLaunchKernelGGL(k_pair_loss_fold, dim3(mde_grid(n_q * (1 + d), MDE_BLOCK, 4096)), dim3(MDE_BLOCK), 0, st, n_q,
                     (int)d, (int)s, pairs, part, row_loss, grad);
  MDE_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_pair_loss_total, dim3(1), dim3(MDE_BLOCK), 0, st, n_q, pairs, SELF ? 2.0 : 1.0, row_loss, loss);
  MDE_LAUNCH_CHECK();
  return MDE_OK;
}

extern "C" int mde_pair_loss(int64_t n, int32_t nf, const float* A, int32_t mode, const float* Dm, float d_scale,
                             int32_t d, const float* X, int32_t kind, float s0, float s1, float s2, int32_t slices,
                             double* loss, float* grad, double* row_loss, void* work, void* stream) {
  const bool source_ok = (A != nullptr) != (Dm != nullptr) && (!A || (nf >= 1 && (mode == 0 || mode == 1)));
  if (!pair_loss_args_ok(n, d, slices) || !source_ok || !pair_loss_kind_ok(kind) || !(d_scale > 0.0f) ||
      !isfinite(d_scale) || !X || !loss || !grad || !row_loss || !work) {
    mde_set_error("mde_pair_loss: invalid arguments (2 <= n < 2^31, 1 <= d <= %d, exactly one of A (nf >= 1, mode 0 / "
                  "1) and Dm, kind one of the MDE_F_L_* losses, d_scale positive and finite, 0 <= slices <= %d, "
                  "non-null X / outputs / work)", PAIR_LOSS_MAX_D, CROSS_MAX_SLICES);
    return MDE_E_INVALID;
  }
  const int64_t s = cross_resolve_slices(n, n, slices);
  if (s < 0) return (int)s;
  double* part = static_cast<double*>(work);
  float* an = reinterpret_cast<float*>(part + s * n * (1 + d));
  if (A) {
    const int rc = mde_row_sqnorm(n, nf, A, an, stream);
    if (rc != MDE_OK) return rc;
  }
  const MdeScalars S = {s0, s1, s2};
  const double pairs = 0.5 * (double)n * (double)(n - 1);
  return pair_loss_run<true>(n, n, nf, A, an, A, an, mode, Dm, d_scale, d, X, X, kind, S, s, pairs, loss, grad,
                             row_loss, part, mde_stream(stream));
}

// The rectangular problem: every (query row, corpus row) pair, a gradient for the query rows only.
extern "C" int mde_pair_loss_cross(int64_t n_q, int64_t n_c, int32_t nf, const float* Q, const float* C, int32_t mode,
                                   const float* Dm, float d_scale, int32_t d, const float* XQ, const float* XC,
                                   int32_t kind, float s0, float s1, float s2, int32_t slices, double* loss,
                                   float* grad, double* row_loss, void* work, void* stream) {
  const bool gram = Q != nullptr && C != nullptr && Dm == nullptr;
  const bool matrix = Q == nullptr && C == nullptr && Dm != nullptr;
  const bool source_ok = matrix || (gram && nf >= 1 && (mode == 0 || mode == 1));
  if (!pair_loss_cross_args_ok(n_q, n_c, d, slices) || !source_ok || !pair_loss_kind_ok(kind) || !(d_scale > 0.0f) ||
      !isfinite(d_scale) || !XQ || !XC || !loss || !grad || !row_loss || !work) {
    mde_set_error("mde_pair_loss_cross: invalid arguments (1 <= n_q, n_c < 2^31, 1 <= d <= %d, either both Q and C (nf "
                  ">= 1, mode 0 / 1) or Dm alone, kind one of the MDE_F_L_* losses, d_scale positive and finite, 0 <= "
                  "slices <= %d, non-null XQ / XC / outputs / work)", PAIR_LOSS_MAX_D, CROSS_MAX_SLICES);
    return MDE_E_INVALID;
  }
  const int64_t s = cross_resolve_slices(n_q, n_c, slices);
  if (s < 0) return (int)s;
  double* part = static_cast<double*>(work);
  float* qn = reinterpret_cast<float*>(part + s * n_q * (1 + d));
  float* cn = qn + n_q;
  if (gram) {
    int rc = mde_row_sqnorm(n_q, nf, Q, qn, stream);
    if (rc == MDE_OK) rc = mde_row_sqnorm(n_c, nf, C, cn, stream);
    if (rc != MDE_OK) return rc;
  }
  const MdeScalars S = {s0, s1, s2};
  const double pairs = (double)n_q * (double)n_c;
  return pair_loss_run<false>(n_q, n_c, nf, Q, qn, C, cn, mode, Dm, d_scale, d, XQ, XC, kind, S, s, pairs, loss, grad,
                              row_loss, part, mde_stream(stream));
}

// The most list entries times slices the walk of mde_pair_loss_cross_rows can hold partials for, over every list
// length 1 .. n_q: slices * n_q for a given count; for the automatic count (resolved from the LIST's length, so that
// a short list still fills the device) s * n_rows <= s * 64 qb < 64 (CROSS_GRID_PER_CU cus + qb) < 64 (GRID_PER_CU +
// 1) cus whenever the corpus is split (qb < cus), and never more than the finest split times n_q.
static int64_t pair_loss_rows_part_rows(int64_t n_q, int64_t n_c, int32_t slices) {
  if (slices != 0) return (int64_t)slices * n_q;
  int cus = 0;
  const int rc = cross_cu_count(&cus);
  if (rc != MDE_OK) return rc;
  const int64_t tiles = (n_c + KNN_BN - 1) / KNN_BN;
  const int64_t finest = tiles / CROSS_MIN_TILES > 1 ? tiles / CROSS_MIN_TILES : 1;
  int64_t split = (int64_t)KNN_BM * (CROSS_GRID_PER_CU + 1) * cus;
  if (split > finest * n_q) split = finest * n_q;
  return split > n_q ? split : n_q;
}

// work: [part_rows, 1 + d] doubles | the row norms of Q, [n_q] floats | the row norms of C, [n_c] floats
extern "C" int64_t mde_pair_loss_cross_rows_work_bytes(int64_t n_q, int64_t n_c, int32_t d, int32_t slices) {
  if (!pair_loss_cross_args_ok(n_q, n_c, d, slices)) {
    mde_set_error("mde_pair_loss_cross_rows_work_bytes: invalid arguments (1 <= n_q, n_c < 2^31, 1 <= d <= %d, 0 <= "
                  "slices <= %d)", PAIR_LOSS_MAX_D, CROSS_MAX_SLICES);
    return MDE_E_INVALID;
  }
  const int64_t part_rows = pair_loss_rows_part_rows(n_q, n_c, slices);
  if (part_rows < 0) return part_rows;
  return part_rows * (1 + d) * 8 + 4 * (n_q + n_c);
}

// The rectangular problem over a list of query rows: per-row sums only, written at the rows' own indices.
extern "C" int mde_pair_loss_cross_rows(int64_t n_q, int64_t n_c, int32_t nf, const float* Q, const float* C,
                                        int32_t mode, const float* Dm, float d_scale, int32_t d, const float* XQ,
                                        const float* XC, int32_t kind, float s0, float s1, float s2, int32_t slices,
                                        int64_t n_rows, const int32_t* rows, double* row_loss, float* row_grad,
                                        void* work, void* stream) {
  const bool gram = Q != nullptr && C != nullptr && Dm == nullptr;
  const bool matrix = Q == nullptr && C == nullptr && Dm != nullptr;
  const bool source_ok = matrix || (gram && nf >= 1 && (mode == 0 || mode == 1));
  const bool rows_ok = n_rows >= 1 && n_rows <= n_q && (rows != nullptr || n_rows == n_q);
  if (!pair_loss_cross_args_ok(n_q, n_c, d, slices) || !source_ok || !rows_ok || !pair_loss_kind_ok(kind) ||
      !(d_scale > 0.0f) || !isfinite(d_scale) || !XQ || !XC || !row_loss || !row_grad || !work) {
    mde_set_error("mde_pair_loss_cross_rows: invalid arguments (1 <= n_q, n_c < 2^31, 1 <= d <= %d, either both Q and "
                  "C (nf >= 1, mode 0 / 1) or Dm alone, kind one of the MDE_F_L_* losses, d_scale positive and finite, "
                  "0 <= slices <= %d, 1 <= n_rows <= n_q and n_rows == n_q without rows, non-null XQ / XC / outputs / "
                  "work)", PAIR_LOSS_MAX_D, CROSS_MAX_SLICES);
    return MDE_E_INVALID;
  }
  const int64_t s = cross_resolve_slices(n_rows, n_c, slices);
  if (s < 0) return (int)s;
  const int64_t part_rows = pair_loss_rows_part_rows(n_q, n_c, slices);
  if (part_rows < 0) return (int)part_rows;
  double* part = static_cast<double*>(work);
  float* qn = reinterpret_cast<float*>(part + part_rows * (1 + d));
  float* cn = qn + n_q;
  if (gram) {
    int rc = mde_row_sqnorm(n_q, nf, Q, qn, stream);
    if (rc == MDE_OK) rc = mde_row_sqnorm(n_c, nf, C, cn, stream);
    if (rc != MDE_OK) return rc;
  }
  const MdeScalars S = {s0, s1, s2};
  hipStream_t st = mde_stream(stream);
  const int rc = pair_loss_walk<false, true>(n_rows, n_c, nf, Q, qn, C, cn, mode, Dm, d_scale, d, XQ, XC, kind, S, s,
                                             part, rows, st);
  if (rc != MDE_OK) return rc;
  hipLaunchKernelGGL(k_pair_loss_fold_rows, dim3(mde_grid(n_rows * (1 + d), MDE_BLOCK, 4096)), dim3(MDE_BLOCK), 0, st,
                     n_rows, (int)d, (int)s, (double)n_c, part, rows, row_loss, row_grad);
  MDE_LAUNCH_CHECK();
  return MDE_OK;
}

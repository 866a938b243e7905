// mde_knn.hip -- exact k-nearest-neighbour search on a data matrix.
//   [ref: pymde/preprocess/data_matrix.py:91-178 k_nearest_neighbors -- sklearn brute force for
//    n < 10 000, pynndescent (approximate, un-vendored) above; here: exact at every size]
// The search itself is k_knn_cross<true> below: the 64x64 Gram tile of mde_knn_tile.h with the data matrix on
// both sides, one slice, and self matches excluded by index.
#include "mde_knn_tile.h"
#include "mde_knn_slices.h"

__global__ __launch_bounds__(MDE_BLOCK) void k_row_sqnorm(int64_t n, int nf, const float* __restrict__ X,
                                                          float* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int64_t w0 = ((int64_t)blockIdx.x * MDE_BLOCK + threadIdx.x) >> 6;
  const int64_t nw = ((int64_t)gridDim.x * MDE_BLOCK) >> 6;
  for (int64_t r = w0; r < n; r += nw) {
    float s = 0.0f;
    for (int c = lane; c < nf; c += 64) {
      const float v = X[r * nf + c];
      s = fmaf(v, v, s);
    }
    s = mde_wave_sum(s);
    if (lane == 0) out[r] = s;
  }
}

// out[r] = |X[r]|^2 (f32, summed as mde_knn's norms are): the row norms the approximate search takes.
extern "C" int mde_row_sqnorm(int64_t n, int32_t nf, const float* data, float* out, void* stream) {
  if (n <= 0 || nf <= 0 || !data || !out) return MDE_E_INVALID;
  if (n >= ((int64_t)1 << 31)) return MDE_E_TOO_LARGE;
  hipLaunchKernelGGL(k_row_sqnorm, dim3(mde_grid(n * 64, MDE_BLOCK, 4096)), dim3(MDE_BLOCK), 0, mde_stream(stream),
                     n, nf, data, out);
  MDE_LAUNCH_CHECK();
  return MDE_OK;
}

// ---------------------------------------------------------------- translation to the column means
// |x|^2 + |y|^2 - 2 x.y in f32 is accurate to ~1e-7 of |x|^2 + |y|^2, so a common offset of the rows that
// dominates their spread swallows the distances.  Euclidean distance is translation invariant: the callers
// search the rows minus their column means instead.  Three kernels, all O(n nf) beside the O(n^2 nf) search.
//
// k_col_stats: workgroup (x, y) owns columns [64 x, 64 x + 64) and the rows 4 y + (tid >> 6) + 4 chunks i: a
// wave reads 64 consecutive floats of one row.  Sum and sum of squares per column in double (the product of
// two floats is exact there), the four row lanes folded through LDS in a fixed order and written to
// part[y][0 / 1][c]; k_col_stats_fold adds the chunks in order -- no floating-point atomics, so the means are
// the same on every run.  The smallest index of a row that holds a NaN or an infinity is min-reduced into
// *bad_row (an integer atomic: order-free).  part may be NULL: the non-finite scan alone.
#define COLS_BX 64
#define COLS_MAX_CHUNKS 512
#define COLS_MAX_PARTIALS ((int64_t)1 << 22)   // chunks * nf: at most 64 MiB of partials
static int col_stats_chunks(int64_t n, int32_t nf) {
  int64_t c = (n + 63) / 64;
  if (c > COLS_MAX_CHUNKS) c = COLS_MAX_CHUNKS;
  if (c > COLS_MAX_PARTIALS / nf) c = COLS_MAX_PARTIALS / nf;
  return c < 1 ? 1 : (int)c;
}

__global__ __launch_bounds__(MDE_BLOCK) void k_col_stats(int64_t n, int nf, const float* __restrict__ X,
                                                         double* __restrict__ part, int* __restrict__ bad_row) {
  static_assert(MDE_BLOCK == 4 * COLS_BX, "k_col_stats: four row lanes of 64 columns");
  __shared__ double sh[3][2][COLS_BX];
  const int cx = threadIdx.x & 63, ry = threadIdx.x >> 6;
  const int c = blockIdx.x * COLS_BX + cx;
  double s = 0.0, q = 0.0;
  int bad = 0x7fffffff;
  if (c < nf)
    for (int64_t r = (int64_t)blockIdx.y * 4 + ry; r < n; r += (int64_t)gridDim.y * 4) {
      const float v = X[r * nf + c];
      s += (double)v;
      q += (double)v * (double)v;
      if (!(fabsf(v) <= 3.402823466e+38f) && (int)r < bad) bad = (int)r;
    }
  if (ry > 0) {
    sh[ry - 1][0][cx] = s;
    sh[ry - 1][1][cx] = q;
  }
  __syncthreads();
  if (part && ry == 0 && c < nf) {
    for (int i = 0; i < 3; ++i) {
      s += sh[i][0][cx];
      q += sh[i][1][cx];
    }
    part[((int64_t)blockIdx.y * 2 + 0) * nf + c] = s;
    part[((int64_t)blockIdx.y * 2 + 1) * nf + c] = q;
  }
  if (bad != 0x7fffffff) atomicMin(bad_row, bad);
}

// stats[c] = mean of column c, stats[nf + c] = its variance (population; clamped at 0), both in double
__global__ __launch_bounds__(MDE_BLOCK) void k_col_stats_fold(int64_t n, int nf, int chunks,
                                                              const double* __restrict__ part,
                                                              double* __restrict__ stats) {
  const int c = blockIdx.x * MDE_BLOCK + threadIdx.x;
  if (c >= nf) return;
  double s = 0.0, q = 0.0;
  for (int y = 0; y < chunks; ++y) {
    s += part[((int64_t)y * 2 + 0) * nf + c];
    q += part[((int64_t)y * 2 + 1) * nf + c];
  }
  const double mean = s / (double)n, var = q / (double)n - mean * mean;
  stats[c] = mean;
  stats[nf + c] = var > 0.0 ? var : 0.0;
}

__global__ void k_bad_row_init(int* bad_row) { *bad_row = 0x7fffffff; }

// out[r][c] = x[r][c] - mu[c], subtracted in double and rounded once (one wave per row, as k_row_sqnorm)
__global__ __launch_bounds__(MDE_BLOCK) void k_rows_subtract(int64_t n, int nf, const float* __restrict__ X,
                                                             const double* __restrict__ mu,
                                                             float* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int64_t w0 = ((int64_t)blockIdx.x * MDE_BLOCK + threadIdx.x) >> 6;
  const int64_t nw = ((int64_t)gridDim.x * MDE_BLOCK) >> 6;
  for (int64_t r = w0; r < n; r += nw)
    for (int c = lane; c < nf; c += 64) out[r * nf + c] = (float)((double)X[r * nf + c] - mu[c]);
}

extern "C" int64_t mde_col_stats_work_bytes(int64_t n, int32_t nf) {
  if (n <= 0 || nf <= 0) {
    mde_set_error("mde_col_stats_work_bytes: invalid arguments (n >= 1, nf >= 1)");
    return MDE_E_INVALID;
  }
  return (int64_t)sizeof(double) * 2 * col_stats_chunks(n, nf) * nf;
}

// stats_out: double [2, nf] on the device = (column means, column variances); bad_row_out: int32 [1] on the
// device = the first row that holds a NaN or an infinity (INT32_MAX when there is none; the statistics mean
// nothing then); work: mde_col_stats_work_bytes(n, nf) bytes of scratch.  stats_out and work both NULL: the
// non-finite scan alone (one pass, no partials, no fold).
extern "C" int mde_col_stats(int64_t n, int32_t nf, const float* data, double* stats_out, int32_t* bad_row_out,
                             void* work, void* stream) {
  if (n <= 0 || nf <= 0 || !data || !bad_row_out || (stats_out == nullptr) != (work == nullptr)) {
    mde_set_error("mde_col_stats: invalid arguments (n >= 1, nf >= 1, non-null data / bad_row_out; stats_out and "
                  "work both given or both NULL)");
    return MDE_E_INVALID;
  }
  if (n >= ((int64_t)1 << 31)) return MDE_E_TOO_LARGE;
  hipStream_t st = mde_stream(stream);
  const int chunks = col_stats_chunks(n, nf);
  double* part = static_cast<double*>(work);
  hipLaunchKernelGGL(k_bad_row_init, dim3(1), dim3(1), 0, st, bad_row_out);
  MDE_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_col_stats, dim3((unsigned)((nf + COLS_BX - 1) / COLS_BX), (unsigned)chunks), dim3(MDE_BLOCK), 0,
                     st, n, nf, data, part, bad_row_out);
  MDE_LAUNCH_CHECK();
  if (!stats_out) return MDE_OK;
  hipLaunchKernelGGL(k_col_stats_fold, dim3((unsigned)((nf + MDE_BLOCK - 1) / MDE_BLOCK)), dim3(MDE_BLOCK), 0, st, n,
                     nf, chunks, part, stats_out);
  MDE_LAUNCH_CHECK();
  return MDE_OK;
}

// out [n, nf] = data - mu (mu: double [nf] on the device), rounded to f32 once.
extern "C" int mde_rows_subtract(int64_t n, int32_t nf, const float* data, const double* mu, float* out,
                                 void* stream) {
  if (n <= 0 || nf <= 0 || !data || !mu || !out) {
    mde_set_error("mde_rows_subtract: invalid arguments (n >= 1, nf >= 1, non-null data / mu / out)");
    return MDE_E_INVALID;
  }
  if (n >= ((int64_t)1 << 31)) return MDE_E_TOO_LARGE;
  hipLaunchKernelGGL(k_rows_subtract, dim3(mde_grid(n * 64, MDE_BLOCK, 4096)), dim3(MDE_BLOCK), 0, mde_stream(stream),
                     n, nf, data, mu, out);
  MDE_LAUNCH_CHECK();
  return MDE_OK;
}

// ---------------------------------------------------------------- the search: self-join and query against corpus (DESIGN sections 6, 6f)
// The Gram tile of mde_knn_tile.h on two matrices and a 2-D grid: workgroup (x, y) owns query rows
// [64 x, 64 x + 64) and scans the corpus columns of slice y, [y * slice_cols, (y + 1) * slice_cols) cut at
// n_c (slice_cols a multiple of 64; a slice past the end is empty and writes an empty list).  Its sorted
// top-k goes to list y of the outputs, laid out [slices, n_q, k]: with one slice these are the final
// outputs, otherwise scratch that k_knn_cross_merge folds.  SELF: Q and C are one matrix (the exact
// self-join of mde_knn) and a row does not list itself; otherwise nothing is excluded.  Columns are
// offered in increasing index, so each list is ordered by (d2, index): insertion only when a candidate beats
// the current k-th best, which becomes rare quickly.
template <bool SELF>
__global__ __launch_bounds__(MDE_BLOCK) void k_knn_cross(int n_q, int n_c, int nf, int k, int64_t slice_cols,
                                                         const float* __restrict__ Q, const float* __restrict__ C,
                                                         const float* __restrict__ qn,
                                                         const float* __restrict__ cn,
                                                         int32_t* __restrict__ idx_out,
                                                         float* __restrict__ d2_out) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const knn_tile_lds s = knn_tile_carve(lds, k, 0);
  const int tid = threadIdx.x;
  const int64_t row0 = (int64_t)blockIdx.x * KNN_BM;
  const int64_t lo = (int64_t)blockIdx.y * slice_cols;
  const int64_t c_lo = lo < n_c ? lo : n_c, c_hi = lo + slice_cols < n_c ? lo + slice_cols : n_c;
  knn_lists_init(s.bestd, s.besti, KNN_BM * k);
  float worst = 3.402823466e+38f;            // thread t < 64: current k-th best of row t
  // the rows this thread stages, (tid >> 5) + 8 q of either side: a row past the matrix reads its last row
  // and is zeroed, so every load stays inside Q / C
  const float* arow[KNN_STG];
  bool aok[KNN_STG];
#pragma unroll
  for (int q = 0; q < KNN_STG; ++q) {
    const int64_t gr = row0 + (tid >> 5) + 8 * q;
    aok[q] = gr < n_q;
    arow[q] = Q + (aok[q] ? gr : n_q - 1) * nf;
  }
  for (int64_t col0 = c_lo; col0 < c_hi; col0 += KNN_BN) {
    const float* brow[KNN_STG];
    bool bok[KNN_STG];
#pragma unroll
    for (int q = 0; q < KNN_STG; ++q) {
      const int64_t gc = col0 + (tid >> 5) + 8 * q;
      bok[q] = gc < n_c;
      brow[q] = C + (bok[q] ? gc : n_c - 1) * nf;
    }
    const f32x16 acc = knn_gram_tile(s.sA, s.sB, nf, arow, aok, brow, bok);
    knn_park_tile(
        s.sD, acc,
        [&](int r, int c) { return row0 + r < n_q && col0 + c < n_c && !(SELF && row0 + r == col0 + c); },
        [&](int r) { return qn[row0 + r]; }, [&](int c) { return cn[col0 + c]; });
    __syncthreads();
    if (tid < KNN_BM)
      mde_topk_merge(s.sD + tid * (KNN_BN + 1), KNN_BN, (int)col0, k, s.bestd + tid * k, s.besti + tid * k, worst);
  }
  __syncthreads();
  const int rows = n_q - row0 < KNN_BM ? (int)(n_q - row0) : KNN_BM;
  const int64_t base = ((int64_t)blockIdx.y * n_q + row0) * k;   // the block's rows are contiguous in list y
  knn_lists_store(s.bestd, s.besti, rows * k, idx_out + base, d2_out + base);
}

// idx_out [n, k] int32 (-1 where fewer than k other items exist), d2_out [n, k] squared Euclidean
// distances, ascending per row.  sqn_work: n floats of scratch.
extern "C" int mde_knn(int64_t n, int32_t nf, const float* data, int32_t k, int32_t* idx_out,
                       float* d2_out, float* sqn_work, void* stream) {
  if (n <= 0 || nf <= 0 || k <= 0 || k > KNN_MAXK || !data || !idx_out || !d2_out || !sqn_work) {
    mde_set_error("mde_knn: invalid arguments (1 <= k <= %d)", KNN_MAXK);
    return MDE_E_INVALID;
  }
  if (n >= ((int64_t)1 << 31)) return MDE_E_TOO_LARGE;
  hipStream_t st = mde_stream(stream);
  hipLaunchKernelGGL(k_row_sqnorm, dim3(mde_grid(n * 64, MDE_BLOCK, 4096)), dim3(MDE_BLOCK), 0, st, n, nf,
                     data, sqn_work);
  MDE_LAUNCH_CHECK();
  const int rc = knn_raise_lds_limit<k_knn_cross<true>>(96 * 1024);
  if (rc != MDE_OK) return rc;
  // one slice of every column tile: the self-join does not split the corpus
  hipLaunchKernelGGL(k_knn_cross<true>, dim3((unsigned)((n + KNN_BM - 1) / KNN_BM)), dim3(MDE_BLOCK),
                     knn_tile_lds_bytes(k, 0), st, (int)n, (int)n, nf, k, (n + KNN_BN - 1) / KNN_BN * KNN_BN, data, data,
                     sqn_work, sqn_work, idx_out, d2_out);
  MDE_LAUNCH_CHECK();
  return MDE_OK;
}

// The slice rule and k_knn_cross_merge, which folds the per-slice lists: mde_knn_slices.h.

extern "C" int64_t mde_knn_cross_work_bytes(int64_t n_q, int64_t n_c, int32_t k, int32_t slices) {
  if (!cross_args_ok(n_q, n_c, k, slices)) {
    mde_set_error("mde_knn_cross_work_bytes: invalid arguments (1 <= k <= %d, 0 <= slices <= %d)", KNN_MAXK,
                  CROSS_MAX_SLICES);
    return MDE_E_INVALID;
  }
  const int64_t s = cross_resolve_slices(n_q, n_c, slices);
  if (s < 0) return s;
  int64_t words = n_q + n_c;                                    // the row norms of Q and C
  if (s > 1) words += 2 * s * n_q * (int64_t)k;                 // partial lists: d2 and idx, [s, n_q, k] each
  return 4 * words;
}

extern "C" int mde_knn_cross(int64_t n_q, int64_t n_c, int32_t nf, const float* Q, const float* C, int32_t k,
                             int32_t slices, int32_t* idx_out, float* d2_out, void* work, void* stream) {
  if (!cross_args_ok(n_q, n_c, k, slices) || nf <= 0 || !Q || !C || !idx_out || !d2_out || !work) {
    mde_set_error("mde_knn_cross: invalid arguments (1 <= k <= %d, 0 <= slices <= %d, n_q, n_c, nf >= 1)",
                  KNN_MAXK, CROSS_MAX_SLICES);
    return MDE_E_INVALID;
  }
  if (n_q >= ((int64_t)1 << 31) || n_c >= ((int64_t)1 << 31)) return MDE_E_TOO_LARGE;
  const int64_t s = cross_resolve_slices(n_q, n_c, slices);
  if (s < 0) return (int)s;
  hipStream_t st = mde_stream(stream);
  float* qn = static_cast<float*>(work);
  float* cn = qn + n_q;
  float* pd = cn + n_c;                                         // [s, n_q, k], used when s > 1
  int32_t* pi = reinterpret_cast<int32_t*>(pd + s * n_q * (int64_t)k);
  hipLaunchKernelGGL(k_row_sqnorm, dim3(mde_grid(n_q * 64, MDE_BLOCK, 4096)), dim3(MDE_BLOCK), 0, st, n_q, nf, Q,
                     qn);
  MDE_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_row_sqnorm, dim3(mde_grid(n_c * 64, MDE_BLOCK, 4096)), dim3(MDE_BLOCK), 0, st, n_c, nf, C,
                     cn);
  MDE_LAUNCH_CHECK();
  const size_t lds_merge = (size_t)KNN_BM * k * 2 * (sizeof(float) + sizeof(int));
  int rc = knn_raise_lds_limit<k_knn_cross<false>>(96 * 1024);
  if (rc == MDE_OK) rc = knn_raise_lds_limit<k_knn_cross_merge>(96 * 1024);
  if (rc != MDE_OK) return rc;
  const int64_t tiles = (n_c + KNN_BN - 1) / KNN_BN;
  const int64_t slice_cols = ((tiles + s - 1) / s) * KNN_BN;    // whole tiles; the last slices may be short or empty
  const unsigned qb = (unsigned)((n_q + KNN_BM - 1) / KNN_BM);
  hipLaunchKernelGGL(k_knn_cross<false>, dim3(qb, (unsigned)s), dim3(MDE_BLOCK), knn_tile_lds_bytes(k, 0), st,
                     (int)n_q, (int)n_c, nf, k, slice_cols, Q, C, qn, cn, s > 1 ? pi : idx_out, s > 1 ? pd : d2_out);
  MDE_LAUNCH_CHECK();
  if (s > 1) {
    hipLaunchKernelGGL(k_knn_cross_merge, dim3(qb), dim3(MDE_BLOCK), lds_merge, st, (int)n_q, k, (int)s, pd, pi,
                       idx_out, d2_out);
    MDE_LAUNCH_CHECK();
  }
  return MDE_OK;
}

// Directed neighbour lists -> edge list for mde_edges_count_unique: pairs_out[r * k + c] = (r, idx[r][c]).
// Empty slots (idx < 0) and, when `val` is given, entries with val > max_value become the self pair
// (r, r), which the edge counter drops [ref: data_matrix.py:147-175 -- neighbours beyond max_distance
// get weight 0 and vanish from the graph].
__global__ __launch_bounds__(MDE_BLOCK) void k_knn_pairs(int64_t total, int k, const int32_t* __restrict__ idx,
                                                         const float* __restrict__ val, float max_value,
                                                         int64_t* __restrict__ pairs) {
  for (int64_t i = (int64_t)blockIdx.x * MDE_BLOCK + threadIdx.x; i < total;
       i += (int64_t)gridDim.x * MDE_BLOCK) {
    const int64_t r = i / k;
    int64_t j = idx[i];
    if (j < 0 || (val && !(val[i] <= max_value))) j = r;
    reinterpret_cast<longlong2*>(pairs)[i] = make_longlong2((long long)r, (long long)j);
  }
}
extern "C" int mde_knn_pairs(int64_t n, int32_t k, const int32_t* idx, const float* val, float max_value,
                             int64_t* pairs_out, void* stream) {
  if (n <= 0 || k <= 0 || !idx || !pairs_out) return MDE_E_INVALID;
  hipLaunchKernelGGL(k_knn_pairs, dim3(mde_grid(n * k, MDE_BLOCK, 4096)), dim3(MDE_BLOCK), 0, mde_stream(stream),
                     n * (int64_t)k, k, idx, val, max_value, pairs_out);
  MDE_LAUNCH_CHECK();
  return MDE_OK;
}

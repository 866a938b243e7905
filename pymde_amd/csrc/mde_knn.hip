// mde_knn.hip -- exact k-nearest-neighbour search on a data matrix.
//   [ref: pymde/preprocess/data_matrix.py:91-178 k_nearest_neighbors -- sklearn brute force for
//    n < 10 000, pynndescent (approximate, un-vendored) above; here: exact at every size]
// Squared distances are formed as |x|^2 + |y|^2 - 2 x.y with the Gram tile x.y on the f32 matrix
// cores (v_mfma_f32_32x32x2_f32, exact f32): a 256-thread workgroup owns 64 query rows and walks
// the candidates 64 at a time; each wave accumulates one 32x32 quadrant of the 64x64 tile over the
// features, staged through LDS in 32-wide chunks (rows padded to 33 floats: conflict-free operand
// reads; the next chunk's global loads overlap the current chunk's MFMAs).  The tile of squared distances is parked in LDS and one thread per query row merges its
// 64 candidates into the row's sorted top-k list (insertion only when a candidate beats the current
// k-th best, which becomes rare quickly).  Self matches are excluded by index.
#include "mde_common.h"
#include "mde_topk.h"

typedef float f32x16 __attribute__((ext_vector_type(16)));

#define KNN_BM 64
#define KNN_BN 64
#define KNN_KB 32
#define KNN_KBP 33
#define KNN_MAXK 64

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

__global__ __launch_bounds__(MDE_BLOCK) void k_knn(int n, int nf, int k, const float* __restrict__ X,
                                                   const float* __restrict__ sqn,
                                                   int32_t* __restrict__ idx_out,
                                                   float* __restrict__ d2_out) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* sA = lds;                           // [KNN_BM][KNN_KBP]
  float* sB = sA + KNN_BM * KNN_KBP;         // [KNN_BN][KNN_KBP]
  float* sD = sB + KNN_BN * KNN_KBP;         // [KNN_BM][KNN_BN + 1] squared distances of the tile
  float* bestd = sD + KNN_BM * (KNN_BN + 1); // [KNN_BM][k]
  int* besti = reinterpret_cast<int*>(bestd + KNN_BM * k);  // [KNN_BM][k]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wi = wave >> 1, wj = wave & 1;   // quadrant of the 64x64 tile
  const int row0 = blockIdx.x * KNN_BM;
  for (int i = tid; i < KNN_BM * k; i += MDE_BLOCK) {
    bestd[i] = 3.402823466e+38f;
    besti[i] = -1;
  }
  float worst = 3.402823466e+38f;            // thread t < 64: current k-th best of row t
  const int li = lane & 31, lk = lane >> 5;
  for (int col0 = 0; col0 < n; col0 += KNN_BN) {
    f32x16 acc;
#pragma unroll
    for (int q = 0; q < 16; ++q) acc[q] = 0.0f;
    // feature chunks of KNN_KB: the next chunk's global loads are issued before the MFMAs of the
    // current one and committed to LDS after them (register double buffering), so the matrix
    // cores do not wait for the staging latency
    constexpr int STG = (KNN_BM * KNN_KB) / MDE_BLOCK;
    float ra[STG], rb[STG];
    auto fetch = [&](int k0) {
#pragma unroll
      for (int q = 0; q < STG; ++q) {
        const int e = tid + q * MDE_BLOCK;
        const int r = e >> 5, c = e & 31;
        const int gr = row0 + r, gc = col0 + r, f = k0 + c;
        // plain loads from clamped addresses, zeroed afterwards: a predicated load is a branch around
        // it and the sixteen loads of a chunk would go out one memory latency after the other
        const int fc = f < nf ? f : nf - 1;
        const float va = X[(int64_t)(gr < n ? gr : n - 1) * nf + fc];
        const float vb = X[(int64_t)(gc < n ? gc : n - 1) * nf + fc];
        ra[q] = (gr < n && f < nf) ? va : 0.0f;
        rb[q] = (gc < n && f < nf) ? vb : 0.0f;
      }
    };
    fetch(0);
    for (int k0 = 0; k0 < nf; k0 += KNN_KB) {
      __syncthreads();
#pragma unroll
      for (int q = 0; q < STG; ++q) {
        const int e = tid + q * MDE_BLOCK;
        const int r = e >> 5, c = e & 31;
        sA[r * KNN_KBP + c] = ra[q];
        sB[r * KNN_KBP + c] = rb[q];
      }
      __syncthreads();
      if (k0 + KNN_KB < nf) fetch(k0 + KNN_KB);
      const float* pa = sA + (wi * 32 + li) * KNN_KBP + lk;
      const float* pb = sB + (wj * 32 + li) * KNN_KBP + lk;
#pragma unroll
      for (int kk = 0; kk < KNN_KB; kk += 2)
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(pa[kk], pb[kk], acc, 0, 0, 0);
    }
    // C/D map of the 32x32 tile: col = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const int r = wi * 32 + (q & 3) + 8 * (q >> 2) + 4 * lk;
      const int c = wj * 32 + li;
      const int gr = row0 + r, gc = col0 + c;
      float d2 = 3.402823466e+38f;
      if (gr < n && gc < n && gr != gc) d2 = fmaxf(sqn[gr] + sqn[gc] - 2.0f * acc[q], 0.0f);
      sD[r * (KNN_BN + 1) + c] = d2;
    }
    __syncthreads();
    if (tid < KNN_BM)
      mde_topk_merge(sD + tid * (KNN_BN + 1), KNN_BN, col0, k, bestd + tid * k, besti + tid * k, worst);
  }
  __syncthreads();
  for (int i = tid; i < KNN_BM * k; i += MDE_BLOCK) {
    const int r = i / k, gr = row0 + r;
    if (gr < n) {
      idx_out[(int64_t)gr * k + (i % k)] = besti[i];
      d2_out[(int64_t)gr * k + (i % k)] = bestd[i];
    }
  }
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
  const size_t lds = sizeof(float) * (size_t)(KNN_BM * KNN_KBP + KNN_BN * KNN_KBP + KNN_BM * (KNN_BN + 1)) +
                     (size_t)KNN_BM * k * (sizeof(float) + sizeof(int));
  static bool attr = false;
  if (!attr) {
    MDE_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k_knn),
                                hipFuncAttributeMaxDynamicSharedMemorySize, 96 * 1024));
    attr = true;
  }
  hipLaunchKernelGGL(k_knn, dim3((unsigned)((n + KNN_BM - 1) / KNN_BM)), dim3(MDE_BLOCK), lds, st, (int)n,
                     nf, k, data, sqn_work, idx_out, d2_out);
  MDE_LAUNCH_CHECK();
  return MDE_OK;
}

// out[r] = |X[r]|^2 (f32, summed as k_knn's norms are): the row norms the approximate search takes.
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

// ---------------------------------------------------------------- query against corpus
// The tile scheme of k_knn on two matrices and a 2-D grid: workgroup (x, y) owns query rows
// [64 x, 64 x + 64) and scans the corpus columns of slice y, [y * slice_cols, (y + 1) * slice_cols) cut at
// n_c (slice_cols a multiple of 64; a slice past the end is empty and writes an empty list).  Its sorted
// top-k goes to list y of the outputs, laid out [slices, n_q, k]: with one slice these are the final
// outputs, otherwise scratch that k_knn_cross_merge folds.  Nothing is excluded as "self".  Columns are
// offered in increasing index, so each list is ordered by (d2, index).
__global__ __launch_bounds__(MDE_BLOCK) void k_knn_cross(int n_q, int n_c, int nf, int k, int64_t slice_cols,
                                                         const float* __restrict__ Q, const float* __restrict__ C,
                                                         const float* __restrict__ qn,
                                                         const float* __restrict__ cn,
                                                         int32_t* __restrict__ idx_out,
                                                         float* __restrict__ d2_out) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* sA = lds;                           // [KNN_BM][KNN_KBP]
  float* sB = sA + KNN_BM * KNN_KBP;         // [KNN_BN][KNN_KBP]
  float* sD = sB + KNN_BN * KNN_KBP;         // [KNN_BM][KNN_BN + 1] squared distances of the tile
  float* bestd = sD + KNN_BM * (KNN_BN + 1); // [KNN_BM][k]
  int* besti = reinterpret_cast<int*>(bestd + KNN_BM * k);  // [KNN_BM][k]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wi = wave >> 1, wj = wave & 1;   // quadrant of the 64x64 tile
  const int64_t row0 = (int64_t)blockIdx.x * KNN_BM;
  const int64_t lo = (int64_t)blockIdx.y * slice_cols;
  const int64_t c_lo = lo < n_c ? lo : n_c, c_hi = lo + slice_cols < n_c ? lo + slice_cols : n_c;
  for (int i = tid; i < KNN_BM * k; i += MDE_BLOCK) {
    bestd[i] = 3.402823466e+38f;
    besti[i] = -1;
  }
  float worst = 3.402823466e+38f;            // thread t < 64: current k-th best of row t
  const int li = lane & 31, lk = lane >> 5;
  for (int64_t col0 = c_lo; col0 < c_hi; col0 += KNN_BN) {
    f32x16 acc;
#pragma unroll
    for (int q = 0; q < 16; ++q) acc[q] = 0.0f;
    constexpr int STG = (KNN_BM * KNN_KB) / MDE_BLOCK;
    float ra[STG], rb[STG];
    auto fetch = [&](int k0) {
#pragma unroll
      for (int q = 0; q < STG; ++q) {
        const int e = tid + q * MDE_BLOCK;
        const int r = e >> 5, c = e & 31;
        const int64_t gr = row0 + r, gc = col0 + r;
        const int f = k0 + c;
        // clamped addresses, zeroed afterwards (as in k_knn): every load stays inside Q / C
        const int fc = f < nf ? f : nf - 1;
        const float va = Q[(gr < n_q ? gr : n_q - 1) * nf + fc];
        const float vb = C[(gc < n_c ? gc : n_c - 1) * nf + fc];
        ra[q] = (gr < n_q && f < nf) ? va : 0.0f;
        rb[q] = (gc < n_c && f < nf) ? vb : 0.0f;
      }
    };
    fetch(0);
    for (int k0 = 0; k0 < nf; k0 += KNN_KB) {
      __syncthreads();
#pragma unroll
      for (int q = 0; q < STG; ++q) {
        const int e = tid + q * MDE_BLOCK;
        const int r = e >> 5, c = e & 31;
        sA[r * KNN_KBP + c] = ra[q];
        sB[r * KNN_KBP + c] = rb[q];
      }
      __syncthreads();
      if (k0 + KNN_KB < nf) fetch(k0 + KNN_KB);
      const float* pa = sA + (wi * 32 + li) * KNN_KBP + lk;
      const float* pb = sB + (wj * 32 + li) * KNN_KBP + lk;
#pragma unroll
      for (int kk = 0; kk < KNN_KB; kk += 2)
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(pa[kk], pb[kk], acc, 0, 0, 0);
    }
    // C/D map of the 32x32 tile: col = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const int r = wi * 32 + (q & 3) + 8 * (q >> 2) + 4 * lk;
      const int c = wj * 32 + li;
      const int64_t gr = row0 + r, gc = col0 + c;
      float d2 = 3.402823466e+38f;
      if (gr < n_q && gc < n_c) d2 = fmaxf(qn[gr] + cn[gc] - 2.0f * acc[q], 0.0f);
      sD[r * (KNN_BN + 1) + c] = d2;
    }
    __syncthreads();
    if (tid < KNN_BM)
      mde_topk_merge(sD + tid * (KNN_BN + 1), KNN_BN, (int)col0, k, bestd + tid * k, besti + tid * k, worst);
  }
  __syncthreads();
  const int rows = n_q - row0 < KNN_BM ? (int)(n_q - row0) : KNN_BM;
  const int64_t base = ((int64_t)blockIdx.y * n_q + row0) * k;   // the block's rows are contiguous in list y
  for (int i = tid; i < rows * k; i += MDE_BLOCK) {
    idx_out[base + i] = besti[i];
    d2_out[base + i] = bestd[i];
  }
}

// Folds the `slices` sorted lists of every query row ([slices, n_q, k], empty slots FLT_MAX / -1) into the
// row's top-k by (d2, index).  A workgroup owns 64 query rows: their 64 k entries of one slice are
// contiguous, are staged through LDS by all threads, and one thread per row merges them.
__global__ __launch_bounds__(MDE_BLOCK) void k_knn_cross_merge(int n_q, int k, int slices,
                                                               const float* __restrict__ pd,
                                                               const int32_t* __restrict__ pi,
                                                               int32_t* __restrict__ idx_out,
                                                               float* __restrict__ d2_out) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* sd = lds;                                          // [KNN_BM][k] one slice's lists
  int* si = reinterpret_cast<int*>(sd + KNN_BM * k);
  float* bestd = reinterpret_cast<float*>(si + KNN_BM * k); // [KNN_BM][k]
  int* besti = reinterpret_cast<int*>(bestd + KNN_BM * k);
  const int tid = threadIdx.x;
  const int64_t row0 = (int64_t)blockIdx.x * KNN_BM;
  const int rows = n_q - row0 < KNN_BM ? (int)(n_q - row0) : KNN_BM;
  for (int i = tid; i < KNN_BM * k; i += MDE_BLOCK) {
    bestd[i] = 3.402823466e+38f;
    besti[i] = -1;
  }
  float worst_d = 3.402823466e+38f;
  int worst_i = -1;
  for (int s = 0; s < slices; ++s) {
    const int64_t base = ((int64_t)s * n_q + row0) * k;
    __syncthreads();
    for (int i = tid; i < rows * k; i += MDE_BLOCK) {
      sd[i] = pd[base + i];
      si[i] = pi[base + i];
    }
    __syncthreads();
    if (tid < rows)
      mde_topk_merge_id(sd + tid * k, si + tid * k, k, k, bestd + tid * k, besti + tid * k, worst_d, worst_i);
  }
  __syncthreads();
  for (int i = tid; i < rows * k; i += MDE_BLOCK) {
    idx_out[row0 * k + i] = besti[i];
    d2_out[row0 * k + i] = bestd[i];
  }
}

// The automatic slice count (slices == 0).  Rule: when the query blocks alone give every CU a workgroup
// (query blocks >= CUs) the corpus is not split; otherwise it is split so that the grid holds about
// CROSS_GRID_PER_CU workgroups per CU, but no finer than CROSS_MIN_TILES 64-column tiles per slice (a
// slice must amortise its list's k entries of merge work and its start-up).  Both constants are
// unmeasured choices until tools/cross_knn_scale.py has run on the device (profiles/r09_cross_knn.txt).
#define CROSS_GRID_PER_CU 4
#define CROSS_MIN_TILES 16
#define CROSS_MAX_SLICES 65535   // gridDim.y
static int cross_cu_count(int* cus) {
  static int cached[64];         // per device ordinal; 0 = not asked yet
  int dev = 0;
  MDE_HIP(hipGetDevice(&dev));
  const bool slot = dev >= 0 && dev < 64;
  if (slot && cached[dev] > 0) {
    *cus = cached[dev];
    return MDE_OK;
  }
  hipDeviceProp_t prop;
  MDE_HIP(hipGetDeviceProperties(&prop, dev));
  *cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 1;
  if (slot) cached[dev] = *cus;
  return MDE_OK;
}
static int64_t cross_auto_slices(int64_t n_q, int64_t n_c, int cus) {
  const int64_t qb = (n_q + KNN_BM - 1) / KNN_BM, tiles = (n_c + KNN_BN - 1) / KNN_BN;
  if (qb >= cus) return 1;
  int64_t s = ((int64_t)CROSS_GRID_PER_CU * cus + qb - 1) / qb;
  if (s > tiles / CROSS_MIN_TILES) s = tiles / CROSS_MIN_TILES;
  if (s > CROSS_MAX_SLICES) s = CROSS_MAX_SLICES;
  return s < 1 ? 1 : s;
}
// slices as given, or the automatic count for 0; a negative MDE_E_* code on failure
static int64_t cross_resolve_slices(int64_t n_q, int64_t n_c, int32_t slices) {
  if (slices != 0) return slices;
  int cus = 0;
  const int rc = cross_cu_count(&cus);
  if (rc != MDE_OK) return rc;
  return cross_auto_slices(n_q, n_c, cus);
}
static bool cross_args_ok(int64_t n_q, int64_t n_c, int32_t k, int32_t slices) {
  return n_q > 0 && n_c > 0 && k > 0 && k <= KNN_MAXK && slices >= 0 && slices <= CROSS_MAX_SLICES;
}

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
  const size_t lds = sizeof(float) * (size_t)(KNN_BM * KNN_KBP + KNN_BN * KNN_KBP + KNN_BM * (KNN_BN + 1)) +
                     (size_t)KNN_BM * k * (sizeof(float) + sizeof(int));
  const size_t lds_merge = (size_t)KNN_BM * k * 2 * (sizeof(float) + sizeof(int));
  static bool attr = false;
  if (!attr) {
    MDE_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k_knn_cross),
                                hipFuncAttributeMaxDynamicSharedMemorySize, 96 * 1024));
    MDE_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k_knn_cross_merge),
                                hipFuncAttributeMaxDynamicSharedMemorySize, 96 * 1024));
    attr = true;
  }
  const int64_t tiles = (n_c + KNN_BN - 1) / KNN_BN;
  const int64_t slice_cols = ((tiles + s - 1) / s) * KNN_BN;    // whole tiles; the last slices may be short or empty
  const unsigned qb = (unsigned)((n_q + KNN_BM - 1) / KNN_BM);
  hipLaunchKernelGGL(k_knn_cross, dim3(qb, (unsigned)s), dim3(MDE_BLOCK), lds, st, (int)n_q, (int)n_c, nf, k,
                     slice_cols, Q, C, qn, cn, s > 1 ? pi : idx_out, s > 1 ? pd : d2_out);
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

// mde_spmm.hip -- C = A B - u v^T for a CSR A [n, nf] and a tall thin dense B [nf, r], 1 <= r <= 256: the
// product behind the sparse principal components (pymde_amd/pca.py).  The rank-one term
// centres a sparse matrix without densifying it: (A - 1 mu^T) B = A B - 1 (mu^T B), and with the transposed
// CSR (A - 1 mu^T)^T Q = A^T Q - mu (1^T Q).
//
// Arithmetic.  Every product and sum is float64, a row's entries in ascending column order; u[i] v[c] is
// subtracted in float64 and the result is rounded to float32 once, at the store.  The kernel is bound by the
// gathers of B rows (4 r bytes per stored entry), not by the fp64 FMA, and the float64 sum keeps the
// cancellation of A B - 1 (mu^T B) harmless.  No atomics: the same bits on every run.
//
// Work split.  The stored entries are cut into windows of SPMM_L consecutive positions of the CSR arrays,
// one wave per window, so the work of a wave is bounded whatever the row lengths are (the transpose of a
// cells x genes matrix has rows of up to n entries).  A row longer than SPMM_L is cut into segments of SPMM_L
// of its own entries.  The wave of window g = [g L, (g + 1) L) handles
//   * every row whose first position lies in the window (empty rows included; the rows that start at nnz go
//     to the last window): a row of at most L entries is finished and stored, of a longer row segment 0 is
//     summed into the partial P0[g];
//   * the one segment s >= 1 of the row that runs across the window's first position, if that segment starts
//     inside the window: summed into the partial P1[g].
// Segments start L positions apart and a long row is longer than L, so a window sees at most one of each
// kind, and `work` is two float64 [r] slots per window.  k_spmm_finish then visits every row and, for a long
// one, adds P0 and its P1 slots in segment order, subtracts, rounds and stores.
//
// Lanes.  The lanes of a wave own the columns c = lane, lane + 64, ... of r (NCH = ceil(r / 64) register
// accumulators), so one entry reads its B row as contiguous 256-byte pieces.  A row's indices / values are
// the same for every lane: 64 of them are loaded across the lanes with one coalesced load each and handed
// out by v_readlane, which leaves the column id in an SGPR and the gather as scalar base + lane offset; four
// entries' gathers are issued before the first FMA.  The row pointers of a window's rows are loaded and
// handed out the same way, so a window of many short rows does not pay one dependent load per row.
#include "mde_common.h"

#define SPMM_L 1024      // entries per segment / positions per window
#define SPMM_MAX_R 256

__device__ __forceinline__ int64_t spmm_readlane64(int64_t v, int l) {
  const int lo = __builtin_amdgcn_readlane((int)(uint32_t)(uint64_t)v, l);
  const int hi = __builtin_amdgcn_readlane((int)((uint64_t)v >> 32), l);
  return (int64_t)(((uint64_t)(uint32_t)hi << 32) | (uint32_t)lo);
}
__device__ __forceinline__ int64_t spmm_uniform64(int64_t v) { return spmm_readlane64(v, 0); }

// first i in [0, n] with indptr[i] >= p (indptr non-decreasing, indptr[n] = nnz; n + 1 when p > nnz)
__device__ __forceinline__ int64_t spmm_first_row_at(const int64_t* __restrict__ indptr, int64_t n, int64_t p) {
  int64_t lo = 0, hi = n + 1;
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (indptr[mid] < p) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// acc[j] += sum over the entries e in [a, b) of values[e] * B[indices[e], lane + 64 j], in ascending e
template <int NCH>
__device__ __forceinline__ void spmm_accumulate(int64_t a, int64_t b, const int32_t* __restrict__ indices,
                                                const float* __restrict__ values, const float* __restrict__ B,
                                                int r, int lane, double (&acc)[NCH]) {
  for (int64_t e0 = a; e0 < b; e0 += 64) {
    const int64_t e = e0 + lane;
    const int col = e < b ? indices[e] : 0;
    const float val = e < b ? values[e] : 0.0f;
    const int m = (int)(b - e0 < 64 ? b - e0 : 64);
    int t = 0;
    for (; t + 4 <= m; t += 4) {
      float x[4][NCH];
      float w[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const float* row = B + (int64_t)__builtin_amdgcn_readlane(col, t + q) * r;
        w[q] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(val), t + q));
#pragma unroll
        for (int j = 0; j < NCH; ++j) x[q][j] = (lane + 64 * j < r) ? row[lane + 64 * j] : 0.0f;
      }
#pragma unroll
      for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int j = 0; j < NCH; ++j) acc[j] = fma((double)w[q], (double)x[q][j], acc[j]);
    }
    for (; t < m; ++t) {
      const float* row = B + (int64_t)__builtin_amdgcn_readlane(col, t) * r;
      const double w = (double)__int_as_float(__builtin_amdgcn_readlane(__float_as_int(val), t));
#pragma unroll
      for (int j = 0; j < NCH; ++j)
        if (lane + 64 * j < r) acc[j] = fma(w, (double)row[lane + 64 * j], acc[j]);
    }
  }
}

// C[i, c] = (float)(acc - u[i] v[c])
template <int NCH>
__device__ __forceinline__ void spmm_store_row(int64_t i, int r, int lane, const double (&acc)[NCH],
                                               const float* __restrict__ u, const double* __restrict__ v,
                                               float* __restrict__ C) {
  const double ui = (v && u) ? (double)u[i] : 1.0;
#pragma unroll
  for (int j = 0; j < NCH; ++j) {
    const int c = lane + 64 * j;
    if (c < r) C[i * r + c] = (float)(v ? acc[j] - ui * v[c] : acc[j]);
  }
}

template <int NCH>
__device__ __forceinline__ void spmm_store_partial(double* __restrict__ slot, int r, int lane,
                                                   const double (&acc)[NCH]) {
#pragma unroll
  for (int j = 0; j < NCH; ++j)
    if (lane + 64 * j < r) slot[lane + 64 * j] = acc[j];
}

template <int NCH>
__global__ __launch_bounds__(MDE_BLOCK) void k_spmm_windows(int64_t n, int64_t nnz, int64_t n_windows, int r,
                                                            const int64_t* __restrict__ indptr,
                                                            const int32_t* __restrict__ indices,
                                                            const float* __restrict__ values,
                                                            const float* __restrict__ B,
                                                            const float* __restrict__ u,
                                                            const double* __restrict__ v, float* __restrict__ C,
                                                            double* __restrict__ P0, double* __restrict__ P1) {
  const int lane = threadIdx.x & 63;
  const int64_t g = spmm_uniform64(((int64_t)blockIdx.x * MDE_BLOCK + threadIdx.x) >> 6);
  if (g >= n_windows) return;
  const int64_t p0 = g * SPMM_L;
  const int64_t row_first = spmm_uniform64(spmm_first_row_at(indptr, n, p0));
  // the rows that start in the window; the last window also takes the (empty) rows that start at nnz
  const int64_t row_end = g == n_windows - 1 ? n : spmm_uniform64(spmm_first_row_at(indptr, n, p0 + SPMM_L));
  double acc[NCH];
  // (1) the segment s >= 1 of the row that runs across p0
  if (row_first > 0 && row_first <= n) {
    const int64_t lo = spmm_uniform64(indptr[row_first - 1]), hi = spmm_uniform64(indptr[row_first]);
    const int64_t start = lo + (p0 - lo + SPMM_L - 1) / SPMM_L * SPMM_L;     // in [p0, p0 + L)
    if (hi - lo > SPMM_L && start < hi) {
#pragma unroll
      for (int j = 0; j < NCH; ++j) acc[j] = 0.0;
      spmm_accumulate<NCH>(start, hi - start < SPMM_L ? hi : start + SPMM_L, indices, values, B, r, lane, acc);
      spmm_store_partial<NCH>(P1 + g * r, r, lane, acc);
    }
  }
  // (2) the rows that start in the window, their pointers 64 at a time
  for (int64_t i0 = row_first; i0 < row_end; i0 += 64) {
    const int cnt = (int)(row_end - i0 < 64 ? row_end - i0 : 64);
    const int64_t plo = lane < cnt ? indptr[i0 + lane] : 0, phi = lane < cnt ? indptr[i0 + lane + 1] : 0;
    for (int t = 0; t < cnt; ++t) {
      const int64_t lo = spmm_readlane64(plo, t), hi = spmm_readlane64(phi, t);
#pragma unroll
      for (int j = 0; j < NCH; ++j) acc[j] = 0.0;
      if (hi - lo > SPMM_L) {
        spmm_accumulate<NCH>(lo, lo + SPMM_L, indices, values, B, r, lane, acc);
        spmm_store_partial<NCH>(P0 + g * r, r, lane, acc);
      } else {
        spmm_accumulate<NCH>(lo, hi, indices, values, B, r, lane, acc);
        spmm_store_row<NCH>(i0 + t, r, lane, acc, u, v, C);
      }
    }
  }
}

// the rows longer than SPMM_L: segment 0 from P0, segments 1, 2, ... from P1, added in that order
template <int NCH>
__global__ __launch_bounds__(MDE_BLOCK) void k_spmm_finish(int64_t n, int r, const int64_t* __restrict__ indptr,
                                                           const float* __restrict__ u,
                                                           const double* __restrict__ v, float* __restrict__ C,
                                                           const double* __restrict__ P0,
                                                           const double* __restrict__ P1) {
  const int lane = threadIdx.x & 63;
  const int64_t w0 = ((int64_t)blockIdx.x * MDE_BLOCK + threadIdx.x) >> 6;
  const int64_t nw = ((int64_t)gridDim.x * MDE_BLOCK) >> 6;
  for (int64_t i = w0; i < n; i += nw) {
    const int64_t lo = indptr[i], hi = indptr[i + 1];
    if (hi - lo <= SPMM_L) continue;
    double acc[NCH];
#pragma unroll
    for (int j = 0; j < NCH; ++j) acc[j] = (lane + 64 * j < r) ? P0[lo / SPMM_L * r + lane + 64 * j] : 0.0;
    for (int64_t start = lo + SPMM_L; start < hi; start += SPMM_L) {
      const double* slot = P1 + start / SPMM_L * r;
#pragma unroll
      for (int j = 0; j < NCH; ++j)
        if (lane + 64 * j < r) acc[j] += slot[lane + 64 * j];
    }
    spmm_store_row<NCH>(i, r, lane, acc, u, v, C);
  }
}

extern "C" int32_t mde_csr_spmm_segment(void) { return SPMM_L; }

static inline int64_t spmm_windows(int64_t nnz) { return nnz / SPMM_L + 1; }

extern "C" int64_t mde_csr_spmm_work_bytes(int64_t n, int64_t nnz, int32_t r) {
  if (n <= 0 || nnz < 0 || r < 1 || r > SPMM_MAX_R) {
    mde_set_error("mde_csr_spmm_work_bytes: invalid arguments (n >= 1, nnz >= 0, 1 <= r <= %d)", SPMM_MAX_R);
    return MDE_E_INVALID;
  }
  return 2 * spmm_windows(nnz) * (int64_t)r * (int64_t)sizeof(double);
}

template <int NCH>
static int spmm_launch(int64_t n, int64_t nnz, int r, const int64_t* indptr, const int32_t* indices,
                       const float* values, const float* B, const float* u, const double* v, float* C,
                       double* work, hipStream_t st) {
  const int64_t nwin = spmm_windows(nnz);
  double* P0 = work;
  double* P1 = work + nwin * r;
  hipLaunchKernelGGL((k_spmm_windows<NCH>), dim3((unsigned)((nwin + 3) / 4)), dim3(MDE_BLOCK), 0, st, n, nnz, nwin,
                     r, indptr, indices, values, B, u, v, C, P0, P1);
  MDE_LAUNCH_CHECK();
  if (nnz > SPMM_L) {   // (no row can be longer than L otherwise)
    hipLaunchKernelGGL((k_spmm_finish<NCH>), dim3(mde_grid(n * 64, MDE_BLOCK, 4096)), dim3(MDE_BLOCK), 0, st, n, r,
                       indptr, u, v, C, P0, P1);
    MDE_LAUNCH_CHECK();
  }
  return MDE_OK;
}

extern "C" int mde_csr_spmm(int64_t n, int32_t nf, int64_t nnz, const int64_t* indptr, const int32_t* indices,
                            const float* values, int32_t r, const float* B, const float* u, const double* v,
                            float* C, void* work, void* stream) {
  if (r < 1 || r > SPMM_MAX_R) {
    mde_set_error("mde_csr_spmm: r must lie in [1, %d] (got %d)", SPMM_MAX_R, (int)r);
    return MDE_E_INVALID;
  }
  if (n <= 0 || nf <= 0 || nnz < 0 || !indptr || (nnz > 0 && (!indices || !values)) || !B || !C || !work) {
    mde_set_error("mde_csr_spmm: invalid arguments (n >= 1, nf >= 1, nnz >= 0, non-null indptr / indices / "
                  "values / B / C / work)");
    return MDE_E_INVALID;
  }
  if (n >= ((int64_t)1 << 31)) {
    mde_set_error("mde_csr_spmm: n must be below 2^31");
    return MDE_E_TOO_LARGE;
  }
  hipStream_t st = mde_stream(stream);
  double* w = static_cast<double*>(work);
  switch ((r + 63) / 64) {
    case 1: return spmm_launch<1>(n, nnz, r, indptr, indices, values, B, u, v, C, w, st);
    case 2: return spmm_launch<2>(n, nnz, r, indptr, indices, values, B, u, v, C, w, st);
    case 3: return spmm_launch<3>(n, nnz, r, indptr, indices, values, B, u, v, C, w, st);
    default: return spmm_launch<4>(n, nnz, r, indptr, indices, values, B, u, v, C, w, st);
  }
}

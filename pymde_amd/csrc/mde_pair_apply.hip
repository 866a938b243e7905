// mde_pair_apply.hip -- the product of the matrix of SQUARED deviations with a thin block of vectors (DESIGN section
// 6p): what classical (Torgerson) scaling and the distance-based triangulation of pymde_amd.classical are made of.
// The matrix S is never stored.
//
//   out[i][k] = sum_j S(i, j) V[j][k]        i < n_q, j < n_c, k < r, 1 <= r <= 32
//
// V float32 [n_c, r], out DOUBLE [n_q, r] (the host subtracts large rank-one terms from it).  S(i, j) comes from one
// of the two sources of the rectangular loss walk (mde_pair_loss.hip):
//   Gram     the 64x64 Gram tile of Q [n_q, nf] against C [n_c, nf] (mde_knn_tile.h), parked as squared distances
//            d2 = fmaxf(|x|^2 + |y|^2 - 2 x.y, 0):  mode 0  S = d2 as it is (never sqrtf and squared again),
//                                                  mode 1  S = (0.5f d2)^2, the product formed in double;
//   matrix   a 64x64 tile of a row-major float32 [n_q, n_c] matrix, read as mde_pair_loss reads it (a wave reads
//            whole 256-byte row segments): S = Dm[i][j]^2 formed in double, so the square is exact.
// skip_diagonal leaves out j == i BY INDEX (n_q == n_c): a duplicate row elsewhere is an ordinary pair, and neither a
// non-zero Dm[i][i] nor the rounding noise of d2(i, i) counts.
//
//   k_pair_apply_walk<RW, MATRIX>  the grid of k_pair_loss_walk: workgroup (x, y) owns 64 rows and the column tiles of
//                      slice y.  Per tile the S side is parked in sD and the 64 rows of V are staged as DOUBLES,
//                      [64][RW] with RW = r padded with zero columns to 8, 16 or 32 (compiled in: the RW accumulators
//                      stay in registers); thread t owns tile row t & 63 and the 16 columns 16 (t >> 6) ...: the
//                      lanes of a wave read the same staged row of V (a broadcast) and 64 rows of sD at stride 65
//                      (conflict-free).  One fma in double per (pair, k).  The four threads of a row are combined
//                      in thread order through LDS.  No floating-point atomics.
//   k_pair_apply_fold  adds the per-slice partials in slice order.
// For a given slice count `out` is the same bits on every run, and a row's result does not depend on which other rows
// share its block.
#include "mde_pair.h"

#define PAIR_APPLY_MAX_R 32

template <int RW, bool MATRIX>
__global__ __launch_bounds__(MDE_BLOCK) void k_pair_apply_walk(int n_q, int n_c, int nf, int mode, int skip, int r,
                                                               int64_t slice_cols, const float* __restrict__ Q,
                                                               const float* __restrict__ qn,
                                                               const float* __restrict__ C,
                                                               const float* __restrict__ cn,
                                                               const float* __restrict__ Dm,
                                                               const float* __restrict__ V,
                                                               double* __restrict__ part) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const knn_tile_lds s = knn_tile_carve(lds, 0, 2 * KNN_BN * RW);
  double* sV = reinterpret_cast<double*>(s.extra);              // [KNN_BN][RW]; starts at a multiple of 16 bytes
  const int tid = threadIdx.x, row = tid & 63, w = tid >> 6;
  const int64_t row0 = (int64_t)blockIdx.x * KNN_BM;
  const int64_t lo = (int64_t)blockIdx.y * slice_cols;
  const int64_t c_lo = lo < n_c ? lo : n_c, c_hi = lo + slice_cols < n_c ? lo + slice_cols : n_c;
  const float* arow[KNN_STG];
  bool qok[KNN_STG];
  if constexpr (!MATRIX) {
#pragma unroll
    for (int q = 0; q < KNN_STG; ++q) {
      const int64_t gr = row0 + (tid >> 5) + 8 * q;
      qok[q] = gr < n_q;
      arow[q] = Q + (qok[q] ? gr : 0) * nf;
    }
  }
  double acc[RW];
#pragma unroll
  for (int k = 0; k < RW; ++k) acc[k] = 0.0;
  for (int64_t col0 = c_lo; col0 < c_hi; col0 += KNN_BN) {
    auto keep = [&](int rr, int cc) {
      return row0 + rr < n_q && col0 + cc < n_c && (!skip || row0 + rr != col0 + cc);
    };
    if constexpr (MATRIX) {
      // wave w takes the tile rows w, w + 4, ...: all sixteen loads go out from clamped addresses before the first
      // is used; what the tile does not have (or the diagonal) is replaced when the registers are parked
      const int lane = tid & 63;
      const int64_t gc = col0 + lane < n_c ? col0 + lane : n_c - 1;
      float v[KNN_BM / 4];
#pragma unroll
      for (int q = 0; q < KNN_BM / 4; ++q) {
        const int64_t gr = row0 + w + 4 * q < n_q ? row0 + w + 4 * q : n_q - 1;
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
      const f32x16 g = knn_gram_tile(s.sA, s.sB, nf, arow, qok, acol, cok);
      knn_park_tile(s.sD, g, keep, [&](int rr) { return qn[row0 + rr]; }, [&](int cc) { return cn[col0 + cc]; });
    }
    // (sV: the walk of the last tile ended before the barrier above, or before those of the Gram tile)
    for (int i = tid; i < KNN_BN * RW; i += MDE_BLOCK) {
      const int c = i / RW, k = i - c * RW;
      sV[i] = (col0 + c < n_c && k < r) ? (double)V[(col0 + c) * r + k] : 0.0;
    }
    __syncthreads();
    const float* pd = s.sD + row * (KNN_BN + 1) + w * PAIR_COLS;
    const double* pv = sV + w * PAIR_COLS * RW;
#pragma unroll 2
    for (int cc = 0; cc < PAIR_COLS; ++cc) {
      const float v = pd[cc];
      double S = 0.0;                                           // what keep() refused is parked as FLT_MAX: adds 0.0
      if (v != PAIR_FLT_MAX) {
        if (MATRIX) {
          S = (double)v * (double)v;
        } else if (mode) {
          const float h = 0.5f * v;
          S = (double)h * (double)h;
        } else {
          S = (double)v;
        }
      }
#pragma unroll
      for (int k = 0; k < RW; ++k) acc[k] = fma(S, pv[cc * RW + k], acc[k]);
    }
  }
  // the four threads of a row in thread order: ((p0 + p1) + p2) + p3, through one [RW][KNN_BM] block of doubles in
  // the place of sV (column-major: the 64 lanes of a wave touch 64 consecutive doubles)
  double* cs = sV;
  for (int u = 0; u < 4; ++u) {
    __syncthreads();                                            // u == 0: the last walk is over
    if (w == u) {
      if (u == 0) {
#pragma unroll
        for (int k = 0; k < RW; ++k) cs[k * KNN_BM + row] = acc[k];
      } else if (u < 3) {
#pragma unroll
        for (int k = 0; k < RW; ++k) cs[k * KNN_BM + row] += acc[k];
      } else if (row0 + row < n_q) {
        double* dst = part + ((int64_t)blockIdx.y * n_q + row0 + row) * r;
#pragma unroll
        for (int k = 0; k < RW; ++k)
          if (k < r) dst[k] = cs[k * KNN_BM + row] + acc[k];
      }
    }
  }
}

// out[i] = the sum over the slices, in slice order, of part[y][i]
__global__ __launch_bounds__(MDE_BLOCK) void k_pair_apply_fold(int64_t total, int slices,
                                                               const double* __restrict__ part,
                                                               double* __restrict__ out) {
  for (int64_t i = (int64_t)blockIdx.x * MDE_BLOCK + threadIdx.x; i < total; i += (int64_t)gridDim.x * MDE_BLOCK) {
    double t = 0.0;
    for (int y = 0; y < slices; ++y) t += part[(int64_t)y * total + i];
    out[i] = t;
  }
}

static bool pair_apply_sizes_ok(int64_t n_q, int64_t n_c, int32_t r, int32_t slices) {
  return n_q >= 1 && n_q < ((int64_t)1 << 31) && n_c >= 1 && n_c < ((int64_t)1 << 31) && r >= 1 &&
         r <= PAIR_APPLY_MAX_R && slices >= 0 && slices <= CROSS_MAX_SLICES;
}

// work: [s, n_q, r] doubles (s > 1) | the row norms of Q, [n_q] floats | the row norms of C, [n_c] floats
extern "C" int64_t mde_pair_sqdist_apply_work_bytes(int64_t n_q, int64_t n_c, int32_t r, int32_t slices) {
  if (!pair_apply_sizes_ok(n_q, n_c, r, slices)) {
    mde_set_error("mde_pair_sqdist_apply_work_bytes: invalid arguments (1 <= n_q, n_c < 2^31, 1 <= r <= %d, 0 <= "
                  "slices <= %d)", PAIR_APPLY_MAX_R, CROSS_MAX_SLICES);
    return MDE_E_INVALID;
  }
  const int64_t s = cross_resolve_slices(n_q, n_c, slices);
  if (s < 0) return s;
  return (s > 1 ? s * n_q * r * 8 : 0) + 4 * (n_q + n_c);
}

using PairApplyKernel = decltype(&k_pair_apply_walk<8, false>);

extern "C" int mde_pair_sqdist_apply(int64_t n_q, int64_t n_c, int32_t nf, const float* Q, const float* C,
                                     int32_t mode, const float* Dm, int32_t skip_diagonal, int32_t r, const float* V,
                                     int32_t slices, double* out, void* work, void* stream) {
  static const PairApplyKernel kernels[2][3] = {
      {k_pair_apply_walk<8, false>, k_pair_apply_walk<16, false>, k_pair_apply_walk<32, false>},
      {k_pair_apply_walk<8, true>, k_pair_apply_walk<16, true>, k_pair_apply_walk<32, true>}};
  const bool gram = Q != nullptr && C != nullptr && Dm == nullptr;
  const bool matrix = Q == nullptr && C == nullptr && Dm != nullptr;
  const bool source_ok = matrix || (gram && nf >= 1 && (mode == 0 || mode == 1));
  if (!pair_apply_sizes_ok(n_q, n_c, r, slices) || !source_ok || (skip_diagonal != 0 && n_q != n_c) || !V || !out ||
      !work) {
    mde_set_error("mde_pair_sqdist_apply: invalid arguments (1 <= n_q, n_c < 2^31, 1 <= r <= %d, either both Q and C "
                  "(nf >= 1, mode 0 / 1) or Dm alone, skip_diagonal only with n_q == n_c, 0 <= slices <= %d, non-null "
                  "V / out / work)", PAIR_APPLY_MAX_R, CROSS_MAX_SLICES);
    return MDE_E_INVALID;
  }
  const int64_t s = cross_resolve_slices(n_q, n_c, slices);
  if (s < 0) return (int)s;
  double* part = static_cast<double*>(work);
  float* qn = reinterpret_cast<float*>(part + (s > 1 ? s * n_q * r : 0));
  float* cn = qn + n_q;
  if (gram) {
    int rc = mde_row_sqnorm(n_q, nf, Q, qn, stream);
    if (rc == MDE_OK) rc = mde_row_sqnorm(n_c, nf, C, cn, stream);
    if (rc != MDE_OK) return rc;
  }
  hipStream_t st = mde_stream(stream);
  const int64_t tiles = (n_c + KNN_BN - 1) / KNN_BN;
  const int64_t slice_cols = ((tiles + s - 1) / s) * KNN_BN;     // whole tiles; the last slices may be short or empty
  const dim3 grid((unsigned)((n_q + KNN_BM - 1) / KNN_BM), (unsigned)s);
  const int width = r <= 8 ? 0 : r <= 16 ? 1 : 2;                // RW = r padded to 8, 16 or 32
  const int rw = 8 << width;
  hipLaunchKernelGGL(kernels[matrix][width], grid, dim3(MDE_BLOCK), knn_tile_lds_bytes(0, 2 * KNN_BN * rw), st,
                     (int)n_q, (int)n_c, nf, mode, skip_diagonal != 0 ? 1 : 0, r, slice_cols, Q, qn, C, cn, Dm, V,
                     s > 1 ? part : out);
  MDE_LAUNCH_CHECK();
  if (s > 1) {
    hipLaunchKernelGGL(k_pair_apply_fold, dim3(mde_grid(n_q * r, MDE_BLOCK, 4096)), dim3(MDE_BLOCK), 0, st, n_q * r,
                       (int)s, part, out);
    MDE_LAUNCH_CHECK();
  }
  return MDE_OK;
}

// mde_std.hip -- the Standardized constraint's kernels: small Gram matrices (f32 MFMA when the widths
// allow), right-multiply, row scale / shift, the tangent projection, C^{-1/2} and the retraction (the
// other solver units: mde_solver.h).
//   [ref: pymde/constraints.py:94-200, pymde/util.py:129-171]
#include "mde_solver.h"

#include <algorithm>
#include <cmath>

typedef float f32x16 __attribute__((ext_vector_type(16)));

// ---------------------------------------------------------------- Gram matrices  out = A^T B
// (a) tiny widths: one thread per row, da*db register accumulators in double
template <int DA, int DB>
__global__ __launch_bounds__(MDE_BLOCK) void k_gram_tiny(int64_t n, const float* __restrict__ A,
                                                         const float* __restrict__ B,
                                                         double* __restrict__ partial /*[m][nb]*/,
                                                         double* __restrict__ out, unsigned int* ticket) {
  __shared__ double smem[8];
  double acc[DA * DB];
#pragma unroll
  for (int i = 0; i < DA * DB; ++i) acc[i] = 0.0;
  for (int64_t r = (int64_t)blockIdx.x * MDE_BLOCK + threadIdx.x; r < n;
       r += (int64_t)gridDim.x * MDE_BLOCK) {
    double a[DA], b[DB];
#pragma unroll
    for (int i = 0; i < DA; ++i) a[i] = A[r * DA + i];
#pragma unroll
    for (int j = 0; j < DB; ++j) b[j] = B[r * DB + j];
#pragma unroll
    for (int i = 0; i < DA; ++i)
#pragma unroll
      for (int j = 0; j < DB; ++j) acc[i * DB + j] = fma(a[i], b[j], acc[i * DB + j]);
  }
#pragma unroll
  for (int q = 0; q < DA * DB; ++q) {
    const double r = mde_block_sum(acc[q], smem);
    if (threadIdx.x == 0) mde_st_partial(partial + (int64_t)q * gridDim.x + blockIdx.x, r);
  }
  // the last workgroup to arrive adds the partials (one wave per entry, fixed order)
  if (!mde_last_block(ticket)) return;
  mde_final_rows(DA * DB, gridDim.x, partial, out, 0ull);
}

// (b) any widths: 16x16 output tile per block, rows split into chunks (grid.y)
__global__ __launch_bounds__(MDE_BLOCK) void k_gram_generic(int64_t n, int da, int db,
                                                            const float* __restrict__ A,
                                                            const float* __restrict__ B,
                                                            int64_t rows_per_chunk, int tiles_j,
                                                            double* __restrict__ partial /*[m][nc]*/) {
  const int ti = blockIdx.x / tiles_j, tj = blockIdx.x % tiles_j;
  const int i = ti * 16 + (threadIdx.x >> 4), j = tj * 16 + (threadIdx.x & 15);
  const int64_t r0 = (int64_t)blockIdx.y * rows_per_chunk;
  int64_t r1 = r0 + rows_per_chunk;
  if (r1 > n) r1 = n;
  double acc = 0.0;
  if (i < da && j < db)
    for (int64_t r = r0; r < r1; ++r) acc = fma((double)A[r * da + i], (double)B[r * db + j], acc);
  if (i < da && j < db) partial[((int64_t)i * db + j) * gridDim.y + blockIdx.y] = acc;
}

// (c) widths that are multiples of 32: f32 MFMA (v_mfma_f32_32x32x2_f32), one 32x32 output tile
// per wave, k = rows of the chunk.  A-operand lane l: A[r + (l>>5)][ti*32 + (l&31)], B alike:
// both are fully coalesced 128-byte row segments.  C/D map: col = l&31,
// row = (reg&3) + 8*(reg>>2) + 4*(l>>5).  Accumulates in f32 over <= 4096 rows per chunk, the
// chunk partials are then summed in double.
__global__ __launch_bounds__(MDE_BLOCK) void k_gram_mfma(int64_t n, int da, int db,
                                                         const float* __restrict__ A,
                                                         const float* __restrict__ B,
                                                         int64_t rows_per_chunk, int tiles_j,
                                                         int ntiles,
                                                         double* __restrict__ partial /*[m][nc]*/) {
  const int lane = threadIdx.x & 63;
  const int tile = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (tile >= ntiles) return;
  const int ti = tile / tiles_j, tj = tile % tiles_j;
  const int64_t r0 = (int64_t)blockIdx.y * rows_per_chunk;
  int64_t r1 = r0 + rows_per_chunk;
  if (r1 > n) r1 = n;
  const int kk = lane >> 5, cc = lane & 31;
  const float* pa = A + (int64_t)ti * 32 + cc;
  const float* pb = B + (int64_t)tj * 32 + cc;
  f32x16 acc;
#pragma unroll
  for (int q = 0; q < 16; ++q) acc[q] = 0.0f;
  for (int64_t r = r0; r < r1; r += 2) {
    const int64_t rr = r + kk;
    const bool ok = rr < r1;
    const float a = ok ? pa[rr * da] : 0.0f;
    const float b = ok ? pb[rr * db] : 0.0f;
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc, 0, 0, 0);
  }
#pragma unroll
  for (int q = 0; q < 16; ++q) {
    const int row = (q & 3) + 8 * (q >> 2) + 4 * kk;
    const int i = ti * 32 + row, j = tj * 32 + cc;
    partial[((int64_t)i * db + j) * gridDim.y + blockIdx.y] = (double)acc[q];
  }
}

// out[q] = sum_c partial[q * nc + c]: one wave per output entry (small outputs; a serial loop per
// entry is latency-bound) or one thread per entry (large outputs)
__global__ __launch_bounds__(64) void k_gram_final_wave(int nc, const double* __restrict__ partial,
                                                        double* __restrict__ out) {
  const int64_t q = blockIdx.x;
  double s = 0.0;
  for (int c = threadIdx.x; c < nc; c += 64) s += partial[q * nc + c];
  s = mde_wave_sum(s);
  if (threadIdx.x == 0) out[q] = s;
}
__global__ void k_gram_final(int64_t m, int nc, const double* __restrict__ partial,
                             double* __restrict__ out) {
  for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < m;
       q += (int64_t)gridDim.x * blockDim.x) {
    double s = 0.0;
    for (int c = 0; c < nc; ++c) s += partial[q * nc + c];
    out[q] = s;
  }
}

static int g_no_mfma = -1;
static int gram_impl(int64_t n, int da, int db, const float* A, const float* B, double* out,
                     double* partial, unsigned int* ticket, hipStream_t st) {
  const int64_t m = (int64_t)da * db;
  if (g_no_mfma < 0) {
    const char* e = getenv("MDE_NO_MFMA");
    g_no_mfma = (e && atoi(e)) ? 1 : 0;
  }
#define TINY(DA_, DB_)                                                                              \
  if (da == DA_ && db == DB_) {                                                                     \
    const int nb = mde_grid(n, MDE_BLOCK * 2, MDE_RED_BLOCKS);                                      \
    hipLaunchKernelGGL((k_gram_tiny<DA_, DB_>), dim3(nb), dim3(MDE_BLOCK), 0, st, n, A, B, partial,  \
                       out, ticket);                                                                \
    MDE_LAUNCH_CHECK();                                                                             \
    return MDE_OK;                                                                                  \
  }
  TINY(1, 1) TINY(2, 2) TINY(3, 3) TINY(4, 4)
#undef TINY
  // chunking: as many row chunks as the partial area holds, at most 256, >= 2 rows each
  int64_t nc = MDE_PARTIAL_DOUBLES / m;
  if (nc > 256) nc = 256;
  if (nc < 1) {
    mde_set_error("gram: %d x %d output does not fit the work buffer", da, db);
    return MDE_E_UNSUPPORTED;
  }
  int64_t rpc = (n + nc - 1) / nc;
  if (rpc < 64) rpc = 64;
  const bool mfma = !g_no_mfma && (da % 32 == 0) && (db % 32 == 0);
  if (mfma) {
    if (rpc > 4096) rpc = 4096;  // bound the f32 accumulation length
    rpc = (rpc + 1) & ~(int64_t)1;
  }
  nc = (n + rpc - 1) / rpc;
  if (mfma && nc * m > MDE_PARTIAL_DOUBLES) {
    // too many chunks for the partial area: lengthen chunks
    nc = MDE_PARTIAL_DOUBLES / m;
    rpc = ((n + nc - 1) / nc + 1) & ~(int64_t)1;
    nc = (n + rpc - 1) / rpc;
  }
  if (mfma) {
    const int tiles_j = db / 32, ntiles = (da / 32) * tiles_j;
    hipLaunchKernelGGL(k_gram_mfma, dim3((ntiles + 3) / 4, (unsigned)nc), dim3(MDE_BLOCK), 0, st, n, da,
                       db, A, B, rpc, tiles_j, ntiles, partial);
  } else {
    const int tiles_i = (da + 15) / 16, tiles_j = (db + 15) / 16;
    hipLaunchKernelGGL(k_gram_generic, dim3(tiles_i * tiles_j, (unsigned)nc), dim3(MDE_BLOCK), 0, st, n,
                       da, db, A, B, rpc, tiles_j, partial);
  }
  MDE_LAUNCH_CHECK();
  if (m <= 65536)
    hipLaunchKernelGGL(k_gram_final_wave, dim3((unsigned)m), dim3(64), 0, st, (int)nc, partial, out);
  else
    hipLaunchKernelGGL(k_gram_final, dim3(mde_grid(m, 256, 256)), dim3(256), 0, st, m, (int)nc, partial,
                       out);
  MDE_LAUNCH_CHECK();
  return MDE_OK;
}

extern "C" int mde_gram(int64_t n, int32_t da, int32_t db, const float* A, const float* B, double* out,
                        double* work, void* stream) {
  if (n <= 0 || da <= 0 || db <= 0 || !A || !B || !out || !work) return MDE_E_INVALID;
  const int dm = da > db ? da : db;
  return gram_impl(n, da, db, A, B, out, work_partials(work, dm), work_ticket(work, TK_GRAM), mde_stream(stream));
}

// ---------------------------------------------------------------- Z (+)= alpha * A M
// out[r][j] = (base ? base[r][j] : 0) + alpha * sum_c A[r][c] M[c][j].   out may alias A or base.
template <int D>
__global__ __launch_bounds__(MDE_BLOCK) void k_rmul_tiny(int64_t n, const float* __restrict__ A,
                                                         const double* __restrict__ M, float alpha,
                                                         const float* base, float* out) {
  float m[D * D];
#pragma unroll
  for (int i = 0; i < D * D; ++i) m[i] = (float)(M[i] * (double)alpha);
  for (int64_t r = (int64_t)blockIdx.x * MDE_BLOCK + threadIdx.x; r < n;
       r += (int64_t)gridDim.x * MDE_BLOCK) {
    float a[D], o[D];
#pragma unroll
    for (int c = 0; c < D; ++c) a[c] = A[r * D + c];
#pragma unroll
    for (int j = 0; j < D; ++j) o[j] = base ? base[r * D + j] : 0.0f;
#pragma unroll
    for (int c = 0; c < D; ++c)
#pragma unroll
      for (int j = 0; j < D; ++j) o[j] = fmaf(a[c], m[c * D + j], o[j]);
#pragma unroll
    for (int j = 0; j < D; ++j) out[r * D + j] = o[j];
  }
}

__global__ __launch_bounds__(MDE_BLOCK) void k_rmul_generic(int64_t n, int d, int d2, int rows_tile,
                                                            const float* __restrict__ A,
                                                            const double* __restrict__ M, float alpha,
                                                            const float* base, float* out) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  float* sa = reinterpret_cast<float*>(smem_raw);  // [rows_tile][d]
  for (int64_t t0 = (int64_t)blockIdx.x * rows_tile; t0 < n; t0 += (int64_t)gridDim.x * rows_tile) {
    int64_t rows = n - t0;
    if (rows > rows_tile) rows = rows_tile;
    __syncthreads();
    for (int64_t i = threadIdx.x; i < rows * d; i += MDE_BLOCK) sa[i] = A[t0 * d + i];
    __syncthreads();
    for (int64_t i = threadIdx.x; i < rows * d2; i += MDE_BLOCK) {
      const int64_t r = i / d2;
      const int j = (int)(i % d2);
      float acc = 0.0f;
      for (int c = 0; c < d; ++c) acc = fmaf(sa[r * d + c], (float)M[(int64_t)c * d2 + j], acc);
      const float b = base ? base[(t0 + r) * d2 + j] : 0.0f;
      out[(t0 + r) * d2 + j] = fmaf(alpha, acc, b);
    }
  }
}

// Widths that are multiples of 32 with d * d2 floats <= 64 KB (d = d2 <= 128): f32 MFMA
// (v_mfma_f32_32x32x2_f32).  A 256-thread workgroup takes 32 rows: their d columns are staged in
// LDS with coalesced loads (row stride d + 1: the A-operand reads then walk distinct banks), M is
// staged once as fp32, and wave w produces the 32 x 32 output tiles j = w, w + 4, ...  Operand
// map as in k_gram_mfma: A-operand lane l = (row l & 31, k = l >> 5), B-operand lane l =
// (k = l >> 5, column l & 31); C/D: column l & 31, row (reg & 3) + 8 (reg >> 2) + 4 (l >> 5).
__global__ __launch_bounds__(MDE_BLOCK) void k_rmul_mfma(int64_t n, int d, int d2, const float* __restrict__ A,
                                                         const double* __restrict__ M, float alpha,
                                                         const float* base, float* out) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  float* sm = reinterpret_cast<float*>(smem_raw);  // [d][d2] fp32 copy of M
  float* sa = sm + (size_t)d * d2;                 // [32][d + 1]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int kk = lane >> 5, cc = lane & 31;
  const int lda = d + 1;
  for (int i = tid; i < d * d2; i += MDE_BLOCK) sm[i] = (float)M[i];
  for (int64_t t0 = (int64_t)blockIdx.x * 32; t0 < n; t0 += (int64_t)gridDim.x * 32) {
    __syncthreads();  // (previous tile's reads of sa are done; sm is ready on the first trip)
    for (int i = tid; i < 32 * d; i += MDE_BLOCK) {
      const int r = i / d, c = i - r * d;
      sa[r * lda + c] = (t0 + r < n) ? A[(t0 + r) * d + c] : 0.0f;
    }
    __syncthreads();
    for (int tj = wave; tj * 32 < d2; tj += MDE_BLOCK / 64) {
      f32x16 acc;
#pragma unroll
      for (int q = 0; q < 16; ++q) acc[q] = 0.0f;
      const float* pa = sa + cc * lda + kk;
      const float* pb = sm + (size_t)kk * d2 + tj * 32 + cc;
#pragma unroll 4
      for (int c = 0; c < d; c += 2)
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(pa[c], pb[(size_t)c * d2], acc, 0, 0, 0);
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const int row = (q & 3) + 8 * (q >> 2) + 4 * kk;
        if (t0 + row < n) {
          const int64_t o = (t0 + row) * d2 + tj * 32 + cc;
          const float b = base ? base[o] : 0.0f;
          out[o] = fmaf(alpha, acc[q], b);
        }
      }
    }
  }
}

static int rmul_impl(int64_t n, int d, int d2, const float* A, const double* M, float alpha,
                     const float* base, float* out, hipStream_t st) {
#define RT(D_)                                                                                     \
  if (d == D_ && d2 == D_) {                                                                       \
    hipLaunchKernelGGL((k_rmul_tiny<D_>), dim3(mde_grid(n, MDE_BLOCK)), dim3(MDE_BLOCK), 0, st, n, A, \
                       M, alpha, base, out);                                                       \
    MDE_LAUNCH_CHECK();                                                                            \
    return MDE_OK;                                                                                 \
  }
  RT(1) RT(2) RT(3) RT(4)
#undef RT
  if (g_no_mfma < 0) {
    const char* e = getenv("MDE_NO_MFMA");
    g_no_mfma = (e && atoi(e)) ? 1 : 0;
  }
  if (!g_no_mfma && d % 32 == 0 && d2 % 32 == 0 && (size_t)d * d2 * sizeof(float) <= 65536 && (A != out || d == d2)) {
    const size_t lds = ((size_t)d * d2 + 32 * (size_t)(d + 1)) * sizeof(float);
    hipLaunchKernelGGL(k_rmul_mfma, dim3(mde_grid(n, 32, 2048)), dim3(MDE_BLOCK), lds, st, n, d, d2, A, M, alpha,
                       base, out);
    MDE_LAUNCH_CHECK();
    return MDE_OK;
  }
  int rows_tile = 8192 / d;
  if (rows_tile < 1) rows_tile = 1;
  if (rows_tile > 64) rows_tile = 64;
  const size_t lds = (size_t)rows_tile * d * sizeof(float);
  hipLaunchKernelGGL(k_rmul_generic, dim3(mde_grid(n, rows_tile, 2048)), dim3(MDE_BLOCK), lds, st, n, d,
                     d2, rows_tile, A, M, alpha, base, out);
  MDE_LAUNCH_CHECK();
  return MDE_OK;
}

extern "C" int mde_right_multiply(int64_t n, int32_t d, int32_t d2, const float* A, const double* M,
                                  float* out, void* stream) {
  if (n <= 0 || d <= 0 || d2 <= 0 || d > 8192 || !A || !M || !out) return MDE_E_INVALID;
  if (A == out && d != d2) return MDE_E_INVALID;
  return rmul_impl(n, d, d2, A, M, 1.0f, nullptr, out, mde_stream(stream));
}

extern "C" int mde_right_multiply_add(int64_t n, int32_t d, int32_t d2, const float* A, const double* M,
                                      float alpha, const float* base, float* out, void* stream) {
  if (n <= 0 || d <= 0 || d2 <= 0 || d > 8192 || !A || !M || !out) return MDE_E_INVALID;
  if (A == out && d != d2) return MDE_E_INVALID;
  return rmul_impl(n, d, d2, A, M, alpha, base, out, mde_stream(stream));
}

__global__ __launch_bounds__(MDE_BLOCK) void k_row_scale(int64_t N, int d, const float* __restrict__ scale,
                                                         float* __restrict__ Z) {
  for (int64_t i = (int64_t)blockIdx.x * MDE_BLOCK + threadIdx.x; i < N;
       i += (int64_t)gridDim.x * MDE_BLOCK)
    Z[i] *= scale[i / d];
}
// Z[r, :] += shift  (shift: d device doubles)
__global__ __launch_bounds__(MDE_BLOCK) void k_shift_rows(int64_t N, int d, const double* __restrict__ shift,
                                                          float* __restrict__ Z) {
  for (int64_t i = (int64_t)blockIdx.x * MDE_BLOCK + threadIdx.x; i < N;
       i += (int64_t)gridDim.x * MDE_BLOCK)
    Z[i] = (float)((double)Z[i] + shift[i % d]);
}
extern "C" int mde_shift_rows(int64_t n, int32_t d, const double* shift, float* Z, void* stream) {
  if (n <= 0 || d <= 0 || !shift || !Z) return MDE_E_INVALID;
  hipLaunchKernelGGL(k_shift_rows, dim3(mde_grid(n * d, MDE_BLOCK)), dim3(MDE_BLOCK), 0, mde_stream(stream),
                     n * d, d, shift, Z);
  MDE_LAUNCH_CHECK();
  return MDE_OK;
}
extern "C" int mde_row_scale(int64_t n, int32_t d, const float* scale, float* Z, void* stream) {
  if (n <= 0 || d <= 0 || !scale || !Z) return MDE_E_INVALID;
  hipLaunchKernelGGL(k_row_scale, dim3(mde_grid(n * d, MDE_BLOCK)), dim3(MDE_BLOCK), 0, mde_stream(stream),
                     n * d, d, scale, Z);
  MDE_LAUNCH_CHECK();
  return MDE_OK;
}

// ---------------------------------------------------------------- Standardized: tangent space
// Z -= (1/n) X (Z^T X)                                    [ref: constraints.py:186-192]
extern "C" int mde_std_tangent(int64_t n, int32_t d, const float* X, float* Z, double* work,
                               void* stream) {
  if (n <= 0 || d <= 0 || d > 2048 || !X || !Z || !work) return MDE_E_INVALID;
  hipStream_t st = mde_stream(stream);
  double* G = work_mats(work);  // d x d : G[i][j] = sum_r Z[r][i] X[r][j]
  if (mde_mfma_width_ok(d)) {
    int rc = mde_mfma_gram(n, d, Z, X, nullptr, G, work_partials(work, d), MDE_PARTIAL_DOUBLES, st);
    if (rc != MDE_OK) return rc;
    return mde_mfma_rmul(n, d, X, G, nullptr, (float)(-1.0 / (double)n), Z, Z, st);
  }
  int rc = gram_impl(n, d, d, Z, X, G, work_partials(work, d), work_ticket(work, TK_GRAM), st);
  if (rc != MDE_OK) return rc;
  return rmul_impl(n, d, d, X, G, (float)(-1.0 / (double)n), Z, Z, st);
}

// The same with the statistics of the result folded in (d <= 4: one launch less per evaluation): what
// mde_std_tangent(X, Z) followed by mde_vec_stats(Z, dir, X) leaves in `stats`.
template <int D>
__global__ __launch_bounds__(MDE_BLOCK) void k_rmul_tiny_stats(int64_t n, const float* __restrict__ X,
                                                               const double* __restrict__ G, float alpha, float* Z,
                                                               const float* __restrict__ dir, double* __restrict__ partial,
                                                               double* stats, unsigned int* __restrict__ ticket,
                                                               MdeMirror mirror) {
  float m[D * D];
#pragma unroll
  for (int i = 0; i < D * D; ++i) m[i] = (float)(G[i] * (double)alpha);
  double gd = 0, gg = 0, g1 = 0, gm = 0, nf = 0, dd = 0, dm = 0, xx = 0;
  for (int64_t r = (int64_t)blockIdx.x * MDE_BLOCK + threadIdx.x; r < n; r += (int64_t)gridDim.x * MDE_BLOCK) {
    float a[D], o[D];
#pragma unroll
    for (int c = 0; c < D; ++c) a[c] = X[r * D + c];
#pragma unroll
    for (int j = 0; j < D; ++j) o[j] = Z[r * D + j];
#pragma unroll
    for (int c = 0; c < D; ++c)
#pragma unroll
      for (int j = 0; j < D; ++j) o[j] = fmaf(a[c], m[c * D + j], o[j]);
#pragma unroll
    for (int j = 0; j < D; ++j) {
      Z[r * D + j] = o[j];
      const double gv = o[j], xv = a[j];
      gg += gv * gv;
      const double ag = fabs(gv);
      g1 += ag;
      gm = ag > gm ? ag : gm;
      nf += (fabsf(o[j]) <= 3.402823466e+38f) ? 0.0 : 1.0;
      xx += xv * xv;
      if (dir) {
        const double dv = dir[r * D + j];
        gd += gv * dv;
        dd += dv * dv;
        const double ad = fabs(dv);
        dm = ad > dm ? ad : dm;
      }
    }
  }
  const double v[8] = {gd, gg, g1, gm, nf, dd, dm, xx};
  mde_publish8(v, (1u << 3) | (1u << 6), partial, gridDim.x, blockIdx.x);
  if (!mde_last_block(ticket)) return;
  mde_final_rows(8, gridDim.x, partial, stats, (1ull << 3) | (1ull << 6));
  mde_mirror_write(mirror);
}

int mde_std_tangent_stats_impl(int64_t n, int32_t d, const float* X, float* Z, const float* dir, double* stats,
                               double* work, void* stream, MdeMirror mirror) {
  hipStream_t st = mde_stream(stream);
  if (d > 4) {
    const int rc = mde_std_tangent(n, d, X, Z, work, stream);
    if (rc != MDE_OK) return rc;
    return mde_vec_stats_impl(n * (int64_t)d, Z, dir, X, stats, work, st, mirror);
  }
  double* G = work_mats(work);
  const int rc = gram_impl(n, d, d, Z, X, G, work_partials(work, d), work_ticket(work, TK_GRAM), st);
  if (rc != MDE_OK) return rc;
  const int nb = mde_grid(n, MDE_BLOCK * 2, MDE_RED_BLOCKS);
  const float alpha = (float)(-1.0 / (double)n);
#define TINY(D_)                                                                                                  \
  if (d == D_)                                                                                                    \
    hipLaunchKernelGGL(k_rmul_tiny_stats<D_>, dim3(nb), dim3(MDE_BLOCK), 0, st, n, X, G, alpha, Z, dir,           \
                       work_partials(work, d), stats, work_ticket(work, TK_STATS), mirror);
  // (the partials go behind the matrices: G itself is still being read by workgroups that start late)
  TINY(1) TINY(2) TINY(3) TINY(4)
#undef TINY
  MDE_LAUNCH_CHECK();
  return MDE_OK;
}

extern "C" int mde_std_tangent_stats(int64_t n, int32_t d, const float* X, float* Z, const float* dir, double* stats,
                                     double* work, void* stream) {
  if (n <= 0 || d <= 0 || d > 2048 || !X || !Z || !stats || !work) return MDE_E_INVALID;
  return mde_std_tangent_stats_impl(n, d, X, Z, dir, stats, work, stream, MdeMirror{});
}

// ---------------------------------------------------------------- C^{-1/2} of a small SPD matrix
// One workgroup.  d = 1, 2: closed form.  d >= 3: coupled Newton-Schulz iteration in double
//   Y0 = C/s, Z0 = I;  T = (3I - Z Y)/2;  Y <- Y T;  Z <- T Z;   Z -> (C/s)^{-1/2}
// with s = ||C||_F.  M = out_scale * C^{-1/2}.  status != 0: C not numerically SPD.
// (a device function of one 256-thread workgroup: also called by the last workgroup of the fused
// small-d retraction kernel, right after it has written C -- hence no __restrict__ / read-only loads)
__device__ void invsqrt_block(int d, const double* C, double out_scale, double* M,
                              double* scratch /* 5 d^2 */, int32_t* status) {
  __shared__ double smem[8];
  __shared__ double sh_val;
  __shared__ int sh_done;
  const int tid = threadIdx.x;
  const int m = d * d;
  if (d == 1) {
    if (tid == 0) {
      const double c = C[0];
      const bool ok = c > 0.0 && c < 1e300;
      M[0] = ok ? out_scale / sqrt(c) : 0.0;
      if (status && !ok) *status = 1;
    }
    return;
  }
  if (d == 2) {
    if (tid == 0) {
      const double a = C[0], b = 0.5 * (C[1] + C[2]), c = C[3];
      const double det = a * c - b * b, tr = a + c;
      const bool ok = det > 0.0 && tr > 0.0 && det < 1e300;
      if (ok) {
        const double s = sqrt(det), t = sqrt(tr + 2.0 * s);
        const double k = out_scale / (s * t);
        M[0] = (c + s) * k;
        M[1] = -b * k;
        M[2] = -b * k;
        M[3] = (a + s) * k;
      } else {
        M[0] = M[1] = M[2] = M[3] = 0.0;
        if (status) *status = 1;
      }
    }
    return;
  }
  double* Y = scratch;
  double* Z = scratch + m;
  double* T = scratch + 2 * (int64_t)m;
  double* Yn = scratch + 3 * (int64_t)m;
  double* Zn = scratch + 4 * (int64_t)m;
  // s = ||C||_F
  double ss = 0.0;
  for (int i = tid; i < m; i += MDE_BLOCK) ss += C[i] * C[i];
  const double tot = mde_block_sum(ss, smem);
  if (tid == 0) sh_val = sqrt(tot);
  __syncthreads();
  const double s = sh_val;
  if (!(s > 0.0) || !(s < 1e300)) {
    for (int i = tid; i < m; i += MDE_BLOCK) M[i] = 0.0;
    if (tid == 0 && status) *status = 1;
    return;
  }
  for (int i = tid; i < m; i += MDE_BLOCK) {
    const int r = i / d, c = i % d;
    Y[i] = 0.5 * (C[i] + C[c * d + r]) / s;  // symmetrise
    Z[i] = (r == c) ? 1.0 : 0.0;
  }
  __syncthreads();
  bool converged = false;
  for (int it = 0; it < 200; ++it) {
    // T = (3I - Z Y)/2, residual = max |I - Z Y|
    double res = 0.0;
    for (int i = tid; i < m; i += MDE_BLOCK) {
      const int r = i / d, c = i % d;
      double acc = 0.0;
      for (int k = 0; k < d; ++k) acc = fma(Z[r * d + k], Y[k * d + c], acc);
      const double e = ((r == c) ? 1.0 : 0.0) - acc;
      res = fabs(e) > res ? fabs(e) : res;
      T[i] = ((r == c) ? 1.0 : 0.0) + 0.5 * e;
    }
    const double rmax = mde_block_max(res, smem);
    if (tid == 0) sh_done = (rmax < 1e-13) ? 1 : ((rmax == rmax && rmax < 1e300) ? 0 : 2);
    __syncthreads();
    if (sh_done == 1) {
      converged = true;
      break;
    }
    if (sh_done == 2) break;
    for (int i = tid; i < m; i += MDE_BLOCK) {
      const int r = i / d, c = i % d;
      double ay = 0.0, az = 0.0;
      for (int k = 0; k < d; ++k) {
        ay = fma(Y[r * d + k], T[k * d + c], ay);
        az = fma(T[r * d + k], Z[k * d + c], az);
      }
      Yn[i] = ay;
      Zn[i] = az;
    }
    __syncthreads();
    for (int i = tid; i < m; i += MDE_BLOCK) {
      Y[i] = Yn[i];
      Z[i] = Zn[i];
    }
    __syncthreads();
  }
  const double k = out_scale / sqrt(s);
  for (int i = tid; i < m; i += MDE_BLOCK) M[i] = converged ? Z[i] * k : 0.0;
  if (tid == 0 && status && !converged) *status = 1;
}
__global__ __launch_bounds__(MDE_BLOCK) void k_invsqrt(int d, const double* C, double out_scale, double* M,
                                                       double* scratch /* 5 d^2 */, int32_t* status) {
  invsqrt_block(d, C, out_scale, M, scratch, status);
}

// ---------------------------------------------------------------- small-d retraction in two launches
// Z <- sqrt(n) (Z - mean) C^{-1/2} for d <= 4.  One pass accumulates the column sums and the RAW
// Gram matrix Z^T Z in double; the last workgroup to arrive forms mean, C = Z^T Z - n mean mean^T
// (the Gram matrix of the centred rows) and out_scale C^{-1/2}; k_center_rmul_tiny then applies
// both.  (Seven launches -- column sums, their reduction, the subtraction, Gram, its reduction,
// the inverse square root, the multiply -- when composed from the general-d pieces.)
// X0 / DIR given: Z <- X0 + t DIR first (the trial point of the line search: one launch less).
template <int D>
__global__ __launch_bounds__(MDE_BLOCK) void k_retract_stats_tiny(int64_t n, float* Z, const float* X0,
                                                                  const float* DIR, float t,
                                                                  int demean, double out_scale,
                                                                  double* partial /* [D*D + D][nb] */,
                                                                  double* mean /* D */, double* C, double* M,
                                                                  double* scratch, int32_t* status,
                                                                  unsigned int* ticket) {
  __shared__ double smem[8];
  constexpr int NQ = D * D + D;
  double acc[NQ];
#pragma unroll
  for (int q = 0; q < NQ; ++q) acc[q] = 0.0;
  for (int64_t r = (int64_t)blockIdx.x * MDE_BLOCK + threadIdx.x; r < n; r += (int64_t)gridDim.x * MDE_BLOCK) {
    double a[D];
    if (DIR) {
#pragma unroll
      for (int i = 0; i < D; ++i) {
        const float z = fmaf(t, DIR[r * D + i], X0[r * D + i]);
        Z[r * D + i] = z;
        a[i] = z;
      }
    } else {
#pragma unroll
      for (int i = 0; i < D; ++i) a[i] = Z[r * D + i];
    }
#pragma unroll
    for (int i = 0; i < D; ++i) {
      acc[D * D + i] += a[i];
#pragma unroll
      for (int j = 0; j < D; ++j) acc[i * D + j] = fma(a[i], a[j], acc[i * D + j]);
    }
  }
  const int nb = gridDim.x;
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    const double r = mde_block_sum(acc[q], smem);
    if (threadIdx.x == 0) mde_st_partial(partial + (int64_t)q * nb + blockIdx.x, r);
  }
  if (!mde_last_block(ticket)) return;
  __shared__ double tot[NQ];
  mde_final_rows(NQ, nb, partial, tot, 0ull);
  __syncthreads();
  if (threadIdx.x < D * D) {
    const int i = threadIdx.x / D, j = threadIdx.x % D;
    const double mi = demean ? tot[D * D + i] / (double)n : 0.0;
    const double mj = demean ? tot[D * D + j] / (double)n : 0.0;
    C[threadIdx.x] = tot[threadIdx.x] - (double)n * mi * mj;
    if (j == 0) mean[i] = mi;
  }
  __threadfence_block();
  __syncthreads();
  invsqrt_block(D, C, out_scale, M, scratch, status);
}

template <int D>
__global__ __launch_bounds__(MDE_BLOCK) void k_center_rmul_tiny(int64_t n, const double* __restrict__ mean,
                                                                const double* __restrict__ M,
                                                                float* __restrict__ Z) {
  double mu[D];
  float m[D * D];
#pragma unroll
  for (int i = 0; i < D; ++i) mu[i] = mean[i];
#pragma unroll
  for (int i = 0; i < D * D; ++i) m[i] = (float)M[i];
  for (int64_t r = (int64_t)blockIdx.x * MDE_BLOCK + threadIdx.x; r < n; r += (int64_t)gridDim.x * MDE_BLOCK) {
    float a[D], o[D];
#pragma unroll
    for (int c = 0; c < D; ++c) a[c] = (float)((double)Z[r * D + c] - mu[c]);
#pragma unroll
    for (int j = 0; j < D; ++j) o[j] = 0.0f;
#pragma unroll
    for (int c = 0; c < D; ++c)
#pragma unroll
      for (int j = 0; j < D; ++j) o[j] = fmaf(a[c], m[c * D + j], o[j]);
#pragma unroll
    for (int j = 0; j < D; ++j) Z[r * D + j] = o[j];
  }
}


// ---------------------------------------------------------------- C^{-1/2}, d >= 32: two launches per step
// The single-workgroup iteration above needs three d^3 double products per step out of global
// memory with 256 threads (22 ms at d = 128).  Here every product is spread over d^2 / 256
// workgroups, two launches per step (T = (3 I - Z Y) / 2 with the residual; then Y T and T Z).
// Every step has its own residual word, so a kernel can tell from the words of the earlier steps
// whether the iteration is over -- no flag kernel, no state to reset -- and the host reads the
// words back after each batch of MDE_NS_BATCH steps instead of enqueuing the worst-case count
// (round 2 enqueued 180 launches + a memset per retraction; near-orthonormal iterates need 6 - 9
// steps).
//   ctl[0] = 2 when C is not usable, ctl[2] = the scale s, ctl[8 + s] = max |I - Z Y| of step s
#define MDE_NS_MAX_STEPS 64
#define MDE_NS_BATCH 6
#define MDE_NS_TOL 1e-13
// 0: still iterating after steps [0, upto); 1: converged (at *where); 2: failed
__device__ __forceinline__ int ns_state(const double* __restrict__ ctl, int upto, int* where) {
  if (ctl[0] == 2.0) return 2;
  for (int s = 0; s < upto; ++s) {
    const double r = ctl[8 + s];
    if (r < MDE_NS_TOL) {
      if (where) *where = s;
      return 1;
    }
    if (!(r < 1e300)) return 2;
  }
  return 0;
}
// Y0 = sym(C) / s, Z0 = I with s = max_i sum_j |sym(C)_ij| >= lambda_max (Gershgorin): for the solver's
// near-orthonormal iterates C ~ n I the eigenvalues of Y0 start close to 1 and the iteration is over
// in 3 - 5 steps (the Frobenius norm used before starts them at 1 / sqrt(d): 9 - 10 steps).
// Every workgroup forms s itself (d^2 doubles out of L2) and initialises its own slice.
__global__ __launch_bounds__(MDE_BLOCK) void k_ns_init(int d, const double* __restrict__ C, double* __restrict__ Y,
                                                       double* __restrict__ Z, double* __restrict__ ctl) {
  __shared__ double smem[8];
  __shared__ double sh;
  const int m = d * d;
  // (column sums of |C|: coalesced; C is symmetric up to rounding, the symmetrised row sums differ in
  // the last bits, which the iteration does not mind)
  double mx = 0.0;
  for (int c = threadIdx.x; c < d; c += MDE_BLOCK) {
    double t = 0.0;
#pragma unroll 8
    for (int r = 0; r < d; ++r) t += fabs(C[r * d + c]);
    t = (t == t) ? t : 1e308;
    mx = t > mx ? t : mx;
  }
  const double tot = mde_block_max(mx, smem);
  if (threadIdx.x == 0) sh = tot;
  __syncthreads();
  const double s = sh;
  const bool ok = (s > 0.0) && (s < 1e300);
  for (int i = blockIdx.x * MDE_BLOCK + threadIdx.x; i < m; i += gridDim.x * MDE_BLOCK) {
    const int r = i / d, c = i % d;
    Y[i] = ok ? 0.5 * (C[i] + C[c * d + r]) / s : 0.0;  // symmetrise
    Z[i] = (r == c) ? 1.0 : 0.0;
  }
  if (blockIdx.x == 0) {
    for (int i = threadIdx.x; i < MDE_NS_MAX_STEPS; i += MDE_BLOCK) ctl[8 + i] = 0.0;
    if (threadIdx.x == 0) {
      ctl[0] = ok ? 0.0 : 2.0;
      ctl[2] = s;
    }
  }
}
// One 32 x 32 tile of P = A B (d x d doubles, row-major) per 256-thread workgroup: thread (ty, tx) owns
// the 2 x 2 outputs at rows 2 ty, columns 2 tx of the tile; the operands pass through LDS in 32-wide
// slabs of the inner index (row stride 33: no bank conflicts on the column reads).
__device__ __forceinline__ void ns_tile_product(int d, const double* __restrict__ A, const double* __restrict__ B,
                                                int ti, int tj, double (&o)[2][2]) {
  __shared__ double As[32][33], Bs[32][33];
  const int ty = threadIdx.x >> 4, tx = threadIdx.x & 15;
  o[0][0] = o[0][1] = o[1][0] = o[1][1] = 0.0;
  for (int k0 = 0; k0 < d; k0 += 32) {
    __syncthreads();
    for (int e = threadIdx.x; e < 1024; e += MDE_BLOCK) {
      const int rr = e >> 5, cc = e & 31;
      const int ar = ti * 32 + rr, ac = k0 + cc, br = k0 + rr, bc = tj * 32 + cc;
      As[rr][cc] = (ar < d && ac < d) ? A[ar * d + ac] : 0.0;
      Bs[rr][cc] = (br < d && bc < d) ? B[br * d + bc] : 0.0;
    }
    __syncthreads();
#pragma unroll 8
    for (int k = 0; k < 32; ++k) {
      const double a0 = As[2 * ty][k], a1 = As[2 * ty + 1][k], b0 = Bs[k][2 * tx], b1 = Bs[k][2 * tx + 1];
      o[0][0] = fma(a0, b0, o[0][0]);
      o[0][1] = fma(a0, b1, o[0][1]);
      o[1][0] = fma(a1, b0, o[1][0]);
      o[1][1] = fma(a1, b1, o[1][1]);
    }
  }
}
// step: T = (3 I - Z Y) / 2 and the residual max |I - Z Y| (atomic max on the bit pattern of a
// non-negative double; the word starts at +0.0).  grid = (tiles, tiles)
__global__ __launch_bounds__(MDE_BLOCK) void k_ns_t(int d, int step, const double* __restrict__ Y,
                                                    const double* __restrict__ Z, double* __restrict__ T,
                                                    double* __restrict__ ctl) {
  if (ns_state(ctl, step, nullptr) != 0) return;
  __shared__ double smem[8];
  double o[2][2];
  ns_tile_product(d, Z, Y, blockIdx.y, blockIdx.x, o);
  const int ty = threadIdx.x >> 4, tx = threadIdx.x & 15;
  double emax = 0.0;
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      const int r = blockIdx.y * 32 + 2 * ty + a, c = blockIdx.x * 32 + 2 * tx + b;
      if (r < d && c < d) {
        const double e = ((r == c) ? 1.0 : 0.0) - o[a][b];
        T[r * d + c] = ((r == c) ? 1.0 : 0.0) + 0.5 * e;
        const double ae = (e == e) ? fabs(e) : 1e308;
        emax = ae > emax ? ae : emax;
      }
    }
  const double mx = mde_block_max(emax, smem);
  if (threadIdx.x == 0)
    atomicMax(reinterpret_cast<unsigned long long*>(ctl + 8 + step), (unsigned long long)__double_as_longlong(mx));
}
// step: (Yn, Zn) = (Y T, T Z) unless the iteration ended with this step's residual.
// grid = (tiles, tiles, 2): z = 0 forms Y T, z = 1 forms T Z
__global__ __launch_bounds__(MDE_BLOCK) void k_ns_yz(int d, int step, const double* __restrict__ Y,
                                                     const double* __restrict__ Z, const double* __restrict__ T,
                                                     double* __restrict__ Yn, double* __restrict__ Zn,
                                                     const double* __restrict__ ctl) {
  if (ns_state(ctl, step + 1, nullptr) != 0) return;
  double o[2][2];
  const bool first = blockIdx.z == 0;
  ns_tile_product(d, first ? Y : T, first ? T : Z, blockIdx.y, blockIdx.x, o);
  double* out = first ? Yn : Zn;
  const int ty = threadIdx.x >> 4, tx = threadIdx.x & 15;
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      const int r = blockIdx.y * 32 + 2 * ty + a, c = blockIdx.x * 32 + 2 * tx + b;
      if (r < d && c < d) out[r * d + c] = o[a][b];
    }
}
// M = out_scale / sqrt(s) * Z of the step that converged (step s left its pair in buffer s & 1)
__global__ __launch_bounds__(MDE_BLOCK) void k_ns_finish(int d, int nsteps, const double* __restrict__ Z0,
                                                         const double* __restrict__ Z1, const double* __restrict__ ctl,
                                                         double out_scale, double* __restrict__ M,
                                                         int32_t* __restrict__ status) {
  int where = 0;
  const bool ok = ns_state(ctl, nsteps, &where) == 1;
  const double* Z = (where & 1) ? Z1 : Z0;
  const double k = ok ? out_scale / sqrt(ctl[2]) : 0.0;
  for (int i = blockIdx.x * MDE_BLOCK + threadIdx.x; i < d * d; i += gridDim.x * MDE_BLOCK) M[i] = ok ? Z[i] * k : 0.0;
  if (blockIdx.x == 0 && threadIdx.x == 0 && status && !ok) *status = 1;
}

// M = out_scale * C^{-1/2}: the single-workgroup kernel for small d, the launch sequence above
// otherwise (SYNC for d >= 32: the residual words are read back after every batch of steps)
static int invsqrt_impl(int d, const double* C, double out_scale, double* M, double* scratch /* 5 d^2 + 8 + 64 */,
                        int32_t* status_dev, hipStream_t st) {
  if (d < 32) {
    hipLaunchKernelGGL(k_invsqrt, dim3(1), dim3(MDE_BLOCK), 0, st, d, C, out_scale, M, scratch, status_dev);
    MDE_LAUNCH_CHECK();
    return MDE_OK;
  }
  const int64_t m = (int64_t)d * d;
  double* Y[2] = {scratch, scratch + 3 * m};
  double* Z[2] = {scratch + m, scratch + 4 * m};
  double* T = scratch + 2 * m;
  double* ctl = scratch + 5 * m;         // 8 + MDE_NS_MAX_STEPS doubles
  hipLaunchKernelGGL(k_ns_init, dim3(mde_grid(m, MDE_BLOCK, 64)), dim3(MDE_BLOCK), 0, st, d, C, Y[0], Z[0], ctl);
  MDE_LAUNCH_CHECK();
  const unsigned nt = (unsigned)((d + 31) / 32);
  int steps = 0;
  double host[8 + MDE_NS_MAX_STEPS];
  bool done = false;
  while (!done && steps < MDE_NS_MAX_STEPS) {
    const int upto = std::min(MDE_NS_MAX_STEPS, steps + MDE_NS_BATCH);
    for (; steps < upto; ++steps) {
      const int h = steps & 1;
      hipLaunchKernelGGL(k_ns_t, dim3(nt, nt), dim3(MDE_BLOCK), 0, st, d, steps, Y[h], Z[h], T, ctl);
      hipLaunchKernelGGL(k_ns_yz, dim3(nt, nt, 2), dim3(MDE_BLOCK), 0, st, d, steps, Y[h], Z[h], T, Y[h ^ 1], Z[h ^ 1], ctl);
    }
    MDE_LAUNCH_CHECK();
    MDE_HIP(hipMemcpyAsync(host, ctl, sizeof(double) * (8 + (size_t)steps), hipMemcpyDeviceToHost, st));
    MDE_HIP(hipStreamSynchronize(st));
    if (host[0] == 2.0) done = true;
    for (int s = 0; s < steps && !done; ++s) done = (host[8 + s] < MDE_NS_TOL) || !(host[8 + s] < 1e300);
  }
  hipLaunchKernelGGL(k_ns_finish, dim3(mde_grid(m, MDE_BLOCK, 64)), dim3(MDE_BLOCK), 0, st, d, steps, Z[0], Z[1], ctl,
                     out_scale, M, status_dev);
  MDE_LAUNCH_CHECK();
  return MDE_OK;
}

// Z <- sqrt(n) (Z - mean) C^{-1/2},  C = (Z-mean)^T (Z-mean)          [ref: util.py:129-161]
// (= sqrt(n) U V^T of the thin SVD Z - mean = U S V^T, the reference's formula.)
// (X0, DIR, t given: Z <- X0 + t DIR first -- folded into the statistics pass at d <= 4)
static int std_retract_impl(int64_t n, int32_t d, float* Z, int32_t demean, double* work, int32_t* status_dev,
                            hipStream_t st, const float* X0 = nullptr, const float* DIR = nullptr, float t = 0.0f) {
  int rc = MDE_OK;
  if (DIR && d > 4) {
    rc = mde_axpy_impl(n * (int64_t)d, t, DIR, X0, Z, st);
    if (rc != MDE_OK) return rc;
  }
  double* mats = work_mats(work);
  const int64_t m = (int64_t)d * d;
  double* C = mats;
  double* M = mats + m;
  double* scratch = mats + 2 * m;  // 5 m
  if (d <= 4) {
    const int nb = mde_grid(n, MDE_BLOCK * 2, MDE_RED_BLOCKS);
    const int nb2 = mde_grid(n, MDE_BLOCK, 2048);
    double* mean = work;  // small area
#define TINY(D_)                                                                                             \
  if (d == D_) {                                                                                             \
    hipLaunchKernelGGL(k_retract_stats_tiny<D_>, dim3(nb), dim3(MDE_BLOCK), 0, st, n, Z, X0, DIR, t,         \
                       (int)demean, sqrt((double)n), work_partials(work, d), mean, C, M, scratch, status_dev, \
                       work_ticket(work, TK_RETRACT));                                                       \
    MDE_LAUNCH_CHECK();                                                                                      \
    hipLaunchKernelGGL(k_center_rmul_tiny<D_>, dim3(nb2), dim3(MDE_BLOCK), 0, st, n, mean, M, Z);             \
    MDE_LAUNCH_CHECK();                                                                                      \
    return MDE_OK;                                                                                           \
  }
    TINY(1) TINY(2) TINY(3) TINY(4)
#undef TINY
  }
  if (mde_mfma_width_ok(d)) {
    // three reads and one write of Z: column means, the Gram matrix of the centred rows (the mean is
    // subtracted in registers), C^{-1/2}, and (Z - mean) M written in place
    double* mean = work;  // small area
    if (demean) {
      rc = mde_mfma_colmean(n, d, Z, work_partials(work, d), mean, st);
      if (rc != MDE_OK) return rc;
    }
    rc = mde_mfma_gram(n, d, Z, Z, demean ? mean : nullptr, C, work_partials(work, d), MDE_PARTIAL_DOUBLES, st);
    if (rc != MDE_OK) return rc;
    rc = invsqrt_impl(d, C, sqrt((double)n), M, scratch, status_dev, st);
    if (rc != MDE_OK) return rc;
    return mde_mfma_rmul(n, d, Z, M, demean ? mean : nullptr, 1.0f, nullptr, Z, st);
  }
  if (demean) {
    rc = mde_center_impl(n, d, Z, work, st);
    if (rc != MDE_OK) return rc;
  }
  rc = gram_impl(n, d, d, Z, Z, C, work_partials(work, d), work_ticket(work, TK_GRAM), st);
  if (rc != MDE_OK) return rc;
  rc = invsqrt_impl(d, C, sqrt((double)n), M, scratch, status_dev, st);
  if (rc != MDE_OK) return rc;
  return rmul_impl(n, d, d, Z, M, 1.0f, nullptr, Z, st);
}

extern "C" int mde_std_retract(int64_t n, int32_t d, float* Z, int32_t demean, double* work,
                               int32_t* status_dev, void* stream) {
  if (n <= 0 || d <= 0 || d > 2048 || !Z || !work) return MDE_E_INVALID;
  return std_retract_impl(n, d, Z, demean, work, status_dev, mde_stream(stream));
}

// Z <- retract(X + t dir): the trial point of the line search under the Standardized constraint
extern "C" int mde_std_retract_step(int64_t n, int32_t d, const float* X, const float* dir, float t, float* Z,
                                    int32_t demean, double* work, int32_t* status_dev, void* stream) {
  if (n <= 0 || d <= 0 || d > 2048 || !X || !dir || !Z || !work) return MDE_E_INVALID;
  return std_retract_impl(n, d, Z, demean, work, status_dev, mde_stream(stream), X, dir, t);
}

// mde_metric.hip -- metrics other than Euclidean on the original data: the prologue
// that turns cosine / correlation into a Euclidean search on unit rows, the exact Manhattan k-NN kernel,
// and the per-edge distance kernel of every metric.  Definitions follow scipy.spatial.distance
// (cosine 1 - u.v / (|u| |v|), correlation = cosine of the row-centred vectors, cityblock sum |u - v|);
// the reference has no metric keyword (its pynndescent call is Euclidean).
#include "mde_knn_tile.h"

// ------------------------------------------------------------------ unit rows for cosine / correlation
// One wave per row (as k_row_sqnorm): the sum (for the mean), the squared norm of the centred row (both in
// double: the row is summed once, not once per pair), then out = (x - mean) / |x - mean|, centred and
// scaled in double and rounded once, so a row with a large offset keeps the digits of its spread.  A row whose
// norm is not positive -- and, when centring, a row whose min equals its max, which the f32 mean may miss
// by an ulp -- has no direction: it is counted in deg[0], its index min-reduced into deg[1], and its
// output is all zero, never NaN.  out may be NULL (the check alone).
__global__ __launch_bounds__(MDE_BLOCK) void k_rows_normalize(int64_t n, int nf, const float* __restrict__ X,
                                                              int center, float* __restrict__ out,
                                                              int* __restrict__ deg) {
  const int lane = threadIdx.x & 63;
  const int64_t w0 = ((int64_t)blockIdx.x * MDE_BLOCK + threadIdx.x) >> 6;
  const int64_t nw = ((int64_t)gridDim.x * MDE_BLOCK) >> 6;
  for (int64_t r = w0; r < n; r += nw) {
    const float* x = X + r * nf;
    double mean = 0.0;
    bool flat = false;
    if (center) {
      double s = 0.0;
      float mx = -3.402823466e+38f, mn = 3.402823466e+38f;
      for (int c = lane; c < nf; c += 64) {
        const float v = x[c];
        s += (double)v;
        mx = fmaxf(mx, v);
        mn = fminf(mn, v);
      }
      mean = mde_wave_sum(s) / (double)nf;
      flat = !(mde_wave_max(mx) > -mde_wave_max(-mn));
    }
    double q = 0.0;
    for (int c = lane; c < nf; c += 64) {
      const double d = (double)x[c] - mean;
      q += d * d;
    }
    q = mde_wave_sum(q);
    const bool bad = flat || !(q > 0.0) || !(q < 1.0e300);
    const double inv = bad ? 0.0 : 1.0 / sqrt(q);
    if (out)
      for (int c = lane; c < nf; c += 64) out[r * nf + c] = (float)(((double)x[c] - mean) * inv);
    if (bad && lane == 0) {
      atomicAdd(deg, 1);
      atomicMin(deg + 1, (int)r);
    }
  }
}

__global__ void k_deg_init(int* deg) {
  deg[0] = 0;
  deg[1] = 0x7fffffff;
}

// deg_out: int32 [2] on the device = (number of degenerate rows, index of the first; INT32_MAX when none).
extern "C" int mde_rows_normalize(int64_t n, int32_t nf, const float* data, int32_t center, float* out,
                                  int32_t* deg_out, void* stream) {
  if (n <= 0 || nf <= 0 || !data || !deg_out) {
    mde_set_error("mde_rows_normalize: invalid arguments (n >= 1, nf >= 1, non-null data / deg_out)");
    return MDE_E_INVALID;
  }
  if (n >= ((int64_t)1 << 31)) return MDE_E_TOO_LARGE;
  hipStream_t st = mde_stream(stream);
  hipLaunchKernelGGL(k_deg_init, dim3(1), dim3(1), 0, st, deg_out);
  hipLaunchKernelGGL(k_rows_normalize, dim3(mde_grid(n * 64, MDE_BLOCK, 4096)), dim3(MDE_BLOCK), 0, st, n, nf,
                     data, center ? 1 : 0, out, deg_out);
  MDE_LAUNCH_CHECK();
  return MDE_OK;
}

// ------------------------------------------------------------------ exact Manhattan k-NN
// The workgroup shape of the Euclidean tile (mde_knn_tile.h): 256 threads own 64 query rows and walk the candidates 64 at
// a time; there is no matrix-core form of sum |x - y|, so each thread holds a 4 x 4 register tile of the
// 64 x 64 block of partial sums (thread (ty, tx) = (tid >> 4, tid & 15): rows 4 ty .., candidates 4 tx ..).
// Feature chunks of 32 are staged through LDS FEATURE-major, [feature][row], so that the four rows (or
// candidates) of a thread at one feature are one 16-byte read: two ds_read_b128 feed 16 subtractions and
// 16 additions of the absolute value (a source modifier of v_add_f32).  Lines are 68 floats: 16-byte
// aligned, and the 16 tx of a wave read 256 contiguous bytes -- one bank row, conflict-free -- while its
// 4 ty read 4 broadcast addresses.  Staging: thread (c = tid & 31, g = tid >> 5) loads feature c of rows
// 4 g .. 4 g + 3 and 32 + 4 g .. (128-byte coalesced across the lanes) and commits them as two 16-byte
// writes; the next chunk's loads are issued before the arithmetic of the current one.  The tile is parked
// in LDS and merged by mde_topk_merge exactly as the Euclidean kernel does.  Zero padding past nf adds
// |0 - 0| = 0; rows past n are masked when the tile is parked.
#define L1_BM 64
#define L1_BN 64
#define L1_KB 32
#define L1_LD 68

// acc += |d| as ONE v_add_f32 with the absolute value as a source modifier.  Written as acc += fabsf(d) the
// compiler pairs the accumulators into v_pk_add_f32, which has no abs modifier, and spends a v_and_b32 per
// element on it (profiles/r08_metric_knn.txt, the ISA counts); this form keeps two VALU operations per
// element pair, v_sub_f32 and v_add_f32.
__device__ __forceinline__ void l1_accumulate(float& acc, float d) {
  asm("v_add_f32 %0, |%1|, %0" : "+v"(acc) : "v"(d));
}

__global__ __launch_bounds__(MDE_BLOCK) void k_knn_l1(int n, int nf, int k, const float* __restrict__ X,
                                                      int32_t* __restrict__ idx_out, float* __restrict__ d_out) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* sA = lds;                           // [L1_KB][L1_LD]
  float* sB = sA + L1_KB * L1_LD;            // [L1_KB][L1_LD]
  float* sD = sB + L1_KB * L1_LD;            // [L1_BM][L1_BN + 1] distances of the tile
  float* bestd = sD + L1_BM * (L1_BN + 1);   // [L1_BM][k]
  int* besti = reinterpret_cast<int*>(bestd + L1_BM * k);  // [L1_BM][k]
  const int tid = threadIdx.x;
  const int tx = tid & 15, ty = tid >> 4;
  const int sc = tid & 31, sg = tid >> 5;
  const int row0 = blockIdx.x * L1_BM;
  knn_lists_init(bestd, besti, L1_BM * k);
  float worst = 3.402823466e+38f;            // thread t < 64: current k-th best of row t
  for (int col0 = 0; col0 < n; col0 += L1_BN) {
    float acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[i][j] = 0.0f;
    float ra[2][4], rb[2][4];
    auto fetch = [&](int k0) {
      const int f = k0 + sc;
      const int fc = f < nf ? f : nf - 1;
#pragma unroll
      for (int q = 0; q < 2; ++q)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int r = (sg + 8 * q) * 4 + i;
          const int gr = row0 + r, gc = col0 + r;
          // plain loads from clamped addresses, zeroed afterwards (as knn_gram_tile: no branch around a load)
          const float va = X[(int64_t)(gr < n ? gr : n - 1) * nf + fc];
          const float vb = X[(int64_t)(gc < n ? gc : n - 1) * nf + fc];
          ra[q][i] = (gr < n && f < nf) ? va : 0.0f;
          rb[q][i] = (gc < n && f < nf) ? vb : 0.0f;
        }
    };
    fetch(0);
    for (int k0 = 0; k0 < nf; k0 += L1_KB) {
      __syncthreads();
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        const int o = sc * L1_LD + (sg + 8 * q) * 4;
        *reinterpret_cast<float4*>(sA + o) = make_float4(ra[q][0], ra[q][1], ra[q][2], ra[q][3]);
        *reinterpret_cast<float4*>(sB + o) = make_float4(rb[q][0], rb[q][1], rb[q][2], rb[q][3]);
      }
      __syncthreads();
      if (k0 + L1_KB < nf) fetch(k0 + L1_KB);
      const float* pa = sA + ty * 4;
      const float* pb = sB + tx * 4;
#pragma unroll
      for (int f = 0; f < L1_KB; ++f) {
        const float4 a4 = *reinterpret_cast<const float4*>(pa + f * L1_LD);
        const float4 b4 = *reinterpret_cast<const float4*>(pb + f * L1_LD);
        const float a[4] = {a4.x, a4.y, a4.z, a4.w};
        const float b[4] = {b4.x, b4.y, b4.z, b4.w};
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j) l1_accumulate(acc[i][j], a[i] - b[j]);
      }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int r = ty * 4 + i, c = tx * 4 + j;
        const int gr = row0 + r, gc = col0 + c;
        sD[r * (L1_BN + 1) + c] = (gr < n && gc < n && gr != gc) ? acc[i][j] : 3.402823466e+38f;
      }
    __syncthreads();
    if (tid < L1_BM)
      mde_topk_merge(sD + tid * (L1_BN + 1), L1_BN, col0, k, bestd + tid * k, besti + tid * k, worst);
  }
  __syncthreads();
  // its own write-out, not knn_lists_store: with the helper the kernel measured 0.8 % slower at 70k x 784
  // (profiles/r11_knn_tile.txt) although the arithmetic loop compiled to the same instructions
  for (int i = tid; i < L1_BM * k; i += MDE_BLOCK) {
    const int r = i / k, gr = row0 + r;
    if (gr < n) {
      idx_out[(int64_t)gr * k + (i % k)] = besti[i];
      d_out[(int64_t)gr * k + (i % k)] = bestd[i];
    }
  }
}

// idx_out [n, k] int32 (-1 where fewer than k other rows exist), d_out [n, k] Manhattan distances (the
// distance itself, not a square), ascending per row, ties to the smaller index.
extern "C" int mde_knn_l1(int64_t n, int32_t nf, const float* data, int32_t k, int32_t* idx_out, float* d_out,
                          void* stream) {
  if (n <= 0 || nf <= 0 || k <= 0 || k > KNN_MAXK || !data || !idx_out || !d_out) {
    mde_set_error("mde_knn_l1: invalid arguments (1 <= k <= %d)", KNN_MAXK);
    return MDE_E_INVALID;
  }
  if (n >= ((int64_t)1 << 31)) return MDE_E_TOO_LARGE;
  const size_t lds = sizeof(float) * (size_t)(2 * L1_KB * L1_LD + L1_BM * (L1_BN + 1)) +
                     (size_t)L1_BM * k * (sizeof(float) + sizeof(int));
  const int rc = knn_raise_lds_limit<k_knn_l1>(96 * 1024);
  if (rc != MDE_OK) return rc;
  hipLaunchKernelGGL(k_knn_l1, dim3((unsigned)((n + L1_BM - 1) / L1_BM)), dim3(MDE_BLOCK), lds, mde_stream(stream),
                     (int)n, nf, k, data, idx_out, d_out);
  MDE_LAUNCH_CHECK();
  return MDE_OK;
}

// ------------------------------------------------------------------ per-edge distances: cosine, correlation, Manhattan
// One wave per edge, one pass over the two rows, sums in double (products of two floats are exact there):
// u.v, |u|^2, |v|^2 (cosine), also sum u, sum v (correlation), sum |u - v| (Manhattan); Euclidean
// pairs stay on mde_distances.  No normalised copy and no |x|^2 + |y|^2 - 2 x.y in f32, so near-duplicate rows keep their
// small distances.  An endpoint outside [0, n) gives NaN; so does an undefined distance (a zero row under
// cosine, a constant row under correlation) -- callers reject such rows first (mde_rows_normalize).
__global__ __launch_bounds__(MDE_BLOCK) void k_pair_metric(int64_t n, int nf, const float* __restrict__ X, int64_t p,
                                                           const int64_t* __restrict__ edges, int metric,
                                                           float* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int64_t w0 = ((int64_t)blockIdx.x * MDE_BLOCK + threadIdx.x) >> 6;
  const int64_t nw = ((int64_t)gridDim.x * MDE_BLOCK) >> 6;
  for (int64_t q = w0; q < p; q += nw) {
    const int64_t i = edges[2 * q], j = edges[2 * q + 1];
    if (i < 0 || i >= n || j < 0 || j >= n) {
      if (lane == 0) out[q] = __int_as_float(0x7fc00000);
      continue;
    }
    const float* u = X + i * nf;
    const float* v = X + j * nf;
    double res;
    if (metric == MDE_METRIC_MANHATTAN) {
      double s = 0.0;
      for (int c = lane; c < nf; c += 64) s += fabs((double)u[c] - (double)v[c]);
      res = mde_wave_sum(s);
    } else {
      double uv = 0.0, uu = 0.0, vv = 0.0, su = 0.0, sv = 0.0;
      for (int c = lane; c < nf; c += 64) {
        const double a = u[c], b = v[c];
        uv += a * b;
        uu += a * a;
        vv += b * b;
        su += a;
        sv += b;
      }
      uv = mde_wave_sum(uv);
      uu = mde_wave_sum(uu);
      vv = mde_wave_sum(vv);
      if (metric == MDE_METRIC_CORRELATION) {
        su = mde_wave_sum(su);
        sv = mde_wave_sum(sv);
        uv -= su * sv / (double)nf;
        uu -= su * su / (double)nf;
        vv -= sv * sv / (double)nf;
      }
      res = 1.0 - uv / sqrt(uu * vv);      // 0 / 0 -> NaN for a row without a direction
      if (res < 0.0) res = 0.0;
    }
    if (lane == 0) out[q] = (float)res;
  }
}

extern "C" int mde_pair_distances_metric(int64_t n, int32_t nf, const float* data, int64_t p, const int64_t* edges,
                                         int32_t metric, float* out, void* stream) {
  if (n <= 0 || nf <= 0 || !data || p < 0 || (p > 0 && (!edges || !out)) || metric < MDE_METRIC_COSINE ||
      metric > MDE_METRIC_MANHATTAN) {
    mde_set_error("mde_pair_distances_metric: invalid arguments (n >= 1, nf >= 1, p >= 0, metric 1..3)");
    return MDE_E_INVALID;
  }
  if (p == 0) return MDE_OK;
  hipLaunchKernelGGL(k_pair_metric, dim3(mde_grid(p * 64, MDE_BLOCK, 8192)), dim3(MDE_BLOCK), 0, mde_stream(stream),
                     n, nf, data, p, edges, metric, out);
  MDE_LAUNCH_CHECK();
  return MDE_OK;
}

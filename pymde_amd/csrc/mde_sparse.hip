// mde_sparse.hip -- sparse data matrices (CSR) on the k-NN and pair-distance paths.
//   [ref: pymde/preprocess/data_matrix.py:11-178 -- scipy.sparse inputs to distances / k_nearest_neighbors]
// Every entry point takes one device CSR: indptr int64 [n + 1], indices int32 (strictly increasing within a
// row), values f32.  k_csr_check validates it first (reads only inside the arrays), and no other kernel
// indexes through it until the check has come back clean.
//
// Exact k-NN (k_sparse_knn).  A 256-thread workgroup owns SPK_Q = 128 query rows, two per lane, and walks
// the candidates SPK_C = 128 at a time (32 per wave).  The query rows are densified into an LDS panel
// P[W][128], one window of W feature columns at a time: each wave scatters its 32 rows' entries of the
// window in and, before the next window's, scatters the previous ones back to zero (O(nnz), not
// O(W x 128)).  The panel is XOR-swizzled by feature so that the scatter (one query column, many features)
// spreads over the banks while a row read (one feature, all queries) stays one conflict-free ds_read_b64
// per lane.  A wave walks its candidates' entries of the window with a cursor per candidate: 64 entries
// are loaded across the lanes, the in-window prefix is found by a ballot, and each entry (f, v) is
// broadcast by readlane and feeds two FMAs against P[f - w0][2 lane, 2 lane + 1] into accumulators indexed
// at compile time.  After the last window the 128 x 128 tile of d2 = max(|q|^2 + |c|^2 - 2 q.c, 0) is
// parked in the (then all-zero) panel, 64 candidates at a time, and merged into the per-query top-k
// lists by mde_topk_merge, the merge of the dense kernel: candidates are offered in increasing index
// order, so ties go to the smaller index, and the result is the same on every run.
//
// Pair distances (k_sparse_pair_dist).  One wave per edge (i, j) sums (a_f - b_f)^2 over the union of the
// two rows' columns -- lanes stride row i's entries and binary-search row j, then stride row j's entries
// absent from row i -- in double, so near-duplicate rows come out near zero rather than as the rounding
// noise of |a|^2 + |b|^2 - 2 a.b.
#include <float.h>
#include <limits.h>

#include "mde_knn_tile.h"   // KNN_MAXK, knn_raise_lds_limit: the panel kernel below has its own tile

#define SPK_Q 128       // query rows per workgroup (two per lane)
#define SPK_C 128       // candidates per tile
#define SPK_CW 32       // candidates per wave
#define SPK_G 8         // candidates whose first 64 entries are loaded together
#define SPK_DS 65       // row stride of the parked d2 half-tile [SPK_Q][64 + 1]
#define SPK_MIN_W 72    // the parked half-tile (SPK_Q x SPK_DS floats) must fit in the panel

// 64-bit wave-uniform value of lane l
__device__ __forceinline__ int64_t spk_readlane64(int64_t v, int l) {
  const int lo = __builtin_amdgcn_readlane((int)(uint32_t)(uint64_t)v, l);
  const int hi = __builtin_amdgcn_readlane((int)((uint64_t)v >> 32), l);
  return (int64_t)(((uint64_t)(uint32_t)hi << 32) | (uint32_t)lo);
}
// float index of panel element (feature offset off, query column q): XOR swizzle by feature, pairs kept
__device__ __forceinline__ int spk_pidx(int off, int q) { return off * SPK_Q + (q ^ ((off & 63) << 1)); }

// ------------------------------------------------------------------ validation
__global__ __launch_bounds__(MDE_BLOCK) void k_csr_check(int64_t n, int nf, int64_t nnz,
                                                         const int64_t* __restrict__ indptr,
                                                         const int32_t* __restrict__ indices,
                                                         int* __restrict__ bad) {
  const int lane = threadIdx.x & 63;
  const int64_t w0 = ((int64_t)blockIdx.x * MDE_BLOCK + threadIdx.x) >> 6;
  const int64_t nw = ((int64_t)gridDim.x * MDE_BLOCK) >> 6;
  for (int64_t r = w0; r < n; r += nw) {
    const int64_t lo = indptr[r], hi = indptr[r + 1];
    bool ok = lo >= 0 && lo <= hi && hi <= nnz && (r != 0 || lo == 0) && (r != n - 1 || hi == nnz);
    if (ok) {
      for (int64_t e = lo + lane; e < hi; e += 64) {
        const int c = indices[e];
        if (c < 0 || c >= nf || (e > lo && indices[e - 1] >= c)) ok = false;
      }
    }
    if (!ok) *bad = 1;
  }
}

static int spk_validate(const char* who, int64_t n, int32_t nf, int64_t nnz, const int64_t* indptr,
                        const int32_t* indices, const float* values, hipStream_t st) {
  if (n <= 0 || nf <= 0 || nnz < 0 || !indptr || (nnz > 0 && (!indices || !values))) {
    mde_set_error("%s: invalid arguments (n >= 1, nf >= 1, nnz >= 0, non-null arrays)", who);
    return MDE_E_INVALID;
  }
  if (n >= ((int64_t)1 << 31)) {
    mde_set_error("%s: n must be below 2^31", who);
    return MDE_E_TOO_LARGE;
  }
  int* flag = nullptr;
  MDE_HIP(hipMalloc(&flag, sizeof(int)));
  int bad = 0;
  hipError_t e = hipMemsetAsync(flag, 0, sizeof(int), st);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(k_csr_check, dim3(mde_grid(n * 64, MDE_BLOCK, 4096)), dim3(MDE_BLOCK), 0, st, n, nf,
                       nnz, indptr, indices, flag);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpyAsync(&bad, flag, sizeof(int), hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  (void)hipFree(flag);
  if (e != hipSuccess) return mde_hip_fail(e, "CSR validation", __FILE__, __LINE__);
  if (bad) {
    mde_set_error("%s: malformed CSR (need indptr[0] == 0, indptr non-decreasing, indptr[n] == nnz, "
                  "0 <= column < nf, columns strictly increasing within a row)", who);
    return MDE_E_INVALID;
  }
  return MDE_OK;
}

extern "C" int mde_sparse_validate(int64_t n, int32_t nf, int64_t nnz, const int64_t* indptr,
                                   const int32_t* indices, const float* values, void* stream) {
  return spk_validate("mde_sparse_validate", n, nf, nnz, indptr, indices, values, mde_stream(stream));
}

// ------------------------------------------------------------------ row squared norms
__global__ __launch_bounds__(MDE_BLOCK) void k_sparse_sqnorm(int64_t n, const int64_t* __restrict__ indptr,
                                                             const float* __restrict__ values,
                                                             float* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int64_t w0 = ((int64_t)blockIdx.x * MDE_BLOCK + threadIdx.x) >> 6;
  const int64_t nw = ((int64_t)gridDim.x * MDE_BLOCK) >> 6;
  for (int64_t r = w0; r < n; r += nw) {
    float s = 0.0f;
    for (int64_t e = indptr[r] + lane; e < indptr[r + 1]; e += 64) {
      const float v = values[e];
      s = fmaf(v, v, s);
    }
    s = mde_wave_sum(s);
    if (lane == 0) out[r] = s;
  }
}

// ------------------------------------------------------------------ exact k-NN
__global__ __launch_bounds__(MDE_BLOCK) void k_sparse_knn(int n, int nf, int k, int W,
                                                          const int64_t* __restrict__ indptr,
                                                          const int32_t* __restrict__ indices,
                                                          const float* __restrict__ values,
                                                          const float* __restrict__ sqn,
                                                          int32_t* __restrict__ idx_out,
                                                          float* __restrict__ d2_out) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* P = lds;                                  // [W][SPK_Q] panel; after the last window, the d2 half-tile
  // byte offset of this lane's query pair in panel row off: ((off << 6 | (off & 63)) << 3) ^ (lane << 3)
  const char* pbase = reinterpret_cast<const char*>(lds);
  float* bestd = P + (size_t)W * SPK_Q;            // [SPK_Q][k]
  int* besti = reinterpret_cast<int*>(bestd + SPK_Q * k);  // [SPK_Q][k]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lane8 = lane << 3;
  const int row0 = blockIdx.x * SPK_Q;
  for (int i = tid; i < SPK_Q * k; i += MDE_BLOCK) {
    bestd[i] = FLT_MAX;
    besti[i] = -1;
  }
  for (int i = tid; i < W * SPK_Q; i += MDE_BLOCK) P[i] = 0.0f;
  float worst = FLT_MAX;                           // thread t < SPK_Q: current k-th best of query t
  // panel columns of this wave: lane l < 32 keeps the entry range of query row row0 + 32 wave + l
  const int qr = row0 + wave * 32 + (lane & 31);
  const int64_t qbeg = (lane < 32 && qr < n) ? indptr[qr] : 0;
  const int64_t qend = (lane < 32 && qr < n) ? indptr[qr + 1] : 0;
  // the two queries of this lane in the distance tile
  const int qa = row0 + 2 * lane, qb = qa + 1;
  const float sqa = qa < n ? sqn[qa] : 0.0f, sqb = qb < n ? sqn[qb] : 0.0f;

  // scatter back to zero the entries [qprev, qcur) of the wave's rows, put there from window wprev
  auto clear_rows = [&](int64_t qprev, int64_t qcur, int wprev) {
    for (int r = 0; r < 32; ++r) {
      const int q = wave * 32 + r;
      const int64_t c1 = spk_readlane64(qcur, r);
      for (int64_t e = spk_readlane64(qprev, r) + lane; e < c1; e += 64) P[spk_pidx(indices[e] - wprev, q)] = 0.0f;
    }
  };

  __syncthreads();
  for (int col0 = 0; col0 < n; col0 += SPK_C) {
    const int cr = col0 + wave * SPK_CW + (lane & 31);
    int64_t ccur = (lane < 32 && cr < n) ? indptr[cr] : 0;   // lane c < 32: cursor of candidate c of the wave
    const int64_t cend = (lane < 32 && cr < n) ? indptr[cr + 1] : 0;
    int64_t qcur = qbeg, qprev = qbeg;
    float2 acc[SPK_CW];
#pragma unroll
    for (int c = 0; c < SPK_CW; ++c) acc[c] = make_float2(0.0f, 0.0f);
    int wprev = 0;
    for (int w0 = 0; w0 < nf; w0 = (nf - w0 > W) ? w0 + W : nf) {
      const int wend = (nf - w0 > W) ? w0 + W : nf;
      // (1) the wave's panel columns: the previous window's entries back to zero, this window's in
      clear_rows(qprev, qcur, wprev);
      for (int r = 0; r < 32; ++r) {
        const int q = wave * 32 + r;
        const int64_t c1 = spk_readlane64(qcur, r), e1 = spk_readlane64(qend, r);
        int64_t c = c1;
        for (;;) {
          const int64_t e = c + lane;
          const int col = e < e1 ? indices[e] : INT_MAX;
          const bool in = col < wend;
          if (in) P[spk_pidx(col - w0, q)] = values[e];
          const int m = __popcll(__ballot(in));
          c += m;
          if (m < 64) break;
        }
        if (lane == r) {
          qprev = c1;
          qcur = c;
        }
      }
      wprev = w0;
      __syncthreads();
      // (2) the wave's candidates against the panel
#pragma unroll
      for (int g = 0; g < SPK_CW; g += SPK_G) {
        int colr[SPK_G];
        float valr[SPK_G];
#pragma unroll
        for (int j = 0; j < SPK_G; ++j) {
          const int64_t e = spk_readlane64(ccur, g + j) + lane, ce = spk_readlane64(cend, g + j);
          colr[j] = e < ce ? indices[e] : INT_MAX;
          valr[j] = e < ce ? values[e] : 0.0f;
        }
#pragma unroll
        for (int j = 0; j < SPK_G; ++j) {
          int64_t cc = spk_readlane64(ccur, g + j);
          const int64_t ce = spk_readlane64(cend, g + j);
          int col = colr[j];
          float val = valr[j];
          float2 a = acc[g + j];
          for (;;) {
            const int m = __popcll(__ballot(col < wend));   // the in-window entries are a prefix
            // four entries per step: their panel reads are in flight together
            int t = 0;
            for (; t + 4 <= m; t += 4) {
              float2 p[4];
              float v[4];
#pragma unroll
              for (int u = 0; u < 4; ++u) {
                const int off = __builtin_amdgcn_readlane(col, t + u) - w0;
                v[u] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(val), t + u));
                p[u] = *reinterpret_cast<const float2*>(pbase + ((((off << 6) | (off & 63)) << 3) ^ lane8));
              }
#pragma unroll
              for (int u = 0; u < 4; ++u) {
                a.x = fmaf(v[u], p[u].x, a.x);
                a.y = fmaf(v[u], p[u].y, a.y);
              }
            }
            for (; t < m; ++t) {
              const int off = __builtin_amdgcn_readlane(col, t) - w0;
              const float v = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(val), t));
              const float2 p = *reinterpret_cast<const float2*>(pbase + ((((off << 6) | (off & 63)) << 3) ^ lane8));
              a.x = fmaf(v, p.x, a.x);
              a.y = fmaf(v, p.y, a.y);
            }
            cc += m;
            if (m < 64) break;
            const int64_t e = cc + lane;
            col = e < ce ? indices[e] : INT_MAX;
            val = e < ce ? values[e] : 0.0f;
          }
          acc[g + j] = a;
          if (lane == g + j) ccur = cc;
        }
      }
      __syncthreads();
    }
    clear_rows(qprev, qcur, wprev);
    __syncthreads();
    // (3) d2 of the tile, parked 64 candidates at a time (waves 2h, 2h + 1) and merged in index order
    float* sD = P;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      if ((wave >> 1) == h) {
#pragma unroll
        for (int c = 0; c < SPK_CW; ++c) {
          const int gc = col0 + wave * SPK_CW + c, lc = (wave & 1) * SPK_CW + c;
          const float sqc = gc < n ? sqn[gc] : 0.0f;
          float da = FLT_MAX, db = FLT_MAX;
          if (gc < n && qa < n && qa != gc) da = fmaxf(sqa + sqc - 2.0f * acc[c].x, 0.0f);
          if (gc < n && qb < n && qb != gc) db = fmaxf(sqb + sqc - 2.0f * acc[c].y, 0.0f);
          sD[(2 * lane) * SPK_DS + lc] = da;
          sD[(2 * lane + 1) * SPK_DS + lc] = db;
        }
      }
      __syncthreads();
      if (tid < SPK_Q)
        mde_topk_merge(sD + tid * SPK_DS, 64, col0 + h * 64, k, bestd + tid * k, besti + tid * k, worst);
      __syncthreads();
    }
    for (int i = tid; i < SPK_Q * SPK_DS; i += MDE_BLOCK) sD[i] = 0.0f;
    __syncthreads();
  }
  for (int i = tid; i < SPK_Q * k; i += MDE_BLOCK) {
    const int r = i / k, gr = row0 + r;
    if (gr < n) {
      idx_out[(int64_t)gr * k + (i % k)] = besti[i];
      d2_out[(int64_t)gr * k + (i % k)] = bestd[i];
    }
  }
}

// panel width W for a given k and feature count: as wide as two workgroups per CU allow (80 KiB each),
// else one (160 KiB); never wider than the features need, never narrower than the parked d2 half-tile
static int spk_window(int k, int nf, size_t* lds_bytes) {
  const int topk = SPK_Q * k * 8;
  int W = ((80 * 1024 - topk) / (SPK_Q * 4)) & ~7;
  if (W < SPK_MIN_W) W = ((160 * 1024 - topk) / (SPK_Q * 4)) & ~7;
  if (nf < W) {                                    // (nf + 7 is formed only here: nf may be 2^31 - 1)
    const int need = (nf + 7) & ~7;
    if (need < W) W = need < SPK_MIN_W ? SPK_MIN_W : need;
  }
  *lds_bytes = (size_t)W * SPK_Q * 4 + (size_t)topk;
  return W;
}

extern "C" int32_t mde_sparse_knn_window(int32_t k, int32_t nf) {
  if (k <= 0 || k > KNN_MAXK || nf <= 0) {
    mde_set_error("mde_sparse_knn_window: invalid arguments (1 <= k <= %d, nf >= 1)", KNN_MAXK);
    return MDE_E_INVALID;
  }
  size_t lds = 0;
  return spk_window(k, nf, &lds);
}

extern "C" int mde_sparse_knn(int64_t n, int32_t nf, int64_t nnz, const int64_t* indptr, const int32_t* indices,
                              const float* values, int32_t k, int32_t* idx_out, float* d2_out, float* sqn_work,
                              void* stream) {
  if (k <= 0 || k > KNN_MAXK || !idx_out || !d2_out || !sqn_work) {
    mde_set_error("mde_sparse_knn: invalid arguments (1 <= k <= %d)", KNN_MAXK);
    return MDE_E_INVALID;
  }
  hipStream_t st = mde_stream(stream);
  const int rc = spk_validate("mde_sparse_knn", n, nf, nnz, indptr, indices, values, st);
  if (rc != MDE_OK) return rc;
  hipLaunchKernelGGL(k_sparse_sqnorm, dim3(mde_grid(n * 64, MDE_BLOCK, 4096)), dim3(MDE_BLOCK), 0, st, n, indptr,
                     values, sqn_work);
  MDE_LAUNCH_CHECK();
  size_t lds = 0;
  const int W = spk_window(k, nf, &lds);
  const int rc_lds = knn_raise_lds_limit<k_sparse_knn>(160 * 1024);
  if (rc_lds != MDE_OK) return rc_lds;
  hipLaunchKernelGGL(k_sparse_knn, dim3((unsigned)((n + SPK_Q - 1) / SPK_Q)), dim3(MDE_BLOCK), lds, st, (int)n,
                     (int)nf, (int)k, W, indptr, indices, values, sqn_work, idx_out, d2_out);
  MDE_LAUNCH_CHECK();
  return MDE_OK;
}

// ------------------------------------------------------------------ pair distances
// first position in cols[lo, hi) holding a column >= f
__device__ __forceinline__ int64_t spk_lower_bound(const int32_t* __restrict__ cols, int64_t lo, int64_t hi, int f) {
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (cols[mid] < f) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

__global__ __launch_bounds__(MDE_BLOCK) void k_sparse_pair_dist(int64_t n, int64_t p, const int64_t* __restrict__ edges,
                                                                const int64_t* __restrict__ indptr,
                                                                const int32_t* __restrict__ indices,
                                                                const float* __restrict__ values,
                                                                float* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int64_t w0 = ((int64_t)blockIdx.x * MDE_BLOCK + threadIdx.x) >> 6;
  const int64_t nw = ((int64_t)gridDim.x * MDE_BLOCK) >> 6;
  for (int64_t q = w0; q < p; q += nw) {
    const int64_t i = edges[2 * q], j = edges[2 * q + 1];
    if (i < 0 || i >= n || j < 0 || j >= n) {
      if (lane == 0) out[q] = __int_as_float(0x7fc00000);   // NaN: endpoint out of range
      continue;
    }
    const int64_t ai = indptr[i], bi = indptr[i + 1], aj = indptr[j], bj = indptr[j + 1];
    double s = 0.0;
    for (int64_t e = ai + lane; e < bi; e += 64) {
      const int f = indices[e];
      const int64_t t = spk_lower_bound(indices, aj, bj, f);
      const float b = (t < bj && indices[t] == f) ? values[t] : 0.0f;
      const double d = (double)values[e] - (double)b;
      s += d * d;
    }
    for (int64_t e = aj + lane; e < bj; e += 64) {
      const int f = indices[e];
      const int64_t t = spk_lower_bound(indices, ai, bi, f);
      if (!(t < bi && indices[t] == f)) {
        const double b = values[e];
        s += b * b;
      }
    }
    s = mde_wave_sum(s);
    if (lane == 0) out[q] = (float)sqrt(s);
  }
}

extern "C" int mde_sparse_distances(int64_t n, int32_t nf, int64_t nnz, const int64_t* indptr,
                                    const int32_t* indices, const float* values, int64_t p,
                                    const int64_t* edges, float* out, void* stream) {
  if (p < 0 || (p > 0 && (!edges || !out))) {
    mde_set_error("mde_sparse_distances: invalid arguments (p >= 0, non-null edges / out)");
    return MDE_E_INVALID;
  }
  hipStream_t st = mde_stream(stream);
  const int rc = spk_validate("mde_sparse_distances", n, nf, nnz, indptr, indices, values, st);
  if (rc != MDE_OK || p == 0) return rc;
  hipLaunchKernelGGL(k_sparse_pair_dist, dim3(mde_grid(p * 64, MDE_BLOCK, 8192)), dim3(MDE_BLOCK), 0, st, n, p,
                     edges, indptr, indices, values, out);
  MDE_LAUNCH_CHECK();
  return MDE_OK;
}

// ------------------------------------------------------------------ unit rows (cosine)
// values_out[e] = values[e] / |row of e| (one wave per row, the norm summed in double): the Euclidean
// kernels above then rank by cosine, d2 = 2 (1 - cos), and the sparsity pattern is kept.  A row without a
// positive norm (empty: explicit zeros are not stored) is counted in deg[0], its index min-reduced into
// deg[1], and its values become zero, never NaN.
__global__ __launch_bounds__(MDE_BLOCK) void k_sparse_rows_normalize(int64_t n, const int64_t* __restrict__ indptr,
                                                                     const float* __restrict__ values,
                                                                     float* __restrict__ out, int* __restrict__ deg) {
  const int lane = threadIdx.x & 63;
  const int64_t w0 = ((int64_t)blockIdx.x * MDE_BLOCK + threadIdx.x) >> 6;
  const int64_t nw = ((int64_t)gridDim.x * MDE_BLOCK) >> 6;
  for (int64_t r = w0; r < n; r += nw) {
    const int64_t lo = indptr[r], hi = indptr[r + 1];
    double q = 0.0;
    for (int64_t e = lo + lane; e < hi; e += 64) {
      const double v = values[e];
      q += v * v;
    }
    q = mde_wave_sum(q);
    const bool bad = !(q > 0.0) || !(q < 1.0e300);
    const float inv = bad ? 0.0f : (float)(1.0 / sqrt(q));
    for (int64_t e = lo + lane; e < hi; e += 64) out[e] = values[e] * inv;
    if (bad && lane == 0) {
      atomicAdd(deg, 1);
      atomicMin(deg + 1, (int)r);
    }
  }
}

extern "C" int mde_sparse_rows_normalize(int64_t n, int32_t nf, int64_t nnz, const int64_t* indptr,
                                         const int32_t* indices, const float* values, float* values_out,
                                         int32_t* deg_out, void* stream) {
  if (!deg_out || (nnz > 0 && !values_out)) {
    mde_set_error("mde_sparse_rows_normalize: invalid arguments (non-null values_out / deg_out)");
    return MDE_E_INVALID;
  }
  hipStream_t st = mde_stream(stream);
  const int rc = spk_validate("mde_sparse_rows_normalize", n, nf, nnz, indptr, indices, values, st);
  if (rc != MDE_OK) return rc;
  const int32_t init[2] = {0, 0x7fffffff};
  MDE_HIP(hipMemcpyAsync(deg_out, init, sizeof(init), hipMemcpyHostToDevice, st));
  MDE_HIP(hipStreamSynchronize(st));        // `init` lives on this stack
  hipLaunchKernelGGL(k_sparse_rows_normalize, dim3(mde_grid(n * 64, MDE_BLOCK, 4096)), dim3(MDE_BLOCK), 0, st, n,
                     indptr, values, values_out, deg_out);
  MDE_LAUNCH_CHECK();
  return MDE_OK;
}

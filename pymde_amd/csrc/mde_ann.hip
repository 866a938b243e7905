// mde_ann.hip -- approximate k-nearest-neighbour search by an inverted file (IVF) with cluster-level
// probing, and the query-against-base search that builds it (k-means assignment, centroid probe lists,
// the exact check behind the recall estimate).
//   [ref: pymde/preprocess/data_matrix.py:125-143 -- pynndescent above 10 000 items; here an IVF search]
//
// Scan (k_ann_scan).  The query positions are cut into tiles of at most 64 rows; a tile names a probe row,
// whose n_probe entries are lists, and a list is a range of base positions.  A 256-thread workgroup owns
// one tile and walks the base positions of its probed lists 64 at a time.  Both sides are read through
// row maps (position -> row of Q / B), so the data matrix is neither permuted nor copied.  The Gram tile
// is the one of k_knn (mde_knn.hip): each wave accumulates a 32x32 quadrant with v_mfma_f32_32x32x2_f32
// over 32-wide feature chunks staged through LDS, the next chunk's global loads issued before the current
// chunk's MFMAs.  The feature order of every dot product is the same as in k_knn, so a pair's squared
// distance |x|^2 + |y|^2 - 2 x.y comes out bit for bit as the exact kernel computes it.  The tile of
// squared distances is parked in LDS and one thread per query row merges it into the row's top-k list
// by (d2, original index) (mde_topk_merge_id): the order in which lists are probed cannot change the
// output.  Self matches are excluded by original row.
//
// Centroids (k_ann_centroids).  One workgroup per list sums its member rows in membership order into
// double accumulators (member stripes combined in a fixed order): no float atomics, a fixed seed gives
// bit-identical centroids.  An empty list keeps its previous centroid.
#include <float.h>
#include <limits.h>

#include <vector>

#include "mde_common.h"
#include "mde_topk.h"

typedef float f32x16 __attribute__((ext_vector_type(16)));

#define ANN_BM 64
#define ANN_BN 64
#define ANN_KB 32
#define ANN_KBP 33
#define ANN_MAXK 64
#define ANN_STG ((ANN_BM * ANN_KB) / MDE_BLOCK)

__global__ __launch_bounds__(MDE_BLOCK) void k_ann_scan(
    int nf, int k, int flags, const float* __restrict__ Q, const float* __restrict__ q_sqn,
    const int32_t* __restrict__ q_map, const float* __restrict__ B, const float* __restrict__ b_sqn,
    const int32_t* __restrict__ b_map, const int64_t* __restrict__ offsets, int n_probe,
    const int32_t* __restrict__ probe, const int64_t* __restrict__ tiles, int32_t* __restrict__ idx_out,
    float* __restrict__ d2_out) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* sA = lds;                           // [ANN_BM][ANN_KBP]
  float* sB = sA + ANN_BM * ANN_KBP;         // [ANN_BN][ANN_KBP]
  float* sD = sB + ANN_BN * ANN_KBP;         // [ANN_BM][ANN_BN + 1] squared distances of the tile
  float* sQn = sD + ANN_BM * (ANN_BN + 1);   // [ANN_BM] query row norms
  float* sCn = sQn + ANN_BM;                 // [ANN_BN] candidate row norms
  int* sQr = reinterpret_cast<int*>(sCn + ANN_BN);  // [ANN_BM] query rows (original index)
  int* sCr = sQr + ANN_BM;                   // [ANN_BN] candidate rows (original index)
  float* bestd = reinterpret_cast<float*>(sCr + ANN_BN);   // [ANN_BM][k]
  int* besti = reinterpret_cast<int*>(bestd + ANN_BM * k);  // [ANN_BM][k]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wi = wave >> 1, wj = wave & 1;   // quadrant of the 64x64 tile
  const int li = lane & 31, lk = lane >> 5;
  const int64_t q_lo = tiles[3 * (int64_t)blockIdx.x], q_hi = tiles[3 * (int64_t)blockIdx.x + 1];
  const int64_t plist = tiles[3 * (int64_t)blockIdx.x + 2];
  const int nq = (int)(q_hi - q_lo);
  const bool exclude_self = flags & 1, scatter = flags & 2;
  if (tid < ANN_BM) {
    const int64_t pos = q_lo + (tid < nq ? tid : 0);
    const int row = q_map ? q_map[pos] : (int)pos;
    sQr[tid] = row;
    sQn[tid] = q_sqn[row];
  }
  for (int i = tid; i < ANN_BM * k; i += MDE_BLOCK) {
    bestd[i] = FLT_MAX;
    besti[i] = -1;
  }
  __syncthreads();
  // the rows this thread stages: r = (tid >> 5) + 8 q; rows past the tile read row 0 of it and are zeroed
  const int c_stage = tid & 31;
  const float* qrow[ANN_STG];
#pragma unroll
  for (int q = 0; q < ANN_STG; ++q) qrow[q] = Q + (int64_t)sQr[(tid >> 5) + 8 * q] * nf;
  float worst_d = FLT_MAX;                   // thread t < 64: current k-th best (d2, index) of query t
  int worst_i = -1;
  // candidate blocks in probe order: (p, col0) walks the lists' ranges 64 positions at a time.  The row
  // ids and norms of the next block are loaded (threads < 64, into registers) while the current one is
  // computed, so the two dependent loads (map, then norm) are off the critical path.
  int p = 0;
  int64_t col0 = 0, c_hi = 0;
  auto advance = [&](int& pp, int64_t& c0, int64_t& ch) {   // to the next non-empty block; pp = n_probe: done
    c0 += ANN_BN;
    while (c0 >= ch && pp < n_probe) {
      if (++pp >= n_probe) break;
      const int list = probe[plist * n_probe + pp];
      c0 = offsets[list];
      ch = offsets[list + 1];
    }
  };
  {
    const int list = probe[plist * n_probe];
    col0 = offsets[list];
    c_hi = offsets[list + 1];
    if (col0 >= c_hi) {
      col0 -= ANN_BN;
      advance(p, col0, c_hi);
    }
  }
  int nx_row = 0;
  float nx_norm = 0.0f;
  auto prefetch = [&](int pp, int64_t c0, int64_t ch) {
    if (tid < ANN_BN && pp < n_probe) {
      const int64_t pos = c0 + (c0 + tid < ch ? tid : 0);
      nx_row = b_map ? b_map[pos] : (int)pos;
      nx_norm = b_sqn[nx_row];
    }
  };
  prefetch(p, col0, c_hi);
  while (p < n_probe) {
    {
      const int nc = (int)(c_hi - col0 < ANN_BN ? c_hi - col0 : ANN_BN);
      __syncthreads();                       // the previous tile's merge is done with sCr / sD
      if (tid < ANN_BN) {
        sCr[tid] = nx_row;
        sCn[tid] = nx_norm;
      }
      __syncthreads();
      int np = p;
      int64_t ncol0 = col0, nc_hi = c_hi;
      advance(np, ncol0, nc_hi);
      prefetch(np, ncol0, nc_hi);
      const float* crow[ANN_STG];
#pragma unroll
      for (int q = 0; q < ANN_STG; ++q) crow[q] = B + (int64_t)sCr[(tid >> 5) + 8 * q] * nf;
      f32x16 acc;
#pragma unroll
      for (int q = 0; q < 16; ++q) acc[q] = 0.0f;
      float ra[ANN_STG], rb[ANN_STG];
      auto fetch = [&](int k0) {
#pragma unroll
        for (int q = 0; q < ANN_STG; ++q) {
          const int r = (tid >> 5) + 8 * q, f = k0 + c_stage;
          const int fc = f < nf ? f : nf - 1;
          const float va = qrow[q][fc];
          const float vb = crow[q][fc];
          ra[q] = (r < nq && f < nf) ? va : 0.0f;
          rb[q] = (r < nc && f < nf) ? vb : 0.0f;
        }
      };
      fetch(0);
      for (int k0 = 0; k0 < nf; k0 += ANN_KB) {
        __syncthreads();
#pragma unroll
        for (int q = 0; q < ANN_STG; ++q) {
          const int r = (tid >> 5) + 8 * q;
          sA[r * ANN_KBP + c_stage] = ra[q];
          sB[r * ANN_KBP + c_stage] = rb[q];
        }
        __syncthreads();
        if (k0 + ANN_KB < nf) fetch(k0 + ANN_KB);
        const float* pa = sA + (wi * 32 + li) * ANN_KBP + lk;
        const float* pb = sB + (wj * 32 + li) * ANN_KBP + lk;
#pragma unroll
        for (int kk = 0; kk < ANN_KB; kk += 2)
          acc = __builtin_amdgcn_mfma_f32_32x32x2f32(pa[kk], pb[kk], acc, 0, 0, 0);
      }
      // C/D map of the 32x32 tile: col = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const int r = wi * 32 + (q & 3) + 8 * (q >> 2) + 4 * lk;
        const int c = wj * 32 + li;
        float d2 = FLT_MAX;
        if (r < nq && c < nc && !(exclude_self && sQr[r] == sCr[c]))
          d2 = fmaxf(sQn[r] + sCn[c] - 2.0f * acc[q], 0.0f);
        sD[r * (ANN_BN + 1) + c] = d2;
      }
      __syncthreads();
      if (tid < nq)
        mde_topk_merge_id(sD + tid * (ANN_BN + 1), sCr, nc, k, bestd + tid * k, besti + tid * k, worst_d,
                          worst_i);
      p = np;
      col0 = ncol0;
      c_hi = nc_hi;
    }
  }
  __syncthreads();
  for (int i = tid; i < ANN_BM * k; i += MDE_BLOCK) {
    const int r = i / k;
    if (r < nq) {
      const int64_t orow = scatter ? (int64_t)sQr[r] : q_lo + r;
      idx_out[orow * k + (i % k)] = besti[i];
      d2_out[orow * k + (i % k)] = bestd[i];
    }
  }
}

// One workgroup per list: centroid = mean of the member rows, summed in membership order.  Threads are
// (feature f, member stripe s); each stripe sums members s, s + S, ... and the stripes are added in order.
__global__ __launch_bounds__(MDE_BLOCK) void k_ann_centroids(int nf, const float* __restrict__ X,
                                                             const int32_t* __restrict__ members,
                                                             const int64_t* __restrict__ offsets,
                                                             float* __restrict__ centroids, int fw) {
  __shared__ double part[MDE_BLOCK];
  const int64_t lo = offsets[blockIdx.x], hi = offsets[blockIdx.x + 1];
  if (hi <= lo) return;                      // an empty list keeps its previous centroid
  const int tid = threadIdx.x, fl = tid % fw, s = tid / fw, S = MDE_BLOCK / fw;
  const double inv = 1.0 / (double)(hi - lo);
  for (int f0 = 0; f0 < nf; f0 += fw) {
    const int f = f0 + fl;
    double acc = 0.0;
    if (f < nf && s < S)
      for (int64_t m = lo + s; m < hi; m += S) acc += (double)X[(int64_t)members[m] * nf + f];
    part[tid] = acc;
    __syncthreads();
    if (tid < fw && f < nf) {
      double t = 0.0;
      for (int j = 0; j < S; ++j) t += part[j * fw + tid];
      centroids[(int64_t)blockIdx.x * nf + f] = (float)(t * inv);
    }
    __syncthreads();
  }
}

// ------------------------------------------------------------------ host side
namespace {

template <typename T>
int ann_fetch(std::vector<T>& h, const T* d, int64_t count, hipStream_t st) {
  h.resize((size_t)count);
  if (count > 0) MDE_HIP(hipMemcpyAsync(h.data(), d, sizeof(T) * (size_t)count, hipMemcpyDeviceToHost, st));
  MDE_HIP(hipStreamSynchronize(st));
  return MDE_OK;
}

int ann_invalid(const char* what) {
  mde_set_error("mde_ann: invalid arguments (%s)", what);
  return MDE_E_INVALID;
}

// offsets [n_lists + 1]: offsets[0] >= 0, non-decreasing, offsets[n_lists] <= n_pos
int ann_check_offsets(const int64_t* offsets, int64_t n_lists, int64_t n_pos, hipStream_t st) {
  std::vector<int64_t> h;
  int rc = ann_fetch(h, offsets, n_lists + 1, st);
  if (rc != MDE_OK) return rc;
  if (h[0] < 0 || h[(size_t)n_lists] > n_pos) return ann_invalid("offsets outside the positions");
  for (int64_t i = 0; i < n_lists; ++i)
    if (h[(size_t)i + 1] < h[(size_t)i]) return ann_invalid("offsets not monotone");
  return MDE_OK;
}

// every entry of a row map in [0, n_rows)
int ann_check_map(const int32_t* map, int64_t n_pos, int64_t n_rows, hipStream_t st) {
  if (!map) return n_pos <= n_rows ? MDE_OK : ann_invalid("more positions than rows without a row map");
  std::vector<int32_t> h;
  int rc = ann_fetch(h, map, n_pos, st);
  if (rc != MDE_OK) return rc;
  for (int32_t v : h)
    if (v < 0 || v >= n_rows) return ann_invalid("row map entry out of range");
  return MDE_OK;
}

}  // namespace

extern "C" int mde_ann_search(int32_t nf, int32_t k, int32_t flags, int64_t n_q, const float* Q,
                              const float* q_sqn, int64_t n_qpos, const int32_t* q_map, int64_t n_b,
                              const float* B, const float* b_sqn, int64_t n_bpos, const int32_t* b_map,
                              int64_t n_lists, const int64_t* offsets, int32_t n_probe, const int32_t* probe,
                              int64_t n_tiles, const int64_t* tiles, int32_t* idx_out, float* d2_out,
                              void* stream) {
  if (!Q || !q_sqn || !B || !b_sqn || !offsets || !probe || !tiles || !idx_out || !d2_out)
    return ann_invalid("null pointer");
  if (k < 1 || k > ANN_MAXK) {
    mde_set_error("mde_ann_search: invalid arguments (1 <= k <= %d)", ANN_MAXK);
    return MDE_E_INVALID;
  }
  if (nf < 1 || n_q < 1 || n_b < 1 || n_qpos < 0 || n_bpos < 0 || n_lists < 1 || n_probe < 1 || n_tiles < 0 ||
      (flags & ~3))
    return ann_invalid("sizes");
  if (n_q >= ((int64_t)1 << 31) || n_b >= ((int64_t)1 << 31) || n_qpos >= ((int64_t)1 << 31) ||
      n_bpos >= ((int64_t)1 << 31) || n_lists >= ((int64_t)1 << 31) || n_tiles >= ((int64_t)1 << 31))
    return MDE_E_TOO_LARGE;
  hipStream_t st = mde_stream(stream);
  int rc = ann_check_offsets(offsets, n_lists, n_bpos, st);
  if (rc != MDE_OK) return rc;
  {
    std::vector<int32_t> h;
    if ((rc = ann_fetch(h, probe, n_lists * (int64_t)n_probe, st)) != MDE_OK) return rc;
    for (int32_t v : h)
      if (v < 0 || v >= n_lists) return ann_invalid("probe list id out of range");
  }
  {
    std::vector<int64_t> h;
    if ((rc = ann_fetch(h, tiles, 3 * n_tiles, st)) != MDE_OK) return rc;
    for (int64_t t = 0; t < n_tiles; ++t) {
      const int64_t lo = h[3 * t], hi = h[3 * t + 1], l = h[3 * t + 2];
      if (lo < 0 || hi <= lo || hi > n_qpos || hi - lo > ANN_BM || l < 0 || l >= n_lists)
        return ann_invalid("query tile");
    }
  }
  if ((rc = ann_check_map(q_map, n_qpos, n_q, st)) != MDE_OK) return rc;
  if (b_map != q_map || n_bpos != n_qpos || n_b != n_q)
    if ((rc = ann_check_map(b_map, n_bpos, n_b, st)) != MDE_OK) return rc;
  if (n_tiles == 0) return MDE_OK;
  const size_t lds = sizeof(float) * (size_t)(ANN_BM * ANN_KBP + ANN_BN * ANN_KBP + ANN_BM * (ANN_BN + 1) +
                                              2 * ANN_BM + 2 * ANN_BN) +
                     (size_t)ANN_BM * k * (sizeof(float) + sizeof(int));
  static bool attr = false;
  if (!attr) {
    MDE_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k_ann_scan),
                                hipFuncAttributeMaxDynamicSharedMemorySize, 96 * 1024));
    attr = true;
  }
  hipLaunchKernelGGL(k_ann_scan, dim3((unsigned)n_tiles), dim3(MDE_BLOCK), lds, st, nf, k, flags, Q, q_sqn,
                     q_map, B, b_sqn, b_map, offsets, n_probe, probe, tiles, idx_out, d2_out);
  MDE_LAUNCH_CHECK();
  return MDE_OK;
}

extern "C" int mde_ann_centroids(int64_t n, int32_t nf, const float* data, int64_t n_members,
                                 const int32_t* members, int64_t n_lists, const int64_t* offsets,
                                 float* centroids, void* stream) {
  if (!data || !members || !offsets || !centroids) return ann_invalid("null pointer");
  if (n < 1 || nf < 1 || n_members < 0 || n_lists < 1) return ann_invalid("sizes");
  if (n >= ((int64_t)1 << 31) || n_lists >= ((int64_t)1 << 31)) return MDE_E_TOO_LARGE;
  hipStream_t st = mde_stream(stream);
  int rc = ann_check_offsets(offsets, n_lists, n_members, st);
  if (rc != MDE_OK) return rc;
  if ((rc = ann_check_map(members, n_members, n, st)) != MDE_OK) return rc;
  int fw = 1;                                // features per pass: the power of two >= nf, at most 256
  while (fw < nf && fw < MDE_BLOCK) fw <<= 1;
  hipLaunchKernelGGL(k_ann_centroids, dim3((unsigned)n_lists), dim3(MDE_BLOCK), 0, st, nf, data, members,
                     offsets, centroids, fw);
  MDE_LAUNCH_CHECK();
  return MDE_OK;
}

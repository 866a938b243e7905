// mde_ann.hip -- approximate k-nearest-neighbour search by an inverted file (IVF) with cluster-level
// probing, and the query-against-base search that builds it (k-means assignment, centroid probe lists,
// the exact check behind the recall estimate).
//   [ref: pymde/preprocess/data_matrix.py:125-143 -- pynndescent above 10 000 items; here an IVF search]
//
// Scan (k_ann_scan).  The query positions are cut into tiles of at most 64 rows; a tile names a probe row,
// whose n_probe entries are lists, and a list is a range of base positions.  A 256-thread workgroup owns
// one tile and walks the base positions of its probed lists 64 at a time.  Both sides are read through
// row maps (position -> row of Q / B), so the data matrix is neither permuted nor copied.  The Gram tile
// and the parked squared distances are those of mde_knn_tile.h, the code the exact kernel (k_knn_cross,
// mde_knn.hip) runs: a pair's |x|^2 + |y|^2 - 2 x.y comes out bit for bit as the exact search computes it.
// One thread per query row merges the parked tile into the row's top-k list by (d2, original index)
// (mde_topk_merge_id): the order in which lists are probed cannot change the output.  Self matches are
// excluded by original row.
//
// Centroids (k_ann_centroids).  One workgroup per list sums its member rows in membership order into
// double accumulators (member stripes combined in a fixed order): no float atomics, a fixed seed gives
// bit-identical centroids.  An empty list keeps its previous centroid.
#include <float.h>
#include <limits.h>

#include <vector>

#include "mde_knn_tile.h"

#define ANN_EXTRA (2 * KNN_BM + 2 * KNN_BN)   // floats of the kernel's own LDS block: norms and rows of a tile

__global__ __launch_bounds__(MDE_BLOCK) void k_ann_scan(
    int nf, int k, int flags, const float* __restrict__ Q, const float* __restrict__ q_sqn,
    const int32_t* __restrict__ q_map, const float* __restrict__ B, const float* __restrict__ b_sqn,
    const int32_t* __restrict__ b_map, const int64_t* __restrict__ offsets, int n_probe,
    const int32_t* __restrict__ probe, const int64_t* __restrict__ tiles, int32_t* __restrict__ idx_out,
    float* __restrict__ d2_out) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const knn_tile_lds s = knn_tile_carve(lds, k, ANN_EXTRA);
  float* sQn = s.extra;                      // [KNN_BM] query row norms
  float* sCn = sQn + KNN_BM;                 // [KNN_BN] candidate row norms
  int* sQr = reinterpret_cast<int*>(sCn + KNN_BN);  // [KNN_BM] query rows (original index)
  int* sCr = sQr + KNN_BM;                   // [KNN_BN] candidate rows (original index)
  const int tid = threadIdx.x;
  const int64_t q_lo = tiles[3 * (int64_t)blockIdx.x], q_hi = tiles[3 * (int64_t)blockIdx.x + 1];
  const int64_t plist = tiles[3 * (int64_t)blockIdx.x + 2];
  const int nq = (int)(q_hi - q_lo);
  const bool exclude_self = flags & 1, scatter = flags & 2;
  if (tid < KNN_BM) {
    const int64_t pos = q_lo + (tid < nq ? tid : 0);
    const int row = q_map ? q_map[pos] : (int)pos;
    sQr[tid] = row;
    sQn[tid] = q_sqn[row];
  }
  knn_lists_init(s.bestd, s.besti, KNN_BM * k);
  __syncthreads();
  // the rows this thread stages: r = (tid >> 5) + 8 q; rows past the tile read row 0 of it and are zeroed
  const float* qrow[KNN_STG];
  bool qok[KNN_STG];
#pragma unroll
  for (int q = 0; q < KNN_STG; ++q) {
    qrow[q] = Q + (int64_t)sQr[(tid >> 5) + 8 * q] * nf;
    qok[q] = (tid >> 5) + 8 * q < nq;
  }
  float worst_d = FLT_MAX;                   // thread t < 64: current k-th best (d2, index) of query t
  int worst_i = -1;
  // candidate blocks in probe order: (p, col0) walks the lists' ranges 64 positions at a time.  The row
  // ids and norms of the next block are loaded (threads < 64, into registers) while the current one is
  // computed, so the two dependent loads (map, then norm) are off the critical path.
  int p = 0;
  int64_t col0 = 0, c_hi = 0;
  auto advance = [&](int& pp, int64_t& c0, int64_t& ch) {   // to the next non-empty block; pp = n_probe: done
    c0 += KNN_BN;
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
      col0 -= KNN_BN;
      advance(p, col0, c_hi);
    }
  }
  int nx_row = 0;
  float nx_norm = 0.0f;
  auto prefetch = [&](int pp, int64_t c0, int64_t ch) {
    if (tid < KNN_BN && pp < n_probe) {
      const int64_t pos = c0 + (c0 + tid < ch ? tid : 0);
      nx_row = b_map ? b_map[pos] : (int)pos;
      nx_norm = b_sqn[nx_row];
    }
  };
  prefetch(p, col0, c_hi);
  while (p < n_probe) {
    {
      const int nc = (int)(c_hi - col0 < KNN_BN ? c_hi - col0 : KNN_BN);
      __syncthreads();                       // the previous tile's merge is done with sCr / sD
      if (tid < KNN_BN) {
        sCr[tid] = nx_row;
        sCn[tid] = nx_norm;
      }
      __syncthreads();
      int np = p;
      int64_t ncol0 = col0, nc_hi = c_hi;
      advance(np, ncol0, nc_hi);
      prefetch(np, ncol0, nc_hi);
      const float* crow[KNN_STG];
      bool cok[KNN_STG];
#pragma unroll
      for (int q = 0; q < KNN_STG; ++q) {
        crow[q] = B + (int64_t)sCr[(tid >> 5) + 8 * q] * nf;
        cok[q] = (tid >> 5) + 8 * q < nc;
      }
      const f32x16 acc = knn_gram_tile(s.sA, s.sB, nf, qrow, qok, crow, cok);
      knn_park_tile(
          s.sD, acc, [&](int r, int c) { return r < nq && c < nc && !(exclude_self && sQr[r] == sCr[c]); },
          [&](int r) { return sQn[r]; }, [&](int c) { return sCn[c]; });
      __syncthreads();
      if (tid < nq)
        mde_topk_merge_id(s.sD + tid * (KNN_BN + 1), sCr, nc, k, s.bestd + tid * k, s.besti + tid * k, worst_d,
                          worst_i);
      p = np;
      col0 = ncol0;
      c_hi = nc_hi;
    }
  }
  __syncthreads();
  // row by row, not knn_lists_store: under `scatter` a tile's rows are not consecutive in the outputs
  for (int i = tid; i < KNN_BM * k; i += MDE_BLOCK) {
    const int r = i / k;
    if (r < nq) {
      const int64_t orow = scatter ? (int64_t)sQr[r] : q_lo + r;
      idx_out[orow * k + (i % k)] = s.besti[i];
      d2_out[orow * k + (i % k)] = s.bestd[i];
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
  if (k < 1 || k > KNN_MAXK) {
    mde_set_error("mde_ann_search: invalid arguments (1 <= k <= %d)", KNN_MAXK);
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
      if (lo < 0 || hi <= lo || hi > n_qpos || hi - lo > KNN_BM || l < 0 || l >= n_lists)
        return ann_invalid("query tile");
    }
  }
  if ((rc = ann_check_map(q_map, n_qpos, n_q, st)) != MDE_OK) return rc;
  if (b_map != q_map || n_bpos != n_qpos || n_b != n_q)
    if ((rc = ann_check_map(b_map, n_bpos, n_b, st)) != MDE_OK) return rc;
  if (n_tiles == 0) return MDE_OK;
  if ((rc = knn_raise_lds_limit<k_ann_scan>(96 * 1024)) != MDE_OK) return rc;
  hipLaunchKernelGGL(k_ann_scan, dim3((unsigned)n_tiles), dim3(MDE_BLOCK), knn_tile_lds_bytes(k, ANN_EXTRA), st, nf, k,
                     flags, Q, q_sqn, q_map, B, b_sqn, b_map, offsets, n_probe, probe, tiles, idx_out, d2_out);
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

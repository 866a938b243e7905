// mde_knn_slices.h -- the corpus split of the query-against-corpus searches, written once: the automatic
// slice rule and the kernel that folds the per-slice lists, shared by mde_knn_cross (mde_knn.hip, the 64x64 f32
// tile) and mde_knn_bf16 (mde_knn_bf16.hip, the 128x128 bf16 tile).
#pragma once
#include "mde_knn_tile.h"

// Folds the `slices` sorted lists of every query row ([slices, n_q, k], empty slots FLT_MAX / -1) into the
// row's top-k by (d2, index).  A workgroup owns 64 query rows: their 64 k entries of one slice are
// contiguous, are staged through LDS by all threads, and one thread per row merges them.
static __global__ __launch_bounds__(MDE_BLOCK) void k_knn_cross_merge(int n_q, int k, int slices,
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
  knn_lists_init(bestd, besti, KNN_BM * k);
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
  knn_lists_store(bestd, besti, rows * k, idx_out + row0 * k, d2_out + row0 * k);
}
static inline size_t knn_cross_merge_lds_bytes(int k) {
  return (size_t)KNN_BM * k * 2 * (sizeof(float) + sizeof(int));
}

// The automatic slice count (slices == 0) of a search whose workgroups own bm query rows and take the corpus
// bn columns at a time.  Rule: when the query blocks alone give every CU a workgroup (query blocks >= CUs)
// the corpus is not split; otherwise it is split so that the grid holds about CROSS_GRID_PER_CU workgroups
// per CU, but no finer than CROSS_MIN_TILES column tiles per slice (a slice must amortise its list's k
// entries of merge work and its start-up).  Both constants are unmeasured choices until
// tools/cross_knn_scale.py has run on the device (profiles/r09_cross_knn.txt).
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
static int64_t cross_auto_slices(int64_t n_q, int64_t n_c, int cus, int bm = KNN_BM, int bn = KNN_BN) {
  const int64_t qb = (n_q + bm - 1) / bm, tiles = (n_c + bn - 1) / bn;
  if (qb >= cus) return 1;
  int64_t s = ((int64_t)CROSS_GRID_PER_CU * cus + qb - 1) / qb;
  if (s > tiles / CROSS_MIN_TILES) s = tiles / CROSS_MIN_TILES;
  if (s > CROSS_MAX_SLICES) s = CROSS_MAX_SLICES;
  return s < 1 ? 1 : s;
}
// slices as given, or the automatic count for 0; a negative MDE_E_* code on failure
static int64_t cross_resolve_slices(int64_t n_q, int64_t n_c, int32_t slices, int bm = KNN_BM, int bn = KNN_BN) {
  if (slices != 0) return slices;
  int cus = 0;
  const int rc = cross_cu_count(&cus);
  if (rc != MDE_OK) return rc;
  return cross_auto_slices(n_q, n_c, cus, bm, bn);
}
static bool cross_args_ok(int64_t n_q, int64_t n_c, int32_t k, int32_t slices) {
  return n_q > 0 && n_c > 0 && k > 0 && k <= KNN_MAXK && slices >= 0 && slices <= CROSS_MAX_SLICES;
}

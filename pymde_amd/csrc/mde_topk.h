// mde_topk.h -- the per-row top-k merges of the five k-NN kernels: by arrival order (mde_topk_merge) in
// k_knn_cross (mde_knn.hip), k_knn_l1 (mde_metric.hip) and k_sparse_knn (mde_sparse.hip), by (d2, index)
// (mde_topk_merge_id) in k_ann_scan (mde_ann.hip) and k_knn_cross_merge (mde_knn.hip).
#pragma once
#include "mde_common.h"

// One thread merges a parked tile row of `ncand` squared distances (candidate c has index c0 + c) into
// its row's sorted top-k list (bd ascending, bi the indices).  `worst` is the current k-th best and is
// kept in a register by the caller between tiles.  A candidate enters only when strictly below the
// k-th best and is inserted behind every equal distance: with candidates offered in increasing index
// order, ties resolve to the smaller index (the order of a stable argsort).
__device__ __forceinline__ void mde_topk_merge(const float* __restrict__ sd, int ncand, int c0, int k,
                                               float* __restrict__ bd, int* __restrict__ bi, float& worst) {
  for (int c = 0; c < ncand; ++c) {
    const float d2 = sd[c];
    if (d2 < worst) {
      int pos = k - 1;
      while (pos > 0 && bd[pos - 1] > d2) {
        bd[pos] = bd[pos - 1];
        bi[pos] = bi[pos - 1];
        --pos;
      }
      bd[pos] = d2;
      bi[pos] = c0 + c;
      worst = bd[k - 1];
    }
  }
}

// The merge of the approximate search (mde_ann.hip): candidate c has original index ids[c] and the list is
// ordered by (d2, index), so the result does not depend on the order in which candidates are offered.
// Entries of FLT_MAX are empty (padding, self) and never enter.  (worst_d, worst_i) is the k-th entry.
__device__ __forceinline__ void mde_topk_merge_id(const float* __restrict__ sd, const int* __restrict__ ids,
                                                  int ncand, int k, float* __restrict__ bd, int* __restrict__ bi,
                                                  float& worst_d, int& worst_i) {
  for (int c = 0; c < ncand; ++c) {
    const float d2 = sd[c];
    if (d2 >= 3.402823466e+38f) continue;
    const int id = ids[c];
    if (d2 < worst_d || (d2 == worst_d && id < worst_i)) {
      int pos = k - 1;
      while (pos > 0 && (bd[pos - 1] > d2 || (bd[pos - 1] == d2 && bi[pos - 1] > id))) {
        bd[pos] = bd[pos - 1];
        bi[pos] = bi[pos - 1];
        --pos;
      }
      bd[pos] = d2;
      bi[pos] = id;
      worst_d = bd[k - 1];
      worst_i = bi[k - 1];
    }
  }
}

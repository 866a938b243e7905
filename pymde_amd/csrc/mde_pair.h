// mde_pair.h -- what the all-pairs walks over the 64x64 Gram tile share: mde_pair_moments.hip (the sums behind the
// global scores of pymde_amd.quality) and mde_pair_loss.hip (the loss and gradient of a dense MDE
// problem).
#pragma once
#include "mde_knn_tile.h"
#include "mde_knn_slices.h"

#define PAIR_FLT_MAX 3.402823466e+38f
#define PAIR_COLS (KNN_BN / 4)                 // columns of a tile row that one thread walks
#define PAIR_TILE (KNN_BM * (KNN_BN + 1))      // floats of a parked tile

// The distance of a parked squared distance: Euclidean (mode 0), or the cosine / correlation distance of unit rows.
__device__ __forceinline__ float pair_dist(float d2, int mode) { return mode ? 0.5f * d2 : sqrtf(d2); }

static inline bool pair_args_ok(int64_t n, int64_t n_q, int32_t slices) {
  return n >= 2 && n < ((int64_t)1 << 31) && n_q >= 1 && n_q < ((int64_t)1 << 31) && slices >= 0 &&
         slices <= CROSS_MAX_SLICES;
}

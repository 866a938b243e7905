// mde_knn_tile.h -- the 64x64 Gram tile of the Euclidean k-NN kernels and the pieces around it, written once:
// k_knn_cross (mde_knn.hip: the exact self-join and the query-against-corpus search), k_ann_scan
// (mde_ann.hip) and k_knn_rank (mde_knn_rank.hip) are this tile under different walks over the candidates;
// k_knn_l1 (mde_metric.hip) has its own VALU tile and shares the lists and the launcher helper.  The same
// squared distance of single listed pairs, without a tile: knn_wave_pair_d2 at the end.
//
// Squared distances are formed as |x|^2 + |y|^2 - 2 x.y with the Gram tile x.y on the f32 matrix cores
// (v_mfma_f32_32x32x2_f32, exact f32): a 256-thread workgroup owns 64 query rows and takes the candidates
// 64 at a time; each wave accumulates one 32x32 quadrant of the 64x64 tile over the features, staged through
// LDS in 32-wide chunks (rows padded to 33 floats: conflict-free operand reads).  The tile of squared
// distances is parked in LDS and one thread per query row merges its 64 candidates into the row's sorted
// top-k list (mde_topk.h).  Every kernel on this tile sums a dot product in the same feature order and forms
// d2 by the same expression, so a pair's squared distance has the same bits in all of them.
#pragma once
#include "mde_common.h"
#include "mde_topk.h"

#define KNN_BM 64     // query rows of a tile
#define KNN_BN 64     // candidates of a tile
#define KNN_KB 32     // features of a staged chunk
#define KNN_KBP 33    // LDS row stride of a chunk
#define KNN_MAXK 64   // longest neighbour list, of every k-NN kernel (dense, Manhattan, sparse, approximate)
#define KNN_STG ((KNN_BM * KNN_KB) / MDE_BLOCK)   // chunk elements a thread stages per side

// Dynamic LDS of a tile kernel: the two staged chunks, the parked tile, `extra` floats of the kernel's own,
// the lists.
static inline size_t knn_tile_lds_bytes(int k, int extra) {
  return sizeof(float) * (size_t)(KNN_BM * KNN_KBP + KNN_BN * KNN_KBP + KNN_BM * (KNN_BN + 1) + extra) +
         (size_t)KNN_BM * k * (sizeof(float) + sizeof(int));
}

// Raises the dynamic-LDS limit of `Kernel` to `bytes`, once per kernel and process.
template <auto Kernel>
static int knn_raise_lds_limit(int bytes) {
  static bool done = false;
  if (!done) {
    MDE_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                bytes));
    done = true;
  }
  return MDE_OK;
}

typedef float f32x16 __attribute__((ext_vector_type(16)));

struct knn_tile_lds {
  float* sA;      // [KNN_BM][KNN_KBP]
  float* sB;      // [KNN_BN][KNN_KBP]
  float* sD;      // [KNN_BM][KNN_BN + 1] squared distances of the tile
  float* extra;   // [extra] the kernel's own
  float* bestd;   // [KNN_BM][k]
  int* besti;     // [KNN_BM][k]
};
__device__ __forceinline__ knn_tile_lds knn_tile_carve(float* lds, int k, int extra) {
  knn_tile_lds s;
  s.sA = lds;
  s.sB = s.sA + KNN_BM * KNN_KBP;
  s.sD = s.sB + KNN_BN * KNN_KBP;
  s.extra = s.sD + KNN_BM * (KNN_BN + 1);
  s.bestd = s.extra + extra;
  s.besti = reinterpret_cast<int*>(s.bestd + KNN_BM * k);
  return s;
}

// Empty lists: `count` = rows * k entries of FLT_MAX / -1.
__device__ __forceinline__ void knn_lists_init(float* bestd, int* besti, int count) {
  for (int i = threadIdx.x; i < count; i += MDE_BLOCK) {
    bestd[i] = 3.402823466e+38f;
    besti[i] = -1;
  }
}
// The lists of a workgroup's first `count` / k rows to consecutive rows of the [., k] outputs.
__device__ __forceinline__ void knn_lists_store(const float* bestd, const int* besti, int count,
                                                int32_t* __restrict__ idx_out, float* __restrict__ d_out) {
  for (int i = threadIdx.x; i < count; i += MDE_BLOCK) {
    idx_out[i] = besti[i];
    d_out[i] = bestd[i];
  }
}

// One wave's 32x32 quadrant of A . B^T over nf features (all 256 threads call it; it holds barriers).
// Thread tid stages column tid & 31 of the tile rows (tid >> 5) + 8 q, q < KNN_STG, of either side: arow[q] /
// brow[q] point at those rows (any readable row where the tile has none) and aok[q] / bok[q] say whether the
// tile has them.  Feature chunks of KNN_KB: the next chunk's global loads are issued before the MFMAs of the
// current one and committed to LDS after them (register double buffering), so the matrix cores do not wait
// for the staging latency.
__device__ __forceinline__ f32x16 knn_gram_tile(float* sA, float* sB, int nf, const float* const (&arow)[KNN_STG],
                                                const bool (&aok)[KNN_STG], const float* const (&brow)[KNN_STG],
                                                const bool (&bok)[KNN_STG]) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wi = wave >> 1, wj = wave & 1;   // quadrant of the 64x64 tile
  const int li = lane & 31, lk = lane >> 5;
  const int sr = tid >> 5, sc = tid & 31;
  f32x16 acc;
#pragma unroll
  for (int q = 0; q < 16; ++q) acc[q] = 0.0f;
  float ra[KNN_STG], rb[KNN_STG];
  // plain loads from clamped addresses: a predicated load is a branch around it and the sixteen loads of a
  // chunk would go out one memory latency after the other.  What the tile does not have is zeroed when the
  // registers are committed, not here: from `ok ? loaded : 0` beside the load the compiler forms that very
  // branch (profiles/r11_knn_tile.txt)
  auto fetch = [&](int k0) {
    const int f = k0 + sc;
    const int fc = f < nf ? f : nf - 1;
#pragma unroll
    for (int q = 0; q < KNN_STG; ++q) {
      ra[q] = arow[q][fc];
      rb[q] = brow[q][fc];
    }
  };
  fetch(0);
  for (int k0 = 0; k0 < nf; k0 += KNN_KB) {
    const bool fok = k0 + sc < nf;
    __syncthreads();
#pragma unroll
    for (int q = 0; q < KNN_STG; ++q) {
      sA[(sr + 8 * q) * KNN_KBP + sc] = (aok[q] && fok) ? ra[q] : 0.0f;
      sB[(sr + 8 * q) * KNN_KBP + sc] = (bok[q] && fok) ? rb[q] : 0.0f;
    }
    __syncthreads();
    if (k0 + KNN_KB < nf) fetch(k0 + KNN_KB);
    const float* pa = sA + (wi * 32 + li) * KNN_KBP + lk;
    const float* pb = sB + (wj * 32 + li) * KNN_KBP + lk;
#pragma unroll
    for (int kk = 0; kk < KNN_KB; kk += 2)
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(pa[kk], pb[kk], acc, 0, 0, 0);
  }
  return acc;
}

// Parks the wave's quadrant in sD as squared distances.  keep(r, c) says whether tile row r may list tile
// candidate c (both exist, not the same item); qn(r) / cn(c) are their squared norms, read only where keep
// holds.  Everything else is parked as FLT_MAX, which no merge lets in.
template <class Keep, class QNorm, class CNorm>
__device__ __forceinline__ void knn_park_tile(float* sD, const f32x16& acc, Keep keep, QNorm qn, CNorm cn) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int wi = wave >> 1, wj = wave & 1, li = lane & 31, lk = lane >> 5;
  // C/D map of the 32x32 tile: col = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
#pragma unroll
  for (int q = 0; q < 16; ++q) {
    const int r = wi * 32 + (q & 3) + 8 * (q >> 2) + 4 * lk;
    const int c = wj * 32 + li;
    float d2 = 3.402823466e+38f;
    if (keep(r, c)) d2 = fmaxf(qn(r) + cn(c) - 2.0f * acc[q], 0.0f);
    sD[r * (KNN_BN + 1) + c] = d2;
  }
}

// The squared distance of listed pairs with the bits the tile gives them (k_knn_rerank of mde_knn_bf16.hip, the
// thresholds of mde_knn_rank.hip).  A wave owns query row qc of Q and a lane the corpus row crow of C (any
// readable row where !valid).  The Gram tile sums a dot product as one feature-ordered fmaf chain from 0 (the
// f32 MFMA rounds once per product, in k order; zero padding adds nothing), so the lane runs that chain over
// f = 0 .. nf - 1 and forms fmaxf(qn + cn - 2 acc, 0) from the norms of k_row_sqnorm.  (2 acc is exact, so the
// expression rounds once whether or not it is contracted.)  The listed rows are gathered through LDS in chunks
// of KNN_RR_KB features: a half wave reads the 128 contiguous bytes of one row per load, and the lane then
// reads its own row conflict-free (stride 33).  mC [64 * KNN_RR_KBP] and mQ [KNN_RR_KB] are the wave's own
// LDS; every thread of the workgroup calls (barriers inside).  FLT_MAX where !valid.
#define KNN_RR_KB 32
#define KNN_RR_KBP 33
__device__ __forceinline__ float knn_wave_pair_d2(float* mC, float* mQ, int nf, const float* __restrict__ Q,
                                                  const float* __restrict__ C, const float* __restrict__ qn,
                                                  const float* __restrict__ cn, int64_t qc, int64_t crow,
                                                  bool valid) {
  const int lane = threadIdx.x & 63;
  const int half = lane >> 5, col = lane & 31;
  float acc = 0.0f;
  for (int k0 = 0; k0 < nf; k0 += KNN_RR_KB) {
    const int f = k0 + col < nf ? k0 + col : nf - 1;    // clamped: a column past nf is never read back
    __syncthreads();
    if (lane < KNN_RR_KB) mQ[lane] = Q[qc * nf + f];
#pragma unroll 8
    for (int i = 0; i < 32; ++i) {
      const int r = 2 * i + half;
      const int64_t src = __shfl((int)crow, r, 64);
      mC[r * KNN_RR_KBP + col] = C[src * nf + f];
    }
    __syncthreads();
    const int kn = nf - k0 < KNN_RR_KB ? nf - k0 : KNN_RR_KB;
    const float* my = mC + lane * KNN_RR_KBP;
    if (kn == KNN_RR_KB) {
#pragma unroll
      for (int kk = 0; kk < KNN_RR_KB; ++kk) acc = fmaf(mQ[kk], my[kk], acc);
    } else {
      for (int kk = 0; kk < kn; ++kk) acc = fmaf(mQ[kk], my[kk], acc);
    }
  }
  float d2 = 3.402823466e+38f;
  if (valid) d2 = fmaxf(qn[qc] + cn[crow] - 2.0f * acc, 0.0f);
  return d2;
}

// mde_knn_bf16.hip -- the two-stage Euclidean k-NN search: every pair is ranked by a bf16
// Gram product on the bf16 matrix cores (v_mfma_f32_32x32x16_bf16, 16x the rate of the f32 MFMA of
// mde_knn_tile.h), each query keeps a shortlist of n_cand >= k candidates, and the shortlist is re-ranked with
// the exact float32 squared distances of the float32 kernels, bit for bit.
//
//   k_rows_to_bf16      the bf16 copy of the (centred) rows, zero padded to a stride of SB_KB, and the f32
//                       squared norms of the rounded rows
//   k_knn_short_bf16    the shortlist: a 128 x 128 tile of |x^|^2 + |y^|^2 - 2 x^.y^ per step, lists by (d2, index)
//   k_knn_cross_merge   (mde_knn_slices.h) folds the lists of the corpus slices
//   k_knn_rerank        exact float32 d2 of every shortlisted pair, the best k by (d2, index)
#include "mde_knn_slices.h"

#define SB_BM 128            // query rows of a workgroup
#define SB_BN 128            // candidates of a tile
#define SB_HALF 64           // candidates parked and merged at a time
#define SB_KB 32             // bf16 features of a staged chunk = two K steps of the MFMA; the row stride's unit
#define SB_KBP 40            // LDS row stride of a chunk in bf16 (80 B: the 16-lane groups of ds_read_b128 hit 64 banks)
#define SB_DP (SB_HALF + 2)  // row stride of the parked half tile (66: the merge scan's 64 lanes hit 64 banks)
#define SB_STAGE_ELEMS (SB_BM * SB_KBP)   // bf16 elements of one side of one buffer
#define SB_STAGE_BYTES (2 * 2 * SB_STAGE_ELEMS * 2)   // two buffers of two sides
#define SB_FLT_MAX 3.402823466e+38f

static_assert(SB_STAGE_BYTES >= SB_BM * SB_DP * 4, "the parked half tile lives in the staging buffers");
static_assert(MDE_BLOCK == 256 && SB_BM == 128 && SB_BN == 128, "four waves of 64 x 64");

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

static inline int64_t bf16_stride(int nf) { return ((int64_t)nf + SB_KB - 1) / SB_KB * SB_KB; }
static inline size_t short_lds_bytes(int nc) {
  return (size_t)SB_STAGE_BYTES + 3 * SB_BM * sizeof(float) + (size_t)SB_BM * nc * (sizeof(float) + sizeof(int));
}

__device__ __forceinline__ uint32_t bf16_rne(float v) {   // finite v; round to nearest, ties to even
  uint32_t u = __float_as_uint(v);
  u += 0x7fffu + ((u >> 16) & 1u);
  return u >> 16;
}

// out[r][c] = bf16((float)((double)x[r][c] - mu[c])) for c < nf, 0 up to the stride nfp (a multiple of SB_KB);
// norm[r] = the f32 squared norm of the rounded row.  One wave per row, a lane takes pairs of columns.
__global__ __launch_bounds__(MDE_BLOCK) void k_rows_to_bf16(int64_t n, int nf, int nfp, const float* __restrict__ X,
                                                            const double* __restrict__ mu,
                                                            uint16_t* __restrict__ out, float* __restrict__ norm) {
  const int lane = threadIdx.x & 63;
  const int64_t w0 = ((int64_t)blockIdx.x * MDE_BLOCK + threadIdx.x) >> 6;
  const int64_t nw = ((int64_t)gridDim.x * MDE_BLOCK) >> 6;
  for (int64_t r = w0; r < n; r += nw) {
    float s = 0.0f;
    for (int c = 2 * lane; c < nfp; c += 128) {
      uint32_t h[2];
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        float v = 0.0f;
        if (c + j < nf) {
          const float x = X[r * nf + c + j];
          v = mu ? (float)((double)x - mu[c + j]) : x;
        }
        h[j] = bf16_rne(v);
        const float vr = __uint_as_float(h[j] << 16);
        s = fmaf(vr, vr, s);
      }
      *reinterpret_cast<uint32_t*>(out + r * nfp + c) = h[0] | (h[1] << 16);
    }
    s = mde_wave_sum(s);
    if (lane == 0) norm[r] = s;
  }
}

// Inserts (d2, id) into the list bd / bi of nc entries ordered by (d2, index) when it beats the last one.
__device__ __forceinline__ void short_insert(float d2, int id, int nc, float* __restrict__ bd, int* __restrict__ bi,
                                             float& worst_d, int& worst_i) {
  if (!(d2 < worst_d || (d2 == worst_d && id < worst_i))) return;
  int pos = nc - 1;
  while (pos > 0) {
    const float pd = bd[pos - 1];
    const int pi = bi[pos - 1];
    if (!(pd > d2 || (pd == d2 && pi > id))) break;
    bd[pos] = pd;
    bi[pos] = pi;
    --pos;
  }
  bd[pos] = d2;
  bi[pos] = id;
  worst_d = bd[nc - 1];
  worst_i = bi[nc - 1];
}

// The shortlist.  Workgroup (x, y) owns query rows [128 x, 128 x + 128) and walks the corpus columns of slice
// y, [y * slice_cols, (y + 1) * slice_cols) cut at n_c (slice_cols a multiple of 128), 128 at a time.  Wave
// (wi, wj) accumulates the 64 x 64 quadrant (wi, wj) of the tile as 2 x 2 MFMA blocks: four 16-byte fragment
// reads feed four MFMAs.  Both sides are staged in chunks of SB_KB features with 16-byte global loads held in
// registers across the MFMAs of the previous chunk, into two LDS buffers: one barrier per chunk.
// The tile is parked in two halves of 64 candidates (waves wj = 0, then wj = 1) over the staging buffers.
// All 256 threads scan a parked half -- thread t the candidates of parity t & 1 of row t >> 1 -- against the
// row's current n_cand-th best, and the even thread of a pair inserts what passed: after the first tiles a
// scan finds nothing and the serial insert does not run.  Lists are ordered by (d2, index), so they do not
// depend on the order of insertion, on the slice count or on the run.  SELF: Q and C are one matrix and a row
// does not list itself.  Output: list y of [slices, n_q, nc].
template <bool SELF>
__global__ __launch_bounds__(MDE_BLOCK) void k_knn_short_bf16(int n_q, int n_c, int nfp, int nc, int64_t slice_cols,
                                                              const uint16_t* __restrict__ Qb,
                                                              const uint16_t* __restrict__ Cb,
                                                              const float* __restrict__ qn,
                                                              const float* __restrict__ cn,
                                                              int32_t* __restrict__ idx_out,
                                                              float* __restrict__ d2_out) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  uint16_t* stage = reinterpret_cast<uint16_t*>(lds);   // [2 buffers][A, B][128][SB_KBP]
  float* sD = lds;                                      // [128][SB_DP], over the staging buffers
  float* swd = lds + SB_STAGE_BYTES / 4;                // [128] the rows' n_cand-th best: distance,
  int* swi = reinterpret_cast<int*>(swd + SB_BM);       // [128] index
  float* sqn = reinterpret_cast<float*>(swi + SB_BM);   // [128] the query norms
  float* bestd = sqn + SB_BM;                           // [128][nc]
  int* besti = reinterpret_cast<int*>(bestd + SB_BM * nc);

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wi = wave >> 1, wj = wave & 1, li = lane & 31, lk = lane >> 5;
  const int64_t row0 = (int64_t)blockIdx.x * SB_BM;
  const int64_t lo = (int64_t)blockIdx.y * slice_cols;
  const int64_t c_lo = lo < n_c ? lo : n_c, c_hi = lo + slice_cols < n_c ? lo + slice_cols : n_c;

  knn_lists_init(bestd, besti, SB_BM * nc);
  if (tid < SB_BM) {
    swd[tid] = SB_FLT_MAX;
    swi[tid] = -1;
    sqn[tid] = row0 + tid < n_q ? qn[row0 + tid] : 0.0f;
  }

  // staging: thread t takes the 16 bytes t & 3 of the rows (t >> 2) + 64 p, p < 2, of either side; a row past
  // the matrix reads the last row (its distances are parked as FLT_MAX), so every load stays inside Qb / Cb
  const int sr = tid >> 2, sseg = tid & 3;
  const int64_t gr0 = row0 + sr, gr1 = gr0 + 64;
  const uint4* const arow0 = reinterpret_cast<const uint4*>(Qb + (gr0 < n_q ? gr0 : n_q - 1) * nfp) + sseg;
  const uint4* const arow1 = reinterpret_cast<const uint4*>(Qb + (gr1 < n_q ? gr1 : n_q - 1) * nfp) + sseg;
  uint4 ra0, ra1, rb0, rb1;   // named registers: arrays reached through a lambda end up in scratch
  // k0 in bf16 elements, a multiple of SB_KB = 4 uint4
#define SB_FETCH(col0_, k0_)                                                                              \
  do {                                                                                                    \
    const int64_t gc0 = (col0_) + sr, gc1 = gc0 + 64;                                                     \
    ra0 = arow0[(k0_) >> 3];                                                                              \
    ra1 = arow1[(k0_) >> 3];                                                                              \
    rb0 = (reinterpret_cast<const uint4*>(Cb + (gc0 < n_c ? gc0 : n_c - 1) * nfp) + sseg)[(k0_) >> 3];    \
    rb1 = (reinterpret_cast<const uint4*>(Cb + (gc1 < n_c ? gc1 : n_c - 1) * nfp) + sseg)[(k0_) >> 3];    \
  } while (0)
  if (c_lo < c_hi) SB_FETCH(c_lo, 0);

  for (int64_t col0 = c_lo; col0 < c_hi; col0 += SB_BN) {
    f32x16 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int q = 0; q < 16; ++q) acc[a][b][q] = 0.0f;
    __syncthreads();   // the scan of the previous tile is over (and the lists are initialised): staging may be written
    int buf = 0;
    for (int k0 = 0; k0 < nfp; k0 += SB_KB, buf ^= 1) {
      uint16_t* sA = stage + buf * 2 * SB_STAGE_ELEMS;
      uint16_t* sB = sA + SB_STAGE_ELEMS;
      *reinterpret_cast<uint4*>(sA + sr * SB_KBP + sseg * 8) = ra0;
      *reinterpret_cast<uint4*>(sA + (sr + 64) * SB_KBP + sseg * 8) = ra1;
      *reinterpret_cast<uint4*>(sB + sr * SB_KBP + sseg * 8) = rb0;
      *reinterpret_cast<uint4*>(sB + (sr + 64) * SB_KBP + sseg * 8) = rb1;
      __syncthreads();
      if (k0 + SB_KB < nfp)
        SB_FETCH(col0, k0 + SB_KB);
      else if (col0 + SB_BN < c_hi)
        SB_FETCH(col0 + SB_BN, 0);       // the next tile's first chunk travels during the merge
#pragma unroll
      for (int ks = 0; ks < SB_KB; ks += 16) {
        bf16x8 fa[2], fb[2];
#pragma unroll
        for (int a = 0; a < 2; ++a) {
          fa[a] = *reinterpret_cast<const bf16x8*>(sA + (wi * 64 + a * 32 + li) * SB_KBP + ks + 8 * lk);
          fb[a] = *reinterpret_cast<const bf16x8*>(sB + (wj * 64 + a * 32 + li) * SB_KBP + ks + 8 * lk);
        }
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
          for (int b = 0; b < 2; ++b)
            acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[a], fb[b], acc[a][b], 0, 0, 0);
      }
    }
    for (int h = 0; h < 2; ++h) {
      __syncthreads();   // h = 0: the last chunk's fragments are read; h = 1: the scan of half 0 is over
      if (wj == h) {
        // C/D map of a 32x32 block: col = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5).  A row past
        // n_q is not masked: its list is never stored.  A column past n_c gets an infinite norm, so an infinite
        // distance, which no list lets in.  No compare per element: their masks would crowd the scalar registers.
#pragma unroll
        for (int b = 0; b < 2; ++b) {
          const int c = b * 32 + li;
          const int64_t gc = col0 + h * SB_HALF + c;
          const float cnv = gc < n_c ? cn[gc] : __builtin_inff();
#pragma unroll
          for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int q = 0; q < 16; ++q) {
              const int r = wi * 64 + a * 32 + (q & 3) + 8 * (q >> 2) + 4 * lk;
              sD[r * SB_DP + c] = fmaxf(sqn[r] + cnv - 2.0f * acc[a][b][q], 0.0f);
            }
        }
      }
      if (SELF) {
        // tile row r (< 128) is parked column c's (< 64) own item when r - c = sdelta: only on the diagonal
        const int64_t sdelta = col0 + h * SB_HALF - row0;
        if (sdelta > -SB_HALF && sdelta < SB_BM) {
          __syncthreads();
          const int r = tid + (int)sdelta;
          if (tid < SB_HALF && r >= 0 && r < SB_BM) sD[r * SB_DP + tid] = __builtin_inff();
        }
      }
      __syncthreads();
      {
        const int r = tid >> 1, par = tid & 1;
        const float* sd = sD + r * SB_DP + par;
        float wd = swd[r];
        uint32_t mask = 0;
#pragma unroll
        for (int c = 0; c < SB_HALF / 2; ++c)   // d < wd as the sign of d - wd: no compare mask per candidate
          mask |= (__float_as_uint(sd[2 * c] - wd) >> 31) << c;
        const uint32_t other = __shfl_xor(mask, 1, 64);
        if (par == 0 && (mask | other)) {
          int wx = swi[r];
          float* bd = bestd + r * nc;
          int* bi = besti + r * nc;
          const int id0 = (int)col0 + h * SB_HALF;
          // bit c of the even thread's mask is candidate 2 c, of the odd thread's 2 c + 1; the list's order
          // does not depend on the order of insertion
          uint64_t m = (uint64_t)mask | ((uint64_t)other << 32);
#pragma unroll 1
          while (m) {
            const int bit = __ffsll((unsigned long long)m) - 1;
            m &= m - 1;
            const int c = 2 * (bit & 31) + (bit >> 5);
            short_insert(sd[c], id0 + c, nc, bd, bi, wd, wx);
          }
          swd[r] = wd;
          swi[r] = wx;
        }
      }
    }
  }
  __syncthreads();
  const int rows = n_q - row0 < SB_BM ? (int)(n_q - row0) : SB_BM;
  const int64_t base = ((int64_t)blockIdx.y * n_q + row0) * nc;   // the block's rows are contiguous in list y
  knn_lists_store(bestd, besti, rows * nc, idx_out + base, d2_out + base);
}

// The re-rank.  A wave owns one query and a lane one entry of its shortlist (nc <= 64 lanes; -1 is skipped).
// d2 is what the float32 kernels give the pair: knn_wave_pair_d2 (mde_knn_tile.h) runs the Gram tile's
// feature-ordered fmaf chain on the shortlisted rows, gathered through LDS.  The best k by (d2, index) are
// placed by rank: a lane counts the entries that precede its own.
__global__ __launch_bounds__(MDE_BLOCK) void k_knn_rerank(int n_q, int nf, int k, int nc, const float* __restrict__ Q,
                                                          const float* __restrict__ C,
                                                          const float* __restrict__ qn,
                                                          const float* __restrict__ cn,
                                                          const int32_t* __restrict__ sidx,
                                                          int32_t* __restrict__ idx_out,
                                                          float* __restrict__ d2_out) {
  __shared__ float sC[4][64 * KNN_RR_KBP];
  __shared__ float sQ[4][KNN_RR_KB];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t q = (int64_t)blockIdx.x * 4 + wave;
  const int64_t qc = q < n_q ? q : n_q - 1;
  const int mine = lane < nc ? sidx[qc * nc + lane] : -1;
  const bool valid = mine >= 0;
  const int64_t crow = valid ? mine : 0;
  float* mC = sC[wave];
  const float d2 = knn_wave_pair_d2(mC, sQ[wave], nf, Q, C, qn, cn, qc, crow, valid);
  const int id = valid ? mine : 0x7fffffff;
  __syncthreads();
  mC[lane] = d2;
  reinterpret_cast<int*>(mC)[64 + lane] = id;
  __syncthreads();
  int rank = 0;
  for (int j = 0; j < nc; ++j) {
    const float dj = mC[j];
    const int ij = reinterpret_cast<const int*>(mC)[64 + j];
    rank += (dj < d2 || (dj == d2 && (ij < id || (ij == id && j < lane)))) ? 1 : 0;
  }
  if (q < n_q && lane < nc && rank < k) {
    idx_out[q * k + rank] = valid ? mine : -1;
    d2_out[q * k + rank] = d2;
  }
}

// ---------------------------------------------------------------- host
static bool bf16_args_ok(int64_t n_q, int64_t n_c, int32_t k, int32_t n_cand, int32_t slices) {
  return cross_args_ok(n_q, n_c, k, slices) && n_cand >= k && n_cand <= KNN_MAXK;
}
static inline int64_t up16(int64_t bytes) { return (bytes + 15) / 16 * 16; }

// The scratch of mde_knn_bf16, every piece at a multiple of 16 bytes.
struct bf16_work {
  int64_t qb, cb, qnb, cnb, qn, cn, sidx, sd2, pd, pi, total;
};
static bf16_work bf16_layout(int64_t n_q, int64_t n_c, int32_t nf, int32_t n_cand, int64_t s, bool self) {
  const int64_t nfp = bf16_stride(nf);
  bf16_work w;
  int64_t o = 0;
  w.qb = o, o += up16(n_q * nfp * 2);
  w.cb = self ? w.qb : o;
  if (!self) o += up16(n_c * nfp * 2);
  w.qnb = o, o += up16(n_q * 4);
  w.cnb = self ? w.qnb : o;
  if (!self) o += up16(n_c * 4);
  w.qn = o, o += up16(n_q * 4);
  w.cn = self ? w.qn : o;
  if (!self) o += up16(n_c * 4);
  w.sidx = o, o += up16(n_q * (int64_t)n_cand * 4);
  w.sd2 = o, o += up16(n_q * (int64_t)n_cand * 4);
  w.pd = o;
  if (s > 1) o += up16(s * n_q * (int64_t)n_cand * 4);
  w.pi = o;
  if (s > 1) o += up16(s * n_q * (int64_t)n_cand * 4);
  w.total = o;
  return w;
}

extern "C" int64_t mde_knn_bf16_work_bytes(int64_t n_q, int64_t n_c, int32_t nf, int32_t k, int32_t n_cand,
                                           int32_t slices) {
  if (!bf16_args_ok(n_q, n_c, k, n_cand, slices) || nf <= 0) {
    mde_set_error("mde_knn_bf16_work_bytes: invalid arguments (1 <= k <= n_cand <= %d, 0 <= slices <= %d, n_q, n_c, "
                  "nf >= 1)", KNN_MAXK, CROSS_MAX_SLICES);
    return MDE_E_INVALID;
  }
  const int64_t s = cross_resolve_slices(n_q, n_c, slices, SB_BM, SB_BN);
  if (s < 0) return s;
  // the larger of the two layouts: a caller need not say here whether the search is a self-join
  return bf16_layout(n_q, n_c, nf, n_cand, s, false).total;
}

extern "C" int mde_knn_bf16(int64_t n_q, int64_t n_c, int32_t nf, const float* Q, const float* C, const double* mu,
                            int32_t self, int32_t k, int32_t n_cand, int32_t slices, int32_t* idx_out,
                            float* d2_out, void* work, void* stream) {
  if (!bf16_args_ok(n_q, n_c, k, n_cand, slices) || nf <= 0 || !Q || !C || !idx_out || !d2_out || !work ||
      (self && (Q != C || n_q != n_c))) {
    mde_set_error("mde_knn_bf16: invalid arguments (1 <= k <= n_cand <= %d, 0 <= slices <= %d, n_q, n_c, nf >= 1; "
                  "self != 0 needs Q == C and n_q == n_c)", KNN_MAXK, CROSS_MAX_SLICES);
    return MDE_E_INVALID;
  }
  if (n_q >= ((int64_t)1 << 31) || n_c >= ((int64_t)1 << 31)) return MDE_E_TOO_LARGE;
  const int64_t s = cross_resolve_slices(n_q, n_c, slices, SB_BM, SB_BN);
  if (s < 0) return (int)s;
  hipStream_t st = mde_stream(stream);
  const bool sj = self != 0;
  const int nfp = (int)bf16_stride(nf);
  const bf16_work w = bf16_layout(n_q, n_c, nf, n_cand, s, sj);
  char* base = static_cast<char*>(work);
  uint16_t* Qb = reinterpret_cast<uint16_t*>(base + w.qb);
  uint16_t* Cb = reinterpret_cast<uint16_t*>(base + w.cb);
  float* qnb = reinterpret_cast<float*>(base + w.qnb);
  float* cnb = reinterpret_cast<float*>(base + w.cnb);
  float* qn = reinterpret_cast<float*>(base + w.qn);
  float* cn = reinterpret_cast<float*>(base + w.cn);
  int32_t* sidx = reinterpret_cast<int32_t*>(base + w.sidx);
  float* sd2 = reinterpret_cast<float*>(base + w.sd2);
  float* pd = reinterpret_cast<float*>(base + w.pd);
  int32_t* pi = reinterpret_cast<int32_t*>(base + w.pi);

  // the bf16 copies with their norms, and the float32 norms of the re-rank (as mde_knn's)
  hipLaunchKernelGGL(k_rows_to_bf16, dim3(mde_grid(n_q * 64, MDE_BLOCK, 4096)), dim3(MDE_BLOCK), 0, st, n_q, nf, nfp,
                     Q, mu, Qb, qnb);
  MDE_LAUNCH_CHECK();
  int rc = mde_row_sqnorm(n_q, nf, Q, qn, stream);
  if (rc != MDE_OK) return rc;
  if (!sj) {
    hipLaunchKernelGGL(k_rows_to_bf16, dim3(mde_grid(n_c * 64, MDE_BLOCK, 4096)), dim3(MDE_BLOCK), 0, st, n_c, nf, nfp,
                       C, mu, Cb, cnb);
    MDE_LAUNCH_CHECK();
    rc = mde_row_sqnorm(n_c, nf, C, cn, stream);
    if (rc != MDE_OK) return rc;
  }

  rc = sj ? knn_raise_lds_limit<k_knn_short_bf16<true>>(112 * 1024)
          : knn_raise_lds_limit<k_knn_short_bf16<false>>(112 * 1024);
  if (rc == MDE_OK) rc = knn_raise_lds_limit<k_knn_cross_merge>(96 * 1024);
  if (rc != MDE_OK) return rc;
  const int64_t tiles = (n_c + SB_BN - 1) / SB_BN;
  const int64_t slice_cols = ((tiles + s - 1) / s) * SB_BN;   // whole tiles; the last slices may be short or empty
  const dim3 grid((unsigned)((n_q + SB_BM - 1) / SB_BM), (unsigned)s);
  int32_t* li = s > 1 ? pi : sidx;
  float* ld = s > 1 ? pd : sd2;
  if (sj)
    hipLaunchKernelGGL(k_knn_short_bf16<true>, grid, dim3(MDE_BLOCK), short_lds_bytes(n_cand), st, (int)n_q, (int)n_c,
                       nfp, n_cand, slice_cols, Qb, Cb, qnb, cnb, li, ld);
  else
    hipLaunchKernelGGL(k_knn_short_bf16<false>, grid, dim3(MDE_BLOCK), short_lds_bytes(n_cand), st, (int)n_q, (int)n_c,
                       nfp, n_cand, slice_cols, Qb, Cb, qnb, cnb, li, ld);
  MDE_LAUNCH_CHECK();
  if (s > 1) {
    hipLaunchKernelGGL(k_knn_cross_merge, dim3((unsigned)((n_q + KNN_BM - 1) / KNN_BM)), dim3(MDE_BLOCK),
                       knn_cross_merge_lds_bytes(n_cand), st, (int)n_q, n_cand, (int)s, pd, pi, sidx, sd2);
    MDE_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(k_knn_rerank, dim3((unsigned)((n_q + 3) / 4)), dim3(MDE_BLOCK), 0, st, (int)n_q, nf, k, n_cand, Q,
                     C, qn, cn, sidx, idx_out, d2_out);
  MDE_LAUNCH_CHECK();
  return MDE_OK;
}

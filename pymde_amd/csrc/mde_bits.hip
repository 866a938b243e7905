// mde_bits.hip -- bit-packed binary data: packing a 0/1 matrix (dense or CSR) into 32-bit
// words, the exact Jaccard / Hamming k-NN search on the packed rows, and the same distances of listed pairs.
// A row of nf features is nw = ceil(nf / 32) words, feature f in bit (f & 31) of word f >> 5, padding bits zero;
// counts[r] is the row's popcount.  With a, b the counts of two rows and t = sum popcount(u & v) over the words:
//   Hamming  float(a + b - 2 t) / float(nf)
//   Jaccard  float(a + b - 2 t) / float(a + b - t), 0 when a + b - t == 0  (scipy.spatial.distance)
// nf < 2^24, so numerator and denominator are exact in float32 and the value is one correctly rounded quotient:
// a pair has the same bits in every kernel here and for every slice count.  The reference has no binary
// distance (its k-NN is Euclidean).
#include "mde_knn_tile.h"
#include "mde_knn_slices.h"

#define BITS_JACCARD 0
#define BITS_HAMMING 1
#define BITS_MAX_NF (1 << 24)

__device__ __forceinline__ float bits_distance(int a, int b, int t, int nf, int kind) {
  const int num = a + b - 2 * t;
  const int den = kind == BITS_HAMMING ? nf : a + b - t;
  return den == 0 ? 0.0f : (float)num / (float)den;
}

// ------------------------------------------------------------------ packing
__global__ void k_bits_bad_init(int* bad_row) { *bad_row = 0x7fffffff; }

// One wave per row: 64 features per step, a ballot of x != 0 is two words; the count is the popcount of the
// same ballots.  A value other than 0 or 1 (NaN included) min-reduces the row into *bad_row.
__global__ __launch_bounds__(MDE_BLOCK) void k_bits_pack(int64_t n, int nf, int nw, const float* __restrict__ X,
                                                         int32_t* __restrict__ words, int32_t* __restrict__ counts,
                                                         int* __restrict__ bad_row) {
  const int lane = threadIdx.x & 63;
  const int64_t w0 = ((int64_t)blockIdx.x * MDE_BLOCK + threadIdx.x) >> 6;
  const int64_t nwv = ((int64_t)gridDim.x * MDE_BLOCK) >> 6;
  for (int64_t r = w0; r < n; r += nwv) {
    const float* x = X + r * nf;
    int cnt = 0;
    bool bad = false;
    for (int c0 = 0; c0 < nf; c0 += 64) {
      const int c = c0 + lane;
      const float v = c < nf ? x[c] : 0.0f;
      bad = bad || !(v == 0.0f || v == 1.0f);
      const unsigned long long m = __ballot(v != 0.0f);
      cnt += __popcll(m);
      const int w = c0 >> 5;
      if (lane == 0) words[r * nw + w] = (int32_t)(uint32_t)m;
      if (lane == 1 && w + 1 < nw) words[r * nw + w + 1] = (int32_t)(uint32_t)(m >> 32);
    }
    if (lane == 0) counts[r] = cnt;
    if (bad) atomicMin(bad_row, (int)r);
  }
}

extern "C" int mde_bits_pack(int64_t n, int32_t nf, const float* data, int32_t* words, int32_t* counts,
                             int32_t* bad_row, void* stream) {
  if (n <= 0 || nf <= 0 || nf >= BITS_MAX_NF || !data || !words || !counts || !bad_row) {
    mde_set_error("mde_bits_pack: invalid arguments (n >= 1, 1 <= nf < 2^24, non-null pointers)");
    return MDE_E_INVALID;
  }
  if (n >= ((int64_t)1 << 31)) return MDE_E_TOO_LARGE;
  hipStream_t st = mde_stream(stream);
  hipLaunchKernelGGL(k_bits_bad_init, dim3(1), dim3(1), 0, st, bad_row);
  MDE_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_bits_pack, dim3(mde_grid(n * 64, MDE_BLOCK, 8192)), dim3(MDE_BLOCK), 0, st, n, nf,
                     (nf + 31) / 32, data, words, counts, bad_row);
  MDE_LAUNCH_CHECK();
  return MDE_OK;
}

// CSR: one wave per row ORs its stored ones into the zeroed words (an integer atomic: order-free, and a
// duplicate entry sets its bit once); a stored value other than 0 or 1, a column outside [0, nf) or a row whose
// extent is not inside [0, nnz) marks the row bad.  k_bits_count then takes the counts from the words.
__global__ __launch_bounds__(MDE_BLOCK) void k_bits_pack_csr(int64_t n, int nf, int nw, int64_t nnz,
                                                             const int64_t* __restrict__ indptr,
                                                             const int32_t* __restrict__ indices,
                                                             const float* __restrict__ values,
                                                             int32_t* __restrict__ words, int* __restrict__ bad_row) {
  const int lane = threadIdx.x & 63;
  const int64_t w0 = ((int64_t)blockIdx.x * MDE_BLOCK + threadIdx.x) >> 6;
  const int64_t nwv = ((int64_t)gridDim.x * MDE_BLOCK) >> 6;
  for (int64_t r = w0; r < n; r += nwv) {
    const int64_t lo = indptr[r], hi = indptr[r + 1];
    bool bad = lo < 0 || hi < lo || hi > nnz;
    if (!bad)
      for (int64_t e = lo + lane; e < hi; e += 64) {
        const int c = indices[e];
        const float v = values[e];
        if (c < 0 || c >= nf || !(v == 0.0f || v == 1.0f))
          bad = true;
        else if (v != 0.0f)
          atomicOr(reinterpret_cast<unsigned int*>(words) + r * nw + (c >> 5), 1u << (c & 31));
      }
    if (bad) atomicMin(bad_row, (int)r);
  }
}
__global__ __launch_bounds__(MDE_BLOCK) void k_bits_count(int64_t n, int nw, const int32_t* __restrict__ words,
                                                          int32_t* __restrict__ counts) {
  const int lane = threadIdx.x & 63;
  const int64_t w0 = ((int64_t)blockIdx.x * MDE_BLOCK + threadIdx.x) >> 6;
  const int64_t nwv = ((int64_t)gridDim.x * MDE_BLOCK) >> 6;
  for (int64_t r = w0; r < n; r += nwv) {
    int cnt = 0;
    for (int w = lane; w < nw; w += 64) cnt += __popc((unsigned int)words[r * nw + w]);
    cnt = mde_wave_sum(cnt);
    if (lane == 0) counts[r] = cnt;
  }
}

extern "C" int mde_bits_pack_csr(int64_t n, int32_t nf, int64_t nnz, const int64_t* indptr, const int32_t* indices,
                                 const float* values, int32_t* words, int32_t* counts, int32_t* bad_row,
                                 void* stream) {
  if (n <= 0 || nf <= 0 || nf >= BITS_MAX_NF || nnz < 0 || !indptr || (nnz > 0 && (!indices || !values)) || !words ||
      !counts || !bad_row) {
    mde_set_error("mde_bits_pack_csr: invalid arguments (n >= 1, 1 <= nf < 2^24, nnz >= 0, non-null pointers)");
    return MDE_E_INVALID;
  }
  if (n >= ((int64_t)1 << 31)) return MDE_E_TOO_LARGE;
  hipStream_t st = mde_stream(stream);
  const int nw = (nf + 31) / 32;
  MDE_HIP(hipMemsetAsync(words, 0, sizeof(int32_t) * (size_t)n * nw, st));
  hipLaunchKernelGGL(k_bits_bad_init, dim3(1), dim3(1), 0, st, bad_row);
  MDE_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_bits_pack_csr, dim3(mde_grid(n * 64, MDE_BLOCK, 8192)), dim3(MDE_BLOCK), 0, st, n, nf, nw, nnz,
                     indptr, indices, values, words, bad_row);
  MDE_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_bits_count, dim3(mde_grid(n * 64, MDE_BLOCK, 8192)), dim3(MDE_BLOCK), 0, st, n, nw, words,
                     counts);
  MDE_LAUNCH_CHECK();
  return MDE_OK;
}

// ------------------------------------------------------------------ the search
// The workgroup shape of k_knn_l1 (mde_metric.hip) on the grid of k_knn_cross (mde_knn.hip): workgroup (x, y)
// owns query rows [64 x, 64 x + 64) and walks the corpus rows of slice y 64 at a time; thread (ty, tx) =
// (tid >> 4, tid & 15) holds the 4 x 4 block (rows 4 ty .., candidates 4 tx ..) of the tile's intersection
// counts as uint32.  Words are staged through LDS WORD-major, [word][row], in chunks of 32 words and lines of
// 68: the four rows of a thread at one word are one 16-byte read, the 16 tx of a wave read 256 contiguous bytes
// and its 4 ty four broadcast addresses (conflict-free, as in k_knn_l1).  acc += __popc(a & b) is v_and_b32 and
// v_bcnt_u32_b32 with the accumulator as its addend: two VALU instructions per 32 feature pairs.  Staging:
// thread (c = tid & 31, g = tid >> 5) loads word c of rows 4 g .. 4 g + 3 and 32 + 4 g .. of either side from
// clamped addresses (zeroed where the tile has no such row or word) and commits two 16-byte writes per side;
// the next chunk's loads are issued before the arithmetic of the current one.
//
// The tile is parked in LDS as float32 distances and merged by mde_topk_merge, one thread per query row.  A
// tile of 6 to 64 words is a few hundred to two thousand VALU instructions per thread, so a merge thread's 64
// LDS reads and compares per tile are no longer small beside it: while parking, every thread compares its 16
// values with the k-th best of their rows (sWorst, written by the merge threads) and raises the row's flag on a
// hit; a merge thread whose flag is down skips its row.  mde_topk_merge admits a candidate only when it is
// strictly below the k-th best, so skipping a row without such a candidate changes nothing: the lists are
// those of the unconditional merge.
#define BITS_BM 64
#define BITS_BN 64
#define BITS_KB 32
#define BITS_LD 68
#ifndef BITS_PRECHECK
#define BITS_PRECHECK 1   // 0: every flag is raised, every merge thread scans its row (the comparison of DESIGN 6v)
#endif

static inline size_t bits_knn_lds_bytes(int k) {
  return sizeof(float) * (size_t)(2 * BITS_KB * BITS_LD + BITS_BM * (BITS_BN + 1) + 2 * BITS_BM) +
         (size_t)BITS_BM * k * (sizeof(float) + sizeof(int));
}

template <bool SELF>
__global__ __launch_bounds__(MDE_BLOCK) void k_bits_knn(int n_q, int n_c, int nw, int nf, int kind, int k,
                                                        int64_t slice_cols, const uint32_t* __restrict__ Q,
                                                        const int32_t* __restrict__ qcnt,
                                                        const uint32_t* __restrict__ C,
                                                        const int32_t* __restrict__ ccnt,
                                                        int32_t* __restrict__ idx_out, float* __restrict__ d_out) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  uint32_t* sA = reinterpret_cast<uint32_t*>(lds);   // [BITS_KB][BITS_LD]
  uint32_t* sB = sA + BITS_KB * BITS_LD;             // [BITS_KB][BITS_LD]
  float* sD = reinterpret_cast<float*>(sB + BITS_KB * BITS_LD);   // [BITS_BM][BITS_BN + 1] distances of the tile
  float* sWorst = sD + BITS_BM * (BITS_BN + 1);      // [BITS_BM] the k-th best of every row
  int* sHit = reinterpret_cast<int*>(sWorst + BITS_BM);   // [BITS_BM] the tile holds a value below it
  float* bestd = reinterpret_cast<float*>(sHit + BITS_BM);   // [BITS_BM][k]
  int* besti = reinterpret_cast<int*>(bestd + BITS_BM * k);  // [BITS_BM][k]
  const int tid = threadIdx.x;
  const int tx = tid & 15, ty = tid >> 4;
  const int sc = tid & 31, sg = tid >> 5;
  const int64_t row0 = (int64_t)blockIdx.x * BITS_BM;
  const int64_t lo = (int64_t)blockIdx.y * slice_cols;
  const int64_t c_lo = lo < n_c ? lo : n_c, c_hi = lo + slice_cols < n_c ? lo + slice_cols : n_c;
  knn_lists_init(bestd, besti, BITS_BM * k);
  if (tid < BITS_BM) {
    sWorst[tid] = 3.402823466e+38f;
    sHit[tid] = 0;
  }
  float worst = 3.402823466e+38f;            // thread t < 64: current k-th best of row t
  int qa[4];                                 // the counts of this thread's four query rows
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int64_t gr = row0 + ty * 4 + i;
    qa[i] = qcnt[gr < n_q ? gr : n_q - 1];
  }
  for (int64_t col0 = c_lo; col0 < c_hi; col0 += BITS_BN) {
    uint32_t acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[i][j] = 0u;
    int cb[4];                               // the counts of this thread's four candidates
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int64_t gc = col0 + tx * 4 + j;
      cb[j] = ccnt[gc < n_c ? gc : n_c - 1];
    }
    uint32_t ra[2][4], rb[2][4];
    auto fetch = [&](int k0) {
      const int w = k0 + sc;
      const int wc = w < nw ? w : nw - 1;
#pragma unroll
      for (int q = 0; q < 2; ++q)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int r = (sg + 8 * q) * 4 + i;
          const int64_t gr = row0 + r, gc = col0 + r;
          // plain loads from clamped addresses, zeroed afterwards (as k_knn_l1: no branch around a load)
          const uint32_t va = Q[(gr < n_q ? gr : n_q - 1) * nw + wc];
          const uint32_t vb = C[(gc < n_c ? gc : n_c - 1) * nw + wc];
          ra[q][i] = (gr < n_q && w < nw) ? va : 0u;
          rb[q][i] = (gc < n_c && w < nw) ? vb : 0u;
        }
    };
    fetch(0);
    for (int k0 = 0; k0 < nw; k0 += BITS_KB) {
      __syncthreads();
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        const int o = sc * BITS_LD + (sg + 8 * q) * 4;
        *reinterpret_cast<uint4*>(sA + o) = make_uint4(ra[q][0], ra[q][1], ra[q][2], ra[q][3]);
        *reinterpret_cast<uint4*>(sB + o) = make_uint4(rb[q][0], rb[q][1], rb[q][2], rb[q][3]);
      }
      __syncthreads();
      if (k0 + BITS_KB < nw) fetch(k0 + BITS_KB);
      const uint32_t* pa = sA + ty * 4;
      const uint32_t* pb = sB + tx * 4;
      const int kn = nw - k0 < BITS_KB ? nw - k0 : BITS_KB;   // words past nw are zero: skipped, not summed
      auto step = [&](int f) {
        const uint4 a4 = *reinterpret_cast<const uint4*>(pa + f * BITS_LD);
        const uint4 b4 = *reinterpret_cast<const uint4*>(pb + f * BITS_LD);
        const uint32_t a[4] = {a4.x, a4.y, a4.z, a4.w};
        const uint32_t b[4] = {b4.x, b4.y, b4.z, b4.w};
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j) acc[i][j] += __popc(a[i] & b[j]);
      };
      if (kn == BITS_KB) {
#pragma unroll
        for (int f = 0; f < BITS_KB; ++f) step(f);
      } else {
        for (int f = 0; f < kn; ++f) step(f);
      }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int r = ty * 4 + i;
      const int64_t gr = row0 + r;
      const float wr = sWorst[r];
      bool hit = !BITS_PRECHECK;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int c = tx * 4 + j;
        const int64_t gc = col0 + c;
        float d = 3.402823466e+38f;
        if (gr < n_q && gc < n_c && !(SELF && gr == gc)) d = bits_distance(qa[i], cb[j], (int)acc[i][j], nf, kind);
        sD[r * (BITS_BN + 1) + c] = d;
        hit = hit || d < wr;
      }
      if (hit) sHit[r] = 1;
    }
    __syncthreads();
    if (tid < BITS_BM && sHit[tid]) {
      mde_topk_merge(sD + tid * (BITS_BN + 1), BITS_BN, (int)col0, k, bestd + tid * k, besti + tid * k, worst);
      sWorst[tid] = worst;
      sHit[tid] = 0;
    }
  }
  __syncthreads();
  const int rows = n_q - row0 < BITS_BM ? (int)(n_q - row0) : BITS_BM;
  const int64_t base = ((int64_t)blockIdx.y * n_q + row0) * k;   // the block's rows are contiguous in list y
  knn_lists_store(bestd, besti, rows * k, idx_out + base, d_out + base);
}

static bool bits_knn_args_ok(int64_t n_q, int64_t n_c, int32_t k, int32_t slices) {
  return cross_args_ok(n_q, n_c, k, slices) && n_q < ((int64_t)1 << 31) && n_c < ((int64_t)1 << 31);
}

extern "C" int64_t mde_bits_knn_work_bytes(int64_t n_q, int64_t n_c, int32_t k, int32_t slices) {
  if (!bits_knn_args_ok(n_q, n_c, k, slices)) {
    mde_set_error("mde_bits_knn_work_bytes: invalid arguments (1 <= k <= %d, 0 <= slices <= %d, 1 <= n_q, n_c < 2^31)",
                  KNN_MAXK, CROSS_MAX_SLICES);
    return MDE_E_INVALID;
  }
  const int64_t s = cross_resolve_slices(n_q, n_c, slices);
  if (s < 0) return s;
  // the partial lists, d and idx, [s, n_q, k] each; never zero bytes, so that `work` is a pointer
  return s > 1 ? 8 * s * n_q * (int64_t)k : 8;
}

extern "C" int mde_bits_knn(int64_t n_q, int64_t n_c, int32_t nw, int32_t nf, const int32_t* Q, const int32_t* q_counts,
                            const int32_t* C, const int32_t* c_counts, int32_t self, int32_t kind, int32_t k,
                            int32_t slices, int32_t* idx_out, float* dist_out, void* work, void* stream) {
  if (!bits_knn_args_ok(n_q, n_c, k, slices) || nf <= 0 || nf >= BITS_MAX_NF || nw != (nf + 31) / 32 || !Q ||
      !q_counts || !C || !c_counts || !idx_out || !dist_out || !work ||
      (kind != BITS_JACCARD && kind != BITS_HAMMING)) {
    mde_set_error("mde_bits_knn: invalid arguments (1 <= k <= %d, 0 <= slices <= %d, 1 <= n_q, n_c < 2^31, "
                  "1 <= nf < 2^24, nw == ceil(nf / 32), kind 0 or 1, non-null pointers)", KNN_MAXK, CROSS_MAX_SLICES);
    return MDE_E_INVALID;
  }
  if (self && (Q != C || n_q != n_c || q_counts != c_counts)) {
    mde_set_error("mde_bits_knn: self != 0 needs Q == C, q_counts == c_counts and n_q == n_c");
    return MDE_E_INVALID;
  }
  const int64_t s = cross_resolve_slices(n_q, n_c, slices);
  if (s < 0) return (int)s;
  hipStream_t st = mde_stream(stream);
  float* pd = static_cast<float*>(work);                        // [s, n_q, k], used when s > 1
  int32_t* pi = reinterpret_cast<int32_t*>(pd + s * n_q * (int64_t)k);
  int rc = self ? knn_raise_lds_limit<k_bits_knn<true>>(96 * 1024) : knn_raise_lds_limit<k_bits_knn<false>>(96 * 1024);
  if (rc == MDE_OK) rc = knn_raise_lds_limit<k_knn_cross_merge>(96 * 1024);
  if (rc != MDE_OK) return rc;
  const int64_t tiles = (n_c + BITS_BN - 1) / BITS_BN;
  const int64_t slice_cols = ((tiles + s - 1) / s) * BITS_BN;   // whole tiles; the last slices may be short or empty
  const unsigned qb = (unsigned)((n_q + BITS_BM - 1) / BITS_BM);
  const uint32_t* Qu = reinterpret_cast<const uint32_t*>(Q);
  const uint32_t* Cu = reinterpret_cast<const uint32_t*>(C);
  if (self)
    hipLaunchKernelGGL(k_bits_knn<true>, dim3(qb, (unsigned)s), dim3(MDE_BLOCK), bits_knn_lds_bytes(k), st, (int)n_q,
                       (int)n_c, nw, nf, kind, k, slice_cols, Qu, q_counts, Cu, c_counts, s > 1 ? pi : idx_out,
                       s > 1 ? pd : dist_out);
  else
    hipLaunchKernelGGL(k_bits_knn<false>, dim3(qb, (unsigned)s), dim3(MDE_BLOCK), bits_knn_lds_bytes(k), st, (int)n_q,
                       (int)n_c, nw, nf, kind, k, slice_cols, Qu, q_counts, Cu, c_counts, s > 1 ? pi : idx_out,
                       s > 1 ? pd : dist_out);
  MDE_LAUNCH_CHECK();
  if (s > 1) {
    hipLaunchKernelGGL(k_knn_cross_merge, dim3(qb), dim3(MDE_BLOCK), knn_cross_merge_lds_bytes(k), st, (int)n_q, k,
                       (int)s, pd, pi, idx_out, dist_out);
    MDE_LAUNCH_CHECK();
  }
  return MDE_OK;
}

// ------------------------------------------------------------------ listed pairs
// One wave per edge: the lanes share the words of the two rows, the intersection is a wave sum of integers, and
// lane 0 forms the value by bits_distance -- the bits the search gives the pair.  NaN for an endpoint outside
// [0, n), as mde_pair_distances_metric.
__global__ __launch_bounds__(MDE_BLOCK) void k_bits_pair(int64_t n, int nw, int nf, const uint32_t* __restrict__ W,
                                                         const int32_t* __restrict__ counts, int64_t p,
                                                         const int64_t* __restrict__ edges, int kind,
                                                         float* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int64_t w0 = ((int64_t)blockIdx.x * MDE_BLOCK + threadIdx.x) >> 6;
  const int64_t nwv = ((int64_t)gridDim.x * MDE_BLOCK) >> 6;
  for (int64_t q = w0; q < p; q += nwv) {
    const int64_t i = edges[2 * q], j = edges[2 * q + 1];
    if (i < 0 || i >= n || j < 0 || j >= n) {
      if (lane == 0) out[q] = __int_as_float(0x7fc00000);
      continue;
    }
    int t = 0;
    for (int w = lane; w < nw; w += 64) t += __popc(W[i * nw + w] & W[j * nw + w]);
    t = mde_wave_sum(t);
    if (lane == 0) out[q] = bits_distance(counts[i], counts[j], t, nf, kind);
  }
}

extern "C" int mde_bits_pair_distances(int64_t n, int32_t nw, int32_t nf, const int32_t* words, const int32_t* counts,
                                       int64_t p, const int64_t* edges, int32_t kind, float* out, void* stream) {
  if (n <= 0 || nf <= 0 || nf >= BITS_MAX_NF || nw != (nf + 31) / 32 || !words || !counts || p < 0 ||
      (p > 0 && (!edges || !out)) || (kind != BITS_JACCARD && kind != BITS_HAMMING)) {
    mde_set_error("mde_bits_pair_distances: invalid arguments (n >= 1, 1 <= nf < 2^24, nw == ceil(nf / 32), p >= 0, "
                  "kind 0 or 1)");
    return MDE_E_INVALID;
  }
  if (p == 0) return MDE_OK;
  hipLaunchKernelGGL(k_bits_pair, dim3(mde_grid(p * 64, MDE_BLOCK, 8192)), dim3(MDE_BLOCK), 0, mde_stream(stream), n,
                     nw, nf, reinterpret_cast<const uint32_t*>(words), counts, p, edges, kind, out);
  MDE_LAUNCH_CHECK();
  return MDE_OK;
}

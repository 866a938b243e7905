// mde_knn_rank.hip -- the rank of listed corpus rows among all corpus rows of a query: what
// trustworthiness, continuity and the k-NN overlap of pymde_amd.quality are computed from.
//
// rank(i, j) = the number of corpus rows l with (d2(i, l), l) < (d2(i, j), j), lexicographically, l != i in a
// self-join: 0-based, ties to the smaller index -- the order every k-NN kernel here lists by.  d2 is the float32
// squared distance of the Euclidean kernels, bit for bit, so the ranks of mde_knn's own lists are 0 .. k - 1.
//
//   k_knn_rank_thresholds  t[i][c] = d2(i, idx[i][c]) by the chain of k_knn_rerank (knn_wave_pair_d2)
//   k_knn_rank<SELF>       one pass of the Gram tile of mde_knn_tile.h on the grid of k_knn_cross; every query
//                          row counts the parked distances that precede each of its thresholds
//   k_knn_rank_fold        sums the per-slice counts (integers: any slice count gives the same ranks)
// and mde_knn_list_overlap, the row-wise intersection size of two neighbour lists.
#include "mde_knn_tile.h"
#include "mde_knn_slices.h"

#define RANK_FLT_MAX 3.402823466e+38f
#define RANK_PER_THREAD (KNN_MAXK / 4)   // thresholds of a thread: c = wave + 4 i
#define RANK_GROUP 4                     // thresholds compared per read of a parked distance

// A wave owns one query row and a lane one entry of its list (m <= 64 lanes).  An entry that names no corpus
// row (negative, or >= n_c) or, in a self-join, the query's own row is not ranked: threshold FLT_MAX, index -1.
__global__ __launch_bounds__(MDE_BLOCK) void k_knn_rank_thresholds(int n_q, int n_c, int nf, int m, int self,
                                                                   const float* __restrict__ Q,
                                                                   const float* __restrict__ C,
                                                                   const float* __restrict__ qn,
                                                                   const float* __restrict__ cn,
                                                                   const int32_t* __restrict__ idx,
                                                                   float* __restrict__ t_out,
                                                                   int32_t* __restrict__ j_out,
                                                                   float* __restrict__ d2_out) {
  __shared__ float sC[4][64 * KNN_RR_KBP];
  __shared__ float sQ[4][KNN_RR_KB];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t q = (int64_t)blockIdx.x * 4 + wave;
  const int64_t qc = q < n_q ? q : n_q - 1;
  const int mine = lane < m ? idx[qc * m + lane] : -1;
  const bool valid = mine >= 0 && mine < n_c && !(self && mine == qc);
  const int64_t crow = valid ? mine : 0;
  const float d2 = knn_wave_pair_d2(sC[wave], sQ[wave], nf, Q, C, qn, cn, qc, crow, valid);
  if (q < n_q && lane < m) {
    t_out[q * m + lane] = d2;
    j_out[q * m + lane] = valid ? mine : -1;
    if (d2_out) d2_out[q * m + lane] = d2;
  }
}

// The count.  Workgroup (x, y) owns query rows [64 x, 64 x + 64) and the corpus columns of slice y, as
// k_knn_cross does, and parks every 64-column tile of squared distances in sD the same way (what does not
// exist, and the row itself when SELF, is FLT_MAX and precedes nothing).  Thread t owns tile row t & 63 and the
// list entries c = (t >> 6) + 4 i, i < 16, of that row: thresholds, indices and counts stay in registers (every
// loop over them is unrolled, and the groups beyond the wave's entries are skipped by a wave-uniform test).
// It walks the 64 parked distances of its row -- the 64 lanes of a wave read 64 rows at stride 65:
// conflict-free -- and compares each with RANK_GROUP thresholds at a time.  The counts go to list y of
// [slices, n_q, m]; `final` (one slice): they are the ranks, -1 for the entries that are not ranked.
template <bool SELF>
__global__ __launch_bounds__(MDE_BLOCK) void k_knn_rank(int n_q, int n_c, int nf, int m, int64_t slice_cols, int final,
                                                        const float* __restrict__ Q, const float* __restrict__ C,
                                                        const float* __restrict__ qn, const float* __restrict__ cn,
                                                        const float* __restrict__ thr,
                                                        const int32_t* __restrict__ jv,
                                                        int32_t* __restrict__ count_out) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const knn_tile_lds s = knn_tile_carve(lds, 0, 0);
  const int tid = threadIdx.x, r = tid & 63, w = tid >> 6;
  const int64_t row0 = (int64_t)blockIdx.x * KNN_BM;
  const int64_t lo = (int64_t)blockIdx.y * slice_cols;
  const int64_t c_lo = lo < n_c ? lo : n_c, c_hi = lo + slice_cols < n_c ? lo + slice_cols : n_c;
  const bool rok = row0 + r < n_q;
  const int64_t mybase = (row0 + r) * m;
  // entries of this wave, and their groups of RANK_GROUP
  const int nt = w < m ? (m - w + 3) / 4 : 0;
  const int ng = (nt + RANK_GROUP - 1) / RANK_GROUP;
  float t[RANK_PER_THREAD];
  int j[RANK_PER_THREAD], cnt[RANK_PER_THREAD];
#pragma unroll
  for (int i = 0; i < RANK_PER_THREAD; ++i) {
    const int c = w + 4 * i;
    const bool have = rok && c < m;
    t[i] = have ? thr[mybase + c] : -1.0f;    // no squared distance precedes -1
    j[i] = have ? jv[mybase + c] : -1;
    cnt[i] = 0;
  }
  const float* arow[KNN_STG];
  bool aok[KNN_STG];
#pragma unroll
  for (int q = 0; q < KNN_STG; ++q) {
    const int64_t gr = row0 + (tid >> 5) + 8 * q;
    aok[q] = gr < n_q;
    arow[q] = Q + (aok[q] ? gr : n_q - 1) * nf;
  }
  for (int64_t col0 = c_lo; col0 < c_hi; col0 += KNN_BN) {
    const float* brow[KNN_STG];
    bool bok[KNN_STG];
#pragma unroll
    for (int q = 0; q < KNN_STG; ++q) {
      const int64_t gc = col0 + (tid >> 5) + 8 * q;
      bok[q] = gc < n_c;
      brow[q] = C + (bok[q] ? gc : n_c - 1) * nf;
    }
    const f32x16 acc = knn_gram_tile(s.sA, s.sB, nf, arow, aok, brow, bok);
    knn_park_tile(
        s.sD, acc,
        [&](int rr, int cc) { return row0 + rr < n_q && col0 + cc < n_c && !(SELF && row0 + rr == col0 + cc); },
        [&](int rr) { return qn[row0 + rr]; }, [&](int cc) { return cn[col0 + cc]; });
    __syncthreads();
    const float* mine = s.sD + r * (KNN_BN + 1);
#pragma unroll
    for (int g = 0; g < RANK_PER_THREAD / RANK_GROUP; ++g) {
      if (g < ng) {
        // tile column cc precedes the listed row j on a tie when col0 + cc < j
        int jr[RANK_GROUP], a[RANK_GROUP];
#pragma unroll
        for (int u = 0; u < RANK_GROUP; ++u) {
          const int64_t rel = (int64_t)j[RANK_GROUP * g + u] - col0;
          jr[u] = rel > KNN_BN ? KNN_BN : (rel < 0 ? 0 : (int)rel);
          a[u] = 0;
        }
#pragma unroll 8
        for (int cc = 0; cc < KNN_BN; ++cc) {
          const float d = mine[cc];
#pragma unroll
          for (int u = 0; u < RANK_GROUP; ++u) {
            const float tu = t[RANK_GROUP * g + u];
            a[u] += (d < tu || (d == tu && cc < jr[u])) ? 1 : 0;
          }
        }
#pragma unroll
        for (int u = 0; u < RANK_GROUP; ++u) cnt[RANK_GROUP * g + u] += a[u];
      }
    }
    // the next tile's park follows the barriers of its knn_gram_tile: every thread is past this walk by then
  }
  if (rok) {
    int32_t* out = count_out + (int64_t)blockIdx.y * n_q * m + mybase;
#pragma unroll
    for (int i = 0; i < RANK_PER_THREAD; ++i) {
      const int c = w + 4 * i;
      if (c < m) out[c] = (final && j[i] < 0) ? -1 : cnt[i];
    }
  }
}

__global__ __launch_bounds__(MDE_BLOCK) void k_knn_rank_fold(int64_t total, int slices,
                                                             const int32_t* __restrict__ part,
                                                             const int32_t* __restrict__ jv,
                                                             int32_t* __restrict__ rank_out) {
  for (int64_t i = (int64_t)blockIdx.x * MDE_BLOCK + threadIdx.x; i < total; i += (int64_t)gridDim.x * MDE_BLOCK) {
    int sum = 0;
    for (int y = 0; y < slices; ++y) sum += part[(int64_t)y * total + i];
    rank_out[i] = jv[i] < 0 ? -1 : sum;
  }
}

static bool rank_args_ok(int64_t n_q, int64_t n_c, int32_t m, int32_t slices) {
  return cross_args_ok(n_q, n_c, m, slices) && n_q < ((int64_t)1 << 31) && n_c < ((int64_t)1 << 31);
}

extern "C" int64_t mde_knn_ranks_work_bytes(int64_t n_q, int64_t n_c, int32_t m, int32_t slices) {
  if (!rank_args_ok(n_q, n_c, m, slices)) {
    mde_set_error("mde_knn_ranks_work_bytes: invalid arguments (1 <= m <= %d, 0 <= slices <= %d, 1 <= n_q, n_c < "
                  "2^31)", KNN_MAXK, CROSS_MAX_SLICES);
    return MDE_E_INVALID;
  }
  const int64_t s = cross_resolve_slices(n_q, n_c, slices);
  if (s < 0) return s;
  int64_t words = n_q + n_c + 2 * n_q * (int64_t)m;     // the row norms of Q and C, the thresholds and their indices
  if (s > 1) words += s * n_q * (int64_t)m;             // the per-slice counts
  return 4 * words;
}

extern "C" int mde_knn_ranks(int64_t n_q, int64_t n_c, int32_t nf, const float* Q, const float* C, int32_t self,
                             int32_t m, const int32_t* idx, int32_t slices, int32_t* rank_out, float* d2_out,
                             void* work, void* stream) {
  if (!rank_args_ok(n_q, n_c, m, slices) || nf <= 0 || !Q || !C || !idx || !rank_out || !work ||
      (self && (Q != C || n_q != n_c))) {
    mde_set_error("mde_knn_ranks: invalid arguments (1 <= m <= %d, 0 <= slices <= %d, 1 <= n_q, n_c < 2^31, nf >= 1, "
                  "non-null Q / C / idx / rank_out / work; self != 0 needs Q == C and n_q == n_c)",
                  KNN_MAXK, CROSS_MAX_SLICES);
    return MDE_E_INVALID;
  }
  const int64_t s = cross_resolve_slices(n_q, n_c, slices);
  if (s < 0) return (int)s;
  hipStream_t st = mde_stream(stream);
  const int64_t total = n_q * (int64_t)m;
  float* qn = static_cast<float*>(work);
  float* cn = qn + n_q;
  float* thr = cn + n_c;                                         // [n_q, m]
  int32_t* jv = reinterpret_cast<int32_t*>(thr + total);         // [n_q, m]
  int32_t* part = jv + total;                                    // [s, n_q, m], used when s > 1
  int rc = mde_row_sqnorm(n_q, nf, Q, qn, stream);
  if (rc == MDE_OK) rc = mde_row_sqnorm(n_c, nf, C, cn, stream);
  if (rc != MDE_OK) return rc;
  hipLaunchKernelGGL(k_knn_rank_thresholds, dim3((unsigned)((n_q + 3) / 4)), dim3(MDE_BLOCK), 0, st, (int)n_q,
                     (int)n_c, nf, m, self != 0, Q, C, qn, cn, idx, thr, jv, d2_out);
  MDE_LAUNCH_CHECK();
  const int64_t tiles = (n_c + KNN_BN - 1) / KNN_BN;
  const int64_t slice_cols = ((tiles + s - 1) / s) * KNN_BN;     // whole tiles; the last slices may be short or empty
  const dim3 grid((unsigned)((n_q + KNN_BM - 1) / KNN_BM), (unsigned)s);
  const size_t lds = knn_tile_lds_bytes(0, 0);                   // the lists of this kernel live in registers
  int32_t* counts = s > 1 ? part : rank_out;
  if (self)
    hipLaunchKernelGGL(k_knn_rank<true>, grid, dim3(MDE_BLOCK), lds, st, (int)n_q, (int)n_c, nf, m, slice_cols,
                       (int)(s == 1), Q, C, qn, cn, thr, jv, counts);
  else
    hipLaunchKernelGGL(k_knn_rank<false>, grid, dim3(MDE_BLOCK), lds, st, (int)n_q, (int)n_c, nf, m, slice_cols,
                       (int)(s == 1), Q, C, qn, cn, thr, jv, counts);
  MDE_LAUNCH_CHECK();
  if (s > 1) {
    hipLaunchKernelGGL(k_knn_rank_fold, dim3(mde_grid(total, MDE_BLOCK, 4096)), dim3(MDE_BLOCK), 0, st, total, (int)s,
                       part, jv, rank_out);
    MDE_LAUNCH_CHECK();
  }
  return MDE_OK;
}

// One thread per row: count_out[i] = the number of entries of a[i] (>= 0) that occur in b[i].
__global__ __launch_bounds__(MDE_BLOCK) void k_knn_list_overlap(int64_t n, int ka, const int32_t* __restrict__ a,
                                                                int kb, const int32_t* __restrict__ b,
                                                                int32_t* __restrict__ count_out) {
  for (int64_t i = (int64_t)blockIdx.x * MDE_BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * MDE_BLOCK) {
    const int32_t* ra = a + i * ka;
    const int32_t* rb = b + i * kb;
    int count = 0;
    for (int x = 0; x < ka; ++x) {
      const int v = ra[x];
      bool found = false;
      for (int y = 0; y < kb; ++y) found = found || rb[y] == v;
      count += (v >= 0 && found) ? 1 : 0;
    }
    count_out[i] = count;
  }
}

extern "C" int mde_knn_list_overlap(int64_t n, int32_t ka, const int32_t* a, int32_t kb, const int32_t* b,
                                    int32_t* count_out, void* stream) {
  if (n <= 0 || ka <= 0 || ka > KNN_MAXK || kb <= 0 || kb > KNN_MAXK || !a || !b || !count_out) {
    mde_set_error("mde_knn_list_overlap: invalid arguments (n >= 1, 1 <= ka, kb <= %d, non-null a / b / count_out)",
                  KNN_MAXK);
    return MDE_E_INVALID;
  }
  hipLaunchKernelGGL(k_knn_list_overlap, dim3(mde_grid(n, MDE_BLOCK, 4096)), dim3(MDE_BLOCK), 0, mde_stream(stream), n,
                     ka, a, kb, b, count_out);
  MDE_LAUNCH_CHECK();
  return MDE_OK;
}

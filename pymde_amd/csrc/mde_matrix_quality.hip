// mde_matrix_quality.hip -- an embedding scored against a matrix of dissimilarities: the sums,
// the Shepard counts and the ranks that pymde_amd.quality's matrix_* and graph_* functions are computed from, where
// the data-side distance is read from a matrix (shortest-path lengths, a caller's matrix) instead of formed from rows.
//
// Dm [n, m] float32 row-major: row i is item i, column b holds the dissimilarity to item items[b] (NULL: b itself).
// A pair (i, b) counts unless items[b] == i or Dm[i][b] is not finite or is FLT_MAX (a missing pair).  For a counted
// pair D = Dm[i][b] and E = |x_i - x_items[b]| = sqrtf of the fmaf chain over the d differences, as mde_pair_loss.
//
//   k_matrix_walk<DC, HIST>  a wave owns MQ_ROWS rows of a 16-row block and walks their columns, lane l the columns
//                            l, l + 64, ...: every wave-load is a 256-byte piece of one row.  The lane reads
//                            items[b] and x_items[b] once per column and uses them for its MQ_ROWS rows; the x of the
//                            rows themselves are wave-uniform.  Element offsets are 64-bit.
//       HIST = false         five double accumulators, two float maxima and a count per row and lane; the 64 lanes
//                            are combined by the xor butterfly, a fixed tree.  A row's result depends on n, m and
//                            the inputs only, not on the grid.
//       HIST = true          the counted pairs increment a bins x bins uint32 block in LDS, flushed once per
//                            workgroup with 64-bit integer atomics; a workgroup takes several row blocks, and the
//                            columns are cut so that none of its counters can wrap.
//   k_matrix_chunk_totals    one workgroup per MQ_CHUNK rows (a constant: the order is fixed) -> partial [8]
//   k_matrix_final_totals    one workgroup adds the partials in chunk order -> totals [8]
//   k_matrix_rank_init       ranks[b][c] = 0, or -1 for an entry that is not ranked
//   k_matrix_rank_count<KC>  workgroup (x, y) owns the 64 columns 64 x ... (lane = column) and the rows of slice y;
//                            the thresholds Dm[l][b] and their rows l sit in LDS at [c][lane]; a wave loads MQ_RR rows
//                            at a time and every lane counts, per list entry, the loaded values that precede it in
//                            the order (value, row).  Integer atomics into ranks: the same for every grid.
#include "mde_common.h"

#define MQ_FLT_MAX 3.402823466e+38f
#define MQ_ROWS 4                       // rows of a wave in the walk
#define MQ_BLOCK_ROWS (4 * MQ_ROWS)     // rows of a workgroup (4 waves)
#define MQ_MAX_BINS 64
#define MQ_MAX_D 8
#define MQ_MAX_K 64
#define MQ_CHUNK 4096                   // rows per workgroup of the totals' first pass
#define MQ_RR 8                         // rows a wave of the rank kernel holds at a time
#define MQ_HIST_GRID 1024               // workgroups along the rows of the histogram walk, at most

template <int DC, bool HIST>
__global__ __launch_bounds__(MDE_BLOCK) void k_matrix_walk(int n, int m, int d, int64_t slice_cols,
                                                           const float* __restrict__ Dm,
                                                           const int32_t* __restrict__ items,
                                                           const float* __restrict__ X, double* __restrict__ row_sums,
                                                           long long* __restrict__ row_count,
                                                           float* __restrict__ row_max, int bins, float a_lo,
                                                           float a_hi, float a_scale, float b_lo, float b_hi,
                                                           float b_scale, unsigned long long* __restrict__ counts) {
  __shared__ unsigned int hist[HIST ? MQ_MAX_BINS * MQ_MAX_BINS : 1];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (HIST) {
    for (int i = threadIdx.x; i < bins * bins; i += MDE_BLOCK) hist[i] = 0u;
    __syncthreads();
  }
  const int64_t c_lo = (int64_t)blockIdx.y * slice_cols;
  const int64_t c_hi = c_lo + slice_cols < m ? c_lo + slice_cols : m;
  const int64_t row_blocks = ((int64_t)n + MQ_BLOCK_ROWS - 1) / MQ_BLOCK_ROWS;
  for (int64_t rb = blockIdx.x; rb < row_blocks; rb += gridDim.x) {
    const int64_t row0 = rb * MQ_BLOCK_ROWS + wave * MQ_ROWS;
    float xi[MQ_ROWS][DC];
    const float* drow[MQ_ROWS];
    bool rok[MQ_ROWS];
#pragma unroll
    for (int r = 0; r < MQ_ROWS; ++r) {
      rok[r] = row0 + r < n;
      const int64_t gi = rok[r] ? row0 + r : n - 1;
      drow[r] = Dm + gi * (int64_t)m;
#pragma unroll
      for (int k = 0; k < DC; ++k) xi[r][k] = k < d ? X[gi * d + k] : 0.0f;
    }
    double sd[MQ_ROWS], se[MQ_ROWS], sdd[MQ_ROWS], see[MQ_ROWS], sde[MQ_ROWS];
    float md[MQ_ROWS], me[MQ_ROWS];
    int cnt[MQ_ROWS];
#pragma unroll
    for (int r = 0; r < MQ_ROWS; ++r) {
      sd[r] = se[r] = sdd[r] = see[r] = sde[r] = 0.0;
      md[r] = me[r] = 0.0f;
      cnt[r] = 0;
    }
#pragma unroll 2
    for (int64_t b = c_lo + lane; b < c_hi; b += 64) {
      float v[MQ_ROWS];
#pragma unroll
      for (int r = 0; r < MQ_ROWS; ++r) v[r] = drow[r][b];
      const int64_t it = items ? (int64_t)items[b] : b;
      float xj[DC];
#pragma unroll
      for (int k = 0; k < DC; ++k) xj[k] = k < d ? X[it * d + k] : 0.0f;
#pragma unroll
      for (int r = 0; r < MQ_ROWS; ++r) {
        const bool have = rok[r] && it != row0 + r && fabsf(v[r]) < MQ_FLT_MAX;   // false for NaN and +-inf too
        float ss = 0.0f;
#pragma unroll
        for (int k = 0; k < DC; ++k) {
          const float diff = xi[r][k] - xj[k];
          ss = fmaf(diff, diff, ss);
        }
        const float D = have ? v[r] : 0.0f;
        const float E = have ? sqrtf(ss) : 0.0f;
        if (HIST) {
          if (have && D >= a_lo && D <= a_hi && E >= b_lo && E <= b_hi) {
            int bd = (int)((D - a_lo) * a_scale), be = (int)((E - b_lo) * b_scale);
            bd = bd < bins - 1 ? bd : bins - 1;
            be = be < bins - 1 ? be : bins - 1;
            atomicAdd(&hist[bd * bins + be], 1u);
          }
        } else {
          const double Dd = (double)D, Ed = (double)E;          // a pair that does not count adds 0.0: no change
          sd[r] += Dd;
          se[r] += Ed;
          sdd[r] = fma(Dd, Dd, sdd[r]);
          see[r] = fma(Ed, Ed, see[r]);
          sde[r] = fma(Dd, Ed, sde[r]);
          md[r] = fmaxf(md[r], D);
          me[r] = fmaxf(me[r], E);
          cnt[r] += have ? 1 : 0;
        }
      }
    }
    if (!HIST) {
#pragma unroll
      for (int r = 0; r < MQ_ROWS; ++r) {
        const double t0 = mde_wave_sum(sd[r]), t1 = mde_wave_sum(se[r]), t2 = mde_wave_sum(sdd[r]);
        const double t3 = mde_wave_sum(see[r]), t4 = mde_wave_sum(sde[r]);
        const float u0 = mde_wave_max(md[r]), u1 = mde_wave_max(me[r]);
        const long long c = mde_wave_sum((long long)cnt[r]);
        if (lane == 0 && rok[r]) {
          double* out = row_sums + (row0 + r) * 5;
          out[0] = t0;
          out[1] = t1;
          out[2] = t2;
          out[3] = t3;
          out[4] = t4;
          row_max[(row0 + r) * 2 + 0] = u0;
          row_max[(row0 + r) * 2 + 1] = u1;
          row_count[row0 + r] = c;
        }
      }
    }
  }
  if (HIST) {
    __syncthreads();
    for (int i = threadIdx.x; i < bins * bins; i += MDE_BLOCK) {
      const unsigned int v = hist[i];
      if (v) atomicAdd(counts + i, (unsigned long long)v);
    }
  }
}

// The 256 threads' eight values, added (5, 6: the largest) in thread order by threads 0 .. 7.
__device__ __forceinline__ void mq_fold8(const double t[8], double* __restrict__ out) {
  __shared__ double part[MDE_BLOCK][8];
#pragma unroll
  for (int v = 0; v < 8; ++v) part[threadIdx.x][v] = t[v];
  __syncthreads();
  if (threadIdx.x < 8) {
    const int v = threadIdx.x;
    const bool is_max = v == 5 || v == 6;
    double a = part[0][v];
    for (int u = 1; u < MDE_BLOCK; ++u) a = is_max ? (part[u][v] > a ? part[u][v] : a) : a + part[u][v];
    out[v] = a;
  }
}

// Workgroup c: thread t adds the rows c MQ_CHUNK + t, + 256, ... in row order.  out = sum D, E, D^2, E^2, D E,
// max D, max E, the count.
__global__ __launch_bounds__(MDE_BLOCK) void k_matrix_chunk_totals(int64_t n, const double* __restrict__ row_sums,
                                                                   const long long* __restrict__ row_count,
                                                                   const float* __restrict__ row_max,
                                                                   double* __restrict__ out) {
  const int64_t lo = (int64_t)blockIdx.x * MQ_CHUNK;
  const int64_t hi = lo + MQ_CHUNK < n ? lo + MQ_CHUNK : n;
  double t[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int64_t i = lo + threadIdx.x; i < hi; i += MDE_BLOCK) {
#pragma unroll
    for (int v = 0; v < 5; ++v) t[v] += row_sums[i * 5 + v];
#pragma unroll
    for (int v = 0; v < 2; ++v) {
      const double mx = (double)row_max[i * 2 + v];
      t[5 + v] = mx > t[5 + v] ? mx : t[5 + v];
    }
    t[7] += (double)row_count[i];
  }
  mq_fold8(t, out + (int64_t)blockIdx.x * 8);
}

__global__ __launch_bounds__(MDE_BLOCK) void k_matrix_final_totals(int64_t chunks, const double* __restrict__ part,
                                                                   double* __restrict__ totals) {
  double t[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int64_t i = threadIdx.x; i < chunks; i += MDE_BLOCK) {
#pragma unroll
    for (int v = 0; v < 8; ++v) {
      const double p = part[i * 8 + v];
      t[v] = (v == 5 || v == 6) ? (p > t[v] ? p : t[v]) : t[v] + p;
    }
  }
  mq_fold8(t, totals);
}

static bool mq_sizes_ok(int64_t n, int64_t m) {
  return n >= 1 && n < ((int64_t)1 << 31) && m >= 1 && m < ((int64_t)1 << 31);
}

// work: the partial totals, [ceil(n / MQ_CHUNK), 8] doubles (the histogram needs none)
extern "C" int64_t mde_matrix_moments_work_bytes(int64_t n, int64_t m) {
  if (!mq_sizes_ok(n, m)) {
    mde_set_error("mde_matrix_moments_work_bytes: invalid arguments (1 <= n < 2^31, 1 <= m < 2^31)");
    return MDE_E_INVALID;
  }
  return ((n + MQ_CHUNK - 1) / MQ_CHUNK) * 8 * (int64_t)sizeof(double);
}

struct mq_hist_args {
  int32_t bins;
  float a_lo, a_hi, b_lo, b_hi;
  int64_t* counts;
};

template <bool HIST>
static void mq_launch_walk(int dc, dim3 grid, hipStream_t st, int n, int m, int d, int64_t slice_cols, const float* Dm,
                           const int32_t* items, const float* X, double* row_sums, long long* row_count,
                           float* row_max, const mq_hist_args* h) {
  const int bins = h ? h->bins : 0;
  const float a_lo = h ? h->a_lo : 0.0f, a_hi = h ? h->a_hi : 0.0f, b_lo = h ? h->b_lo : 0.0f;
  const float b_hi = h ? h->b_hi : 0.0f;
  const float a_scale = h ? (float)bins / (a_hi - a_lo) : 0.0f, b_scale = h ? (float)bins / (b_hi - b_lo) : 0.0f;
  unsigned long long* counts = h ? reinterpret_cast<unsigned long long*>(h->counts) : nullptr;
#define MQ_WALK(DC)                                                                                                   \
  hipLaunchKernelGGL((k_matrix_walk<DC, HIST>), grid, dim3(MDE_BLOCK), 0, st, n, m, d, slice_cols, Dm, items, X,      \
                     row_sums, row_count, row_max, bins, a_lo, a_hi, a_scale, b_lo, b_hi, b_scale, counts)
  if (dc == 2)
    MQ_WALK(2);
  else if (dc == 4)
    MQ_WALK(4);
  else
    MQ_WALK(8);
#undef MQ_WALK
}

static int mq_run(const char* who, int64_t n, int64_t m, const float* Dm, const int32_t* items, int32_t d,
                  const float* X, double* row_sums, int64_t* row_count, float* row_max, double* totals,
                  const mq_hist_args* h, void* work, void* stream) {
  const bool hist_ok = !h || (h->bins >= 1 && h->bins <= MQ_MAX_BINS && h->a_hi > h->a_lo && h->b_hi > h->b_lo &&
                              h->counts);
  if (!mq_sizes_ok(n, m) || d < 1 || d > MQ_MAX_D || !Dm || !X || (!items && m != n) || !hist_ok ||
      (!h && (!row_sums || !row_count || !row_max || !totals || !work))) {
    mde_set_error("%s: invalid arguments (1 <= n < 2^31, 1 <= m < 2^31 and m == n without items, 1 <= d <= %d, "
                  "non-null Dm / X / outputs%s)", who, MQ_MAX_D,
                  h ? "; 1 <= bins <= 64, d_hi > d_lo, e_hi > e_lo" : " / work");
    return MDE_E_INVALID;
  }
  hipStream_t st = mde_stream(stream);
  const int dc = d <= 2 ? 2 : (d <= 4 ? 4 : 8);
  const int64_t row_blocks = (n + MQ_BLOCK_ROWS - 1) / MQ_BLOCK_ROWS;
  if (h) {
    // a workgroup takes `per` row blocks and one column slice: per * 16 * slice_cols pairs, kept below 2^31
    const int64_t gx = row_blocks < MQ_HIST_GRID ? row_blocks : MQ_HIST_GRID;
    const int64_t per = (row_blocks + gx - 1) / gx;
    int64_t slice_cols = (((int64_t)1 << 31) - 1) / (per * MQ_BLOCK_ROWS);
    if (slice_cols > m) slice_cols = m;
    const int64_t gy = (m + slice_cols - 1) / slice_cols;
    if (gy > 65535) {
      mde_set_error("%s: a %lld x %lld matrix needs more than 65535 column slices", who, (long long)n, (long long)m);
      return MDE_E_TOO_LARGE;
    }
    mq_launch_walk<true>(dc, dim3((unsigned)gx, (unsigned)gy), st, (int)n, (int)m, d, slice_cols, Dm, items, X,
                         nullptr, nullptr, nullptr, h);
    MDE_LAUNCH_CHECK();
    return MDE_OK;
  }
  mq_launch_walk<false>(dc, dim3((unsigned)row_blocks), st, (int)n, (int)m, d, m, Dm, items, X, row_sums,
                        reinterpret_cast<long long*>(row_count), row_max, nullptr);
  MDE_LAUNCH_CHECK();
  const int64_t chunks = (n + MQ_CHUNK - 1) / MQ_CHUNK;
  double* part = static_cast<double*>(work);
  hipLaunchKernelGGL(k_matrix_chunk_totals, dim3((unsigned)chunks), dim3(MDE_BLOCK), 0, st, n, row_sums,
                     reinterpret_cast<const long long*>(row_count), row_max, part);
  MDE_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_matrix_final_totals, dim3(1), dim3(MDE_BLOCK), 0, st, chunks, part, totals);
  MDE_LAUNCH_CHECK();
  return MDE_OK;
}

extern "C" int mde_matrix_moments(int64_t n, int64_t m, const float* Dm, const int32_t* items, int32_t d,
                                  const float* X, double* row_sums, int64_t* row_count, float* row_max,
                                  double* totals, void* work, void* stream) {
  return mq_run("mde_matrix_moments", n, m, Dm, items, d, X, row_sums, row_count, row_max, totals, nullptr, work,
                stream);
}

extern "C" int mde_matrix_histogram(int64_t n, int64_t m, const float* Dm, const int32_t* items, int32_t d,
                                    const float* X, int32_t bins, float d_lo, float d_hi, float e_lo, float e_hi,
                                    int64_t* counts, void* stream) {
  const mq_hist_args h = {bins, d_lo, d_hi, e_lo, e_hi, counts};
  return mq_run("mde_matrix_histogram", n, m, Dm, items, d, X, nullptr, nullptr, nullptr, nullptr, &h, nullptr,
                stream);
}

// ---------------------------------------------------------------- ranks within the columns
// An entry l = idx[b][c] is ranked when it names a row (0 <= l < n) other than the column's own item.
__device__ __forceinline__ bool mq_ranked(int l, int n, int64_t own) { return l >= 0 && l < n && (int64_t)l != own; }

__global__ __launch_bounds__(MDE_BLOCK) void k_matrix_rank_init(int n, int64_t total, int k,
                                                                const int32_t* __restrict__ items,
                                                                const int32_t* __restrict__ idx,
                                                                int32_t* __restrict__ ranks) {
  for (int64_t i = (int64_t)blockIdx.x * MDE_BLOCK + threadIdx.x; i < total; i += (int64_t)gridDim.x * MDE_BLOCK) {
    const int64_t b = i / k;
    ranks[i] = mq_ranked(idx[i], n, items ? (int64_t)items[b] : b) ? 0 : -1;
  }
}

template <int KC>
__global__ __launch_bounds__(MDE_BLOCK) void k_matrix_rank_count(int n, int m, int k, int64_t slice_rows,
                                                                 const float* __restrict__ Dm,
                                                                 const int32_t* __restrict__ items,
                                                                 const int32_t* __restrict__ idx,
                                                                 int32_t* __restrict__ ranks) {
  __shared__ float sT[KC][64];                                  // [c][lane]: conflict-free
  __shared__ int sJ[KC][64];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t b = (int64_t)blockIdx.x * 64 + lane;
  const bool bok = b < m;
  const int64_t own = bok ? (items ? (int64_t)items[b] : b) : -1;
  // a threshold that names no row is NaN: nothing precedes it
  for (int c = wave; c < k; c += 4) {
    const int l = bok ? idx[b * k + c] : -1;
    const bool ranked = mq_ranked(l, n, own);
    sT[c][lane] = ranked ? Dm[(int64_t)l * m + b] : __builtin_nanf("");
    sJ[c][lane] = ranked ? l : -1;
  }
  __syncthreads();
  int cnt[KC];
#pragma unroll
  for (int c = 0; c < KC; ++c) cnt[c] = 0;
  const int64_t r_lo = (int64_t)blockIdx.y * slice_rows;
  const int64_t r_hi = r_lo + slice_rows < n ? r_lo + slice_rows : n;
  for (int64_t j0 = r_lo + wave * MQ_RR; j0 < r_hi; j0 += 4 * MQ_RR) {
    float v[MQ_RR];
#pragma unroll
    for (int r = 0; r < MQ_RR; ++r) {
      const int64_t j = j0 + r;
      // the column's own item and what does not exist are NaN: they precede nothing
      v[r] = (bok && j < r_hi && j != own) ? Dm[j * (int64_t)m + b] : __builtin_nanf("");
    }
#pragma unroll
    for (int c = 0; c < KC; ++c) {
      if (c < k) {
        const float t = sT[c][lane];
        const int64_t rel = (int64_t)sJ[c][lane] - j0;          // row j0 + r precedes row l on a tie when r < rel
        const int jr = rel > MQ_RR ? MQ_RR : (rel < 0 ? 0 : (int)rel);
        int a = 0;
#pragma unroll
        for (int r = 0; r < MQ_RR; ++r) a += (v[r] < t || (v[r] == t && r < jr)) ? 1 : 0;
        cnt[c] += a;
      }
    }
  }
  if (bok) {
#pragma unroll
    for (int c = 0; c < KC; ++c)
      if (c < k && sJ[c][lane] >= 0 && cnt[c]) atomicAdd(ranks + b * k + c, cnt[c]);
  }
}

extern "C" int mde_matrix_ranks(int64_t n, int64_t m, const float* Dm, const int32_t* items, int32_t k,
                                const int32_t* idx, int32_t* ranks, void* stream) {
  if (!mq_sizes_ok(n, m) || k < 1 || k > MQ_MAX_K || !Dm || !idx || !ranks || (!items && m != n)) {
    mde_set_error("mde_matrix_ranks: invalid arguments (1 <= n < 2^31, 1 <= m < 2^31 and m == n without items, "
                  "1 <= k <= %d, non-null Dm / idx / ranks)", MQ_MAX_K);
    return MDE_E_INVALID;
  }
  hipStream_t st = mde_stream(stream);
  const int64_t total = m * (int64_t)k;
  hipLaunchKernelGGL(k_matrix_rank_init, dim3(mde_grid(total, MDE_BLOCK, 4096)), dim3(MDE_BLOCK), 0, st, (int)n, total,
                     k, items, idx, ranks);
  MDE_LAUNCH_CHECK();
  // about 4096 workgroups: row slices of whole steps (4 waves x MQ_RR rows)
  const int64_t tiles = (m + 63) / 64, step = 4 * MQ_RR;
  int64_t s = (4096 + tiles - 1) / tiles;
  const int64_t steps = (n + step - 1) / step;
  if (s > steps) s = steps;
  if (s > 65535) s = 65535;
  const int64_t slice_rows = ((steps + s - 1) / s) * step;
  const dim3 grid((unsigned)tiles, (unsigned)((n + slice_rows - 1) / slice_rows));
  if (k <= 16)
    hipLaunchKernelGGL(k_matrix_rank_count<16>, grid, dim3(MDE_BLOCK), 0, st, (int)n, (int)m, k, slice_rows, Dm, items,
                       idx, ranks);
  else
    hipLaunchKernelGGL(k_matrix_rank_count<MQ_MAX_K>, grid, dim3(MDE_BLOCK), 0, st, (int)n, (int)m, k, slice_rows, Dm,
                       items, idx, ranks);
  MDE_LAUNCH_CHECK();
  return MDE_OK;
}

// mde_landmarks.hip -- landmark selection on the device: farthest-point (maxmin) and k-means++ (D^2) sampling
// (DESIGN section 6n).  Both are sequential in the landmarks: landmark t is chosen from every row's squared
// distance to its nearest landmark among 0 .. t-1, so each landmark costs one pass over the data.
//
//   state   mind2[r]    float32 squared distance of row r to its nearest landmark so far; -1 once r is a landmark
//           nearest[r]  position in idx_out of that landmark (ties keep the earlier one)
//   step t  k_landmark_update   d2(r, landmark t-1) for every row, lowers mind2 / nearest, marks the landmark,
//                               leaves per-segment partials in `work`
//           k_landmark_select_farthest / _d2   read the partials, write idx_out[t] and radius2_out[t]
//
// Nothing is read back by the host: the whole selection is 2 m + 1 launches on one stream.
//
// Same bits for every grid and on every run.  d2 is the difference form sum_f (x_f - l_f)^2 (0 between equal rows),
// summed in an order that depends on n_features alone: feature f sits in the 4-float chunk c = f / 4, chunk c
// belongs to lane c % G of the G lanes that share the row, a lane adds its features in increasing f with one fma
// each, and the G lanes are folded by an xor butterfly.  The rows are cut into segments of seg_rows(n) rows, a
// function of n alone; a workgroup owns a contiguous run of whole segments (how many is the grid's only freedom),
// and the partials -- the largest (mind2, smallest row), the float64 sum of mind2 over the unselected rows, the
// smallest unselected row -- are per segment, each folded in a fixed order.
#include "mde_common.h"
#include "mde_rng.h"

#define LM_STAGE_CHUNKS 1024                 // float4 chunks of the landmark row that LDS holds at a time (16 KiB)
#define LM_STAGE_FLOATS (4 * LM_STAGE_CHUNKS)
#define LM_MAX_SEGMENTS 4096
#define LM_SEG_QUANTUM 64                    // a segment is a multiple of this many rows
#define LM_NO_ROW 0x7fffffff

// rows per segment: at most LM_MAX_SEGMENTS segments, whole multiples of LM_SEG_QUANTUM rows
static inline int64_t lm_seg_rows(int64_t n) {
  const int64_t per = (n + LM_MAX_SEGMENTS - 1) / LM_MAX_SEGMENTS;
  return (per + LM_SEG_QUANTUM - 1) / LM_SEG_QUANTUM * LM_SEG_QUANTUM;
}
static inline int lm_segments(int64_t n) { return (int)((n + lm_seg_rows(n) - 1) / lm_seg_rows(n)); }

// `work`: double sum[nseg] | float vmax[nseg] | int32 vrow[nseg] | int32 minrow[nseg]
struct LmPartials {
  double* sum;
  float* vmax;
  int32_t* vrow;
  int32_t* minrow;
};
static inline __host__ __device__ LmPartials lm_partials(void* work, int nseg) {
  LmPartials p;
  p.sum = static_cast<double*>(work);
  p.vmax = reinterpret_cast<float*>(p.sum + nseg);
  p.vrow = reinterpret_cast<int32_t*>(p.vmax + nseg);
  p.minrow = p.vrow + nseg;
  return p;
}

__global__ __launch_bounds__(MDE_BLOCK) void k_landmark_init(int n, int start, float* __restrict__ mind2,
                                                             int32_t* __restrict__ nearest, int32_t* idx_out,
                                                             float* radius2_out) {
  for (int64_t r = (int64_t)blockIdx.x * MDE_BLOCK + threadIdx.x; r < n; r += (int64_t)gridDim.x * MDE_BLOCK) {
    mind2[r] = __builtin_inff();
    nearest[r] = 0;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    idx_out[0] = start;
    radius2_out[0] = __builtin_inff();
  }
}

// chunks [k0, k1) of the landmark row -> LDS (VEC: 16-byte loads; otherwise the floats [4 k0, min(4 k1, nf)))
template <bool VEC>
__device__ __forceinline__ void lm_stage(const float* __restrict__ lrow, int nf, int k0, int k1, float* lds) {
  if (VEC) {
    const float4* src = reinterpret_cast<const float4*>(lrow);
    float4* dst = reinterpret_cast<float4*>(lds);
    for (int c = k0 + threadIdx.x; c < k1; c += MDE_BLOCK) dst[c - k0] = src[c];
  } else {
    const int f1 = 4 * k1 < nf ? 4 * k1 : nf;
    for (int f = 4 * k0 + threadIdx.x; f < f1; f += MDE_BLOCK) lds[f - 4 * k0] = lrow[f];
  }
}

// acc[u] += sum of (x_f - l_f)^2 over this lane's chunks c = k0 + g, k0 + g + G, .. < k1 of the row rowp[u], for U
// rows at once.  The chunks are taken J at a time with a trip count that is the same for every lane: all J * U loads
// of a batch are issued before the first is used (a chunk past the end is loaded from the last one and dropped), so
// a wave has one memory latency per batch, not per chunk.  The additions keep the order of increasing c.
template <int G, int U, int J, bool VEC>
__device__ __forceinline__ void lm_accumulate(float (&acc)[U], const float* const (&rowp)[U], int nf, int k0, int k1,
                                              int g, const float* lds) {
  for (int b = k0 + g; b - g < k1; b += J * G) {
    if (VEC) {
      const float4* l4 = reinterpret_cast<const float4*>(lds);
      float4 x[U][J], l[J];
      bool ok[J];
#pragma unroll
      for (int j = 0; j < J; ++j) {
        const int c = b + j * G;
        ok[j] = c < k1;
        const int cc = ok[j] ? c : k1 - 1;
#pragma unroll
        for (int u = 0; u < U; ++u) x[u][j] = reinterpret_cast<const float4*>(rowp[u])[cc];
        l[j] = l4[cc - k0];
      }
#pragma unroll
      for (int j = 0; j < J; ++j) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const float dx = x[u][j].x - l[j].x, dy = x[u][j].y - l[j].y;
          const float dz = x[u][j].z - l[j].z, dw = x[u][j].w - l[j].w;
          float a = acc[u];
          a = __builtin_fmaf(dx, dx, a);
          a = __builtin_fmaf(dy, dy, a);
          a = __builtin_fmaf(dz, dz, a);
          a = __builtin_fmaf(dw, dw, a);
          acc[u] = ok[j] ? a : acc[u];
        }
      }
    } else {
      float x[U][J][4], l[J][4];
      bool ok[J][4];
#pragma unroll
      for (int j = 0; j < J; ++j) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int f = 4 * (b + j * G) + i;
          ok[j][i] = b + j * G < k1 && f < nf;
          const int ff = ok[j][i] ? f : nf - 1;
#pragma unroll
          for (int u = 0; u < U; ++u) x[u][j][i] = rowp[u][ff];
          l[j][i] = lds[ok[j][i] ? ff - 4 * k0 : 0];
        }
      }
#pragma unroll
      for (int j = 0; j < J; ++j) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
#pragma unroll
          for (int u = 0; u < U; ++u) {
            const float d = x[u][j][i] - l[j][i];
            acc[u] = ok[j][i] ? __builtin_fmaf(d, d, acc[u]) : acc[u];
          }
        }
      }
    }
  }
}

// One landmark's pass.  G lanes share a row (a power of two, the smallest that gives every 4-float chunk of a short
// row its own lane); a workgroup takes MDE_BLOCK / G rows at a time, U such groups of rows in flight.
template <int G, int U, bool VEC>
__global__ __launch_bounds__(MDE_BLOCK) void k_landmark_update(int n, int nf, const float* __restrict__ data, int t,
                                                               const int32_t* __restrict__ idx, int seg_rows, int nseg,
                                                               float* __restrict__ mind2,
                                                               int32_t* __restrict__ nearest, void* work) {
  __shared__ __attribute__((aligned(16))) float lds[LM_STAGE_FLOATS];
  __shared__ double s_sum[MDE_BLOCK / MDE_WAVE];
  __shared__ float s_max[MDE_BLOCK / MDE_WAVE];
  __shared__ int s_row[MDE_BLOCK / MDE_WAVE];
  __shared__ int s_min[MDE_BLOCK / MDE_WAVE];
  constexpr int RP = MDE_BLOCK / G;    // rows per pass of the workgroup
  constexpr int J = G == 64 ? 4 : 1;   // chunks of a row a lane has in flight (with G < 64 a lane has one chunk)
  const int grp = threadIdx.x / G, g = threadIdx.x % G;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int lrow = idx[t];
  const float* __restrict__ lptr = data + (int64_t)lrow * nf;
  const int nchunks = (nf + 3) >> 2;
  const bool multi = nchunks > LM_STAGE_CHUNKS;
  const LmPartials part = lm_partials(work, nseg);
  // this workgroup's run of segments
  const int seg_lo = (int)((int64_t)blockIdx.x * nseg / gridDim.x);
  const int seg_hi = (int)((int64_t)(blockIdx.x + 1) * nseg / gridDim.x);
  if (seg_lo >= seg_hi) return;
  if (!multi) {
    lm_stage<VEC>(lptr, nf, 0, nchunks, lds);
    __syncthreads();
  }
  for (int seg = seg_lo; seg < seg_hi; ++seg) {
    const int64_t row_lo = (int64_t)seg * seg_rows;
    const int64_t row_hi = row_lo + seg_rows < n ? row_lo + seg_rows : n;
    double sum = 0.0;
    float bmax = -1.0f;
    int brow = LM_NO_ROW, minrow = LM_NO_ROW;
    for (int64_t r0 = row_lo; r0 < row_hi; r0 += RP * U) {
      float acc[U], old[U];
      const float* rowp[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int64_t r = r0 + u * RP + grp;
        acc[u] = 0.0f;
        rowp[u] = data + (r < row_hi ? r : row_hi - 1) * nf;  // (a row past the end is loaded in bounds and dropped)
        // the row's state is asked for ahead of its features: it is there when the sum is
        old[u] = (g == 0 && r < row_hi) ? mind2[r] : 0.0f;
      }
      if (!multi) {
        lm_accumulate<G, U, J, VEC>(acc, rowp, nf, 0, nchunks, g, lds);
      } else {
        for (int k0 = 0; k0 < nchunks; k0 += LM_STAGE_CHUNKS) {
          const int k1 = k0 + LM_STAGE_CHUNKS < nchunks ? k0 + LM_STAGE_CHUNKS : nchunks;
          __syncthreads();
          lm_stage<VEC>(lptr, nf, k0, k1, lds);
          __syncthreads();
          lm_accumulate<G, U, J, VEC>(acc, rowp, nf, k0, k1, g, lds);
        }
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const float d2 = mde_group_sum<G>(acc[u]);
        const int64_t r = r0 + u * RP + grp;
        if (g == 0 && r < row_hi) {
          float v = old[u];
          if (d2 < v) {
            v = d2;
            mind2[r] = d2;
            nearest[r] = t;
          }
          if (r == lrow) {
            v = -1.0f;
            mind2[r] = -1.0f;
          }
          if (v >= 0.0f) {
            sum += (double)v;
            if (v > bmax || (v == bmax && (int)r < brow)) {
              bmax = v;
              brow = (int)r;
            }
            if ((int)r < minrow) minrow = (int)r;
          }
        }
      }
    }
    // fold the segment: lanes by xor butterflies, then the four waves in order
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      sum += __shfl_xor(sum, o, 64);
      const float om = __shfl_xor(bmax, o, 64);
      const int orow = __shfl_xor(brow, o, 64);
      const int omin = __shfl_xor(minrow, o, 64);
      if (om > bmax || (om == bmax && orow < brow)) {
        bmax = om;
        brow = orow;
      }
      minrow = omin < minrow ? omin : minrow;
    }
    __syncthreads();
    if (lane == 0) {
      s_sum[wave] = sum;
      s_max[wave] = bmax;
      s_row[wave] = brow;
      s_min[wave] = minrow;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      for (int w = 1; w < MDE_BLOCK / MDE_WAVE; ++w) {
        sum += s_sum[w];
        if (s_max[w] > bmax || (s_max[w] == bmax && s_row[w] < brow)) {
          bmax = s_max[w];
          brow = s_row[w];
        }
        minrow = s_min[w] < minrow ? s_min[w] : minrow;
      }
      part.sum[seg] = sum;
      part.vmax[seg] = bmax;
      part.vrow[seg] = brow;
      part.minrow[seg] = minrow;
    }
  }
}

// exclusive prefix of `v` over the 256 threads in thread order (fixed order: an up-sweep inside each wave, the waves
// in sequence); *total receives the sum over all threads.  smem: >= 4 doubles.
__device__ __forceinline__ double lm_block_exclusive(double v, double* smem, double* total) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  double inc = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const double up = __shfl_up(inc, o, 64);
    if (lane >= o) inc += up;
  }
  __syncthreads();
  if (lane == 63) smem[wave] = inc;
  __syncthreads();
  double base = 0.0, all = 0.0;
  for (int w = 0; w < MDE_BLOCK / MDE_WAVE; ++w) {
    if (w == wave) base = all;
    all += smem[w];
  }
  *total = all;
  return base + (inc - v);
}

__device__ __forceinline__ int lm_block_min(int v, int* smem /* >= 4 ints */) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const int w = __shfl_xor(v, o, 64);
    v = w < v ? w : v;
  }
  __syncthreads();
  if ((threadIdx.x & 63) == 0) smem[threadIdx.x >> 6] = v;
  __syncthreads();
  int r = smem[0];
  for (int w = 1; w < MDE_BLOCK / MDE_WAVE; ++w) r = smem[w] < r ? smem[w] : r;
  return r;
}

// farthest point: the largest mind2 among the unselected rows, ties to the smallest row.  One workgroup.
__global__ __launch_bounds__(MDE_BLOCK) void k_landmark_select_farthest(int nseg, int t, const void* work,
                                                                        int32_t* idx_out, float* radius2_out) {
  __shared__ float s_max[MDE_BLOCK / MDE_WAVE];
  __shared__ int s_row[MDE_BLOCK / MDE_WAVE];
  const LmPartials part = lm_partials(const_cast<void*>(work), nseg);
  float bmax = -1.0f;
  int brow = LM_NO_ROW;
  for (int s = threadIdx.x; s < nseg; s += MDE_BLOCK) {
    const float v = part.vmax[s];
    const int r = part.vrow[s];
    if (v > bmax || (v == bmax && r < brow)) {
      bmax = v;
      brow = r;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float om = __shfl_xor(bmax, o, 64);
    const int orow = __shfl_xor(brow, o, 64);
    if (om > bmax || (om == bmax && orow < brow)) {
      bmax = om;
      brow = orow;
    }
  }
  if ((threadIdx.x & 63) == 0) {
    s_max[threadIdx.x >> 6] = bmax;
    s_row[threadIdx.x >> 6] = brow;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < MDE_BLOCK / MDE_WAVE; ++w)
      if (s_max[w] > bmax || (s_max[w] == bmax && s_row[w] < brow)) {
        bmax = s_max[w];
        brow = s_row[w];
      }
    idx_out[t] = brow;
    radius2_out[t] = bmax;
  }
}

// k-means++: the smallest row whose inclusive prefix sum of mind2 (unselected rows, row order, float64) exceeds
// u_t * total.  The prefix at a segment's first row is the fold of the segment sums before it; inside the segment
// the rows are added in order.  One workgroup: first the segment, then the row inside it.
__global__ __launch_bounds__(MDE_BLOCK) void k_landmark_select_d2(int n, int seg_rows, int nseg, int t, uint64_t seed,
                                                                  const void* work,
                                                                  const float* __restrict__ mind2, int32_t* idx_out,
                                                                  float* radius2_out) {
  __shared__ double s_d[MDE_BLOCK / MDE_WAVE];
  __shared__ int s_i[MDE_BLOCK / MDE_WAVE];
  __shared__ double s_base[MDE_BLOCK];
  const LmPartials part = lm_partials(const_cast<void*>(work), nseg);
  const int tid = threadIdx.x;
  // thread i folds the segments [i q, (i + 1) q)
  const int q = (nseg + MDE_BLOCK - 1) / MDE_BLOCK;
  const int s0 = tid * q < nseg ? tid * q : nseg;
  const int s1 = s0 + q < nseg ? s0 + q : nseg;
  double local = 0.0;
  for (int s = s0; s < s1; ++s) local += part.sum[s];
  double total;
  const double before = lm_block_exclusive(local, s_d, &total);
  int choice;
  if (!(total > 0.0)) {
    // every remaining row duplicates a landmark: the smallest unselected row
    int mr = LM_NO_ROW;
    for (int s = tid; s < nseg; s += MDE_BLOCK) mr = part.minrow[s] < mr ? part.minrow[s] : mr;
    choice = lm_block_min(mr, s_i);
  } else {
    const double target = mde_uniform01(seed, (uint64_t)t) * total;
    // the first segment whose inclusive prefix exceeds the target, and the prefix in front of it
    int cand = LM_NO_ROW, lastpos = -1;
    double acc = before;
    s_base[tid] = 0.0;
    for (int s = s0; s < s1; ++s) {
      const double v = part.sum[s];
      const double nxt = acc + v;
      if (cand == LM_NO_ROW && v > 0.0 && nxt > target) {  // (v > 0: the segment holds a row that can be taken)
        cand = s;
        s_base[tid] = acc;
      }
      if (v > 0.0) lastpos = s;
      acc = nxt;
    }
    int seg = lm_block_min(cand, s_i);
    double base;
    if (seg == LM_NO_ROW) {
      // the product rounded up to the total: the last segment that holds a positive row, searched from its own sum
      seg = -lm_block_min(-lastpos, s_i);
      base = target;
    } else {
      base = s_base[seg / q];
    }
    // inside the segment: thread i adds the rows [i c, (i + 1) c) of it
    const int64_t row_lo = (int64_t)seg * seg_rows;
    const int64_t row_hi = row_lo + seg_rows < n ? row_lo + seg_rows : n;
    const int c = (seg_rows + MDE_BLOCK - 1) / MDE_BLOCK;
    const int64_t a = row_lo + (int64_t)tid * c < row_hi ? row_lo + (int64_t)tid * c : row_hi;
    const int64_t b = a + c < row_hi ? a + c : row_hi;
    double mine = 0.0;
    int lastrow = -1;
    for (int64_t r = a; r < b; ++r) {
      const float v = mind2[r];
      if (v > 0.0f) {
        mine += (double)v;
        lastrow = (int)r;
      }
    }
    double seg_total;
    double run = base + lm_block_exclusive(mine, s_d, &seg_total);
    int found = LM_NO_ROW;
    for (int64_t r = a; r < b; ++r) {
      const float v = mind2[r];
      if (v > 0.0f) {
        run += (double)v;
        if (found == LM_NO_ROW && run > target) found = (int)r;
      }
    }
    choice = lm_block_min(found, s_i);
    // (the segment's sum and the in-order prefix differ in the last bits: no row may pass the target; its last
    // positive row then does)
    if (choice == LM_NO_ROW) choice = -lm_block_min(-lastrow, s_i);
  }
  if (tid == 0) {
    idx_out[t] = choice;
    radius2_out[t] = mind2[choice];
  }
}

__global__ __launch_bounds__(MDE_BLOCK) void k_landmark_finish(int m, const int32_t* __restrict__ idx,
                                                               float* __restrict__ mind2) {
  for (int t = blockIdx.x * MDE_BLOCK + threadIdx.x; t < m; t += gridDim.x * MDE_BLOCK) mind2[idx[t]] = 0.0f;
}

template <int G, int U>
static void lm_launch_update(bool vec, int grid, hipStream_t st, int n, int nf, const float* data, int t,
                             const int32_t* idx, int seg_rows, int nseg, float* mind2, int32_t* nearest, void* work) {
  if (vec)
    hipLaunchKernelGGL((k_landmark_update<G, U, true>), dim3(grid), dim3(MDE_BLOCK), 0, st, n, nf, data, t, idx,
                       seg_rows, nseg, mind2, nearest, work);
  else
    hipLaunchKernelGGL((k_landmark_update<G, U, false>), dim3(grid), dim3(MDE_BLOCK), 0, st, n, nf, data, t, idx,
                       seg_rows, nseg, mind2, nearest, work);
}

static bool lm_sizes_ok(int64_t n, int32_t nf, int64_t m) {
  return n >= 1 && nf >= 1 && nf <= (1 << 30) && m >= 1 && m <= n;   // (4 * chunk indices stay inside int32)
}

extern "C" int64_t mde_select_landmarks_work_bytes(int64_t n, int32_t nf, int64_t m) {
  if (!lm_sizes_ok(n, nf, m)) {
    mde_set_error("mde_select_landmarks_work_bytes: invalid arguments (1 <= m <= n, 1 <= nf <= 2^30)");
    return MDE_E_INVALID;
  }
  if (n >= ((int64_t)1 << 31)) {
    mde_set_error("mde_select_landmarks_work_bytes: n = %lld rows; the kernels index rows in int32 (n < 2^31)",
                  (long long)n);
    return MDE_E_TOO_LARGE;
  }
  return (int64_t)lm_segments(n) * (sizeof(double) + sizeof(float) + 2 * sizeof(int32_t)) + 64;
}

extern "C" int mde_select_landmarks(int64_t n, int32_t nf, const float* data, int64_t m, int32_t method,
                                    int64_t start, uint64_t seed, int32_t* idx_out, float* radius2_out,
                                    float* mind2_out, int32_t* nearest_out, void* work, void* stream) {
  if (!lm_sizes_ok(n, nf, m) || start < 0 || start >= n || (method != 0 && method != 1) || !data || !idx_out ||
      !radius2_out || !mind2_out || !nearest_out || !work) {
    mde_set_error("mde_select_landmarks: invalid arguments (1 <= m <= n, 1 <= nf <= 2^30, 0 <= start < n, method 0 "
                  "(farthest point) or 1 (k-means++), non-null data / idx_out / radius2_out / mind2_out / "
                  "nearest_out / work)");
    return MDE_E_INVALID;
  }
  if (n >= ((int64_t)1 << 31)) {
    mde_set_error("mde_select_landmarks: n = %lld rows; the kernels index rows in int32 (n < 2^31)", (long long)n);
    return MDE_E_TOO_LARGE;
  }
  hipStream_t st = mde_stream(stream);
  const int seg_rows = (int)lm_seg_rows(n), nseg = lm_segments(n);
  const bool vec = (nf % 4 == 0) && (reinterpret_cast<uintptr_t>(data) % 16 == 0);
  const int nchunks = (nf + 3) / 4;
  int G = 1;
  while (G < 64 && G < nchunks) G <<= 1;
  // a workgroup streams about 128 KiB or more: the landmark row is staged once per workgroup
  const int64_t seg_bytes = (int64_t)seg_rows * nf * 4;
  int64_t per_block = (128 * 1024 + seg_bytes - 1) / seg_bytes;
  if (per_block < 1) per_block = 1;
  int grid = (int)((nseg + per_block - 1) / per_block);
  const int forced = env_int("MDE_LANDMARK_BLOCKS", 0);  // (tests: the results do not depend on the grid)
  if (forced > 0) grid = forced;
  if (grid > nseg) grid = nseg;
  if (grid < 1) grid = 1;

  hipLaunchKernelGGL(k_landmark_init, dim3(mde_grid(n, MDE_BLOCK)), dim3(MDE_BLOCK), 0, st, (int)n, (int)start,
                     mind2_out, nearest_out, idx_out, radius2_out);
  MDE_LAUNCH_CHECK();
  for (int64_t t = 1; t <= m; ++t) {
    // the pass of landmark t - 1
    const int tl = (int)(t - 1);
    switch (G) {
#define LM_CASE(GG, UU)                                                                                           \
  case GG:                                                                                                        \
    lm_launch_update<GG, UU>(vec, grid, st, (int)n, nf, data, tl, idx_out, seg_rows, nseg, mind2_out, nearest_out, \
                             work);                                                                               \
    break;
      LM_CASE(1, 1)
      LM_CASE(2, 1)
      LM_CASE(4, 1)
      LM_CASE(8, 2)
      LM_CASE(16, 4)
      LM_CASE(32, 4)
      LM_CASE(64, 2)
#undef LM_CASE
    }
    MDE_LAUNCH_CHECK();
    if (t == m) break;
    if (method == 0)
      hipLaunchKernelGGL(k_landmark_select_farthest, dim3(1), dim3(MDE_BLOCK), 0, st, nseg, (int)t, work, idx_out,
                         radius2_out);
    else
      hipLaunchKernelGGL(k_landmark_select_d2, dim3(1), dim3(MDE_BLOCK), 0, st, (int)n, seg_rows, nseg, (int)t, seed,
                         work, mind2_out, idx_out, radius2_out);
    MDE_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(k_landmark_finish, dim3(mde_grid(m, MDE_BLOCK)), dim3(MDE_BLOCK), 0, st, (int)m, idx_out,
                     mind2_out);
  MDE_LAUNCH_CHECK();
  return MDE_OK;
}

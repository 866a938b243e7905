// mde_graph_sssp.hip -- shortest-path lengths from a chosen list of source nodes to every node.
//   [ref: pymde/preprocess/graph.py:286-474 solves from EVERY node; the reference has no "from these m nodes"]
// The output is node-major, out[v][b] = length from sources[b] to v, which is the [n_new, n_old] distance matrix the
// landmark placement reads.  In that layout one wave owns one node u and 64 consecutive source columns (a "tile"):
// a neighbour v of u contributes out[v][64 g .. 64 g + 63] -- one contiguous 256-byte load -- and the neighbour's
// index and the edge length are the same for all 64 lanes.  The sweep is the pull-style Bellman-Ford relaxation of
// mde_graph.hip, in place:
//      out[u][b] = min(out[u][b], min_{v ~ u} out[v][b] + w_uv)
// Every stored value is the float32 left-to-right sum along a real walk from the source and only ever decreases; a
// wave that reads a neighbour's tile while another wave lowers it sees the old or the new value of each float, both
// lengths of real walks, so no atomics are needed and the fixed point (the minimum over walks of that sum: float32
// addition of non-negative numbers is monotone) does not depend on the schedule.
//
// Work skipping: a tile can only improve through a neighbour's tile that changed in the sweep before.  Per node and
// per 64 tiles (4096 columns) one 64-bit word holds "tile g changed in this sweep"; two such arrays alternate between
// sweeps (written in sweep t, read in sweep t + 1, so a kernel boundary lies between the write and the read).  A wave
// takes (node u, word wi): it gathers the words of u's neighbours (one 8-byte load per neighbour for all 64 tiles),
// and for tile g loads only the neighbours whose bit g is set.  A node nobody near changed costs its adjacency and
// those words, no distance.  Nodes of degree above SS_HEAVY go to a second launch where a team of SS_TEAM waves splits
// the neighbour list and reduces the 64 minima through LDS.
#include <vector>

#include "mde_common.h"
#include "mde_plan.h"

#define SS_HEAVY 128                 // largest degree the one-wave kernel takes
#define SS_TEAM 16                   // waves of a team of the heavy kernel
#define SS_CHECK 4                   // sweeps between two read-backs of the "changed" word

typedef unsigned long long ss_word;

// a word every lane holds the same value of, moved to scalar registers
__device__ __forceinline__ ss_word ss_uniform(ss_word x) {
  const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)x);
  const unsigned hi = __builtin_amdgcn_readfirstlane((unsigned)(x >> 32));
  return ((ss_word)hi << 32) | lo;
}

__device__ __forceinline__ ss_word ss_wave_or(ss_word x) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) x |= __shfl_xor(x, o, 64);
  return ss_uniform(x);
}

__global__ __launch_bounds__(MDE_BLOCK) void k_ss_init(int64_t n, int64_t m, const int64_t* __restrict__ sources,
                                                       float* __restrict__ out) {
  for (int64_t i = (int64_t)blockIdx.x * MDE_BLOCK + threadIdx.x; i < n * m; i += (int64_t)gridDim.x * MDE_BLOCK) {
    const int64_t v = i / m, b = i - v * m;
    out[i] = (sources[b] == v) ? 0.0f : INFINITY;
  }
}

// the tiles that hold a source "changed" in the sweep before the first (several sources may share a word)
__global__ __launch_bounds__(MDE_BLOCK) void k_ss_seed(int64_t n, int64_t m, const int64_t* __restrict__ sources,
                                                       ss_word* __restrict__ flags) {
  const int64_t b = (int64_t)blockIdx.x * MDE_BLOCK + threadIdx.x;
  if (b >= m) return;
  const int64_t g = b >> 6;
  atomicOr(flags + (g >> 6) * n + sources[b], 1ull << (g & 63));
}

__global__ __launch_bounds__(MDE_BLOCK) void k_ss_heavy_list(int64_t n, const int32_t* __restrict__ rowptr,
                                                             int32_t* __restrict__ heavy, int* __restrict__ count) {
  const int64_t u = (int64_t)blockIdx.x * MDE_BLOCK + threadIdx.x;
  if (u < n && rowptr[u + 1] - rowptr[u] > SS_HEAVY) heavy[atomicAdd(count, 1)] = (int32_t)u;
}

// best = min(best, out[v_j][col] + w_j) over the lanes j of `mask` (the neighbour lane j holds); four loads in flight
__device__ __forceinline__ float ss_pull(ss_word mask, int v, float wl, const float* out, int64_t m, int64_t col,
                                         bool active, float best) {
  while (mask) {
    float d[4], ww[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      d[r] = INFINITY;
      ww[r] = 0.0f;
      if (mask) {
        const int j = __ffsll((long long)mask) - 1;
        mask &= mask - 1;
        const int64_t vj = __builtin_amdgcn_readlane(v, j);
        ww[r] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(wl), j));
        if (active) d[r] = out[vj * m + col];
      }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float cand = d[r] + ww[r];
      best = cand < best ? cand : best;
    }
  }
  return best;
}

// One sweep.  NW = 1: every wave of the grid takes items (node u, word wi) with degree(u) <= SS_HEAVY.  NW = SS_TEAM:
// a workgroup of NW waves takes one item (heavy[.], wi) at a time.  prev / cur: [n_words][n] tile bits.
template <int NW>
__global__ __launch_bounds__(NW == 1 ? MDE_BLOCK : NW * 64) void k_ss_relax(
    int64_t n, int64_t m, int n_words, const int32_t* __restrict__ rowptr, const int32_t* __restrict__ nbr,
    const float* __restrict__ w, float max_length, const int32_t* __restrict__ heavy, int64_t n_heavy, float* out,
    const ss_word* __restrict__ prev, ss_word* __restrict__ cur, int* __restrict__ changed,
    unsigned long long* __restrict__ relaxed) {
  __shared__ float s_best[NW == 1 ? 1 : NW][64];
  __shared__ ss_word s_need[NW == 1 ? 1 : NW];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t n_groups = (m + 63) >> 6;
  int64_t item, n_items, stride;
  if (NW == 1) {
    item = ((int64_t)blockIdx.x * MDE_BLOCK + threadIdx.x) >> 6;
    stride = ((int64_t)gridDim.x * MDE_BLOCK) >> 6;
    n_items = n * n_words;
  } else {
    item = blockIdx.x;
    stride = gridDim.x;
    n_items = n_heavy * n_words;
  }
  unsigned long long done = 0;
  for (; item < n_items; item += stride) {
    const int64_t rows = NW == 1 ? n : n_heavy;
    const int wi = (int)(item / rows);
    const int64_t u = NW == 1 ? item - (int64_t)wi * rows : (int64_t)heavy[item - (int64_t)wi * rows];
    const int h0 = rowptr[u], h1 = rowptr[u + 1];
    if (NW == 1 && h1 - h0 > SS_HEAVY) continue;  // the heavy launch owns this node's tiles and bits
    const ss_word* pw = prev + (int64_t)wi * n;
    // this wave's first chunk of neighbours stays in registers; further chunks are read again per tile
    const int hf = h0 + 64 * (NW == 1 ? 0 : wave);
    int v0 = 0;
    float w0 = 1.0f;
    ss_word f0 = 0;
    if (hf + lane < h1) {
      v0 = nbr[hf + lane];
      if (w) w0 = w[hf + lane];
      f0 = pw[v0];
    }
    ss_word need = f0;
    for (int hb = hf + 64 * NW; hb < h1; hb += 64 * NW)
      if (hb + lane < h1) need |= pw[nbr[hb + lane]];
    need = ss_wave_or(need);
    if (NW > 1) {
      __syncthreads();  // (the previous item's s_best / s_need have been read)
      if (lane == 0) s_need[wave] = need;
      __syncthreads();
      need = 0;
#pragma unroll
      for (int q = 0; q < NW; ++q) need |= s_need[q];
      need = ss_uniform(need);
    }
    ss_word now = 0;
    for (ss_word todo = need; todo; todo &= todo - 1) {
      const int g = __ffsll((long long)todo) - 1;
      const int64_t col = (((int64_t)wi << 6) + g) * 64 + lane;
      if ((((int64_t)wi << 6) + g) >= n_groups) break;  // (never set: bits past the last tile stay zero)
      const bool active = col < m;
      float best = ss_pull(__ballot((f0 >> g) & 1ull), v0, w0, out, m, col, active, INFINITY);
      for (int hb = hf + 64 * NW; hb < h1; hb += 64 * NW) {
        int v = 0;
        float wl = 1.0f;
        ss_word f = 0;
        if (hb + lane < h1) {
          v = nbr[hb + lane];
          if (w) wl = w[hb + lane];
          f = pw[v];
        }
        best = ss_pull(__ballot((f >> g) & 1ull), v, wl, out, m, col, active, best);
      }
      if (NW > 1) {
        __syncthreads();
        s_best[wave][lane] = best;
        __syncthreads();
        if (wave == 0) {
#pragma unroll
          for (int q = 1; q < NW; ++q) best = s_best[q][lane] < best ? s_best[q][lane] : best;
        }
      }
      if (wave == 0 || NW == 1) {
        bool lower = false;
        if (active) {
          float* at = out + u * m + col;
          lower = best < *at && best <= max_length;
          if (lower) *at = best;
        }
        if (__any(lower)) now |= 1ull << g;
        ++done;
      }
    }
    if ((wave == 0 || NW == 1) && lane == 0) {
      cur[(int64_t)wi * n + u] = now;
      if (now) *changed = 1;
    }
  }
  if ((wave == 0 || NW == 1) && lane == 0 && done) atomicAdd(relaxed, done);
}

static thread_local int64_t g_ss_stats[4] = {0, 0, 0, 0};

// What the last mde_graph_distances_from call of this thread did: stats[0] sweeps launched, [1] tiles (node, 64
// columns) it relaxed, [2] tiles per sweep (n * ceil(m / 64)), [3] nodes of degree above the one-wave limit.
extern "C" int mde_graph_distances_stats(int64_t* stats) {
  if (!stats) return MDE_E_INVALID;
  for (int q = 0; q < 4; ++q) stats[q] = g_ss_stats[q];
  return MDE_OK;
}

// out[v * m + b] = shortest-path length from sources[b] to v (0 at the source, +inf where no path of length <=
// max_length exists).  plan, w, max_length as for mde_graph_shortest_paths; sources: m node indices in any order,
// repeats allowed (device or host memory).  SYNC.
extern "C" int mde_graph_distances_from(const mde_plan* plan, const float* w, float max_length, int64_t m,
                                        const int64_t* sources, float* out, void* stream) {
  if (!plan || !sources || !out) {
    mde_set_error("mde_graph_distances_from: plan, sources and out must not be NULL");
    return MDE_E_INVALID;
  }
  if (plan->row_lo != 0 || plan->row_hi != plan->n) {
    mde_set_error("mde_graph_distances_from needs a full (unsharded) plan");
    return MDE_E_INVALID;
  }
  if (m < 1) {
    mde_set_error("mde_graph_distances_from needs at least one source, got m = %lld", (long long)m);
    return MDE_E_INVALID;
  }
  hipStream_t st = mde_stream(stream);
  const int64_t n = plan->n;
  if (n < 1 || n >= ((int64_t)1 << 31)) return MDE_E_TOO_LARGE;
  // the sources are checked on the host before anything is launched (a copy, no kernel)
  std::vector<int64_t> host((size_t)m);
  MDE_HIP(hipMemcpyAsync(host.data(), sources, (size_t)m * sizeof(int64_t), hipMemcpyDefault, st));
  MDE_HIP(hipStreamSynchronize(st));
  for (int64_t b = 0; b < m; ++b)
    if (host[b] < 0 || host[b] >= n) {
      mde_set_error("mde_graph_distances_from: sources[%lld] = %lld lies outside [0, n) = [0, %lld)", (long long)b,
                    (long long)host[b], (long long)n);
      return MDE_E_INVALID;
    }
  if (!(max_length > 0.0f)) max_length = INFINITY;
  const int64_t n_groups = (m + 63) >> 6;
  const int n_words = (int)((n_groups + 63) >> 6);
  const size_t words = (size_t)n * n_words;
  MdeDeviceBuf<int64_t> dev_sources;
  MdeDeviceBuf<ss_word> flags;
  MdeDeviceBuf<int32_t> heavy;
  MdeDeviceBuf<unsigned long long> counters;  // [0] tiles relaxed | [1] heavy count (int) | [2..] changed[SS_CHECK] (int)
  MDE_HIP(dev_sources.alloc((size_t)m * sizeof(int64_t)));
  MDE_HIP(flags.alloc(2 * words * sizeof(ss_word)));
  MDE_HIP(heavy.alloc((size_t)n * sizeof(int32_t)));
  MDE_HIP(counters.alloc((2 + SS_CHECK) * sizeof(unsigned long long)));
  MDE_HIP(hipMemcpyAsync(dev_sources.get(), host.data(), (size_t)m * sizeof(int64_t), hipMemcpyHostToDevice, st));
  MDE_HIP(hipMemsetAsync(flags.get(), 0, 2 * words * sizeof(ss_word), st));
  MDE_HIP(hipMemsetAsync(counters.get(), 0, (2 + SS_CHECK) * sizeof(unsigned long long), st));
  unsigned long long* relaxed = counters.get();
  int* heavy_count = reinterpret_cast<int*>(counters.get() + 1);
  int* changed = reinterpret_cast<int*>(counters.get() + 2);  // one word per sweep between two read-backs
  hipLaunchKernelGGL(k_ss_init, dim3(mde_grid(n * m, MDE_BLOCK, 16384)), dim3(MDE_BLOCK), 0, st, n, m,
                     dev_sources.get(), out);
  MDE_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_ss_seed, dim3((unsigned)((m + MDE_BLOCK - 1) / MDE_BLOCK)), dim3(MDE_BLOCK), 0, st, n, m,
                     dev_sources.get(), flags.get());
  MDE_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_ss_heavy_list, dim3((unsigned)((n + MDE_BLOCK - 1) / MDE_BLOCK)), dim3(MDE_BLOCK), 0, st, n,
                     plan->rowptr, heavy.get(), heavy_count);
  MDE_LAUNCH_CHECK();
  int n_heavy = 0;
  MDE_HIP(hipMemcpyAsync(&n_heavy, heavy_count, sizeof(int), hipMemcpyDeviceToHost, st));
  MDE_HIP(hipStreamSynchronize(st));
  const int grid_light = mde_grid((int64_t)words * 64, MDE_BLOCK, 32768);
  const int grid_heavy = mde_grid((int64_t)n_heavy * n_words, 1, 4096);
  ss_word *prev = flags.get(), *cur = flags.get() + words;
  int64_t sweeps = 0;
  bool converged = false;
  // a walk of fewest edges among the shortest has at most n - 1 of them: sweep n - 1 is the last that can change a
  // value, and one more shows that nothing did (a sweep that changes nothing is the fixed point)
  while (!converged && sweeps < n) {
    MDE_HIP(hipMemsetAsync(changed, 0, SS_CHECK * sizeof(int), st));
    int s = 0;
    for (; s < SS_CHECK && sweeps < n; ++s, ++sweeps) {
      hipLaunchKernelGGL(k_ss_relax<1>, dim3(grid_light), dim3(MDE_BLOCK), 0, st, n, m, n_words, plan->rowptr,
                         plan->nbr, w, max_length, (const int32_t*)nullptr, (int64_t)0, out, prev, cur,
                         changed + s, relaxed);
      MDE_LAUNCH_CHECK();
      if (n_heavy > 0) {
        hipLaunchKernelGGL(k_ss_relax<SS_TEAM>, dim3(grid_heavy), dim3(SS_TEAM * 64), 0, st, n, m, n_words,
                           plan->rowptr, plan->nbr, w, max_length, heavy.get(), (int64_t)n_heavy, out, prev, cur,
                           changed + s, relaxed);
        MDE_LAUNCH_CHECK();
      }
      ss_word* t = prev;
      prev = cur;
      cur = t;
    }
    int h[SS_CHECK];
    MDE_HIP(hipMemcpyAsync(h, changed, SS_CHECK * sizeof(int), hipMemcpyDeviceToHost, st));
    MDE_HIP(hipStreamSynchronize(st));
    converged = h[s - 1] == 0;
  }
  unsigned long long tiles = 0;
  MDE_HIP(hipMemcpyAsync(&tiles, relaxed, sizeof(tiles), hipMemcpyDeviceToHost, st));
  MDE_HIP(hipStreamSynchronize(st));
  g_ss_stats[0] = sweeps;
  g_ss_stats[1] = (int64_t)tiles;
  g_ss_stats[2] = n * n_groups;
  g_ss_stats[3] = n_heavy;
  if (!converged) {
    mde_set_error("mde_graph_distances_from: still changing after %lld sweeps over %lld nodes (negative or NaN "
                  "edge lengths?)", (long long)sweeps, (long long)n);
    return MDE_E_INVALID;
  }
  return MDE_OK;
}

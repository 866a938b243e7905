// mde_affinity.hip -- edge weights from the distances of directed neighbour lists:
//   mde_knn_calibrate   per-row calibration of a kernel over a row's kept entries: the Gaussian bandwidth of
//                       t-SNE's perplexity (kind 0) or UMAP's smooth k-NN distances (kind 1);
//   mde_knn_symmetrize  the undirected edges of those lists -- the edge set and order of mde_knn_pairs +
//                       mde_edges_count_unique -- with the two directions' conditionals combined.
// A row has at most KNN_MAXK = 64 entries, so a row is one aligned group of G lanes (G = the next power of two
// at or above k): one entry per lane, every sum a xor butterfly over the group, one exp per lane per bisection
// step.  All row arithmetic is double, the order of every sum is fixed by G alone, and a row reads nothing but
// its own entries: the same bits on every run and for every grid.
#include <hipcub/hipcub.hpp>

#include <cmath>

#include "mde_common.h"
#include "mde_knn_tile.h"   // KNN_MAXK

// The library is built with -ffp-contract=fast, which fuses d * d - m into one fma whatever a contract pragma
// says; the fused value is not zero at the minimum (m is the ROUNDED product), and the entries tied at the
// minimum would no longer be found.  A value that passes through here is rounded before anything uses it.
__device__ __forceinline__ double aff_rounded(double v) {
  asm volatile("" : "+v"(v));
  return v;
}

#define AFF_MAX_STEPS 400                    // doubling + bisection steps of a root search
#define AFF_BRACKET 3.552713678800501e-15    // 2^-48: the bracket ends below this share of its upper end

template <int G>
__device__ __forceinline__ double aff_group_min(double v) {
#pragma unroll
  for (int o = G / 2; o > 0; o >>= 1) {
    const double w = __shfl_xor(v, o, 64);
    v = w < v ? w : v;
  }
  return v;
}
template <int G>
__device__ __forceinline__ int aff_group_count(bool b) {
  return mde_group_sum<G, int>(b ? 1 : 0);
}

// Root of an increasing (UMAP: sum exp(-g / x) in x) or decreasing (perplexity: the entropy in beta) function
// of one variable over a group: `above(x)` is true where the root lies above x.  Doubling from x0 until the
// root is bracketed, then bisection; every lane of the group holds the same x, lo and hi throughout, and the
// loop runs until every group of the wave is done (finished groups and groups without a search idle with
// their state frozen), so the butterflies inside `above` always see all 64 lanes.
template <typename Above>
__device__ __forceinline__ double aff_root(bool search, double x0, Above above) {
  double lo = 0.0, hi = INFINITY, x = x0;
  bool done = !search;
  for (int it = 0; it < AFF_MAX_STEPS; ++it) {
    if (__all(done)) break;
    const bool up = above(x);
    if (!done) {
      if (up) {
        lo = x;
        x = std::isinf(hi) ? 2.0 * x : 0.5 * (lo + hi);
      } else {
        hi = x;
        x = 0.5 * (lo + hi);
      }
      if (!std::isinf(hi) && hi - lo <= AFF_BRACKET * hi) done = true;
    }
  }
  return 0.5 * (lo + hi);
}

template <int G>
__global__ __launch_bounds__(MDE_BLOCK) void k_knn_calibrate(int64_t n, int k, const int32_t* __restrict__ idx,
                                                             const float* __restrict__ val, int root, double scale,
                                                             int has_max, float max_value, int kind,
                                                             double perplexity, int32_t* __restrict__ idx_out,
                                                             float* __restrict__ p_out, float* __restrict__ bandwidth,
                                                             float* __restrict__ offset) {
  constexpr int ROWS = MDE_BLOCK / G;           // rows of a workgroup per pass
  const int slot = threadIdx.x % G, sub = threadIdx.x / G;
  const int64_t passes = (n + ROWS - 1) / ROWS;
  for (int64_t pass = blockIdx.x; pass < passes; pass += gridDim.x) {   // (uniform over the workgroup)
    const int64_t row = pass * ROWS + sub;
    const bool in_row = row < n && slot < k;
    const int64_t at = row * k + slot;
    int32_t j = -1;
    double d = 0.0;
    if (in_row) {
      j = idx[at];
      const float v = val[at];
      if (j < 0 || j >= n || j == row || (has_max && !(v <= max_value))) j = -1;
      const double vd = (double)v;
      d = scale * (root ? sqrt(vd > 0.0 ? vd : 0.0) : vd);
    }
    const bool kept = j >= 0;
    if (!kept) d = 0.0;
    const int ki = aff_group_count<G>(kept);
    double p = 0.0, bw = 0.0, off = 0.0;
    if (kind == 0) {
      // s_j = d_j^2 - min d_j^2, p_j = exp(-beta s_j) / Z, H(beta) = log Z + beta sum_j p_j s_j = log(perplexity)
      const double q = aff_rounded(d * d);
      const double qmin = aff_group_min<G>(kept ? q : INFINITY);
      off = aff_group_min<G>(kept ? d : INFINITY);
      const double s = kept ? q - qmin : 0.0;
      const int c = aff_group_count<G>(kept && s == 0.0);
      const bool uniform = ki > 0 && (perplexity >= (double)ki || c == ki);
      const bool tied = ki > 0 && !uniform && perplexity <= (double)c;
      const bool search = ki > 0 && !uniform && !tied;
      const double target = log(perplexity);
      const double s_sum = mde_group_sum<G, double>(s);
      const double x0 = search ? (double)(ki - c) / s_sum : 1.0;      // 1 / mean of the positive s_j
      auto entropy_above = [&](double beta) {
        const double e = kept ? exp(-beta * s) : 0.0;
        const double z = mde_group_sum<G, double>(e);
        const double es = mde_group_sum<G, double>(e * s);
        return log(z) + beta * (es / z) > target;
      };
      const double beta = aff_root(search, x0, entropy_above);
      if (search) {
        const double e = kept ? exp(-beta * s) : 0.0;
        p = e / mde_group_sum<G, double>(e);
        bw = beta;
      } else if (uniform) {
        p = kept ? 1.0 / (double)ki : 0.0;
      } else if (tied) {
        p = (kept && s == 0.0) ? 1.0 / (double)c : 0.0;
        bw = INFINITY;
      }
      if (ki == 0) off = 0.0;
    } else {
      // rho = the smallest positive d_j, g_j = max(d_j - rho, 0), p_j = exp(-g_j / sigma), sum_j p_j = log2(k_i)
      const double rmin = aff_group_min<G>(kept && d > 0.0 ? d : INFINITY);
      const double rho = std::isinf(rmin) ? 0.0 : rmin;
      const double g = kept ? (d - rho > 0.0 ? d - rho : 0.0) : 0.0;
      const double floor_ = ki > 0 ? 1e-3 * (mde_group_sum<G, double>(d) / (double)ki) : 0.0;
      const int c = aff_group_count<G>(kept && g == 0.0);
      const double target = ki > 0 ? log2((double)ki) : 0.0;
      const bool search = c < 6 && ki > (1 << c);   // log2(k_i) > c, in integers (k_i <= 64); implies c < k_i
      const double g_sum = mde_group_sum<G, double>(g);
      const double x0 = search ? g_sum / (double)(ki - c) : 1.0;      // mean of the positive g_j
      auto sum_below = [&](double sigma) {
        const double e = kept ? (g == 0.0 ? 1.0 : exp(-g / sigma)) : 0.0;
        return mde_group_sum<G, double>(e) < target;
      };
      double sigma = aff_root(search, x0, sum_below);
      if (!search) sigma = 0.0;                 // c == k_i, or the limit sigma -> 0
      sigma = sigma > floor_ ? sigma : floor_;
      if (kept) p = (c == ki) ? 1.0 : (g == 0.0 ? 1.0 : (sigma == 0.0 ? 0.0 : exp(-g / sigma)));
      bw = sigma;
      off = rho;
    }
    if (in_row) {
      idx_out[at] = j;
      p_out[at] = kept ? (float)p : 0.0f;
    }
    if (row < n && slot == 0) {
      bandwidth[row] = (float)bw;
      offset[row] = (float)off;
    }
  }
}

template <int G>
static void launch_calibrate(int64_t n, int k, const int32_t* idx, const float* val, int root, double scale,
                             int has_max, float max_value, int kind, double perplexity, int32_t* idx_out,
                             float* p_out, float* bandwidth, float* offset, hipStream_t st) {
  const int64_t passes = (n + MDE_BLOCK / G - 1) / (MDE_BLOCK / G);
  hipLaunchKernelGGL(k_knn_calibrate<G>, dim3(mde_grid(passes, 1, 8192)), dim3(MDE_BLOCK), 0, st, n, k, idx, val,
                     root, scale, has_max, max_value, kind, perplexity, idx_out, p_out, bandwidth, offset);
}

static int affinity_sizes_ok(const char* who, int64_t n, int32_t k) {
  if (n < 1 || k < 1 || k > KNN_MAXK) {
    mde_set_error("%s: invalid arguments (n >= 1, 1 <= k <= %d)", who, KNN_MAXK);
    return MDE_E_INVALID;
  }
  if (n >= ((int64_t)1 << 31) || n * (int64_t)k >= ((int64_t)1 << 31) - 1) {
    mde_set_error("%s supports n k < 2^31 - 1 list entries", who);
    return MDE_E_TOO_LARGE;
  }
  return MDE_OK;
}

extern "C" int mde_knn_calibrate(int64_t n, int32_t k, const int32_t* idx, const float* val, int32_t root,
                                 double scale, int32_t has_max, float max_value, int32_t kind, double perplexity,
                                 int32_t* idx_out, float* p_out, float* bandwidth_out, float* offset_out,
                                 void* stream) {
  int rc = affinity_sizes_ok("mde_knn_calibrate", n, k);
  if (rc != MDE_OK) return rc;
  if (!idx || !val || !idx_out || !p_out || !bandwidth_out || !offset_out || !(scale > 0.0) || std::isinf(scale) ||
      (kind != 0 && kind != 1) || (kind == 0 && !(perplexity > 0.0)) || (has_max && max_value != max_value)) {
    mde_set_error("mde_knn_calibrate: invalid arguments (kind 0 with perplexity > 0, or kind 1; scale > 0)");
    return MDE_E_INVALID;
  }
  hipStream_t st = mde_stream(stream);
#define AFF_LAUNCH(G)                                                                                          \
  launch_calibrate<G>(n, k, idx, val, root != 0, scale, has_max != 0, max_value, kind, perplexity, idx_out, p_out, \
                      bandwidth_out, offset_out, st)
  if (k <= 1) AFF_LAUNCH(1);
  else if (k <= 2) AFF_LAUNCH(2);
  else if (k <= 4) AFF_LAUNCH(4);
  else if (k <= 8) AFF_LAUNCH(8);
  else if (k <= 16) AFF_LAUNCH(16);
  else if (k <= 32) AFF_LAUNCH(32);
  else AFF_LAUNCH(64);
#undef AFF_LAUNCH
  MDE_LAUNCH_CHECK();
  return MDE_OK;
}

// ---------------------------------------------------------------- symmetrisation
// Entry (i, c) with j = idx[i][c] >= 0 looks i up in row j's list and emits the edge {i, j} when i < j or when
// j does not list i: every undirected edge once.  key = min * n + max, a = the conditional of the smaller
// row's entry (0 when it has none), b the larger row's.  A wave reserves its output slots with one atomic;
// the radix sort by key that follows fixes the order, and keys are distinct, so the result does not depend on
// which wave arrived first.
__global__ __launch_bounds__(MDE_BLOCK) void k_knn_symmetrize(int64_t n, int k, int64_t total,
                                                              const int32_t* __restrict__ idx,
                                                              const float* __restrict__ p, int rule,
                                                              uint64_t* __restrict__ keys, float* __restrict__ w,
                                                              unsigned int* __restrict__ count) {
  const int lane = threadIdx.x & 63;
  for (int64_t base = (int64_t)blockIdx.x * MDE_BLOCK; base < total; base += (int64_t)gridDim.x * MDE_BLOCK) {
    const int64_t t = base + threadIdx.x;
    bool emit = false;
    uint64_t key = 0;
    float wt = 0.0f;
    if (t < total) {
      const int64_t i = t / k;
      const int64_t j = idx[t];
      if (j >= 0 && j < n && j != i) {
        const int32_t* row = idx + j * k;
        int found = -1;
        for (int c = 0; c < k; ++c)
          if (row[c] == (int32_t)i) found = c;
        emit = i < j || found < 0;
        if (emit) {
          const float mine = p[t], theirs = found >= 0 ? p[j * k + found] : 0.0f;
          const float a = i < j ? mine : theirs, b = i < j ? theirs : mine;
          const uint64_t lo = (uint64_t)(i < j ? i : j), hi = (uint64_t)(i < j ? j : i);
          key = lo * (uint64_t)n + hi;
          wt = rule == 0 ? 0.5f * (a + b) : (float)((double)a + (double)b - (double)a * (double)b);
        }
      }
    }
    const unsigned long long mask = __ballot(emit);
    if (mask) {
      unsigned int first = 0;
      if (lane == 0) first = atomicAdd(count, (unsigned int)__popcll(mask));
      first = __shfl(first, 0, 64);
      if (emit) {
        const unsigned int at = first + (unsigned int)__popcll(mask & ((1ull << lane) - 1ull));
        keys[at] = key;
        w[at] = wt;
      }
    }
  }
}

__global__ __launch_bounds__(MDE_BLOCK) void k_affinity_edges(int64_t n, int64_t m, const uint64_t* __restrict__ keys,
                                                              int64_t* __restrict__ edges) {
  for (int64_t e = (int64_t)blockIdx.x * MDE_BLOCK + threadIdx.x; e < m; e += (int64_t)gridDim.x * MDE_BLOCK) {
    const uint64_t key = keys[e];
    reinterpret_cast<longlong2*>(edges)[e] = make_longlong2((long long)(key / (uint64_t)n),
                                                             (long long)(key % (uint64_t)n));
  }
}

extern "C" int mde_knn_symmetrize(int64_t n, int32_t k, const int32_t* idx, const float* p, int32_t rule,
                                  int64_t* edges_out, float* weights_out, int64_t* count_host, void* stream) {
  int rc = affinity_sizes_ok("mde_knn_symmetrize", n, k);
  if (rc != MDE_OK) return rc;
  if (!idx || !p || !edges_out || !weights_out || !count_host || (rule != 0 && rule != 1)) {
    mde_set_error("mde_knn_symmetrize: invalid arguments (rule 0 = mean or 1 = union)");
    return MDE_E_INVALID;
  }
  hipStream_t st = mde_stream(stream);
  *count_host = 0;
  const int64_t total = n * (int64_t)k;
  MdeDeviceBuf<uint64_t> keys, sorted;
  MdeDeviceBuf<float> w;
  MdeDeviceBuf<unsigned int> count;
  MdeDeviceBuf<char> tmp;
  MDE_HIP(keys.alloc(total * sizeof(uint64_t)));
  MDE_HIP(w.alloc(total * sizeof(float)));
  MDE_HIP(count.alloc(sizeof(unsigned int)));
  MDE_HIP(hipMemsetAsync(count.get(), 0, sizeof(unsigned int), st));
  hipLaunchKernelGGL(k_knn_symmetrize, dim3(mde_grid(total, MDE_BLOCK, 4096)), dim3(MDE_BLOCK), 0, st, n, k, total,
                     idx, p, rule, keys.get(), w.get(), count.get());
  MDE_LAUNCH_CHECK();
  unsigned int m32 = 0;
  MDE_HIP(hipMemcpyAsync(&m32, count.get(), sizeof(unsigned int), hipMemcpyDeviceToHost, st));
  MDE_HIP(hipStreamSynchronize(st));
  const int64_t m = (int64_t)m32;
  if (m == 0) return MDE_OK;
  if (m > total) return MDE_E_INVALID;   // (cannot happen: every entry emits at most once)
  MDE_HIP(sorted.alloc(m * sizeof(uint64_t)));
  int end_bit = 1;
  while (end_bit < 64 && (((uint64_t)n * (uint64_t)n) >> end_bit)) ++end_bit;
  size_t tb = 0;
  MDE_HIP(hipcub::DeviceRadixSort::SortPairs(nullptr, tb, keys.get(), sorted.get(), w.get(), weights_out, (int)m, 0,
                                             end_bit, st));
  MDE_HIP(tmp.alloc(tb ? tb : 16));
  MDE_HIP(hipcub::DeviceRadixSort::SortPairs(tmp.get(), tb, keys.get(), sorted.get(), w.get(), weights_out, (int)m, 0,
                                             end_bit, st));
  hipLaunchKernelGGL(k_affinity_edges, dim3(mde_grid(m, MDE_BLOCK, 4096)), dim3(MDE_BLOCK), 0, st, n, m, sorted.get(),
                     edges_out);
  MDE_LAUNCH_CHECK();
  MDE_HIP(hipStreamSynchronize(st));
  *count_host = m;
  return MDE_OK;
}

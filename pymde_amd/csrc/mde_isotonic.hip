// mde_isotonic.hip -- weighted isotonic regression: the nondecreasing `out` that minimises
// sum_i w_i (y_i - out_i)^2.  The fit is the left slope of the greatest convex minorant of the cumulative-sum
// diagram P_i = (W_i, S_i), i = 0 .. p, with W_i = sum_{k<i} w_k and S_i = sum_{k<i} w_k (y_k - ybar): a lower
// convex hull of p + 1 points that are already sorted in x.  It is built as a merge tree, so that no loop depends
// on the data for its length (pool-adjacent-violators is one sequential chain):
//
//   prefix    k_iso_scan<false> (per-workgroup sums of w and w y) -> k_iso_mean (ybar) -> k_iso_scan<false> (sums of
//             w and w (y - ybar)) -> k_iso_scan_parts -> k_iso_scan<true> (W, S; `out` filled with -inf);
//   leaves    k_iso_leaf: one workgroup per ISO_LEAF points staged in LDS; a thread runs Graham's scan over its
//             ISO_K consecutive points, then log2(MDE_BLOCK) levels merge neighbouring lists inside LDS;
//   tree      per level k_iso_tangent (one wave per pair of neighbouring nodes) and k_iso_copy (the merged list,
//             contiguous, into the other hull buffer); an odd node is carried up;
//   expand    k_iso_values writes a block's mean at its first element, and a running maximum over `out`
//             (k_iso_max<false> -> k_iso_max_parts -> k_iso_max<true>) carries it to the block's other elements.
//
// A merge of two x-separated convex chains A (left) and B (right) keeps a prefix A[0 .. la] and a suffix
// B[rb ..]: the ends of their lower common tangent.  With t(l) the point of B that the slope from A[l] is
// smallest at -- a binary search, the slope falls and then rises along a convex chain -- A[l] stays a vertex
// exactly when slope(A[l-1], A[l]) < slope(A[l], B[t(l)]), which holds for a prefix of A: la is the last such l
// (a binary search in LDS, a 64-way search over the lanes of a wave in the tree) and rb = t(la).  Comparisons
// are cross products of double differences.  Where rounding makes a comparison inconsistent the searches still
// end on valid indices and the chain is convex up to that rounding; the running maximum then makes `out`
// nondecreasing exactly, moving nothing by more than the rounding that caused it.
//
// Every sum is a double in an order fixed by p alone, there is no atomic, no grid barrier and no flag between
// workgroups: the same bits on every run.  Every loop runs at most ISO_LEAF or 32 times.
#include <cmath>

#include "mde_common.h"

#define ISO_LEAF 1024                       // points of a leaf
#define ISO_K (ISO_LEAF / MDE_BLOCK)        // points a thread scans by itself
#define ISO_ITEMS 8                         // scans: consecutive elements of a thread per tile
#define ISO_TILE (MDE_BLOCK * ISO_ITEMS)
#define ISO_MAX_PARTS 4096                  // workgroups of a scan (a workgroup walks <= 256 tiles at p = 2^31)
#define ISO_COPY 4                          // k_iso_copy / k_iso_values: positions per thread
#define ISO_ALIGN 256

static_assert(ISO_K * MDE_BLOCK == ISO_LEAF && ISO_LEAF <= 65536, "leaf-relative indices are uint16_t");
static_assert(MDE_BLOCK == 256, "four waves per workgroup");

// ---------------------------------------------------------------- work buffer
struct IsoLayout {
  int64_t n_points, n_leaves, n_parts, per_wg;
  int64_t mean, part, offs, fpart, foffs, W, S, hull[2], cnt[2], meta, bytes;
};

static inline int64_t iso_up(int64_t b) { return (b + ISO_ALIGN - 1) / ISO_ALIGN * ISO_ALIGN; }

static IsoLayout iso_layout(int64_t p) {
  IsoLayout L;
  L.n_points = p + 1;
  L.n_leaves = (L.n_points + ISO_LEAF - 1) / ISO_LEAF;
  const int64_t tiles = (p + ISO_TILE - 1) / ISO_TILE;
  const int64_t tiles_per_wg = (tiles + ISO_MAX_PARTS - 1) / ISO_MAX_PARTS;
  L.per_wg = (tiles_per_wg < 1 ? 1 : tiles_per_wg) * ISO_TILE;
  L.n_parts = p > 0 ? (p + L.per_wg - 1) / L.per_wg : 1;
  int64_t at = 0;
  L.mean = at, at += ISO_ALIGN;
  L.part = at, at += iso_up(2 * ISO_MAX_PARTS * sizeof(double));
  L.offs = at, at += iso_up(2 * ISO_MAX_PARTS * sizeof(double));
  L.fpart = at, at += iso_up(ISO_MAX_PARTS * sizeof(float));
  L.foffs = at, at += iso_up(ISO_MAX_PARTS * sizeof(float));
  L.W = at, at += iso_up(L.n_points * sizeof(double));
  L.S = at, at += iso_up(L.n_points * sizeof(double));
  for (int b = 0; b < 2; ++b) L.hull[b] = at, at += iso_up(L.n_points * sizeof(int32_t));
  for (int b = 0; b < 2; ++b) L.cnt[b] = at, at += iso_up(L.n_leaves * sizeof(int32_t));
  L.meta = at, at += iso_up((L.n_leaves + 1) / 2 * sizeof(int2));
  L.bytes = at;
  return L;
}

// ---------------------------------------------------------------- workgroup scans (256 threads, fixed order)
__device__ __forceinline__ double iso_block_excl_sum(double v, double* smem /* 4 */, double* total) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  double inc = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const double u = __shfl_up(inc, o, 64);
    if (lane >= o) inc += u;
  }
  double exc = __shfl_up(inc, 1, 64);
  if (lane == 0) exc = 0.0;
  __syncthreads();
  if (lane == 63) smem[wave] = inc;
  __syncthreads();
  double base = 0.0, tot = 0.0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    if (i < wave) base += smem[i];
    tot += smem[i];
  }
  *total = tot;
  return base + exc;
}

__device__ __forceinline__ float iso_block_excl_max(float v, float* smem /* 4 */, float* total) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  float inc = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const float u = __shfl_up(inc, o, 64);
    if (lane >= o) inc = fmaxf(inc, u);
  }
  float exc = __shfl_up(inc, 1, 64);
  if (lane == 0) exc = -INFINITY;
  __syncthreads();
  if (lane == 63) smem[wave] = inc;
  __syncthreads();
  float base = -INFINITY, tot = -INFINITY;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    if (i < wave) base = fmaxf(base, smem[i]);
    tot = fmaxf(tot, smem[i]);
  }
  *total = tot;
  return fmaxf(base, exc);
}

// ---------------------------------------------------------------- prefix sums
// Workgroup b walks the elements [b per_wg, (b + 1) per_wg) tile by tile.  WRITE = false: its sums of w and
// w (y - *mean) (mean == NULL: of w y) go to part[b] and part[n_parts + b].  WRITE = true: W[i + 1] and S[i + 1],
// from the exclusive scan of those sums in `offs`, and out[i] = -inf for the running maximum of the expansion.
template <bool WRITE>
__global__ __launch_bounds__(MDE_BLOCK) void k_iso_scan(int64_t p, int64_t per_wg, int n_parts,
                                                        const float* __restrict__ y, const float* __restrict__ w,
                                                        const double* __restrict__ mean, double* __restrict__ part,
                                                        const double* __restrict__ offs, double* __restrict__ W,
                                                        double* __restrict__ S, float* __restrict__ out) {
  __shared__ double sm[8];
  const int64_t lo = (int64_t)blockIdx.x * per_wg;
  const int64_t hi = lo + per_wg < p ? lo + per_wg : p;
  const double m = mean ? *mean : 0.0;
  double carry_w = WRITE ? offs[blockIdx.x] : 0.0, carry_s = WRITE ? offs[n_parts + blockIdx.x] : 0.0;
  for (int64_t t = lo; t < hi; t += ISO_TILE) {
    const int64_t i0 = t + (int64_t)threadIdx.x * ISO_ITEMS;
    double lw[ISO_ITEMS], ls[ISO_ITEMS], tw = 0.0, ts = 0.0;
#pragma unroll
    for (int k = 0; k < ISO_ITEMS; ++k) {
      const int64_t i = i0 + k;
      if (i < hi) {
        const double wi = w ? (double)w[i] : 1.0;
        tw += wi;
        ts += wi * ((double)y[i] - m);
      }
      lw[k] = tw;
      ls[k] = ts;
    }
    double tot_w, tot_s;
    const double ew = iso_block_excl_sum(tw, sm, &tot_w);
    const double es = iso_block_excl_sum(ts, sm + 4, &tot_s);
    if (WRITE) {
#pragma unroll
      for (int k = 0; k < ISO_ITEMS; ++k) {
        const int64_t i = i0 + k;
        if (i < hi) {
          W[i + 1] = carry_w + (ew + lw[k]);
          S[i + 1] = carry_s + (es + ls[k]);
          out[i] = -INFINITY;
        }
      }
    }
    carry_w += tot_w;
    carry_s += tot_s;
  }
  if (!WRITE && threadIdx.x == 0) {
    part[blockIdx.x] = carry_w;
    part[n_parts + blockIdx.x] = carry_s;
  }
  if (WRITE && blockIdx.x == 0 && threadIdx.x == 0) W[0] = 0.0, S[0] = 0.0;
}

// one workgroup: ybar = sum w y / sum w from the n_parts <= ISO_MAX_PARTS partial sums
__global__ __launch_bounds__(MDE_BLOCK) void k_iso_mean(int n_parts, const double* __restrict__ part,
                                                        double* __restrict__ mean) {
  __shared__ double sm[8];
  const int chunk = (n_parts + MDE_BLOCK - 1) / MDE_BLOCK;
  double sw = 0.0, ss = 0.0;
  for (int k = 0; k < chunk; ++k) {
    const int b = threadIdx.x * chunk + k;
    if (b < n_parts) sw += part[b], ss += part[n_parts + b];
  }
  double tot_w, tot_s;
  iso_block_excl_sum(sw, sm, &tot_w);
  iso_block_excl_sum(ss, sm + 4, &tot_s);
  if (threadIdx.x == 0) *mean = tot_s / tot_w;
}

// one workgroup: offs = exclusive scan of both rows of part
__global__ __launch_bounds__(MDE_BLOCK) void k_iso_scan_parts(int n_parts, const double* __restrict__ part,
                                                              double* __restrict__ offs) {
  __shared__ double sm[8];
  const int chunk = (n_parts + MDE_BLOCK - 1) / MDE_BLOCK;
  double sw = 0.0, ss = 0.0;
  for (int k = 0; k < chunk; ++k) {
    const int b = threadIdx.x * chunk + k;
    if (b < n_parts) sw += part[b], ss += part[n_parts + b];
  }
  double tot;
  double ew = iso_block_excl_sum(sw, sm, &tot), es = iso_block_excl_sum(ss, sm + 4, &tot);
  for (int k = 0; k < chunk; ++k) {
    const int b = threadIdx.x * chunk + k;
    if (b < n_parts) {
      offs[b] = ew, offs[n_parts + b] = es;
      ew += part[b], es += part[n_parts + b];
    }
  }
}

// ---------------------------------------------------------------- the tangent of two chains
struct IsoPoints {       // the diagram: global memory, or a leaf's copy in LDS
  const double* W;
  const double* S;
};
template <typename I>
struct IsoList {         // a chain: indices into the diagram
  const I* h;
  __device__ __forceinline__ int operator()(int k) const { return (int)h[k]; }
};

// t(a): the first j at which the slope from the point a = (wa, sa), left of B, no longer falls towards B[j + 1]
template <typename I>
__device__ __forceinline__ int iso_tangent(const IsoPoints& pt, double wa, double sa, const IsoList<I>& B, int nb) {
  int lo = 0, hi = nb - 1;
  for (int it = 0; it < 32 && lo < hi; ++it) {
    const int mid = lo + ((hi - lo) >> 1);
    const int j0 = B(mid), j1 = B(mid + 1);
    const double w0 = pt.W[j0], s0 = pt.S[j0], w1 = pt.W[j1], s1 = pt.S[j1];
    if ((s1 - s0) * (w0 - wa) <= (s0 - sa) * (w1 - w0)) lo = mid + 1;   // slope(B[j], B[j+1]) <= slope(a, B[j])
    else hi = mid;
  }
  return lo;
}

// A[l], l >= 1, stays a vertex beside B: slope(A[l-1], A[l]) < slope(A[l], B[t(A[l])])
template <typename I>
__device__ __forceinline__ bool iso_keeps(const IsoPoints& pt, const IsoList<I>& A, int l, const IsoList<I>& B,
                                          int nb) {
  const int a0 = A(l - 1), a1 = A(l);
  const double w0 = pt.W[a0], s0 = pt.S[a0], w1 = pt.W[a1], s1 = pt.S[a1];
  const int bt = B(iso_tangent(pt, w1, s1, B, nb));
  const double wt = pt.W[bt], st = pt.S[bt];
  return (s1 - s0) * (wt - w1) < (st - s1) * (w1 - w0);
}

template <typename I>
__device__ __forceinline__ int iso_tangent_from(const IsoPoints& pt, const IsoList<I>& A, int l,
                                                const IsoList<I>& B, int nb) {
  const int a = A(l);
  return iso_tangent(pt, pt.W[a], pt.S[a], B, nb);
}

// ---------------------------------------------------------------- leaves
__global__ __launch_bounds__(MDE_BLOCK) void k_iso_leaf(int64_t n_points, const double* __restrict__ W,
                                                        const double* __restrict__ S, int32_t* __restrict__ hull,
                                                        int32_t* __restrict__ cnt_out) {
  __shared__ double lW[ISO_LEAF], lS[ISO_LEAF];
  __shared__ uint16_t idx[2][ISO_LEAF];
  __shared__ int cnt[2][MDE_BLOCK];
  __shared__ int2 meta[MDE_BLOCK / 2];
  const int t = threadIdx.x;
  const int64_t base = (int64_t)blockIdx.x * ISO_LEAF;
  const int npts = (int)(n_points - base < ISO_LEAF ? n_points - base : ISO_LEAF);
  for (int q = t; q < ISO_LEAF; q += MDE_BLOCK) {
    const bool in = q < npts;
    lW[q] = in ? W[base + q] : 0.0;
    lS[q] = in ? S[base + q] : 0.0;
  }
  __syncthreads();
  const IsoPoints pt{lW, lS};
  // Graham's scan over the thread's own points; its slots of idx[0] are the stack
  {
    uint16_t* st = idx[0] + t * ISO_K;
    int n = 0;
#pragma unroll
    for (int k = 0; k < ISO_K; ++k) {
      const int c = t * ISO_K + k;
      if (c < npts) {
#pragma unroll
        for (int pop = 0; pop < ISO_K; ++pop) {
          if (n < 2) break;
          const int a = st[n - 2], b = st[n - 1];
          if ((lS[b] - lS[a]) * (lW[c] - lW[b]) < (lS[c] - lS[b]) * (lW[b] - lW[a])) break;
          --n;
        }
        st[n++] = (uint16_t)c;
      }
    }
    cnt[0][t] = n;
  }
  __syncthreads();
  int cur = 0;
  for (int span = ISO_K; span < ISO_LEAF; span <<= 1) {      // a node of this level owns `span` slots
    const int merges = ISO_LEAF / (2 * span);
    if (t < merges) {
      const int ca = cnt[cur][2 * t], cb = cnt[cur][2 * t + 1];
      const IsoList<uint16_t> A{idx[cur] + 2 * t * span}, B{idx[cur] + (2 * t + 1) * span};
      int la = ca - 1, rb = 0;
      if (cb > 0) {
        int lo = 0, hi = ca - 1;
        for (int it = 0; it < 32 && lo < hi; ++it) {
          const int mid = lo + ((hi - lo + 1) >> 1);
          if (iso_keeps(pt, A, mid, B, cb)) lo = mid;
          else hi = mid - 1;
        }
        la = lo;
        rb = iso_tangent_from(pt, A, la, B, cb);
      }
      meta[t] = make_int2(la, rb);
      cnt[cur ^ 1][t] = la + 1 + cb - rb;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < ISO_K; ++k) {
      const int pos = t * ISO_K + k;
      const int node = pos / (2 * span), r = pos - node * 2 * span;
      if (r < cnt[cur ^ 1][node]) {
        const int2 m = meta[node];
        idx[cur ^ 1][pos] = r <= m.x ? idx[cur][pos] : idx[cur][node * 2 * span + span + m.y + (r - m.x - 1)];
      }
    }
    __syncthreads();
    cur ^= 1;
  }
  const int n = cnt[cur][0];
  for (int q = t; q < n; q += MDE_BLOCK) hull[base + q] = (int32_t)(base + idx[cur][q]);
  if (t == 0) cnt_out[blockIdx.x] = n;
}

// ---------------------------------------------------------------- a level of the tree
// One wave per output node j: the chains of the input nodes 2 j and 2 j + 1 lie at hull + (2 j) span and
// hull + (2 j + 1) span.  The 64 lanes test 64 evenly spaced candidates for la per step; an interval of n
// candidates shrinks below n / 64, so six steps serve any chain shorter than 2^31.
__global__ __launch_bounds__(MDE_BLOCK) void k_iso_tangent(int64_t nodes_in, int64_t span,
                                                           const int32_t* __restrict__ hull,
                                                           const int32_t* __restrict__ cnt_in,
                                                           int32_t* __restrict__ cnt_out, int2* __restrict__ meta,
                                                           const double* __restrict__ W,
                                                           const double* __restrict__ S) {
  const int lane = threadIdx.x & 63;
  const int64_t j = (int64_t)blockIdx.x * (MDE_BLOCK / 64) + (threadIdx.x >> 6);
  if (j >= (nodes_in + 1) / 2) return;                       // (uniform over the wave)
  const int ca = cnt_in[2 * j], cb = 2 * j + 1 < nodes_in ? cnt_in[2 * j + 1] : 0;
  const IsoPoints pt{W, S};
  const IsoList<int32_t> A{hull + 2 * j * span}, B{hull + (2 * j + 1) * span};
  int la = ca - 1, rb = 0;
  if (cb > 0) {
    int64_t lo = 0, hi = ca - 1;
    for (int it = 0; it < 6 && lo < hi; ++it) {
      const int64_t step = (hi - lo + 63) >> 6;
      const int64_t c = lo + (lane + 1) * step;
      bool ok = false;
      if (c <= hi) ok = iso_keeps(pt, A, (int)c, B, cb);
      const unsigned long long miss = ~__ballot(ok);
      const int m = miss ? __ffsll((long long)miss) - 1 : 64;   // candidates kept before the first that is not
      const int64_t top = lo + (m + 1) * step - 1;
      lo += m * step;
      hi = top < hi ? top : hi;
    }
    la = (int)lo;
    rb = iso_tangent_from(pt, A, la, B, cb);
  }
  if (lane == 0) {
    meta[j] = make_int2(la, rb);
    cnt_out[j] = la + 1 + cb - rb;
  }
}

// position o of the output buffer belongs to node o >> shift (2 span = 1 << shift slots): A[0 .. la], B[rb ..]
__global__ __launch_bounds__(MDE_BLOCK) void k_iso_copy(int64_t n_points, int shift, int64_t span,
                                                        const int32_t* __restrict__ in, int32_t* __restrict__ out,
                                                        const int2* __restrict__ meta,
                                                        const int32_t* __restrict__ cnt_out) {
#pragma unroll
  for (int k = 0; k < ISO_COPY; ++k) {
    const int64_t o = ((int64_t)blockIdx.x * ISO_COPY + k) * MDE_BLOCK + threadIdx.x;
    if (o >= n_points) continue;
    const int64_t j = o >> shift, r = o - (j << shift);
    if (r >= cnt_out[j]) continue;
    const int2 m = meta[j];
    out[o] = r <= m.x ? in[o] : in[(j << shift) + span + m.y + (r - m.x - 1)];
  }
}

// ---------------------------------------------------------------- expansion
// block k of the fit: the elements [H[k], H[k + 1]); its value goes to its first element
__global__ __launch_bounds__(MDE_BLOCK) void k_iso_values(int64_t n_points, const int32_t* __restrict__ H,
                                                          const int32_t* __restrict__ count,
                                                          const double* __restrict__ W, const double* __restrict__ S,
                                                          const double* __restrict__ mean, float* __restrict__ out) {
  const int64_t blocks = (int64_t)count[0] - 1;
  const double m = *mean;
#pragma unroll
  for (int k = 0; k < ISO_COPY; ++k) {
    const int64_t b = ((int64_t)blockIdx.x * ISO_COPY + k) * MDE_BLOCK + threadIdx.x;
    if (b >= blocks || b + 1 >= n_points) continue;
    const int64_t s = H[b], e = H[b + 1];
    out[s] = (float)(m + (S[e] - S[s]) / (W[e] - W[s]));
  }
}

// running maximum over out, in place: the layout of k_iso_scan
template <bool WRITE>
__global__ __launch_bounds__(MDE_BLOCK) void k_iso_max(int64_t p, int64_t per_wg, float* __restrict__ out,
                                                       float* __restrict__ part, const float* __restrict__ offs) {
  __shared__ float sm[4];
  const int64_t lo = (int64_t)blockIdx.x * per_wg;
  const int64_t hi = lo + per_wg < p ? lo + per_wg : p;
  float carry = WRITE ? offs[blockIdx.x] : -INFINITY;
  for (int64_t t = lo; t < hi; t += ISO_TILE) {
    const int64_t i0 = t + (int64_t)threadIdx.x * ISO_ITEMS;
    float lm[ISO_ITEMS], tm = -INFINITY;
#pragma unroll
    for (int k = 0; k < ISO_ITEMS; ++k) {
      const int64_t i = i0 + k;
      if (i < hi) tm = fmaxf(tm, out[i]);
      lm[k] = tm;
    }
    float tot;
    const float em = fmaxf(carry, iso_block_excl_max(tm, sm, &tot));
    if (WRITE) {
#pragma unroll
      for (int k = 0; k < ISO_ITEMS; ++k) {
        const int64_t i = i0 + k;
        if (i < hi) out[i] = fmaxf(em, lm[k]);
      }
    }
    carry = fmaxf(carry, tot);
  }
  if (!WRITE && threadIdx.x == 0) part[blockIdx.x] = carry;
}

__global__ __launch_bounds__(MDE_BLOCK) void k_iso_max_parts(int n_parts, const float* __restrict__ part,
                                                             float* __restrict__ offs) {
  __shared__ float sm[4];
  const int chunk = (n_parts + MDE_BLOCK - 1) / MDE_BLOCK;
  float tm = -INFINITY;
  for (int k = 0; k < chunk; ++k) {
    const int b = threadIdx.x * chunk + k;
    if (b < n_parts) tm = fmaxf(tm, part[b]);
  }
  float tot;
  float em = iso_block_excl_max(tm, sm, &tot);
  for (int k = 0; k < chunk; ++k) {
    const int b = threadIdx.x * chunk + k;
    if (b < n_parts) {
      offs[b] = em;
      em = fmaxf(em, part[b]);
    }
  }
}

// ---------------------------------------------------------------- C ABI
static int iso_size_ok(const char* who, int64_t p) {
  if (p < 0) {
    mde_set_error("%s: invalid arguments (p >= 0)", who);
    return MDE_E_INVALID;
  }
  if (p > ((int64_t)1 << 31) - 2) {
    mde_set_error("%s supports p <= 2^31 - 2 values", who);
    return MDE_E_TOO_LARGE;
  }
  return MDE_OK;
}

extern "C" int32_t mde_isotonic_leaf(void) { return ISO_LEAF; }

extern "C" int64_t mde_isotonic_work_bytes(int64_t p) {
  const int rc = iso_size_ok("mde_isotonic_work_bytes", p);
  if (rc != MDE_OK) return rc;
  return iso_layout(p).bytes;
}

extern "C" int mde_isotonic(int64_t p, const float* y, const float* w, float* out, void* work, void* stream) {
  const int rc = iso_size_ok("mde_isotonic", p);
  if (rc != MDE_OK) return rc;
  if (p == 0) return MDE_OK;
  if (!y || !out || !work) {
    mde_set_error("mde_isotonic: y, out and work must not be NULL");
    return MDE_E_INVALID;
  }
  hipStream_t st = mde_stream(stream);
  const IsoLayout L = iso_layout(p);
  char* base = static_cast<char*>(work);
  double* mean = reinterpret_cast<double*>(base + L.mean);
  double* part = reinterpret_cast<double*>(base + L.part);
  double* offs = reinterpret_cast<double*>(base + L.offs);
  float* fpart = reinterpret_cast<float*>(base + L.fpart);
  float* foffs = reinterpret_cast<float*>(base + L.foffs);
  double* W = reinterpret_cast<double*>(base + L.W);
  double* S = reinterpret_cast<double*>(base + L.S);
  int32_t* hull[2] = {reinterpret_cast<int32_t*>(base + L.hull[0]), reinterpret_cast<int32_t*>(base + L.hull[1])};
  int32_t* cnt[2] = {reinterpret_cast<int32_t*>(base + L.cnt[0]), reinterpret_cast<int32_t*>(base + L.cnt[1])};
  int2* meta = reinterpret_cast<int2*>(base + L.meta);
  const int np = (int)L.n_parts;
  const dim3 blk(MDE_BLOCK), one(1), parts(np);

  hipLaunchKernelGGL(k_iso_scan<false>, parts, blk, 0, st, p, L.per_wg, np, y, w, (const double*)nullptr, part,
                     (const double*)nullptr, (double*)nullptr, (double*)nullptr, (float*)nullptr);
  hipLaunchKernelGGL(k_iso_mean, one, blk, 0, st, np, part, mean);
  hipLaunchKernelGGL(k_iso_scan<false>, parts, blk, 0, st, p, L.per_wg, np, y, w, (const double*)mean, part,
                     (const double*)nullptr, (double*)nullptr, (double*)nullptr, (float*)nullptr);
  hipLaunchKernelGGL(k_iso_scan_parts, one, blk, 0, st, np, part, offs);
  hipLaunchKernelGGL(k_iso_scan<true>, parts, blk, 0, st, p, L.per_wg, np, y, w, (const double*)mean, part,
                     (const double*)offs, W, S, out);
  MDE_LAUNCH_CHECK();

  hipLaunchKernelGGL(k_iso_leaf, dim3((unsigned)L.n_leaves), blk, 0, st, L.n_points, W, S, hull[0], cnt[0]);
  MDE_LAUNCH_CHECK();
  int cur = 0, shift = 0;
  while ((1 << shift) < ISO_LEAF) ++shift;
  const unsigned copy_grid = (unsigned)((L.n_points + ISO_COPY * MDE_BLOCK - 1) / (ISO_COPY * MDE_BLOCK));
  for (int64_t nodes = L.n_leaves, span = ISO_LEAF; nodes > 1; nodes = (nodes + 1) / 2, span <<= 1) {
    ++shift;                                                   // 2 span = 1 << shift
    const int64_t nodes_out = (nodes + 1) / 2;
    hipLaunchKernelGGL(k_iso_tangent, dim3((unsigned)((nodes_out + 3) / 4)), blk, 0, st, nodes, span, hull[cur],
                       cnt[cur], cnt[cur ^ 1], meta, W, S);
    hipLaunchKernelGGL(k_iso_copy, dim3(copy_grid), blk, 0, st, L.n_points, shift, span, hull[cur], hull[cur ^ 1],
                       meta, cnt[cur ^ 1]);
    MDE_LAUNCH_CHECK();
    cur ^= 1;
  }

  hipLaunchKernelGGL(k_iso_values, dim3(copy_grid), blk, 0, st, L.n_points, hull[cur], cnt[cur], W, S, mean, out);
  hipLaunchKernelGGL(k_iso_max<false>, parts, blk, 0, st, p, L.per_wg, out, fpart, (const float*)nullptr);
  hipLaunchKernelGGL(k_iso_max_parts, one, blk, 0, st, np, fpart, foffs);
  hipLaunchKernelGGL(k_iso_max<true>, parts, blk, 0, st, p, L.per_wg, out, fpart, (const float*)foffs);
  MDE_LAUNCH_CHECK();
  return MDE_OK;
}

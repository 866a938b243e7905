// mde_group_nearest.hip -- the nearest pair of rows between every two groups of a data matrix.
//   [ref: sklearn.manifold.Isomap joins the components of its neighbour graph by their nearest pairs, found on the
//    host one pair of components at a time; the reference has no such step]
// The 64x64 Gram tile of mde_knn_tile.h under a walk that the labels cut.  The rows are ordered by label (a stable
// radix sort of (label, row): inside a group the rows ascend) and read through that row map by the tile's staging
// pointers, as k_ann_scan reads its maps -- no gathered copy.  The sorted positions are cut into blocks of at most
// 64 that never straddle a label boundary, so a block carries one label, on the query and on the candidate side.
// Workgroup (x, y) owns query block x (label A) and walks the candidate blocks of slice y whose label is above A:
// blocks are in label order, so those are the blocks from the first block of group A + 1 on, and the same-group
// tiles and the symmetric half are never formed.  A computed tile holds one pair of labels (A, B): it is reduced to
// its minimum under the key (d2, query position, candidate position) -- positions ascend with the rows inside a
// group, so this is the key (d2, a, b) -- and merged into the block's best for label B, one LDS slot per label.
// The block writes its slots to work[slice][block][label]; k_group_fold takes the minimum over the blocks of A and
// the slices in a fixed order and under the same key.  A squared distance is the float32 value of mde_knn_cross
// (the feature-ordered MFMA chain, fmaxf(qn + cn - 2 acc, 0), norms from k_row_sqnorm) and does not depend on the
// slice that formed it; minima under a total order do not depend on the order they are taken in.  No atomics.
#include <vector>

#include "mde_knn_tile.h"
#include "mde_knn_slices.h"
#include "mde_plan.h"

#define GN_MAX_GROUPS 1024
#define GN_EXTRA (3 * GN_MAX_GROUPS + 2 * KNN_BM + 16)   // best d2 / query pos / candidate pos per label, two norm rows, four wave minima

static int gn_bits_for(uint32_t maxval) {
  int b = 1;
  while (b < 32 && (maxval >> b)) ++b;
  return b;
}

// keys[i] = labels[i] where that is a group, `groups` (a bucket nothing reads) otherwise; vals[i] = i
__global__ __launch_bounds__(MDE_BLOCK) void k_group_keys(int n, int groups, const int32_t* __restrict__ labels,
                                                          uint32_t* __restrict__ keys, uint32_t* __restrict__ vals) {
  const int i = blockIdx.x * MDE_BLOCK + threadIdx.x;
  if (i >= n) return;
  const int g = labels[i];
  keys[i] = (g >= 0 && g < groups) ? (uint32_t)g : (uint32_t)groups;
  vals[i] = (uint32_t)i;
}

// goff[g] = first sorted position whose key is >= g, g = 0 .. groups + 1 (goff[groups + 1] = n)
__global__ __launch_bounds__(MDE_BLOCK) void k_group_offsets(int n, int groups, const uint32_t* __restrict__ keys,
                                                             int32_t* __restrict__ goff) {
  const int i = blockIdx.x * MDE_BLOCK + threadIdx.x;
  if (i > n) return;
  const int lo = i == 0 ? 0 : (int)keys[i - 1] + 1;
  const int hi = i == n ? groups + 1 : (int)keys[i];
  for (int g = lo; g <= hi; ++g) goff[g] = i;
}

struct gn_best {
  float d;
  int a, b;   // positions (kernel) or rows (fold): the order is the same inside a pair of groups
};
__device__ __forceinline__ bool gn_less(float d, int a, int b, const gn_best& o) {
  return d < o.d || (d == o.d && (a < o.a || (a == o.a && b < o.b)));
}

// blk: [3][nb] label | first position | rows of each block; gfirst: [groups + 1] first block of each group.
// part_*: [slices][nb][groups].
__global__ __launch_bounds__(MDE_BLOCK) void k_group_nearest(int nf, int groups, int nb, int per_slice,
                                                             const float* __restrict__ X,
                                                             const float* __restrict__ sqn,
                                                             const int32_t* __restrict__ map,
                                                             const int32_t* __restrict__ blk,
                                                             const int32_t* __restrict__ gfirst,
                                                             float* __restrict__ part_d, int32_t* __restrict__ part_a,
                                                             int32_t* __restrict__ part_b) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const knn_tile_lds s = knn_tile_carve(lds, 0, GN_EXTRA);
  float* bd = s.extra;                                         // [GN_MAX_GROUPS]
  int* ba = reinterpret_cast<int*>(bd + GN_MAX_GROUPS);        // [GN_MAX_GROUPS]
  int* bb = ba + GN_MAX_GROUPS;                                // [GN_MAX_GROUPS]
  float* sQn = reinterpret_cast<float*>(bb + GN_MAX_GROUPS);   // [KNN_BM]
  float* sCn = sQn + KNN_BM;                                   // [KNN_BN]
  float* wd = sCn + KNN_BN;                                    // [4] the waves' minima of a tile
  int* wr = reinterpret_cast<int*>(wd + 4);                    // [4]
  int* wc = wr + 4;                                            // [4]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int qb = blockIdx.x;
  const int A = blk[qb], a0 = blk[nb + qb], na = blk[2 * nb + qb];
  for (int g = tid; g < groups; g += MDE_BLOCK) {
    bd[g] = 3.402823466e+38f;
    ba[g] = -1;
    bb[g] = -1;
  }
  if (tid < KNN_BM) sQn[tid] = sqn[map[a0 + (tid < na ? tid : 0)]];
  const float* arow[KNN_STG];
  bool aok[KNN_STG];
#pragma unroll
  for (int q = 0; q < KNN_STG; ++q) {
    const int r = (tid >> 5) + 8 * q;
    aok[q] = r < na;
    arow[q] = X + (int64_t)map[a0 + (aok[q] ? r : 0)] * nf;
  }
  // the slice's candidate blocks, cut to those of a larger label (blocks are in label order)
  const int64_t lo = (int64_t)blockIdx.y * per_slice;
  int cb_lo = gfirst[A + 1], cb_hi = lo + per_slice < nb ? (int)(lo + per_slice) : nb;
  if (lo > cb_lo) cb_lo = lo < nb ? (int)lo : nb;
  for (int cb = cb_lo; cb < cb_hi; ++cb) {
    const int B = blk[cb], b0 = blk[nb + cb], nc = blk[2 * nb + cb];
    if (tid < KNN_BN) sCn[tid] = sqn[map[b0 + (tid < nc ? tid : 0)]];
    const float* brow[KNN_STG];
    bool bok[KNN_STG];
#pragma unroll
    for (int q = 0; q < KNN_STG; ++q) {
      const int c = (tid >> 5) + 8 * q;
      bok[q] = c < nc;
      brow[q] = X + (int64_t)map[b0 + (bok[q] ? c : 0)] * nf;
    }
    const f32x16 acc = knn_gram_tile(s.sA, s.sB, nf, arow, aok, brow, bok);   // (its barriers publish sQn / sCn)
    knn_park_tile(
        s.sD, acc, [&](int r, int c) { return r < na && c < nc; }, [&](int r) { return sQn[r]; },
        [&](int c) { return sCn[c]; });
    __syncthreads();
    // wave w: the minimum of columns [16 w, 16 w + 16) over the 64 rows, by (d2, row, column)
    float d = 3.402823466e+38f;
    int r = lane, c = 16 * wave;
    {
      const float* row = s.sD + lane * (KNN_BN + 1) + 16 * wave;
#pragma unroll
      for (int j = 0; j < 16; ++j)
        if (row[j] < d) {
          d = row[j];
          c = 16 * wave + j;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float od = __shfl_xor(d, o, 64);
      const int orr = __shfl_xor(r, o, 64), oc = __shfl_xor(c, o, 64);
      if (od < d || (od == d && orr < r)) {   // (one column range per wave: equal rows do not meet)
        d = od;
        r = orr;
        c = oc;
      }
    }
    if (lane == 0) {
      wd[wave] = d;
      wr[wave] = r;
      wc[wave] = c;
    }
    __syncthreads();
    if (tid == 0) {
      gn_best t = {wd[0], wr[0], wc[0]};
#pragma unroll
      for (int w = 1; w < 4; ++w)
        if (gn_less(wd[w], wr[w], wc[w], t)) t = {wd[w], wr[w], wc[w]};
      const gn_best have = {bd[B], ba[B], bb[B]};
      if (t.d < 3.402823466e+38f && gn_less(t.d, a0 + t.a, b0 + t.b, have)) {
        bd[B] = t.d;
        ba[B] = a0 + t.a;
        bb[B] = b0 + t.b;
      }
    }
  }
  __syncthreads();
  const int64_t base = ((int64_t)blockIdx.y * nb + qb) * groups;
  for (int g = tid; g < groups; g += MDE_BLOCK) {
    part_d[base + g] = bd[g];
    part_a[base + g] = ba[g] < 0 ? -1 : map[ba[g]];
    part_b[base + g] = bb[g] < 0 ? -1 : map[bb[g]];
  }
}

// One thread per ordered pair (A, B): the diagonal, and for A < B the fold over the blocks of A and the slices.
__global__ __launch_bounds__(MDE_BLOCK) void k_group_fold(int groups, int nb, int slices,
                                                          const int32_t* __restrict__ gfirst,
                                                          const float* __restrict__ part_d,
                                                          const int32_t* __restrict__ part_a,
                                                          const int32_t* __restrict__ part_b,
                                                          float* __restrict__ d2_out, int32_t* __restrict__ row_out) {
  const int i = blockIdx.x * MDE_BLOCK + threadIdx.x;
  if (i >= groups * groups) return;
  const int A = i / groups, B = i - A * groups;
  if (A > B) return;
  gn_best best = {3.402823466e+38f, -1, -1};
  if (A < B)
    for (int sl = 0; sl < slices; ++sl)
      for (int qb = gfirst[A]; qb < gfirst[A + 1]; ++qb) {
        const int64_t at = ((int64_t)sl * nb + qb) * groups + B;
        const float d = part_d[at];
        if (d < 3.402823466e+38f && gn_less(d, part_a[at], part_b[at], best)) best = {d, part_a[at], part_b[at]};
      }
  d2_out[A * groups + B] = best.d;
  d2_out[B * groups + A] = best.d;
  row_out[A * groups + B] = best.a;
  row_out[B * groups + A] = best.b;
}

static bool gn_args_ok(int64_t n, int32_t groups, int32_t slices) {
  return n >= 1 && n < ((int64_t)1 << 31) && groups >= 2 && groups <= GN_MAX_GROUPS && slices >= 0 &&
         slices <= CROSS_MAX_SLICES;
}
static int64_t gn_max_blocks(int64_t n, int32_t groups) { return (n + KNN_BM - 1) / KNN_BM + groups; }
static int64_t gn_align(int64_t words) { return (words + 3) & ~(int64_t)3; }

extern "C" int64_t mde_group_nearest_work_bytes(int64_t n, int32_t groups, int32_t slices) {
  if (!gn_args_ok(n, groups, slices)) {
    mde_set_error("mde_group_nearest_work_bytes: invalid arguments (1 <= n < 2^31, 2 <= groups <= %d, 0 <= slices "
                  "<= %d)", GN_MAX_GROUPS, CROSS_MAX_SLICES);
    return MDE_E_INVALID;
  }
  const int64_t s = cross_resolve_slices(n, n, slices);
  if (s < 0) return s;
  const int64_t nbmax = gn_max_blocks(n, groups);
  // norms, map and three sort arrays | group offsets | block table | first blocks | partials
  const int64_t words = gn_align(n) * 5 + gn_align(groups + 2) + gn_align(3 * nbmax) + gn_align(groups + 1) +
                        3 * s * nbmax * groups;
  return 4 * words;
}

extern "C" int mde_group_nearest(int64_t n, int32_t nf, const float* X, const int32_t* labels, int32_t groups,
                                 int32_t slices, float* d2_out, int32_t* row_out, void* work, void* stream) {
  if (!gn_args_ok(n, groups, slices) || nf <= 0 || !X || !labels || !d2_out || !row_out || !work) {
    mde_set_error("mde_group_nearest: invalid arguments (1 <= n < 2^31, nf >= 1, 2 <= groups <= %d, 0 <= slices <= "
                  "%d, non-null X / labels / d2_out / row_out / work)", GN_MAX_GROUPS, CROSS_MAX_SLICES);
    return MDE_E_INVALID;
  }
  const int64_t s64 = cross_resolve_slices(n, n, slices);
  if (s64 < 0) return (int)s64;
  hipStream_t st = mde_stream(stream);
  const int64_t nbmax = gn_max_blocks(n, groups);
  float* sqn = static_cast<float*>(work);
  int32_t* map = reinterpret_cast<int32_t*>(sqn + gn_align(n));
  uint32_t* keys = reinterpret_cast<uint32_t*>(map + gn_align(n));
  uint32_t* keys2 = keys + gn_align(n);
  uint32_t* vals = keys2 + gn_align(n);
  int32_t* goff = reinterpret_cast<int32_t*>(vals + gn_align(n));
  int32_t* blk = goff + gn_align(groups + 2);
  int32_t* gfirst = blk + gn_align(3 * nbmax);
  float* part = reinterpret_cast<float*>(gfirst + gn_align(groups + 1));
  int rc = mde_row_sqnorm(n, nf, X, sqn, stream);
  if (rc != MDE_OK) return rc;
  const dim3 block(MDE_BLOCK);
  hipLaunchKernelGGL(k_group_keys, dim3((unsigned)((n + MDE_BLOCK - 1) / MDE_BLOCK)), block, 0, st, (int)n, groups,
                     labels, keys, vals);
  MDE_LAUNCH_CHECK();
  MdeDeviceBuf<char> tmp;
  size_t tmp_bytes = 0;
  const int end_bit = gn_bits_for((uint32_t)groups);
  MDE_HIP(mde_sort_pairs_u32(nullptr, tmp_bytes, keys, keys2, vals, reinterpret_cast<uint32_t*>(map), (int)n, 0,
                             end_bit, st));
  MDE_HIP(tmp.alloc(tmp_bytes ? tmp_bytes : 16));
  MDE_HIP(mde_sort_pairs_u32(tmp.get(), tmp_bytes, keys, keys2, vals, reinterpret_cast<uint32_t*>(map), (int)n, 0,
                             end_bit, st));
  hipLaunchKernelGGL(k_group_offsets, dim3((unsigned)((n + 1 + MDE_BLOCK - 1) / MDE_BLOCK)), block, 0, st, (int)n,
                     groups, keys2, goff);
  MDE_LAUNCH_CHECK();
  // the block table is built on the host from the groups' offsets (at most 1026 integers)
  std::vector<int32_t> off((size_t)groups + 2);
  MDE_HIP(hipMemcpyAsync(off.data(), goff, off.size() * sizeof(int32_t), hipMemcpyDeviceToHost, st));
  MDE_HIP(hipStreamSynchronize(st));
  std::vector<int32_t> first((size_t)groups + 1);
  int64_t nb = 0;
  for (int g = 0; g < groups; ++g) {
    first[g] = (int32_t)nb;
    nb += (off[g + 1] - off[g] + KNN_BM - 1) / KNN_BM;
  }
  first[groups] = (int32_t)nb;
  const dim3 fold_grid((unsigned)(((int64_t)groups * groups + MDE_BLOCK - 1) / MDE_BLOCK));
  if (nb == 0) {                               // no row carries a label of [0, groups): every entry is empty
    MDE_HIP(hipMemsetAsync(gfirst, 0, ((size_t)groups + 1) * sizeof(int32_t), st));
    hipLaunchKernelGGL(k_group_fold, fold_grid, block, 0, st, groups, 0, 0, gfirst, part,
                       reinterpret_cast<int32_t*>(part), reinterpret_cast<int32_t*>(part), d2_out, row_out);
    MDE_LAUNCH_CHECK();
    return MDE_OK;
  }
  std::vector<int32_t> table((size_t)(3 * nb));
  for (int g = 0, b = 0; g < groups; ++g)
    for (int32_t p = off[g]; p < off[g + 1]; p += KNN_BM, ++b) {
      table[b] = g;
      table[nb + b] = p;
      table[2 * nb + b] = off[g + 1] - p < KNN_BM ? off[g + 1] - p : KNN_BM;
    }
  MDE_HIP(hipMemcpyAsync(blk, table.data(), table.size() * sizeof(int32_t), hipMemcpyHostToDevice, st));
  MDE_HIP(hipMemcpyAsync(gfirst, first.data(), first.size() * sizeof(int32_t), hipMemcpyHostToDevice, st));
  int64_t s = s64 < nb ? s64 : nb;             // (an empty slice would only write empty partials)
  const int per_slice = (int)((nb + s - 1) / s);
  s = (nb + per_slice - 1) / per_slice;
  float* part_d = part;
  int32_t* part_a = reinterpret_cast<int32_t*>(part_d + s * nb * groups);
  int32_t* part_b = part_a + s * nb * groups;
  rc = knn_raise_lds_limit<k_group_nearest>(96 * 1024);
  if (rc != MDE_OK) return rc;
  hipLaunchKernelGGL(k_group_nearest, dim3((unsigned)nb, (unsigned)s), block, knn_tile_lds_bytes(0, GN_EXTRA), st, nf,
                     groups, (int)nb, per_slice, X, sqn, map, blk, gfirst, part_d, part_a, part_b);
  MDE_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_group_fold, fold_grid, block, 0, st, groups, (int)nb, (int)s, gfirst, part_d, part_a, part_b,
                     d2_out, row_out);
  MDE_LAUNCH_CHECK();
  MDE_HIP(hipStreamSynchronize(st));           // (the host tables above are read by the copies until here)
  return MDE_OK;
}

// mde_ann_refine.hip -- one neighbour-of-neighbour pass over k-NN lists: what repairs the
// misses of the inverted-file search (mde_ann.hip) at the borders of its lists.
//   [ref: pymde/preprocess/data_matrix.py:125-143 -- pynndescent above 10 000 items; here one local join]
//
// Row i holds a list N(i) of k entries ordered by (d2, index) and a reverse list R(i) (the rows that list i,
// built on the host side of pymde_amd/ann.py).  Its candidates are R(i) and N(j) for every j of N(i) and
// R(i); the new list is the k smallest of N(i) and the candidates under (d2, index).  The pass reads the
// previous lists and writes new ones (Jacobi), and the top-k of a set under a total order does not depend on
// the order of the visits: the output is the same on every run, whatever the filters below let through.
//
// k_knn_refine.  A wave owns one row and a workgroup four; lane l < k holds entry l of the list in registers.
//   fill    the raw candidates (c < k: R(i)[c]; else join (c - k) / k, slot (c - k) % k) are taken 64 at a
//           time, one per lane.  A lane drops its candidate when it is -1, the row itself, in the list, or
//           seen earlier in this row -- a per-wave open-addressed set in LDS (integer compare-and-swap, a few
//           probes; when the set is half full the test is skipped: it only saves distances).  The survivors
//           are compacted into a ring of 128 until 64 wait or the raw candidates are used up.
//   d2      up to 64 waiting candidates, one per lane, by knn_wave_pair_d2: the float32 distance the searches
//           give that pair, bit for bit.  It holds barriers, so the four waves run the same number of rounds:
//           the loop ends when no wave has a candidate left, and a wave without one passes valid = false.
//   insert  the candidates that beat the k-th entry are taken one by one from their ballot: the position is
//           the number of entries that precede (dc, ic), the lanes from there on shift up by one.  A
//           candidate that is already listed (a duplicate the set did not catch) is skipped here, so the
//           result never depends on the set.
#include <limits.h>

#include "mde_knn_tile.h"

#define REFINE_FLT_MAX 3.402823466e+38f
#define REFINE_NONE INT_MAX          // index of an empty entry: (FLT_MAX, INT_MAX) follows every real entry
#define REFINE_SET 1024              // slots of a wave's seen-set
#define REFINE_SET_FULL 512          // entries from which the seen-test is skipped
#define REFINE_PROBES 8
#define REFINE_RING 128              // waiting candidates of a wave (fewer than 64 + a batch of 64)

__device__ __forceinline__ bool refine_less(float da, int ia, float db, int ib) {
  return da < db || (da == db && ia < ib);
}
__device__ __forceinline__ int refine_lane_i(int v, int l) { return __builtin_amdgcn_readlane(v, l); }
__device__ __forceinline__ float refine_lane_f(float v, int l) {
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l));
}

__global__ __launch_bounds__(MDE_BLOCK) void k_knn_refine(int n, int nf, int k, const float* __restrict__ X,
                                                          const float* __restrict__ sqn,
                                                          const int32_t* __restrict__ idx_in,
                                                          const float* __restrict__ d2_in,
                                                          const int32_t* __restrict__ rev,
                                                          int32_t* __restrict__ idx_out, float* __restrict__ d2_out,
                                                          int32_t* __restrict__ changed_out,
                                                          unsigned long long* __restrict__ evaluated) {
  __shared__ float sC[4][64 * KNN_RR_KBP];
  __shared__ float sQ[4][KNN_RR_KB];
  __shared__ int sSet[4][REFINE_SET];
  __shared__ int sRing[4][REFINE_RING];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t q = (int64_t)blockIdx.x * 4 + wave;
  const bool live = q < n;
  const int64_t qc = live ? q : n - 1;
  const bool mine = live && lane < k;
  int* set = sSet[wave];
  int* ring = sRing[wave];
  for (int s = lane; s < REFINE_SET; s += 64) set[s] = -1;

  // the list: one entry per lane, empty entries (and lanes >= k) are (FLT_MAX, NONE)
  const int own = mine ? idx_in[qc * k + lane] : -1;
  const bool has = own >= 0 && own < n;
  int li = has ? own : REFINE_NONE;
  float ld = has ? d2_in[qc * k + lane] : REFINE_FLT_MAX;
  const int li0 = li;
  // the joins: the listed rows and the reverse neighbours; one that is both joins once
  const int nbr = has ? own : -1;
  int rv = mine ? rev[qc * k + lane] : -1;
  if (rv < 0 || rv >= n || rv == qc) rv = -1;
  int rjoin = rv;
  for (int t = 0; t < k; ++t)
    if (rv == refine_lane_i(li, t)) rjoin = -1;

  const int total = live ? k + 2 * k * k : 0;   // raw candidates (k <= 64: at most 8256)
  int r0 = 0, head = 0, npend = 0, nset = 0;
  unsigned int neval = 0;
  __syncthreads();
  for (;;) {
    // ---- fill: filter raw candidates until 64 wait
    while (npend < 64 && r0 < total) {
      const int c = r0 + lane;
      const int cc = c >= k ? c - k : 0;
      const int join = cc / k, slot = cc - join * k;
      const int ja = __shfl(nbr, join & 63, 64), jb = __shfl(rjoin, (join - k) & 63, 64);
      const int j = join < k ? ja : jb;
      int cand = -1;
      if (c < k)
        cand = rv;                                // (r0 = 0: lane c holds R(i)[c])
      else if (c < total && j >= 0)
        cand = idx_in[(int64_t)j * k + slot];
      bool keep = cand >= 0 && cand < n && cand != qc;
      if (__ballot(keep)) {
        for (int t = 0; t < k; ++t) keep = keep && cand != refine_lane_i(li, t);
      }
      bool added = false;
      if (keep && nset < REFINE_SET_FULL) {
        unsigned int s = ((unsigned int)cand * 2654435761u) >> 22;    // top 10 bits: a slot of REFINE_SET
        for (int p = 0; p < REFINE_PROBES; ++p) {
          const int old = atomicCAS(&set[s], -1, cand);
          if (old == -1) {
            added = true;
            break;
          }
          if (old == cand) {
            keep = false;
            break;
          }
          s = (s + 1) & (REFINE_SET - 1);
        }
      }
      nset += __popcll(__ballot(added));
      const unsigned long long km = __ballot(keep);
      if (keep) ring[(head + npend + __popcll(km & ((1ull << lane) - 1ull))) & (REFINE_RING - 1)] = cand;
      npend += __popcll(km);
      r0 += 64;
    }
    // ---- all four waves together: done when none has a candidate waiting (the barrier also orders the ring)
    if (!__syncthreads_or(npend > 0)) break;
    const int take = npend < 64 ? npend : 64;
    const int cand = lane < take ? ring[(head + lane) & (REFINE_RING - 1)] : -1;
    head = (head + take) & (REFINE_RING - 1);
    npend -= take;
    neval += take;
    const bool valid = cand >= 0;
    const float dc_mine = knn_wave_pair_d2(sC[wave], sQ[wave], nf, X, X, sqn, sqn, qc, valid ? cand : 0, valid);
    // ---- insert
    float wd = refine_lane_f(ld, k - 1);
    int wi = refine_lane_i(li, k - 1);
    unsigned long long m = __ballot(valid && dc_mine < REFINE_FLT_MAX && refine_less(dc_mine, cand, wd, wi));
    while (m) {
      const int b = __ffsll((long long)m) - 1;
      m &= m - 1;
      const float dc = refine_lane_f(dc_mine, b);
      const int ic = refine_lane_i(cand, b);
      if (!refine_less(dc, ic, wd, wi)) continue;
      if (__ballot(lane < k && li == ic)) continue;
      const int pos = __popcll(__ballot(lane < k && refine_less(ld, li, dc, ic)));
      const float ud = __shfl_up(ld, 1, 64);
      const int ui = __shfl_up(li, 1, 64);
      if (lane < k) {
        if (lane > pos) {
          ld = ud;
          li = ui;
        } else if (lane == pos) {
          ld = dc;
          li = ic;
        }
      }
      wd = refine_lane_f(ld, k - 1);
      wi = refine_lane_i(li, k - 1);
    }
  }
  if (live) {
    if (lane < k) {
      idx_out[q * k + lane] = li == REFINE_NONE ? -1 : li;
      d2_out[q * k + lane] = ld;
    }
    const unsigned long long ch = __ballot(lane < k && li != li0);
    if (lane == 0) {
      if (ch) atomicAdd(changed_out, 1);
      if (neval) atomicAdd(evaluated, (unsigned long long)neval);
    }
  }
}

static bool refine_sizes_ok(int64_t n, int32_t k) {
  return n >= 1 && n < ((int64_t)1 << 31) && k >= 1 && k <= KNN_MAXK;
}

extern "C" int64_t mde_knn_refine_work_bytes(int64_t n, int32_t k) {
  if (!refine_sizes_ok(n, k)) {
    mde_set_error("mde_knn_refine_work_bytes: invalid arguments (1 <= k <= %d, 1 <= n < 2^31)", KNN_MAXK);
    return MDE_E_INVALID;
  }
  return 16;   // [0] uint64: the distances evaluated by the pass
}

extern "C" int mde_knn_refine(int64_t n, int32_t nf, const float* X, const float* sqn, int32_t k,
                              const int32_t* idx_in, const float* d2_in, const int32_t* rev, int32_t* idx_out,
                              float* d2_out, int32_t* changed_out, void* work, void* stream) {
  if (!refine_sizes_ok(n, k) || nf < 1 || !X || !sqn || !idx_in || !d2_in || !rev || !idx_out || !d2_out ||
      !changed_out || !work || idx_out == idx_in || d2_out == d2_in) {
    mde_set_error("mde_knn_refine: invalid arguments (1 <= k <= %d, 1 <= n < 2^31, nf >= 1, non-null X / sqn / "
                  "idx_in / d2_in / rev / idx_out / d2_out / changed_out / work; the outputs are not the inputs)",
                  KNN_MAXK);
    return MDE_E_INVALID;
  }
  hipStream_t st = mde_stream(stream);
  MDE_HIP(hipMemsetAsync(changed_out, 0, sizeof(int32_t), st));
  MDE_HIP(hipMemsetAsync(work, 0, 16, st));
  hipLaunchKernelGGL(k_knn_refine, dim3((unsigned)((n + 3) / 4)), dim3(MDE_BLOCK), 0, st, (int)n, nf, k, X, sqn,
                     idx_in, d2_in, rev, idx_out, d2_out, changed_out, static_cast<unsigned long long*>(work));
  MDE_LAUNCH_CHECK();
  return MDE_OK;
}

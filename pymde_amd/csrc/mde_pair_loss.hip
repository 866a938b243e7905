// mde_pair_loss.hip -- the loss and the gradient of a DENSE MDE problem: a loss of pymde_amd.losses
// over ALL n (n - 1) / 2 pairs without an edge list, what pymde_amd.DenseMDE minimises, in O(n) memory beside D.
//
// For every row i and every row j != i (by index: a duplicate of row i elsewhere counts)
//   E = |x_i - x_j| from the differences (never |x|^2 + |y|^2 - 2 x.y: the gradient multiplies f'(E) / E by x_i - x_j,
//       and the expansion cancels for close points, exactly where f'(E) / E is large),
//   D = d_scale * the original deviation of the pair, from one of two sources:
//       Gram     the 64x64 Gram tile of the prepared data rows A [n, nf] (mde_knn_tile.h), parked as squared distances,
//                through pair_dist(d2, mode): bit for bit the D of mde_pair_moments;
//       matrix   a 64x64 tile of a row-major float32 [n, n] matrix, parked in the same LDS block (a wave reads whole
//                256-byte row segments; 64-bit offsets);
//   (l, gd) = mde_eval_rt(kind, E^2, a0 = D, a1 = 1 / D^2, scalars), gd = l'(E) / E under the reference's
//       NaN / Inf -> 1 rule (mde_fix_g),
//   row_loss[i] = sum_j l,  G[i, :] = sum_j gd (x_i - x_j),  loss = sum_i row_loss[i] / (2 P),  grad = G / P,
//   P = n (n - 1) / 2: MDE(n, d, all_edges(n), loss(deviations)).average_distortion and its gradient.
//
//   k_pair_loss_walk   the grid of k_pair_walk: workgroup (x, y) owns 64 rows and the column tiles of slice y.  Per
//                      tile the D side is parked in sD and the 64 column rows of X are staged as [64][DC] floats
//                      (DC = d padded with zeros to 1, 2, 3 or 8); thread t owns tile row t & 63, kept in registers,
//                      and the 16 columns 16 (t >> 6) ...: the lanes of a wave read the same staged column (a
//                      broadcast) and 64 rows of sD at stride 65 (conflict-free).  1 + DC double accumulators per
//                      thread, every product formed in double from its float32 terms; the four threads of a row are
//                      combined in thread order.  No floating-point atomics.
//   k_pair_loss_fold   adds the per-slice partials in slice order: row_loss, and grad = G / P rounded once
//   k_pair_loss_total  one workgroup reduces row_loss to the loss in a fixed order
// For a given slice count the loss, the gradient and row_loss are the same bits on every run.
//
// mde_pair_loss_cross is the RECTANGULAR form, what pymde_amd.DensePlacement minimises: the rows
// are n_q free query rows (Q, XQ), the columns n_c fixed corpus rows (C, XC), D comes from the Gram tile of Q against
// C or from an [n_q, n_c] matrix, and nothing is "self".  The same kernels: SELF = false drops the row != col test at
// compile time and makes k_pair_loss_walk take its rows from a LIST; the fold divides by P = n_q n_c and the total by
// 1 P instead of 2 P, since every pair is in one row.  No gradient for XC.
//
// mde_pair_loss_cross_rows is the same walk over a list of query rows that the caller passes, what
// the per-row placement solver (mde_rows.hip) evaluates once its first rows have finished: workgroup x owns the list
// entries 64 x ..., reads Q, the row norms, XQ and the Dm row through the list, and the fold writes row_loss and
// row_grad = G / n_c at the rows' own indices.  mde_pair_loss_cross is this call with no list (every row, in order),
// the divisor P, and the total.
//
// mde_pair_loss_weighted, mde_pair_loss_cross_weighted and mde_pair_loss_cross_rows_weighted are
// the three calls with a weight per pair -- D^-p formed here, or a matrix W whose zeros are MISSING pairs (WSRC, another
// compile-time variant of k_pair_loss_walk) -- and with the number of pairs that count passed in.  The unweighted calls
// launch the WSRC = PAIR_W_NONE instantiations.  mde_pair_weights_check, at the end, is the one pass over W that
// pymde_amd.dense validates it with.
#include <math.h>

#include "mde_pair.h"
#include "mde_functions.h"

#define PAIR_LOSS_MAX_D 8
#define PAIR_LOSS_XS (KNN_BN * PAIR_LOSS_MAX_D)   // floats of the staged column rows of X: 2 KB

// The weight of a pair, a compile-time variant of the walk:
//   PAIR_W_NONE    what the walk was: the weighted kinds get a1 = 1 / D^2, nothing else is weighted;
//   PAIR_W_POWER   w = D^-p from the pair's own D (after d_scale): no per-pair array, either source of D;
//   PAIR_W_MATRIX  w = W[i][j], a row-major float32 matrix shaped like Dm, whose 64x64 tile is loaded as the Dm
//                  tile is and parked in the idle tile after sD; w == 0 is a MISSING pair: it is skipped before its D
//                  (which may be NaN or infinite in a matrix) is looked at.
// For the weighted kinds w takes the place of a1; for every other kind f and gd are multiplied by w in float32.
#define PAIR_W_NONE MDE_PAIR_W_NONE
#define PAIR_W_POWER MDE_PAIR_W_POWER
#define PAIR_W_MATRIX MDE_PAIR_W_MATRIX
struct PairWeights {
  const float* W;   // PAIR_W_MATRIX: [n_q, n_c] (the square problem: [n, n])
  float p;          // PAIR_W_POWER: the exponent
  int pclass;       // PAIR_W_POWER: 0, 1, 2 for p == 0, 1, 2 (exact forms), 3 for powf
};

// D^-p.  p = 2 is the expression of the losses' default weights (the same bits), p = 1 one IEEE division, p = 0
// exactly 1; D = 0 gives what these expressions give (+inf for p > 0), as the default weights do.
__device__ __forceinline__ float pair_power_weight(float D, int pclass, float p) {
  if (pclass == 2) return 1.0f / (D * D);
  if (pclass == 1) return 1.0f / D;
  if (pclass == 0) return 1.0f;
  return powf(D, -p);
}

// SELF is the square problem: the workgroup's 64 rows are the rows 64 x ... themselves and `rows` is not read.
// !SELF is the rectangular one, and its rows come from a LIST: the workgroup's rows are the list entries 64 x ... of
// `rows` (NULL: the rows themselves), n_q is the length of the list, and the partials are indexed by list position.
template <int DC, bool MATRIX, bool SELF, int WSRC>
__global__ __launch_bounds__(MDE_BLOCK) void k_pair_loss_walk(int n_q, int n_c, int nf, int d, int mode,
                                                              int64_t slice_cols, const float* __restrict__ Q,
                                                              const float* __restrict__ qn,
                                                              const float* __restrict__ C,
                                                              const float* __restrict__ cn,
                                                              const float* __restrict__ Dm,
                                                              const float* __restrict__ XQ,
                                                              const float* __restrict__ XC, int kind, int weighted,
                                                              MdeScalars S, float d_scale,
                                                              double* __restrict__ part,
                                                              const int32_t* __restrict__ rows, PairWeights wt) {
  constexpr bool WMAT = WSRC == PAIR_W_MATRIX, ROWS = !SELF;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const knn_tile_lds s = knn_tile_carve(lds, 0, PAIR_TILE + PAIR_LOSS_XS + (ROWS ? KNN_BM : 0));
  float* sW = s.extra;                                          // [KNN_BM][KNN_BN + 1] the weights of the tile (WMAT)
  float* sX = s.extra + PAIR_TILE;                              // [KNN_BN][DC]
  const int tid = threadIdx.x, r = tid & 63, w = tid >> 6;
  const int64_t row0 = (int64_t)blockIdx.x * KNN_BM;
  int* sRow = reinterpret_cast<int*>(sX + PAIR_LOSS_XS);        // [KNN_BM] the rows of the list entries (ROWS)
  if constexpr (ROWS) {
    if (tid < KNN_BM) sRow[tid] = row0 + tid < n_q ? (rows ? rows[row0 + tid] : (int)(row0 + tid)) : 0;
    __syncthreads();
  }
  // the row behind tile row rr: any readable row where the list has ended
  auto row_of = [&](int rr) -> int64_t { return ROWS ? (int64_t)sRow[rr] : row0 + rr; };
  const int64_t lo = (int64_t)blockIdx.y * slice_cols;
  const int64_t c_lo = lo < n_c ? lo : n_c, c_hi = lo + slice_cols < n_c ? lo + slice_cols : n_c;
  float xi[DC];                                                 // the thread's own row
#pragma unroll
  for (int k = 0; k < DC; ++k) xi[k] = (row0 + r < n_q && k < d) ? XQ[row_of(r) * d + k] : 0.0f;
  const float* arow[KNN_STG];
  bool qok[KNN_STG];
  if constexpr (!MATRIX) {
#pragma unroll
    for (int q = 0; q < KNN_STG; ++q) {
      const int64_t gr = row0 + (tid >> 5) + 8 * q;
      qok[q] = gr < n_q;
      arow[q] = Q + (qok[q] ? (ROWS ? row_of((tid >> 5) + 8 * q) : gr) : 0) * nf;
    }
  }
  double sl = 0.0, sg[DC];
#pragma unroll
  for (int k = 0; k < DC; ++k) sg[k] = 0.0;
  for (int64_t col0 = c_lo; col0 < c_hi; col0 += KNN_BN) {
    auto keep = [&](int rr, int cc) {
      return row0 + rr < n_q && col0 + cc < n_c && (!SELF || row0 + rr != col0 + cc);
    };
    // the tile of W: loaded and parked as the Dm tile below is; what the tile does not have gets the weight 0
    float wv[WMAT ? KNN_BM / 4 : 1];
    auto load_w = [&]() {
      const int lane = tid & 63;
      const int64_t gc = col0 + lane < n_c ? col0 + lane : n_c - 1;
#pragma unroll
      for (int q = 0; q < KNN_BM / 4; ++q) {
        const int64_t gr = ROWS ? row_of(w + 4 * q) : (row0 + w + 4 * q < n_q ? row0 + w + 4 * q : n_q - 1);
        wv[q] = wt.W[gr * (int64_t)n_c + gc];
      }
    };
    auto park_w = [&]() {
      const int lane = tid & 63;
#pragma unroll
      for (int q = 0; q < KNN_BM / 4; ++q) sW[(w + 4 * q) * (KNN_BN + 1) + lane] = keep(w + 4 * q, lane) ? wv[q] : 0.0f;
    };
    if constexpr (MATRIX) {
      // wave w takes the tile rows w, w + 4, ...: all sixteen loads go out from clamped addresses before the first is
      // used, and what the tile does not have (or the diagonal of the square walk) is replaced when the registers are
      // parked
      const int lane = tid & 63;
      const int64_t gc = col0 + lane < n_c ? col0 + lane : n_c - 1;
      float v[KNN_BM / 4];
#pragma unroll
      for (int q = 0; q < KNN_BM / 4; ++q) {
        const int64_t gr = ROWS ? row_of(w + 4 * q) : (row0 + w + 4 * q < n_q ? row0 + w + 4 * q : n_q - 1);
        v[q] = Dm[gr * (int64_t)n_c + gc];
      }
      if constexpr (WMAT) load_w();
      __syncthreads();                                          // the walk of the last tile is over
#pragma unroll
      for (int q = 0; q < KNN_BM / 4; ++q)
        s.sD[(w + 4 * q) * (KNN_BN + 1) + lane] = keep(w + 4 * q, lane) ? v[q] : PAIR_FLT_MAX;
      if constexpr (WMAT) park_w();
    } else {
      const float* acol[KNN_STG];
      bool cok[KNN_STG];
#pragma unroll
      for (int q = 0; q < KNN_STG; ++q) {
        const int64_t gc = col0 + (tid >> 5) + 8 * q;
        cok[q] = gc < n_c;
        acol[q] = C + (cok[q] ? gc : n_c - 1) * nf;
      }
      // the park follows the barriers of knn_gram_tile: every thread is past the walk of the last tile by then
      const f32x16 acc = knn_gram_tile(s.sA, s.sB, nf, arow, qok, acol, cok);
      knn_park_tile(s.sD, acc, keep, [&](int rr) { return qn[row_of(rr)]; }, [&](int cc) { return cn[col0 + cc]; });
      // (the tile of W in four batches of four rows, after the Gram tile: sixteen loads held over the tile's feature
      // loop cost its occupancy)
      if constexpr (WMAT) {
        const int lane = tid & 63;
        const int64_t gc = col0 + lane < n_c ? col0 + lane : n_c - 1;
#pragma unroll 1
        for (int q0 = 0; q0 < KNN_BM / 4; q0 += 4) {
          float b[4];
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const int rr = w + 4 * (q0 + q);
            const int64_t gr = ROWS ? row_of(rr) : (row0 + rr < n_q ? row0 + rr : n_q - 1);
            b[q] = wt.W[gr * (int64_t)n_c + gc];
          }
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const int rr = w + 4 * (q0 + q);
            sW[rr * (KNN_BN + 1) + lane] = keep(rr, lane) ? b[q] : 0.0f;
          }
        }
      }
    }
    for (int i = tid; i < KNN_BN * DC; i += MDE_BLOCK) {
      const int c = i / DC, k = i - c * DC;
      sX[i] = (col0 + c < n_c && k < d) ? XC[(col0 + c) * d + k] : 0.0f;
    }
    __syncthreads();
    const float* pd = s.sD + r * (KNN_BN + 1) + w * PAIR_COLS;
    const float* px = sX + w * PAIR_COLS * DC;
    const float* pw = sW + r * (KNN_BN + 1) + w * PAIR_COLS;
#pragma unroll 4
    for (int cc = 0; cc < PAIR_COLS; ++cc) {
      const float v = pd[cc];
      float wgt = 0.0f;
      bool counts = v != PAIR_FLT_MAX;                          // what keep() refused is parked as FLT_MAX
      if constexpr (WMAT) {
        wgt = pw[cc];                                           // ... and with the weight 0
        counts = counts && wgt > 0.0f;                          // a missing pair: its D is never evaluated
      }
      if (counts) {
        const float D = (MATRIX ? v : pair_dist(v, mode)) * d_scale;
        float diff[DC], ss = 0.0f;
#pragma unroll
        for (int k = 0; k < DC; ++k) {
          diff[k] = xi[k] - px[cc * DC + k];
          ss = fmaf(diff[k], diff[k], ss);
        }
        float a1;
        if constexpr (WSRC == PAIR_W_NONE) {
          a1 = weighted ? 1.0f / (D * D) : 0.0f;                // the losses' default weights
        } else {
          if constexpr (WSRC == PAIR_W_POWER) wgt = pair_power_weight(D, wt.pclass, wt.p);
          a1 = weighted ? wgt : 0.0f;                           // WeightedQuadratic(deviations, weights)
        }
        float f, gd;
        mde_eval_rt(kind, ss, D, a1, S, f, gd);
        gd = mde_fix_g(gd);
        if constexpr (WSRC != PAIR_W_NONE) {
          if (!weighted) {
            f *= wgt;
            gd *= wgt;
          }
        }
        sl += (double)f;
#pragma unroll
        for (int k = 0; k < DC; ++k) sg[k] = fma((double)gd, (double)diff[k], sg[k]);
      }
    }
  }
  __syncthreads();                                              // the last walk is over: sD and the tile after it are free
  constexpr int NV = 1 + DC;
  double* cs = reinterpret_cast<double*>(s.sD);                 // [4][KNN_BM][NV]; sD starts at a multiple of 8 bytes
  double* mine = cs + ((size_t)w * KNN_BM + r) * NV;
  mine[0] = sl;
#pragma unroll
  for (int k = 0; k < DC; ++k) mine[1 + k] = sg[k];
  __syncthreads();
  // thread (row, v) adds value v of the row's four threads in thread order
  for (int i = tid; i < KNN_BM * NV; i += MDE_BLOCK) {
    const int rr = i / NV, v = i - NV * rr;
    if (row0 + rr < n_q && v <= d) {
      double t = cs[((size_t)0 * KNN_BM + rr) * NV + v];
#pragma unroll
      for (int u = 1; u < 4; ++u) t += cs[((size_t)u * KNN_BM + rr) * NV + v];
      part[((int64_t)blockIdx.y * n_q + row0 + rr) * (1 + d) + v] = t;
    }
  }
}
static_assert(4 * KNN_BM * (1 + PAIR_LOSS_MAX_D) * sizeof(double) <= 2 * PAIR_TILE * sizeof(float),
              "the row partials must fit in the parked tile and the tile after it");

// row_loss[row] and grad[row, :] = G / divisor from the per-slice partials [slices, n_rows, 1 + d], added in slice
// order.  The partials are indexed by list position, the outputs by the row itself (`rows`; NULL: the position is the
// row, as in the square problem).  The divisor is P for the joint calls and n_c for the list calls, so that there a
// row's result does not depend on the list it came in.
__global__ __launch_bounds__(MDE_BLOCK) void k_pair_loss_fold(int64_t n_rows, int d, int slices, double divisor,
                                                              const double* __restrict__ part,
                                                              const int32_t* __restrict__ rows,
                                                              double* __restrict__ row_loss,
                                                              float* __restrict__ grad) {
  const int64_t total = n_rows * (1 + d);
  for (int64_t i = (int64_t)blockIdx.x * MDE_BLOCK + threadIdx.x; i < total; i += (int64_t)gridDim.x * MDE_BLOCK) {
    double t = 0.0;
    for (int y = 0; y < slices; ++y) t += part[(int64_t)y * total + i];
    const int64_t pos = i / (1 + d);
    const int v = (int)(i - pos * (1 + d));
    const int64_t row = rows ? (int64_t)rows[pos] : pos;
    if (v == 0)
      row_loss[row] = t;
    else
      grad[row * d + v - 1] = (float)(t / divisor);
  }
}

// One workgroup: thread t adds the rows t, t + 256, ... in row order, thread 0 then adds the 256 threads' sums in
// thread order.  loss = sum_i row_loss[i] / (factor * pairs): factor 2 for the square problem, where every pair is in
// two rows, 1 for the rectangular one.
__global__ __launch_bounds__(MDE_BLOCK) void k_pair_loss_total(int64_t n, double pairs, double factor,
                                                               const double* __restrict__ row_loss,
                                                               double* __restrict__ loss) {
  __shared__ double sums[MDE_BLOCK];
  double t = 0.0;
  for (int64_t i = threadIdx.x; i < n; i += MDE_BLOCK) t += row_loss[i];
  sums[threadIdx.x] = t;
  __syncthreads();
  if (threadIdx.x == 0) {
    double a = sums[0];
    for (int u = 1; u < MDE_BLOCK; ++u) a += sums[u];
    loss[0] = a / (factor * pairs);
  }
}

static bool pair_loss_kind_ok(int32_t kind) { return kind >= MDE_F_L_QUADRATIC && kind <= MDE_F_L_LOG1P; }
static bool pair_loss_args_ok(int64_t n, int32_t d, int32_t slices) {
  return pair_args_ok(n, n, slices) && d >= 1 && d <= PAIR_LOSS_MAX_D;
}
static bool pair_loss_cross_args_ok(int64_t n_q, int64_t n_c, int32_t d, int32_t slices) {
  return n_q >= 1 && n_q < ((int64_t)1 << 31) && n_c >= 1 && n_c < ((int64_t)1 << 31) && slices >= 0 &&
         slices <= CROSS_MAX_SLICES && d >= 1 && d <= PAIR_LOSS_MAX_D;
}

// work: [s, n, 1 + d] doubles | the row norms of A, [n] floats (the Gram source; the room is there for either source)
extern "C" int64_t mde_pair_loss_work_bytes(int64_t n, int32_t d, int32_t slices) {
  if (!pair_loss_args_ok(n, d, slices)) {
    mde_set_error("mde_pair_loss_work_bytes: invalid arguments (2 <= n < 2^31, 1 <= d <= %d, 0 <= slices <= %d)",
                  PAIR_LOSS_MAX_D, CROSS_MAX_SLICES);
    return MDE_E_INVALID;
  }
  const int64_t s = cross_resolve_slices(n, n, slices);
  if (s < 0) return s;
  return s * n * (1 + d) * 8 + 4 * n;
}

// work: [s, n_q, 1 + d] doubles | the row norms of Q, [n_q] floats | the row norms of C, [n_c] floats
extern "C" int64_t mde_pair_loss_cross_work_bytes(int64_t n_q, int64_t n_c, int32_t d, int32_t slices) {
  if (!pair_loss_cross_args_ok(n_q, n_c, d, slices)) {
    mde_set_error("mde_pair_loss_cross_work_bytes: invalid arguments (1 <= n_q, n_c < 2^31, 1 <= d <= %d, 0 <= slices "
                  "<= %d)", PAIR_LOSS_MAX_D, CROSS_MAX_SLICES);
    return MDE_E_INVALID;
  }
  const int64_t s = cross_resolve_slices(n_q, n_c, slices);
  if (s < 0) return s;
  return s * n_q * (1 + d) * 8 + 4 * (n_q + n_c);
}

// The arguments of one walk, filled once per entry point: n_q rows (the rectangular problem: list entries, the rows of
// `rows`) against the n_c columns in s slices; part [s, n_q, 1 + d]; qn / cn are read by the Gram source only, and a
// non-null Dm is the matrix source.
struct PairWalk {
  int64_t n_q, n_c;
  int32_t nf, mode;
  const float *Q, *qn, *C, *cn, *Dm;
  float d_scale;
  int32_t d;
  const float *XQ, *XC;
  int32_t kind;
  MdeScalars S;
  int64_t s;
  double* part;
  const int32_t* rows;
  int32_t wsrc;
  PairWeights wt;
  hipStream_t st;
};

// The one launch of the walk: the instantiation <DC, MATRIX, SELF, WSRC> is looked up, not branched to.
// (PAIR_WALK_WIDTHS takes SELF from the template it is used in.)
using PairWalkKernel = decltype(&k_pair_loss_walk<1, false, true, PAIR_W_NONE>);
static_assert(PAIR_W_NONE == 0 && PAIR_W_POWER == 1 && PAIR_W_MATRIX == 2, "the weight source indexes the kernels");
#define PAIR_WALK_WIDTHS(MATRIX, WSRC)                                                   \
  {k_pair_loss_walk<1, MATRIX, SELF, WSRC>, k_pair_loss_walk<2, MATRIX, SELF, WSRC>,     \
   k_pair_loss_walk<3, MATRIX, SELF, WSRC>, k_pair_loss_walk<PAIR_LOSS_MAX_D, MATRIX, SELF, WSRC>}
template <bool SELF>
static int pair_loss_walk(const PairWalk& a) {
  static const PairWalkKernel kernels[2][3][4] = {
      {PAIR_WALK_WIDTHS(false, PAIR_W_NONE), PAIR_WALK_WIDTHS(false, PAIR_W_POWER),
       PAIR_WALK_WIDTHS(false, PAIR_W_MATRIX)},
      {PAIR_WALK_WIDTHS(true, PAIR_W_NONE), PAIR_WALK_WIDTHS(true, PAIR_W_POWER),
       PAIR_WALK_WIDTHS(true, PAIR_W_MATRIX)}};
  const int64_t tiles = (a.n_c + KNN_BN - 1) / KNN_BN;
  const int64_t slice_cols = ((tiles + a.s - 1) / a.s) * KNN_BN;   // whole tiles; the last slices may be short or empty
  const dim3 grid((unsigned)((a.n_q + KNN_BM - 1) / KNN_BM), (unsigned)a.s);
  const size_t lds = knn_tile_lds_bytes(0, PAIR_TILE + PAIR_LOSS_XS + (SELF ? 0 : KNN_BM));
  const int weighted = a.kind == MDE_F_L_WEIGHTED_QUADRATIC || a.kind == MDE_F_L_WEIGHTED_POWER;
  const int width = a.d <= 3 ? a.d - 1 : 3;                         // DC = d padded to 1, 2, 3 or 8
  hipLaunchKernelGGL(kernels[a.Dm != nullptr][a.wsrc][width], grid, dim3(MDE_BLOCK), lds, a.st, (int)a.n_q,
                     (int)a.n_c, a.nf, a.d, a.mode, slice_cols, a.Q, a.qn, a.C, a.cn, a.Dm, a.XQ, a.XC, a.kind, weighted,
                     a.S, a.d_scale, a.part, a.rows, a.wt);
  MDE_LAUNCH_CHECK();
  return MDE_OK;
}
#undef PAIR_WALK_WIDTHS

// The fold of a walk and, where `loss` is asked for, the total over its n_q rows: loss = sum row_loss / (factor *
// divisor), factor 2 for the square problem, where every pair is in two rows, 1 for the rectangular one.
static int pair_loss_fold(const PairWalk& a, double divisor, double factor, double* loss, double* row_loss,
                          float* grad) {
  hipLaunchKernelGGL(k_pair_loss_fold, dim3(mde_grid(a.n_q * (1 + a.d), MDE_BLOCK, 4096)), dim3(MDE_BLOCK), 0, a.st,
                     a.n_q, (int)a.d, (int)a.s, divisor, a.part, a.rows, row_loss, grad);
  MDE_LAUNCH_CHECK();
  if (loss) {
    hipLaunchKernelGGL(k_pair_loss_total, dim3(1), dim3(MDE_BLOCK), 0, a.st, a.n_q, divisor, factor, row_loss, loss);
    MDE_LAUNCH_CHECK();
  }
  return MDE_OK;
}

// The weight arguments of the *_weighted entry points; `pairs` is looked at where the entry point has one.
static bool pair_weights_ok(const char* fn, int32_t wsrc, float p, const float* W, bool has_pairs, double pairs) {
  const bool source_ok = wsrc == PAIR_W_NONE || wsrc == PAIR_W_POWER || wsrc == PAIR_W_MATRIX;
  const bool w_ok = wsrc == PAIR_W_MATRIX ? W != nullptr : W == nullptr;
  if (source_ok && w_ok && p >= 0.0f && isfinite(p) && (!has_pairs || (pairs > 0.0 && isfinite(pairs)))) return true;
  mde_set_error("%s: invalid weights (the source is MDE_PAIR_W_NONE, MDE_PAIR_W_POWER or MDE_PAIR_W_MATRIX; W is "
                "non-null under MDE_PAIR_W_MATRIX and NULL otherwise: one source, not both; p is finite and >= 0%s)",
                fn, has_pairs ? "; pairs is finite and > 0" : "");
  return false;
}
static PairWeights pair_weights(int32_t wsrc, float p, const float* W) {
  PairWeights wt;
  wt.W = wsrc == PAIR_W_MATRIX ? W : nullptr;
  wt.p = p;
  wt.pclass = p == 0.0f ? 0 : p == 1.0f ? 1 : p == 2.0f ? 2 : 3;
  return wt;
}

// The square problem behind mde_pair_loss (no weights, pairs = n (n - 1) / 2) and mde_pair_loss_weighted: rows and
// columns are the same items, the diagonal is left out.
static int pair_loss_square(const char* fn, int64_t n, int32_t nf, const float* A, int32_t mode, const float* Dm,
                            float d_scale, int32_t d, const float* X, int32_t kind, float s0, float s1, float s2,
                            int32_t slices, int32_t wsrc, float p, const float* W, double pairs, double* loss,
                            float* grad, double* row_loss, void* work, void* stream) {
  const bool source_ok = (A != nullptr) != (Dm != nullptr) && (!A || (nf >= 1 && (mode == 0 || mode == 1)));
  if (!pair_loss_args_ok(n, d, slices) || !source_ok || !pair_loss_kind_ok(kind) || !(d_scale > 0.0f) ||
      !isfinite(d_scale) || !X || !loss || !grad || !row_loss || !work) {
    mde_set_error("%s: invalid arguments (2 <= n < 2^31, 1 <= d <= %d, exactly one of A (nf >= 1, mode 0 / "
                  "1) and Dm, kind one of the MDE_F_L_* losses, d_scale positive and finite, 0 <= slices <= %d, "
                  "non-null X / outputs / work)", fn, PAIR_LOSS_MAX_D, CROSS_MAX_SLICES);
    return MDE_E_INVALID;
  }
  if (!pair_weights_ok(fn, wsrc, p, W, true, pairs)) return MDE_E_INVALID;
  const int64_t s = cross_resolve_slices(n, n, slices);
  if (s < 0) return (int)s;
  double* part = static_cast<double*>(work);
  float* an = reinterpret_cast<float*>(part + s * n * (1 + d));
  if (A) {
    const int rc = mde_row_sqnorm(n, nf, A, an, stream);
    if (rc != MDE_OK) return rc;
  }
  PairWalk a;
  a.n_q = n, a.n_c = n, a.nf = nf, a.mode = mode;
  a.Q = A, a.qn = an, a.C = A, a.cn = an, a.Dm = Dm;
  a.d_scale = d_scale, a.d = d, a.XQ = X, a.XC = X, a.kind = kind, a.S = MdeScalars{s0, s1, s2};
  a.s = s, a.part = part, a.rows = nullptr;
  a.wsrc = wsrc, a.wt = pair_weights(wsrc, p, W), a.st = mde_stream(stream);
  const int rc = pair_loss_walk<true>(a);
  return rc != MDE_OK ? rc : pair_loss_fold(a, pairs, 2.0, loss, row_loss, grad);
}

extern "C" int mde_pair_loss(int64_t n, int32_t nf, const float* A, int32_t mode, const float* Dm, float d_scale,
                             int32_t d, const float* X, int32_t kind, float s0, float s1, float s2, int32_t slices,
                             double* loss, float* grad, double* row_loss, void* work, void* stream) {
  return pair_loss_square("mde_pair_loss", n, nf, A, mode, Dm, d_scale, d, X, kind, s0, s1, s2, slices, PAIR_W_NONE,
                          0.0f, nullptr, 0.5 * (double)n * (double)(n - 1), loss, grad, row_loss, work, stream);
}

// mde_pair_loss with a weight per pair and the count of the pairs that count passed in.
extern "C" int mde_pair_loss_weighted(int64_t n, int32_t nf, const float* A, int32_t mode, const float* Dm,
                                      float d_scale, int32_t d, const float* X, int32_t kind, float s0, float s1,
                                      float s2, int32_t slices, int32_t wsource, float p, const float* W, double pairs,
                                      double* loss, float* grad, double* row_loss, void* work, void* stream) {
  return pair_loss_square("mde_pair_loss_weighted", n, nf, A, mode, Dm, d_scale, d, X, kind, s0, s1, s2, slices,
                          wsource, p, W, pairs, loss, grad, row_loss, work, stream);
}

// The most list entries times slices the walk of mde_pair_loss_cross_rows can hold partials for, over every list
// length 1 .. n_q: slices * n_q for a given count; for the automatic count (resolved from the LIST's length, so that
// a short list still fills the device) s * n_rows <= s * 64 qb < 64 (CROSS_GRID_PER_CU cus + qb) < 64 (GRID_PER_CU +
// 1) cus whenever the corpus is split (qb < cus), and never more than the finest split times n_q.
static int64_t pair_loss_rows_part_rows(int64_t n_q, int64_t n_c, int32_t slices) {
  if (slices != 0) return (int64_t)slices * n_q;
  int cus = 0;
  const int rc = cross_cu_count(&cus);
  if (rc != MDE_OK) return rc;
  const int64_t tiles = (n_c + KNN_BN - 1) / KNN_BN;
  const int64_t finest = tiles / CROSS_MIN_TILES > 1 ? tiles / CROSS_MIN_TILES : 1;
  int64_t split = (int64_t)KNN_BM * (CROSS_GRID_PER_CU + 1) * cus;
  if (split > finest * n_q) split = finest * n_q;
  return split > n_q ? split : n_q;
}

// work: [part_rows, 1 + d] doubles | the row norms of Q, [n_q] floats | the row norms of C, [n_c] floats
extern "C" int64_t mde_pair_loss_cross_rows_work_bytes(int64_t n_q, int64_t n_c, int32_t d, int32_t slices) {
  if (!pair_loss_cross_args_ok(n_q, n_c, d, slices)) {
    mde_set_error("mde_pair_loss_cross_rows_work_bytes: invalid arguments (1 <= n_q, n_c < 2^31, 1 <= d <= %d, 0 <= "
                  "slices <= %d)", PAIR_LOSS_MAX_D, CROSS_MAX_SLICES);
    return MDE_E_INVALID;
  }
  const int64_t part_rows = pair_loss_rows_part_rows(n_q, n_c, slices);
  if (part_rows < 0) return part_rows;
  return part_rows * (1 + d) * 8 + 4 * (n_q + n_c);
}

// The rectangular problem: the (query row, corpus row) pairs of the n_rows query rows of `rows` (NULL: all n_q), a
// gradient for the query rows only, the per-row sums written at the rows' own indices.  The JOINT calls
// (mde_pair_loss_cross and its weighted form) have no list: all rows, partials as mde_pair_loss_cross_work_bytes lays
// them out, the gradient divided by `pairs`, and the total.  The list calls divide by n_c and have neither `pairs`
// nor `loss`.
static int pair_loss_rect(const char* fn, bool joint, int64_t n_q, int64_t n_c, int32_t nf, const float* Q,
                          const float* C, int32_t mode, const float* Dm, float d_scale, int32_t d, const float* XQ,
                          const float* XC, int32_t kind, float s0, float s1, float s2, int32_t slices, int64_t n_rows,
                          const int32_t* rows, int32_t wsrc, float p, const float* W, double pairs, double* loss,
                          double* row_loss, float* row_grad, void* work, void* stream) {
  const bool gram = Q != nullptr && C != nullptr && Dm == nullptr;
  const bool matrix = Q == nullptr && C == nullptr && Dm != nullptr;
  const bool source_ok = matrix || (gram && nf >= 1 && (mode == 0 || mode == 1));
  const bool rows_ok = joint || (n_rows >= 1 && n_rows <= n_q && (rows != nullptr || n_rows == n_q));
  if (!pair_loss_cross_args_ok(n_q, n_c, d, slices) || !source_ok || !rows_ok || !pair_loss_kind_ok(kind) ||
      !(d_scale > 0.0f) || !isfinite(d_scale) || !XQ || !XC || (joint && !loss) || !row_loss || !row_grad || !work) {
    mde_set_error("%s: invalid arguments (1 <= n_q, n_c < 2^31, 1 <= d <= %d, either both Q and C (nf >= 1, mode 0 / "
                  "1) or Dm alone, kind one of the MDE_F_L_* losses, d_scale positive and finite, 0 <= slices <= %d, "
                  "%snon-null XQ / XC / outputs / work)", fn, PAIR_LOSS_MAX_D, CROSS_MAX_SLICES,
                  joint ? "" : "1 <= n_rows <= n_q and n_rows == n_q without rows, ");
    return MDE_E_INVALID;
  }
  if (!pair_weights_ok(fn, wsrc, p, W, joint, pairs)) return MDE_E_INVALID;
  const int64_t s = cross_resolve_slices(n_rows, n_c, slices);
  if (s < 0) return (int)s;
  const int64_t part_rows = joint ? s * n_q : pair_loss_rows_part_rows(n_q, n_c, slices);
  if (part_rows < 0) return (int)part_rows;
  double* part = static_cast<double*>(work);
  float* qn = reinterpret_cast<float*>(part + part_rows * (1 + d));
  float* cn = qn + n_q;
  if (gram) {
    int rc = mde_row_sqnorm(n_q, nf, Q, qn, stream);
    if (rc == MDE_OK) rc = mde_row_sqnorm(n_c, nf, C, cn, stream);
    if (rc != MDE_OK) return rc;
  }
  PairWalk a;
  a.n_q = n_rows, a.n_c = n_c, a.nf = nf, a.mode = mode;
  a.Q = Q, a.qn = qn, a.C = C, a.cn = cn, a.Dm = Dm;
  a.d_scale = d_scale, a.d = d, a.XQ = XQ, a.XC = XC, a.kind = kind, a.S = MdeScalars{s0, s1, s2};
  a.s = s, a.part = part, a.rows = rows;
  a.wsrc = wsrc, a.wt = pair_weights(wsrc, p, W), a.st = mde_stream(stream);
  const int rc = pair_loss_walk<false>(a);
  return rc != MDE_OK ? rc : pair_loss_fold(a, joint ? pairs : (double)n_c, 1.0, loss, row_loss, row_grad);
}

extern "C" int mde_pair_loss_cross(int64_t n_q, int64_t n_c, int32_t nf, const float* Q, const float* C, int32_t mode,
                                   const float* Dm, float d_scale, int32_t d, const float* XQ, const float* XC,
                                   int32_t kind, float s0, float s1, float s2, int32_t slices, double* loss,
                                   float* grad, double* row_loss, void* work, void* stream) {
  return pair_loss_rect("mde_pair_loss_cross", true, n_q, n_c, nf, Q, C, mode, Dm, d_scale, d, XQ, XC, kind, s0, s1,
                        s2, slices, n_q, nullptr, PAIR_W_NONE, 0.0f, nullptr, (double)n_q * (double)n_c, loss,
                        row_loss, grad, work, stream);
}

// mde_pair_loss_cross with a weight per pair, W [n_q, n_c], and the count of the pairs that count passed in.
extern "C" int mde_pair_loss_cross_weighted(int64_t n_q, int64_t n_c, int32_t nf, const float* Q, const float* C,
                                            int32_t mode, const float* Dm, float d_scale, int32_t d, const float* XQ,
                                            const float* XC, int32_t kind, float s0, float s1, float s2,
                                            int32_t slices, int32_t wsource, float p, const float* W, double pairs,
                                            double* loss, float* grad, double* row_loss, void* work, void* stream) {
  return pair_loss_rect("mde_pair_loss_cross_weighted", true, n_q, n_c, nf, Q, C, mode, Dm, d_scale, d, XQ, XC, kind,
                        s0, s1, s2, slices, n_q, nullptr, wsource, p, W, pairs, loss, row_loss, grad, work, stream);
}

extern "C" int mde_pair_loss_cross_rows(int64_t n_q, int64_t n_c, int32_t nf, const float* Q, const float* C,
                                        int32_t mode, const float* Dm, float d_scale, int32_t d, const float* XQ,
                                        const float* XC, int32_t kind, float s0, float s1, float s2, int32_t slices,
                                        int64_t n_rows, const int32_t* rows, double* row_loss, float* row_grad,
                                        void* work, void* stream) {
  return pair_loss_rect("mde_pair_loss_cross_rows", false, n_q, n_c, nf, Q, C, mode, Dm, d_scale, d, XQ, XC, kind, s0,
                        s1, s2, slices, n_rows, rows, PAIR_W_NONE, 0.0f, nullptr, 0.0, nullptr, row_loss, row_grad,
                        work, stream);
}

// mde_pair_loss_cross_rows with a weight per pair; W [n_q, n_c] is read through the list as Dm is.  The divisor
// stays n_c (there is no `pairs`): the per-row solver's arithmetic does not change.
extern "C" int mde_pair_loss_cross_rows_weighted(int64_t n_q, int64_t n_c, int32_t nf, const float* Q, const float* C,
                                                 int32_t mode, const float* Dm, float d_scale, int32_t d,
                                                 const float* XQ, const float* XC, int32_t kind, float s0, float s1,
                                                 float s2, int32_t slices, int64_t n_rows, const int32_t* rows,
                                                 int32_t wsource, float p, const float* W, double* row_loss,
                                                 float* row_grad, void* work, void* stream) {
  return pair_loss_rect("mde_pair_loss_cross_rows_weighted", false, n_q, n_c, nf, Q, C, mode, Dm, d_scale, d, XQ, XC,
                        kind, s0, s1, s2, slices, n_rows, rows, wsource, p, W, 0.0, nullptr, row_loss, row_grad, work,
                        stream);
}

// ---------------------------------------------------------------------------------------------------------------------
// mde_pair_weights_check: what pymde_amd.dense has to know of a weight matrix before the walk may
// trust it, in ONE pass over W (and over Dm when there is one).  Workgroup (x, y) takes the 64x64 tiles (x, y),
// (x, y + gridDim.y), ... (at most PAIR_WC_SLICES workgroups share a row block, so a row's kept count costs that many
// integer atomics, not one per tile): wave w reads the 256-byte segments of the tile rows w, w + 4, ... (lane =
// column), and,
// for the square problem, the mirror tiles of W and Dm are staged in LDS first so that W[j][i] is read coalesced too.
// Integer counters only (ballot + popcount per wave, one integer atomic per wave and counter; the maxima as the bit
// patterns of non-negative floats, which order as unsigned integers): the results do not depend on the order.
#define PAIR_WC_COUNTS 5   // non-finite w | negative w | kept pairs | rows without a kept pair | kept with a bad D
#define PAIR_WC_SLICES 16  // workgroups per row block
#define PAIR_WC_TOPS 4     // max |W - W^T| | max |W| | max |Dm - Dm^T| over the kept | max Dm over the kept

__device__ __forceinline__ float pair_wave_max(float v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

template <bool SQUARE>
__global__ __launch_bounds__(MDE_BLOCK) void k_pair_weights_check(int n_q, int n_c, const float* __restrict__ W,
                                                                  const float* __restrict__ Dm,
                                                                  unsigned long long* __restrict__ counts,
                                                                  unsigned* __restrict__ tops,
                                                                  int32_t* __restrict__ row_kept) {
  __shared__ float tW[SQUARE ? PAIR_TILE : 1], tD[SQUARE ? PAIR_TILE : 1];   // the mirror tiles, [col][row]
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int64_t row0 = (int64_t)blockIdx.x * KNN_BM;
  const int64_t tiles_c = ((int64_t)n_c + KNN_BN - 1) / KNN_BN;
  unsigned long long c_bad = 0, c_neg = 0, c_kept = 0, c_badd = 0;   // the wave's counts: the same in every lane
  float m_asym = 0.0f, m_top = 0.0f, md_asym = 0.0f, md_top = 0.0f;
  int row_count[KNN_BM / 4];                                         // of the wave's rows w, w + 4, ...; likewise
#pragma unroll
  for (int q = 0; q < KNN_BM / 4; ++q) row_count[q] = 0;
  auto finite = [](float v) { return fabsf(v) <= PAIR_FLT_MAX; };
  for (int64_t ct = blockIdx.y; ct < tiles_c; ct += gridDim.y) {
    const int64_t col0 = ct * KNN_BN;
    if constexpr (SQUARE) {
      __syncthreads();                                          // the last tile's mirrors have been read
      const int64_t gc = row0 + lane < n_c ? row0 + lane : n_c - 1;
#pragma unroll
      for (int q = 0; q < KNN_BM / 4; ++q) {
        const int64_t gr = col0 + w + 4 * q < n_q ? col0 + w + 4 * q : n_q - 1;
        tW[(w + 4 * q) * (KNN_BN + 1) + lane] = W[gr * (int64_t)n_c + gc];
        if (Dm) tD[(w + 4 * q) * (KNN_BN + 1) + lane] = Dm[gr * (int64_t)n_c + gc];
      }
      __syncthreads();
    }
    const int64_t j = col0 + lane, gc = j < n_c ? j : n_c - 1;
#pragma unroll
    for (int q = 0; q < KNN_BM / 4; ++q) {
      const int rr = w + 4 * q;
      const int64_t i = row0 + rr, gr = i < n_q ? i : n_q - 1;
      const bool in = i < n_q && j < n_c && (!SQUARE || i != j);     // the diagonal of a square W is ignored
      const float a = W[gr * (int64_t)n_c + gc];
      const bool fin = finite(a), kept = in && a > 0.0f;
      c_bad += __popcll(__ballot(in && !fin));
      c_neg += __popcll(__ballot(in && a < 0.0f));
      c_kept += __popcll(__ballot(kept && (!SQUARE || i < j)));
      row_count[q] += __popcll(__ballot(kept));
      if constexpr (SQUARE) {
        const float diff = fabsf(a - tW[lane * (KNN_BN + 1) + rr]);
        if (in && fin) m_top = fmaxf(m_top, fabsf(a));
        if (in && fin && finite(diff)) m_asym = fmaxf(m_asym, diff);
      }
      if (Dm) {
        const float dv = Dm[gr * (int64_t)n_c + gc];
        const bool d_ok = dv >= 0.0f && finite(dv);
        c_badd += __popcll(__ballot(kept && !d_ok));
        if constexpr (SQUARE) {
          const float diff = fabsf(dv - tD[lane * (KNN_BN + 1) + rr]);
          if (kept && d_ok) md_top = fmaxf(md_top, dv);
          if (kept && d_ok && finite(diff)) md_asym = fmaxf(md_asym, diff);
        }
      }
    }
  }
  m_asym = pair_wave_max(m_asym), m_top = pair_wave_max(m_top);
  md_asym = pair_wave_max(md_asym), md_top = pair_wave_max(md_top);
  if (lane == 0) {
#pragma unroll
    for (int q = 0; q < KNN_BM / 4; ++q)
      if (row_count[q] > 0) atomicAdd(&row_kept[row0 + w + 4 * q], row_count[q]);   // (kept implies a row of W)
    if (c_bad) atomicAdd(&counts[0], c_bad);
    if (c_neg) atomicAdd(&counts[1], c_neg);
    if (c_kept) atomicAdd(&counts[2], c_kept);
    if (c_badd) atomicAdd(&counts[4], c_badd);
    if (SQUARE) {
      atomicMax(&tops[0], __float_as_uint(m_asym));
      atomicMax(&tops[1], __float_as_uint(m_top));
      atomicMax(&tops[2], __float_as_uint(md_asym));
      atomicMax(&tops[3], __float_as_uint(md_top));
    }
  }
}

// counts[3] = the number of rows whose kept count is zero
__global__ __launch_bounds__(MDE_BLOCK) void k_pair_weights_empty_rows(int64_t n_q,
                                                                       const int32_t* __restrict__ row_kept,
                                                                       unsigned long long* __restrict__ counts) {
  unsigned long long c = 0;
  // (whole waves: every lane of a wave runs the same number of rounds, so the ballot sees all of them)
  for (int64_t i0 = (int64_t)blockIdx.x * MDE_BLOCK; i0 < n_q; i0 += (int64_t)gridDim.x * MDE_BLOCK) {
    const int64_t i = i0 + threadIdx.x;
    c += __popcll(__ballot(i < n_q && row_kept[i < n_q ? i : n_q - 1] == 0));
  }
  if ((threadIdx.x & 63) == 0 && c) atomicAdd(&counts[3], c);
}

extern "C" int mde_pair_weights_check(int64_t n_q, int64_t n_c, int32_t square, const float* W, const float* Dm,
                                      int64_t* counts, float* tops, int32_t* row_kept, void* stream) {
  if (n_q < 1 || n_q >= ((int64_t)1 << 31) || n_c < 1 || n_c >= ((int64_t)1 << 31) || (square != 0 && square != 1) ||
      (square && n_q != n_c) || !W || !counts || !tops || !row_kept) {
    mde_set_error("mde_pair_weights_check: invalid arguments (1 <= n_q, n_c < 2^31, square 0 or 1 and then n_q == n_c, "
                  "non-null W / counts / tops / row_kept)");
    return MDE_E_INVALID;
  }
  hipStream_t st = mde_stream(stream);
  MDE_HIP(hipMemsetAsync(counts, 0, PAIR_WC_COUNTS * sizeof(int64_t), st));
  MDE_HIP(hipMemsetAsync(tops, 0, PAIR_WC_TOPS * sizeof(float), st));
  MDE_HIP(hipMemsetAsync(row_kept, 0, (size_t)n_q * sizeof(int32_t), st));
  const int64_t tiles_c = (n_c + KNN_BN - 1) / KNN_BN;
  const dim3 grid((unsigned)((n_q + KNN_BM - 1) / KNN_BM),
                  (unsigned)(tiles_c < PAIR_WC_SLICES ? tiles_c : PAIR_WC_SLICES));
  unsigned long long* c = reinterpret_cast<unsigned long long*>(counts);
  unsigned* t = reinterpret_cast<unsigned*>(tops);
  if (square)
    hipLaunchKernelGGL(k_pair_weights_check<true>, grid, dim3(MDE_BLOCK), 0, st, (int)n_q, (int)n_c, W, Dm, c, t,
                       row_kept);
  else
    hipLaunchKernelGGL(k_pair_weights_check<false>, grid, dim3(MDE_BLOCK), 0, st, (int)n_q, (int)n_c, W, Dm, c, t,
                       row_kept);
  MDE_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_pair_weights_empty_rows, dim3(mde_grid(n_q, MDE_BLOCK, 4096)), dim3(MDE_BLOCK), 0, st, n_q,
                     row_kept, c);
  MDE_LAUNCH_CHECK();
  return MDE_OK;
}

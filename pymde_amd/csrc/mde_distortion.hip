// mde_distortion.hip -- the hot kernel: fused forward + backward of the average distortion
//   E(X) = (1/p) sum_k f_k(||x_i - x_j||),   dE/dX
// [ref: pymde/average_distortion.py:62-106 `_AverageDistortion.forward/backward`] and the unfused
// fallback used for arbitrary Python callables: the entry points, the choice of the kernel, and the
// pipelined general-d kernel (k_fused_wide4p).  The other CSR kernels are units of their own:
// mde_fused_small.hip (d <= 4), mde_fused_wide.hip (general d, unpipelined); what they share is in
// mde_fused.h.  The edge-order evaluators are in mde_edge_eval.hip.
//
// Execution model (CDNA4, wave64): the plan is a symmetrised incidence CSR.  A group of G
// lanes owns one vertex row v at a time; the lanes stride over the row's half-edges
// (coalesced int32 neighbour + fp32 parameter streams), gather x_u (the only random access,
// served by L2 / Infinity Cache: the table is n*d*4 bytes), evaluate f and f'/d in registers,
// accumulate g (x_v - x_u) and reduce across the G lanes with xor butterflies (DPP).  There
// are no atomics and no [p, d] temporaries; the reference materialises five of them.
// Each edge is visited from both endpoints, so its loss term is counted with weight 1/2.
#include "mde_fused.h"

int mde_ring_try(mde_plan* plan, const float* X, int d, const mde_func* f, float grad_scale,
                  float* grad, float inv_p, hipStream_t st, int* nblocks, float* loss_out,
                  double loss_scale);

// ---------------------------------------------------------------- general-d fused kernel, pipelined form (round 6)
// Rows of ncol = ceil(d / 4) float4 columns, GL lanes x K4 float4s per half-edge with GL * (K4 - 1) < ncol <= GL * K4 (GL = 1 .. 32,
// K4 = 2 .. 4: every d = 5 .. 512; d = 128 is <8, 4>).  Same lane layout as k_fused_wide<wide_f4, GL, K4>
// (GL lanes share a half-edge, 64 / GL half-edges per wave step); what changes is everything around the arithmetic:
//  * the row gathers of step s + 1 are in flight while step s is evaluated (two register buffers, the loop unrolled
//    by two; the meta words -- neighbour id, parameters -- run two steps ahead, the next row's first meta words and
//    row pointers a whole row ahead): a wave never sits behind its own loads with nothing issued;
//  * |x_v - x_u|^2 with packed fp32 math (v_pk_add_f32 / v_pk_fma_f32: 16 instructions instead of 32), the sum over
//    the lanes of a group with DPP adds instead of LDS permutes;
//  * the E partial gradient rows of a wave are added by a TRANSPOSING reduction (v_permlane32_swap / v_permlane16_swap:
//    one swap + one add folds two registers into one whose halves hold the two sums): 12 swaps + 16 adds for the 16
//    floats of a lane instead of 48 LDS permutes + 48 adds, and every lane ends up owning one float4 of the row;
//  * XCD-aware row order: the rows are cut into chunks of 2^chunk_log rows, chunk c belongs to XCD c % 8 (block b runs
//    on XCD b % 8), and the waves of an XCD walk ITS chunks in order -- the rows an XCD works on at any moment are a
//    band of ~1000 consecutive rows, so on a graph with locality (neighbours within a window of the vertex order)
//    the band's neighbours stay in that XCD's 4 MB L2 instead of being fetched by all eight.
// Summation order inside a row: fixed by the row's own half-edge positions (steps of E from the row's first entry),
// so a vertex-range shard produces the bits of the single process.
typedef float wide_f4 __attribute__((ext_vector_type(4)));
typedef float wide_f2 __attribute__((ext_vector_type(2)));
typedef unsigned wide_u2 __attribute__((ext_vector_type(2)));
typedef wide_f4 wide_f4u __attribute__((aligned(4)));  // a float4 at any float of a row (unaligned access mode)
template <int GL>
__device__ __forceinline__ float wide_group_sum(float v) {
  static_assert(GL == 1 || GL == 2 || GL == 4 || GL == 8 || GL == 16 || GL == 32, "group widths of the pipelined kernel");
  if constexpr (GL >= 2) v += __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0xB1, 0xF, 0xF, true));   // quad_perm [1,0,3,2]
  if constexpr (GL >= 4) v += __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0x4E, 0xF, 0xF, true));   // quad_perm [2,3,0,1]
  if constexpr (GL >= 8) v += __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0x141, 0xF, 0xF, true));  // row_half_mirror
  if constexpr (GL >= 16) v += __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0x140, 0xF, 0xF, true));  // row_mirror
  if constexpr (GL >= 32) v += __shfl_xor(v, 16, 64);
  return v;
}
// a <- the xor-32 sums of a in lanes 0..31 and of b in lanes 32..63
__device__ __forceinline__ float wide_fold32(float a, float b) {
  const wide_u2 r = __builtin_amdgcn_permlane32_swap(__float_as_uint(a), __float_as_uint(b), false, false);
  return __uint_as_float(r.x) + __uint_as_float(r.y);
}
// a <- the xor-16 sums of a in rows 0, 2 and of b in rows 1, 3 (rows of 16 lanes)
__device__ __forceinline__ float wide_fold16(float a, float b) {
  const wide_u2 r = __builtin_amdgcn_permlane16_swap(__float_as_uint(a), __float_as_uint(b), false, false);
  return __uint_as_float(r.x) + __uint_as_float(r.y);
}
template <int GL, int K4, bool INDIRECT, class Fn>
__global__ __launch_bounds__(MDE_BLOCK) void k_fused_wide4p(
    int nrows, int row_lo, int d, int chunk_log, const int32_t* __restrict__ order, const int32_t* __restrict__ rowptr,
    const int32_t* __restrict__ nbr,
    const int32_t* __restrict__ eid, const float* __restrict__ a0, const float* __restrict__ a1, int a0_scalar,
    int a1_scalar, const float* __restrict__ X, float* __restrict__ grad, double* __restrict__ loss_partials,
    Fn fn, float inv_p, float grad_scale) {
  __shared__ double smem[8];
  constexpr int E = 64 / GL;   // half-edges per wave step
  constexpr int WPB = MDE_BLOCK / 64;
  const int lane = threadIdx.x & 63;
  const int lig = lane & (GL - 1);
  const int sub = lane / GL;
  const int xcd = blockIdx.x & 7;
  const int wpx = (gridDim.x >> 3) * WPB;  // waves per XCD (the grid is a multiple of 8 blocks)
  const int cmask = (1 << chunk_log) - 1;
  float loss = 0.0f;
  const EdgeParams<INDIRECT> params(eid, a0, a1, a0_scalar, a1_scalar);
  // Columns: float4 number c covers the floats [4 c, 4 c + 4) of a row, except the row's LAST column when d is not a
  // multiple of 4: that one covers [d - 4, d) -- shifted back so that it stays inside the row -- and only its last
  // d % 4 components count.  Rows start at multiples of d floats, so the 16-byte accesses are 4-byte aligned only
  // (the hardware's unaligned access mode; wide_f4u below).  A lane's columns are lig + j GL, j < K4, with
  // GL (K4 - 1) < ncol <= GL K4: only its last column can be the row's last, or lie behind it (then it loads the
  // row's last column again and every component is masked).
  const int ncol = (d + 3) >> 2, rem = d & 3;
  const int c_mine = lig + (K4 - 1) * GL;
  const bool tail_dead = c_mine >= ncol;
  const bool tail_part = rem != 0 && c_mine == ncol - 1;
  const int off_tail = (tail_dead || tail_part) ? (rem ? d - 4 : 4 * (ncol - 1)) : 4 * c_mine;
  const int first_kept = tail_dead ? 4 : (tail_part ? 4 - rem : 0);  // components below it are masked
  const wide_f2 keep_lo = {first_kept <= 0 ? 1.0f : 0.0f, first_kept <= 1 ? 1.0f : 0.0f};
  const wide_f2 keep_hi = {first_kept <= 2 ? 1.0f : 0.0f, first_kept <= 3 ? 1.0f : 0.0f};

  // position of the i-th row of this XCD's sequence in the processing order, or -1 behind the end; the row at a
  // position is order[position] when the plan carries a processing order (mde_plan_row_order), the position itself
  // otherwise
  auto pos_of = [&](int i) __attribute__((always_inline)) -> int {
    const int q = ((((i >> chunk_log) << 3) + xcd) << chunk_log) + (i & cmask);
    return q < nrows ? q : -1;
  };
  auto row_at = [&](int q) __attribute__((always_inline)) -> int {
    return (q >= 0 && order) ? order[q] : q;
  };
  auto row_of = [&](int i) __attribute__((always_inline)) -> int { return row_at(pos_of(i)); };
  struct Meta {
    int u;
    float p0, p1;
  };
  auto load_meta = [&](int h, int end) __attribute__((always_inline)) -> Meta {
    Meta m;
    int hh = h < end ? h : end - 1;
    hh = hh < 0 ? 0 : hh;
    m.u = nbr[hh];
    params.load(hh, m.p0, m.p1);
    return m;
  };
  auto load_rows = [&](wide_f4 (&x)[K4], int64_t u) __attribute__((always_inline)) {
    const float* p = X + u * d;
#pragma unroll
    for (int j = 0; j < K4 - 1; ++j) x[j] = *reinterpret_cast<const wide_f4u*>(p + 4 * (lig + j * GL));
    x[K4 - 1] = *reinterpret_cast<const wide_f4u*>(p + off_tail);
  };
  // the lane's column j of gradient row v (j >= K4, or a column behind the row's end: nothing; the row's last column
  // when d is not a multiple of 4: its last d % 4 components, one by one -- the float4 would overlap the column before)
  auto store_col = [&](int64_t v, int j, wide_f4 val) __attribute__((always_inline)) {
    float* g = grad + v * d;
    if (j < K4 - 1) {
      *reinterpret_cast<wide_f4u*>(g + 4 * (lig + j * GL)) = val;
    } else if (j == K4 - 1 && !tail_dead) {
      if (!tail_part) {
        *reinterpret_cast<wide_f4u*>(g + off_tail) = val;
      } else {
        if (rem >= 3) g[d - 3] = val.y;
        if (rem >= 2) g[d - 2] = val.z;
        g[d - 1] = val.w;
      }
    }
  };

  int i = __builtin_amdgcn_readfirstlane((int)(blockIdx.x >> 3) * WPB + (int)(threadIdx.x >> 6));
  int r = row_of(i);
  int beg = 0, end = 0, r_n = -1, beg_n = 0, end_n = 0, r_nn = -1, beg_nn = 0, end_nn = 0, r_n3 = -1;
  Meta mA = {0, 0.f, 0.f}, mB = mA, m0n = mA, m1n = mA;
  wide_f4 xv[K4], bufA[K4], bufB[K4];
  if (r >= 0) {
    beg = rowptr[r];
    end = rowptr[r + 1];
    mA = load_meta(beg + sub, end);
    mB = load_meta(beg + E + sub, end);
    r_n = row_of(i + wpx);
    if (r_n >= 0) {
      beg_n = rowptr[r_n];
      end_n = rowptr[r_n + 1];
      m0n = load_meta(beg_n + sub, end_n);
      m1n = load_meta(beg_n + E + sub, end_n);
      r_nn = row_of(i + 2 * wpx);
      if (r_nn >= 0) {
        beg_nn = rowptr[r_nn];
        end_nn = rowptr[r_nn + 1];
        r_n3 = row_of(i + 3 * wpx);
      }
    }
    load_rows(xv, (int64_t)row_lo + r);
    load_rows(bufA, mA.u);
#pragma unroll
    for (int j = 0; j < K4; ++j) {
      xv[j] = -xv[j];
      asm volatile("" : "+v"(xv[j]));
    }
  }
  // The wave's rows form ONE software pipeline: at the top of a row bufA already holds (or is about to receive) the
  // gathers of the row's first step -- issued by the previous row's last step --, its first two meta words are in
  // registers, and so are the row pointers and the first two meta words of the row after it and the row pointers of
  // the row after that.
  while (r >= 0) {
    const int64_t v = (int64_t)row_lo + r;
    // (an empty row runs one step with every lane dead -- clamped positions, nothing added: no special case for the
    // compiler's load bookkeeping to be conservative about)
    const int nsteps = end > beg ? (end - beg + E - 1) / E : 1;
    // three rows ahead: the row pointers; four rows ahead: which row that is (scalar loads; they are back by the
    // time the row's end rotates them in)
    i += wpx;
    int beg_n3 = 0, end_n3 = 0;
    if (r_n3 >= 0) {
      beg_n3 = rowptr[r_n3];
      end_n3 = rowptr[r_n3 + 1];
    }
    const int r_n4 = r_n3 >= 0 ? row_of(i + 3 * wpx) : -1;
    // the next row's x_v, a row ahead like everything else of it; the first two meta words of the row after next
    // (loaded here, not at the row's end: the copy into the registers the next trip reads would otherwise wait for
    // loads that have only just gone out; behind the last row beg_nn = end_nn = 0: position 0)
    wide_f4 xvn[K4];
    load_rows(xvn, (int64_t)row_lo + (r_n >= 0 ? r_n : r));
    const Meta m0nn = load_meta(beg_nn + sub, end_nn);
    const Meta m1nn = load_meta(beg_nn + E + sub, end_nn);
    wide_f2 acc[2 * K4];
#pragma unroll
    for (int j = 0; j < 2 * K4; ++j) acc[j] = wide_f2{0.f, 0.f};

    // one step: x holds the gathered rows of E half-edges (one per group of GL lanes).
    // (xv holds -x_v: dd = x_u - x_v is then a packed ADD -- hipcc has no packed form for a subtraction of two
    // register pairs --, the accumulators collect -g (x_v - x_u) and the sign goes into the scale of the final
    // store: negation is exact, every intermediate is the negative of the plain form's, bit for bit)
    auto step = [&](wide_f4 (&x)[K4], const Meta& m, bool live) __attribute__((always_inline)) {
      __builtin_amdgcn_sched_barrier(0);
      wide_f2 dd[2 * K4], s2 = {0.f, 0.f}, t2 = {0.f, 0.f};
#pragma unroll
      for (int j = 0; j < K4; ++j) {
        dd[2 * j] = wide_f2{xv[j].x, xv[j].y} + wide_f2{x[j].x, x[j].y};
        dd[2 * j + 1] = wide_f2{xv[j].z, xv[j].w} + wide_f2{x[j].z, x[j].w};
        if (j == K4 - 1) {
          // (x 1 where the row is exactly GL x K4 float4s wide: exact)
          dd[2 * j] *= keep_lo;
          dd[2 * j + 1] *= keep_hi;
        }
        s2 = dd[2 * j] * dd[2 * j] + s2;
        t2 = dd[2 * j + 1] * dd[2 * j + 1] + t2;
      }
      s2 += t2;
      const float ss = wide_group_sum<GL>(s2.x + s2.y);
      float f, gd;
      fn.eval(ss, m.p0, m.p1, f, gd);
      float g = mde_fix_g(gd * inv_p);
      if (!live) {
        g = 0.0f;
        f = 0.0f;
      }
      if (lig == 0) loss += f;
      const wide_f2 g2 = {g, g};
#pragma unroll
      for (int j = 0; j < 2 * K4; ++j) acc[j] = g2 * dd[j] + acc[j];
      __builtin_amdgcn_sched_barrier(0);
    };

    int h = beg;
    int k = 0;
    do {
      // (every load below is issued on every trip -- clamped positions behind the row's end --: a branch around a
      // gather makes the compiler's vmcnt bookkeeping wait for EVERYTHING at the next use.  Meta words go out before
      // the gathers that follow them: vmcnt counts in order -- both of a trip's at its top, so that the rotation at
      // its bottom finds them behind gathers that step B has already waited for.)
      const Meta mC = load_meta(h + 2 * E + sub, end);
      const Meta mD = load_meta(h + 3 * E + sub, end);
      load_rows(bufB, mB.u);
      step(bufA, mA, h + sub < end);
      const bool last = k + 2 >= nsteps;
      load_rows(bufA, last ? m0n.u : mC.u);   // behind the row's last step: the NEXT row's first gathers
      if (k + 1 < nsteps) step(bufB, mB, h + E + sub < end);
      mA = mC;
      mB = mD;
      h += 2 * E;
      k += 2;
    } while (k < nsteps);
    mA = m0n;
    mB = m1n;
    m0n = m0nn;
    m1n = m1nn;
    if (grad) {
      // transposing reduction over the E groups of the wave (lanes with equal lig)
      const float gsc = -grad_scale;
      float e[16];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        e[2 * j] = j < 2 * K4 ? acc[j < 2 * K4 ? j : 0].x : 0.0f;
        e[2 * j + 1] = j < 2 * K4 ? acc[j < 2 * K4 ? j : 0].y : 0.0f;
      }
      // xor 32: element k with k + 8 -> lanes < 32 keep k, lanes >= 32 keep k + 8
      float e8[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) e8[k] = wide_fold32(e[k], e[k + 8]);
      if constexpr (GL == 32) {
        // lane (b5, lig): float4s 2 b5 and 2 b5 + 1 of the row
        const int j0 = (lane >> 5) * 2;
        store_col(v, j0, wide_f4{e8[0], e8[1], e8[2], e8[3]} * gsc);
        store_col(v, j0 + 1, wide_f4{e8[4], e8[5], e8[6], e8[7]} * gsc);
      } else {
        // xor 16: element k with k + 4 -> rows 0, 2 keep k, rows 1, 3 keep k + 4
        float e4[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) e4[k] = wide_fold16(e8[k], e8[k + 4]);
        if constexpr (GL <= 8) {
#pragma unroll
          for (int k = 0; k < 4; ++k)
            e4[k] += __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(e4[k]), 0x128, 0xF, 0xF, true));  // row_ror:8
        }
        if constexpr (GL <= 4) {
          // (period 8 now: one more rotation by 4 adds the other residue)
#pragma unroll
          for (int k = 0; k < 4; ++k)
            e4[k] += __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(e4[k]), 0x124, 0xF, 0xF, true));  // row_ror:4
        }
        if constexpr (GL <= 2) {
#pragma unroll
          for (int k = 0; k < 4; ++k)
            e4[k] += __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(e4[k]), 0x4E, 0xF, 0xF, true));   // quad_perm [2,3,0,1]
        }
        if constexpr (GL == 1) {
#pragma unroll
          for (int k = 0; k < 4; ++k)
            e4[k] += __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(e4[k]), 0xB1, 0xF, 0xF, true));   // quad_perm [1,0,3,2]
        }
        // lane (b5, b4, .): float4 number b4 + 2 b5 of the row; below GL = 16 the lanes with (lane & 15) >= GL hold
        // copies
        const int j = (lane >> 4) & 3;
        if ((lane & 15) < GL) store_col(v, j, wide_f4{e4[0], e4[1], e4[2], e4[3]} * gsc);
      }
    }
    // xv <- -x_v of the next row (see step()); the asm keeps hipcc from folding the sign back into a subtraction
#pragma unroll
    for (int j = 0; j < K4; ++j) {
      xv[j] = -xvn[j];
      asm volatile("" : "+v"(xv[j]));
    }
    r = r_n;
    beg = beg_n;
    end = end_n;
    r_n = r_nn;
    beg_n = beg_nn;
    end_n = end_nn;
    r_nn = r_n3;
    beg_nn = beg_n3;
    end_nn = end_n3;
    r_n3 = r_n4;
  }
  const double bs = mde_block_sum((double)loss, smem);
  if (threadIdx.x == 0) loss_partials[blockIdx.x] = bs;
}

// loss = scale * sum(partials[0..nb)) in a fixed order (one block)
__global__ void k_finalize_loss(double* __restrict__ partials, int nb, double scale,
                                float* __restrict__ loss_out) {
  __shared__ double smem[8];
  double s = 0.0;
  for (int i = threadIdx.x; i < nb; i += blockDim.x) s += partials[i];
  const double t = mde_block_sum(s, smem);
  if (threadIdx.x == 0) {
    *loss_out = (float)(t * scale);
    partials[MDE_PARTIALS_LOSS_D] = t * scale;
  }
}

template <int GL, int K4, bool IND, class Fn>
static int launch_wide4p(FusedArgs& A, const Fn& fn) {
  const mde_plan* P = A.plan;
  const int nrows = fused_row_grid(A, 64);
  A.nblocks = (A.nblocks + 7) & ~7;  // (the row order is per XCD: block b runs on XCD b % 8)
  // chunks of up to 2048 rows, at least 64 chunks (8 per XCD) so that short row ranges still fill every XCD
  int chunk_log = env_int("MDE_WIDE_CHUNK", 11);
  while (chunk_log > 0 && ((int64_t)64 << chunk_log) > nrows) --chunk_log;
  // graphs whose locality is hidden by the vertex numbering: a breadth-first processing order, built once per plan
  // and kept only when it brings the endpoints of an edge closer together (mde_plan.hip: mde_plan_row_order)
  const int order_env = env_int("MDE_ROW_ORDER", 1);
  if (order_env && P->order_state == 0) {
    const int rc = mde_plan_row_order(const_cast<mde_plan*>(P), order_env, A.st, nullptr);
    if (rc != MDE_OK) return rc;
  }
  hipLaunchKernelGGL((k_fused_wide4p<GL, K4, IND, Fn>), dim3(A.nblocks), dim3(MDE_BLOCK), 0, A.st, nrows,
                     (int)mde_plan_row_lo(P), A.d, chunk_log, P->order, mde_plan_rowptr(P), mde_plan_nbr(P), mde_plan_eid(P),
                     A.a0, A.a1, A.a0_scalar, A.a1_scalar, A.X, A.grad, A.partials, fn, A.inv_p, A.grad_scale);
  MDE_LAUNCH_CHECK();
  return MDE_OK;
}
// GL lanes x K4 float4s cover the row of d4 = ceil(d / 4) float4 columns: GL * (K4 - 1) < d4 <= GL * K4 (the lanes
// of the last float4 that lie behind the row's end are masked)
template <bool IND, class Fn>
static int launch_wide4p_d(FusedArgs& A, const Fn& fn) {
  const int d4 = (A.d + 3) >> 2;
  if (d4 == 2) return launch_wide4p<1, 2, IND, Fn>(A, fn);
  if (d4 == 3) return launch_wide4p<1, 3, IND, Fn>(A, fn);
  if (d4 == 4) return launch_wide4p<1, 4, IND, Fn>(A, fn);
  if (d4 <= 6) return launch_wide4p<2, 3, IND, Fn>(A, fn);
  if (d4 <= 8) return launch_wide4p<2, 4, IND, Fn>(A, fn);
  if (d4 <= 12) return launch_wide4p<4, 3, IND, Fn>(A, fn);
  if (d4 <= 16) return launch_wide4p<4, 4, IND, Fn>(A, fn);
  if (d4 <= 24) return launch_wide4p<8, 3, IND, Fn>(A, fn);
  if (d4 <= 32) return launch_wide4p<8, 4, IND, Fn>(A, fn);
  if (d4 <= 48) return launch_wide4p<16, 3, IND, Fn>(A, fn);
  if (d4 <= 64) return launch_wide4p<16, 4, IND, Fn>(A, fn);
  if (d4 <= 96) return launch_wide4p<32, 3, IND, Fn>(A, fn);
  return launch_wide4p<32, 4, IND, Fn>(A, fn);
}

// Which kernel: d <= 4 the small-d unit; every d = 5 .. 512 the pipelined kernel, whose 16-byte accesses start at
// any float of a row (4-byte aligned; the hardware's unaligned access mode), so d need not be a multiple of 4;
// wider rows, and everything with MDE_WIDE_P=0, the unpipelined kernel.
enum { KERNEL_SMALL, KERNEL_WIDE4P, KERNEL_WIDE };
static int pick_kernel(int d) {
  if (d <= 4) return KERNEL_SMALL;
  return (d <= 512 && env_int("MDE_WIDE_P", 1)) ? KERNEL_WIDE4P : KERNEL_WIDE;
}
static int dispatch_fused(FusedArgs& A, const mde_func* f) {
  switch (pick_kernel(A.d)) {
    case KERNEL_SMALL: return mde_fused_small(A, f);
    case KERNEL_WIDE: return mde_fused_wide(A, f);
  }
  const MdeFuncArgs a = func_args(f);
  if (func_is_log1p15(f)) return launch_wide4p_d<false>(A, FnSingle<MDE_F_LOG1P, 2>{a});
  return launch_wide4p_d<false>(A, FnRuntime{a});
}
static int dispatch_unfused(FusedArgs& A, mde_unfused which) {
  switch (pick_kernel(A.d)) {
    case KERNEL_SMALL: return mde_fused_small_unfused(A, which);
    case KERNEL_WIDE: return mde_fused_wide_unfused(A, which);
  }
  if (which == MDE_UNFUSED_SCATTER) return launch_wide4p_d<true>(A, FnScatter{});
  return launch_wide4p_d<true>(A, FnDistBackward{});
}

int mde_check_func(const mde_func* f) {
  if (!f || !mde_kind_valid(f->kind) || (f->kind_neg != MDE_F_NONE && !mde_kind_valid(f->kind_neg))) {
    mde_set_error("unknown distortion function kind");
    return MDE_E_UNSUPPORTED;
  }
  if (!f->a0) {
    mde_set_error("distortion function has no per-edge parameter array");
    return MDE_E_INVALID;
  }
  const bool needs_a1 = f->kind == MDE_F_L_WEIGHTED_QUADRATIC || f->kind == MDE_F_L_WEIGHTED_POWER ||
                        f->kind_neg == MDE_F_L_WEIGHTED_QUADRATIC ||
                        f->kind_neg == MDE_F_L_WEIGHTED_POWER;
  if (needs_a1 && !f->a1) {
    mde_set_error("weighted loss needs the second per-edge array (a1)");
    return MDE_E_INVALID;
  }
  return MDE_OK;
}

extern "C" int mde_average_distortion(mde_plan* plan, const float* X, int32_t d, const mde_func* f,
                                      float grad_scale, float* grad, float* loss_out, void* stream) {
  if (!plan || !X || d <= 0 || !loss_out) return MDE_E_INVALID;
  int rc = mde_check_func(f);
  if (rc != MDE_OK) return rc;
  const int64_t p = mde_plan_p(plan);
  FusedArgs A(plan, X, d, f->a0, f->a1, f->a0_scalar, f->a1_scalar, grad, p > 0 ? (float)(1.0 / (double)p) : 0.0f,
              grad_scale, stream);
  // every edge is seen from both endpoints: weight 1/2; mean over p edges
  const double scale = p > 0 ? 0.5 / (double)p : 0.0;
  if (f->layout == 1) {
    // parameters are in LDS-ring order: the LDS-resident kernel (mde_ring.hip), which also
    // reduces the loss (last workgroup to arrive)
    rc = mde_ring_try(plan, X, d, f, grad_scale, grad, A.inv_p, A.st, &A.nblocks, loss_out, scale);
    if (rc == 0) {
      mde_set_error("mde_func.layout = 1 but the plan has no LDS-ring layout for d = %d", d);
      return MDE_E_INVALID;
    }
    return rc < 0 ? rc : MDE_OK;
  }
  A.loss_out = loss_out;
  A.loss_scale = scale;
  rc = dispatch_fused(A, f);
  if (rc != MDE_OK) return rc;
  if (!A.loss_done) {
    hipLaunchKernelGGL(k_finalize_loss, dim3(1), dim3(MDE_BLOCK), 0, A.st, A.partials, A.nblocks, scale,
                       loss_out);
    MDE_LAUNCH_CHECK();
  }
  return MDE_OK;
}

extern "C" int mde_scatter(const mde_plan* plan, const float* X, int32_t d, const float* gnorm,
                           const float* dist, float scale, float* grad, void* stream) {
  if (!plan || !X || d <= 0 || !gnorm || !dist || !grad) return MDE_E_INVALID;
  FusedArgs A(plan, X, d, gnorm, dist, 0, 0, grad, 1.0f, scale, stream);
  return dispatch_unfused(A, MDE_UNFUSED_SCATTER);
}

extern "C" int mde_distances_backward(const mde_plan* plan, const float* X, int32_t d,
                                      const float* gout, float* grad, void* stream) {
  if (!plan || !X || d <= 0 || !gout || !grad) return MDE_E_INVALID;
  FusedArgs A(plan, X, d, gout, gout, 0, 0, grad, 1.0f, 1.0f, stream);
  return dispatch_unfused(A, MDE_UNFUSED_DIST_BACKWARD);
}

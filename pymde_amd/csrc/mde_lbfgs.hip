// mde_lbfgs.hip -- the device-resident L-BFGS memory: history update and two-loop recursion with every
// decision taken on the device, in one launch (small vectors), four launches, or two halves for a
// row-sharded solve (the other solver units: mde_solver.h).
//   [ref: pymde/lbfgs.py:461-530]
// All reductions are two-stage (block partials in double, one fixed-order final pass): no
// atomics, bitwise reproducible.
#include "mde_solver.h"

#include <algorithm>
#include <atomic>
#include <cmath>

// ---------------------------------------------------------------- L-BFGS memory
#define MDE_LB_GROUP 8
#define MDE_LB_NVAL (4 + 5 * MDE_LB_GROUP)

// Device-resident bookkeeping of mde_lbfgs_dev_step: the Gram matrices of the stored pairs, the
// slot permutation and the direction coefficients never visit the host.
#define MDE_LB_MAX 63
#define MDE_LB_LD 64
struct LbDev {
  int count;                  // stored pairs
  int accepted;               // 1: the last staged pair was stored (y.s > 1e-10, lbfgs.py:472)
  int order[MDE_LB_LD];       // permutation of the history+1 slots: [0, count) oldest first, [count] = spare
  double H;                   // y.s / y.y of the newest pair (lbfgs.py:486)
  double SY[MDE_LB_LD * MDE_LB_LD];  // SY[i][j] = s_i . y_j
  double YY[MDE_LB_LD * MDE_LB_LD];  // YY[i][j] = y_i . y_j
  float c_g;                  // d = c_g g + sum_j cs[j] s_j + cy[j] y_j
  float cs[MDE_LB_LD];
  float cy[MDE_LB_LD];
};

struct mde_lbfgs {
  int64_t N = 0;
  int history = 0;
  float* buf = nullptr;  // 2 (history+1) N floats: slot k holds s_k, then y_k
  struct LbDev* dev = nullptr;  // device-resident bookkeeping of the step
};

extern "C" int mde_lbfgs_create(int64_t N, int32_t history, mde_lbfgs** out) {
  if (!out || N <= 0 || history <= 0 || history > 63) return MDE_E_INVALID;
  mde_lbfgs* o = new mde_lbfgs();
  o->N = N;
  o->history = history;
  hipError_t e = hipMalloc(&o->buf, sizeof(float) * 2 * (size_t)(history + 1) * (size_t)N);
  if (e != hipSuccess) {
    delete o;
    return mde_hip_fail(e, "hipMalloc(lbfgs history)", __FILE__, __LINE__);
  }
  e = hipMalloc(&o->dev, sizeof(LbDev));
  if (e != hipSuccess) {
    (void)hipFree(o->buf);
    delete o;
    return mde_hip_fail(e, "hipMalloc(lbfgs device state)", __FILE__, __LINE__);
  }
  *out = o;
  return MDE_OK;
}
extern "C" int mde_lbfgs_destroy(mde_lbfgs* o) {
  if (!o) return MDE_OK;
  if (o->buf) (void)hipFree(o->buf);
  if (o->dev) (void)hipFree(o->dev);
  delete o;
  return MDE_OK;
}

// ---------------------------------------------------------------- device-driven step
// The history update and the two-loop recursion with every decision taken on the device: the
// stage kernel finds its slots through LbDev, k_lbfgs_direction folds the staged dots into the Gram
// matrices (accept / drop oldest, lbfgs.py:472-486) and runs the recursion in coefficient form
// (lbfgs.py:490-507), the combine kernel reads the coefficients from LbDev.  No host read-back.
__global__ void k_lbfgs_dev_reset(LbDev* __restrict__ dv, int history) {
  const int t = threadIdx.x;
  if (t <= history) dv->order[t] = t;
  if (t == 0) {
    dv->count = 0;
    dv->accepted = 0;
    dv->H = 1.0;
    dv->c_g = -1.0f;
  }
}

// Sums over the 64 lanes of NV values at once: lane q < NV returns the total of val[q].  A butterfly
// in which every lane keeps half of its values per step (63 shuffles for up to 64 values; NV
// separate wave sums are 6 NV of them, and behind a run-time `q < nval` each is a serial chain of six
// cross-lane latencies -- 15 us of the 28 the staging kernel took at N = 140k).
template <int NV>
__device__ __forceinline__ double lb_transpose_sum(const double (&val)[NV]) {
  static_assert(NV <= 64, "one value per lane at most");
  double a[64];
#pragma unroll
  for (int k = 0; k < 64; ++k) a[k] = k < NV ? val[k] : 0.0;
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const bool hi = (lane & o) != 0;
#pragma unroll
    for (int k = 0; k < o; ++k) {
      if (k >= NV) continue;  // both halves are zero in every lane
      const double keep = hi ? a[k + o] : a[k];
      const double send = hi ? a[k] : a[k + o];
      a[k] = keep + __shfl_xor(send, o, 64);
    }
  }
  return a[0];
}

// The staging pass of the device-driven step over the elements i = b * MDE_BLOCK + thread (+ k nb
// MDE_BLOCK): the new pair y = g - g_prev, s = t d is written to the spare slot, g_prev <- g, and the
// workgroup's share of every dot product the history update needs goes to partial[row * nb + b]
// (rows 0..3: y*.s*, y*.y*, s*.g, y*.g; 4 + 5 j + k: pair j: s_j.y*, y_j.y*, s*.y_j, s_j.g, y_j.g),
// G stored pairs per pass (8; 12 when the history is 9..12 pairs: one pass instead of two, whose second
// would read the vectors again for the last few pairs).  PUBLISH: relaxed device-scope stores (read again
// inside the launch).
template <bool PUBLISH, int G = MDE_LB_GROUP>
__device__ __forceinline__ void lb_stage_phase(int64_t N, const float* __restrict__ g, float* __restrict__ g_prev,
                                               const float* __restrict__ d, float t, float* __restrict__ buf,
                                               const LbDev* __restrict__ dv, double* __restrict__ partial,
                                               double (*sm)[4 + 5 * G]) {
  constexpr int NVAL = 4 + 5 * G;
  const int count = dv->count;
  const int spare = dv->order[count];
  float* s_new = buf + (int64_t)(2 * spare) * N;
  float* y_new = buf + (int64_t)(2 * spare + 1) * N;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int nb = gridDim.x, b = blockIdx.x;
  for (int done = 0; done == 0 || done < count; done += G) {
    const bool first = done == 0;
    int pc = count - done;
    if (pc > G) pc = G;
    const float* ps[G];
    const float* py[G];
#pragma unroll
    for (int j = 0; j < G; ++j) {
      const int slot = (j < pc) ? dv->order[done + j] : spare;
      ps[j] = buf + (int64_t)(2 * slot) * N;
      py[j] = buf + (int64_t)(2 * slot + 1) * N;
    }
    double val[NVAL];
#pragma unroll
    for (int q = 0; q < NVAL; ++q) val[q] = 0.0;
    for (int64_t i = (int64_t)b * MDE_BLOCK + threadIdx.x; i < N; i += (int64_t)nb * MDE_BLOCK) {
      const float gv = g[i];
      float yv, sv;
      if (first) {
        yv = gv - g_prev[i];
        sv = t * d[i];
        y_new[i] = yv;
        s_new[i] = sv;
        g_prev[i] = gv;
        val[0] = fma((double)yv, (double)sv, val[0]);
        val[1] = fma((double)yv, (double)yv, val[1]);
        val[2] = fma((double)sv, (double)gv, val[2]);
        val[3] = fma((double)yv, (double)gv, val[3]);
      } else {
        yv = y_new[i];
        sv = s_new[i];
      }
      // all sixteen loads before the first use (slots beyond pc alias the spare pair: valid memory,
      // their sums are never written) -- a branch per pair would serialise sixteen memory latencies
      float sj[G], yj[G];
#pragma unroll
      for (int j = 0; j < G; ++j) {
        sj[j] = ps[j][i];
        yj[j] = py[j][i];
      }
#pragma unroll
      for (int j = 0; j < G; ++j) {
        const double sd = sj[j], yd = yj[j];
        val[4 + 5 * j + 0] = fma(sd, (double)yv, val[4 + 5 * j + 0]);  // s_j . y*
        val[4 + 5 * j + 1] = fma(yd, (double)yv, val[4 + 5 * j + 1]);  // y_j . y*
        val[4 + 5 * j + 2] = fma((double)sv, yd, val[4 + 5 * j + 2]);  // s* . y_j
        val[4 + 5 * j + 3] = fma(sd, (double)gv, val[4 + 5 * j + 3]);  // s_j . g
        val[4 + 5 * j + 4] = fma(yd, (double)gv, val[4 + 5 * j + 4]);  // y_j . g
      }
    }
    // lane q holds the wave's total of value q -> LDS -> thread q adds the four waves
    const int nval = 4 + 5 * pc;
    const double tot = lb_transpose_sum<NVAL>(val);
    if (lane < NVAL) sm[wave][lane] = tot;
    __syncthreads();
    if ((int)threadIdx.x < nval && (first || threadIdx.x >= 4)) {
      const int q = threadIdx.x;
      double r = 0.0;
#pragma unroll
      for (int w = 0; w < MDE_BLOCK / 64; ++w) r += sm[w][q];
      const int row = q < 4 ? q : 4 + 5 * done + (q - 4);
      if (PUBLISH)
        mde_st_partial(partial + (int64_t)row * nb + b, r);
      else
        partial[(int64_t)row * nb + b] = r;
    }
    __syncthreads();
  }
}

// Results of the direction step, kept in LDS until they are written back to LbDev.
struct LbOut {
  int m, accepted;
  double H;
  float c_g;
  float cs[MDE_LB_LD], cy[MDE_LB_LD];
  int order[MDE_LB_LD];
  double Sg[MDE_LB_LD], Yg[MDE_LB_LD], cq[MDE_LB_LD], al[MDE_LB_LD], cr[MDE_LB_LD];  // scratch of the recursion
};

// LDS written by some lanes of ONE wave and read by others: the hardware executes a wave's LDS
// accesses in order, the compiler must not move them across this point (no workgroup barrier: in the
// fused kernel the other waves of the block do not take part).
__device__ __forceinline__ void lb_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

// One wave.  Lane j owns column j of everything; the Gram matrices (SY, YY: LD x LD doubles of LDS,
// LD > history) are edited in place, the coefficients of the new direction go to *o.  `dots` as
// k_lb_reduce leaves them.  Nothing of LbDev is written.
template <int LD>
__device__ void lb_direction_core(const LbDev* __restrict__ dv, const double* dots, int history, double* SY,
                                  double* YY, LbOut* o) {
  const int j = threadIdx.x & 63;
  const int c = dv->count;
  {
    // the stored Gram matrices -> LDS, eight row groups per batch with all their loads in flight
    // together (a loop of one row per trip pays one memory latency per row: 10 us at ten pairs)
    constexpr int RP = 64 / (LD < 64 ? LD : 64);  // rows per pass of the 64 lanes
    const int col = j % LD, rsub = j / LD;
    for (int i0 = 0; i0 < c; i0 += 8 * RP) {
      double vs[8], vy[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int i = i0 + u * RP + rsub;
        const bool in = i < c && col < c;
        vs[u] = in ? dv->SY[i * MDE_LB_LD + col] : 0.0;
        vy[u] = in ? dv->YY[i * MDE_LB_LD + col] : 0.0;
      }
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int i = i0 + u * RP + rsub;
        if (i < c) {
          SY[i * LD + col] = vs[u];
          YY[i * LD + col] = vy[u];
        }
      }
    }
  }
  const double ys = dots[0], yy = dots[1], sg_new = dots[2], yg_new = dots[3];
  // per stored pair j: s_j.y*, y_j.y*, s*.y_j, s_j.g, y_j.g
  double s_old_ynew = 0, y_old_ynew = 0, snew_y_old = 0, Sg = 0, Yg = 0;
  if (j < c) {
    s_old_ynew = dots[4 + 5 * j + 0];
    y_old_ynew = dots[4 + 5 * j + 1];
    snew_y_old = dots[4 + 5 * j + 2];
    Sg = dots[4 + 5 * j + 3];
    Yg = dots[4 + 5 * j + 4];
  }
  const bool accepted = ys > 1e-10;  // lbfgs.py:472
  int m = c;
  double H = dv->H;
  int ord = (j <= history) ? dv->order[j] : 0;
  lb_wave_sync();
  if (accepted) {
    // append row / column c
    if (j < c) {
      SY[j * LD + c] = s_old_ynew;
      SY[c * LD + j] = snew_y_old;
      YY[j * LD + c] = y_old_ynew;
      YY[c * LD + j] = y_old_ynew;
    }
    if (j == c) {
      SY[c * LD + c] = ys;
      YY[c * LD + c] = yy;
      Sg = sg_new;
      Yg = yg_new;
    }
    lb_wave_sync();
    m = c + 1;
    H = ys / yy;  // lbfgs.py:486
    if (c == history) {
      // drop the oldest pair (lbfgs.py:474-478): shift everything up / left by one
      // (in place, rows ascending: row i is read before row i - 1 is written, and a wave's LDS
      // accesses execute in program order; per-lane row buffers would live in scratch memory --
      // twenty dependent memory round trips, most of this kernel's 12 us)
      for (int i = 1; i < m; ++i) {
        const double a = (j + 1 < m && j + 1 < LD) ? SY[i * LD + j + 1] : 0.0;
        const double y = (j + 1 < m && j + 1 < LD) ? YY[i * LD + j + 1] : 0.0;
        if (j < LD) {
          SY[(i - 1) * LD + j] = a;
          YY[(i - 1) * LD + j] = y;
        }
      }
      Sg = __shfl_down(Sg, 1, 64);
      Yg = __shfl_down(Yg, 1, 64);
      m = history;
      lb_wave_sync();
    }
    // slot permutation: the spare becomes the newest pair; when full, the oldest slot is the new spare
    if (c == history) {
      const int first = __shfl(ord, 0, 64);
      const int next = __shfl_down(ord, 1, 64);
      ord = (j < history) ? next : first;
    }
  }
  double my_cq = 0.0, my_cr = 0.0;
  if constexpr (LD <= 16) {
    // Short histories (the default memory is 10): lane i keeps row i and column i of SY and row i of
    // YY in registers; both loops are substitutions in which lane k finishes its coefficient, hands it
    // to the others with v_readlane and every later lane folds it into its own running sum -- LD
    // fully unrolled steps of a readlane and one FMA, no LDS and no cross-lane sums (the two loops
    // take 1 us; one wave sum per step took 9, the same recursion serially from LDS 9 as well).
    auto bcast = [](double v, int k) {
      const int lo = __builtin_amdgcn_readlane(__double2loint(v), k), hi = __builtin_amdgcn_readlane(__double2hiint(v), k);
      return __hiloint2double(hi, lo);
    };
    const int li = j < LD ? j : 0;
    double rS[LD], cS[LD], rY[LD];
#pragma unroll
    for (int k = 0; k < LD; ++k) {
      rS[k] = SY[li * LD + k];
      cS[k] = SY[k * LD + li];
      rY[k] = YY[li * LD + k];
    }
    const double rho = (j < m) ? 1.0 / SY[li * LD + li] : 0.0;
    double acc = -Sg, al = 0.0, cq = 0.0;
#pragma unroll
    for (int k = LD - 1; k >= 0; --k) {
      const double a_k = bcast(rho * acc, k);
      if (k < m) {
        if (j == k) {
          al = a_k;
          cq = -a_k;
        }
        if (j < k) acc = fma(-a_k, rS[k], acc);
      }
    }
    double yq = -Yg;
#pragma unroll
    for (int k = 0; k < LD; ++k) {
      const double cqk = bcast(cq, k);
      if (k < m) yq = fma(cqk, rY[k], yq);
    }
    double acc2 = H * yq, cr = 0.0;
#pragma unroll
    for (int k = 0; k < LD; ++k) {
      const double c_k = bcast(al - rho * acc2, k);
      if (k < m) {
        if (j == k) cr = c_k;
        if (j > k) acc2 = fma(c_k, cS[k], acc2);
      }
    }
    my_cq = cq;
    my_cr = cr;
  } else {
    // two-loop recursion in coefficient form: q = -g + sum cq_j y_j ; r = H q + sum cr_j s_j.  m is a
    // dozen: every lane runs the SAME serial recursion on the LDS copies (uniform addresses: broadcast
    // reads) -- ~m^2 dependent fp64 FMAs, 2 us; one cross-lane sum per step was 20 serial round trips
    // of six shuffles each, 9 of the kernel's 12 us.
    if (j < LD) {
      o->Sg[j] = Sg;
      o->Yg[j] = Yg;
    }
    lb_wave_sync();
    for (int i = m - 1; i >= 0; --i) {
      double a0 = -o->Sg[i], a1 = 0.0;
      int k = i + 1;
      for (; k + 1 < m; k += 2) {
        a0 = fma(o->cq[k], SY[i * LD + k], a0);
        a1 = fma(o->cq[k + 1], SY[i * LD + k + 1], a1);
      }
      if (k < m) a0 = fma(o->cq[k], SY[i * LD + k], a0);
      const double a = (a0 + a1) / SY[i * LD + i];
      lb_wave_sync();
      if (j == 0) {
        o->al[i] = a;
        o->cq[i] = -a;
      }
      lb_wave_sync();
    }
    for (int i = 0; i < m; ++i) {
      double q0 = -o->Yg[i], q1 = 0.0;
      int k = 0;
      for (; k + 1 < m; k += 2) {
        q0 = fma(o->cq[k], YY[i * LD + k], q0);
        q1 = fma(o->cq[k + 1], YY[i * LD + k + 1], q1);
      }
      if (k < m) q0 = fma(o->cq[k], YY[i * LD + k], q0);
      double r0 = H * (q0 + q1), r1 = 0.0;
      k = 0;
      for (; k + 1 < i; k += 2) {
        r0 = fma(o->cr[k], SY[k * LD + i], r0);
        r1 = fma(o->cr[k + 1], SY[(k + 1) * LD + i], r1);
      }
      if (k < i) r0 = fma(o->cr[k], SY[k * LD + i], r0);
      const double c = o->al[i] - (r0 + r1) / SY[i * LD + i];
      lb_wave_sync();
      if (j == 0) o->cr[i] = c;
      lb_wave_sync();
      if (j == i) {
        my_cr = c;
        my_cq = o->cq[i];
      }
    }
  }
  o->cs[j] = (j < m) ? (float)my_cr : 0.0f;
  o->cy[j] = (j < m) ? (float)(H * my_cq) : 0.0f;
  o->order[j] = ord;
  if (j == 0) {
    o->m = m;
    o->accepted = accepted ? 1 : 0;
    o->H = H;
    o->c_g = (float)(-H);
  }
  lb_wave_sync();
}

// One wave: *o and the edited Gram matrices -> LbDev.
template <int LD>
__device__ void lb_write_back(LbDev* __restrict__ dv, int history, const double* SY, const double* YY,
                              const LbOut* o) {
  const int j = threadIdx.x & 63;
  const int m = o->m;
  if (j < m) {
    dv->cs[j] = o->cs[j];
    dv->cy[j] = o->cy[j];
  }
  if (o->accepted) {
    for (int i = 0; i < m; ++i) {
      if (j < m) {
        dv->SY[i * MDE_LB_LD + j] = SY[i * LD + j];
        dv->YY[i * MDE_LB_LD + j] = YY[i * LD + j];
      }
    }
    if (j <= history) dv->order[j] = o->order[j];
  }
  if (j == 0) {
    dv->count = m;
    dv->accepted = o->accepted;
    dv->H = o->H;
    dv->c_g = o->c_g;
  }
}

#define MDE_LB_DIR_LDS(LD) (2 * (LD) * (LD) * sizeof(double) + sizeof(LbOut))
template <int LD>
__global__ __launch_bounds__(64) void k_lbfgs_direction(LbDev* __restrict__ dv, const double* __restrict__ dots,
                                                        int history, MdeGate gate) {
  if (mde_gate_closed(gate)) return;
  extern __shared__ __attribute__((aligned(16))) char lb_lds[];
  double* SY = reinterpret_cast<double*>(lb_lds);
  double* YY = SY + LD * LD;
  LbOut* out = reinterpret_cast<LbOut*>(YY + LD * LD);
  lb_direction_core<LD>(dv, dots, history, SY, YY, out);
  lb_write_back<LD>(dv, history, SY, YY, out);
}

// ---- the same step in ONE launch, for vectors small enough that launches, not bytes, are what an
// iteration costs (configs 2 and 3: N = 140k / 80k floats; every kernel boundary is ~5 us on this
// stack and the four launches below took 60 us of a 150 us iteration).  At most 128 workgroups, all
// resident at once, in phases separated by a grid-wide arrival counter:
//   1. stage the new pair and form the partial dot products of the workgroup's own elements;
//   -- every workgroup has published its partials (relaxed device-scope stores, as mde_last_block) --
//   2. workgroup q adds row q of the partials and publishes the dot product; -- arrival counter --
//      EVERY workgroup then runs the direction step on the same numbers in its own LDS: identical
//      coefficients everywhere, nothing to broadcast;
//   3. combine the new direction over the workgroup's own elements (it re-reads only what it wrote
//      itself in phase 1), publish the statistics partials; the last workgroup to arrive reduces
//      them and writes the bookkeeping back to LbDev (everyone has finished reading it by then).
#define MDE_LB_FUSED_LD 16       // history <= 15
#ifndef MDE_LB_FUSED_MAXN
#define MDE_LB_FUSED_MAXN (1 << 18)
#endif
#define MDE_LB_FUSED_MAXBLOCKS 512
// (the flag rows, work_lb_flags, fill their region of the small area exactly)
static_assert(MDE_WS_LB_FLAGS + 3 * MDE_LB_FUSED_MAXBLOCKS / 2 == MDE_WS_LB_VERDICT, "k_lb_fused: flag rows and verdict words");
// (design probe, -DMDE_LB_PROBE: workgroup 0 leaves wall-clock stamps -- 100 MHz -- of its phases behind the
// verdict words; tools/lbfused_probe.py prints them)
#ifdef MDE_LB_PROBE
#define LB_STAMP(k)                                                                                    \
  do {                                                                                                 \
    if (blockIdx.x == 0 && threadIdx.x == 0) reinterpret_cast<unsigned long long*>(verdict + 8)[k] = wall_clock64(); \
  } while (0)
#else
#define LB_STAMP(k) ((void)0)
#endif
// G: history pairs per pass over the vectors (8, or 12 when the history has 9 .. 12 pairs: ONE pass in both
// streaming phases instead of two -- the phases are bound by the latency of their dependent trips)
template <int G>
__global__ __launch_bounds__(MDE_BLOCK) void k_lb_fused(int64_t N, const float* __restrict__ g, float* __restrict__ g_prev,
                                                        const float* d, float t, float* __restrict__ buf,
                                                        LbDev* __restrict__ dv, int history, float* out,  // (out may be d)
                                                        double* __restrict__ partial, double* __restrict__ stats,
                                                        unsigned int* __restrict__ flags, unsigned int epoch,
                                                        unsigned int spin_limit, MdeGate gate) {
  if (mde_gate_closed(gate)) return;  // (every workgroup reads the same word: all of them leave, or none)
  constexpr int LD = MDE_LB_FUSED_LD;
  extern __shared__ char lb_debug_lds[];  // (only a test asks for dynamic LDS: it limits the workgroups per CU)
  (void)lb_debug_lds;
  // words behind the three flag rows: [0] = epoch once some workgroup gave up waiting, [1] = epoch once
  // the step is complete (k_lb_rescue redoes the step from the staged sums when it is not)
  unsigned int* verdict = flags + 3 * MDE_LB_FUSED_MAXBLOCKS;
  __shared__ double sm[MDE_BLOCK / 64][4 + 5 * G];
  __shared__ double s_dots[4 + 5 * LD];
  __shared__ double s_SY[LD * LD], s_YY[LD * LD];
  __shared__ LbOut s_out;
  const int count = dv->count;
  const int wave = threadIdx.x >> 6;
  const int nb = gridDim.x, b = blockIdx.x;
  LB_STAMP(0);
  // ---- phase 1
  lb_stage_phase<true, G>(N, g, g_prev, d, t, buf, dv, partial, sm);
  LB_STAMP(1);
  // Arrival point `which`: every workgroup raises its own flag word to this launch's epoch (plain
  // device-scope stores to distinct addresses; an arrival COUNTER costs ~20 ns per workgroup because
  // same-address atomics are executed one after the other at the memory side -- 5.6 us for 274
  // workgroups, three times per launch), the waiting workgroups read all flags, one per thread.
  auto grid_arrive = [&](int which, bool wait) {
    __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0): this thread's published values have completed
    __syncthreads();
    unsigned int* f = flags + which * MDE_LB_FUSED_MAXBLOCKS;
    if (threadIdx.x == 0) __hip_atomic_store(f + b, epoch + (unsigned int)which, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (!wait) return true;
    // The arrival points need every workgroup of the launch resident at once (an ordinary launch of at
    // most 128 workgroups: normally true).  A workgroup that does not see the others arrive within the
    // spin limit -- another process holds the CUs -- says so in verdict[0] and LEAVES: nobody gets past
    // a later arrival point then, nothing of the step's outputs is final, and k_lb_rescue (queued
    // behind this kernel) redoes the step from the staged sums.  Never a wrong direction, never a hang.
    for (unsigned int spins = 0;; ++spins) {
      bool ok = true;
      for (int k = threadIdx.x; k < nb; k += MDE_BLOCK)
        ok = ok && __hip_atomic_load(f + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == epoch + (unsigned int)which;
      if (__syncthreads_and(ok ? 1 : 0)) break;
      const bool failed = __hip_atomic_load(verdict, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == epoch;
      if (__syncthreads_or((failed || spins >= spin_limit) ? 1 : 0)) {
        if (threadIdx.x == 0) __hip_atomic_store(verdict, epoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        return false;
      }
      __builtin_amdgcn_s_sleep(1);
    }
    return __hip_atomic_load(verdict, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != epoch;
  };
  if (!grid_arrive(0, true)) return;
  LB_STAMP(2);
  // ---- phase 2a: workgroup q adds row q of the partials (k_lb_reduce: same order of additions)
  const int nrows = 4 + 5 * count;
  double* dots_g = partial + (int64_t)(4 + 5 * LD + 8) * nb;  // behind the dot-product and statistics rows
  for (int q = b; q < nrows; q += nb) {
    double r = 0.0;
    for (int k = threadIdx.x; k < nb; k += MDE_BLOCK) r += mde_ld_partial(partial + (int64_t)q * nb + k);
    const double tot = mde_block_sum(r, &sm[0][0]);
    if (threadIdx.x == 0) mde_st_partial(dots_g + q, tot);
    __syncthreads();
  }
  LB_STAMP(3);
  if (!grid_arrive(1, true)) return;
  LB_STAMP(4);
  // ---- phase 2b: every workgroup runs the direction step on the same numbers
  for (int q = threadIdx.x; q < nrows; q += MDE_BLOCK) s_dots[q] = mde_ld_partial(dots_g + q);
  __syncthreads();
  if (wave == 0) lb_direction_core<LD>(dv, s_dots, history, s_SY, s_YY, &s_out);
  __syncthreads();
  LB_STAMP(5);
  // ---- phase 3 (k_lb_combine_all), with the coefficients and the slot order of s_out
  const int m = s_out.m;
  const float c_g = s_out.c_g;
  double gd = 0, gg = 0, g1 = 0, gm = 0, nf = 0, dd = 0, dm = 0;
  for (int64_t i = (int64_t)b * MDE_BLOCK + threadIdx.x; i < N; i += (int64_t)nb * MDE_BLOCK) {
    const float gv = g[i];
    float v = c_g * gv;
    for (int j0 = 0; j0 < m; j0 += G) {
      float sv[G], yv[G];
#pragma unroll
      for (int j = 0; j < G; ++j) {
        const int jj = (j0 + j < m) ? j0 + j : 0;
        const float* sp = buf + (int64_t)(2 * s_out.order[jj]) * N;
        sv[j] = sp[i];
        yv[j] = sp[N + i];
      }
#pragma unroll
      for (int j = 0; j < G; ++j)
        if (j0 + j < m) v = fmaf(s_out.cy[j0 + j], yv[j], fmaf(s_out.cs[j0 + j], sv[j], v));
    }
    out[i] = v;
    const double gvd = gv, dv2 = v;
    gg += gvd * gvd;
    const double ag = fabs(gvd);
    g1 += ag;
    gm = ag > gm ? ag : gm;
    nf += (fabsf(gv) <= 3.402823466e+38f) ? 0.0 : 1.0;
    gd += gvd * dv2;
    dd += dv2 * dv2;
    const double ad = fabs(dv2);
    dm = ad > dm ? ad : dm;
  }
  const double v8[8] = {gd, gg, g1, gm, nf, dd, dm, 0.0};
  double* spart = partial + (int64_t)(4 + 5 * LD) * nb;  // behind the dot-product rows
  mde_publish8(v8, (1u << 3) | (1u << 6), spart, nb, b);
  LB_STAMP(6);
  // workgroup 0 finishes: the statistics rows, and the bookkeeping back to LbDev (everyone has
  // finished reading it when the third flag is up)
  if (!grid_arrive(2, b == 0)) return;
  if (b != 0) return;
  LB_STAMP(7);
  mde_final_rows(8, nb, spart, stats, (1ull << 3) | (1ull << 6));
  if (wave == 0) lb_write_back<LD>(dv, history, s_SY, s_YY, &s_out);
  __builtin_amdgcn_s_waitcnt(0x0F70);
  __syncthreads();
  if (threadIdx.x == 0) __hip_atomic_store(verdict + 1, epoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  LB_STAMP(8);
}

// Queued behind every k_lb_fused launch: nothing to do when that launch completed (verdict[1] ==
// epoch; one workgroup, a few microseconds).  Otherwise -- some workgroup gave up at an arrival point --
// ONE workgroup redoes phases 2 and 3 from the sums every workgroup staged in phase 1 (phase 1 has no
// waits: all of them ran it; its side effects -- g_prev <- g, the new pair in its slot -- are exactly
// what the four-launch path leaves behind its first launch), slowly but correctly: row sums, the
// direction step, d_out and its statistics, the bookkeeping.
__global__ __launch_bounds__(MDE_BLOCK) void k_lb_rescue(int64_t N, const float* __restrict__ g, const float* __restrict__ buf,
                                                         LbDev* __restrict__ dv, int history, float* out, int nb,
                                                         double* __restrict__ partial, double* __restrict__ stats,
                                                         unsigned int* __restrict__ flags, unsigned int epoch, MdeGate gate) {
  constexpr int LD = MDE_LB_FUSED_LD;
  if (mde_gate_closed(gate)) return;
  unsigned int* verdict = flags + 3 * MDE_LB_FUSED_MAXBLOCKS;
  if (__hip_atomic_load(verdict + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == epoch) return;
  if (threadIdx.x == 0) verdict[2] += 1u;  // (how often the rescue had to run: tests read it from the work buffer)
  __shared__ double sm[MDE_BLOCK / 64][MDE_LB_NVAL];
  __shared__ double s_dots[4 + 5 * LD];
  __shared__ double s_SY[LD * LD], s_YY[LD * LD];
  __shared__ LbOut s_out;
  const int wave = threadIdx.x >> 6;
  const int nrows = 4 + 5 * dv->count;
  for (int q = 0; q < nrows; ++q) {
    double r = 0.0;
    for (int k = threadIdx.x; k < nb; k += MDE_BLOCK) r += mde_ld_partial(partial + (int64_t)q * nb + k);
    const double tot = mde_block_sum(r, &sm[0][0]);
    if (threadIdx.x == 0) s_dots[q] = tot;
    __syncthreads();
  }
  if (wave == 0) lb_direction_core<LD>(dv, s_dots, history, s_SY, s_YY, &s_out);
  __syncthreads();
  const int m = s_out.m;
  const float c_g = s_out.c_g;
  double gd = 0, gg = 0, g1 = 0, gm = 0, nf = 0, dd = 0, dm = 0;
  for (int64_t i = threadIdx.x; i < N; i += MDE_BLOCK) {
    const float gv = g[i];
    float v = c_g * gv;
    for (int j = 0; j < m; ++j) {
      const float* sp = buf + (int64_t)(2 * s_out.order[j]) * N;
      v = fmaf(s_out.cy[j], sp[N + i], fmaf(s_out.cs[j], sp[i], v));
    }
    out[i] = v;
    const double gvd = gv, dv2 = v;
    gg += gvd * gvd;
    const double ag = fabs(gvd);
    g1 += ag;
    gm = ag > gm ? ag : gm;
    nf += (fabsf(gv) <= 3.402823466e+38f) ? 0.0 : 1.0;
    gd += gvd * dv2;
    dd += dv2 * dv2;
    const double ad = fabs(dv2);
    dm = ad > dm ? ad : dm;
  }
  const double v8[8] = {gd, gg, g1, gm, nf, dd, dm, 0.0};
  for (int q = 0; q < 8; ++q) {
    const bool is_max = q == 3 || q == 6;
    const double r = is_max ? mde_block_max(v8[q], &sm[0][0]) : mde_block_sum(v8[q], &sm[0][0]);
    if (threadIdx.x == 0) stats[q] = r;
    __syncthreads();
  }
  if (wave == 0) lb_write_back<LD>(dv, history, s_SY, s_YY, &s_out);
}

// ---- the device-driven step in four launches
// (1) k_lb_stage_all: stage the new pair and form every dot product against the stored pairs, eight
//     pairs per pass over the vectors; (2) k_lb_reduce adds the workgroups' partials to `dots`.
// (3) k_lbfgs_direction (above).
// (4) k_lb_combine_all: d_out from all pairs, its statistics against g in the same pass, reduced by
//     the last workgroup (what mde_vec_stats(g, d_out, NULL) writes).
template <int G>
__global__ __launch_bounds__(MDE_BLOCK) void k_lb_stage_all(int64_t N, const float* __restrict__ g,
                                                            float* __restrict__ g_prev,
                                                            const float* __restrict__ d, float t,
                                                            float* __restrict__ buf,
                                                            const LbDev* __restrict__ dv,
                                                            double* __restrict__ partial, MdeGate gate) {
  if (mde_gate_closed(gate)) return;
  __shared__ double sm[MDE_BLOCK / 64][4 + 5 * G];
  lb_stage_phase<false, G>(N, g, g_prev, d, t, buf, dv, partial, sm);
}

// dots[q] = sum_b partial[q * nb + b] for the 4 + 5 count rows that were written (one workgroup per
// row: 54 rows of up to 1024 partials are too much for one last workgroup)
__global__ void k_lb_reduce(int nb, const double* __restrict__ partial, const LbDev* __restrict__ dv,
                            double* __restrict__ dots, MdeGate gate) {
  if (mde_gate_closed(gate)) return;
  __shared__ double smem[8];
  const int q = blockIdx.x;
  if (q >= 4 + 5 * dv->count) return;
  double s = 0.0;
  for (int b = threadIdx.x; b < nb; b += blockDim.x) s += partial[(int64_t)q * nb + b];
  const double r = mde_block_sum(s, smem);
  if (threadIdx.x == 0) dots[q] = r;
}

// statistics rows as in k_vec_stats (x absent): 0 g.d 1 g.g 2 sum|g| 3 max|g| 4 #nonfinite 5 d.d 6 max|d| 7 0
__global__ __launch_bounds__(MDE_BLOCK) void k_lb_combine_all(int64_t N, const float* __restrict__ g,
                                                              const float* __restrict__ buf,
                                                              const LbDev* __restrict__ dv,
                                                              float* __restrict__ out,
                                                              double* __restrict__ partial,
                                                              double* __restrict__ stats,
                                                              unsigned int* __restrict__ ticket, MdeGate gate) {
  if (mde_gate_closed(gate)) return;
  __shared__ double smem[8];
  __shared__ float s_cs[MDE_LB_LD + MDE_LB_GROUP], s_cy[MDE_LB_LD + MDE_LB_GROUP];
  __shared__ int s_slot[MDE_LB_LD + MDE_LB_GROUP];
  const int count = dv->count;
  const float c_g = dv->c_g;
  if (threadIdx.x < MDE_LB_LD + MDE_LB_GROUP) {
    const bool in = (int)threadIdx.x < count;
    s_cs[threadIdx.x] = in ? dv->cs[threadIdx.x] : 0.0f;
    s_cy[threadIdx.x] = in ? dv->cy[threadIdx.x] : 0.0f;
    s_slot[threadIdx.x] = in ? dv->order[threadIdx.x] : 0;
  }
  __syncthreads();
  double gd = 0, gg = 0, g1 = 0, gm = 0, nf = 0, dd = 0, dm = 0;
  auto tally = [&](float gv, float v) __attribute__((always_inline)) {
    const double gvd = gv, dv2 = v;
    gg += gvd * gvd;
    const double ag = fabs(gvd);
    g1 += ag;
    gm = ag > gm ? ag : gm;
    nf += (fabsf(gv) <= 3.402823466e+38f) ? 0.0 : 1.0;
    gd += gvd * dv2;
    dd += dv2 * dv2;
    const double ad = fabs(dv2);
    dm = ad > dm ? ad : dm;
  };
  // 16-byte form (N a multiple of 4, 16-byte aligned vectors -- every history slot then is too): four
  // times the bytes per load instruction; 256 MB vectors: 3.8 -> TB/s measured in profiles/
  const bool vec = (N & 3) == 0 && ((reinterpret_cast<uintptr_t>(g) | reinterpret_cast<uintptr_t>(buf) |
                                     reinterpret_cast<uintptr_t>(out)) & 15) == 0;
  const int64_t N4 = vec ? (N >> 2) : 0;
  for (int64_t i = (int64_t)blockIdx.x * MDE_BLOCK + threadIdx.x; i < N4; i += (int64_t)gridDim.x * MDE_BLOCK) {
    const float4 gv = reinterpret_cast<const float4*>(g)[i];
    float4 v = make_float4(c_g * gv.x, c_g * gv.y, c_g * gv.z, c_g * gv.w);
    for (int j0 = 0; j0 < count; j0 += MDE_LB_GROUP) {
      float4 sv[MDE_LB_GROUP], yv[MDE_LB_GROUP];
#pragma unroll
      for (int j = 0; j < MDE_LB_GROUP; ++j) {
        const float4* sp = reinterpret_cast<const float4*>(buf + (int64_t)(2 * s_slot[j0 + j]) * N);
        sv[j] = sp[i];
        yv[j] = sp[N4 + i];
      }
#pragma unroll
      for (int j = 0; j < MDE_LB_GROUP; ++j)
        if (j0 + j < count) {
          const float cs = s_cs[j0 + j], cy = s_cy[j0 + j];
          v.x = fmaf(cy, yv[j].x, fmaf(cs, sv[j].x, v.x));
          v.y = fmaf(cy, yv[j].y, fmaf(cs, sv[j].y, v.y));
          v.z = fmaf(cy, yv[j].z, fmaf(cs, sv[j].z, v.z));
          v.w = fmaf(cy, yv[j].w, fmaf(cs, sv[j].w, v.w));
        }
    }
    reinterpret_cast<float4*>(out)[i] = v;
    tally(gv.x, v.x);
    tally(gv.y, v.y);
    tally(gv.z, v.z);
    tally(gv.w, v.w);
  }
  for (int64_t i = (N4 << 2) + (int64_t)blockIdx.x * MDE_BLOCK + threadIdx.x; i < N;
       i += (int64_t)gridDim.x * MDE_BLOCK) {
    const float gv = g[i];
    float v = c_g * gv;
    for (int j0 = 0; j0 < count; j0 += MDE_LB_GROUP) {
      // the sixteen loads of eight pairs before the first use (entries beyond count: slot 0, weight 0)
      float sv[MDE_LB_GROUP], yv[MDE_LB_GROUP];
#pragma unroll
      for (int j = 0; j < MDE_LB_GROUP; ++j) {
        const float* sp = buf + (int64_t)(2 * s_slot[j0 + j]) * N;
        sv[j] = sp[i];
        yv[j] = sp[N + i];
      }
#pragma unroll
      for (int j = 0; j < MDE_LB_GROUP; ++j)
        if (j0 + j < count) v = fmaf(s_cy[j0 + j], yv[j], fmaf(s_cs[j0 + j], sv[j], v));
    }
    out[i] = v;
    tally(gv, v);
  }
  const int nb = gridDim.x, b = blockIdx.x;
  const double v8[8] = {gd, gg, g1, gm, nf, dd, dm, 0.0};
  mde_publish8(v8, (1u << 3) | (1u << 6), partial, nb, b);
  if (!mde_last_block(ticket)) return;
  mde_final_rows(8, nb, partial, stats, (1ull << 3) | (1ull << 6));
}

extern "C" int mde_lbfgs_dev_reset(mde_lbfgs* o, void* stream) {
  if (!o || !o->dev) return MDE_E_INVALID;
  hipLaunchKernelGGL(k_lbfgs_dev_reset, dim3(1), dim3(64), 0, mde_stream(stream), o->dev, o->history);
  MDE_LAUNCH_CHECK();
  return MDE_OK;
}

// (environment knobs are read once, not per step: MDE_LB_UNFUSED forces the four-launch path;
// MDE_LB_DEBUG = "blocks,spins,lds_bytes" lets a test launch more workgroups than can be resident and
// watch the rescue kernel take over; mde_lbfgs_debug_knobs changes them inside a process)
struct LbKnobs {
  bool unfused;
  int blocks, spins, lds;
  int max_blocks;  // workgroups of the one-launch step (MDE_LB_MAXBLOCKS: design probe)
  LbKnobs() : unfused(getenv("MDE_LB_UNFUSED") != nullptr), blocks(0), spins(0), lds(0), max_blocks(256) {
    if (const char* e = getenv("MDE_LB_DEBUG")) sscanf(e, "%d,%d,%d", &blocks, &spins, &lds);
    if (const char* e = getenv("MDE_LB_MAXBLOCKS")) max_blocks = std::min(std::max(atoi(e), 1), MDE_LB_FUSED_MAXBLOCKS);
  }
};
static LbKnobs& lb_knobs() {
  static LbKnobs k;
  return k;
}
// (test hook: one process-wide record, no synchronisation -- see include/mde_hip.h)
extern "C" int mde_lbfgs_debug_knobs(int32_t unfused, int32_t blocks, int32_t spins, int32_t lds_bytes) {
  LbKnobs& k = lb_knobs();
  if (unfused >= 0) k.unfused = unfused != 0;
  if (blocks >= 0) k.blocks = blocks;
  if (spins >= 0) k.spins = spins;
  if (lds_bytes >= 0) {
    if (lds_bytes == 0 && k.lds > 0) {
      // back to no dynamic LDS: the attribute a test raised on the kernels goes back too
      MDE_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k_lb_fused<12>), hipFuncAttributeMaxDynamicSharedMemorySize, 0));
      MDE_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k_lb_fused<MDE_LB_GROUP>),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, 0));
    }
    k.lds = lds_bytes;
  }
  return MDE_OK;
}

// The four-launch form in its two halves (the whole step runs one behind the other, a row-sharded solve
// sums `dots` across the ranks in between).  Stage: launches (1) and (2), the dot products into `dots`.
static int lb_stage_launch(mde_lbfgs* o, const float* g, float* g_prev, const float* d, float t, double* dots,
                           double* work, hipStream_t st, MdeGate gate) {
  const int64_t N = o->N;
  double* partial = work + MDE_SMALL_DOUBLES;
  const int nb = mde_grid(N, MDE_BLOCK * 2, 1024);
  if (o->history > MDE_LB_GROUP && o->history <= 12)
    hipLaunchKernelGGL(k_lb_stage_all<12>, dim3(nb), dim3(MDE_BLOCK), 0, st, N, g, g_prev, d, t, o->buf, o->dev, partial, gate);
  else
    hipLaunchKernelGGL(k_lb_stage_all<MDE_LB_GROUP>, dim3(nb), dim3(MDE_BLOCK), 0, st, N, g, g_prev, d, t, o->buf,
                       o->dev, partial, gate);
  MDE_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_lb_reduce, dim3(4 + 5 * o->history), dim3(MDE_BLOCK), 0, st, nb, partial, o->dev, dots, gate);
  MDE_LAUNCH_CHECK();
  return MDE_OK;
}
// Finish: launches (3) and (4), from `dots` to d_out and its statistics.
static int lb_finish_launch(mde_lbfgs* o, const float* g, float* d_out, double* stats, const double* dots, double* work,
                            hipStream_t st, MdeGate gate) {
  const int64_t N = o->N;
  double* partial = work + MDE_SMALL_DOUBLES;
  if (o->history < 16) {
    hipLaunchKernelGGL(k_lbfgs_direction<16>, dim3(1), dim3(64), MDE_LB_DIR_LDS(16), st, o->dev, dots, o->history, gate);
  } else {
    static bool dir_attr = false;
    if (!dir_attr) {
      MDE_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k_lbfgs_direction<MDE_LB_LD>),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, (int)MDE_LB_DIR_LDS(MDE_LB_LD)));
      dir_attr = true;
    }
    hipLaunchKernelGGL(k_lbfgs_direction<MDE_LB_LD>, dim3(1), dim3(64), MDE_LB_DIR_LDS(MDE_LB_LD), st, o->dev, dots,
                       o->history, gate);
  }
  MDE_LAUNCH_CHECK();
  const int nbc = mde_grid(N, MDE_BLOCK * 2, MDE_RED_BLOCKS);  // (its last workgroup adds nbc partials per row)
  hipLaunchKernelGGL(k_lb_combine_all, dim3(nbc), dim3(MDE_BLOCK), 0, st, N, g, o->buf, o->dev, d_out, partial,
                     stats, work_ticket(work, TK_LB_COMBINE), gate);
  MDE_LAUNCH_CHECK();
  return MDE_OK;
}

// One whole L-BFGS direction update without a host round trip: stage (y = g - g_prev, s = t d,
// g_prev <- g), accept / reject, two-loop recursion, d_out = the new direction, stats as
// mde_vec_stats(g, d_out, NULL).  ASYNC.
int mde_lbfgs_dev_step_impl(mde_lbfgs* o, const float* g, float* g_prev, const float* d, float t, float* d_out,
                            double* stats, double* work, void* stream, MdeGate gate) {
  if (!o || !o->dev || !g || !g_prev || !d || !d_out || !stats || !work) return MDE_E_INVALID;
  hipStream_t st = mde_stream(stream);
  const int64_t N = o->N;
  double* partial = work + MDE_SMALL_DOUBLES;
  const LbKnobs& knobs = lb_knobs();
  if (N <= MDE_LB_FUSED_MAXN && o->history < MDE_LB_FUSED_LD && !knobs.unfused) {
    // At most 256 workgroups: the arrival points need every workgroup of the launch resident at once.
    // The kernel fits two workgroups per CU (198 VGPRs), i.e. 512 on the chip -- 256 leaves half of that
    // to whatever else is resident, e.g. the same kernel of another process sharing the GPU.  (Round 4:
    // 128 until the phase stamps of tools/lbfused_probe.py showed the two streaming phases at 11.6 us
    // each at N = 140k -- five dependent trips per thread, nothing to hide their latency behind.)
    // Residency is still not GUARANTEED by an ordinary launch: a workgroup that waits longer than the
    // spin limit gives up, and k_lb_rescue (always queued behind) redoes the step -- see k_lb_fused.
    int nbf = mde_grid(N, MDE_BLOCK, knobs.max_blocks);
    if (knobs.blocks > 0) nbf = std::min(knobs.blocks, MDE_LB_FUSED_MAXBLOCKS);
    const unsigned int spin_limit = knobs.spins > 0 ? (unsigned int)knobs.spins : (1u << 20);
    static std::atomic<unsigned int> launches{0};  // one epoch per launch, shared by every solver object
    const unsigned int epoch = 4u * (launches.fetch_add(1u) + 1u);
    auto kern = (o->history > MDE_LB_GROUP && o->history <= 12) ? k_lb_fused<12> : k_lb_fused<MDE_LB_GROUP>;
    if (knobs.lds > 0)
      MDE_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, knobs.lds));
    hipLaunchKernelGGL(kern, dim3(nbf), dim3(MDE_BLOCK), (size_t)std::max(knobs.lds, 0), st, N, g, g_prev, d, t, o->buf,
                       o->dev, o->history, d_out, partial, stats, work_lb_flags(work), epoch, spin_limit, gate);
    MDE_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_lb_rescue, dim3(1), dim3(MDE_BLOCK), 0, st, N, g, o->buf, o->dev, o->history, d_out, nbf, partial, stats,
                       work_lb_flags(work), epoch, gate);
    MDE_LAUNCH_CHECK();
    return MDE_OK;
  }
  double* dots = work;  // the small area: 4 + 5 * 63 doubles at most
  const int rc = lb_stage_launch(o, g, g_prev, d, t, dots, work, st, gate);
  if (rc != MDE_OK) return rc;
  return lb_finish_launch(o, g, d_out, stats, dots, work, st, gate);
}
extern "C" int mde_lbfgs_dev_step(mde_lbfgs* o, const float* g, float* g_prev, const float* d, float t,
                                  float* d_out, double* stats, double* work, void* stream) {
  return mde_lbfgs_dev_step_impl(o, g, g_prev, d, t, d_out, stats, work, stream, MdeGate{nullptr, 0u});
}

// ---- round 6: the same step in two halves, for a solve whose vectors are sharded by rows across ranks
// (pymde_amd/optim.py, _ShardedEngine).  Every rank keeps the history of ITS rows only (o->N = its elements):
// mde_lbfgs_dev_stage stages the pair and leaves the 4 + 5 * history inner products over the rank's elements in
// work[0 ..); the caller sums them across the ranks in place (one small all-reduce of doubles); mde_lbfgs_dev_finish
// takes the accept / drop-oldest decision and runs the two-loop recursion on those sums -- every rank the same
// arithmetic on the same numbers -- and writes the rank's rows of the new direction, with the statistics of (g, d_out)
// over its elements (partial: the caller reduces them, mde_rank_reduce).  Always the four-launch form's kernels.
extern "C" int mde_lbfgs_dev_stage(mde_lbfgs* o, const float* g, float* g_prev, const float* d, float t, double* work,
                                   void* stream) {
  if (!o || !o->dev || !g || !g_prev || !d || !work) return MDE_E_INVALID;
  return lb_stage_launch(o, g, g_prev, d, t, work, work, mde_stream(stream), MdeGate{nullptr, 0u});
}
extern "C" int mde_lbfgs_dev_finish(mde_lbfgs* o, const float* g, float* d_out, double* stats, double* work, void* stream) {
  if (!o || !o->dev || !g || !d_out || !stats || !work) return MDE_E_INVALID;
  return lb_finish_launch(o, g, d_out, stats, work, work, mde_stream(stream), MdeGate{nullptr, 0u});
}
extern "C" int32_t mde_lbfgs_dev_dots(const mde_lbfgs* o) { return o ? 4 + 5 * o->history : 0; }

// out[q] = sum (or max, bit q of max_mask) over the ranks r, in rank order, of in[r * count + q]  (q < count <= 64);
// loss_slot >= 0: that slot's result also goes to *loss_out as a float.  The per-rank records of a sharded solve --
// statistics boards and loss shares, gathered with one all-gather -- reduced with mixed operations in one launch.
__global__ void k_rank_reduce(int world, int count, unsigned long long max_mask, const double* __restrict__ in,
                              double* __restrict__ out, int loss_slot, float* __restrict__ loss_out) {
  const int q = threadIdx.x;
  if (q >= count) return;
  const bool is_max = (max_mask >> q) & 1ull;
  double a = in[q];
  for (int r = 1; r < world; ++r) {
    const double v = in[(size_t)r * count + q];
    a = is_max ? (v > a ? v : a) : a + v;
  }
  out[q] = a;
  if (q == loss_slot && loss_out) *loss_out = (float)a;
}
extern "C" int mde_rank_reduce(int32_t world, int32_t count, uint64_t max_mask, const double* in, double* out,
                               int32_t loss_slot, float* loss_out, void* stream) {
  if (world < 1 || count < 1 || count > 64 || !in || !out) return MDE_E_INVALID;
  hipLaunchKernelGGL(k_rank_reduce, dim3(1), dim3(64), 0, mde_stream(stream), (int)world, (int)count,
                     (unsigned long long)max_mask, in, out, (int)loss_slot, loss_out);
  MDE_LAUNCH_CHECK();
  return MDE_OK;
}

// copies of the device bookkeeping for tests: count, accepted
extern "C" int mde_lbfgs_dev_info(const mde_lbfgs* o, int32_t* count_host, int32_t* accepted_host,
                                  void* stream) {
  if (!o || !o->dev || !count_host || !accepted_host) return MDE_E_INVALID;
  hipStream_t st = mde_stream(stream);
  int h[2] = {0, 0};
  MDE_HIP(hipMemcpyAsync(h, o->dev, sizeof(h), hipMemcpyDeviceToHost, st));
  MDE_HIP(hipStreamSynchronize(st));
  *count_host = h[0];
  *accepted_host = h[1];
  return MDE_OK;
}

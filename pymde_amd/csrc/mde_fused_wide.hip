// mde_fused_wide.hip -- the unpipelined general-d fused kernel.  Since the pipelined kernel
// (mde_distortion.hip: k_fused_wide4p) took every d = 5 .. 512 this is what runs behind it:
// d = 513 .. 2048, and MDE_WIDE_P=0, the comparator of the tests.
#include "mde_fused.h"

// One wave owns a row.  GL lanes cooperate on one half-edge (64 / GL half-edges in flight per wave
// step); lane `lig` holds the columns c = lig + j*GL, j < K, of a row.  A column is one float (T =
// float: any d, any alignment) or one float4 (T = wide_f4: d a multiple of 4 and 16-byte aligned
// rows -- a row gather is 16 bytes per lane per instruction, a quarter of the load instructions).
typedef float wide_f4 __attribute__((ext_vector_type(4)));

MDE_DEV float wide_sq(float d, float ss) { return fmaf(d, d, ss); }
MDE_DEV float wide_sq(wide_f4 d, float ss) {
  ss = fmaf(d.x, d.x, ss);
  ss = fmaf(d.y, d.y, ss);
  ss = fmaf(d.z, d.z, ss);
  return fmaf(d.w, d.w, ss);
}
MDE_DEV float wide_fma(float g, float d, float acc) { return fmaf(g, d, acc); }
MDE_DEV wide_f4 wide_fma(float g, wide_f4 d, wide_f4 acc) { return acc + g * d; }
MDE_DEV float wide_xor_add(float a, int o) { return a + __shfl_xor(a, o, 64); }
MDE_DEV wide_f4 wide_xor_add(wide_f4 a, int o) {
  a.x += __shfl_xor(a.x, o, 64);
  a.y += __shfl_xor(a.y, o, 64);
  a.z += __shfl_xor(a.z, o, 64);
  a.w += __shfl_xor(a.w, o, 64);
  return a;
}

template <class T, int GL, int K, bool INDIRECT, class Fn>
__global__ __launch_bounds__(MDE_BLOCK) void k_fused_wide(
    int nrows, int row_lo, int ncol, const int32_t* __restrict__ rowptr, const int32_t* __restrict__ nbr,
    const int32_t* __restrict__ eid, const float* __restrict__ a0, const float* __restrict__ a1, int a0_scalar,
    int a1_scalar, const T* __restrict__ X, T* __restrict__ grad, double* __restrict__ loss_partials, Fn fn,
    float inv_p, float grad_scale) {
  __shared__ double smem[8];
  constexpr int E = 64 / GL;  // half-edges per wave step
  // independent steps in flight (row gathers are long-latency HBM reads at large d)
  constexpr int U = K <= 2 ? 4 : (K * sizeof(T) <= 16 ? 2 : 1);
  // The 16-byte form fetches a step's neighbour ids and parameters one step AHEAD, so that their
  // latency overlaps the row gathers of the current step instead of preceding them.  Not the 4-byte
  // form: the second set of meta registers costs 9 of its 36 instantiations one or two waves per SIMD.
  constexpr bool V16 = sizeof(T) == 16;
  const int lane = threadIdx.x & 63;
  const int lig = lane & (GL - 1);
  const int sub = lane / GL;  // which of the E half-edges this lane works on
  const int wave = (blockIdx.x * MDE_BLOCK + threadIdx.x) >> 6;
  const int nwaves = (gridDim.x * MDE_BLOCK) >> 6;
  float loss = 0.0f;
  const EdgeParams<INDIRECT> params(eid, a0, a1, a0_scalar, a1_scalar);
  const T zero = T{};
  const bool full = V16 && ncol == GL * K;

  for (int r = wave; r < nrows; r += nwaves) {
    const int beg = rowptr[r], end = rowptr[r + 1];
    const int64_t v = (int64_t)row_lo + r;
    T xv[K], acc[K];
#pragma unroll
    for (int j = 0; j < K; ++j) {
      const int c = lig + j * GL;
      xv[j] = (c < ncol) ? X[v * ncol + c] : zero;
      acc[j] = zero;
    }
    // of the U steps of a trip: is there a half-edge, its neighbour, its parameters
    auto load_meta = [&](int h0, bool (&live)[U], int64_t (&u)[U], float (&p0)[U], float (&p1)[U])
                         __attribute__((always_inline)) {
#pragma unroll
      for (int q = 0; q < U; ++q) {
        const int h = h0 + q * E + sub;
        live[q] = h < end;
        const int hh = live[q] ? h : beg;
        u[q] = nbr[hh];
        params.load(hh, p0[q], p1[q]);
      }
    };
    bool live_n[U];
    int64_t u_n[U];
    float p0_n[U], p1_n[U];
    if (V16 && beg < end) load_meta(beg, live_n, u_n, p0_n, p1_n);
    for (int h0 = beg; h0 < end; h0 += E * U) {
      bool live[U];
      int64_t u[U];
      float p0[U], p1[U];
      if constexpr (V16) {
#pragma unroll
        for (int q = 0; q < U; ++q) {
          live[q] = live_n[q];
          u[q] = u_n[q];
          p0[q] = p0_n[q];
          p1[q] = p1_n[q];
        }
      } else {
        load_meta(h0, live, u, p0, p1);
      }
      T xu[U][K];
      if (full) {
        // (every lane has a column: plain loads -- a predicated load is a branch around it, and the
        // gathers of a step then go out one after the other)
#pragma unroll
        for (int q = 0; q < U; ++q)
#pragma unroll
          for (int j = 0; j < K; ++j) xu[q][j] = X[u[q] * ncol + lig + j * GL];
      } else {
#pragma unroll
        for (int q = 0; q < U; ++q)
#pragma unroll
          for (int j = 0; j < K; ++j) {
            const int c = lig + j * GL;
            xu[q][j] = (c < ncol) ? X[u[q] * ncol + c] : zero;
          }
      }
      if (V16 && h0 + E * U < end) load_meta(h0 + E * U, live_n, u_n, p0_n, p1_n);
#pragma unroll
      for (int q = 0; q < U; ++q) {
        T diff[K];
        float ss = 0.0f;
#pragma unroll
        for (int j = 0; j < K; ++j) {
          diff[j] = xv[j] - xu[q][j];
          ss = wide_sq(diff[j], ss);
        }
        ss = mde_group_sum<GL>(ss);
        float f, gd;
        fn.eval(ss, p0[q], p1[q], f, gd);
        float g = mde_fix_g(gd * inv_p);
        if (!live[q]) {
          g = 0.0f;
          f = 0.0f;
        }
        if (lig == 0) loss += f;
#pragma unroll
        for (int j = 0; j < K; ++j) acc[j] = wide_fma(g, diff[j], acc[j]);
      }
    }
    if (grad) {
      // combine the E sub-groups (lanes with equal lig): xor over the sub index bits
#pragma unroll
      for (int j = 0; j < K; ++j) {
#pragma unroll
        for (int o = 32; o >= GL; o >>= 1) acc[j] = wide_xor_add(acc[j], o);
      }
      if (sub == 0) {
#pragma unroll
        for (int j = 0; j < K; ++j) {
          const int c = lig + j * GL;
          if (c < ncol) grad[v * ncol + c] = acc[j] * grad_scale;
        }
      }
    }
  }
  const double bs = mde_block_sum((double)loss, smem);
  if (threadIdx.x == 0) loss_partials[blockIdx.x] = bs;
}

template <class T, int GL, int K, bool IND, class Fn>
static int launch_wide_gk(FusedArgs& A, const Fn& fn) {
  const mde_plan* P = A.plan;
  const int nrows = fused_row_grid(A, 64);
  hipLaunchKernelGGL((k_fused_wide<T, GL, K, IND, Fn>), dim3(A.nblocks), dim3(MDE_BLOCK), 0, A.st, nrows,
                     (int)mde_plan_row_lo(P), A.d / (int)(sizeof(T) / sizeof(float)), mde_plan_rowptr(P),
                     mde_plan_nbr(P), mde_plan_eid(P), A.a0, A.a1, A.a0_scalar, A.a1_scalar,
                     reinterpret_cast<const T*>(A.X), reinterpret_cast<T*>(A.grad), A.partials, fn, A.inv_p,
                     A.grad_scale);
  MDE_LAUNCH_CHECK();
  return MDE_OK;
}

template <bool IND, class Fn>
static int launch_wide(FusedArgs& A, const Fn& fn) {
  const int d = A.d;
  if ((d & 3) == 0 && ((reinterpret_cast<uintptr_t>(A.X) | reinterpret_cast<uintptr_t>(A.grad)) & 15) == 0) {
    const int d4 = d >> 2;
    if (d4 <= 2) return launch_wide_gk<wide_f4, 2, 1, IND, Fn>(A, fn);
    if (d4 <= 4) return launch_wide_gk<wide_f4, 4, 1, IND, Fn>(A, fn);
    if (d4 <= 8) return launch_wide_gk<wide_f4, 8, 1, IND, Fn>(A, fn);
    if (d4 <= 16) return launch_wide_gk<wide_f4, 16, 1, IND, Fn>(A, fn);
    // FOUR float4s per lane where the row is wide enough -- 8 lanes cooperate on a 512-byte row instead of
    // 32, a wave step takes 8 half-edges instead of 2 and the cross-lane sum of |x_v - x_u|^2 is 3 steps instead of 5:
    // config 5 (d = 128, uniform graph) 3.13 -> 2.93 ms (6.5 -> 7.0 of the 7.4 TB/s random-row ceiling), neighbours within
    // 1000 / 100 rows 2.36 -> 1.66 / 1.84 -> 1.20 ms (`profiles/r06_d128_locality.txt`)
    if (d4 <= 32) return launch_wide_gk<wide_f4, 8, 4, IND, Fn>(A, fn);
    if (d4 <= 64) return launch_wide_gk<wide_f4, 16, 4, IND, Fn>(A, fn);
    if (d4 <= 128) return launch_wide_gk<wide_f4, 32, 4, IND, Fn>(A, fn);
    if (d4 <= 256) return launch_wide_gk<wide_f4, 64, 4, IND, Fn>(A, fn);
    if (d4 <= 512) return launch_wide_gk<wide_f4, 64, 8, IND, Fn>(A, fn);
  }
  if (d <= 8) return launch_wide_gk<float, 8, 1, IND, Fn>(A, fn);
  if (d <= 16) return launch_wide_gk<float, 16, 1, IND, Fn>(A, fn);
  if (d <= 32) return launch_wide_gk<float, 32, 1, IND, Fn>(A, fn);
  if (d <= 64) return launch_wide_gk<float, 64, 1, IND, Fn>(A, fn);
  if (d <= 128) return launch_wide_gk<float, 64, 2, IND, Fn>(A, fn);
  if (d <= 256) return launch_wide_gk<float, 64, 4, IND, Fn>(A, fn);
  if (d <= 512) return launch_wide_gk<float, 64, 8, IND, Fn>(A, fn);
  if (d <= 1024) return launch_wide_gk<float, 64, 16, IND, Fn>(A, fn);
  if (d <= 2048) return launch_wide_gk<float, 64, 32, IND, Fn>(A, fn);
  mde_set_error("embedding dimension %d > 2048 is not supported by the fused kernel", d);
  return MDE_E_UNSUPPORTED;
}

int mde_fused_wide(FusedArgs& A, const mde_func* f) {
  const MdeFuncArgs a = func_args(f);
  if (func_is_log1p15(f)) return launch_wide<false>(A, FnSingle<MDE_F_LOG1P, 2>{a});
  return launch_wide<false>(A, FnRuntime{a});
}

int mde_fused_wide_unfused(FusedArgs& A, mde_unfused which) {
  if (which == MDE_UNFUSED_SCATTER) return launch_wide<true>(A, FnScatter{});
  return launch_wide<true>(A, FnDistBackward{});
}

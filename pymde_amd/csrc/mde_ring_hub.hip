// mde_ring_hub.hip -- the rows the LDS-ring layout peels off (mde_ring_rows.h): evaluated from the CSR plan behind
// the ring kernel, on the same stream.  A unit of its own: a plan without hub rows never loads these kernels.
#include "mde_ring.h"

// ---------------------------------------------------------------- round 6: the peeled hub rows
// One workgroup per segment of MDE_HUB_SEG consecutive CSR positions of ONE hub row: gather x_u, evaluate (run-time
// functor; the parameters come from the caller's per-edge arrays through the plan's edge ids -- mde_func.e0 / e1 --,
// the ring-order streams do not hold these entries), sum g (x_v - x_u) and the loss terms over the segment in a fixed
// order (lane-strided partial sums, wave butterflies, waves in order; double).  k_hub_finish adds a row's segments in
// order, writes the gradient row (overwriting the zeros the ring kernel's epilogue left there) and adds the hub rows'
// loss to the ring kernel's: same stream, behind it.  count_all, loss_band: the layout's rule for who adds an edge's loss term.
template <int D>
__global__ __launch_bounds__(MDE_BLOCK) void k_hub_rows(const int32_t* __restrict__ hub_rows, const int32_t* __restrict__ hub_seg,
                                                        int row_lo, const int32_t* __restrict__ nbr,
                                                        const int32_t* __restrict__ eid, const float* __restrict__ e0,
                                                        const float* __restrict__ e1, int e0_scalar, int e1_scalar,
                                                        const float* __restrict__ X, FnRuntime fn, float inv_p, int count_all,
                                                        int loss_band, double* __restrict__ partial) {
  __shared__ double smem[8];
  const int sgi = blockIdx.x;
  const int hi = hub_seg[4 * sgi], beg = hub_seg[4 * sgi + 1], end = hub_seg[4 * sgi + 2];
  const int64_t v = (int64_t)row_lo + hub_rows[hi];
  float xv[D];
#pragma unroll
  for (int c = 0; c < D; ++c) xv[c] = X[v * D + c];
  const float e0s = e0_scalar ? e0[0] : 0.0f;
  const float e1s = (e1 && e1_scalar) ? e1[0] : 0.0f;
  double acc[D], loss = 0.0;
#pragma unroll
  for (int c = 0; c < D; ++c) acc[c] = 0.0;
  for (int h = beg + (int)threadIdx.x; h < end; h += MDE_BLOCK) {
    const int u = nbr[h], k = eid[h];
    const float p0 = e0_scalar ? e0s : e0[k];
    const float p1 = (e1 && !e1_scalar) ? e1[k] : e1s;
    float diff[D], ss = 0.0f;
#pragma unroll
    for (int c = 0; c < D; ++c) {
      diff[c] = xv[c] - X[(size_t)u * D + c];
      ss = fmaf(diff[c], diff[c], ss);
    }
    float f, gd;
    fn.eval(ss, p0, p1, f, gd);
    const float g = mde_fix_g(gd * inv_p);
    // (the twin entry of this half-edge sits in a ring stream: the same rule on both sides)
    if (count_all || ring_counts((uint32_t)v, (uint32_t)u, (uint32_t)loss_band)) loss += (double)f;
#pragma unroll
    for (int c = 0; c < D; ++c) acc[c] += (double)(g * diff[c]);
  }
#pragma unroll
  for (int c = 0; c < D; ++c) {
    const double t = mde_block_sum(acc[c], smem);
    if (threadIdx.x == 0) partial[(size_t)sgi * 8 + c] = t;
  }
  const double tl = mde_block_sum(loss, smem);
  if (threadIdx.x == 0) partial[(size_t)sgi * 8 + 4] = tl;
}

// One wave per hub row (blocks 0 .. n_hub - 1): the lanes add the row's segments lane-strided, a butterfly adds the lanes
// (fixed order); the last block adds the segments' loss terms the same way.  (The first version gave a row to ONE
// thread: the 977 segments of a 5e5-degree hub were 977 dependent loads, 148 us.)
template <int D>
__global__ __launch_bounds__(64) void k_hub_finish(int n_hub, int n_seg, const int32_t* __restrict__ hub_rows,
                                                   const int32_t* __restrict__ hub_first,
                                                   const double* __restrict__ partial, int row_lo, float grad_scale,
                                                   float* __restrict__ grad, double loss_scale, float* __restrict__ loss_out,
                                                   double* __restrict__ loss_d) {
  const int lane = threadIdx.x;
  if ((int)blockIdx.x < n_hub) {
    if (!grad) return;
    const int i = blockIdx.x;
    double a[D];
#pragma unroll
    for (int c = 0; c < D; ++c) a[c] = 0.0;
    for (int sg = hub_first[i] + lane; sg < hub_first[i + 1]; sg += 64) {
#pragma unroll
      for (int c = 0; c < D; ++c) a[c] += partial[(size_t)sg * 8 + c];
    }
#pragma unroll
    for (int c = 0; c < D; ++c) a[c] = mde_wave_sum(a[c]);
    if (lane == 0) {
      const int64_t v = (int64_t)row_lo + hub_rows[i];
#pragma unroll
      for (int c = 0; c < D; ++c) grad[v * D + c] = (float)a[c] * grad_scale;
    }
    return;
  }
  double t = 0.0;
  for (int sg = lane; sg < n_seg; sg += 64) t += partial[(size_t)sg * 8 + 4];
  const double tot = mde_wave_sum(t);
  // (the ring kernel left its part of the loss in *loss_d in double: the hub rows' part is added before the one rounding)
  if (lane == 0) {
    *loss_d += tot * loss_scale;
    *loss_out = (float)*loss_d;
  }
}

template <int D>
static int hub_launch_d(const RingArgs& A, const mde_func* f, const float* e0, const float* e1, int e0_scalar, int e1_scalar) {
  const mde_plan* plan = A.plan;
  const mde_ring_layout& L = plan->ring;
  FnRuntime fn{func_args(f)};
  hipLaunchKernelGGL(k_hub_rows<D>, dim3(L.n_hub_segs), dim3(MDE_BLOCK), 0, A.st, L.hub_rows, L.hub_seg, (int)plan->row_lo, plan->nbr,
                     plan->eid, e0, e1, e0_scalar, e1_scalar, A.X, fn, A.inv_p, L.count_all, L.loss_band, L.hub_partial);
  MDE_LAUNCH_CHECK();
  const int nb = L.n_hub_rows + 1;
  // (the ring kernel's rule: the smaller endpoint adds f -> 2 x the caller's half-weight; count_all: every entry f / 2)
  hipLaunchKernelGGL(k_hub_finish<D>, dim3(nb), dim3(64), 0, A.st, L.n_hub_rows, L.n_hub_segs, L.hub_rows, L.hub_first,
                     L.hub_partial, (int)plan->row_lo, A.grad_scale, A.grad, (L.count_all ? 1.0 : 2.0) * A.loss_scale, A.loss_out,
                     plan->partials + MDE_PARTIALS_LOSS_D);
  MDE_LAUNCH_CHECK();
  return MDE_OK;
}

int mde_ring_launch_hub(const RingArgs& A, const mde_func* f) {
  // the hub rows read their parameters in the caller's edge order
  const float *e0 = f->e0, *e1 = f->e1;
  int e0_scalar = 0, e1_scalar = 0;
  if (f->a0_scalar == 1) {
    e0 = f->a0;
    e0_scalar = 1;
  }
  if (f->a1 && f->a1_scalar) {
    e1 = f->a1;
    e1_scalar = 1;
  }
  if (!e0 || (f->a1 && !e1)) {
    mde_set_error("this plan's LDS-ring layout peels %d hub rows off to the CSR hub kernel: mde_func.e0 (and e1 for two-parameter "
                  "functions) must point at the per-edge arrays in the caller's edge order", A.plan->ring.n_hub_rows);
    return MDE_E_INVALID;
  }
  switch (A.d) {
    case 1: return hub_launch_d<1>(A, f, e0, e1, e0_scalar, e1_scalar);
    case 2: return hub_launch_d<2>(A, f, e0, e1, e0_scalar, e1_scalar);
    case 3: return hub_launch_d<3>(A, f, e0, e1, e0_scalar, e1_scalar);
    default: return hub_launch_d<4>(A, f, e0, e1, e0_scalar, e1_scalar);
  }
}

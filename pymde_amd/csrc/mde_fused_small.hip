// mde_fused_small.hip -- the fused CSR kernels of embedding dimensions d = 1 .. 4: a row per group
// of lanes (k_fused_small) and edge-balanced tiles (k_fused_flat + k_flat_fixup).
#include "mde_fused.h"

// ---------------------------------------------------------------- small-d fused kernel
// D in {1,2,3,4}: one lane per half-edge, G lanes per row.
template <int D, int G, bool INDIRECT, class Fn>
__global__ __launch_bounds__(MDE_BLOCK) void k_fused_small(
    int nrows, int row_lo, const int32_t* __restrict__ rowptr, const int32_t* __restrict__ nbr,
    const int32_t* __restrict__ eid, const float* __restrict__ a0, const float* __restrict__ a1,
    int a0_scalar, int a1_scalar, const float* __restrict__ X, float* __restrict__ grad,
    double* __restrict__ loss_partials, Fn fn, float inv_p, float grad_scale) {
  __shared__ double smem[8];
  const int lig = threadIdx.x & (G - 1);
  const int group = (blockIdx.x * MDE_BLOCK + threadIdx.x) / G;
  const int ngroups = (gridDim.x * MDE_BLOCK) / G;
  float loss = 0.0f;
  const EdgeParams<INDIRECT> params(eid, a0, a1, a0_scalar, a1_scalar);

  for (int r = group; r < nrows; r += ngroups) {
    const int beg = rowptr[r], end = rowptr[r + 1];
    const int64_t v = (int64_t)row_lo + r;
    const VecD<D> xv = load_row<D>(X, v);
    float acc[D];
#pragma unroll
    for (int c = 0; c < D; ++c) acc[c] = 0.0f;
#pragma unroll 2
    for (int h = beg + lig; h < end; h += G) {
      const int u = nbr[h];
      float p0, p1;
      params.load(h, p0, p1);
      const VecD<D> xu = load_row<D>(X, u);
      float diff[D], ss = 0.0f;
#pragma unroll
      for (int c = 0; c < D; ++c) {
        diff[c] = xv.v[c] - xu.v[c];
        ss = fmaf(diff[c], diff[c], ss);
      }
      float f, gd;
      fn.eval(ss, p0, p1, f, gd);
      const float g = mde_fix_g(gd * inv_p);
      loss += f;
#pragma unroll
      for (int c = 0; c < D; ++c) acc[c] = fmaf(g, diff[c], acc[c]);
    }
    if (grad) {
#pragma unroll
      for (int c = 0; c < D; ++c) acc[c] = mde_group_sum<G>(acc[c]);
      if (lig == 0) store_row<D>(grad, v, acc, grad_scale);
    }
  }
  const double bs = mde_block_sum((double)loss, smem);
  if (threadIdx.x == 0) loss_partials[blockIdx.x] = bs;
}

// ---------------------------------------------------------------- small-d, edge-balanced
// The row-per-group kernel above waits on three dependent memory hops per row (row pointer ->
// neighbour -> x_u) and its waves run as long as their longest row: on graphs with hubs (k-NN
// graphs, scale-free graphs) it is latency-bound (70 us for 2.9M half-edges).  Here a wave takes a
// TILE of MDE_FLAT_T consecutive half-edge positions instead -- every load of the tile is issued
// before the first use, whatever the rows look like -- and sums the contributions of equal rows
// with a segmented scan across the lanes (rows are contiguous runs of positions).  A run that lies
// inside the tile is a finished gradient row.  A row that crosses tile boundaries leaves one
// record per tile (the tile's first run if the row began earlier, its last run if the row goes
// on); k_flat_fixup adds the records of such a row in tile order.  Tiles are aligned to global
// half-edge positions (phase = positions of the rows below row_lo, mod the tile), so a row is
// summed by the same lanes in the same order whichever rank owns it: shards stay bit-equal to
// the single-process result.  No atomics.
template <int D, bool INDIRECT, class Fn>
__global__ __launch_bounds__(MDE_BLOCK) void k_fused_flat(
    int64_t H, int phase, int64_t n_tiles, int row_lo, const int32_t* __restrict__ hrow,
    const int32_t* __restrict__ nbr, const int32_t* __restrict__ eid, const float* __restrict__ a0,
    const float* __restrict__ a1, int a0_scalar, int a1_scalar, const float* __restrict__ X,
    float* __restrict__ grad, float* __restrict__ rec, double* __restrict__ loss_partials, Fn fn,
    float inv_p, float grad_scale) {
  __shared__ double smem[8];
  constexpr int U = MDE_FLAT_U;
  const int lane = threadIdx.x & 63;
  const int64_t wave0 = ((int64_t)blockIdx.x * MDE_BLOCK + threadIdx.x) >> 6;
  const int64_t nwaves = ((int64_t)gridDim.x * MDE_BLOCK) >> 6;
  const EdgeParams<INDIRECT> params(eid, a0, a1, a0_scalar, a1_scalar);
  float loss = 0.0f;
  for (int64_t t = wave0; t < n_tiles; t += nwaves) {
    const int64_t base = t * MDE_FLAT_T - phase;  // local position of the tile's first slot
    int row[U], un[U];
    float p0[U], p1[U];
    bool ok[U];
    // ---- every index / parameter load of the tile
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t h = base + u * 64 + lane;
      ok[u] = h >= 0 && h < H;
      const int64_t hc = ok[u] ? h : 0;
      const int rr = hrow[hc];  // (hc is in range either way: a plain load, the select afterwards)
      row[u] = ok[u] ? rr : -1;
      un[u] = nbr[hc];
      params.load(hc, p0[u], p1[u]);
    }
    // rows of the positions just before and just after the tile: a first run with the former
    // began earlier, a last run with the latter goes on
    const int prev_row = base > 0 ? hrow[base - 1] : -1;
    const int next_row = base + MDE_FLAT_T < H ? hrow[base + MDE_FLAT_T] : -1;
    // ---- every gather of the tile
    VecD<D> xv[U], xu[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      xv[u] = load_row<D>(X, (int64_t)row_lo + (ok[u] ? row[u] : 0));
      xu[u] = load_row<D>(X, un[u]);
    }
    float c[U][D];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      float ss = 0.0f;
#pragma unroll
      for (int k = 0; k < D; ++k) {
        c[u][k] = xv[u].v[k] - xu[u].v[k];
        ss = fmaf(c[u][k], c[u][k], ss);
      }
      float f, gd;
      fn.eval(ss, p0[u], p1[u], f, gd);
      const float g = ok[u] ? mde_fix_g(gd * inv_p) : 0.0f;
      loss += ok[u] ? f : 0.0f;
#pragma unroll
      for (int k = 0; k < D; ++k) c[u][k] *= g;
    }
    if (!grad) continue;
    // ---- rows: segmented inclusive scan per wave iteration, carry from one iteration to the next
    int carry_row = -1, first_row = -1, first_ends = 0;
    float carry[D], first_tot[D];
#pragma unroll
    for (int k = 0; k < D; ++k) carry[k] = first_tot[k] = 0.0f;
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int key = row[u];
#pragma unroll
      for (int off = 1; off < 64; off <<= 1) {
        const int k2 = __shfl_up(key, off, 64);
        const bool same = lane >= off && k2 == key;
#pragma unroll
        for (int k = 0; k < D; ++k) {
          const float v2 = __shfl_up(c[u][k], off, 64);
          c[u][k] += same ? v2 : 0.0f;
        }
      }
      float tot[D];
#pragma unroll
      for (int k = 0; k < D; ++k) tot[k] = c[u][k] + (key == carry_row ? carry[k] : 0.0f);
      // row of the next position: the lane above, or lane 0 of the next iteration / tile
      int nxt = __shfl_down(key, 1, 64);
      const int over = (u + 1 < U) ? __builtin_amdgcn_readlane(row[(u + 1 < U) ? u + 1 : u], 0) : next_row;
      if (lane == 63) nxt = over;
      const bool row_ends = key >= 0 && nxt != key;  // the row's last position
      if (row_ends && key != prev_row) store_row<D>(grad, (int64_t)row_lo + key, tot, grad_scale);
      // the run that began before the tile ends here: its record (at most one lane of the tile)
      const unsigned long long m = __ballot(row_ends && key == prev_row);
      if (m) {
        const int src = __builtin_ctzll(m);
        first_row = __builtin_amdgcn_readlane(key, src);
        first_ends = 1;
#pragma unroll
        for (int k = 0; k < D; ++k) first_tot[k] = __shfl(tot[k], src, 64);
      }
      // lane 63's row goes on: carry its running sum into the next iteration (or out of the tile)
      const int k63 = __builtin_amdgcn_readlane(key, 63);
      carry_row = (k63 >= 0 && over == k63) ? k63 : -1;
#pragma unroll
      for (int k = 0; k < D; ++k) carry[k] = __shfl(tot[k], 63, 64);
    }
    if (lane == 0) {
      // records: [first | last] x (row, ends, sum[4], -, -)
      float* r0 = rec + (size_t)t * 16;
      int last_row = -1;
      if (carry_row >= 0) {
        if (carry_row == prev_row) {  // the whole tile is one row that began earlier and goes on
          first_row = carry_row;
          first_ends = 0;
#pragma unroll
          for (int k = 0; k < D; ++k) first_tot[k] = carry[k];
        } else {
          last_row = carry_row;
        }
      }
      reinterpret_cast<int*>(r0)[0] = first_row;
      reinterpret_cast<int*>(r0)[1] = first_ends;
      reinterpret_cast<int*>(r0)[8] = last_row;
#pragma unroll
      for (int k = 0; k < D; ++k) {
        r0[2 + k] = first_tot[k];
        r0[10 + k] = carry[k];
      }
    }
  }
  const double bs = mde_block_sum((double)loss, smem);
  if (threadIdx.x == 0) loss_partials[blockIdx.x] = bs;
}

// rows that cross tile boundaries: the tile in which such a row ends adds its records in tile order
// (its extra last workgroup adds the loss partials of the fused kernel: no third launch)
template <int D>
__global__ __launch_bounds__(MDE_BLOCK) void k_flat_fixup(int64_t n_tiles, int phase, int row_lo,
                                                          const int32_t* __restrict__ rowptr,
                                                          const float* __restrict__ rec,
                                                          float* __restrict__ grad, float grad_scale,
                                                          double* __restrict__ loss_partials, int nparts,
                                                          double loss_scale, float* __restrict__ loss_out) {
  if (loss_out && blockIdx.x == gridDim.x - 1) {
    __shared__ double smem[8];
    double s = 0.0;
    for (int i = threadIdx.x; i < nparts; i += MDE_BLOCK) s += loss_partials[i];
    const double tot = mde_block_sum(s, smem);
    if (threadIdx.x == 0) {
      *loss_out = (float)(tot * loss_scale);
      loss_partials[MDE_PARTIALS_LOSS_D] = tot * loss_scale;
    }
    return;
  }
  const int64_t t = (int64_t)blockIdx.x * MDE_BLOCK + threadIdx.x;
  if (t >= n_tiles) return;
  const float* rt = rec + (size_t)t * 16;
  const int r = reinterpret_cast<const int*>(rt)[0];
  if (r < 0 || reinterpret_cast<const int*>(rt)[1] == 0) return;
  const int64_t ta = ((int64_t)rowptr[r] + phase) / MDE_FLAT_T;  // the tile the row begins in
  float s[D];
#pragma unroll
  for (int k = 0; k < D; ++k) s[k] = rec[(size_t)ta * 16 + 10 + k];
  for (int64_t q = ta + 1; q <= t; ++q) {
#pragma unroll
    for (int k = 0; k < D; ++k) s[k] += rec[(size_t)q * 16 + 2 + k];
  }
  const int64_t v = (int64_t)row_lo + r;
#pragma unroll
  for (int k = 0; k < D; ++k) grad[v * D + k] = s[k] * grad_scale;
}

// ---------------------------------------------------------------- launch
static int pick_group(float avg_degree) {
  // MDE_GROUP (tuning experiments) is read once per process: tests/test_gpu_kernels.py sets it for
  // a child process and relies on later changes of the environment not reaching the library
  static const int group_override = env_int("MDE_GROUP", -1);
  if (group_override > 0) return group_override;
  // few, very long rows (dense problems such as all-pairs distance graphs): widen the group so
  // that the grid still fills the chip
  if (avg_degree >= 1024.f) return 64;
  if (avg_degree >= 256.f) return 32;
  if (avg_degree >= 48.f) return 16;
  if (avg_degree >= 20.f) return 8;
  return 4;
}

template <int D, int G, bool IND, class Fn>
static int launch_small_g(FusedArgs& A, const Fn& fn) {
  const mde_plan* P = A.plan;
  const int nrows = fused_row_grid(A, G);
  hipLaunchKernelGGL((k_fused_small<D, G, IND, Fn>), dim3(A.nblocks), dim3(MDE_BLOCK), 0, A.st, nrows,
                     (int)mde_plan_row_lo(P), mde_plan_rowptr(P), mde_plan_nbr(P), mde_plan_eid(P), A.a0, A.a1,
                     A.a0_scalar, A.a1_scalar, A.X, A.grad, A.partials, fn, A.inv_p, A.grad_scale);
  MDE_LAUNCH_CHECK();
  return MDE_OK;
}

template <int D, bool IND, class Fn>
static int launch_flat(FusedArgs& A, const Fn& fn) {
  mde_plan* P = const_cast<mde_plan*>(A.plan);
  int rc = mde_plan_flat(P, A.st);
  if (rc != MDE_OK) return rc;
  const int64_t nloc = P->row_hi - P->row_lo;
  const int phase = (int)(P->h_offset % MDE_FLAT_T);
  float* gloc = A.grad ? A.grad + (size_t)P->row_lo * D : nullptr;
  if (A.grad && P->has_empty) MDE_HIP(hipMemsetAsync(gloc, 0, (size_t)nloc * D * sizeof(float), A.st));
  const int nb = mde_grid(P->n_tiles * 64, MDE_BLOCK, 2048);
  A.nblocks = nb;
  hipLaunchKernelGGL((k_fused_flat<D, IND, Fn>), dim3(nb), dim3(MDE_BLOCK), 0, A.st, P->H, phase, P->n_tiles,
                     (int)P->row_lo, P->hrow, P->nbr, P->eid, A.a0, A.a1, A.a0_scalar, A.a1_scalar, A.X, A.grad,
                     P->flat_rec, A.partials, fn, A.inv_p, A.grad_scale);
  MDE_LAUNCH_CHECK();
  if (A.grad) {
    const unsigned fb = (unsigned)((P->n_tiles + MDE_BLOCK - 1) / MDE_BLOCK);
    hipLaunchKernelGGL(k_flat_fixup<D>, dim3(fb + (A.loss_out ? 1u : 0u)), dim3(MDE_BLOCK), 0, A.st, P->n_tiles, phase,
                       (int)P->row_lo, P->rowptr, P->flat_rec, A.grad, A.grad_scale, A.partials, nb, A.loss_scale,
                       A.loss_out);
    MDE_LAUNCH_CHECK();
    if (A.loss_out) A.loss_done = 1;
  }
  return MDE_OK;
}

template <int D, bool IND, class Fn>
static int launch_small(FusedArgs& A, const Fn& fn) {
  // sparse graphs (the usual case): edge-balanced tiles.  Dense problems (hundreds of half-edges
  // per row on average, e.g. all-pairs distance graphs) keep a row per 32 / 64 lanes: enough loads
  // in flight per row, and no segmented scan (config 3: 0.67 vs 0.77 ms per evaluation)
  // MDE_FLAT: unset / 1 the edge-balanced kernel on sparse graphs, 2 always, 0 never
  const int fm = env_int("MDE_FLAT", 1);
  if (fm != 0 && A.plan->H > 0 && (fm == 2 || A.plan->avg_degree < 256.f))
    return launch_flat<D, IND, Fn>(A, fn);
  switch (pick_group(A.plan->avg_degree)) {
    case 4: return launch_small_g<D, 4, IND, Fn>(A, fn);
    case 8: return launch_small_g<D, 8, IND, Fn>(A, fn);
    case 32: return launch_small_g<D, 32, IND, Fn>(A, fn);
    case 64: return launch_small_g<D, 64, IND, Fn>(A, fn);
    default: return launch_small_g<D, 16, IND, Fn>(A, fn);
  }
}
template <bool IND, class Fn>
static int launch_small_d(FusedArgs& A, const Fn& fn) {
  switch (A.d) {
    case 1: return launch_small<1, IND, Fn>(A, fn);
    case 2: return launch_small<2, IND, Fn>(A, fn);
    case 3: return launch_small<3, IND, Fn>(A, fn);
    default: return launch_small<4, IND, Fn>(A, fn);
  }
}
// (the dedicated functors exist for d = 2 and 3 only)
template <class Fn>
static int launch_small_23(FusedArgs& A, const Fn& fn) {
  if (A.d == 2) return launch_small<2, false, Fn>(A, fn);
  return launch_small<3, false, Fn>(A, fn);
}

// dedicated instantiations for the functions the recipes use by default; everything else
// goes through the universal run-time functor.
int mde_fused_small(FusedArgs& A, const mde_func* f) {
  const MdeFuncArgs a = func_args(f);
  if (A.d == 2 || A.d == 3) {
    const int ea = mde_exp_class(f->s0), en = mde_exp_class(f->n0);
    if (f->kind_neg == MDE_F_NONE) {
      if (f->kind == MDE_F_QUADRATIC) return launch_small_23(A, FnSingle<MDE_F_QUADRATIC, 0>{a});
      if (f->kind == MDE_F_LOG1P && ea == 2) return launch_small_23(A, FnSingle<MDE_F_LOG1P, 2>{a});
      if (f->kind == MDE_F_L_QUADRATIC) return launch_small_23(A, FnSingle<MDE_F_L_QUADRATIC, 0>{a});
      if (f->kind == MDE_F_L_ABSOLUTE) return launch_small_23(A, FnSingle<MDE_F_L_ABSOLUTE, 0>{a});
      if (f->kind == MDE_F_L_HUBER) return launch_small_23(A, FnSingle<MDE_F_L_HUBER, 0>{a});
    } else if (f->kind == MDE_F_LOG1P && ea == 2) {
      if (f->kind_neg == MDE_F_LOG && en == 1)
        return launch_small_23(A, FnPushPull<MDE_F_LOG1P, 2, MDE_F_LOG, 1>{a});
      if (f->kind_neg == MDE_F_LOGRATIO && en == 3)
        return launch_small_23(A, FnPushPull<MDE_F_LOG1P, 2, MDE_F_LOGRATIO, 3>{a});
    }
  }
  return launch_small_d<false>(A, FnRuntime{a});
}

int mde_fused_small_unfused(FusedArgs& A, mde_unfused which) {
  if (which == MDE_UNFUSED_SCATTER) return launch_small_d<true>(A, FnScatter{});
  return launch_small_d<true>(A, FnDistBackward{});
}

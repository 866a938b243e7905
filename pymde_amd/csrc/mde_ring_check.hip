// mde_ring_check.hip -- device self-checks of a built LDS-ring layout (mde_plan_ring_check): the lane-stable pairs
// the kernel's accumulator read-ahead relies on, and who adds an edge's loss term.  A unit of its own: only a
// process that asks for the check loads these kernels.
#include "mde_ring.h"

// One wave per pair of iterations (it, it + 1), it even: a real row (address below the dummy rows) of the second
// iteration that the first holds on ANOTHER lane breaks the kernel's accumulator read-ahead.  out[0] += such
// entries, out[1] += real rows held by both iterations (on one lane), out[2] += pairs checked.
__global__ __launch_bounds__(MDE_BLOCK) void k_ring_pair_check(int64_t npairs, const uint32_t* __restrict__ packed, int d, int R,
                                                               unsigned long long* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int64_t nw = ((int64_t)gridDim.x * MDE_BLOCK) >> 6;
  const uint32_t mask = d == 2 ? 0xfff8u : 0xfffcu, dummy = (uint32_t)R * 4u * (uint32_t)d;
  unsigned long long split = 0, shared = 0, pairs = 0;
  for (int64_t pr = ((int64_t)blockIdx.x * MDE_BLOCK + threadIdx.x) >> 6; pr < npairs; pr += nw) {
    const int64_t it = 2 * pr;
    const size_t base = ((size_t)(it >> 2) * 64 + (size_t)lane) * 4 + (size_t)(it & 3);
    const uint32_t ra = packed[base] & mask, rb = packed[base + 1] & mask;
    int found = -1;
    for (int k = 0; k < 64; ++k)
      if ((uint32_t)__builtin_amdgcn_readlane((int)ra, k) == rb) found = k;
    const bool real = rb < dummy;
    split += __popcll(__ballot(real && found >= 0 && found != lane));
    shared += __popcll(__ballot(real && found >= 0));
    ++pairs;
  }
  if (lane == 0) {
    atomicAdd(&out[0], split);
    atomicAdd(&out[1], shared);
    atomicAdd(&out[2], pairs);
  }
}

// Who adds an edge's loss term, as the KERNEL will decide it (layouts that are not permuted).  One wave per iteration:
// every real entry adds 0x10000 (seen) + 1 (when its term is added here: block class 1, or class 2 and the per-lane
// test -- bit 31 of the packed word at d = 2, the rule recomputed from the addresses otherwise) to its edge's word of
// `hist`.  out[4] += entries whose bit 31 (d = 2) disagrees with ring_counts recomputed from (row, column), padding
// entries with the bit set included.
__global__ __launch_bounds__(MDE_BLOCK) void k_ring_loss_mark(int64_t nit, int nseg, const int32_t* __restrict__ wave_iter,
                                                              const uint32_t* __restrict__ hdr, const uint32_t* __restrict__ packed,
                                                              const int32_t* __restrict__ peid, int d, int R, int Q, int C, int S,
                                                              int ring_off, int row_lo, int loss_band, int64_t p,
                                                              uint32_t* __restrict__ hist, unsigned long long* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int64_t nw = ((int64_t)gridDim.x * MDE_BLOCK) >> 6;
  const uint32_t cbytes = (uint32_t)C * 4u * (uint32_t)d;
  unsigned long long mism = 0;
  for (int64_t it = ((int64_t)blockIdx.x * MDE_BLOCK + threadIdx.x) >> 6; it < nit; it += nw) {
    int lo = 0, hi = nseg;  // wave_iter[lo] <= it < wave_iter[hi]
    while (hi - lo > 1) {
      const int mid = (lo + hi) >> 1;
      if ((int64_t)wave_iter[mid] <= it) lo = mid; else hi = mid;
    }
    const int rb = (lo / MDE_RING_NCW) / Q;
    const size_t idx = ((size_t)(it >> 2) * 64 + (size_t)lane) * 4 + (size_t)(it & 3);
    const uint32_t w = packed[idx];
    const int32_t e = peid[idx];
    const bool bit = d == 2 && (w & MDE_RING_COUNTS_BIT) != 0u;
    if (e < 0 || (int64_t)e >= p) {
      mism += bit ? 1u : 0u;
      continue;
    }
    const uint32_t hm = hdr[MDE_RING_HW * it];
    const uint32_t bcls = hdr[MDE_RING_HW * (it & ~(int64_t)3) + 3] & 3u;
    const uint32_t rowaddr = d == 2 ? (w & 0xfff8u) : (w & 0xfffcu);
    const uint32_t coladdr = d == 2 ? ((w >> 13) & 0x3fff8u) : ((w >> 14) & 0x3fffcu);
    const uint32_t off = coladdr - (uint32_t)ring_off;
    const uint32_t slot = off / cbytes, cidx = (off - slot * cbytes) / (4u * (uint32_t)d);
    const uint32_t ms = hm % (uint32_t)S;
    const uint32_t j = hm + (slot >= ms ? slot - ms : slot + (uint32_t)S - ms);
    const uint32_t u = j * (uint32_t)C + cidx;
    const uint32_t v = (uint32_t)row_lo + (uint32_t)rb * (uint32_t)R + rowaddr / (4u * (uint32_t)d);
    const bool rule = ring_counts(v, u, (uint32_t)loss_band);
    if (d == 2 && bit != rule) ++mism;
    const bool here = bcls == 0u ? false : (bcls == 1u ? true : (d == 2 ? bit : rule));
    atomicAdd(&hist[e], 0x10000u + (here ? 1u : 0u));
  }
  mism = mde_wave_sum(mism);
  if (lane == 0 && mism) atomicAdd(&out[4], mism);
}

// ... and the peeled hub rows' half-edges (k_hub_rows decides with ring_counts): one workgroup per segment
__global__ __launch_bounds__(MDE_BLOCK) void k_ring_loss_mark_hub(const int32_t* __restrict__ hub_rows, const int32_t* __restrict__ hub_seg,
                                                                  int row_lo, const int32_t* __restrict__ nbr,
                                                                  const int32_t* __restrict__ eid, int loss_band, int64_t p,
                                                                  uint32_t* __restrict__ hist) {
  const int sgi = blockIdx.x;
  const int hi = hub_seg[4 * sgi], beg = hub_seg[4 * sgi + 1], end = hub_seg[4 * sgi + 2];
  const uint32_t v = (uint32_t)row_lo + (uint32_t)hub_rows[hi];
  for (int h = beg + (int)threadIdx.x; h < end; h += MDE_BLOCK) {
    const int32_t e = eid[h];
    if (e < 0 || (int64_t)e >= p) continue;
    atomicAdd(&hist[e], 0x10000u + (ring_counts(v, (uint32_t)nbr[h], (uint32_t)loss_band) ? 1u : 0u));
  }
}

// out[3] += edges whose loss term is not added exactly once (of the edges with both entries in this plan; an edge with
// one entry here -- a sharded plan -- may add at most one), out[5] += edges with both entries here
__global__ __launch_bounds__(MDE_BLOCK) void k_ring_loss_count(int64_t p, const uint32_t* __restrict__ hist,
                                                               unsigned long long* __restrict__ out) {
  unsigned long long bad = 0, both = 0;
  for (int64_t e = (int64_t)blockIdx.x * MDE_BLOCK + threadIdx.x; e < p; e += (int64_t)gridDim.x * MDE_BLOCK) {
    const uint32_t seen = hist[e] >> 16, c = hist[e] & 0xffffu;
    both += seen == 2u;
    bad += seen > 2u || (seen == 2u && c != 1u) || (seen == 1u && c > 1u);
  }
  bad = mde_wave_sum(bad);
  both = mde_wave_sum(both);
  if ((threadIdx.x & 63) == 0) {
    if (bad) atomicAdd(&out[3], bad);
    if (both) atomicAdd(&out[5], both);
  }
}

extern "C" int mde_plan_ring_check(const mde_plan* plan, int64_t* out_host, void* stream) {
  if (!plan || !out_host) return MDE_E_INVALID;
  const mde_ring_layout& L = plan->ring;
  for (int i = 0; i < 8; ++i) out_host[i] = 0;
  if (!L.packed || L.n_iters == 0) return MDE_OK;
  hipStream_t st = mde_stream(stream);
  MdeDeviceBuf<unsigned long long> dout;
  MdeDeviceBuf<uint32_t> hist;
  const bool loss_check = !L.count_all && plan->p > 0;
  hipError_t e = dout.alloc(8 * sizeof(unsigned long long));
  if (e == hipSuccess) e = hipMemsetAsync(dout, 0, 8 * sizeof(unsigned long long), st);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(k_ring_pair_check, dim3(mde_grid(L.n_iters / 2 * 64, MDE_BLOCK, 4096)), dim3(MDE_BLOCK), 0, st,
                       L.n_iters / 2, L.packed, L.d, L.rows_per_block, dout);
    e = hipGetLastError();
  }
  if (e == hipSuccess && loss_check) e = hist.alloc((size_t)plan->p * sizeof(uint32_t));
  if (e == hipSuccess && loss_check) e = hipMemsetAsync(hist, 0, (size_t)plan->p * sizeof(uint32_t), st);
  if (e == hipSuccess && loss_check) {
    hipLaunchKernelGGL(k_ring_loss_mark, dim3(mde_grid(L.n_iters * 64, MDE_BLOCK, 8192)), dim3(MDE_BLOCK), 0, st, L.n_iters,
                       L.n_row_blocks * L.col_groups * MDE_RING_NCW, L.wave_iter, L.hdr, L.packed, L.eid, L.d, L.rows_per_block,
                       L.col_groups, L.chunk_cols, L.slots, L.ring_off, (int)plan->row_lo, L.loss_band, plan->p, hist, dout);
    e = hipGetLastError();
  }
  if (e == hipSuccess && loss_check && L.n_hub_segs > 0) {
    hipLaunchKernelGGL(k_ring_loss_mark_hub, dim3(L.n_hub_segs), dim3(MDE_BLOCK), 0, st, L.hub_rows, L.hub_seg, (int)plan->row_lo,
                       plan->nbr, plan->eid, L.loss_band, plan->p, hist);
    e = hipGetLastError();
  }
  if (e == hipSuccess && loss_check) {
    hipLaunchKernelGGL(k_ring_loss_count, dim3(mde_grid(plan->p, MDE_BLOCK, 4096)), dim3(MDE_BLOCK), 0, st, plan->p, hist, dout);
    e = hipGetLastError();
  }
  unsigned long long h[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (e == hipSuccess) e = hipMemcpyAsync(h, dout, sizeof(h), hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e != hipSuccess) {
    mde_set_error("mde_plan_ring_check: %s", hipGetErrorString(e));
    return MDE_E_HIP;
  }
  for (int i = 0; i < 8; ++i) out_host[i] = (int64_t)h[i];
  return MDE_OK;
}

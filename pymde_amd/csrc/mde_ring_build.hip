// mde_ring_build.hip -- builds the LDS-ring layout (layout 1) of a plan: the builder's kernels, then build_ring as a
// list of stages over one RingBuild state.  What the layout is for: the essay at the top of mde_ring.hip; which rows
// go where: mde_ring_rows.h.  A unit of its own: the build loads neither the parameter, check and hub kernels nor
// (mde_ring.h) the ring kernel's instantiations.
#include <algorithm>
#include <chrono>
#include <vector>

#include "mde_ring_layout.h"

// ---------------------------------------------------------------- layout construction
// Row -> consumer wave map of a workgroup (row block rb, column group g).  A row has ONE wave (nobody else
// touches its accumulator), but WHICH wave is free: the packed words carry absolute LDS addresses, so a
// wave's ownership of a row exists only as "which stream its entries are in".  Rounds 2-4 cut the block into 8
// contiguous row ranges of equal half-edge count.  On a random graph the entries a range finds in a chunk are
// Poisson, the ranges' positions along the column sweep drift apart like random walks (at equal iteration
// index the 8 waves of a config-4 workgroup are spread over 5 chunks on average, 8 at the 90th percentile),
// and a ring slot is free only when ALL consumers are past it: with 9 slots and a 5-chunk pair window the
// fast waves wait for the slow ones most of the time (a third of the consumer loop was polling).
// Here the rows are dealt to the waves one by one, greedily: the column sweep of the group is cut into
// MDE_RING_BUCKETS buckets, P_w[b] is the number of entries wave w holds in buckets <= b, and a row with
// prefix counts c[b] goes to the wave that minimises sum_b (P_w[b] - mean_w P[b]) c[b] -- the steepest descent
// of sum_w sum_b (P_w[b] - mean)^2.  Every wave then reaches every bucket boundary with (almost) the same
// number of entries behind it: spread 1.9 chunks on average, 3 at the 90th percentile (simulation and
// MDE_RING_STATS), which the ring's slack of 4 covers.  One wave per workgroup, rows in order.
// wmap[(rb * Q + g) * R + local row] = wave | rank of the row inside its wave << 8; wrows[stream] = rows.
#ifndef MDE_RING_BUCKETS
#define MDE_RING_BUCKETS 32
#endif
__global__ __launch_bounds__(64) void k_ring_assign(int nloc, int R, int Q, int NC, int C, int contiguous,
                                                    const int32_t* __restrict__ rowptr,
                                                    const int32_t* __restrict__ nbr, uint32_t* __restrict__ wmap,
                                                    int32_t* __restrict__ wrows) {
  constexpr int B = MDE_RING_BUCKETS, NCWP = MDE_RING_NCW <= 8 ? 8 : 16, LPW = 64 / NCWP, BPL = B / LPW;
  static_assert(MDE_RING_NCW <= 16 && B % LPW == 0 && B <= 64, "lane map of k_ring_assign");
  __shared__ int hist[B];
  __shared__ float cpre[B];
  const int wg = blockIdx.x, rb = wg / Q, g = wg % Q, lane = threadIdx.x;
  const int j_lo = (int)(((int64_t)g * NC + Q - 1) / Q), j_hi = (int)(((int64_t)(g + 1) * NC + Q - 1) / Q);
  const int nj = max(1, j_hi - j_lo);
  const int r0 = rb * R, nr = min(R, nloc - r0);
  const int w = lane / LPW, bg = lane % LPW;
  uint32_t* out = wmap + (size_t)wg * R;
  if (contiguous) {
    // (MDE_RING_ASSIGN=0, design comparison: the contiguous ranges of equal half-edge count of rounds 2-4)
    const int64_t lo = rowptr[r0], hi = rowptr[r0 + nr];
    int bd[MDE_RING_NCW + 1];
    for (int t = 0; t <= MDE_RING_NCW; ++t) {
      const int64_t target = lo + ((hi - lo) * t) / MDE_RING_NCW;
      int a = r0, b = r0 + nr;
      while (a < b) {
        const int mid = (a + b) >> 1;
        if (rowptr[mid] >= target) b = mid; else a = mid + 1;
      }
      bd[t] = (t == MDE_RING_NCW) ? r0 + nr : a;
    }
    for (int r = lane; r < nr; r += 64) {
      int ww = 0;
      for (int t = 1; t < MDE_RING_NCW; ++t) ww += (bd[t] <= r0 + r);
      out[r] = (uint32_t)ww | ((uint32_t)(r0 + r - bd[ww]) << 8);
    }
    if (lane < MDE_RING_NCW) wrows[wg * MDE_RING_NCW + lane] = bd[lane + 1] - bd[lane];
    return;
  }
  float P[BPL], T[BPL];
#pragma unroll
  for (int k = 0; k < BPL; ++k) P[k] = T[k] = 0.0f;
  int myrows = 0;
  for (int r = 0; r < nr; ++r) {
    const int beg = rowptr[r0 + r], end = rowptr[r0 + r + 1];
    if (lane < B) hist[lane] = 0;
    __syncthreads();
    for (int q = beg + lane; q < end; q += 64) {
      const int j = nbr[q] / C;
      if (j >= j_lo && j < j_hi) atomicAdd(&hist[(int)(((int64_t)(j - j_lo) * B) / nj)], 1);
    }
    __syncthreads();
    int h = lane < B ? hist[lane] : 0;
#pragma unroll
    for (int o = 1; o < B; o <<= 1) {
      const int t = __shfl_up(h, o, 64);
      if (lane >= o) h += t;
    }
    if (lane < B) cpre[lane] = (float)h;
    __syncthreads();
    float c[BPL], cost = 0.0f;
#pragma unroll
    for (int k = 0; k < BPL; ++k) {
      c[k] = cpre[bg * BPL + k];
      cost = fmaf(P[k] - T[k] * (1.0f / MDE_RING_NCW), c[k], cost);
    }
#pragma unroll
    for (int o = 1; o < LPW; o <<= 1) cost += __shfl_xor(cost, o, 64);
    // the best wave: lowest cost, then fewest rows (rows without entries in this group are dealt evenly), then lowest id
    float bc = w < MDE_RING_NCW ? cost : 3.0e38f;
    int bn = myrows, bw = w;
#pragma unroll
    for (int o = LPW; o < 64; o <<= 1) {
      const float oc = __shfl_xor(bc, o, 64);
      const int on = __shfl_xor(bn, o, 64), ow = __shfl_xor(bw, o, 64);
      const bool take = oc < bc || (oc == bc && (on < bn || (on == bn && ow < bw)));
      bc = take ? oc : bc;
      bn = take ? on : bn;
      bw = take ? ow : bw;
    }
    if (lane == 0) out[r] = (uint32_t)bw | ((uint32_t)bn << 8);
#pragma unroll
    for (int k = 0; k < BPL; ++k) {
      T[k] += c[k];
      if (w == bw) P[k] += c[k];
    }
    myrows += (w == bw);
  }
  if (bg == 0 && w < MDE_RING_NCW) wrows[wg * MDE_RING_NCW + w] = myrows;
}

// key = ((rb * Q + column group) * NCW + wave) << JB | chunk; CSR order (row, edge id) is kept
// inside equal keys by the stable sort
__global__ __launch_bounds__(MDE_BLOCK) void k_ring_keys(int nrows, const int32_t* __restrict__ rowptr,
                                                         const int32_t* __restrict__ nbr,
                                                         const uint32_t* __restrict__ wmap, int R, int Q,
                                                         int NC, int C, int JB, uint32_t* __restrict__ keys,
                                                         uint32_t* __restrict__ vals, int32_t* __restrict__ hrow) {
  constexpr int G = 16;  // (>= the largest Q: lane t of a group holds the row's wave in column group t)
  const int lig = threadIdx.x & (G - 1);
  const int group = (blockIdx.x * MDE_BLOCK + threadIdx.x) / G;
  const int ngroups = (gridDim.x * MDE_BLOCK) / G;
  const int rmax = ((nrows + ngroups - 1) / ngroups) * ngroups;  // (every group runs the same trips: shuffles below)
  for (int r = group; r < rmax; r += ngroups) {
    const bool has = r < nrows;
    const int beg = has ? rowptr[r] : 0, end = has ? rowptr[r + 1] : 0;
    const int rb = has ? r / R : 0;
    const uint32_t wv = (has && lig < Q) ? (wmap[((size_t)rb * Q + lig) * R + (r - rb * R)] & 0xffu) : 0u;
    for (int q0 = beg; q0 < end; q0 += G) {
      const int q = q0 + lig;
      const bool in = q < end;
      const uint32_t j = in ? (uint32_t)(nbr[q] / C) : 0u;
      const uint32_t g = (uint32_t)(((uint64_t)j * (uint64_t)Q) / (uint64_t)NC);
      const uint32_t w = (uint32_t)__shfl((int)wv, (int)g, G);
      if (in) {
        keys[q] = ((((uint32_t)rb * (uint32_t)Q + g) * MDE_RING_NCW + w) << JB) | j;
        vals[q] = (uint32_t)q;
        hrow[q] = r;
      }
    }
  }
}

// ---- round 6: layouts with PEELED hub rows and / or PERMUTED row blocks (plan_rows, mde_ring_rows.h)
// row_slot[r] = rb * R + s: LDS slot s of row block rb holds local row r; -1: the row is peeled off to the hub
// kernel.  slot_cum[t] = half-edges in the slots below t.  The builder kernels below are the slot-indexed twins of
// k_ring_assign (contiguous mode) and k_ring_keys; downstream of them `hrow` holds SLOTS, and k_ring_meta /
// k_ring_pack run unchanged (slot - rb * R is the address of the row's x_v and accumulator).
__global__ __launch_bounds__(64) void k_ring_assign_slots(int R, int Q, const int32_t* __restrict__ slot_cum,
                                                          uint32_t* __restrict__ wmap, int32_t* __restrict__ wrows) {
  const int wg = blockIdx.x, rb = wg / Q, lane = threadIdx.x;
  const int s0 = rb * R;
  uint32_t* out = wmap + (size_t)wg * R;
  const int64_t lo = slot_cum[s0], hi = slot_cum[s0 + R];
  int bd[MDE_RING_NCW + 1];
  for (int t = 0; t <= MDE_RING_NCW; ++t) {
    const int64_t target = lo + ((hi - lo) * t) / MDE_RING_NCW;
    int a = s0, b = s0 + R;
    while (a < b) {
      const int mid = (a + b) >> 1;
      if (slot_cum[mid] >= target) b = mid; else a = mid + 1;
    }
    bd[t] = (t == MDE_RING_NCW) ? s0 + R : a;
  }
  for (int r = lane; r < R; r += 64) {
    int ww = 0;
    for (int t = 1; t < MDE_RING_NCW; ++t) ww += (bd[t] <= s0 + r);
    out[r] = (uint32_t)ww | ((uint32_t)(s0 + r - bd[ww]) << 8);
  }
  if (lane < MDE_RING_NCW) wrows[wg * MDE_RING_NCW + lane] = bd[lane + 1] - bd[lane];
}

// in: hrow[q] = local row of CSR position q (k_ring_hrow).  out: the stream key of q (the sentinel stream `nseg`,
// which no wave walks, for the entries of peeled rows), vals[q] = q, hrow[q] = the row's slot
__global__ __launch_bounds__(MDE_BLOCK) void k_ring_keys_slots(int64_t H, const int32_t* __restrict__ nbr,
                                                               const int32_t* __restrict__ row_slot,
                                                               const uint32_t* __restrict__ wmap, int R, int Q, int NC, int C,
                                                               int JB, uint32_t nseg, uint32_t* __restrict__ keys,
                                                               uint32_t* __restrict__ vals, int32_t* __restrict__ hrow) {
  for (int64_t q = (int64_t)blockIdx.x * MDE_BLOCK + threadIdx.x; q < H; q += (int64_t)gridDim.x * MDE_BLOCK) {
    const int sl = row_slot[hrow[q]];
    vals[q] = (uint32_t)q;
    if (sl < 0) {
      keys[q] = nseg << JB;
      hrow[q] = 0;
      continue;
    }
    const int rb = sl / R;
    const uint32_t j = (uint32_t)(nbr[q] / C);
    const uint32_t g = (uint32_t)(((uint64_t)j * (uint64_t)Q) / (uint64_t)NC);
    const uint32_t w = wmap[((size_t)rb * Q + g) * R + (sl - rb * R)] & 0xffu;
    keys[q] = ((((uint32_t)rb * (uint32_t)Q + g) * MDE_RING_NCW + w) << JB) | j;
    hrow[q] = sl;
  }
}
__global__ __launch_bounds__(MDE_BLOCK) void k_ring_rows_to_slots(int64_t H, const int32_t* __restrict__ row_slot,
                                                                  int32_t* __restrict__ hrow) {
  for (int64_t q = (int64_t)blockIdx.x * MDE_BLOCK + threadIdx.x; q < H; q += (int64_t)gridDim.x * MDE_BLOCK)
    hrow[q] = max(row_slot[hrow[q]], 0);
}

__global__ __launch_bounds__(MDE_BLOCK) void k_ring_gather_u32(int64_t H, const uint32_t* __restrict__ idx,
                                                               const uint32_t* __restrict__ in,
                                                               uint32_t* __restrict__ out) {
  for (int64_t h = (int64_t)blockIdx.x * MDE_BLOCK + threadIdx.x; h < H; h += (int64_t)gridDim.x * MDE_BLOCK)
    out[h] = in[idx[h]];
}

// hrow[q] = local row of CSR position q
__global__ __launch_bounds__(MDE_BLOCK) void k_ring_hrow(int nrows, const int32_t* __restrict__ rowptr,
                                                         int32_t* __restrict__ hrow) {
  constexpr int G = 16;
  const int lig = threadIdx.x & (G - 1);
  const int group = (blockIdx.x * MDE_BLOCK + threadIdx.x) / G;
  const int ngroups = (gridDim.x * MDE_BLOCK) / G;
  for (int r = group; r < nrows; r += ngroups)
    for (int q = rowptr[r] + lig; q < rowptr[r + 1]; q += G) hrow[q] = r;
}

// seg[t] = first sorted position whose stream id (key >> JB) >= t, t = 0..nseg
__global__ __launch_bounds__(MDE_BLOCK) void k_ring_seg(int64_t H, uint32_t nseg, int JB,
                                                        const uint32_t* __restrict__ keys,
                                                        int32_t* __restrict__ seg) {
  for (int64_t h = (int64_t)blockIdx.x * MDE_BLOCK + threadIdx.x; h <= H;
       h += (int64_t)gridDim.x * MDE_BLOCK) {
    const int64_t prev = (h == 0) ? -1 : (int64_t)(keys[h - 1] >> JB);
    int64_t cur = (h == H) ? (int64_t)nseg : (int64_t)(keys[h] >> JB);
    if (cur > (int64_t)nseg) cur = nseg;
    for (int64_t t = prev + 1; t <= cur; ++t) seg[t] = (int32_t)h;
  }
}

// Cut each (block, group, wave) stream into wave iterations: up to 64 entries, taken in stream
// order, whose chunks lie within SPAN of the oldest one (the ring holds them all at once).
//   * The rows of an iteration are DISTINCT (always): every lane does its own LDS read-add-write
//     of its row's accumulator, nothing is folded across lanes.  An entry whose row is taken waits
//     for the next iteration (a row's entries still reach its accumulator in stream order); a hub
//     row therefore costs padding, and mde_plan_layout gives up on the ring when that gets out of
//     hand (auto mode).
//   * Bank classes: an iteration takes at most `cap` entries per row bank class and per column
//     bank class (the 8-byte LDS slot mod 32 at d = 2) -- with the lane placement of k_ring_pack
//     every 32-lane pass of its LDS reads is then at most cap/2 deep (tools/sched_sim.cpp: cap 4
//     costs ~1 % padding and takes the modelled LDS clocks per iteration from 26 to 22; the
//     unplaced, uncapped layout of round 2 measured ~40).  An entry that lost `force` times goes
//     out regardless of the caps (never against a taken row).
// Lanes freed by waiting entries are refilled from the stream (a few rounds), so iterations stay
// full.  One wave per stream; FILL = false counts the iterations, FILL = true writes, per iteration,
// the sorted positions of its entries, their number and the oldest chunk still needed (it_m).
#ifndef MDE_RING_FORCE
#define MDE_RING_FORCE 3
#endif
#ifndef MDE_RING_CARRY
#define MDE_RING_CARRY 256  // waiting entries a stream can hold
#endif
#ifndef MDE_RING_ROUNDS
#define MDE_RING_ROUNDS 6    // batches of new entries offered per iteration
#endif
__host__ __device__ constexpr int ring_cls_shift(int d) { return d == 2 ? 3 : (d == 4 ? 4 : 2); }
__host__ __device__ constexpr int ring_cls_mask(int d) { return d == 4 ? 15 : 31; }
// meta[pos] for every sorted position: rank of the row inside its wave (bits 15:0) | row bank class (23:16) | column bank
// class (31:24) -- everything the scheduler needs of an entry besides its chunk (keys[pos] & JM), in
// stream order: the scheduler's loads are contiguous (round 3 chased pos -> vals -> hrow / nbr, three
// dependent random loads per candidate: 2 x 43 ms at config 4)
__global__ __launch_bounds__(MDE_BLOCK) void k_ring_meta(int64_t H, const uint32_t* __restrict__ keys,
                                                         const uint32_t* __restrict__ vals,
                                                         const int32_t* __restrict__ hrow,
                                                         const int32_t* __restrict__ nbr,
                                                         const uint32_t* __restrict__ wmap, int JB, int R, int Q, int d,
                                                         uint32_t* __restrict__ meta) {
  const int sh = ring_cls_shift(d), cm = ring_cls_mask(d), rowbytes = 4 * d;
  for (int64_t pos = (int64_t)blockIdx.x * MDE_BLOCK + threadIdx.x; pos < H; pos += (int64_t)gridDim.x * MDE_BLOCK) {
    const uint32_t q = vals[pos];
    const int wg = (int)((keys[pos] >> JB) / MDE_RING_NCW), rb = wg / Q;
    const uint32_t row = (uint32_t)(hrow[q] - rb * R);
    const uint32_t rc = ((row * (uint32_t)rowbytes) >> sh) & (uint32_t)cm;
    const uint32_t cc = (((uint32_t)nbr[q] * (uint32_t)rowbytes) >> sh) & (uint32_t)cm;  // (chunks start on class 0)
    meta[pos] = (wmap[(size_t)wg * R + row] >> 8) | (rc << 16) | (cc << 24);
  }
}

template <bool FILL>
__global__ __launch_bounds__(64) void k_ring_schedule(int nseg, const int32_t* __restrict__ seg,
                                                      const int32_t* __restrict__ wrows,
                                                      const uint32_t* __restrict__ keys,
                                                      const uint32_t* __restrict__ meta, uint32_t JM, int SPAN,
                                                      int R, int Q, int NC, int d, int cap, int bail_factor,
                                                      int32_t* __restrict__ iters,
                                                      const int32_t* __restrict__ iter_base,
                                                      int32_t* __restrict__ it_ent, int32_t* __restrict__ it_cnt,
                                                      int32_t* __restrict__ it_m, int flag_rows,
                                                      const int32_t* __restrict__ caps) {
  extern __shared__ int flag[];                  // [flag_rows] per row of the WAVE: priority of the entry that holds it
  __shared__ int cq_pos[2][MDE_RING_CARRY];      // waiting entries (sorted position), double buffered,
  __shared__ uint32_t cq_meta[2][MDE_RING_CARRY];  // ... their meta word,
  __shared__ int cq_chunk[2][MDE_RING_CARRY];    // ... their chunk
  __shared__ int cq_age[2][MDE_RING_CARRY];
  __shared__ int em[64], em_row[64];             // entries of the iteration being formed
  __shared__ int rcnt[32], ccnt[32];             // entries per bank class in it
  const int i = blockIdx.x, lane = threadIdx.x;
  if (i >= nseg) return;
  for (int r = lane; r < flag_rows; r += 64) flag[r] = 0x7fffffff;
  __syncthreads();
  const int beg = seg[i], end = seg[i + 1];
  constexpr int row_base = 0;  // (the meta words carry the rank of a row inside its wave)
  const int first = FILL ? iter_base[i] : 0;
  int out = first, next = beg, nc = 0, cur = 0;
  // counting pass, auto mode: a stream that needs several times the iterations its entries would fill
  // (a hub row: one entry per iteration) makes the caller give the layout up -- stop counting there
  // (an iteration holds at most one entry per row of the wave: a short tail block is not a hub)
  const int nrows_w = max(1, wrows[i]);
  const int per_it = nrows_w < 64 ? nrows_w : 64;
  // (a sparse stream -- the short last row block -- needs its iterations for the chunk windows it has to
  // walk, a pair of iterations per SPAN + 1 chunks: that is not a hub either)
  const int walk = 2 * ((NC / Q + SPAN + 1) / (SPAN + 1));
  // FILL with `caps`: the single-pass build -- the stream writes into a region of caps[i] iterations
  // (the same bound) and reports how many it used
  const int bail = caps ? caps[i] - 4
                        : ((!FILL && bail_factor > 0) ? bail_factor * max((end - beg + per_it - 1) / per_it, walk) + 64 : 0x7fffffff);
  int last_chunk = (int)(((int64_t)((i / MDE_RING_NCW) % Q) * NC + Q - 1) / Q);
  int m_lead = 0;
  while (nc > 0 || next < end) {
    const int m = nc > 0 ? cq_chunk[cur][0] : (int)(keys[next] & JM);  // oldest candidate's chunk
    // the chunk window is anchored at the first iteration of a PAIR (the kernel does one hand-shake
    // per pair: it waits for the newest chunk of both)
    if (((out - first) & 1) == 0) m_lead = m;
    const int lim = m_lead + SPAN;
    int nem = 0, nnew = 0, mx = 0;  // emitted so far, waiting so far (into buffer cur ^ 1), newest chunk emitted
    if (lane < 32) rcnt[lane] = ccnt[lane] = 0;
    __syncthreads();
    // offer a batch of candidates (stream order = ascending priority)
    auto offer = [&](int pos, uint32_t mw, int chunk, int age, int prio) {
      const int row = pos >= 0 ? (int)(mw & 0xffffu) - row_base : 0;  // (relative to the wave's first row)
      const int rc = pos >= 0 ? (int)((mw >> 16) & 0xffu) : -1, cc = pos >= 0 ? (int)(mw >> 24) : -2;
      if (pos >= 0) atomicMin(&flag[row], prio);
      __syncthreads();
      const bool rowwin = pos >= 0 && flag[row] == prio;
      // how many earlier row winners of this batch share my classes (whether or not they pass
      // their own caps: slightly pessimistic, deterministic and parallel)
      int rkR = 0, rkC = 0;
      const int rcw = rowwin ? rc : -1, ccw = rowwin ? cc : -2;
      for (int c = 0; c < 32; ++c) {
        const unsigned long long mr = __ballot(rcw == c), mc = __ballot(ccw == c);
        if (rc == c) rkR = __popcll(mr & ((1ull << lane) - 1ull));
        if (cc == c) rkC = __popcll(mc & ((1ull << lane) - 1ull));
      }
      const bool capok = rowwin && (rcnt[rc] + rkR < cap) && (ccnt[cc] + rkC < cap);
      const bool win = rowwin && (capok || age >= MDE_RING_FORCE);
      // winners beyond the 64th wait as well (they keep their turn: age unchanged)
      const unsigned long long wm = __ballot(win);
      const int widx = nem + __popcll(wm & ((1ull << lane) - 1ull));
      const bool emit = win && widx < 64;
      if (emit) {
        em[widx] = pos;
        em_row[widx] = row;
        atomicAdd(&rcnt[rc], 1);
        atomicAdd(&ccnt[cc], 1);
      }
      mx = max(mx, emit ? chunk : 0);
      const bool lose = pos >= 0 && !emit;
      const unsigned long long lm = __ballot(lose);
      const int lidx = nnew + __popcll(lm & ((1ull << lane) - 1ull));
      if (lose && lidx < MDE_RING_CARRY) {
        cq_pos[cur ^ 1][lidx] = pos;
        cq_meta[cur ^ 1][lidx] = mw;
        cq_chunk[cur ^ 1][lidx] = chunk;
        cq_age[cur ^ 1][lidx] = win ? age : age + 1;
      }
      // (overflow of the waiting queue cannot happen: a batch is only offered while
      // nnew + 64 <= MDE_RING_CARRY)
      nem += __popcll(__ballot(emit));
      nnew += __popcll(lm);
      __syncthreads();
    };
    int prio = 0;
    // the waiting entries first, 64 at a time
    for (int c0 = 0; c0 < nc; c0 += 64) {
      const int k = c0 + lane;
      const bool has = k < nc;
      offer(has ? cq_pos[cur][k] : -1, has ? cq_meta[cur][k] : 0u, has ? cq_chunk[cur][k] : 0, has ? cq_age[cur][k] : 0,
            prio + lane);
      prio += 64;
    }
    // then new entries while lanes are free and the window allows (a few rounds: entries that
    // have to wait leave their lane to the next ones)
    for (int round = 0; round < MDE_RING_ROUNDS && nem < 64 && next < end && nnew + 64 <= MDE_RING_CARRY; ++round) {
      const int want = 64 - nem;
      const int cand = next + lane;
      const bool in = lane < want && cand < end;
      const int chunk = in ? (int)(keys[cand] & JM) : 0x7fffffff;
      const bool take = in && chunk <= lim;
      const int ntake = __popcll(__ballot(take));
      if (ntake == 0) break;
      offer(take ? cand : -1, take ? meta[cand] : 0u, chunk, 0, prio + lane);
      prio += 64;
      next += ntake;
    }
    // the rows claimed in this iteration are released (a waiting entry keeps its row claimed until
    // here: later entries of that row do not overtake it)
    if (lane < nem) flag[em_row[lane]] = 0x7fffffff;
    for (int k = lane; k < nnew; k += 64) flag[(int)(cq_meta[cur ^ 1][k] & 0xffffu) - row_base] = 0x7fffffff;
    mx = mde_wave_max(mx);
    if (nem > 0) last_chunk = mx;  // newest chunk the iteration references
    if (FILL) {
      if (lane < nem) it_ent[(size_t)out * 64 + lane] = em[lane];
      if (lane == 0) {
        it_cnt[out] = nem | (last_chunk << 8);
        it_m[out] = m;
      }
    }
    ++out;
    nc = nnew;
    cur ^= 1;
    __syncthreads();
    if (out - first > bail) {
      if (lane == 0) iters[i] = 1 << 25;  // (x 64 entries = 2^31: over the 32-bit position limit checked below)
      return;
    }
  }
  // a stream is stored in blocks of 4 iterations (one 16-byte load per lane): pad with empty ones
  while ((out - first) & 3) {
    if (FILL && lane == 0) {
      it_cnt[out] = 0 | (last_chunk << 8);
      it_m[out] = last_chunk;
    }
    ++out;
  }
  if (iters && lane == 0) iters[i] = out - first;
}

// caps[i] = iterations reserved for stream i by the single-pass build: `factor` times what its entries
// (or its chunk windows) need at least, a multiple of 4
__global__ __launch_bounds__(MDE_BLOCK) void k_ring_caps(int nseg, const int32_t* __restrict__ seg,
                                                         const int32_t* __restrict__ wrows, int R, int Q, int NC, int SPAN,
                                                         int factor, int32_t* __restrict__ caps) {
  const int i = blockIdx.x * MDE_BLOCK + threadIdx.x;
  if (i > nseg) return;
  if (i == nseg) {
    caps[i] = 0;
    return;
  }
  const int nrows_w = max(1, wrows[i]);
  const int per_it = nrows_w < 64 ? nrows_w : 64;
  const int walk = 2 * ((NC / Q + SPAN + 1) / (SPAN + 1));
  const int need = max((seg[i + 1] - seg[i] + per_it - 1) / per_it, walk);
  caps[i] = (factor * need + 64 + 4 + 3) & ~3;
}

// Lane placement of one iteration, wave-parallel (round 3 ran a serial Euler split on one lane per
// iteration: 170 ms of the layout build).  LDS bank rules of gfx950 (tools/valuprobe): a wave64 b64 read
// is served in two passes of 32 lanes and costs, per pass, the deepest bank class (8-byte slot mod
// 32); a b64 write in four passes of 16 lanes over 16 classes.  The row side carries three of the
// four random accesses of an entry (x_v, accumulator read, accumulator write), so the ROW classes
// are dealt evenly: entries of a class alternate between the two 32-lane halves, and inside a half the
// entries of a class mod 16 alternate between its two 16-lane quarters (classes with an odd count hand
// their extra entry to the halves / quarters in turn).  The column classes are capped by the
// scheduler and otherwise left as they fall.
// in: act (lane holds an entry), rc (its row class, 0..31).  out: the lane that handles the entry.
__device__ __forceinline__ int ring_place_wave(bool act, int rc, int lane) {
  const unsigned long long lt = (1ull << lane) - 1ull;
  int rank = 0, par = 0, oddacc = 0;
  for (int c = 0; c < 32; ++c) {
    const unsigned long long m = __ballot(act && rc == c);
    if (rc == c) {
      rank = __popcll(m & lt);
      par = oddacc & 1;
    }
    oddacc += __popcll(m) & 1;
  }
  const int half = (rank + par) & 1;
  int quarter = 0;
  for (int h = 0; h < 2; ++h) {
    int oa = 0;
    for (int c = 0; c < 16; ++c) {
      const unsigned long long m = __ballot(act && half == h && (rc & 15) == c);
      if (half == h && (rc & 15) == c) quarter = (__popcll(m & lt) + (oa & 1)) & 1;
      oa += __popcll(m) & 1;
    }
  }
  int pos = 0;
  for (int g = 0; g < 4; ++g) {
    const unsigned long long m = __ballot(act && half * 2 + quarter == g);
    if (half * 2 + quarter == g) pos = __popcll(m & lt);
  }
  // (a quarter holds at most 16: a half gets at most ceil(cnt / 2) <= 32 entries, a quarter half of that)
  return half * 32 + quarter * 16 + pos;
}

// One wave per iteration: deal its <= 64 entries to the lanes, pad to 64 with dummies, write
// packed words, edge ids and the header.
__global__ __launch_bounds__(MDE_BLOCK) void k_ring_pack(int64_t nit, int nseg, const int32_t* __restrict__ iter_base,
                                                         const int32_t* __restrict__ src_base,
                                                         const int32_t* __restrict__ it_ent,
                                                         const int32_t* __restrict__ it_cnt,
                                                         const int32_t* __restrict__ it_m,
                                                         const uint32_t* __restrict__ keys,
                                                         const uint32_t* __restrict__ vals,
                                                         const int32_t* __restrict__ hrow,
                                                         const int32_t* __restrict__ nbr,
                                                         const int32_t* __restrict__ eid, int R, int Q, int C, int S,
                                                         int ring_off, int JB, int d, int row_lo, int place, int count_all,
                                                         int loss_band, uint32_t* __restrict__ packed,
                                                         int32_t* __restrict__ peid, uint32_t* __restrict__ hdr) {
  __shared__ uint8_t s_taken[MDE_BLOCK / 64][64], s_free[MDE_BLOCK / 64][64];
  __shared__ uint32_t s_prow[MDE_BLOCK / 64][64];  // the rows of a pair's first iteration, by lane
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int64_t nw = ((int64_t)gridDim.x * MDE_BLOCK) >> 6;
  const uint32_t JM = (1u << JB) - 1u;
  const int sh = ring_cls_shift(d), cm = ring_cls_mask(d);
  const uint32_t cbytes = (uint32_t)C * 4u * (uint32_t)d;
  // (the waves of a block run the same number of trips: the barriers below are block-wide)
  for (int64_t itb = (int64_t)blockIdx.x * (MDE_BLOCK / 64); itb < nit; itb += nw) {
    const int64_t it = itb + wv;
    const bool valid = it < nit;
    // where the scheduler left iteration `it` (the single-pass build reserves a region per stream):
    // stream s = the last one with iter_base[s] <= it
    int64_t src = it;
    if (valid && src_base) {
      int lo = 0, hi = nseg;  // iter_base[lo] <= it < iter_base[hi]
      while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if ((int64_t)iter_base[mid] <= it) lo = mid; else hi = mid;
      }
      src = (int64_t)src_base[lo] + (it - (int64_t)iter_base[lo]);
    }
    const int cw = valid ? __builtin_amdgcn_readfirstlane(it_cnt[src]) : 0;  // entries | newest chunk << 8
    const int cnt = cw & 0xff;
    const bool act = valid && lane < cnt;
    uint32_t key = 0, q = 0, col = 0, rowaddr = 0, ring = 0;
    int grow = 0, rcls = 0;
    if (act) {
      const int pos = it_ent[(size_t)src * 64 + lane];
      key = keys[pos];
      q = vals[pos];
      const int rb = (int)((key >> JB) / MDE_RING_NCW) / Q;
      grow = hrow[q];
      rowaddr = (uint32_t)(grow - rb * R) * 4u * (uint32_t)d;
      const uint32_t j = key & JM;
      col = (uint32_t)nbr[q];
      ring = (uint32_t)ring_off + (j % (uint32_t)S) * cbytes + (col - j * (uint32_t)C) * 4u * (uint32_t)d;
      rcls = (int)((rowaddr >> sh) & (uint32_t)cm);
    }
    s_taken[wv][lane] = 0;
    s_prow[wv][lane] = 0xffffffffu;
    __syncthreads();
    // Lane-stable pairs: the kernel reads both accumulators of a pair of iterations before it writes either, so
    // a row that occurs in both iterations must sit on the SAME lane in both (the second takes the first's
    // updated value from a register there).  The first iteration of a pair (even `it`, wave wv) is dealt as
    // before; the second (wave wv + 1 of the same trip: itb is a multiple of 4) pins such entries to the first's
    // lanes and deals the others as they fall -- an entry whose lane a pinned one took moves to a free lane.
    const bool second = (it & 1) != 0;
    int l = lane;
    if (!second) {
      if (place) l = ring_place_wave(act, rcls, lane);
      if (act) {
        s_taken[wv][l] = 1;
        s_prow[wv][l] = rowaddr;
      }
    }
    __syncthreads();
    int pin = -1;
    if (second) {
      const uint32_t prow = s_prow[wv - 1][lane];
#pragma unroll 8
      for (int k = 0; k < 64; ++k)
        if ((uint32_t)__builtin_amdgcn_readlane((int)prow, k) == rowaddr) pin = k;
      pin = act ? pin : -1;
      if (place) l = ring_place_wave(act && pin < 0, rcls, lane);
      if (pin >= 0) {
        l = pin;
        s_taken[wv][l] = 1;
      }
    }
    __syncthreads();
    // (the unpinned entries' lanes are distinct: each one tests and takes its own)
    const bool moved = second && act && pin < 0 && s_taken[wv][l];
    if (second && act && !moved) s_taken[wv][l] = 1;
    __syncthreads();
    {
      // the lanes nobody took, in ascending order: first for the moved entries, then for the padding entries
      const bool fr = !s_taken[wv][lane];
      const unsigned long long fm = __ballot(fr);
      if (fr) s_free[wv][__popcll(fm & ((1ull << lane) - 1ull))] = (uint8_t)lane;
    }
    __syncthreads();
    const unsigned long long mvm = __ballot(moved);
    const int nmoved = __popcll(mvm);
    if (moved) l = s_free[wv][__popcll(mvm & ((1ull << lane) - 1ull))];
    // whose loss terms: one of the edge's two entries by ring_counts (grow is the local row there: the smaller vertex,
    // flipped between bands of loss_band vertices); a permuted layout (grow is a slot) adds every entry's with weight 1/2
    const bool counts = act && (count_all || ring_counts((uint32_t)(row_lo + grow), col, (uint32_t)loss_band));
    const int ncount = __popcll(__ballot(counts));
    const uint32_t lclass = ncount == 0 ? 0u : (ncount == cnt ? 1u : 2u);
    // chunk window of the iteration: the oldest chunk its stream still needs (waiting entries
    // included) .. the newest chunk it references
    const uint32_t m = valid ? (uint32_t)__builtin_amdgcn_readfirstlane(it_m[src]) : 0u;
    const uint32_t need = max((uint32_t)(cw >> 8), m);
    // the padding lanes read a column that is resident for sure: the first one of the oldest chunk
    // of the PAIR of iterations (the kernel waits for that chunk before it issues the pair's reads)
    const uint32_t mpad = valid ? (uint32_t)__builtin_amdgcn_readfirstlane(it_m[src & ~(int64_t)1]) : 0u;  // (regions start on multiples of 4)
    // element (iteration it, lane l) of a stream lives at ((it / 4) * 64 + l) * 4 + it % 4
    const size_t base = ((size_t)(it >> 2) * 64) * 4 + (size_t)(it & 3);
    if (act) {
      packed[base + (size_t)l * 4] = ring_pack_word(d, rowaddr, ring) | ((d == 2 && counts) ? MDE_RING_COUNTS_BIT : 0u);
      peid[base + (size_t)l * 4] = eid[q];
    } else if (valid) {
      // padding: a dummy row slot of the lane's own bank class, a resident column
      const int lf = s_free[wv][nmoved + lane - cnt];
      packed[base + (size_t)lf * 4] = ring_pack_word(d, (uint32_t)(R + (lf & 31)) * 4u * (uint32_t)d,
                                                     (uint32_t)ring_off + (mpad % (uint32_t)S) * cbytes);
      peid[base + (size_t)lf * 4] = -1;
    }
    if (lane == 0 && valid) {
      hdr[MDE_RING_HW * it] = m;
      hdr[MDE_RING_HW * it + 1] = need;
      hdr[MDE_RING_HW * it + 2] = lclass;
      hdr[MDE_RING_HW * it + 3] = (cnt < 64 ? MDE_RING_H3_PAD : 0u) | ((uint32_t)cnt << 8) | ((uint32_t)ncount << 16);
    }
    __syncthreads();
  }
}

// loss class of every block of four iterations (header word 3 of its first iteration, bits 1:0)
__global__ __launch_bounds__(MDE_BLOCK) void k_ring_block_class(int64_t nblocks, uint32_t* __restrict__ hdr) {
  const int64_t b = (int64_t)blockIdx.x * MDE_BLOCK + threadIdx.x;
  if (b >= nblocks) return;
  bool any0 = false, any1 = false, any2 = false;
  for (int q = 0; q < 4; ++q) {
    const uint32_t* h = hdr + (size_t)MDE_RING_HW * (4 * b + q);
    if ((h[3] >> 8) == 0u) continue;  // an empty iteration adds nothing whatever the class
    any0 |= h[2] == 0u;
    any1 |= h[2] == 1u;
    any2 |= h[2] == 2u;
  }
  const uint32_t cls = (any2 || (any0 && any1)) ? 2u : (any1 ? 1u : 0u);
  hdr[(size_t)MDE_RING_HW * 4 * b + 3] = (hdr[(size_t)MDE_RING_HW * 4 * b + 3] & ~3u) | cls;
  // one hand-shake per pair of iterations: the first one's `need` covers both.  An EMPTY iteration
  // reads no column (its lanes sit on the first column of the pair's oldest chunk, k_ring_pack) and
  // asks for nothing: on a sparse stream its own m may lie far beyond the pair's window.
  for (int t = 0; t < 2; ++t) {
    uint32_t* h0 = hdr + (size_t)MDE_RING_HW * (4 * b + 2 * t);
    uint32_t* h1 = h0 + MDE_RING_HW;
    uint32_t need = h0[0];
    if ((h0[3] >> 8) != 0u) need = max(need, h0[1]);
    if ((h1[3] >> 8) != 0u) need = max(need, h1[1]);
    h0[1] = need;
  }
}

// stats[0] = iterations with padding, stats[1] = iterations that add loss terms for every entry,
// stats[2] = iterations with the per-lane loss test
__global__ __launch_bounds__(MDE_BLOCK) void k_ring_stats(int64_t nit, const uint32_t* __restrict__ hdr,
                                                          unsigned long long* __restrict__ stats) {
  unsigned long long a = 0, b = 0, c = 0;
  for (int64_t i = (int64_t)blockIdx.x * MDE_BLOCK + threadIdx.x; i < nit; i += (int64_t)gridDim.x * MDE_BLOCK) {
    a += (hdr[MDE_RING_HW * i + 3] & MDE_RING_H3_PAD) ? 1u : 0u;
    b += hdr[MDE_RING_HW * i + 2] == 1u;
    c += hdr[MDE_RING_HW * i + 2] == 2u;
  }
  a = mde_wave_sum(a);
  b = mde_wave_sum(b);
  c = mde_wave_sum(c);
  if ((threadIdx.x & 63) == 0) {
    atomicAdd(&stats[0], a);
    atomicAdd(&stats[1], b);
    atomicAdd(&stats[2], c);
  }
}

// How the loss terms are spread (mde_plan_ring_loss_balance).  One wave per workgroup: wg[2 * g] = entries of its
// streams, wg[2 * g + 1] = those that add their loss term (header word 3); cls[c] += blocks of four iterations of
// loss class c.
__global__ __launch_bounds__(64) void k_ring_loss_stats(const int32_t* __restrict__ wave_iter, const uint32_t* __restrict__ hdr,
                                                        unsigned long long* __restrict__ wg, unsigned long long* __restrict__ cls) {
  const int g = blockIdx.x, lane = threadIdx.x;
  const int64_t i0 = wave_iter[(size_t)g * MDE_RING_NCW], i1 = wave_iter[(size_t)(g + 1) * MDE_RING_NCW];
  unsigned long long ent = 0, cnt = 0, c0 = 0, c1 = 0, c2 = 0;
  for (int64_t i = i0 + lane; i < i1; i += 64) {
    const uint32_t h3 = hdr[MDE_RING_HW * i + 3];
    ent += (h3 >> 8) & 0xffu;
    cnt += (h3 >> 16) & 0xffu;
    if ((i & 3) == 0) {  // (streams start on multiples of 4)
      c0 += (h3 & 3u) == 0u;
      c1 += (h3 & 3u) == 1u;
      c2 += (h3 & 3u) == 2u;
    }
  }
  ent = mde_wave_sum(ent);
  cnt = mde_wave_sum(cnt);
  c0 = mde_wave_sum(c0);
  c1 = mde_wave_sum(c1);
  c2 = mde_wave_sum(c2);
  if (lane == 0) {
    wg[2 * g] = ent;
    wg[2 * g + 1] = cnt;
    atomicAdd(&cls[0], c0);
    atomicAdd(&cls[1], c1);
    atomicAdd(&cls[2], c2);
  }
}

// How evenly a workgroup's consumer waves advance along the column sweep (round 6, late).  The ring couples the
// eight waves of a workgroup: nobody can be more than the ring's slack (~4 chunks) ahead of the slowest.  On a uniform
// graph every wave finds about the same number of entries in every chunk and the coupling costs nothing; on a graph
// whose links stay near the diagonal of the vertex order (data sorted by class: 2/3 of the links inside clusters of
// 1000 consecutive items) each wave's entries sit in the few chunks that hold ITS rows' clusters, the waves take
// turns instead of working side by side, and the launch takes what ONE wave at a time would: n = 1M, 50M such edges
// ran 1.28 ms on the ring kernel against 0.66 on the CSR kernels (0.16 for the uniform graph), n = 100k 0.22 against
// 0.05 (tools/r6_clusters.sh).  crit[wg] = sum over groups of GW chunks of the LARGEST entry count among the
// workgroup's waves, tot[wg] = all its entries: crit / (tot / NCW) is ~1.1 for a uniform graph (the maximum of eight
// Poisson counts), up to NCW when the waves' entries never share a chunk group.  One thread per (workgroup, group):
// sixteen binary searches in the sorted keys.
__global__ __launch_bounds__(MDE_BLOCK) void k_ring_sweep_balance(int nwg, int ngroups, int GW, int JB,
                                                                  const uint32_t* __restrict__ keys,
                                                                  const int32_t* __restrict__ seg,
                                                                  unsigned long long* __restrict__ crit,
                                                                  unsigned long long* __restrict__ tot) {
  const int64_t idx = (int64_t)blockIdx.x * MDE_BLOCK + threadIdx.x;
  if (idx >= (int64_t)nwg * ngroups) return;
  const int wg = (int)(idx / ngroups), g = (int)(idx % ngroups);
  unsigned long long mx = 0, sm = 0;
  for (int w = 0; w < MDE_RING_NCW; ++w) {
    const uint32_t s = (uint32_t)wg * MDE_RING_NCW + (uint32_t)w;
    const int32_t lo = seg[s], hi = seg[s + 1];
    const uint64_t k0 = ((uint64_t)s << JB) + (uint64_t)g * GW, k1 = k0 + (uint64_t)GW;
    auto lower = [&](uint64_t key) {
      int32_t a = lo, b = hi;  // first position in [lo, hi) whose key >= `key`
      while (a < b) {
        const int32_t m = a + ((b - a) >> 1);
        if ((uint64_t)keys[m] < key) a = m + 1; else b = m;
      }
      return a;
    };
    const unsigned long long c = (unsigned long long)(lower(k1) - lower(k0));
    mx = c > mx ? c : mx;
    sm += c;
  }
  if (sm) {
    atomicAdd(&crit[wg], mx);
    atomicAdd(&tot[wg], sm);
  }
}

// ---------------------------------------------------------------- the build: one state, a list of stages
// Everything build_ring allocates has its owner here: an error or a "keep the CSR layout" return frees it all, and
// commit() is the only place where ownership leaves (to plan->ring).  The buffers are allocated in the order they
// are listed in the stages -- hipMalloc order and sizes decide the build's peak memory and, through first-touch
// mapping (~10 ms per GB), most of its time.
struct RingBuild {
  mde_plan* plan;
  int d;
  hipStream_t st;
  RingSizes z;
  RowPlan rp;  // (the host vectors stay alive until the build's last synchronisation)
  int64_t nloc, H;
  int64_t H_ring = 0;  // half-edges the ring streams hold (the rest belongs to peeled rows)
  int nseg = 0;
  uint32_t JM = 0;
  // what the stages hand on
  size_t tmp_bytes = 0;
  int cap = 0, place = 1, flag_rows = 64, loss_band = 0;
  size_t flag_bytes = 0;
  bool single = false;
  int32_t total_iters = 0;
  std::vector<unsigned long long> lstat;  // per workgroup entries | entries that add their loss term, then the three class counts
  // scratch
  MdeDeviceBuf<uint32_t> keys, vals, keys2, vals2, wmap;
  MdeDeviceBuf<int32_t> hrow, wrows, seg, iters, row_slot, slot_cum, caps, cap_base, it_ent, it_cnt, it_m;
  MdeDeviceBuf<char> tmp;
  // what the plan keeps
  MdeDeviceBuf<uint32_t> packed, hdr;
  MdeDeviceBuf<int32_t> peid, iter_base, slot_row, hub_rows, hub_seg, hub_first;
  MdeDeviceBuf<double> hub_partial;
  MdeDeviceBuf<float> partial;
  // buffers that serve twice
  uint32_t* meta() const { return keys; }  // the scheduler's meta words: keys is free once the stream sort has left its result in keys2
  uint32_t* skey() const { return reinterpret_cast<uint32_t*>(hrow.get()); }  // the stream keys during the by-column pre-sort (hrow is rebuilt behind it)
  unsigned long long* stat_words() const { return reinterpret_cast<unsigned long long*>(iters.get()); }  // MDE_RING_STATS, >= 3 words
  int64_t Hp() const { return (int64_t)total_iters * 64; }  // padded half-edge count
  int nwg() const { return z.NRB * z.Q; }

  RingBuild(mde_plan* plan_, int d_, const RingSizes& z_, hipStream_t st_)
      : plan(plan_), d(d_), st(st_), z(z_), nloc(plan_->row_hi - plan_->row_lo), H(plan_->H) {}

  // (MDE_RING_STATS: where the build's time goes, host side included)
  const bool stats_on = ring_stats_on();
  std::chrono::steady_clock::time_point t_last = std::chrono::steady_clock::now();
  void tick(const char* what) {
    if (!stats_on) return;
    (void)hipStreamSynchronize(st);
    const auto t1 = std::chrono::steady_clock::now();
    fprintf(stderr, "[mde ring build] %-28s %8.2f ms\n", what, std::chrono::duration<double, std::milli>(t1 - t_last).count());
    t_last = t1;
  }
};

// A stage returns 1 to go on, 0 when the caller keeps the CSR layout, < 0 on error (build_ring's own convention).
#define RING_STAGE(call)          \
  do {                            \
    const int rc__ = (call);      \
    if (rc__ != 1) return rc__;   \
  } while (0)
static int ring_fail(hipError_t e, const char* what) { return mde_hip_fail(e, what, __FILE__, __LINE__); }

// which rows are peeled off to the hub kernel, and whether the rest are dealt to the row blocks (round 6): the row
// pointers go to the host, plan_rows (mde_ring_rows.h) does the rest
static int plan_the_rows(RingBuild& b) {
  RingSizes& z = b.z;
  const int hub_env = env_int("MDE_RING_HUB", -1);       // 0: never peel; N > 0: peel rows with more than N half-edges
  const int perm_env = env_int("MDE_RING_PERMUTE", -1);  // 0 / 1: never / always deal the rows to the blocks
  std::vector<int32_t> rowptr;
  if (hub_env != 0 || perm_env != 0) {
    rowptr.resize((size_t)b.nloc + 1);
    MDE_HIP(hipMemcpyAsync(rowptr.data(), b.plan->rowptr, rowptr.size() * sizeof(int32_t), hipMemcpyDeviceToHost, b.st));
    MDE_HIP(hipStreamSynchronize(b.st));
  }
  const RowPlan& rp = b.rp;
  if (!plan_rows(rowptr.data(), b.nloc, b.H, z.R, z.NRB, MDE_RING_NCW, hub_env, perm_env, &b.rp)) {
    mde_set_error("ring layout: a row block overflowed while the rows were dealt (internal error)");
    return MDE_E_INVALID;
  }
  if (rp.mapped && ring_stats_on())
    fprintf(stderr, "[mde ring] rows: threshold %d half-edges, max degree %d, %zu hub rows with %lld half-edges (%.2f%%) peeled into %zu "
            "segments; blocks %s (%d)\n", rp.threshold, rp.max_deg, rp.hub_rows.size(), (long long)rp.hub_half_edges,
            100.0 * (double)rp.hub_half_edges / (double)std::max<int64_t>(b.H, 1), rp.hub_seg.size() / 4,
            rp.permuted ? "DEALT by degree" : "of consecutive rows", rp.nrb);
  if (rp.mapped && rp.nrb != z.NRB) {
    z.NRB = rp.nrb;
    z.Q = choose_col_groups(b.plan, z.NRB, z.qmax, z.NC);
    if ((int64_t)z.NRB * z.Q > MDE_MAX_PARTIALS || bits_for_u64((uint64_t)((int64_t)z.NRB * z.Q * MDE_RING_NCW)) + z.JB > 32) return 0;
  }
  b.H_ring = rp.H_ring;
  if (b.H_ring <= 0) return 0;
  b.nseg = z.NRB * z.Q * MDE_RING_NCW;
  b.JM = (1u << z.JB) - 1u;
  return 1;
}

static int alloc_scratch(RingBuild& b) {
  const RingSizes& z = b.z;
  const size_t hb = (size_t)b.H * sizeof(uint32_t), sb = ((size_t)b.nseg + 1) * sizeof(int32_t);
  MDE_HIP(b.keys.alloc(hb));
  MDE_HIP(b.vals.alloc(hb));
  MDE_HIP(b.keys2.alloc(hb));
  MDE_HIP(b.vals2.alloc(hb));
  MDE_HIP(b.hrow.alloc(hb));
  MDE_HIP(b.wrows.alloc(sb));
  MDE_HIP(b.wmap.alloc((size_t)z.NRB * z.Q * z.R * sizeof(uint32_t)));
  MDE_HIP(b.seg.alloc(sb));
  MDE_HIP(b.iters.alloc(sb));
  MDE_HIP(b.iter_base.alloc(sb));
  b.tick("scratch allocations");
  return 1;
}

static hipError_t upload(MdeDeviceBuf<int32_t>& dst, const std::vector<int32_t>& src, hipStream_t st) {
  hipError_t e = dst.alloc(std::max<size_t>(src.size(), 1) * sizeof(int32_t));
  if (e == hipSuccess && !src.empty()) e = hipMemcpyAsync(dst, src.data(), src.size() * sizeof(int32_t), hipMemcpyHostToDevice, st);
  return e;
}
static int upload_row_plan(RingBuild& b) {
  const RowPlan& rp = b.rp;
  if (!rp.mapped) return 1;
  MDE_HIP(upload(b.row_slot, rp.row_slot, b.st));
  MDE_HIP(upload(b.slot_cum, rp.slot_cum, b.st));
  if (rp.permuted) MDE_HIP(upload(b.slot_row, rp.slot_row, b.st));
  if (!rp.hub_rows.empty()) {
    MDE_HIP(upload(b.hub_rows, rp.hub_rows, b.st));
    MDE_HIP(upload(b.hub_seg, rp.hub_seg, b.st));
    MDE_HIP(upload(b.hub_first, rp.hub_first, b.st));
    MDE_HIP(b.hub_partial.alloc((rp.hub_seg.size() / 4) * 8 * sizeof(double)));
  }
  return 1;
}

// row (or slot) -> wave map, then every CSR position's stream key
static int make_keys(RingBuild& b) {
  const RingSizes& z = b.z;
  const mde_plan* plan = b.plan;
  if (b.rp.mapped) {
    hipLaunchKernelGGL(k_ring_assign_slots, dim3(z.NRB * z.Q), dim3(64), 0, b.st, z.R, z.Q, b.slot_cum, b.wmap, b.wrows);
    MDE_LAUNCH_CHECK();
    b.tick("slot -> wave assignment");
    hipLaunchKernelGGL(k_ring_hrow, dim3(mde_grid(b.nloc * 16, MDE_BLOCK, 4096)), dim3(MDE_BLOCK), 0, b.st, (int)b.nloc, plan->rowptr, b.hrow);
    MDE_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_ring_keys_slots, dim3(mde_grid(b.H, MDE_BLOCK, 8192)), dim3(MDE_BLOCK), 0, b.st, b.H, plan->nbr, b.row_slot, b.wmap,
                       z.R, z.Q, z.NC, z.C, z.JB, (uint32_t)b.nseg, b.keys, b.vals, b.hrow);
    MDE_LAUNCH_CHECK();
  } else {
    // MDE_RING_ASSIGN=1: the greedy, sweep-balanced row -> wave map (14.6 ms at config 4, no faster: see k_ring_assign);
    // default: contiguous row ranges of equal half-edge count
    const int contiguous = env_int("MDE_RING_ASSIGN", 0) == 0;
    hipLaunchKernelGGL(k_ring_assign, dim3(z.NRB * z.Q), dim3(64), 0, b.st, (int)b.nloc, z.R, z.Q, z.NC, z.C, contiguous, plan->rowptr,
                       plan->nbr, b.wmap, b.wrows);
    MDE_LAUNCH_CHECK();
    b.tick("row -> wave assignment");
    hipLaunchKernelGGL(k_ring_keys, dim3(mde_grid(b.nloc * 16, MDE_BLOCK, 4096)), dim3(MDE_BLOCK), 0, b.st, (int)b.nloc, plan->rowptr,
                       plan->nbr, b.wmap, z.R, z.Q, z.NC, z.C, z.JB, b.keys, b.vals, b.hrow);
    MDE_LAUNCH_CHECK();
  }
  b.tick("keys kernel");
  return 1;
}

// the stable sort by stream key: (keys, vals) -> (keys2, vals2)
static int sort_entries(RingBuild& b) {
  const RingSizes& z = b.z;
  const mde_plan* plan = b.plan;
  const int H = (int)b.H;
  const size_t hb = (size_t)b.H * sizeof(uint32_t);
  size_t scan_bytes = 0;
  const int end_bit = std::min(32, bits_for_u64((uint64_t)b.nseg) + z.JB), col_bits = bits_for_u64((uint64_t)plan->n);
  MDE_HIP(mde_sort_pairs_u32(nullptr, b.tmp_bytes, b.keys, b.keys2, b.vals, b.vals2, H, 0, end_bit, b.st));
  MDE_HIP(mde_exclusive_sum_i32(nullptr, scan_bytes, b.iters, b.iter_base, b.nseg + 1, b.st));
  if (scan_bytes > b.tmp_bytes) b.tmp_bytes = scan_bytes;
  MDE_HIP(mde_sort_pairs_u32(nullptr, scan_bytes, b.keys, b.keys2, b.vals, b.vals2, H, 0, col_bits, b.st));
  if (scan_bytes > b.tmp_bytes) b.tmp_bytes = scan_bytes;
  MDE_HIP(b.tmp.alloc(b.tmp_bytes ? b.tmp_bytes : 16));
  b.tick("sort size queries + temp allocation");
  // Dense graphs (many entries per row and chunk): in CSR order the entries of ONE row follow each
  // other inside a chunk, and an iteration -- distinct rows -- would find a handful of rows in its
  // look-ahead.  Order the entries by column first (stable): inside a (stream, chunk) they then come
  // column by column, and the rows adjacent to one column are distinct.
  const bool dense = (double)b.H_ring > 0.5 * (double)b.nloc * (double)z.NC;
  if (env_int("MDE_RING_BYCOL", dense ? 1 : 0) != 0) {
    // keys2 = columns, sorted with vals -> (keys, vals2); then keys2 = stream keys in that order
    MDE_HIP(hipMemcpyAsync(b.keys2, plan->nbr, hb, hipMemcpyDeviceToDevice, b.st));
    MDE_HIP(hipMemcpyAsync(b.skey(), b.keys, hb, hipMemcpyDeviceToDevice, b.st));
    MDE_HIP(mde_sort_pairs_u32(b.tmp, b.tmp_bytes, b.keys2, b.keys, b.vals, b.vals2, H, 0, col_bits, b.st));
    hipLaunchKernelGGL(k_ring_gather_u32, dim3(mde_grid(b.H, MDE_BLOCK, 4096)), dim3(MDE_BLOCK), 0, b.st, b.H, b.vals2, b.skey(), b.keys);
    MDE_LAUNCH_CHECK();
    MDE_HIP(hipMemcpyAsync(b.vals, b.vals2, hb, hipMemcpyDeviceToDevice, b.st));
    hipLaunchKernelGGL(k_ring_hrow, dim3(mde_grid(b.nloc * 16, MDE_BLOCK, 4096)), dim3(MDE_BLOCK), 0, b.st, (int)b.nloc, plan->rowptr, b.hrow);
    MDE_LAUNCH_CHECK();
    if (b.rp.mapped) {
      hipLaunchKernelGGL(k_ring_rows_to_slots, dim3(mde_grid(b.H, MDE_BLOCK, 8192)), dim3(MDE_BLOCK), 0, b.st, b.H, b.row_slot, b.hrow);
      MDE_LAUNCH_CHECK();
    }
  }
  MDE_HIP(mde_sort_pairs_u32(b.tmp, b.tmp_bytes, b.keys, b.keys2, b.vals, b.vals2, H, 0, end_bit, b.st));
  b.tick("radix sort");
  return 1;
}

// where each stream starts in the sorted order, the scheduler's meta words, and the LDS its row flags need
static int segments_and_meta(RingBuild& b) {
  const RingSizes& z = b.z;
  hipLaunchKernelGGL(k_ring_seg, dim3(mde_grid(b.H + 1, MDE_BLOCK, 4096)), dim3(MDE_BLOCK), 0, b.st, b.H, (uint32_t)b.nseg, z.JB, b.keys2, b.seg);
  MDE_LAUNCH_CHECK();
  MDE_HIP(hipMemsetAsync(b.iters, 0, ((size_t)b.nseg + 1) * sizeof(int32_t), b.st));
  b.tick("keys, sorts, segments");
  // bank-class cap of the scheduler and the lane placement (environment: design ablations only)
  b.cap = std::max(1, env_int("MDE_RING_CAP", b.d == 4 ? 8 : 4));
  b.place = env_int("MDE_RING_PLACE", 1);
  // (the sorted positions [0, H_ring) are the ring's entries; the entries of peeled rows sort behind them)
  hipLaunchKernelGGL(k_ring_meta, dim3(mde_grid(b.H_ring, MDE_BLOCK, 8192)), dim3(MDE_BLOCK), 0, b.st, b.H_ring, b.keys2, b.vals2, b.hrow,
                     b.plan->nbr, b.wmap, z.JB, z.R, z.Q, b.d, b.meta());
  MDE_LAUNCH_CHECK();
  // rows of the largest wave range (the scheduler keeps one LDS word per row of its wave)
  std::vector<int32_t> hwr((size_t)b.nseg);
  MDE_HIP(hipMemcpyAsync(hwr.data(), b.wrows, hwr.size() * sizeof(int32_t), hipMemcpyDeviceToHost, b.st));
  MDE_HIP(hipStreamSynchronize(b.st));
  for (int i = 0; i < b.nseg; ++i) b.flag_rows = std::max(b.flag_rows, hwr[(size_t)i]);
  b.flag_rows = (b.flag_rows + 63) / 64 * 64;
  b.flag_bytes = (size_t)b.flag_rows * sizeof(int);
  return 1;
}

// base = exclusive scan of counts[0 .. nseg], *total = base[nseg]; synchronises.
// A stream that runs out of its region marks itself with 2^25 iterations (k_ring_schedule), which the callers
// recognise in the SUM of all streams' counts -- 2^25 x 64 entries are past the 32-bit position limit.  The sum is a
// 32-bit scan: 128 marked streams add up to 2^32 = 0 and the overflow went unseen (round 6: the planted-cluster graph
// at n = 1M with MDE_RING_ASSIGN=1 marked exactly 1024 streams; the regions were then used as if they had sufficed and
// the pack kernel faulted).  With look_for_bailed the counts themselves are looked at, and *total is set to -1 when
// any stream is marked.
static hipError_t scan_streams(RingBuild& b, const int32_t* counts, int32_t* base, bool look_for_bailed, int32_t* total) {
  std::vector<int32_t> h(look_for_bailed ? (size_t)b.nseg : 0);
  hipError_t e = mde_exclusive_sum_i32(b.tmp, b.tmp_bytes, counts, base, b.nseg + 1, b.st);
  if (e == hipSuccess) e = hipMemcpyAsync(total, base + b.nseg, sizeof(int32_t), hipMemcpyDeviceToHost, b.st);
  if (e == hipSuccess && look_for_bailed) e = hipMemcpyAsync(h.data(), counts, h.size() * sizeof(int32_t), hipMemcpyDeviceToHost, b.st);
  if (e == hipSuccess) e = hipStreamSynchronize(b.st);
  if (e != hipSuccess) return e;
  for (int32_t c : h)
    if (c >= (1 << 25)) {
      *total = -1;
      break;
    }
  return hipSuccess;
}
// it_ent / it_cnt / it_m for n iterations
static hipError_t alloc_iterations(RingBuild& b, int64_t n) {
  hipError_t e = b.it_ent.alloc((size_t)n * 64 * sizeof(int32_t));
  if (e == hipSuccess) e = b.it_cnt.alloc((size_t)n * sizeof(int32_t));
  if (e == hipSuccess) e = b.it_m.alloc((size_t)n * sizeof(int32_t));
  return e;
}
static void free_iterations(RingBuild& b) {
  b.it_ent.reset();
  b.it_cnt.reset();
  b.it_m.reset();
}
static bool fits_positions(int32_t total_iters) { return total_iters > 0 && (int64_t)total_iters * 64 < ((int64_t)1 << 31) - 64; }

// Single pass: every stream schedules into a region of caps[i] iterations (2 x what its entries or its
// chunk windows need at least) and reports how many it used; k_ring_pack compacts.  Leaves b.single false when a
// stream overflows its region (a hub row) or the regions do not fit the memory.
static int schedule_single_pass(RingBuild& b) {
  const RingSizes& z = b.z;
  const size_t sb = ((size_t)b.nseg + 1) * sizeof(int32_t);
  MDE_HIP(b.caps.alloc(sb));
  MDE_HIP(b.cap_base.alloc(sb));
  int32_t total_cap = 0;
  // (regions of 2 x the minimum: the scratch they take is what the build's time goes into -- fresh device
  // memory costs ~10 ms per GB to map on first use, more than the kernels that fill it)
  hipLaunchKernelGGL(k_ring_caps, dim3((b.nseg + 1 + MDE_BLOCK - 1) / MDE_BLOCK), dim3(MDE_BLOCK), 0, b.st, b.nseg, b.seg, b.wrows, z.R, z.Q,
                     z.NC, z.span, 2, b.caps);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = scan_streams(b, b.caps, b.cap_base, false, &total_cap);
  if (e != hipSuccess) return ring_fail(e, "ring layout: stream capacities");
  b.single = total_cap > 0 && (int64_t)total_cap * 64 < ((int64_t)1 << 33);
  if (b.single && alloc_iterations(b, total_cap) != hipSuccess) {
    (void)hipGetLastError();
    b.single = false;  // (not enough memory for the generous regions: count first)
    free_iterations(b);
  }
  if (!b.single) return 1;
  hipLaunchKernelGGL(k_ring_schedule<true>, dim3(b.nseg), dim3(64), b.flag_bytes, b.st, b.nseg, b.seg, b.wrows, b.keys2, b.meta(), b.JM, z.span,
                     z.R, z.Q, z.NC, b.d, b.cap, 4, b.iters, b.cap_base, b.it_ent, b.it_cnt, b.it_m, b.flag_rows, b.caps);
  e = hipGetLastError();
  if (e == hipSuccess) e = scan_streams(b, b.iters, b.iter_base, true, &b.total_iters);
  if (e != hipSuccess) return ring_fail(e, "ring layout: single-pass schedule");
  b.tick("meta + single scheduling pass");
  if (!fits_positions(b.total_iters)) {
    // a stream overflowed its region (a row with many times the average degree; or the layout is too
    // large for 32-bit positions): count first -- that pass decides whether the layout is given up
    b.single = false;
    free_iterations(b);
  }
  return 1;
}

// Cut the streams into wave iterations (k_ring_schedule).  The single pass first; when it does not do, the exact
// two-pass route: count here (with the give-up limit of auto mode), allocate and fill in pack_layout.  (Round 3
// always counted first: the scheduler ran twice.)  0: too large for 32-bit positions, or a stream gave up.
static int schedule(RingBuild& b) {
  const RingSizes& z = b.z;
  RING_STAGE(schedule_single_pass(b));
  if (!b.single) {
    hipLaunchKernelGGL(k_ring_schedule<false>, dim3(b.nseg), dim3(64), b.flag_bytes, b.st, b.nseg, b.seg, b.wrows, b.keys2, b.meta(), b.JM,
                       z.span, z.R, z.Q, z.NC, b.d, b.cap, panel_mode() == 1 ? 0 : 4, b.iters, nullptr, nullptr, nullptr, nullptr,
                       b.flag_rows, nullptr);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = scan_streams(b, b.iters, b.iter_base, true, &b.total_iters);
    if (e != hipSuccess) return ring_fail(e, "ring layout: counting pass");
    b.tick("meta + counting pass");
  }
  return fits_positions(b.total_iters) ? 1 : 0;
}

// Auto mode, with the iterations counted: is the layout still worth it?  (Rounds 3-5 gave up beyond 35 % padding --
// hub rows, which are peeled now, and sparse streams, whose half-filled iterations still beat the CSR kernel's
// gathers several times over.)  The streams' mean length is priced; a stream far beyond it would be a hub the
// threshold let through, and 4 x padding says as much.
// ... and how much of that runs side by side: the slowest workgroup's critical path along the sweep over the
// mean stream (k_ring_sweep_balance; ~1.1 on a uniform graph, which the 0.21 us per iteration already contain)
static int still_worth_it(RingBuild& b) {
  if (panel_mode() == 1) return 1;
  const RingSizes& z = b.z;
  const mde_plan* plan = b.plan;
  const int nwg = b.nwg(), GW = 4, ngroups = (z.NC + GW - 1) / GW;
  double serial = 1.0;
  {
    MdeDeviceBuf<unsigned long long> bal;
    std::vector<unsigned long long> hb((size_t)2 * nwg);
    hipError_t e = bal.alloc(hb.size() * sizeof(unsigned long long));
    if (e == hipSuccess) e = hipMemsetAsync(bal, 0, hb.size() * sizeof(unsigned long long), b.st);
    if (e == hipSuccess) {
      hipLaunchKernelGGL(k_ring_sweep_balance, dim3((unsigned)(((int64_t)nwg * ngroups + MDE_BLOCK - 1) / MDE_BLOCK)), dim3(MDE_BLOCK),
                         0, b.st, nwg, ngroups, GW, z.JB, b.keys2, b.seg, bal, bal.get() + nwg);
      e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(hb.data(), bal, hb.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, b.st);
    if (e == hipSuccess) e = hipStreamSynchronize(b.st);
    if (e != hipSuccess) return ring_fail(e, "ring layout: sweep balance");
    unsigned long long cmax = 0, tsum = 0;
    for (int i = 0; i < nwg; ++i) {
      cmax = std::max(cmax, hb[(size_t)i]);
      tsum += hb[(size_t)nwg + i];
    }
    if (tsum > 0) serial = (double)cmax / ((double)tsum / (double)b.nseg);
  }
  const double t_ring = std::max(1.0, serial / 1.15) * ring_time_us((double)b.total_iters / (double)b.nseg, z.NC, z.Q, nwg) +
                        (double)b.rp.hub_half_edges * 1.3e-5;
  if (ring_stats_on())
    fprintf(stderr, "[mde ring] sweep balance: critical path of the slowest workgroup / mean stream = %.2f\n", serial);
  // (mid regime: what the dealt layout and the hub launches add -- the slot map's gathers and a loss term on every
  // entry ~30 % per iteration, two more launches ~4 us: preferential attachment at n = 100k, out-degree 20 ran
  // 0.042 ms on the ring against 0.031 on the CSR kernel, tools/r6_midsize_skew.sh)
  const double mid_ring = plan->ring.cost_scale * (b.rp.permuted ? 1.3 : 1.0) * t_ring + MDE_RING_FIXED_US +
                          (b.rp.hub_half_edges > 0 ? 4.0 : 0.0);
  const bool mid_bad = mid_regime(plan, b.d) && mid_ring > 0.85 * (csr_time_us(plan, b.d) + MDE_CSR_FIXED_US);
  return ((double)b.Hp() > 4.0 * (double)b.H_ring || t_ring > 0.9 * csr_time_us(plan, b.d) || mid_bad) ? 0 : 1;
}

static int alloc_outputs(RingBuild& b) {
  const RingSizes& z = b.z;
  hipError_t e = hipSuccess;
  if (!b.single) e = alloc_iterations(b, b.total_iters);
  if (e == hipSuccess) e = b.packed.alloc((size_t)b.Hp() * sizeof(uint32_t));
  if (e == hipSuccess) e = b.peid.alloc((size_t)b.Hp() * sizeof(int32_t));
  if (e == hipSuccess) e = b.hdr.alloc((size_t)b.total_iters * MDE_RING_HW * sizeof(uint32_t));
  // (+ two words per row block behind the rows: ticket and flag of the in-launch sum of Q = 2 groups, zero between launches)
  const size_t partial_floats = (size_t)z.Q * (size_t)b.nloc * (size_t)b.d;
  if (e == hipSuccess && z.Q > 1) e = b.partial.alloc(sizeof(float) * (partial_floats + 2 * (size_t)z.NRB));
  if (e == hipSuccess && z.Q > 1) e = hipMemsetAsync(b.partial.get() + partial_floats, 0, sizeof(float) * 2 * (size_t)z.NRB, b.st);
  if (e != hipSuccess) return ring_fail(e, "ring layout: output allocations");
  b.tick("output allocations");
  return 1;
}

// Who adds an edge's loss term (ring_counts, mde_ring.h).  "The smaller vertex" puts the loss arithmetic on one
// corner of the (row block, column group) grid: the workgroups of the low row blocks' upper column group add a
// term on every entry, those of the high row blocks' lower group on none, and a launch of one round ends with its
// slowest workgroup.  Bands of W vertices with the rule flipped between bands of unlike parity give every workgroup
// about half: ~8 bands per column group, W a multiple of the block height (a wave's rows lie in one band, so the
// iterations stay all-or-none except where a chunk window crosses a band's edge).  d = 2 only (the per-lane test
// of those iterations is bit 31 of the packed word; d = 3 has no spare bit), full plans only (the shards of a
// sharded problem choose R independently and must agree on the rule), not for permuted layouts (every entry
// adds f / 2 there).  MDE_RING_LOSS_BAND: the band in row blocks, 0 = the smaller vertex everywhere.
static int choose_loss_band(const RingBuild& b) {
  const RingSizes& z = b.z;
  if (b.d != 2 || b.rp.permuted || b.plan->row_lo != 0 || b.nloc != b.plan->n) return 0;
  int64_t wb = std::max<int64_t>(1, (int64_t)z.NRB / (8 * (int64_t)z.Q));
  wb = std::max(0, env_int("MDE_RING_LOSS_BAND", (int)wb));
  return (int)std::min<int64_t>(wb * (int64_t)z.R, (int64_t)1 << 30);
}

// the fill pass of the two-pass route, then lanes, packed words, edge ids and headers
static int pack_layout(RingBuild& b) {
  const RingSizes& z = b.z;
  const mde_plan* plan = b.plan;
  if (!b.single) {
    hipLaunchKernelGGL(k_ring_schedule<true>, dim3(b.nseg), dim3(64), b.flag_bytes, b.st, b.nseg, b.seg, b.wrows, b.keys2, b.meta(), b.JM, z.span,
                       z.R, z.Q, z.NC, b.d, b.cap, 0, nullptr, b.iter_base, b.it_ent, b.it_cnt, b.it_m, b.flag_rows, nullptr);
    MDE_LAUNCH_CHECK();
  }
  b.loss_band = choose_loss_band(b);
  hipLaunchKernelGGL(k_ring_pack, dim3(mde_grid(b.Hp(), MDE_BLOCK, 8192)), dim3(MDE_BLOCK), 0, b.st, (int64_t)b.total_iters, b.nseg,
                     b.iter_base, b.single ? b.cap_base.get() : nullptr, b.it_ent, b.it_cnt, b.it_m, b.keys2, b.vals2, b.hrow, plan->nbr,
                     plan->eid, z.R, z.Q, z.C, z.S, z.ring_off, z.JB, b.d, (int)plan->row_lo, b.place, b.rp.permuted ? 1 : 0, b.loss_band,
                     b.packed, b.peid, b.hdr);
  MDE_LAUNCH_CHECK();
  MDE_HIP(hipStreamSynchronize(b.st));  // (cap_base is read by the pack kernel)
  b.caps.reset();
  b.cap_base.reset();
  hipLaunchKernelGGL(k_ring_block_class, dim3((unsigned)((b.total_iters / 4 + MDE_BLOCK - 1) / MDE_BLOCK)), dim3(MDE_BLOCK), 0, b.st,
                     (int64_t)(b.total_iters / 4), b.hdr);
  MDE_LAUNCH_CHECK();
  MDE_HIP(hipStreamSynchronize(b.st));
  b.tick("fill pass, pack, classes");
  return 1;
}

// how the loss terms fell on the workgroups (mde_plan_ring_loss_balance)
static int loss_statistics(RingBuild& b) {
  const int nwg = b.nwg();
  b.lstat.assign((size_t)2 * nwg + 3, 0ull);
  const size_t lb = b.lstat.size() * sizeof(unsigned long long);
  MdeDeviceBuf<unsigned long long> dl;
  hipError_t e = dl.alloc(lb);
  if (e == hipSuccess) e = hipMemsetAsync(dl, 0, lb, b.st);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(k_ring_loss_stats, dim3(nwg), dim3(64), 0, b.st, b.iter_base, b.hdr, dl, dl.get() + 2 * (size_t)nwg);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpyAsync(b.lstat.data(), dl, lb, hipMemcpyDeviceToHost, b.st);
  if (e == hipSuccess) e = hipStreamSynchronize(b.st);
  return e == hipSuccess ? 1 : ring_fail(e, "ring layout: loss statistics");
}

// MDE_RING_STATS: how even the streams are, a self-check of the hand-shake contract, how far apart a workgroup's
// waves run, and the layout's sizes.  Reads iter_base and hdr once.
static int report(RingBuild& b) {
  const RingSizes& z = b.z;
  const int nseg = b.nseg, total_iters = b.total_iters;
  unsigned long long hstat[3] = {0, 0, 0};
  MDE_HIP(hipMemsetAsync(b.stat_words(), 0, sizeof(hstat), b.st));
  hipLaunchKernelGGL(k_ring_stats, dim3(256), dim3(MDE_BLOCK), 0, b.st, (int64_t)total_iters, b.hdr, b.stat_words());
  MDE_HIP(hipMemcpyAsync(hstat, b.stat_words(), sizeof(hstat), hipMemcpyDeviceToHost, b.st));
  MDE_HIP(hipStreamSynchronize(b.st));
  std::vector<int32_t> hb((size_t)nseg + 1);
  std::vector<uint32_t> hh((size_t)total_iters * MDE_RING_HW);
  MDE_HIP(hipMemcpy(hb.data(), b.iter_base, hb.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
  MDE_HIP(hipMemcpy(hh.data(), b.hdr, hh.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
  {
    // how even are the consumer waves' streams?  (the slowest wave sets the kernel's duration)
    int mx = 0, mn = 1 << 30, wg_mx = 0;
    for (int i = 0; i < nseg; ++i) {
      mx = std::max(mx, hb[i + 1] - hb[i]);
      mn = std::min(mn, hb[i + 1] - hb[i]);
    }
    for (int g = 0; g + MDE_RING_NCW <= nseg; g += MDE_RING_NCW) wg_mx = std::max(wg_mx, hb[g + MDE_RING_NCW] - hb[g]);
    fprintf(stderr, "[mde ring] iterations per consumer wave: min %d mean %.1f max %d; per workgroup: mean %.1f max %d\n", mn,
            (double)total_iters / nseg, mx, (double)total_iters * MDE_RING_NCW / nseg, wg_mx);
  }
  {
    // self-check of the hand-shake contract: per pair of iterations, newest chunk - published chunk <= window
    long long bad = 0;
    int worst = 0;
    for (int64_t it = 0; it + 1 < total_iters; it += 2) {
      const int gap = (int)hh[it * MDE_RING_HW + 1] - (int)hh[it * MDE_RING_HW];
      if (gap > z.span || hh[(it + 1) * MDE_RING_HW] < hh[it * MDE_RING_HW]) {
        if (bad < 8)
          fprintf(stderr, "[mde ring] pair at iteration %lld: m %u need %u | next m %u need %u\n", (long long)it, hh[it * MDE_RING_HW],
                  hh[it * MDE_RING_HW + 1], hh[(it + 1) * MDE_RING_HW], hh[(it + 1) * MDE_RING_HW + 1]);
        ++bad;
      }
      worst = std::max(worst, gap);
    }
    fprintf(stderr, "[mde ring] hand-shake contract: %lld of %d pairs exceed the window (worst gap %d chunks)\n", bad, total_iters / 2, worst);
  }
  {
    // how far apart are the consumer waves of a workgroup along the column sweep?  At the same fraction of
    // their streams: newest minus oldest chunk over the waves (a ring slot is free when ALL of them are past it)
    std::vector<int> sp;
    for (int g0 = 0; g0 + MDE_RING_NCW <= nseg; g0 += MDE_RING_NCW) {
      int len = 1 << 30;
      for (int w = 0; w < MDE_RING_NCW; ++w) len = std::min(len, hb[g0 + w + 1] - hb[g0 + w]);
      if (len < 16) continue;
      for (int k = 0; k < len; k += 2) {
        int lo = 1 << 30, hi2 = 0;
        for (int w = 0; w < MDE_RING_NCW; ++w) {
          const int nit_w = hb[g0 + w + 1] - hb[g0 + w];
          const int64_t it = hb[g0 + w] + (((int64_t)k * nit_w / len) & ~(int64_t)1);
          const int m = (int)hh[it * MDE_RING_HW];
          lo = std::min(lo, m);
          hi2 = std::max(hi2, m);
        }
        sp.push_back(hi2 - lo);
      }
    }
    if (!sp.empty()) {
      std::sort(sp.begin(), sp.end());
      double mean = 0;
      for (int v : sp) mean += v;
      fprintf(stderr, "[mde ring] spread of a workgroup's consumer waves along the column sweep (chunks): mean %.2f median %d p90 %d max %d\n",
              mean / sp.size(), sp[sp.size() / 2], sp[sp.size() * 9 / 10], sp.back());
    }
  }
  fprintf(stderr, "[mde ring] d=%d R=%d NRB=%d Q=%d chunks=%d x %d cols, window %d, cap %d, placement %d: %d iterations for %lld half-edges "
          "(%.1f%% padding), %.1f%% with padding lanes; loss terms: %.1f%% of the iterations add all, %.2f%% test per lane\n",
          b.d, z.R, z.NRB, z.Q, z.NC, z.C, z.span, b.cap, b.place, total_iters, (long long)b.H_ring,
          100.0 * ((double)b.Hp() - (double)b.H_ring) / (double)b.H_ring, 100.0 * hstat[0] / total_iters, 100.0 * hstat[1] / total_iters,
          100.0 * hstat[2] / total_iters);
  return 1;
}

// the one place where ownership leaves the build: the old layout goes, the plan takes the new one's buffers
static void commit(RingBuild& b) {
  const RingSizes& z = b.z;
  const RowPlan& rp = b.rp;
  mde_ring_release(b.plan);
  mde_ring_layout& L = b.plan->ring;
  L.d = b.d;
  L.rows_per_block = z.R;
  L.n_row_blocks = z.NRB;
  L.col_groups = z.Q;
  L.chunk_cols = z.C;
  L.n_chunks = z.NC;
  L.ring_off = z.ring_off;
  L.slots = z.S;
  L.n_iters = b.total_iters;
  L.H = b.Hp();
  L.packed = b.packed.release();
  L.eid = b.peid.release();
  L.hdr = b.hdr.release();
  L.wave_iter = b.iter_base.release();
  L.partial = b.partial.release();
  L.slot_row = b.slot_row.release();
  L.count_all = rp.permuted ? 1 : 0;
  L.loss_band = b.loss_band;
  double lo = 2.0, hi = -1.0;
  for (int g = 0; g < b.nwg(); ++g) {
    if (b.lstat[2 * (size_t)g] == 0) continue;
    const double sh = (double)b.lstat[2 * (size_t)g + 1] / (double)b.lstat[2 * (size_t)g];
    lo = std::min(lo, sh);
    hi = std::max(hi, sh);
  }
  L.loss_share_min = hi < 0.0 ? 0.0 : lo;
  L.loss_share_max = hi < 0.0 ? 0.0 : hi;
  for (int c = 0; c < 3; ++c) L.class_blocks[c] = (int64_t)b.lstat[2 * (size_t)b.nwg() + c];
  L.n_hub_rows = (int)rp.hub_rows.size();
  L.n_hub_segs = (int)(rp.hub_seg.size() / 4);
  L.hub_half_edges = rp.hub_half_edges;
  L.hub_rows = b.hub_rows.release();
  L.hub_seg = b.hub_seg.release();
  L.hub_first = b.hub_first.release();
  L.hub_partial = b.hub_partial.release();
}

int build_ring(mde_plan* plan, int d, const RingSizes& sizes, hipStream_t st) {
  RingBuild b(plan, d, sizes, st);
  RING_STAGE(plan_the_rows(b));      // 0: the dealt blocks no longer fit the key, or nothing is left for the ring
  RING_STAGE(alloc_scratch(b));
  RING_STAGE(upload_row_plan(b));
  RING_STAGE(make_keys(b));
  RING_STAGE(sort_entries(b));
  RING_STAGE(segments_and_meta(b));
  RING_STAGE(schedule(b));           // 0: too large for 32-bit positions, or (auto mode) a stream gave up
  RING_STAGE(still_worth_it(b));     // 0: auto mode keeps the CSR kernels
  RING_STAGE(alloc_outputs(b));
  RING_STAGE(pack_layout(b));
  RING_STAGE(loss_statistics(b));
  if (b.stats_on) RING_STAGE(report(b));
  commit(b);
  return 1;
}

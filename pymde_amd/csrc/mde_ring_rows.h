// mde_ring_rows.h -- which rows of a plan go where in the LDS-ring layout: plain host C++ (no HIP include), so that
// tests/host/ring_rows_test.cpp can compile it with any C++17 compiler.  mde_ring_build.hip copies the row pointers
// to the host and calls plan_rows.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <vector>

#define MDE_HUB_SEG 512  // CSR positions per segment of a peeled hub row (one workgroup of k_hub_rows each)

// ---------------------------------------------------------------- round 6: which rows go where
// The layout of rounds 3-5 cut the vertex order into blocks of R consecutive rows and put every row's entries into
// the ring streams.  Two kinds of graph broke it (profiles/r06_cliff_probe.txt):
//   * HUB rows.  The rows of a wave iteration are distinct (one lane = one accumulator), so a row with more
//     entries than its wave's stream has iterations stretches that stream: one vertex of degree 5e5 in a
//     config-4 graph made one wave run 250 336 iterations where the others run 772 (28 ms per evaluation, and auto
//     mode gave the whole layout up for the CSR kernel at 1.4 ms).  Rows with more than T = max(256, H / (blocks x
//     NCW x 128)) half-edges -- half a stream's iterations per column group -- are PEELED: no ring stream holds
//     their entries (sentinel key), and k_hub_rows / k_hub_finish evaluate them from the CSR plan behind the ring
//     kernel.  Their rows are disjoint from the ring's: still one writer per row, fixed order, no atomics.
//   * degrees that DRIFT along the vertex order (preferential attachment: the early vertices collect the edges).
//     Blocks of consecutive rows then hold unequal work and the launch runs as long as its heaviest workgroup
//     (0.80 ms on a 1M-vertex preferential-attachment graph against 0.16 uniform).  When the heaviest block holds
//     more than 1.08 x the mean, the rows are DEALT to the blocks instead: sorted by degree (counting sort) and
//     handed out boustrophedon, every block gets the same number of rows and, to within one row's degree, the same
//     number of half-edges; inside a block the rows keep ascending order.  slot_row records which row sits in which
//     LDS slot; the kernel gathers x_v and scatters the gradient rows through it.
// Host code: one pass over the row pointers (copied to the host: 4 bytes per row) -- the ring layout is built once
// per edge list.
struct RowPlan {
  bool mapped = false, permuted = false;
  int nrb = 0;
  int64_t H_ring = 0;
  std::vector<int32_t> row_slot;   // [nloc]
  std::vector<int32_t> slot_row;   // [nrb * R] (permuted only)
  std::vector<int32_t> slot_cum;   // [nrb * R + 1]
  std::vector<int32_t> hub_rows, hub_first, hub_seg;  // hub_seg: [segments][4] = hub index, first position, end position, 0
  int64_t hub_half_edges = 0;
  int threshold = 0;
  int32_t max_deg = 0;  // (of the rows looked at for peeling: the MDE_RING_STATS report)
};

// rowptr[0 .. nloc]: the plan's row pointers (H = rowptr[nloc] half-edges), R rows per block, NRB = ceil(nloc / R)
// blocks, ncw consumer waves per workgroup.  hub_env (MDE_RING_HUB): 0 never peel, N > 0 peel rows with more than N
// half-edges, < 0 the threshold above; perm_env (MDE_RING_PERMUTE): 0 / 1 never / always deal the rows to the blocks,
// < 0 when the heaviest block asks for it.  With both 0 rowptr is not read.  Returns false when a row block overflowed
// while the rows were dealt (an internal error).
static inline bool plan_rows(const int32_t* rowptr, int64_t nloc, int64_t H, int R, int NRB, int ncw, int hub_env, int perm_env,
                             RowPlan* rp) {
  rp->nrb = NRB;
  rp->H_ring = H;
  if (hub_env == 0 && perm_env == 0) return true;
  int T = (int)std::max<int64_t>(256, H / ((int64_t)NRB * ncw * 128));
  if (hub_env > 0) T = hub_env;
  rp->threshold = T;
  // hub rows
  int64_t hub_he = 0;
  if (hub_env != 0) {
    for (int64_t r = 0; r < nloc; ++r) {
      const int32_t deg = rowptr[r + 1] - rowptr[r];
      rp->max_deg = std::max(rp->max_deg, deg);
      if (deg > T) {
        rp->hub_rows.push_back((int32_t)r);
        hub_he += deg;
      }
    }
    if (2 * hub_he > H) {  // (most of the graph in "hub" rows: a dense problem, not a hub -- the ring takes it whole)
      rp->hub_rows.clear();
      hub_he = 0;
    }
  }
  const bool peel = !rp->hub_rows.empty();
  // work per block of R consecutive rows (peeled rows count nothing)
  bool permute = perm_env == 1;
  if (perm_env < 0) {
    int64_t heaviest = 0;
    size_t hi = 0;
    for (int b = 0; b < NRB; ++b) {
      const int64_t r0 = (int64_t)b * R, r1 = std::min<int64_t>(nloc, r0 + R);
      int64_t w = rowptr[r1] - rowptr[r0];
      while (hi < rp->hub_rows.size() && rp->hub_rows[hi] < r1) {
        w -= rowptr[rp->hub_rows[hi] + 1] - rowptr[rp->hub_rows[hi]];
        ++hi;
      }
      heaviest = std::max(heaviest, w);
    }
    permute = NRB > 1 && (double)heaviest > 1.08 * (double)(H - hub_he) / (double)NRB;
  }
  if (!peel && !permute) return true;
  rp->mapped = true;
  rp->permuted = permute;
  rp->hub_half_edges = hub_he;
  rp->H_ring = H - hub_he;
  rp->row_slot.assign((size_t)nloc, -1);
  std::vector<uint8_t> is_hub((size_t)nloc, 0);
  for (int32_t r : rp->hub_rows) is_hub[(size_t)r] = 1;
  if (!permute) {
    // slots = rows; the peeled ones hold nothing
    rp->slot_cum.assign((size_t)NRB * R + 1, 0);
    int64_t cum = 0;
    for (int64_t r = 0; r < (int64_t)NRB * R; ++r) {
      rp->slot_cum[(size_t)r] = (int32_t)cum;
      if (r < nloc && !is_hub[(size_t)r]) {
        rp->row_slot[(size_t)r] = (int32_t)r;
        cum += rowptr[r + 1] - rowptr[r];
      }
    }
    rp->slot_cum[(size_t)NRB * R] = (int32_t)cum;
  } else {
    // counting sort by degree, heaviest first; boustrophedon deal; rows ascending inside a block
    const int64_t nring = nloc - (int64_t)rp->hub_rows.size();
    const int nrb = (int)std::max<int64_t>(1, (nring + R - 1) / R);
    rp->nrb = nrb;
    int32_t dmax = 0;
    for (int64_t r = 0; r < nloc; ++r)
      if (!is_hub[(size_t)r]) dmax = std::max(dmax, rowptr[r + 1] - rowptr[r]);
    std::vector<int64_t> start((size_t)dmax + 2, 0);
    for (int64_t r = 0; r < nloc; ++r)
      if (!is_hub[(size_t)r]) ++start[(size_t)(dmax - (rowptr[r + 1] - rowptr[r])) + 1];
    for (size_t k = 1; k < start.size(); ++k) start[k] += start[k - 1];
    std::vector<int32_t> block((size_t)nloc, -1);
    for (int64_t r = 0; r < nloc; ++r) {
      if (is_hub[(size_t)r]) continue;
      const int64_t rank = start[(size_t)(dmax - (rowptr[r + 1] - rowptr[r]))]++;
      const int64_t pos = rank % (2 * (int64_t)nrb);
      block[(size_t)r] = (int32_t)(pos < nrb ? pos : 2 * (int64_t)nrb - 1 - pos);
    }
    std::vector<int32_t> fill((size_t)nrb, 0);
    rp->slot_row.assign((size_t)nrb * R, -1);
    std::vector<int32_t> slot_deg((size_t)nrb * R, 0);
    for (int64_t r = 0; r < nloc; ++r) {
      const int b = block[(size_t)r];
      if (b < 0) continue;
      const int sidx = fill[(size_t)b]++;
      if (sidx >= R) return false;
      const size_t sl = (size_t)b * R + (size_t)sidx;
      rp->slot_row[sl] = (int32_t)r;
      rp->row_slot[(size_t)r] = (int32_t)sl;
      slot_deg[sl] = rowptr[r + 1] - rowptr[r];
    }
    rp->slot_cum.assign((size_t)nrb * R + 1, 0);
    int64_t cum = 0;
    for (size_t t = 0; t < (size_t)nrb * R; ++t) {
      rp->slot_cum[t] = (int32_t)cum;
      cum += slot_deg[t];
    }
    rp->slot_cum[(size_t)nrb * R] = (int32_t)cum;
  }
  // segments of the hub rows
  rp->hub_first.reserve(rp->hub_rows.size() + 1);
  for (size_t i = 0; i < rp->hub_rows.size(); ++i) {
    rp->hub_first.push_back((int32_t)(rp->hub_seg.size() / 4));
    const int32_t r = rp->hub_rows[i];
    for (int64_t b = rowptr[r]; b < rowptr[r + 1]; b += MDE_HUB_SEG) {
      rp->hub_seg.push_back((int32_t)i);
      rp->hub_seg.push_back((int32_t)b);
      rp->hub_seg.push_back((int32_t)std::min<int64_t>(rowptr[r + 1], b + MDE_HUB_SEG));
      rp->hub_seg.push_back(0);
    }
  }
  rp->hub_first.push_back((int32_t)(rp->hub_seg.size() / 4));
  return true;
}

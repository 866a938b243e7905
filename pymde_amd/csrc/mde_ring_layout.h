// mde_ring_layout.h -- what the layout decision (mde_ring.hip) and the layout builder (mde_ring_build.hip) share.
#pragma once
#include "mde_ring.h"
#include "mde_ring_rows.h"

struct RingSizes {
  int R, NRB, Q, C, NC, S, JB, ring_off, span, qmax;
};

// MDE_PANEL env: unset / -1 auto, 0 never, 1 whenever the layout is feasible (read at every layout
// decision, so a test can switch it inside one process)
static inline int panel_mode() { return env_int("MDE_PANEL", -1); }
// MDE_RING_STATS (set to anything): the builder reports its sizes, timings and self-checks on stderr
static inline bool ring_stats_on() { return getenv("MDE_RING_STATS") != nullptr; }

static inline int bits_for_u64(uint64_t maxval) {
  int b = 1;
  while (b < 64 && (maxval >> b)) ++b;
  return b;
}

// the cost model of mde_ring.hip, asked again by the builder once the iterations are counted
#define MDE_RING_FIXED_US 11.0
#define MDE_CSR_FIXED_US 7.0
MDE_INTERNAL double ring_time_us(double iters_per_wave, int NC, int Q, int nwg);
MDE_INTERNAL double csr_time_us(const mde_plan* plan, int d);
MDE_INTERNAL bool mid_regime(const mde_plan* plan, int d);
MDE_INTERNAL int choose_col_groups(const mde_plan* plan, int64_t nrb, int qmax, int64_t nc);

void mde_ring_release(mde_plan* plan);  // mde_ring.hip: frees plan->ring

// Builds plan->ring for dimension d with the sizes choose_sizes (mde_ring.hip) picked.  1: built; 0: not worthwhile
// or not feasible, the caller keeps the CSR layout; < 0: error.  plan->ring is touched only when 1 is returned.
MDE_INTERNAL int build_ring(mde_plan* plan, int d, const RingSizes& sizes, hipStream_t st);  // mde_ring_build.hip

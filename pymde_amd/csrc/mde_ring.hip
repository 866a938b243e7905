// mde_ring.hip -- LDS-resident variant of the fused average-distortion kernel for small
// embedding dimensions (d <= 4) on graphs whose embedding table does not fit L2 (layout 1): the
// layout decision (sizes and cost model), the queries and the dispatcher.  The kernel itself is
// mde_ring_kernel.h, instantiated per family of distortion functions in mde_ring_k_*.hip; the layout is built
// by mde_ring_build.hip (which rows go where: mde_ring_rows.h), the parameter streams by mde_ring_params.hip,
// the layout's self-checks are mde_ring_check.hip and the peeled hub rows' kernels mde_ring_hub.hip -- one unit
// per subsystem, because HIP loads a unit's code object on the first launch of one of its kernels (mde_ring.h).
// [ref: pymde/average_distortion.py:62-106 -- the same loss and gradient]
//
// Why: the CSR kernel's only random access is the gather of x_u, and random 8-byte gathers are
// bound by the L2 request rate (~100 G/s from an 8 MB table: >= 1 ms for 10^8 half-edges whatever
// the HBM rate).  Here every random access is served by LDS:
//
//   * a workgroup of 12 waves owns a block of R rows (R <= 7872 at d = 2) and one of Q column
//     groups: the rows' x_v and their fp32 gradient accumulators stay in LDS for the whole kernel
//     (2 x 63 KB); with Q > 1 the groups' partial gradients are added by k_ring_combine;
//   * the embedding table streams through a ring of S chunk slots in what is left of the 160 KB (9
//     slots of 4 KB at d = 2), staged by 4 producer waves through their VGPRs (global_load_dwordx4 ->
//     ds_write_b128, two chunks in flight per wave: the bytes in flight need no ring slot);
//   * the other 8 waves are consumers.  Each owns a fixed range of the block's rows and walks
//     its own contiguous stream of packed half-edges (absolute LDS addresses of x_v and x_u, 4
//     bytes, chunk-major) -- because a row has exactly one wave that ever touches its accumulator,
//     the update is a plain LDS read-add-write, the summation order is fixed by the layout
//     (bitwise reproducible), and the waves need NO workgroup barrier between prologue and epilogue;
//   * producers and consumers synchronise through a handful of LDS words: a consumer publishes
//     the oldest chunk it still reads (prog[w]), a producer the next chunk it has not landed yet
//     (F[p]); one hand-shake per PAIR of wave iterations, the pair's slots released as soon as its
//     LDS reads are issued;
//   * LDS fp32 atomics would remove the one-writer rule, but ds_add_f32 retires ~0.16 lanes per
//     clock per CU on gfx950 (tools/ldsprobe) -- 20x slower than read-add-write.  The layout
//     builder therefore makes the rows of a wave iteration DISTINCT (an entry whose row is taken
//     waits for the next iteration), caps the entries per LDS bank class on the row and on the
//     column side, and deals the entries to the lanes so that every 32-lane read pass and every
//     16-lane write pass is as shallow as the classes allow;
//   * every edge is evaluated from both endpoints (owner-computes gradient rows), but its LOSS term
//     is added once: by the entry whose row is the smaller vertex.  The header says per BLOCK of four
//     iterations whether none / all / some of its entries do (three copies of the block body, one
//     branch per block: half of the blocks skip the loss arithmetic).
// What bounds it (round 4, profiles/r04_att_summary.md): the consumers' loop is bound by the
// instructions it issues (VALU busy ~75 % of the launch), the staging by its bytes in flight; the two
// add up (0.10 ms + 0.078 ms per GB staged at config 4) because both are work on the same SIMDs.
#include <algorithm>
#include <cmath>

#include "mde_ring_layout.h"

// What an evaluation costs on either kernel, in microseconds -- the rule that picks the layout since round 6.  A ring
// workgroup takes whichever is longer: its consumer waves' iterations (~0.21 us each: config 4, 776 per wave,
// 0.16 ms) or the chunks that pass through its ring (~0.14 us each -- the hand-shake rate, not the bytes: n = 2M at
// degree 50 runs 3907 chunks per workgroup in 0.55 ms whatever the producers' depth or number, tools/r6_prod_sweep.sh);
// the launch runs ceil(workgroups / 256) rounds of them.  The CSR kernels gather x_u from L2 / HBM: 1.1-1.7 ms per
// 1e8 half-edges when the table overflows L2 (profiles/r06_cliff_probe.txt), ~0.6 when it does not.
double ring_time_us(double iters_per_wave, int NC, int Q, int nwg) {
  const double rounds = std::ceil((double)nwg / 256.0);
  return rounds * std::max(0.21 * iters_per_wave, 0.14 * (double)NC / (double)Q);
}
double csr_time_us(const mde_plan* plan, int d) {
  return (double)plan->H * ((int64_t)plan->n * d * 4 >= (6 << 20) ? 1.3e-5 : 0.6e-5);
}
// The regime between the MNIST-sized problems and the benchmark shape (round 6, late): the table sits in L2 and there
// are fewer than 16 M half-edges -- rounds 3-6 kept the CSR kernels there without asking.  tools/r6_midsize2.sh, ring
// forced against auto, d = 2, ms per evaluation: n = 150k at degree 50 0.0935 -> 0.0356, 100k 0.0604 -> 0.0273, 50k
// 0.0357 -> 0.0187; at degree 20 150k 0.0402 -> 0.0241, 100k 0.0312 -> 0.0214, 50k 0.0186 -> 0.0164, 20k 0.0162 -> 0.0151:
// the ring's iterations cost what they cost at config 4, in front of ~11 us of fixed cost (two launches, a prologue
// that fills 61 KB of LDS per workgroup, the groups' partial rows), the CSR kernels' 0.6e-5 us per half-edge sit on ~7.
// d = 2 and 3 only: d = 1 and 4 run the run-time functor on the ring kernel (2.7 x the compile-time kinds).
bool mid_regime(const mde_plan* plan, int d) {
  return (int64_t)plan->n * d * 4 < (6 << 20) && plan->H < ((int64_t)16 << 20);
}
// (MDE_RING_FIXED_US and MDE_CSR_FIXED_US: mde_ring_layout.h)
// ... and the ring kernel's iterations cost what the FUNCTION costs (profiles/r05_function_sweep.txt, ms per step at
// config-4 size: Quadratic 0.157 .. Huber 0.178, Logistic / Power / Log / SoftFractional 0.20-0.23, PushAndPull 0.2065,
// the run-time functor 0.44), while the CSR kernels' gathers hide most of it: a neighbour-preserving problem of 100k
// items (3.9 M half-edges, PushAndPull(Log1p, LogRatio)) runs 0.0296 ms on the CSR kernel and 0.0329 on the ring, at
// 200k items 0.0509 against 0.0432 (tools/r6_pn_scale.py).  mde_plan_function_hint tells the plan which function is
// coming; the scale multiplies the ring's estimate in the mid regime only.
static double function_cost_scale(int kind, int kind_neg) {
  if (kind_neg != MDE_F_NONE) return 1.3;
  switch (kind) {
    case MDE_F_LOG1P: case MDE_F_QUADRATIC: case MDE_F_LINEAR: case MDE_F_CUBIC: case MDE_F_INVPOWER: case MDE_F_HUBER:
    case MDE_F_L_QUADRATIC: case MDE_F_L_WEIGHTED_QUADRATIC: case MDE_F_L_ABSOLUTE: case MDE_F_L_HUBER: case MDE_F_L_CUBIC:
      return 1.05;
    case MDE_F_LOGISTIC: case MDE_F_POWER: case MDE_F_LOG: case MDE_F_SIGMOID: case MDE_F_HINGE: case MDE_F_LOGRATIO:
    case MDE_F_L_POWER: case MDE_F_L_LOGISTIC: case MDE_F_L_FRACTIONAL: case MDE_F_L_SOFT_FRACTIONAL:
      return 1.35;
    default:
      return 2.7;  // private kinds: the run-time functor
  }
}
extern "C" int mde_plan_function_hint(mde_plan* plan, int32_t kind, int32_t kind_neg) {
  if (!plan) return MDE_E_INVALID;
  plan->ring.cost_scale = (float)function_cost_scale(kind, kind_neg);
  return MDE_OK;
}

// Decide the block height and the column groups for dimension d; false when the layout is not
// worthwhile (the caller keeps the CSR kernel).
// Column groups per row block.  Default: one workgroup per CU (256 / row blocks).  Round 6: more than that when the
// cost model says so -- 193 row blocks (d = 3 at n = 1M) leave a quarter of the CUs idle with Q = 1 and need two
// rounds with Q = 2; with Q = 5 the 965 workgroups run 4 rounds of a fifth of the table each: 0.496 -> 0.444 ms
// (tools/r6_d3_sweep.sh), which the model predicts (547 -> 452 us).  A workgroup's fixed cost (prologue, epilogue,
// partial rows) is priced at 4 us; the default stays unless another Q is 5 % better.  MDE_RING_Q: design probe.
int choose_col_groups(const mde_plan* plan, int64_t nrb, int qmax, int64_t nc) {
  int Q = (int)std::min<int64_t>(qmax, std::max<int64_t>(1, 256 / nrb));
  const double its1 = 1.4 * (double)plan->H / ((double)nrb * MDE_RING_NCW * 64.0);
  auto cost = [&](int q) {
    const double rounds = std::ceil((double)(nrb * q) / 256.0);
    return ring_time_us(its1 / q, (int)nc, q, (int)(nrb * q)) + 4.0 * rounds;
  };
  const double base = cost(Q);
  double best = base;
  for (int q = 1; q <= qmax; ++q)
    if ((int64_t)nrb * q <= MDE_MAX_PARTIALS && cost(q) < 0.95 * base && cost(q) < best) {
      best = cost(q);
      Q = q;
    }
  return std::max(1, std::min(qmax, env_int("MDE_RING_Q", Q)));  // (Q lies in 1 .. qmax: unset changes nothing)
}

static bool choose_sizes(const mde_plan* plan, int d, RingSizes* z) {
  const int64_t nloc = plan->row_hi - plan->row_lo;
  if (d < 1 || d > 4 || nloc <= 0 || plan->H <= 0) return false;
  const int mode = panel_mode();
  if (mode == 0) return false;
  // Geometry: NRB row blocks x Q column groups ~ one workgroup per CU (256).  Tall blocks first:
  // the staging volume is NRB x table bytes (every workgroup streams the table past its rows), and
  // many rows per consumer wave keep the distinct-rows iterations full.  The block height is capped
  // by what fits the LDS next to a ring of >= 8 chunks (ring_row_cap); the CUs left over are filled
  // with column groups of at least `minch` chunks each (one ring window), whose partial rows a second
  // launch adds.  Config 4 (n = 1M, d = 2): 128 blocks of 7872 rows x 2 column groups; an 8-way shard
  // of it: 16 blocks x 16 groups; a dense 40k-node problem: 32 blocks of 1280 rows x 8 groups.
  const int C = ring_chunk_cols(d);
  const int64_t nc = (plan->n + C - 1) / C;
  if (nc > 65535 || nc < 2) return false;
  // (a stream ends with a few thin iterations -- the waiting entries drain under the distinct-rows rule --
  // and is padded to whole blocks: a column group must be long enough to amortise that; 10 chunks are
  // the column counts round 3 tuned with chunks twice as wide)
  const int minch = std::max(1, env_int("MDE_RING_MINCH", 10));
  const int qmax = (int)std::min<int64_t>(16, std::max<int64_t>(1, nc / minch));
  int64_t pr = (nloc * qmax + 255) / 256;
  if (pr < 64 * MDE_RING_NCW) pr = 64 * MDE_RING_NCW;  // >= 64 rows per consumer wave, even if CUs stay empty
  pr = env_int("MDE_RING_ROWS", (int)pr);
  if (pr > nloc) pr = nloc;
  pr = ((pr + 63) / 64) * 64;
  const int64_t pr_max = ring_row_cap(d);
  if (pr > pr_max) pr = pr_max;
  const int64_t nrb = (nloc + pr - 1) / pr;
  int Q = choose_col_groups(plan, nrb, qmax, nc);
  if (nrb * Q > MDE_MAX_PARTIALS) return false;
  const int jb = bits_for_u64((uint64_t)nc - 1);
  if (bits_for_u64((uint64_t)(nrb * Q * MDE_RING_NCW)) + jb > 32) return false;
  if (mode != 1) {
    // auto: a 64-entry iteration must fit the ring window, and the launch must be worth its fixed
    // costs: either the table overflows L2 (the CSR kernel's gathers go to HBM), or there are enough
    // half-edges that 64 B of L2 traffic per 8-byte gather is what the CSR kernel spends its time on
    // (40k nodes, 100M half-edges: 0.60 -> 0.30 ms per evaluation)
    // Round 6: in that regime the cost model is asked too, with both sides' fixed costs (below); d = 1 and 4 stay
    if (mid_regime(plan, d) && d != 2 && d != 3) return false;
  }
  const int S = ring_slots_for(d, (int)pr);
  if (S < 6) return false;
  int span = ring_max_span(S);
  span = std::min(S - 2, std::max(1, env_int("MDE_RING_SPAN", span)));  // (ring_max_span lies in 1 .. S - 2 for S >= 6)
  // auto (rounds 3-5): "a pair of 64-entry iterations must fit the ring window", i.e. >= 128 / (0.8 span) entries
  // per consumer wave and chunk -- which sent d = 3 at n = 1M, n >= 1.6M at degree 50 and everything sparser to
  // the CSR kernels at 1.1-1.7 ms per 1e8 half-edges, although the ring kernel with half-filled iterations takes
  // 0.27-0.5 there (profiles/r06_cliff_probe.txt).  Round 6: the cost model decides (sparse streams pad, so their
  // iterations are priced at 1.4 x the minimum; the count after scheduling is checked again in build_ring).
  if (mode != 1) {
    const double its = 1.4 * (double)plan->H / ((double)nrb * Q * MDE_RING_NCW * 64.0);
    if (ring_time_us(its, (int)nc, Q, (int)(nrb * Q)) > 0.75 * csr_time_us(plan, d)) return false;
    if (mid_regime(plan, d) &&
        plan->ring.cost_scale * ring_time_us(its, (int)nc, Q, (int)(nrb * Q)) + MDE_RING_FIXED_US >
            0.7 * (csr_time_us(plan, d) + MDE_CSR_FIXED_US))
      return false;
  }
  z->qmax = qmax;
  z->R = (int)pr;
  z->NRB = (int)nrb;
  z->Q = Q;
  z->C = C;
  z->NC = (int)nc;
  z->S = S;
  z->ring_off = ring_off_for(d, (int)pr);
  z->span = span;
  z->JB = jb;
  return true;
}

static void ring_free(mde_ring_layout& L) {
  if (L.packed) (void)hipFree(L.packed);
  if (L.eid) (void)hipFree(L.eid);
  if (L.hdr) (void)hipFree(L.hdr);
  if (L.wave_iter) (void)hipFree(L.wave_iter);
  if (L.partial) (void)hipFree(L.partial);
  void* extra[] = {L.slot_row, L.hub_rows, L.hub_seg, L.hub_first, L.hub_partial};
  for (void* q : extra)
    if (q) (void)hipFree(q);
  L = mde_ring_layout();
}
void mde_ring_release(mde_plan* plan) { ring_free(plan->ring); }

// layout the fused kernel will use for dimension d: 0 = CSR, 1 = LDS ring (built on first
// request).  Negative: error.
extern "C" int mde_plan_layout(mde_plan* plan, int32_t d, void* stream) {
  if (!plan || d <= 0) return MDE_E_INVALID;
  if (plan->ring.packed && plan->ring.d == d) return 1;
  RingSizes z;
  if (!choose_sizes(plan, d, &z)) return 0;
  if (plan->ring.rejected_d == d && panel_mode() != 1) return 0;
  const int rc = build_ring(plan, d, z, mde_stream(stream));
  if (rc == 0) plan->ring.rejected_d = d;
  return rc;
}

// number of entries of a per-half-edge parameter array in the given layout (layout 1: the padded
// stream + MDE_RING_CB_VALUES spare entries, where a codebook stream keeps its value table)
extern "C" int64_t mde_plan_layout_half_edges(const mde_plan* plan, int32_t layout) {
  if (!plan) return 0;
  return (layout == 1 && plan->ring.packed) ? plan->ring.H + MDE_RING_CB_VALUES : plan->H;
}

// dst[0] (device double) <- the loss of the plan's last mde_average_distortion in double, before its rounding to float
extern "C" int mde_plan_loss_double(const mde_plan* plan, double* dst, void* stream) {
  if (!plan || !dst) return MDE_E_INVALID;
  MDE_HIP(hipMemcpyAsync(dst, plan->partials + MDE_PARTIALS_LOSS_D, sizeof(double), hipMemcpyDeviceToDevice, mde_stream(stream)));
  return MDE_OK;
}

extern "C" int mde_plan_ring_info(const mde_plan* plan, int64_t* info) {
  if (!plan || !info) return MDE_E_INVALID;
  const mde_ring_layout& L = plan->ring;
  for (int i = 0; i < 16; ++i) info[i] = 0;
  if (!L.packed) return MDE_OK;
  info[0] = 1;
  info[1] = L.d;
  info[2] = L.rows_per_block;
  info[3] = L.n_row_blocks;
  info[4] = L.col_groups;
  info[5] = L.n_chunks;
  info[6] = L.slots;
  info[7] = L.n_iters;
  info[8] = plan->H - L.hub_half_edges;
  info[9] = L.H;
  info[10] = L.slot_row ? 1 : 0;
  info[11] = L.n_hub_rows;
  info[12] = L.hub_half_edges;
  info[13] = L.n_hub_segs;
  info[14] = L.loss_band;
  return MDE_OK;
}

extern "C" int mde_plan_ring_loss_balance(const mde_plan* plan, double* out) {
  if (!plan || !out) return MDE_E_INVALID;
  const mde_ring_layout& L = plan->ring;
  for (int i = 0; i < 8; ++i) out[i] = 0.0;
  if (!L.packed) return MDE_OK;
  out[0] = (double)L.loss_band;
  for (int c = 0; c < 3; ++c) out[1 + c] = (double)L.class_blocks[c];
  out[4] = L.loss_share_min;
  out[5] = L.loss_share_max;
  return MDE_OK;
}

// ---------------------------------------------------------------- dispatch
// Called by mde_average_distortion.  Returns 1 when the ring kernel was launched (it also writes
// *loss_out = loss_scale * sum of the workgroups' partials; nblocks = number of partials), 0 when
// the caller should use the CSR kernel, < 0 on error.
int mde_ring_try(mde_plan* plan, const float* X, int d, const mde_func* f, float grad_scale,
                 float* grad, float inv_p, hipStream_t st, int* nblocks, float* loss_out,
                 double loss_scale) {
  if (!plan->ring.packed || plan->ring.d != d) return 0;
  const RingArgs A{plan, X, d, f->a0, f->a1, f->a0_scalar, f->a1_scalar, grad, inv_p, grad_scale, st,
                   loss_out, loss_scale};
  // the family's unit first (one code object touched per process), the run-time functor otherwise
  int rc = 0;
  if (f->kind_neg != MDE_F_NONE)
    rc = mde_ring_launch_pushpull(A, f, nblocks);
  else if (f->kind == MDE_F_LOG1P)
    rc = mde_ring_launch_log1p(A, f, nblocks);
  else if (f->kind == MDE_F_L_QUADRATIC || f->kind == MDE_F_L_WEIGHTED_QUADRATIC || f->kind == MDE_F_L_ABSOLUTE ||
           f->kind == MDE_F_L_HUBER)
    rc = mde_ring_launch_loss(A, f, nblocks);
  else if (f->kind == MDE_F_L_CUBIC || f->kind == MDE_F_L_POWER || f->kind == MDE_F_L_LOGISTIC ||
           f->kind == MDE_F_L_FRACTIONAL || f->kind == MDE_F_L_SOFT_FRACTIONAL)
    rc = mde_ring_launch_loss2(A, f, nblocks);
  else if (f->kind == MDE_F_LOGISTIC || f->kind == MDE_F_SIGMOID || f->kind == MDE_F_HINGE || f->kind == MDE_F_POWER ||
           f->kind == MDE_F_INVPOWER || f->kind == MDE_F_LOGRATIO)
    rc = mde_ring_launch_penalty2(A, f, nblocks);
  else
    rc = mde_ring_launch_penalty(A, f, nblocks);
  if (rc == 0) rc = mde_ring_launch_runtime(A, f, nblocks);
  if (rc == 1 && plan->ring.n_hub_rows > 0) {
    const int hrc = mde_ring_launch_hub(A, f);
    if (hrc != MDE_OK) return hrc;
  }
  return rc;
}

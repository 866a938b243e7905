// mde_solver.h -- what the solver-side units share (internal): the layout of the work buffer, the host
// mirror and the gate of a pre-enqueued step, and the host functions that cross the units.
//   mde_vec.hip    axpy, vector statistics, column sums / centring, anchors, rows on a sphere
//   mde_std.hip    Gram matrices, right-multiply, the Standardized tangent projection and retraction
//   mde_lbfgs.hip  the device-resident L-BFGS memory and its direction step
//   mde_turn.hip   one solver iteration as two calls
// A kernel is launched only from the unit that defines it; the units reach each other through the host
// functions declared at the end of this file.
#pragma once
#include "mde_common.h"

// mde_mfma.hip: the projections' kernels at widths 32 / 64 / 128
bool mde_mfma_width_ok(int d);
int mde_mfma_colmean(int64_t n, int d, const float* Z, double* partial, double* mean, hipStream_t st);
int mde_mfma_gram(int64_t n, int d, const float* A, const float* B, const double* mean, double* out, double* partial,
                  int64_t max_partial, hipStream_t st);
int mde_mfma_rmul(int64_t n, int d, const float* A, const double* M, const double* mean, float alpha, const float* base,
                  float* out, hipStream_t st);

// ---------------------------------------------------------------- work buffer layout
// [0, 4096)                    small scalars / staging
// [4096, 4096 + 8 d^2)         d x d matrices (Gram result, Newton-Schulz iterates, M)
// [4096 + 8 d^2, ...)          reduction partials (<= MDE_PARTIAL_DOUBLES)
#define MDE_SMALL_DOUBLES 4096
#define MDE_PARTIAL_DOUBLES (4 << 20)
#define MDE_RED_BLOCKS 256
// the small area, in doubles (one place: the users are spread over the four units):
//   [0, 2048)      column means, Gram staging and other per-launch scalars
//   [2304, 3072)   k_lb_fused: three rows of MDE_LB_FUSED_MAXBLOCKS arrival flags (32-bit words)
//   [3072, 3076)   k_lb_fused / k_lb_rescue: gave-up, done and rescue-count words; [3076, 3088) probe stamps (-DMDE_LB_PROBE)
//   [3200]         the gate word of a pre-enqueued L-BFGS step (mde_turn_*)
//   [4064, 4096)   arrival tickets of the reductions that finish in their last workgroup
#define MDE_WS_MEAN_END 2048
#define MDE_WS_LB_FLAGS 2304
#define MDE_WS_LB_VERDICT 3072
#define MDE_WS_LB_VERDICT_END 3088
#define MDE_WS_TURN_GATE 3200
#define MDE_WS_TICKETS (MDE_SMALL_DOUBLES - 32)
static_assert(MDE_WS_MEAN_END <= MDE_WS_LB_FLAGS && MDE_WS_LB_VERDICT_END <= MDE_WS_TURN_GATE &&
                  MDE_WS_TURN_GATE + 1 <= MDE_WS_TICKETS && MDE_WS_TICKETS + 32 == MDE_SMALL_DOUBLES,
              "small area of the work buffer: regions overlap");
static inline double* work_mats(double* work) { return work + MDE_SMALL_DOUBLES; }
// arrival counters of the kernels that finish their reduction in the last workgroup: the last 32
// doubles of the small area (zero between launches; the caller zeroes the buffer once)
enum { TK_STATS = 0, TK_GRAM = 1, TK_CENTER = 2, TK_LB_STAGE = 3, TK_LB_COMBINE = 4, TK_RETRACT = 5 };
static inline unsigned int* work_ticket(double* work, int which) {
  return reinterpret_cast<unsigned int*>(work + MDE_WS_TICKETS) + which;
}
static inline double* work_partials(double* work, int d) {
  return work + MDE_SMALL_DOUBLES + 8 * (int64_t)d * d;
}
// the flag words of the fused kernel: doubles [MDE_WS_LB_FLAGS, MDE_WS_LB_VERDICT) of the work buffer's small area
// (three rows of MDE_LB_FUSED_MAXBLOCKS 32-bit words; zero or an older epoch between launches), the verdict
// words right behind them
static inline unsigned int* work_lb_flags(double* work) { return reinterpret_cast<unsigned int*>(work + MDE_WS_LB_FLAGS); }
// the gate word of the pre-enqueued L-BFGS step (MdeGate): a double of the work buffer's small area nobody
// else uses
static inline unsigned int* work_turn_gate(double* work) { return reinterpret_cast<unsigned int*>(work + MDE_WS_TURN_GATE); }

// eight block-wide reductions with two barriers: wave results to LDS, thread q < 8 combines the waves
// and publishes partial[q * nb + b] (rows in max_mask: maxima)
__device__ __forceinline__ void mde_publish8(const double (&v)[8], unsigned max_mask, double* partial, int nb, int b) {
  __shared__ double sm8[MDE_BLOCK / 64][8];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    const double r = ((max_mask >> q) & 1u) ? mde_wave_max(v[q]) : mde_wave_sum(v[q]);
    if (lane == 0) sm8[wave][q] = r;
  }
  __syncthreads();
  if (threadIdx.x < 8) {
    const int q = threadIdx.x;
    double r = sm8[0][q];
#pragma unroll
    for (int w = 1; w < MDE_BLOCK / 64; ++w) r = ((max_mask >> q) & 1u) ? (sm8[w][q] > r ? sm8[w][q] : r) : r + sm8[w][q];
    mde_st_partial(partial + q * nb + b, r);
  }
}

// ---------------------------------------------------------------- host mirror of the solver's read-back
// The last kernel of an evaluation can write [loss | status | pad | board[0,24)] straight into the pinned
// host mirror (device-visible at the same address) instead of a copy being enqueued behind it: one launch
// (~4 us of a ~0.1 ms iteration) less.  host == nullptr: nothing is written.
struct MdeMirror {
  const float* loss_dev;
  const int32_t* status;
  const double* board;   // the device board whose first 8 doubles are `stats` of the kernel
  char* host;
  int head_bytes;        // bytes of [loss | status | pad] in front of the board
  double seq;            // written behind the 24 board entries once they are out (polled by the host)
  // mde_turn_*: the first pass of the line search at t = 1 decided HERE (the host reads the verdict in
  // mirrored board slot 8 and does not test again), and a word that opens or closes the L-BFGS step of
  // the next iteration, which is queued right behind this kernel (see MdeGate).  gate == nullptr: none.
  unsigned int* gate;
  unsigned int gate_value;
  double f0, c1, c2;
};
// A launch that runs only when the iteration before it accepted its first trial point: the kernels of
// the next L-BFGS direction update are enqueued BEHIND an iteration's last kernel, before the host has
// seen its result (the host's turn-around -- mirror write, poll, test, launch -- was 15 us in which the
// GPU idled, `tools/iter_trace.sh`); that last kernel writes `value` to the word when the trial is
// accepted, anything else when it is not, and the gated kernels leave at once unless they find `value`.
// word == nullptr: an ordinary launch.
struct MdeGate {
  const unsigned int* word;
  unsigned int value;
};
__device__ __forceinline__ bool mde_gate_closed(const MdeGate& g) {
  return g.word != nullptr && __hip_atomic_load(g.word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != g.value;
}
// Where the TAGGED copy of the record lives: four 64-byte lines behind the plain mirror, each seven payload doubles
// and the sequence number -- [loss, status, board[0..24)] -- written by ONE store instruction of one wave, so that a
// line and its tag arrive together whatever the order the lines reach host memory in.  (Round 6: the plain form --
// data, system-scope fences, then the sequence word in a line of its own -- let the host read a record ONE
// ITERATION OLD about once in thirty cold-started solves: the sequence word can pass the data lines on the way to
// host memory (the solves' iterates were unaffected -- the device decides the trial from device memory -- but the
// recorded loss and step size of that iteration were the previous one's, and the bit-for-bit test of the turn calls
// against the call-by-call loop failed now and then).)
#define MDE_MIRROR_TAG_LINES 4
__host__ __device__ __forceinline__ double* mde_mirror_tagged(const double* host_board) {
  return reinterpret_cast<double*>((reinterpret_cast<uintptr_t>(host_board + 32) + 63) & ~(uintptr_t)63);
}
__device__ __forceinline__ void mde_mirror_write(const MdeMirror& m) {
  if (!m.host) return;
  __shared__ double s_pay[7 * MDE_MIRROR_TAG_LINES];
  __threadfence_block();
  __syncthreads();  // the statistics rows written by this block are visible to it
  double* hb = reinterpret_cast<double*>(m.host + m.head_bytes);
  if (threadIdx.x < 24 && !(m.gate && threadIdx.x == 8)) {  // (slot 8: the verdict below, when there is one)
    const volatile double* b = m.board;
    s_pay[2 + threadIdx.x] = b[threadIdx.x];
  }
  if (threadIdx.x >= 24 && threadIdx.x < 26) s_pay[2 + threadIdx.x] = 0.0;  // (spare payload slots)
  if (threadIdx.x == 32) s_pay[0] = (double)*reinterpret_cast<const volatile float*>(m.loss_dev);
  if (threadIdx.x == 33) s_pay[1] = m.status ? (double)*reinterpret_cast<const volatile int32_t*>(m.status) : 0.0;
  if (m.gate && threadIdx.x == 34) {
    // [ref: lbfgs.py:88-110, first pass of the bracketing loop at t = 1: finite, Armijo, curvature]
    // (separately rounded product and sum: the value the host-side search computes)
    // (five independent loads in flight at once: relaxed device-scope loads, not `volatile` ones, which
    // the compiler keeps apart -- a memory latency each, in the last kernel of every iteration)
    const double gtd_new = __hip_atomic_load(m.board + 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const double gtd0 = __hip_atomic_load(m.board + 16, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const double nonfinite = __hip_atomic_load(m.board + 4, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const double f_new = (double)__hip_atomic_load(m.loss_dev, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const int st = m.status ? __hip_atomic_load(m.status, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0;
    const bool bad = !(fabs(f_new) <= 1.7976931348623157e308) || nonfinite != 0.0;
    const bool accept = !bad && !(f_new > __dadd_rn(m.f0, __dmul_rn(m.c1, gtd0))) && (fabs(gtd_new) <= -__dmul_rn(m.c2, gtd0));
    s_pay[2 + 8] = accept ? 1.0 : 0.0;
    *m.gate = (accept && st == 0) ? m.gate_value : 0u;
  }
  __syncthreads();
  // the plain mirror (what rounds 3-5 read; kept for whoever looks at the pinned buffer directly)
  if (threadIdx.x < 24) hb[threadIdx.x] = s_pay[2 + threadIdx.x];
  if (threadIdx.x == 32) *reinterpret_cast<float*>(m.host) = (float)s_pay[0];
  if (threadIdx.x == 33) *reinterpret_cast<int32_t*>(m.host + 4) = (int32_t)s_pay[1];
  // the tagged lines: the second wave's lanes 0..31 write 32 consecutive doubles, slot 7 of every line the tag
  if (threadIdx.x >= 64 && threadIdx.x < 64 + 8 * MDE_MIRROR_TAG_LINES) {
    const int t = (int)threadIdx.x - 64;
    mde_mirror_tagged(hb)[t] = (t & 7) == 7 ? m.seq : s_pay[(t >> 3) * 7 + (t & 7)];
  }
  // the sequence word goes out behind the data: every writer fences to system scope, then one thread
  // publishes (the host polls it instead of waiting for the stream's completion signal)
  __threadfence_system();
  __syncthreads();
  if (threadIdx.x == 0) {
    hb[24] = m.seq;
    __threadfence_system();
  }
}

// ---------------------------------------------------------------- host functions that cross the units
// mde_vec.hip
int mde_axpy_impl(int64_t N, float alpha, const float* x, const float* y, float* out, hipStream_t st);
int mde_vec_stats_impl(int64_t N, const float* g, const float* d, const float* x, double* stats, double* work,
                       hipStream_t st, MdeMirror mirror = MdeMirror{});
int mde_center_impl(int64_t n, int d, float* Z, double* work, hipStream_t st, const float* X0 = nullptr,
                    const float* DIR = nullptr, float t = 0.0f, int halves = 3, double scale = 1.0);
// mde_std.hip
int mde_std_tangent_stats_impl(int64_t n, int32_t d, const float* X, float* Z, const float* dir, double* stats,
                               double* work, void* stream, MdeMirror mirror);
// mde_lbfgs.hip
int mde_lbfgs_dev_step_impl(mde_lbfgs* o, const float* g, float* g_prev, const float* d, float t, float* d_out,
                            double* stats, double* work, void* stream, MdeGate gate);

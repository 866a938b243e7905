// mde_turn.hip -- one solver iteration as two calls: host code only, every launch goes through the
// other solver units (mde_solver.h).
//   [ref: the loop accelerated is pymde/optim.py:100-175 + pymde/lbfgs.py:390-590]
#include "mde_solver.h"

#include <atomic>
#include <cmath>

static bool turn_pre_enabled() {
  static const bool on = getenv("MDE_TURN_NOPRE") == nullptr;  // (design probe: no look-ahead of the L-BFGS step)
  return on;
}

// One iteration: [L-BFGS step unless step_done] retraction of X + dir, evaluation, statistics -- whose
// kernel also DECIDES the first pass of the line search (f0, c1, c2: MdeMirror) -- and, with allow_pre, the
// L-BFGS step of the iteration after this one behind a gate that opens iff this trial is accepted.
static int turn_enqueue_impl(mde_turn_desc* T, int32_t cur, float t_prev, double f0, double c1, double c2,
                             bool allow_pre, bool step_done, void* stream) {
  if (!T || (cur != 0 && cur != 1) || (T->kind != 0 && T->kind != 1)) return MDE_E_INVALID;
  const int64_t N = T->n * (int64_t)T->d;
  float* Xc = T->X[cur];
  float* Xt = T->X[1 - cur];
  int rc = MDE_OK;
  if (!step_done) {
    rc = mde_lbfgs_dev_step_impl(T->lbfgs, T->g, T->g_prev, T->dir, t_prev, T->dir, T->board + 16, T->work, stream,
                                 MdeGate{nullptr, 0u});
    if (rc != MDE_OK) return rc;
  }
  if (T->kind == 0)
    rc = mde_center_step(T->n, T->d, Xc, T->dir, 1.0f, Xt, T->work, stream);
  else
    rc = mde_std_retract_step(T->n, T->d, Xc, T->dir, 1.0f, Xt, 1, T->work, T->status, stream);
  if (rc != MDE_OK) return rc;
  rc = mde_average_distortion(T->plan, Xt, T->d, T->func, 1.0f, T->g, T->loss_dev, stream);
  if (rc != MDE_OK) return rc;
  // the last kernel writes [loss | status | board] into the pinned mirror itself (no copy behind it)
  static std::atomic<unsigned long long> turns{0};
  const unsigned long long id = turns.fetch_add(1ull) + 1ull;
  T->seq = (double)id;  // (exact in a double for 2^53 iterations)
  unsigned int gate_value = (unsigned int)(id & 0xffffffffull);
  if (gate_value == 0u) gate_value = 1u;
  MdeMirror mirror{T->loss_dev, T->status, T->board, reinterpret_cast<char*>(T->host_dst),
                   (int)(T->read_bytes - 8 * 24), T->seq, work_turn_gate(T->work), gate_value, f0, c1, c2};
  if (T->kind == 0)
    rc = mde_vec_stats_impl(N, T->g, T->dir, Xt, T->board, T->work, mde_stream(stream), mirror);
  else
    rc = mde_std_tangent_stats_impl(T->n, T->d, Xt, T->g, T->dir, T->board, T->work, stream, mirror);
  if (rc != MDE_OK) return rc;
  T->pre_id = 0.0;
  if (allow_pre && turn_pre_enabled()) {
    // the direction update of the NEXT iteration (an accepted first trial is the step t = 1), gated
    rc = mde_lbfgs_dev_step_impl(T->lbfgs, T->g, T->g_prev, T->dir, 1.0f, T->dir, T->board + 16, T->work, stream,
                                 MdeGate{work_turn_gate(T->work), gate_value});
    if (rc != MDE_OK) return rc;
    T->pre_id = (double)gate_value;
  }
  return MDE_OK;
}

extern "C" int mde_turn_enqueue(mde_turn_desc* T, int32_t cur, float t_prev, double f0, double c1, double c2,
                                int32_t allow_pre, void* stream) {
  // a gated L-BFGS step that has run but was not followed by its iteration (mde_turn_wait with allow_next = 0
  // on an accepted trial; out[20] said so) IS this iteration's step: running it again would stage s = t d with
  // the direction the first run has already overwritten and y = g - g_prev = 0
  const bool pending = T && T->pre_id == -1.0;
  if (pending) T->pre_id = 0.0;
  return turn_enqueue_impl(T, cur, t_prev, f0, c1, c2, allow_pre != 0, pending, stream);
}

extern "C" int mde_turn_wait(mde_turn_desc* T, int32_t cur, double f0, int32_t allow_next, double c1, double c2,
                             double eps_pre, double* out, void* stream) {
  if (!T || !out || (cur != 0 && cur != 1)) return MDE_E_INVALID;
  // Poll the sequence word the iteration's last kernel writes behind its data (a completion signal
  // takes microseconds longer to reach a waiting thread); the stream is queried now and then, so the
  // wait also ends -- with everything visible -- should the word never show up.
  {
    const volatile double* flag = T->host_board + 24;
    hipStream_t st = mde_stream(stream);
    for (unsigned spins = 0;; ++spins) {
      if (*flag == T->seq) break;
      if ((spins & 255u) == 255u) {
        const hipError_t e = hipStreamQuery(st);
        if (e == hipSuccess) break;
        if (e != hipErrorNotReady) MDE_HIP(e);
      }
    }
    std::atomic_thread_fence(std::memory_order_acquire);
  }
  // The record is read from the TAGGED lines (mde_mirror_write): every 64-byte line carries the sequence number in
  // its last slot and arrives whole, so a line whose tag is this iteration's holds this iteration's values.  A line
  // that is still on its way is waited for; should one never arrive (it cannot once the stream is idle) that is an error.
  double pay[7 * MDE_MIRROR_TAG_LINES];
  {
    const volatile double* tg = mde_mirror_tagged(T->host_board);
    hipStream_t st = mde_stream(stream);
    bool synced = false;
    for (unsigned spins = 0;; ++spins) {
      bool ok = true;
      for (int l = 0; l < MDE_MIRROR_TAG_LINES; ++l) ok = ok && tg[8 * l + 7] == T->seq;
      if (ok) {
        std::atomic_thread_fence(std::memory_order_acquire);
        for (int l = 0; l < MDE_MIRROR_TAG_LINES; ++l)
          for (int q = 0; q < 7; ++q) pay[7 * l + q] = tg[8 * l + q];
        // (a line rewritten between the tag check and the copy is impossible: the next iteration is not enqueued yet)
        break;
      }
      if ((spins & 4095u) == 4095u) {
        if (synced) {
          mde_set_error("mde_turn_wait: the iteration's record never reached the host mirror");
          return MDE_E_HIP;
        }
        MDE_HIP(hipStreamSynchronize(st));
        synced = true;
      }
    }
  }
  const double f_new = pay[0];
  const double* hb = pay + 2;  // board[0..24)
  const int32_t status_word = (int32_t)pay[1];
  for (int q = 0; q < 8; ++q) {
    out[4 + q] = hb[q];
    out[12 + q] = hb[16 + q];
  }
  out[0] = f_new;
  out[3] = (double)status_word;
  // the first pass of the bracketing loop at t = 1 (lbfgs.py:88-110): not bad, Armijo, curvature -- decided
  // by the iteration's last kernel (mde_mirror_write) from f0 as passed when it was enqueued; the gate of a
  // pre-enqueued L-BFGS step followed THAT verdict, so it is the one to go by
  (void)f0;
  const bool accept = hb[8] != 0.0;
  out[1] = accept ? 1.0 : 0.0;
  out[2] = 0.0;
  const bool step_done = accept && status_word == 0 && T->pre_id > 0.0;  // (its gate opened)
  T->pre_id = 0.0;
  out[20] = 0.0;
  if (step_done && !allow_next) {
    // the speculative step of the next iteration has run (g_prev <- g, a new history pair, dir and the
    // direction statistics overwritten) and the caller does not want that iteration launched now: the step
    // stays PENDING -- the next mde_turn_enqueue on this descriptor takes it as done -- and the caller is told
    T->pre_id = -1.0;
    out[20] = 1.0;
  }
  if (accept && allow_next && status_word == 0) {
    // (hb[1]: |g|^2 at the accepted point -- the next iteration goes on to another one iff it is above eps)
    const bool allow_pre = eps_pre >= 0.0 && std::sqrt(hb[1]) > eps_pre;
    const int rc = turn_enqueue_impl(T, 1 - cur, 1.0f, f_new, c1, c2, allow_pre, step_done, stream);
    if (rc != MDE_OK) return rc;
    out[2] = 1.0;
  }
  return MDE_OK;
}

// mde_rows.hip -- the per-row solver of a dense placement: the objective of
// pymde_amd.DensePlacement is a sum of n independent d-dimensional problems (d <= 8), one per new row, and these two
// kernels advance ALL of them in lock step, one BFGS iteration with a backtracking line search per row, so that every
// row has its own step length, its own curvature and its own stopping test.
//
// One thread per row; the row's vectors and its d x d inverse-Hessian estimate stay in registers (DC = d padded with
// zeros to 1, 2, 3 or 8, the widths of the dense walk).  The state is float32; the inner products, the Armijo test and
// the BFGS update are formed in double from the float32 terms and rounded once, as the dense walk forms its sums.  No
// floating-point atomics: the only atomics are the integer adds of the three status counters, one per wave.
//
//   k_rows_init   from the evaluation at the start: f = row_loss / n_c, g = row_grad, H = I, p = -g,
//                 t = min(1, 1 / |g|_1) (the reference's first step), fresh; converged if |g|_2 <= eps
//   k_rows_step   from the evaluation at x_trial: accept (Armijo, c1 = 1e-4) -> BFGS update, adopt, stopping tests,
//                 new direction, t = 1; reject -> interpolated t clamped to [0.1 t, 0.5 t], step floor
// and both write the next trial point: x + t p for an active row, x for every other row, whose state is not touched.
//
// flags[i]: bits 0-1 the status (MDE_ROWS_ACTIVE / CONVERGED / STALLED), bit 2 "fresh" (H is still the identity it
// was set to: the first accepted pair scales it by s.y / y.y, Nocedal & Wright (6.20)), bits 3.. the number of
// accepted steps in a row that lowered f by at most 1e-7 |f| (two of them stall the row: what ends Absolute, whose
// gradient never vanishes).
#include <math.h>

#include "mde_common.h"

#define ROWS_MAX_D 8
#define ROWS_C1 1e-4
#define ROWS_CURV 1e-10       // the pair (s, y) is used when s.y > ROWS_CURV |s| |y|
#define ROWS_SMALL 1e-7       // a decrease of at most ROWS_SMALL |f| is "small"
#define ROWS_FLOOR 1e-10      // the row stalls when t max|p| <= ROWS_FLOOR max(1, max|x|)
#define ROWS_FRESH 4
#define ROWS_COUNT_SHIFT 3

// counts[status] += the rows of this wave with that status (status < 0: no row)
__device__ __forceinline__ void rows_count(int status, unsigned long long* counts) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int v = 0; v < 3; ++v) {
    const unsigned long long m = __ballot(status == v);
    if (lane == 0 && m) atomicAdd(counts + v, (unsigned long long)__popcll(m));
  }
}

template <int DC>
__global__ __launch_bounds__(MDE_BLOCK) void k_rows_init(int64_t n, int d, double n_c, float eps,
                                                         const float* __restrict__ x,
                                                         const double* __restrict__ row_loss,
                                                         const float* __restrict__ row_grad, double* __restrict__ f,
                                                         float* __restrict__ g, float* __restrict__ H,
                                                         float* __restrict__ p, float* __restrict__ t,
                                                         int32_t* __restrict__ flags, float* __restrict__ x_trial,
                                                         unsigned long long* __restrict__ counts) {
  const int64_t i = (int64_t)blockIdx.x * MDE_BLOCK + threadIdx.x;
  int status = -1;
  if (i < n) {
    const double fi = row_loss[i] / n_c;
    float gi[DC];
    double l1 = 0.0, l2 = 0.0;
    bool finite = isfinite(fi);
#pragma unroll
    for (int k = 0; k < DC; ++k) {
      gi[k] = k < d ? row_grad[i * d + k] : 0.0f;
      finite = finite && isfinite(gi[k]);
      l1 += fabs((double)gi[k]);
      l2 = fma((double)gi[k], (double)gi[k], l2);
    }
    status = !finite ? MDE_ROWS_STALLED : (sqrt(l2) <= (double)eps ? MDE_ROWS_CONVERGED : MDE_ROWS_ACTIVE);
    const float ti = (float)fmin(1.0, 1.0 / l1);
    f[i] = fi;
    t[i] = ti;
    flags[i] = status | ROWS_FRESH;
#pragma unroll
    for (int k = 0; k < DC; ++k)
      if (k < d) {
        const float xk = x[i * d + k];
        g[i * d + k] = gi[k];
        p[i * d + k] = -gi[k];
        x_trial[i * d + k] = status == MDE_ROWS_ACTIVE ? (float)fma((double)ti, -(double)gi[k], (double)xk) : xk;
#pragma unroll
        for (int b = 0; b < DC; ++b)
          if (b < d) H[(i * d + k) * d + b] = k == b ? 1.0f : 0.0f;
      }
  }
  rows_count(status, counts);
}

template <int DC>
__global__ __launch_bounds__(MDE_BLOCK) void k_rows_step(int64_t n, int d, double n_c, float eps,
                                                         float* __restrict__ x, double* __restrict__ f,
                                                         float* __restrict__ g, float* __restrict__ H,
                                                         float* __restrict__ p, float* __restrict__ t,
                                                         int32_t* __restrict__ flags, float* __restrict__ x_trial,
                                                         const double* __restrict__ row_loss,
                                                         const float* __restrict__ row_grad,
                                                         unsigned long long* __restrict__ counts) {
  const int64_t i = (int64_t)blockIdx.x * MDE_BLOCK + threadIdx.x;
  int status = -1;
  if (i < n) {
    const int fl = flags[i];
    status = fl & 3;
    if (status != MDE_ROWS_ACTIVE) {
#pragma unroll
      for (int k = 0; k < DC; ++k)
        if (k < d) x_trial[i * d + k] = x[i * d + k];
    } else {
      int fresh = fl & ROWS_FRESH, small = fl >> ROWS_COUNT_SHIFT;
      float xi[DC], gi[DC], pi[DC], xt[DC], gt[DC];
#pragma unroll
      for (int k = 0; k < DC; ++k) {
        const bool in = k < d;
        xi[k] = in ? x[i * d + k] : 0.0f;
        gi[k] = in ? g[i * d + k] : 0.0f;
        pi[k] = in ? p[i * d + k] : 0.0f;
        xt[k] = in ? x_trial[i * d + k] : 0.0f;
        gt[k] = in ? row_grad[i * d + k] : 0.0f;
      }
      const double fi = f[i], ft = row_loss[i] / n_c;
      float ti = t[i];
      double gp = 0.0;
      bool finite = isfinite(ft);
#pragma unroll
      for (int k = 0; k < DC; ++k) {
        gp = fma((double)gi[k], (double)pi[k], gp);
        finite = finite && isfinite(gt[k]);
      }
      if (finite && ft <= fi + ROWS_C1 * (double)ti * gp) {
        // ---- accept: the pair (s, y), the update, the new iterate
        double s[DC], y[DC], sy = 0.0, ss = 0.0, yy = 0.0, g2 = 0.0;
        bool same = true;
#pragma unroll
        for (int k = 0; k < DC; ++k) {
          s[k] = (double)xt[k] - (double)xi[k];
          y[k] = (double)gt[k] - (double)gi[k];
          sy = fma(s[k], y[k], sy);
          ss = fma(s[k], s[k], ss);
          yy = fma(y[k], y[k], yy);
          g2 = fma((double)gt[k], (double)gt[k], g2);
          same = same && xt[k] == xi[k];
        }
        float Hm[DC][DC];
#pragma unroll
        for (int a = 0; a < DC; ++a)
#pragma unroll
          for (int b = 0; b < DC; ++b) Hm[a][b] = (a < d && b < d) ? H[(i * d + a) * d + b] : 0.0f;
        bool h_changed = false;
        if (sy > ROWS_CURV * sqrt(ss) * sqrt(yy)) {
          if (fresh) {
            const float scale = (float)(sy / yy);
#pragma unroll
            for (int a = 0; a < DC; ++a)
#pragma unroll
              for (int b = 0; b < DC; ++b) Hm[a][b] = (a == b && a < d) ? scale : 0.0f;
            fresh = 0;
          }
          // H <- (I - rho s y^T) H (I - rho y s^T) + rho s s^T
          //    = H - rho s (H^T y)^T - rho (H y) s^T + (rho^2 y^T H y + rho) s s^T
          const double rho = 1.0 / sy;
          double Hy[DC], Hty[DC], yHy = 0.0;
#pragma unroll
          for (int a = 0; a < DC; ++a) {
            Hy[a] = 0.0;
            Hty[a] = 0.0;
#pragma unroll
            for (int b = 0; b < DC; ++b) {
              Hy[a] = fma((double)Hm[a][b], y[b], Hy[a]);
              Hty[a] = fma((double)Hm[b][a], y[b], Hty[a]);
            }
          }
#pragma unroll
          for (int a = 0; a < DC; ++a) yHy = fma(y[a], Hy[a], yHy);
          const double c = rho * rho * yHy + rho;
#pragma unroll
          for (int a = 0; a < DC; ++a)
#pragma unroll
            for (int b = 0; b < DC; ++b)
              Hm[a][b] = (float)((double)Hm[a][b] - rho * (s[a] * Hty[b] + Hy[a] * s[b]) + c * s[a] * s[b]);
          h_changed = true;
        }
        const double drop = fi - ft;
        small = drop <= ROWS_SMALL * fabs(fi) ? small + 1 : 0;
        f[i] = ft;
#pragma unroll
        for (int k = 0; k < DC; ++k) {
          xi[k] = xt[k];
          gi[k] = gt[k];
          if (k < d) {
            x[i * d + k] = xt[k];
            g[i * d + k] = gt[k];
          }
        }
        if (sqrt(g2) <= (double)eps)
          status = MDE_ROWS_CONVERGED;
        else if (same || small >= 2)
          status = MDE_ROWS_STALLED;
        else {
          double gp2 = 0.0;
#pragma unroll
          for (int a = 0; a < DC; ++a) {
            double hg = 0.0;
#pragma unroll
            for (int b = 0; b < DC; ++b) hg = fma((double)Hm[a][b], (double)gi[b], hg);
            pi[a] = (float)(-hg);
            gp2 = fma((double)gi[a], (double)pi[a], gp2);
          }
          if (!(gp2 < 0.0)) {                                   // not a descent direction: start over from -g
#pragma unroll
            for (int a = 0; a < DC; ++a) {
              pi[a] = -gi[a];
#pragma unroll
              for (int b = 0; b < DC; ++b) Hm[a][b] = (a == b && a < d) ? 1.0f : 0.0f;
            }
            fresh = ROWS_FRESH;
            h_changed = true;
          }
          ti = 1.0f;
          t[i] = ti;
#pragma unroll
          for (int k = 0; k < DC; ++k)
            if (k < d) p[i * d + k] = pi[k];
        }
        if (h_changed) {
#pragma unroll
          for (int a = 0; a < DC; ++a)
#pragma unroll
            for (int b = 0; b < DC; ++b)
              if (a < d && b < d) H[(i * d + a) * d + b] = Hm[a][b];
        }
      } else {
        // ---- reject: the minimiser of the parabola through f, g.p and f_t, kept within [0.1 t, 0.5 t]
        const double td = (double)ti, denom = ft - fi - gp * td;
        double tn = 0.5 * td;
        if (isfinite(denom) && denom > 0.0) {
          tn = -gp * td * td / (2.0 * denom);
          tn = fmin(fmax(tn, 0.1 * td), 0.5 * td);
        }
        ti = (float)tn;
        t[i] = ti;
        float pmax = 0.0f, xmax = 1.0f;
#pragma unroll
        for (int k = 0; k < DC; ++k) {
          pmax = fmaxf(pmax, fabsf(pi[k]));
          xmax = fmaxf(xmax, fabsf(xi[k]));
        }
        if ((double)ti * (double)pmax <= ROWS_FLOOR * (double)xmax) status = MDE_ROWS_STALLED;
      }
      flags[i] = status | fresh | (small << ROWS_COUNT_SHIFT);
#pragma unroll
      for (int k = 0; k < DC; ++k)
        if (k < d)
          x_trial[i * d + k] =
              status == MDE_ROWS_ACTIVE ? (float)fma((double)ti, (double)pi[k], (double)xi[k]) : xi[k];
    }
  }
  rows_count(status, counts);
}

static bool rows_args_ok(int64_t n, int32_t d, int64_t n_c, float eps) {
  return n >= 1 && n < ((int64_t)1 << 31) && d >= 1 && d <= ROWS_MAX_D && n_c >= 1 && eps >= 0.0f;
}

extern "C" int mde_rows_init(int64_t n, int32_t d, int64_t n_c, float eps, const float* x, const double* row_loss,
                             const float* row_grad, double* f, float* g, float* H, float* p, float* t, int32_t* flags,
                             float* x_trial, int64_t* counts, void* stream) {
  if (!rows_args_ok(n, d, n_c, eps) || !x || !row_loss || !row_grad || !f || !g || !H || !p || !t || !flags ||
      !x_trial || !counts) {
    mde_set_error("mde_rows_init: invalid arguments (1 <= n < 2^31, 1 <= d <= %d, n_c >= 1, eps >= 0, non-null "
                  "arrays)", ROWS_MAX_D);
    return MDE_E_INVALID;
  }
  hipStream_t st = mde_stream(stream);
  MDE_HIP(hipMemsetAsync(counts, 0, 3 * sizeof(int64_t), st));
  const dim3 grid((unsigned)((n + MDE_BLOCK - 1) / MDE_BLOCK));
  unsigned long long* cnt = reinterpret_cast<unsigned long long*>(counts);
#define ROWS_INIT(DC)                                                                                             \
  hipLaunchKernelGGL(k_rows_init<DC>, grid, dim3(MDE_BLOCK), 0, st, n, (int)d, (double)n_c, eps, x, row_loss,      \
                     row_grad, f, g, H, p, t, flags, x_trial, cnt)
  if (d == 1)
    ROWS_INIT(1);
  else if (d == 2)
    ROWS_INIT(2);
  else if (d == 3)
    ROWS_INIT(3);
  else
    ROWS_INIT(ROWS_MAX_D);
#undef ROWS_INIT
  MDE_LAUNCH_CHECK();
  return MDE_OK;
}

extern "C" int mde_rows_step(int64_t n, int32_t d, int64_t n_c, float eps, float* x, double* f, float* g, float* H,
                             float* p, float* t, int32_t* flags, float* x_trial, const double* row_loss,
                             const float* row_grad, int64_t* counts, void* stream) {
  if (!rows_args_ok(n, d, n_c, eps) || !x || !f || !g || !H || !p || !t || !flags || !x_trial || !row_loss ||
      !row_grad || !counts) {
    mde_set_error("mde_rows_step: invalid arguments (1 <= n < 2^31, 1 <= d <= %d, n_c >= 1, eps >= 0, non-null "
                  "arrays)", ROWS_MAX_D);
    return MDE_E_INVALID;
  }
  hipStream_t st = mde_stream(stream);
  MDE_HIP(hipMemsetAsync(counts, 0, 3 * sizeof(int64_t), st));
  const dim3 grid((unsigned)((n + MDE_BLOCK - 1) / MDE_BLOCK));
  unsigned long long* cnt = reinterpret_cast<unsigned long long*>(counts);
#define ROWS_STEP(DC)                                                                                             \
  hipLaunchKernelGGL(k_rows_step<DC>, grid, dim3(MDE_BLOCK), 0, st, n, (int)d, (double)n_c, eps, x, f, g, H, p, t, \
                     flags, x_trial, row_loss, row_grad, cnt)
  if (d == 1)
    ROWS_STEP(1);
  else if (d == 2)
    ROWS_STEP(2);
  else if (d == 3)
    ROWS_STEP(3);
  else
    ROWS_STEP(ROWS_MAX_D);
#undef ROWS_STEP
  MDE_LAUNCH_CHECK();
  return MDE_OK;
}

// mde_vec.hip -- the solver-side vector kernels: axpy, fused vector statistics, column sums /
// centring, anchors and rows on a sphere (the other solver units: mde_solver.h).
//   constraints  [ref: pymde/constraints.py:94-231]
//   vector ops   [ref: pymde/lbfgs.py:350-376, 461-530; pymde/optim.py:94-147]
// All reductions are two-stage (block partials in double, one fixed-order final pass): no
// atomics, bitwise reproducible.
#include "mde_solver.h"

extern "C" int64_t mde_work_doubles(int32_t d) {
  const int64_t dd = (int64_t)(d > 0 ? d : 1);
  return MDE_SMALL_DOUBLES + 8 * dd * dd + MDE_PARTIAL_DOUBLES;
}

// device -> pinned host copy on the stream (the solver's one read-back per evaluation)
extern "C" int mde_copy_to_host(void* dst_host, const void* src_dev, int64_t bytes, void* stream) {
  if (!dst_host || !src_dev || bytes < 0) return MDE_E_INVALID;
  if (bytes == 0) return MDE_OK;
  MDE_HIP(hipMemcpyAsync(dst_host, src_dev, (size_t)bytes, hipMemcpyDeviceToHost, mde_stream(stream)));
  return MDE_OK;
}

// ---------------------------------------------------------------- axpy
__global__ __launch_bounds__(MDE_BLOCK) void k_axpy(int64_t N, float alpha,
                                                    const float* __restrict__ x,
                                                    const float* __restrict__ y,
                                                    float* __restrict__ out) {
  const int64_t stride = (int64_t)gridDim.x * MDE_BLOCK;
  const int64_t N4 = N >> 2;
  const bool al = ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(y) |
                    reinterpret_cast<uintptr_t>(out)) & 15) == 0;
  if (al) {
    for (int64_t i = (int64_t)blockIdx.x * MDE_BLOCK + threadIdx.x; i < N4; i += stride) {
      const float4 a = reinterpret_cast<const float4*>(x)[i];
      const float4 b = reinterpret_cast<const float4*>(y)[i];
      reinterpret_cast<float4*>(out)[i] = make_float4(fmaf(alpha, a.x, b.x), fmaf(alpha, a.y, b.y),
                                                      fmaf(alpha, a.z, b.z), fmaf(alpha, a.w, b.w));
    }
    for (int64_t i = (N4 << 2) + (int64_t)blockIdx.x * MDE_BLOCK + threadIdx.x; i < N; i += stride)
      out[i] = fmaf(alpha, x[i], y[i]);
  } else {
    for (int64_t i = (int64_t)blockIdx.x * MDE_BLOCK + threadIdx.x; i < N; i += stride)
      out[i] = fmaf(alpha, x[i], y[i]);
  }
}

int mde_axpy_impl(int64_t N, float alpha, const float* x, const float* y, float* out, hipStream_t st) {
  hipLaunchKernelGGL(k_axpy, dim3(mde_grid((N + 3) / 4, MDE_BLOCK)), dim3(MDE_BLOCK), 0, st, N, alpha, x, y, out);
  MDE_LAUNCH_CHECK();
  return MDE_OK;
}
extern "C" int mde_axpy(int64_t N, float alpha, const float* x, const float* y, float* out,
                        void* stream) {
  if (N < 0 || (N > 0 && (!x || !y || !out))) return MDE_E_INVALID;
  if (N == 0) return MDE_OK;
  return mde_axpy_impl(N, alpha, x, y, out, mde_stream(stream));
}

// ---------------------------------------------------------------- vector statistics
// partial[q * nb + b], q: 0 g.d 1 g.g 2 sum|g| 3 max|g| 4 #nonfinite 5 d.d 6 max|d| 7 x.x
__global__ __launch_bounds__(MDE_BLOCK) void k_vec_stats(int64_t N, const float* __restrict__ g,
                                                         const float* __restrict__ d,
                                                         const float* __restrict__ x,
                                                         double* __restrict__ partial,
                                                         double* stats,
                                                         unsigned int* __restrict__ ticket, MdeMirror mirror) {
  __shared__ double smem[8];
  double gd = 0, gg = 0, g1 = 0, gm = 0, nf = 0, dd = 0, dm = 0, xx = 0;
  auto one = [&](float gv, float dvf, float xvf) __attribute__((always_inline)) {
    const double gvd = gv;
    gg += gvd * gvd;
    const double ag = fabs(gvd);
    g1 += ag;
    gm = ag > gm ? ag : gm;  // NaN never wins; counted below
    nf += (fabsf(gv) <= 3.402823466e+38f) ? 0.0 : 1.0;
    if (d) {
      const double dv = dvf;
      gd += gvd * dv;
      dd += dv * dv;
      const double ad = fabs(dv);
      dm = ad > dm ? ad : dm;
    }
    if (x) {
      const double xv = xvf;
      xx += xv * xv;
    }
  };
  // 16-byte loads (256 MB vectors at d = 128: the 4-byte form ran at 0.7 TB/s); each thread keeps its
  // own fixed subsequence, so the sums do not depend on timing
  const bool vec = ((reinterpret_cast<uintptr_t>(g) | reinterpret_cast<uintptr_t>(d ? d : g) |
                     reinterpret_cast<uintptr_t>(x ? x : g)) & 15) == 0;
  const int64_t N4 = vec ? (N >> 2) : 0;
  const float4* g4 = reinterpret_cast<const float4*>(g);
  const float4* d4 = reinterpret_cast<const float4*>(d);
  const float4* x4 = reinterpret_cast<const float4*>(x);
  const int64_t stride = (int64_t)gridDim.x * MDE_BLOCK;
  const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
  // four 16-byte loads per array in flight per thread, unpredicated in the main loop (a predicated
  // load is a branch: the loads of a trip then go out one memory latency after the other)
  int64_t i = (int64_t)blockIdx.x * MDE_BLOCK + threadIdx.x;
  if (d && x) {
    for (; i + 3 * stride < N4; i += 4 * stride) {
      float4 ga[4], da[4], xa[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        ga[u] = g4[i + u * stride];
        da[u] = d4[i + u * stride];
        xa[u] = x4[i + u * stride];
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        one(ga[u].x, da[u].x, xa[u].x);
        one(ga[u].y, da[u].y, xa[u].y);
        one(ga[u].z, da[u].z, xa[u].z);
        one(ga[u].w, da[u].w, xa[u].w);
      }
    }
  }
  // the remaining trips (fewer than four when d and x are given), their loads issued TOGETHER from clamped
  // indices and only the arithmetic predicated (round 5: 2M-element vectors on 256 workgroups are ~8 float4 per
  // thread -- one unrolled trip and then three or four dependent ones, a memory latency each: 18 -> ~11 us; the
  // elements a thread adds, and their order, are what they were)
  while (i < N4) {
    float4 ga[4], da[4], xa[4];
    bool in[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int64_t iu = i + u * stride;
      in[u] = iu < N4;
      const int64_t ic = in[u] ? iu : N4 - 1;
      ga[u] = g4[ic];
      da[u] = d ? d4[ic] : z4;
      xa[u] = x ? x4[ic] : z4;
    }
#pragma unroll
    for (int u = 0; u < 4; ++u)
      if (in[u]) {
        one(ga[u].x, da[u].x, xa[u].x);
        one(ga[u].y, da[u].y, xa[u].y);
        one(ga[u].z, da[u].z, xa[u].z);
        one(ga[u].w, da[u].w, xa[u].w);
      }
    i += 4 * stride;
  }
  for (int64_t i = (N4 << 2) + (int64_t)blockIdx.x * MDE_BLOCK + threadIdx.x; i < N; i += stride)
    one(g[i], d ? d[i] : 0.0f, x ? x[i] : 0.0f);
  const int nb = gridDim.x, b = blockIdx.x;
  const double v[8] = {gd, gg, g1, gm, nf, dd, dm, xx};
  mde_publish8(v, (1u << 3) | (1u << 6), partial, nb, b);
  // the last block to arrive reduces the partials (fixed order: independent of arrival order)
  if (!mde_last_block(ticket)) return;
  mde_final_rows(8, nb, partial, stats, (1ull << 3) | (1ull << 6));
  mde_mirror_write(mirror);
}

int mde_vec_stats_impl(int64_t N, const float* g, const float* d, const float* x, double* stats,
                       double* work, hipStream_t st, MdeMirror mirror) {
  const int nb = mde_grid(N, MDE_BLOCK * 8, MDE_RED_BLOCKS);
  hipLaunchKernelGGL(k_vec_stats, dim3(nb), dim3(MDE_BLOCK), 0, st, N, g, d, x, work + MDE_SMALL_DOUBLES, stats,
                     work_ticket(work, TK_STATS), mirror);
  MDE_LAUNCH_CHECK();
  return MDE_OK;
}

extern "C" int mde_vec_stats(int64_t N, const float* g, const float* d, const float* x,
                             double* stats, double* work, void* stream) {
  if (N <= 0 || !g || !stats || !work) return MDE_E_INVALID;
  return mde_vec_stats_impl(N, g, d, x, stats, work, mde_stream(stream));
}

// ---------------------------------------------------------------- column sums / centring
// threads are laid out (rows_per_pass x dp), dp = pow2 >= min(d,256); coalesced over columns
// STEP: Z <- X0 + t DIR first (the line-search trial point: one launch less than axpy + centring; the
// sums are those of the rounded floats, exactly what the two launches produce)
template <bool STEP>
__global__ __launch_bounds__(MDE_BLOCK) void k_colsum(int64_t n, int d, int dp, float* Z, const float* X0,
                                                      const float* DIR, float t,
                                                      double* __restrict__ partial /* [nb][d] */,
                                                      double* __restrict__ mean, unsigned int* ticket) {
  __shared__ double sm[MDE_BLOCK];
  const int tc = threadIdx.x & (dp - 1);
  const int tr = threadIdx.x / dp;
  const int rpp = MDE_BLOCK / dp;
  for (int c0 = 0; c0 < d; c0 += dp) {
    const int c = c0 + tc;
    double s = 0.0;
    if (c < d) {
      // eight rows of the thread's sequence in flight (clamped indices, the arithmetic predicated; round 5: one
      // row per trip was a memory latency per row -- 17 us for 24 MB at n = 1M, d = 2); the rows a thread adds,
      // and their order, are what they were
      const int64_t rstep = (int64_t)gridDim.x * rpp;
      for (int64_t r0 = (int64_t)blockIdx.x * rpp + tr; r0 < n; r0 += 8 * rstep) {
        float a[8], b[8];
        bool in[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          const int64_t r = r0 + u * rstep;
          in[u] = r < n;
          const int64_t rc = in[u] ? r : n - 1;
          if (STEP) {
            a[u] = DIR[rc * d + c];
            b[u] = X0[rc * d + c];
          } else {
            a[u] = Z[rc * d + c];
            b[u] = 0.0f;
          }
        }
#pragma unroll
        for (int u = 0; u < 8; ++u)
          if (in[u]) {
            float z;
            if (STEP) {
              z = fmaf(t, a[u], b[u]);
              Z[(r0 + u * rstep) * d + c] = z;
            } else {
              z = a[u];
            }
            s += (double)z;
          }
      }
    }
    __syncthreads();
    sm[threadIdx.x] = s;
    __syncthreads();
    if (tr == 0 && c < d) {
      double t = 0.0;
      for (int k = 0; k < rpp; ++k) t += sm[k * dp + tc];
      mde_st_partial(partial + (int64_t)blockIdx.x * d + c, t);
    }
  }
  // narrow matrices (ticket given): the last workgroup to arrive turns the partial sums into the
  // column means; wide ones leave that to k_colsum_final (one wave per column, in parallel)
  if (!ticket || !mde_last_block(ticket)) return;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, nb = gridDim.x;
  for (int c = wave; c < d; c += MDE_BLOCK / 64) {
    double s = 0.0;
    for (int b = lane; b < nb; b += 64) s += mde_ld_partial(partial + (int64_t)b * d + c);
    s = mde_wave_sum(s);
    if (lane == 0) mean[c] = s / (double)n;
  }
}
// mean[c] = (sum_b partial[b][c]) / n
// (one wave per column: lane-strided partial sums + a fixed-order wave reduction)
__global__ __launch_bounds__(64) void k_colsum_final(int nb, int d, int64_t n, const double* __restrict__ partial,
                                                     double* __restrict__ mean) {
  const int c = blockIdx.x;
  double s = 0.0;
  for (int b = threadIdx.x; b < nb; b += 64) s += partial[(int64_t)b * d + c];
  s = mde_wave_sum(s);
  if (threadIdx.x == 0) mean[c] = s / (double)n;
}
__global__ __launch_bounds__(MDE_BLOCK) void k_sub_mean(int64_t N, int d, float* __restrict__ Z,
                                                        const double* __restrict__ mean, double scale = 1.0) {
  const int64_t stride = (int64_t)gridDim.x * MDE_BLOCK;
  for (int64_t i0 = (int64_t)blockIdx.x * MDE_BLOCK + threadIdx.x; i0 < N; i0 += 4 * stride) {
    float z[4];
    bool in[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      in[u] = i0 + u * stride < N;
      z[u] = Z[in[u] ? i0 + u * stride : N - 1];
    }
#pragma unroll
    for (int u = 0; u < 4; ++u)
      if (in[u]) Z[i0 + u * stride] = (float)((double)z[u] - scale * mean[(i0 + u * stride) % d]);  // (scale = 1: exact)
  }
}

static int pow2_ge(int x) {
  int p = 1;
  while (p < x) p <<= 1;
  return p;
}

// halves: 1 = the column means only (left in work[0 .. d)), 2 = the subtraction only (of scale x work[0 .. d)), 3 = both
int mde_center_impl(int64_t n, int d, float* Z, double* work, hipStream_t st, const float* X0, const float* DIR,
                    float t, int halves, double scale) {
  double* mean = work;  // d doubles (d <= 2048 fits the small area)
  double* partial = work_partials(work, d);
  int dp = pow2_ge(d);
  if (dp > MDE_BLOCK) dp = MDE_BLOCK;
  const int rpp = MDE_BLOCK / dp;
  int nb = mde_grid(n, rpp * 8, MDE_RED_BLOCKS);
  // (a last workgroup adding d columns of nb partials one after the other only pays for a few columns)
  const bool fused_final = d <= 16;
  if (!(halves & 1)) {
    hipLaunchKernelGGL(k_sub_mean, dim3(mde_grid(n * d, MDE_BLOCK)), dim3(MDE_BLOCK), 0, st, n * d, d, Z, mean, scale);
    MDE_LAUNCH_CHECK();
    return MDE_OK;
  }
  if (DIR)
    hipLaunchKernelGGL(k_colsum<true>, dim3(nb), dim3(MDE_BLOCK), 0, st, n, d, dp, Z, X0, DIR, t, partial, mean,
                       fused_final ? work_ticket(work, TK_CENTER) : (unsigned int*)nullptr);
  else
    hipLaunchKernelGGL(k_colsum<false>, dim3(nb), dim3(MDE_BLOCK), 0, st, n, d, dp, Z, X0, DIR, t, partial, mean,
                       fused_final ? work_ticket(work, TK_CENTER) : (unsigned int*)nullptr);
  MDE_LAUNCH_CHECK();
  if (!fused_final) {
    hipLaunchKernelGGL(k_colsum_final, dim3(d), dim3(64), 0, st, nb, d, n, partial, mean);
    MDE_LAUNCH_CHECK();
  }
  if (!(halves & 2)) return MDE_OK;
  hipLaunchKernelGGL(k_sub_mean, dim3(mde_grid(n * d, MDE_BLOCK)), dim3(MDE_BLOCK), 0, st, n * d, d, Z,
                     mean, scale);
  MDE_LAUNCH_CHECK();
  return MDE_OK;
}

// The two halves of mde_center_step for a row-sharded solve (round 6): _begin forms this rank's rows of Z = X + t dir
// (dir == NULL: Z as it is) and leaves the column MEANS over these n rows in work[0 .. d); the caller sums them across
// the ranks in place; _end subtracts scale x work[0 .. d) (scale = this rank's share of the rows, n / n_total).
extern "C" int mde_center_step_begin(int64_t n, int32_t d, const float* X, const float* dir, float t, float* Z, double* work,
                                     void* stream) {
  if (n <= 0 || d <= 0 || d > 2048 || !Z || !work || (dir && !X)) return MDE_E_INVALID;
  return mde_center_impl(n, d, Z, work, mde_stream(stream), dir ? X : nullptr, dir, t, 1);
}
extern "C" int mde_center_step_end(int64_t n, int32_t d, float* Z, double* work, double scale, void* stream) {
  if (n <= 0 || d <= 0 || d > 2048 || !Z || !work) return MDE_E_INVALID;
  return mde_center_impl(n, d, Z, work, mde_stream(stream), nullptr, nullptr, 0.0f, 2, scale);
}

extern "C" int mde_center(int64_t n, int32_t d, float* Z, double* work, void* stream) {
  if (n <= 0 || d <= 0 || d > 2048 || !Z || !work) return MDE_E_INVALID;
  return mde_center_impl(n, d, Z, work, mde_stream(stream));
}

// Z <- centre(X + t DIR): the trial point of the line search under the Centered constraint
extern "C" int mde_center_step(int64_t n, int32_t d, const float* X, const float* dir, float t, float* Z,
                               double* work, void* stream) {
  if (n <= 0 || d <= 0 || d > 2048 || !X || !dir || !Z || !work) return MDE_E_INVALID;
  return mde_center_impl(n, d, Z, work, mde_stream(stream), X, dir, t);
}

// ---------------------------------------------------------------- anchors
__global__ void k_anchor_rows(int64_t na, int d, const int64_t* __restrict__ anchors,
                              const float* __restrict__ values, float* __restrict__ Z) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < na * d;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t a = i / d;
    const int c = (int)(i % d);
    Z[anchors[a] * d + c] = values ? values[i] : 0.0f;
  }
}
extern "C" int mde_anchor_rows(int64_t n_anchors, int32_t d, const int64_t* anchors,
                               const float* values, float* Z, void* stream) {
  if (n_anchors < 0 || d <= 0 || (n_anchors > 0 && (!anchors || !Z))) return MDE_E_INVALID;
  if (n_anchors == 0) return MDE_OK;
  hipLaunchKernelGGL(k_anchor_rows, dim3(mde_grid(n_anchors * d, MDE_BLOCK)), dim3(MDE_BLOCK), 0,
                     mde_stream(stream), n_anchors, d, anchors, values, Z);
  MDE_LAUNCH_CHECK();
  return MDE_OK;
}

// ---------------------------------------------------------------- rows on a sphere
// [ref: constraints.py:203-231, `_Sphere`: private there, used by no recipe]  X == NULL: the retraction
// Z[r] <- (Z[r] / |Z[r]|) radius (divide, then multiply, as the reference does); else the tangent projection
// Z[r] -= (1 / radius) (Z[r] . X[r]) X[r] -- the reference's own scale, 1 / radius and not 1 / radius^2.
// Narrow rows: one thread per row; wide rows: one wave per row, lanes strided over the columns.
template <bool TANGENT>
__global__ __launch_bounds__(MDE_BLOCK) void k_sphere_narrow(int64_t n, int d, const float* __restrict__ X,
                                                             float* __restrict__ Z, float radius) {
  for (int64_t r = (int64_t)blockIdx.x * MDE_BLOCK + threadIdx.x; r < n; r += (int64_t)gridDim.x * MDE_BLOCK) {
    float* z = Z + r * d;
    float s = 0.0f;
    if (TANGENT) {
      const float* x = X + r * d;
      for (int c = 0; c < d; ++c) s = fmaf(z[c], x[c], s);
      const float k = (1.0f / radius) * s;
      for (int c = 0; c < d; ++c) z[c] -= k * x[c];
    } else {
      for (int c = 0; c < d; ++c) s = fmaf(z[c], z[c], s);
      const float nrm = sqrtf(s);
      for (int c = 0; c < d; ++c) z[c] = (z[c] / nrm) * radius;
    }
  }
}
template <bool TANGENT>
__global__ __launch_bounds__(MDE_BLOCK) void k_sphere_wide(int64_t n, int d, const float* __restrict__ X,
                                                           float* __restrict__ Z, float radius) {
  const int lane = threadIdx.x & 63;
  const int64_t wpg = MDE_BLOCK / 64;
  for (int64_t r = (int64_t)blockIdx.x * wpg + (threadIdx.x >> 6); r < n; r += (int64_t)gridDim.x * wpg) {
    float* z = Z + r * d;
    const float* x = TANGENT ? X + r * d : z;
    double s = 0.0;
    for (int c = lane; c < d; c += 64) s += (double)z[c] * (double)x[c];
    s = mde_wave_sum(s);  // (a butterfly: every lane holds the sum)
    if (TANGENT) {
      const float k = (1.0f / radius) * (float)s;
      for (int c = lane; c < d; c += 64) z[c] -= k * x[c];
    } else {
      const float nrm = sqrtf((float)s);
      for (int c = lane; c < d; c += 64) z[c] = (z[c] / nrm) * radius;
    }
  }
}
extern "C" int mde_sphere_rows(int64_t n, int32_t d, const float* X, float* Z, float radius, void* stream) {
  if (n <= 0 || d <= 0 || !Z || !(radius > 0.0f)) return MDE_E_INVALID;
  hipStream_t st = mde_stream(stream);
  if (d <= 32) {
    const int nb = mde_grid(n, MDE_BLOCK);
    if (X)
      hipLaunchKernelGGL(k_sphere_narrow<true>, dim3(nb), dim3(MDE_BLOCK), 0, st, n, d, X, Z, radius);
    else
      hipLaunchKernelGGL(k_sphere_narrow<false>, dim3(nb), dim3(MDE_BLOCK), 0, st, n, d, X, Z, radius);
  } else {
    const int nb = mde_grid(n, MDE_BLOCK / 64);
    if (X)
      hipLaunchKernelGGL(k_sphere_wide<true>, dim3(nb), dim3(MDE_BLOCK), 0, st, n, d, X, Z, radius);
    else
      hipLaunchKernelGGL(k_sphere_wide<false>, dim3(nb), dim3(MDE_BLOCK), 0, st, n, d, X, Z, radius);
  }
  MDE_LAUNCH_CHECK();
  return MDE_OK;
}

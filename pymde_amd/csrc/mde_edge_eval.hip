// mde_edge_eval.hip -- the edge-order evaluators behind MDE.differences / distances / distortions
// [ref: pymde/problem.py:246-308, average_distortion.py:38-55].
#include "mde_fused.h"

// GL lanes per edge, components strided over the lanes.
template <int GL, bool WRITE_DIFF>
__global__ __launch_bounds__(MDE_BLOCK) void k_edge_order(int64_t p, int d,
                                                          const int64_t* __restrict__ edges,
                                                          const float* __restrict__ X,
                                                          float* __restrict__ out) {
  const int lig = threadIdx.x & (GL - 1);
  const int64_t g0 = ((int64_t)blockIdx.x * MDE_BLOCK + threadIdx.x) / GL;
  const int64_t ng = ((int64_t)gridDim.x * MDE_BLOCK) / GL;
  for (int64_t k = g0; k < p; k += ng) {
    const longlong2 e = reinterpret_cast<const longlong2*>(edges)[k];
    float ss = 0.0f;
    for (int c = lig; c < d; c += GL) {
      const float df = X[e.x * d + c] - X[e.y * d + c];
      if constexpr (WRITE_DIFF) out[k * d + c] = df;
      ss = fmaf(df, df, ss);
    }
    if constexpr (!WRITE_DIFF) {
      ss = mde_group_sum<GL>(ss);
      // sqrt(sum of squares): correctly rounded sqrt, as torch's pow(2).sum().sqrt()
      if (lig == 0) out[k] = sqrtf(ss);
    }
  }
}

template <bool WRITE_DIFF>
static int launch_edge_order(int64_t n, int64_t p, const int64_t* edges, const float* X, int d,
                             float* out, hipStream_t st) {
  if (n <= 0 || p < 0 || d <= 0 || (p > 0 && (!edges || !X || !out))) return MDE_E_INVALID;
  if (p == 0) return MDE_OK;
#define EO(GLV)                                                                                   \
  hipLaunchKernelGGL((k_edge_order<GLV, WRITE_DIFF>), dim3(mde_grid(p * GLV, MDE_BLOCK, 4096)),   \
                     dim3(MDE_BLOCK), 0, st, p, d, edges, X, out)
  if (d <= 4)
    EO(1);
  else if (d <= 16)
    EO(4);
  else if (d <= 64)
    EO(16);
  else
    EO(64);
#undef EO
  MDE_LAUNCH_CHECK();
  return MDE_OK;
}

extern "C" int mde_differences(int64_t n, int64_t p, const int64_t* edges, const float* X, int32_t d,
                               float* diff_out, void* stream) {
  return launch_edge_order<true>(n, p, edges, X, d, diff_out, mde_stream(stream));
}
extern "C" int mde_distances(int64_t n, int64_t p, const int64_t* edges, const float* X, int32_t d,
                             float* dist_out, void* stream) {
  return launch_edge_order<false>(n, p, edges, X, d, dist_out, mde_stream(stream));
}

__global__ __launch_bounds__(MDE_BLOCK) void k_distortions(int64_t p, const float* __restrict__ dist,
                                                           const float* __restrict__ a0,
                                                           const float* __restrict__ a1, int a0_scalar,
                                                           int a1_scalar, FnRuntime fn,
                                                           float* __restrict__ out,
                                                           float* __restrict__ dout) {
  const EdgeParams<false> params(nullptr, a0, a1, a0_scalar, a1_scalar);
  for (int64_t k = (int64_t)blockIdx.x * MDE_BLOCK + threadIdx.x; k < p;
       k += (int64_t)gridDim.x * MDE_BLOCK) {
    const float dk = dist[k];
    float p0, p1;
    params.load(k, p0, p1);
    float f, gd;
    fn.eval(dk * dk, p0, p1, f, gd);
    out[k] = f;
    if (dout) dout[k] = gd * dk;  // f'(d) = (f'(d)/d) d
  }
}

extern "C" int mde_distortions(int64_t p, const float* dist, const mde_func* f, float* out,
                               float* dout, void* stream) {
  if (p < 0 || (p > 0 && (!dist || !out))) return MDE_E_INVALID;
  int rc = mde_check_func(f);
  if (rc != MDE_OK) return rc;
  if (p == 0) return MDE_OK;
  FnRuntime fn{func_args(f)};
  hipLaunchKernelGGL(k_distortions, dim3(mde_grid(p, MDE_BLOCK, 4096)), dim3(MDE_BLOCK), 0,
                     mde_stream(stream), p, dist, f->a0, f->a1, f->a0_scalar, f->a1_scalar, fn, out, dout);
  MDE_LAUNCH_CHECK();
  return MDE_OK;
}

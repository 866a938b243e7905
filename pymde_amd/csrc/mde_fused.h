// mde_fused.h -- what the fused CSR kernels share: the per-half-edge parameter loader, row loads and
// stores for d <= 4, the functors of the two unfused paths, the launch arguments
// and the entry points of the units (mde_distortion.hip picks one of them per call).
#pragma once
#include "mde_common.h"
#include "mde_functions.h"
#include "mde_plan.h"

// ---------------------------------------------------------------- device pieces
// The parameters (a0, a1) of half-edge position h: one value for every edge (scalar), one per
// position, or -- INDIRECT, the unfused paths -- one per edge, found through eid[h].
template <bool INDIRECT>
struct EdgeParams {
  const int32_t* eid;
  const float *a0, *a1;
  int a0_scalar, a1_scalar;
  float a0s, a1s;
  MDE_DEV EdgeParams(const int32_t* eid_, const float* a0_, const float* a1_, int a0_scalar_, int a1_scalar_)
      : eid(eid_), a0(a0_), a1(a1_), a0_scalar(a0_scalar_), a1_scalar(a1_scalar_),
        a0s(a0_scalar_ ? a0_[0] : 0.0f), a1s((a1_ && a1_scalar_) ? a1_[0] : 0.0f) {}
  template <class Index>
  MDE_DEV void load(Index h, float& p0, float& p1) const {
    p1 = a1s;
    if constexpr (INDIRECT) {
      const int k = eid[h];
      p0 = a0[k];
      p1 = a1[k];
    } else {
      p0 = a0_scalar ? a0s : a0[h];
      if (a1 && !a1_scalar) p1 = a1[h];
    }
  }
};

// rows of D <= 4 floats: one 8- / 16-byte access at D = 2 / 4
template <int D>
struct VecD {
  float v[D];
};
template <int D>
MDE_DEV VecD<D> load_row(const float* __restrict__ X, int64_t r) {
  VecD<D> o;
  if constexpr (D == 2) {
    const float2 t = reinterpret_cast<const float2*>(X)[r];
    o.v[0] = t.x;
    o.v[1] = t.y;
  } else if constexpr (D == 4) {
    const float4 t = reinterpret_cast<const float4*>(X)[r];
    o.v[0] = t.x;
    o.v[1] = t.y;
    o.v[2] = t.z;
    o.v[3] = t.w;
  } else {
#pragma unroll
    for (int c = 0; c < D; ++c) o.v[c] = X[r * D + c];
  }
  return o;
}
template <int D>
MDE_DEV void store_row(float* __restrict__ grad, int64_t v, const float (&acc)[D], float scale) {
  if constexpr (D == 2) {
    reinterpret_cast<float2*>(grad)[v] = make_float2(acc[0] * scale, acc[1] * scale);
  } else if constexpr (D == 4) {
    reinterpret_cast<float4*>(grad)[v] =
        make_float4(acc[0] * scale, acc[1] * scale, acc[2] * scale, acc[3] * scale);
  } else {
#pragma unroll
    for (int c = 0; c < D; ++c) grad[v * D + c] = acc[c] * scale;
  }
}

// functors of the unfused paths (parameters through eid: INDIRECT)
struct FnScatter {  // a0 = d(mean f)/d(dist) from autograd, a1 = dist  (average_distortion.py:81)
  MDE_DEV void eval(float ss, float a0, float a1, float& f, float& gd) const {
    f = 0.0f;
    gd = a0 / a1;
  }
};
struct FnDistBackward {  // backward of the 2-norm, average_distortion.py:46-52
  MDE_DEV void eval(float ss, float a0, float a1, float& f, float& gd) const {
    f = 0.0f;
    gd = a0 * mde_rcp(mde_sqrt(ss));
  }
};
enum mde_unfused { MDE_UNFUSED_SCATTER, MDE_UNFUSED_DIST_BACKWARD };

// ---------------------------------------------------------------- host pieces
double* mde_plan_partials(mde_plan* p);  // mde_plan.hip

struct FusedArgs {
  const mde_plan* plan;
  const float* X;
  int d;
  const float *a0, *a1;
  int a0_scalar, a1_scalar;
  float* grad;
  double* partials;
  float inv_p, grad_scale;
  hipStream_t st;
  int nblocks = 0;  // out
  // in: where the loss goes (a kernel that has a follow-up launch anyway reduces it there and sets
  // loss_done; otherwise mde_average_distortion launches k_finalize_loss)
  float* loss_out = nullptr;
  double loss_scale = 0.0;
  int loss_done = 0;
  FusedArgs(const mde_plan* plan_, const float* X_, int d_, const float* a0_, const float* a1_, int a0_scalar_,
            int a1_scalar_, float* grad_, float inv_p_, float grad_scale_, void* stream)
      : plan(plan_), X(X_), d(d_), a0(a0_), a1(a1_), a0_scalar(a0_scalar_), a1_scalar(a1_scalar_), grad(grad_),
        partials(mde_plan_partials(const_cast<mde_plan*>(plan_))), inv_p(inv_p_), grad_scale(grad_scale_),
        st(mde_stream(stream)) {}
};

// grid of a kernel in which `lanes` lanes own one row at a time: sets A.nblocks, returns the rows
static inline int fused_row_grid(FusedArgs& A, int lanes) {
  const int nrows = (int)(mde_plan_row_hi(A.plan) - mde_plan_row_lo(A.plan));
  A.nblocks = mde_grid((int64_t)nrows * lanes, MDE_BLOCK, 2048);
  return nrows;
}

// the one compile-time functor of the general-d kernels: Log1p(1.5), the recipes' default attractive
// penalty (config 5, d = 128: the run-time functor's switch and general pow cost 0.5 ms of the 3.7 ms
// launch)
static inline bool func_is_log1p15(const mde_func* f) {
  return f->kind_neg == MDE_F_NONE && f->kind == MDE_F_LOG1P && mde_exp_class(f->s0) == 2;
}

// The units.  Each picks its own functor instantiation: for a distortion function `f` (dedicated
// instantiations for what the recipes use by default, the run-time functor otherwise) or for one of
// the two unfused paths.
MDE_INTERNAL int mde_fused_small(FusedArgs& A, const mde_func* f);          // d = 1 .. 4  (mde_fused_small.hip)
MDE_INTERNAL int mde_fused_small_unfused(FusedArgs& A, mde_unfused which);
MDE_INTERNAL int mde_fused_wide(FusedArgs& A, const mde_func* f);           // d = 5 .. 2048, unpipelined (mde_fused_wide.hip)
MDE_INTERNAL int mde_fused_wide_unfused(FusedArgs& A, mde_unfused which);
MDE_INTERNAL int mde_check_func(const mde_func* f);                         // mde_distortion.hip

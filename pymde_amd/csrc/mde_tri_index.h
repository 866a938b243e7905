// mde_tri_index.h -- the triangular bijection of the edge sampler: pair index in [0, C(n,2)) -> edge (u < v) in the
// (i, j) order [ref: pymde/preprocess/preprocess.py:64-69].  No HIP include: k_sample_keys (mde_edges.hip) calls it on
// the device, tests/host/tri_index_test.cpp compiles it with any C++17 compiler and checks it against 128-bit integers.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define MDE_TRI_HD __host__ __device__ __forceinline__
#else
#define MDE_TRI_HD inline
#endif

// index of the pair (u, u + 1): the number of pairs whose first item is below u.  n < 2^31: every product fits
MDE_TRI_HD uint64_t mde_tri_row_offset(int64_t n, int64_t u) {
  return (uint64_t)u * (uint64_t)n - (uint64_t)u * (uint64_t)(u + 1) / 2;
}

// (u, v) of pair `idx` < n (n - 1) / 2, 2 <= n < 2^31: u is the largest row with off(u) <= idx,
//   u = n - 2 - floor(sqrt(4 n (n-1) - 8 idx - 7) / 2 - 1/2),   v = idx - off(u) + u + 1.
// The discriminant is formed in 64-bit integers, where it is exact and at least 1 (4 n (n-1) < 2^64, idx <= C(n,2) - 1);
// formed in doubles it cancels to a negative number next to the last pair once 4 n (n-1) passes 2^53, and the
// square root of that is a NaN whose conversion to an integer is undefined.  The double square root is a first guess
// that the two loops correct in integers; they take a step or two at most (rounding the exact discriminant to 53 bits
// moves its root by less than 2^-21) and their count is returned so that the host test can bound it.
MDE_TRI_HD int mde_tri_index(int64_t n, uint64_t idx, int64_t* u_out, int64_t* v_out) {
  const uint64_t disc = 4 * (uint64_t)n * (uint64_t)(n - 1) - 8 * idx - 7;
  int64_t u = n - 2 - (int64_t)floor(sqrt((double)disc) / 2.0 - 0.5);
  if (u < 0) u = 0;
  if (u > n - 2) u = n - 2;
  int steps = 0;
  while (u > 0 && mde_tri_row_offset(n, u) > idx) --u, ++steps;
  while (u < n - 2 && mde_tri_row_offset(n, u + 1) <= idx) ++u, ++steps;
  *u_out = u;
  *v_out = (int64_t)(idx - mde_tri_row_offset(n, u)) + u + 1;
  return steps;
}

// mde_rng.h -- the counter-based generator of the sampling kernels: one SplitMix64 stream per draw.
// Draw t of a seed is mde_splitmix64(seed ^ mde_splitmix64(t)): no state, so every draw can be formed by whichever
// thread needs it, and a host replay in 64-bit integers gives the same bits.
#pragma once
#include <stdint.h>

#include <hip/hip_runtime.h>

__host__ __device__ __forceinline__ uint64_t mde_splitmix64(uint64_t x) {
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}

// draw t of `seed` as a double in [0, 1): the top 53 bits
__host__ __device__ __forceinline__ double mde_uniform01(uint64_t seed, uint64_t t) {
  return (double)(mde_splitmix64(seed ^ mde_splitmix64(t)) >> 11) * (1.0 / 9007199254740992.0);
}

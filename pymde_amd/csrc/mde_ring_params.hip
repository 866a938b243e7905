// mde_ring_params.hip -- per-edge parameter arrays in the order of the LDS-ring layout (layout 1): the plain fp32
// stream, the 8-value codebook in the packed words' low bits (and its two-value form, the pair codebook) and the
// 255-value byte index.  A unit of its own: these kernels run when a function is bound to a plan, after the layout
// build and apart from it.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "mde_ring.h"

__global__ __launch_bounds__(MDE_BLOCK) void k_expand_ring(int64_t H, const int32_t* __restrict__ eid,
                                                           const float* __restrict__ in,
                                                           float* __restrict__ out) {
  for (int64_t q = (int64_t)blockIdx.x * MDE_BLOCK + threadIdx.x; q < H;
       q += (int64_t)gridDim.x * MDE_BLOCK)
    out[q] = eid[q] >= 0 ? in[eid[q]] : 0.0f;  // padding entries: weight 0 (f = 0 for every penalty)
}

extern "C" int mde_plan_expand_layout(const mde_plan* plan, int32_t layout, const float* in_edge,
                                      float* out_half, void* stream) {
  if (!plan || !in_edge || !out_half) return MDE_E_INVALID;
  if (layout == 0) return mde_plan_expand(plan, in_edge, out_half, stream);
  if (layout != 1 || !plan->ring.eid) {
    mde_set_error("mde_plan_expand_layout: the LDS-ring layout has not been built");
    return MDE_E_INVALID;
  }
  if (plan->ring.H == 0) return MDE_OK;
  hipLaunchKernelGGL(k_expand_ring, dim3(mde_grid(plan->ring.H, MDE_BLOCK, 4096)), dim3(MDE_BLOCK), 0,
                     mde_stream(stream), plan->ring.H, plan->ring.eid, in_edge, out_half);
  MDE_LAUNCH_CHECK();
  return MDE_OK;
}

// ---------------------------------------------------------------- parameter codebooks
// Neighbour-graph problems carry very few distinct per-edge parameters (k-NN weights 1 / 2, -1 for
// repulsive pairs).  At d = 2 the packed word's ring offset is a multiple of 8, so its 3 low bits
// can hold an index into a table of 8 values: the kernel then streams 4 bytes per half-edge
// instead of 8 (packed word + fp32 parameter) and looks the parameter up in LDS.  Entry 0 is the
// weight 0 of padding lanes, entries 1..7 the (at most 7) distinct values of the array.
#define MDE_CB_EMPTY 0xFFFFFFFFu  // (a NaN pattern: NaN parameters simply disable the codebook)

// distinct bit patterns of in[0..p): inserted into table[1..8) with compare-and-swap; *overflow is
// set when an 8th value (or the EMPTY pattern) shows up.  A value goes through the workgroup's own
// table first (LDS compare-and-swap) and only the thread that put it THERE carries it to the global
// one: <= 8 global atomics per workgroup.  (Round 4 until then: every thread met an empty table at
// its first element and went to the global one -- half a million compare-and-swaps on one address,
// 9.4 ms for a scan that reads 200 MB.)
__global__ __launch_bounds__(MDE_BLOCK) void k_codebook_scan(int64_t p, const float* __restrict__ in,
                                                             unsigned int* __restrict__ table,
                                                             int* __restrict__ overflow) {
  __shared__ unsigned int stb[MDE_RING_CB_VALUES];
  if (threadIdx.x < MDE_RING_CB_VALUES) stb[threadIdx.x] = MDE_CB_EMPTY;
  __syncthreads();
  unsigned int last0 = MDE_CB_EMPTY, last1 = MDE_CB_EMPTY;
  const int64_t stride = (int64_t)gridDim.x * MDE_BLOCK;
  constexpr int U = 4;  // independent loads in flight per thread
  for (int64_t i0 = (int64_t)blockIdx.x * MDE_BLOCK + threadIdx.x; i0 < p; i0 += U * stride) {
    unsigned int vv[U];
    bool in_range[U];
#pragma unroll
    for (int k = 0; k < U; ++k) {
      const int64_t i = i0 + k * stride;
      in_range[k] = i < p;
      vv[k] = in_range[k] ? __float_as_uint(in[i]) : 0u;
    }
#pragma unroll
    for (int k = 0; k < U; ++k) {
      const unsigned int v = vv[k];
      if (!in_range[k]) continue;
      if (v == MDE_CB_EMPTY) {  // (the pattern that marks a free slot: a NaN, no codebook)
        *overflow = 1;
        return;
      }
      if (v == last0 || v == last1) continue;
      last1 = last0;
      last0 = v;
      bool placed = false, mine = false;
      for (int s = 0; s < MDE_RING_CB_VALUES && !placed; ++s) {
        const unsigned int old = atomicCAS(&stb[s], MDE_CB_EMPTY, v);
        mine = (old == MDE_CB_EMPTY);
        placed = mine || old == v;
      }
      if (placed && !mine) continue;  // some thread of this workgroup has carried it already
      placed = false;
      for (int s = 1; s < MDE_RING_CB_VALUES && !placed; ++s) {
        unsigned int cur = __hip_atomic_load(&table[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (cur == MDE_CB_EMPTY) cur = atomicCAS(&table[s], MDE_CB_EMPTY, v);
        placed = (cur == MDE_CB_EMPTY || cur == v);
      }
      if (!placed) {
        *overflow = 1;
        return;
      }
    }
  }
}

// out[q] = packed[q] | index of in[eid[q]] in table (padding entries keep index 0)
// PAIR (the pair codebook, at most two values): table[0..1] are the values and the index is ONE bit, so a padding
// entry selects table[0] -- a real weight.  What keeps it silent is its distance: its column field is pointed at its
// own row, a dummy row in the x_v region (resident from the prologue on, zero, never written), so x_v - x_u = 0
// exactly and a function with kZeroAtZero adds nothing.
template <bool PAIR>
__global__ __launch_bounds__(MDE_BLOCK) void k_codebook_pack(int64_t H, int d, const uint32_t* __restrict__ packed,
                                                             const int32_t* __restrict__ eid,
                                                             const float* __restrict__ in,
                                                             const unsigned int* __restrict__ table,
                                                             uint32_t* __restrict__ out) {
  unsigned int tb[MDE_RING_CB_VALUES];
#pragma unroll
  for (int s = 0; s < MDE_RING_CB_VALUES; ++s) tb[s] = table[s];
  for (int64_t q = (int64_t)blockIdx.x * MDE_BLOCK + threadIdx.x; q < H;
       q += (int64_t)gridDim.x * MDE_BLOCK) {
    uint32_t w = packed[q];
    if (eid[q] >= 0) {
      const unsigned int v = __float_as_uint(in[eid[q]]);
      uint32_t idx = 0;
      if (PAIR) {
        idx = (tb[1] == v) ? 1u : 0u;  // (one value: both entries hold it, either index will do)
      } else {
#pragma unroll
        for (int s = 1; s < MDE_RING_CB_VALUES; ++s) idx = (tb[s] == v) ? (uint32_t)s : idx;
      }
      w |= idx;  // (padding entries keep index 0 = weight 0)
    } else if (PAIR) {
      // (ring_pack_word: the row address in the low half, the column address / 8 or / 4 from bit 16; d = 2 keeps
      // its loss flag in bit 31)
      w = d == 2 ? ((w & 0x8000ffffu) | (((w & 0xfff8u) >> 3) << 16)) : ((w & 0xffffu) | (((w & 0xfffcu) >> 2) << 16));
    }
    out[q] = w;
  }
}

// Try to put a per-edge parameter array into codebook form for layout 1.  On success
// (*n_values_host in 1..7 at d = 2, 1..3 at d = 3) out_half holds the H packed words with the value index
// in their low bits, followed by the 8-entry value table; pass it as mde_func.a0 with a0_scalar = *form_host:
// 2, or 4 -- the pair codebook -- when `f` is given, the array has one or two values and every entry of f whose two
// ends coincide adds zero (mde_zero_at_zero; MDE_CODEBOOK_PAIR=0: never).
// *n_values_host = 0: not applicable (another d, too many distinct values, NaNs) -- nothing is
// written and the caller uses mde_plan_expand_layout.  SYNC.
static int expand_codebook(const mde_plan* plan, const mde_func* f, const float* in_edge, float* out_half,
                           int32_t* n_values_host, int32_t* form_host, void* stream) {
  if (!plan || !in_edge || !out_half || !n_values_host || !form_host) return MDE_E_INVALID;
  *n_values_host = 0;
  *form_host = 0;
  const mde_ring_layout& L = plan->ring;
  // (the index rides in the bits the row address leaves free: 3 at d = 2 -- up to 7 values --, 2 at d = 3 --
  // up to 3, enough for a neighbour graph's {1, 2, -1})
  if (!L.packed || (L.d != 2 && L.d != 3) || L.H == 0 || plan->p == 0) return MDE_OK;
  const int max_values = L.d == 2 ? 7 : 3;
  if (env_int("MDE_CODEBOOK", 1) == 0) return MDE_OK;
  hipStream_t st = mde_stream(stream);
  unsigned int* table = reinterpret_cast<unsigned int*>(out_half) + L.H;  // the spare entries
  // (the overflow flag lives in the plan's reduction scratch: no allocation per call)
  int* overflow = reinterpret_cast<int*>(plan->partials + MDE_MAX_PARTIALS + 1);
  hipError_t err = hipMemsetAsync(overflow, 0, sizeof(int), st);
  if (err == hipSuccess) err = hipMemsetAsync(table, 0xFF, MDE_RING_CB_VALUES * sizeof(unsigned int), st);
  unsigned int host_tb[MDE_RING_CB_VALUES];
  int host_overflow = 0;
  if (err == hipSuccess) {
    hipLaunchKernelGGL(k_codebook_scan, dim3(mde_grid(plan->p, MDE_BLOCK, 2048)), dim3(MDE_BLOCK), 0, st, plan->p,
                       in_edge, table, overflow);
    err = hipGetLastError();
  }
  if (err == hipSuccess) err = hipMemcpyAsync(host_tb, table, sizeof(host_tb), hipMemcpyDeviceToHost, st);
  if (err == hipSuccess) err = hipMemcpyAsync(&host_overflow, overflow, sizeof(int), hipMemcpyDeviceToHost, st);
  if (err == hipSuccess) err = hipStreamSynchronize(st);
  if (err != hipSuccess) return mde_hip_fail(err, "parameter codebook scan", __FILE__, __LINE__);
  if (host_overflow) return MDE_OK;
  // canonical order (the insertion order above depends on scheduling): ascending bit patterns
  int nv = 0;
  unsigned int vals[MDE_RING_CB_VALUES];
  vals[0] = 0u;  // +0.0f: the padding lanes' weight
  for (int s = 1; s < MDE_RING_CB_VALUES; ++s)
    if (host_tb[s] != MDE_CB_EMPTY) vals[1 + nv++] = host_tb[s];
  if (nv == 0 || nv > max_values) return MDE_OK;
  // (finite values of ordinary size only: the kernel skips the NaN/Inf fix-up of f'/d for codebook
  // streams -- the functors that keep f'/d finite at d = 0 do so with a reciprocal of up to 1e30, which a
  // weight beyond 2e8 would carry to Inf (times x_v - x_u = 0: NaN where the reference has 0); weights
  // beyond 1e6 stream as fp32 next to the packed word instead, with the fix-up)
  for (int s = 1; s <= nv; ++s) {
    float fv;
    memcpy(&fv, &vals[s], sizeof(float));
    if (!std::isfinite(fv) || std::fabs(fv) > 1.0e6f) return MDE_OK;
  }
  for (int a = 2; a <= nv; ++a)
    for (int b = a; b > 1 && vals[b - 1] > vals[b]; --b) {
      const unsigned int t = vals[b];
      vals[b] = vals[b - 1];
      vals[b - 1] = t;
    }
  for (int s = nv + 1; s < MDE_RING_CB_VALUES; ++s) vals[s] = MDE_CB_EMPTY;
  const bool pair = f && nv <= 2 && env_int("MDE_CODEBOOK_PAIR", 1) != 0 &&
                    mde_zero_at_zero(f->kind, f->kind_neg, mde_exp_class(f->s0));
  if (pair) {
    // the table of the pair form: the two values a lane can select, both finite (one value: twice)
    vals[0] = vals[1];
    vals[1] = nv == 2 ? vals[2] : vals[1];
    vals[2] = MDE_CB_EMPTY;
  }
  err = hipMemcpyAsync(table, vals, sizeof(vals), hipMemcpyHostToDevice, st);
  if (err == hipSuccess) {
    hipLaunchKernelGGL(pair ? k_codebook_pack<true> : k_codebook_pack<false>, dim3(mde_grid(L.H, MDE_BLOCK, 4096)), dim3(MDE_BLOCK),
                       0, st, L.H, L.d, L.packed, L.eid, in_edge, table, reinterpret_cast<uint32_t*>(out_half));
    err = hipGetLastError();
  }
  const hipError_t esync = hipStreamSynchronize(st);  // `vals` is a stack buffer: wait whatever the launch said
  if (err == hipSuccess) err = esync;
  if (err != hipSuccess) return mde_hip_fail(err, "parameter codebook pack", __FILE__, __LINE__);
  *n_values_host = nv;
  *form_host = pair ? 4 : 2;
  return MDE_OK;
}
extern "C" int mde_plan_expand_codebook(const mde_plan* plan, const float* in_edge, float* out_half,
                                        int32_t* n_values_host, void* stream) {
  int32_t form = 0;
  return expand_codebook(plan, nullptr, in_edge, out_half, n_values_host, &form, stream);
}
extern "C" int mde_plan_expand_codebook_for(const mde_plan* plan, const mde_func* f, const float* in_edge, float* out_half,
                                            int32_t* n_values_host, int32_t* form_host, void* stream) {
  if (!f) return MDE_E_INVALID;
  return expand_codebook(plan, f, in_edge, out_half, n_values_host, form_host, stream);
}

// ---------------------------------------------------------------- byte-index parameter streams
// Up to 255 distinct per-edge parameters (the hop counts of a distance-preserving problem on a graph are tens of
// distinct integers; quantised similarity weights): one index BYTE per entry beside the packed words -- 5 B per
// half-edge instead of 8 -- and a 256-entry value table that the kernel keeps in the 1 KB behind its chunk ring.
// The distinct bit patterns are collected in a hash table (per workgroup in LDS first, the winners carried to the
// global one), the host sorts them (canonical order: ascending bit patterns, entry 0 = the padding lanes' +0.0),
// and k_bytes_pack looks every entry's value up by bisection.
#define MDE_BX_SLOTS 1024  // hash slots (a power of two, >= 4 x the values a table holds)
__device__ __forceinline__ uint32_t bx_hash(uint32_t v) {
  v ^= v >> 16;
  v *= 0x7feb352du;
  v ^= v >> 15;
  v *= 0x846ca68bu;
  v ^= v >> 16;
  return v & (MDE_BX_SLOTS - 1);
}
// insert v into an open-addressing table; returns 1 when v was not there before, 0 when it was, -1 when the table is full
__device__ __forceinline__ int bx_insert(unsigned int* tb, uint32_t v) {
  uint32_t h = bx_hash(v);
  for (int probe = 0; probe < MDE_BX_SLOTS; ++probe) {
    const unsigned int old = atomicCAS(&tb[h], MDE_CB_EMPTY, v);
    if (old == MDE_CB_EMPTY) return 1;
    if (old == v) return 0;
    h = (h + 1) & (MDE_BX_SLOTS - 1);
  }
  return -1;
}
// state[0] = number of distinct values in the global table, state[1] = overflow flag
__global__ __launch_bounds__(MDE_BLOCK) void k_bytes_scan(int64_t p, const float* __restrict__ in,
                                                          unsigned int* __restrict__ table, int* __restrict__ state) {
  __shared__ unsigned int stb[MDE_BX_SLOTS];
  __shared__ int s_count;
  for (int i = threadIdx.x; i < MDE_BX_SLOTS; i += MDE_BLOCK) stb[i] = MDE_CB_EMPTY;
  if (threadIdx.x == 0) s_count = 0;
  __syncthreads();
  unsigned int last0 = MDE_CB_EMPTY, last1 = MDE_CB_EMPTY;
  const int64_t stride = (int64_t)gridDim.x * MDE_BLOCK;
  for (int64_t i = (int64_t)blockIdx.x * MDE_BLOCK + threadIdx.x; i < p; i += stride) {
    // (continuous weights: some workgroup sees its 256th value within its first few elements -- everybody leaves)
    if (__hip_atomic_load(&state[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return;
    const unsigned int v = __float_as_uint(in[i]);
    if (v == last0 || v == last1) continue;
    last1 = last0;
    last0 = v;
    if (v == MDE_CB_EMPTY) {  // (the pattern that marks a free slot: a NaN, no table)
      state[1] = 1;
      return;
    }
    const int fresh = bx_insert(stb, v);
    if (fresh == 0) continue;  // some thread of this workgroup has carried it already
    if (fresh < 0 || atomicAdd(&s_count, 1) >= MDE_RING_BX_VALUES - 1) {
      state[1] = 1;
      return;
    }
    const int g = bx_insert(table, v);
    if (g < 0 || (g == 1 && atomicAdd(&state[0], 1) >= MDE_RING_BX_VALUES - 1)) {
      state[1] = 1;
      return;
    }
  }
}

// out[q] = index of in[eid[q]] in the sorted table (entries 1..nv; padding entries keep index 0)
__global__ __launch_bounds__(MDE_BLOCK) void k_bytes_pack(int64_t H, const int32_t* __restrict__ eid,
                                                          const float* __restrict__ in,
                                                          const unsigned int* __restrict__ table, int nv,
                                                          uint8_t* __restrict__ out) {
  __shared__ unsigned int tb[MDE_RING_BX_VALUES];
  for (int i = threadIdx.x; i < MDE_RING_BX_VALUES; i += MDE_BLOCK) tb[i] = table[i];
  __syncthreads();
  for (int64_t q = (int64_t)blockIdx.x * MDE_BLOCK + threadIdx.x; q < H; q += (int64_t)gridDim.x * MDE_BLOCK) {
    uint32_t idx = 0;
    if (eid[q] >= 0) {
      const unsigned int v = __float_as_uint(in[eid[q]]);
      int lo = 1, hi = nv;  // tb[1..nv] ascending, v is one of them
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (tb[mid] < v) lo = mid + 1; else hi = mid;
      }
      idx = (uint32_t)lo;
    }
    out[q] = (uint8_t)idx;
  }
}

// Try to put a per-edge parameter array into byte-index form for layout 1 (d = 2, 3).  On success
// (*n_values_host in 1..255) out_half holds the H index bytes (in the order of the packed words: one 32-bit word
// per lane and block of four iterations) followed by the 256-entry value table; pass it as mde_func.a0 with
// a0_scalar = 3.  *n_values_host = 0: not applicable (another d, more distinct values, NaNs, values beyond 1e6,
// no room behind the ring) -- nothing usable is written and the caller streams fp32.  SYNC.
extern "C" int mde_plan_expand_bytes(const mde_plan* plan, const float* in_edge, float* out_half,
                                     int32_t* n_values_host, void* stream) {
  if (!plan || !in_edge || !out_half || !n_values_host) return MDE_E_INVALID;
  *n_values_host = 0;
  const mde_ring_layout& L = plan->ring;
  if (!L.packed || (L.d != 2 && L.d != 3) || L.H < 4 * MDE_RING_BX_VALUES || plan->p == 0) return MDE_OK;
  if (MDE_RING_LDS_BYTES - (L.ring_off + L.slots * ring_chunk_bytes(L.d)) < 4 * MDE_RING_BX_VALUES) return MDE_OK;
  if (env_int("MDE_BYTE_STREAM", 1) == 0) return MDE_OK;
  hipStream_t st = mde_stream(stream);
  MdeDeviceBuf<unsigned int> dtable;  // the hash table, then the two state words
  MDE_HIP(dtable.alloc(MDE_BX_SLOTS * sizeof(unsigned int) + 2 * sizeof(int)));
  int* dstate = reinterpret_cast<int*>(dtable.get() + MDE_BX_SLOTS);
  hipError_t err = hipMemsetAsync(dtable, 0xFF, MDE_BX_SLOTS * sizeof(unsigned int), st);
  if (err == hipSuccess) err = hipMemsetAsync(dstate, 0, 2 * sizeof(int), st);
  std::vector<unsigned int> host_tb(MDE_BX_SLOTS);
  int host_state[2] = {0, 0};
  if (err == hipSuccess) {
    hipLaunchKernelGGL(k_bytes_scan, dim3(mde_grid(plan->p, MDE_BLOCK, 2048)), dim3(MDE_BLOCK), 0, st, plan->p, in_edge, dtable,
                       dstate);
    err = hipGetLastError();
  }
  if (err == hipSuccess) err = hipMemcpyAsync(host_tb.data(), dtable, MDE_BX_SLOTS * sizeof(unsigned int), hipMemcpyDeviceToHost, st);
  if (err == hipSuccess) err = hipMemcpyAsync(host_state, dstate, sizeof(host_state), hipMemcpyDeviceToHost, st);
  if (err == hipSuccess) err = hipStreamSynchronize(st);
  if (err != hipSuccess) return mde_hip_fail(err, "byte-index stream: value scan", __FILE__, __LINE__);
  std::vector<unsigned int> vals;
  if (!host_state[1])
    for (unsigned int v : host_tb)
      if (v != MDE_CB_EMPTY) vals.push_back(v);
  bool ok = !host_state[1] && !vals.empty() && (int)vals.size() <= MDE_RING_BX_VALUES - 1;
  // (finite values of ordinary size only, as for the codebook: the kernel skips the NaN / Inf fix-up of f'/d)
  for (size_t i = 0; ok && i < vals.size(); ++i) {
    float fv;
    memcpy(&fv, &vals[i], sizeof(float));
    if (!std::isfinite(fv) || std::fabs(fv) > 1.0e6f) ok = false;
  }
  if (!ok) return MDE_OK;
  std::sort(vals.begin(), vals.end());
  const int nv = (int)vals.size();
  std::vector<unsigned int> tb(MDE_RING_BX_VALUES, 0u);  // entry 0 = +0.0f (padding lanes), unused entries 0 too
  for (int i = 0; i < nv; ++i) tb[1 + i] = vals[i];
  unsigned int* table = reinterpret_cast<unsigned int*>(out_half) + L.H / 4;  // behind the H index bytes
  err = hipMemcpyAsync(table, tb.data(), MDE_RING_BX_VALUES * sizeof(unsigned int), hipMemcpyHostToDevice, st);
  if (err == hipSuccess) {
    hipLaunchKernelGGL(k_bytes_pack, dim3(mde_grid(L.H, MDE_BLOCK, 4096)), dim3(MDE_BLOCK), 0, st, L.H, L.eid, in_edge, table, nv,
                       reinterpret_cast<uint8_t*>(out_half));
    err = hipGetLastError();
  }
  if (err == hipSuccess) err = hipStreamSynchronize(st);  // (`tb` is a host buffer)
  if (err != hipSuccess) return mde_hip_fail(err, "byte-index stream: pack", __FILE__, __LINE__);
  *n_values_host = nv;
  return MDE_OK;
}

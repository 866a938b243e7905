// mde_graph_components.hip -- the connected components of a graph.
//   [ref: the reference leaves components to scipy.sparse.csgraph.connected_components on the host]
// Hooking and pointer jumping on one parent array (the Shiloach-Vishkin family in its FastSV form): par[v] starts as
// v and only ever decreases.  Two invariants hold after every write, whatever the schedule:
//      par[v] <= v          and          par[v] lies in the component of v.
// A round is two launches:
//   hook   node u reads m = min over its neighbours v of par[v] and offers it to its own parent's slot and to its
//          own: atomicMin(par + par[u], m), atomicMin(par + u, m).  The first hooks the tree of u below a smaller
//          neighbouring tree, the second is FastSV's shortcut for u itself.
//   jump   par[u] <- par[... par[u]], CC_JUMPS steps up the tree (one writer per slot; a reader sees the old or the
//          new value, both ancestors).
// A round in which neither launch changed a slot is the fixed point: every tree is a star (the jump changed
// nothing), and the two ends of every edge have the same parent (the hook changed nothing), so a component has one
// root r with par[r] = r, and r <= every node of it: the smallest node.  The fixed point is unique, so the integer
// atomicMin decides nothing about the result.  How far a node's parent lies below it grows geometrically with the
// rounds (a hook reaches past a neighbour's parent, a jump past CC_JUMPS ancestors), so the rounds follow log n, not
// the hop diameter: a path of 20 000 nodes takes 11 rounds under a random renumbering, where min-label propagation
// takes thousands.  No kernel waits on another workgroup; the host reads one flag back per round and gives up after
// CC_MAX_ROUNDS.
// Rows of more than CC_HEAVY neighbours are left to a second hook launch, a wave per row (as the heavy nodes of
// mde_graph_sssp.hip): a thread per row would walk a hub's whole list alone.
// Labels: a root's label is the number of roots below it (an exclusive sum of the root flags), which is the rank of
// the component by its smallest node -- scipy's numbering.
#include "mde_common.h"
#include "mde_plan.h"

#define CC_HEAVY 64                  // largest degree the thread-per-node hook takes
#define CC_JUMPS 4                   // steps up the tree per jump launch
#define CC_MAX_ROUNDS 256            // far above 2 log2 n for n < 2^31; the host loop never spins

__global__ __launch_bounds__(MDE_BLOCK) void k_cc_init(int n, const int32_t* __restrict__ rowptr, int32_t* par,
                                                       int32_t* __restrict__ heavy, int* __restrict__ heavy_count) {
  const int u = blockIdx.x * MDE_BLOCK + threadIdx.x;
  if (u >= n) return;
  par[u] = u;
  if (rowptr[u + 1] - rowptr[u] > CC_HEAVY) heavy[atomicAdd(heavy_count, 1)] = u;
}

// counters: [0] changed in this round | [1] hook operations that lowered a slot, all rounds
__device__ __forceinline__ void cc_offer(int32_t* par, int u, int m, bool active, unsigned long long* hooks,
                                         int* changed) {
  bool lowered = false;
  if (active) {
    const int pu = par[u];
    if (m < pu) {
      // (pu <= u, so the second offer is needed only where u is not its own parent)
      lowered = atomicMin(par + pu, m) > m;
      if (pu != u) lowered |= atomicMin(par + u, m) > m;
    }
  }
  const unsigned long long won = __ballot(lowered);
  if (won && (threadIdx.x & 63) == __ffsll((long long)won) - 1) {
    atomicAdd(hooks, (unsigned long long)__popcll(won));
    *changed = 1;
  }
}

__global__ __launch_bounds__(MDE_BLOCK) void k_cc_hook(int n, const int32_t* __restrict__ rowptr,
                                                       const int32_t* __restrict__ nbr, int32_t* par,
                                                       unsigned long long* hooks, int* changed) {
  const int u = blockIdx.x * MDE_BLOCK + threadIdx.x;
  bool active = u < n;
  int m = 0x7fffffff;
  if (active) {
    const int h0 = rowptr[u], h1 = rowptr[u + 1];
    active = h1 - h0 <= CC_HEAVY && h1 > h0;
    if (active)
      for (int h = h0; h < h1; ++h) {
        const int pv = par[nbr[h]];
        m = pv < m ? pv : m;
      }
  }
  cc_offer(par, u, m, active, hooks, changed);
}

// a wave per node of heavy[]: the lanes split the neighbour list
__global__ __launch_bounds__(MDE_BLOCK) void k_cc_hook_heavy(int n_heavy, const int32_t* __restrict__ heavy,
                                                             const int32_t* __restrict__ rowptr,
                                                             const int32_t* __restrict__ nbr, int32_t* par,
                                                             unsigned long long* hooks, int* changed) {
  const int lane = threadIdx.x & 63;
  const int item = (blockIdx.x * MDE_BLOCK + threadIdx.x) >> 6;   // (uniform over the wave)
  if (item >= n_heavy) return;
  const int u = heavy[item];
  int m = 0x7fffffff;
  for (int h = rowptr[u] + lane; h < rowptr[u + 1]; h += 64) {
    const int pv = par[nbr[h]];
    m = pv < m ? pv : m;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const int other = __shfl_xor(m, o, 64);
    m = other < m ? other : m;
  }
  cc_offer(par, u, m, lane == 0, hooks, changed);
}

__global__ __launch_bounds__(MDE_BLOCK) void k_cc_jump(int n, int32_t* par, int* changed) {
  const int u = blockIdx.x * MDE_BLOCK + threadIdx.x;
  if (u >= n) return;
  const int p0 = par[u];
  int p = p0;
#pragma unroll 1
  for (int s = 0; s < CC_JUMPS; ++s) {
    const int q = par[p];
    if (q == p) break;
    p = q;
  }
  if (p != p0) {
    par[u] = p;   // (p < p0: the one writer of this slot in this launch)
    *changed = 1;
  }
}

__global__ __launch_bounds__(MDE_BLOCK) void k_cc_roots(int n, const int32_t* __restrict__ par,
                                                        int32_t* __restrict__ is_root) {
  const int u = blockIdx.x * MDE_BLOCK + threadIdx.x;
  if (u < n) is_root[u] = par[u] == u ? 1 : 0;
}

__global__ __launch_bounds__(MDE_BLOCK) void k_cc_labels(int n, const int32_t* __restrict__ par,
                                                         const int32_t* __restrict__ rank,
                                                         int32_t* __restrict__ labels) {
  const int u = blockIdx.x * MDE_BLOCK + threadIdx.x;
  if (u < n) labels[u] = rank[par[u]];
}

static thread_local int64_t g_cc_stats[3] = {0, 0, 0};

// What the last mde_graph_components call of this thread did: stats[0] rounds (the last one changed nothing),
// [1] kernel launches, [2] hook operations that lowered a slot of the parent array.
extern "C" int mde_graph_components_stats(int64_t* stats) {
  if (!stats) return MDE_E_INVALID;
  for (int q = 0; q < 3; ++q) stats[q] = g_cc_stats[q];
  return MDE_OK;
}

extern "C" int mde_graph_components(const mde_plan* plan, int32_t* labels_out, int64_t* count_host, void* stream) {
  if (!plan || !labels_out || !count_host) {
    mde_set_error("mde_graph_components: plan, labels_out and count_host must not be NULL");
    return MDE_E_INVALID;
  }
  if (plan->row_lo != 0 || plan->row_hi != plan->n) {
    mde_set_error("mde_graph_components needs a full (unsharded) plan");
    return MDE_E_INVALID;
  }
  const int64_t n64 = plan->n;
  if (n64 < 1 || n64 >= ((int64_t)1 << 31)) return MDE_E_TOO_LARGE;
  const int n = (int)n64;
  hipStream_t st = mde_stream(stream);
  MdeDeviceBuf<int32_t> par, heavy, rank;
  MdeDeviceBuf<unsigned long long> counters;   // [0] hooks | [1] heavy count (int) | [2] changed (int)
  MdeDeviceBuf<char> tmp;
  MDE_HIP(par.alloc((size_t)n * sizeof(int32_t)));
  MDE_HIP(heavy.alloc((size_t)n * sizeof(int32_t)));
  MDE_HIP(rank.alloc((size_t)n * sizeof(int32_t)));
  MDE_HIP(counters.alloc(3 * sizeof(unsigned long long)));
  MDE_HIP(hipMemsetAsync(counters.get(), 0, 3 * sizeof(unsigned long long), st));
  unsigned long long* hooks = counters.get();
  int* heavy_count = reinterpret_cast<int*>(counters.get() + 1);
  int* changed = reinterpret_cast<int*>(counters.get() + 2);
  const dim3 grid((unsigned)((n64 + MDE_BLOCK - 1) / MDE_BLOCK)), block(MDE_BLOCK);
  int64_t launches = 0, rounds = 0;
  hipLaunchKernelGGL(k_cc_init, grid, block, 0, st, n, plan->rowptr, par.get(), heavy.get(), heavy_count);
  MDE_LAUNCH_CHECK();
  ++launches;
  int n_heavy = 0;
  MDE_HIP(hipMemcpyAsync(&n_heavy, heavy_count, sizeof(int), hipMemcpyDeviceToHost, st));
  MDE_HIP(hipStreamSynchronize(st));
  bool converged = plan->H == 0;               // no edge: every node is its own component
  while (!converged && rounds < CC_MAX_ROUNDS) {
    MDE_HIP(hipMemsetAsync(changed, 0, sizeof(int), st));
    hipLaunchKernelGGL(k_cc_hook, grid, block, 0, st, n, plan->rowptr, plan->nbr, par.get(), hooks, changed);
    MDE_LAUNCH_CHECK();
    ++launches;
    if (n_heavy > 0) {
      hipLaunchKernelGGL(k_cc_hook_heavy, dim3((unsigned)(((int64_t)n_heavy * 64 + MDE_BLOCK - 1) / MDE_BLOCK)), block,
                         0, st, n_heavy, heavy.get(), plan->rowptr, plan->nbr, par.get(), hooks, changed);
      MDE_LAUNCH_CHECK();
      ++launches;
    }
    hipLaunchKernelGGL(k_cc_jump, grid, block, 0, st, n, par.get(), changed);
    MDE_LAUNCH_CHECK();
    ++launches;
    ++rounds;
    int h = 0;
    MDE_HIP(hipMemcpyAsync(&h, changed, sizeof(int), hipMemcpyDeviceToHost, st));
    MDE_HIP(hipStreamSynchronize(st));
    converged = h == 0;
  }
  unsigned long long hooked = 0;
  MDE_HIP(hipMemcpyAsync(&hooked, hooks, sizeof(hooked), hipMemcpyDeviceToHost, st));
  MDE_HIP(hipStreamSynchronize(st));
  g_cc_stats[0] = rounds;
  g_cc_stats[1] = launches;
  g_cc_stats[2] = (int64_t)hooked;
  if (!converged) {
    mde_set_error("mde_graph_components: still changing after %d rounds over %lld nodes", CC_MAX_ROUNDS,
                  (long long)n64);
    return MDE_E_INVALID;
  }
  // labels: the exclusive sum of the root flags numbers the roots in node order (heavy[] is free: the flags)
  int32_t* is_root = heavy.get();
  hipLaunchKernelGGL(k_cc_roots, grid, block, 0, st, n, par.get(), is_root);
  MDE_LAUNCH_CHECK();
  size_t tmp_bytes = 0;
  MDE_HIP(mde_exclusive_sum_i32(nullptr, tmp_bytes, is_root, rank.get(), n, st));
  MDE_HIP(tmp.alloc(tmp_bytes ? tmp_bytes : 16));
  MDE_HIP(mde_exclusive_sum_i32(tmp.get(), tmp_bytes, is_root, rank.get(), n, st));
  hipLaunchKernelGGL(k_cc_labels, grid, block, 0, st, n, par.get(), rank.get(), labels_out);
  MDE_LAUNCH_CHECK();
  int32_t last[2] = {0, 0};
  MDE_HIP(hipMemcpyAsync(&last[0], rank.get() + (n - 1), sizeof(int32_t), hipMemcpyDeviceToHost, st));
  MDE_HIP(hipMemcpyAsync(&last[1], is_root + (n - 1), sizeof(int32_t), hipMemcpyDeviceToHost, st));
  MDE_HIP(hipStreamSynchronize(st));
  g_cc_stats[1] = launches + 3;                // (the scan's own launches are the library's)
  *count_host = (int64_t)last[0] + last[1];
  return MDE_OK;
}

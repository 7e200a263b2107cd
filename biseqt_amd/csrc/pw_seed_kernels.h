// pw_seed_kernels.h -- device code shared by the pairwise seed index (pw_seeds.hip), the N-way one (pw_mseeds.hip) and the
// query-batched one (pw_qseeds.hip): the k-mer encoder (K5a), the direct-address table of the join (K5b), the diagonal
// starts of K7's sorted points, the 64-bit widening and the last-offset read
// used around rocPRIM's scans, and the connected components of a CSR graph (K7's hook / compress).  Kernels live in an
// anonymous namespace: each translation unit gets its own copy.  The three include it through pw_seed_host.h, which holds
// the host code that launches most of these kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pw_hip_host.h"

namespace {

constexpr int kMaxMasks = 16;
struct MaskSets { uint64_t set[kMaxMasks]; int n; };

// ---- K5a ------------------------------------------------------------------------------------------------
// Key type K: 32 bits whenever L^k (the masked key included) fits -- DNA words up to k = 15 -- which cuts the sort's
// traffic from 12 to 8 bytes per k-mer and pass; 64 bits otherwise.
template <typename K>
__global__ __launch_bounds__(256) void k_encode(const uint8_t* __restrict__ seq, int64_t n, int k, int L,
                                                uint64_t kinv, MaskSets ms, K* __restrict__ keys,
                                                uint32_t* __restrict__ pos) {
  __shared__ uint8_t tile[256 + 64];
  const int64_t base = (int64_t)blockIdx.x * 256;
  const int64_t nk = n - k + 1;
  for (int t = (int)threadIdx.x; t < 256 + k - 1; t += 256) {
    const int64_t p = base + t;
    tile[t] = p < n ? seq[p] : 0;
  }
  __syncthreads();
  const int64_t p = base + threadIdx.x;
  if (p >= nk) return;
  uint64_t v = 0, lets = 0;
  for (int t = 0; t < k; t++) {
    const uint32_t c = tile[threadIdx.x + t];
    v = v * (uint64_t)L + c;
    lets |= 1ull << c;
  }
  bool masked = false;
  for (int i = 0; i < ms.n; i++) masked |= lets == ms.set[i];
  keys[p] = (K)(masked ? kinv : v);
  pos[p] = (uint32_t)p;
}

// ---- K5b's direct-address table ---------------------------------------------------------------------------
// tab[q] = number of elements of the sorted keys `other` below q, for q = 0 .. kinv + 1: element i (the first of its run)
// fills the keys after the previous run's key up to its own; one extra thread fills the tail.  (Used only when the keys
// are dense enough that these gaps are short: table_pays, pw_seed_host.h.)
template <typename K>
__global__ __launch_bounds__(256) void k_table_fill(const K* __restrict__ other, int64_t no, uint64_t kinv, uint32_t* __restrict__ tab) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i > no) return;
  const int64_t prev = i > 0 ? (int64_t)other[i - 1] : -1;
  const int64_t cur = i < no ? (int64_t)other[i] : (int64_t)kinv + 1;
  for (int64_t q = prev + 1; q <= cur; q++) tab[q] = (uint32_t)i;
}

__global__ __launch_bounds__(256) void k_widen(const uint32_t* __restrict__ in, int64_t n, uint64_t* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) out[i] = in[i];
}
__device__ __forceinline__ int cc_root(const int* __restrict__ parent, int v) {
  int p = parent[v];
  while (p != v) { v = p; p = parent[v]; }
  return v;
}
__global__ __launch_bounds__(256) void k_cc_init(const uint8_t* __restrict__ avail, int64_t n, int* __restrict__ parent) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) parent[i] = avail[i] ? (int)i : -1;
}
__global__ __launch_bounds__(256) void k_cc_hook(const uint64_t* __restrict__ off, const uint32_t* __restrict__ cnt,
                                                 const uint32_t* __restrict__ adj, int64_t n, int* __restrict__ parent,
                                                 int* __restrict__ changed) {
  const int64_t u = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (u >= n || parent[u] < 0) return;
  const uint64_t b = off[u], e = b + cnt[u];
  for (uint64_t t = b; t < e; t++) {
    const int v = (int)adj[t];
    if (parent[v] < 0) continue;
    const int ru = cc_root(parent, (int)u), rv = cc_root(parent, v);
    if (ru != rv) { atomicMin(&parent[ru > rv ? ru : rv], ru > rv ? rv : ru); *changed = 1; }
  }
}
__global__ __launch_bounds__(256) void k_cc_compress(int64_t n, int* __restrict__ parent) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n && parent[i] >= 0) parent[i] = cc_root(parent, (int)i);
}

__global__ void k_total(const uint64_t* __restrict__ off, const uint64_t* __restrict__ cnt, int64_t ns,
                        unsigned long long* __restrict__ out) {
  if (threadIdx.x == 0 && blockIdx.x == 0) out[0] = ns > 0 ? off[ns - 1] + cnt[ns - 1] : 0ull;
}

// ---- K7: start of every diagonal's run in the (d, a)-sorted keys of the neighbourhood graph ----------------
__global__ __launch_bounds__(256) void k_graph_dstart(const uint64_t* __restrict__ keys, int64_t n, int64_t nd, uint32_t* __restrict__ dstart) {
  const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (q > nd) return;
  dstart[q] = (uint32_t)lower_bound_dev<uint64_t>(keys, n, (uint64_t)q << 32);
}

}  // namespace

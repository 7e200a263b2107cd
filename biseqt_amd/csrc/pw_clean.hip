// pw_clean.hip -- K19: tip removal and bubble popping on the reduced overlap graph (include/pw_graph.h, CLEANING, holds the
// contract).  One round works on the decomposition that pw_graph.hip's unitig stages leave behind -- kept-arc counts, chain
// links, and the doubling state that gives every live vertex its head, its rank and, at the head, the member count and the
// smallest vertex of its component -- and is five launches, one thread per vertex or per arc:
//   - k_clean_cand: the tail of every linear component writes, at its head, whether the component is a tip or a bubble
//     candidate, the tail itself, and a bubble candidate's source and sink.
//   - k_clean_tips: the tail t of a tip candidate walks, for every kept arc t -> w, the row of w ^ 1 -- its kept arcs are the
//     twins of the kept arcs entering w -- and compares (n, mr) with the component of every other arc's tail.
//   - k_clean_bubbles: the head of a bubble candidate goes across the row of its source to the heads of the parallel
//     candidates and compares (n, mr) where source and sink agree.
//   - k_clean_drop: every vertex looks its component's verdict up through the head of its doubling state and stores it for
//     its read.
//   - k_clean_arcs: every kept arc with an end on a dropped read gets PW_ARC_REMOVED | PW_ARC_DROPPED.
// Order independence: every verdict is a function of the decomposition alone, which no kernel of the round changes before
// k_clean_arcs; a component's verdict has one writer (its tail for a tip, its head for a bubble, and no component is both);
// the two vertices of a read never carry different non-zero verdicts (the contract's last paragraph), so the byte stores of
// k_clean_drop are stores of one constant; an arc has one writer.  No atomics, no LDS, no scratch, and no kernel waits for
// another workgroup: every dependency is a launch boundary on the stream.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/pw_graph.h"
#include "pw_graph_launch.h"

static_assert(sizeof(pw_graph_clean_params) == 16, "cleaning parameter record must be 16 bytes");

namespace pw {

namespace {

#define CL_TRY(call) do { const hipError_t e_ = (call); if (e_ != hipSuccess) return e_; } while (0)

// D (n_d members, smallest read mr_d, tip candidate or not) is stronger than the tip candidate C
__device__ __forceinline__ bool cl_stronger(bool cand_d, int n_d, int mr_d, int n_c, int mr_c) {
  return !cand_d || n_d > n_c || (n_d == n_c && mr_d < mr_c);
}

}  // namespace

// cflag / ctail / cs / cz at the head of every linear component (cflag is zeroed before), written by the component's tail
__global__ __launch_bounds__(256) void k_clean_cand(const pw_graph_arc* __restrict__ arcs, const GraphChain* __restrict__ st,
                                                    const int32_t* __restrict__ succ, const uint8_t* __restrict__ cut,
                                                    const uint8_t* __restrict__ contained, const uint8_t* __restrict__ dropped,
                                                    const uint32_t* __restrict__ out, const int32_t* __restrict__ one, int V, int max_tip,
                                                    int max_bubble, uint8_t* __restrict__ cflag, int32_t* __restrict__ ctail,
                                                    int32_t* __restrict__ cs, int32_t* __restrict__ cz) {
  const int t = (int)(blockIdx.x * 256 + threadIdx.x);
  if (t >= V || (contained[t >> 1] | dropped[t >> 1])) return;
  const int nx = succ[t];
  if (nx >= 0 && !cut[nx]) return;                        // not a tail
  const GraphChain c = st[t];
  if (c.nxt >= 0 || (uint32_t)c.hd >= (uint32_t)V) return;          // (never after the cut: every chain has a head)
  const int h = c.hd;
  if (cut[h]) return;                                     // circular
  const long long n = (long long)c.d + 1;
  const uint32_t in_h = out[h ^ 1], out_t = out[t];
  uint8_t f = 0;
  if (max_tip > 0 && n <= max_tip && in_h == 0 && out_t >= 1) f |= 1;
  if (max_bubble > 0 && n <= max_bubble && in_h == 1 && out_t == 1) {
    const int s = arcs[one[h ^ 1]].w ^ 1, z = arcs[one[t]].w;       // the twin of the arc leaving h ^ 1 enters h
    const int rh = h >> 1, rt = t >> 1;
    if ((uint32_t)s < (uint32_t)V && (uint32_t)z < (uint32_t)V && (s >> 1) != rh && (s >> 1) != rt && (z >> 1) != rh && (z >> 1) != rt) {
      f |= 2; cs[h] = s; cz[h] = z;
    }
  }
  if (f) { cflag[h] = f; ctail[h] = t; }
}

// cdrop[h] = 1 for a tip candidate that a stronger component competes with (cdrop is zeroed before)
__global__ __launch_bounds__(256) void k_clean_tips(const pw_graph_arc* __restrict__ arcs, const long long* __restrict__ rows,
                                                    const GraphChain* __restrict__ st, const uint8_t* __restrict__ cflag,
                                                    const int32_t* __restrict__ ctail, const int32_t* __restrict__ hcnt,
                                                    const int32_t* __restrict__ hmin, int V, uint8_t* __restrict__ cdrop) {
  const int t = (int)(blockIdx.x * 256 + threadIdx.x);
  if (t >= V) return;
  const int h = st[t].hd;
  if ((uint32_t)h >= (uint32_t)V || !(cflag[h] & 1) || ctail[h] != t) return;
  const int n_c = hcnt[h], mr_c = hmin[h] >> 1;
  for (long long i = rows[t]; i < rows[t + 1]; i++) {
    if (arcs[i].flags & PW_ARC_REMOVED) continue;
    const int w = arcs[i].w;
    if ((uint32_t)w >= (uint32_t)V) continue;             // (never: vertices come from validated read indices)
    for (long long j = rows[w ^ 1]; j < rows[(w ^ 1) + 1]; j++) {
      if (arcs[j].flags & PW_ARC_REMOVED) continue;
      const int u = arcs[j].w ^ 1;                        // the twin of w ^ 1 -> u ^ 1 is u -> w
      if (u == t || (uint32_t)u >= (uint32_t)V) continue;
      const int hd = st[u].hd;
      if ((uint32_t)hd >= (uint32_t)V) continue;          // (never)
      if (cl_stronger(cflag[hd] & 1, hcnt[hd], hmin[hd] >> 1, n_c, mr_c)) { cdrop[h] = 1; return; }
    }
  }
}

// cdrop[h] = 2 for a bubble candidate that loses against a parallel one
__global__ __launch_bounds__(256) void k_clean_bubbles(const pw_graph_arc* __restrict__ arcs, const long long* __restrict__ rows,
                                                       const uint8_t* __restrict__ cflag, const int32_t* __restrict__ cs,
                                                       const int32_t* __restrict__ cz, const int32_t* __restrict__ hcnt,
                                                       const int32_t* __restrict__ hmin, int V, uint8_t* __restrict__ cdrop) {
  const int h = (int)(blockIdx.x * 256 + threadIdx.x);
  if (h >= V || !(cflag[h] & 2)) return;
  const int s = cs[h], z = cz[h];
  const int n_c = hcnt[h], mr_c = hmin[h] >> 1;
  for (long long j = rows[s]; j < rows[s + 1]; j++) {
    if (arcs[j].flags & PW_ARC_REMOVED) continue;
    const int g = arcs[j].w;
    if (g == h || (uint32_t)g >= (uint32_t)V || !(cflag[g] & 2) || cs[g] != s || cz[g] != z) continue;
    const int n_d = hcnt[g], mr_d = hmin[g] >> 1;
    if (n_d > n_c || (n_d == n_c && mr_d < mr_c)) { cdrop[h] = 2; return; }
  }
}

// dropped[r] = the verdict of the component of either vertex of r
__global__ __launch_bounds__(256) void k_clean_drop(const GraphChain* __restrict__ st, const uint8_t* __restrict__ cdrop, int V,
                                                    uint8_t* __restrict__ dropped) {
  const int v = (int)(blockIdx.x * 256 + threadIdx.x);
  if (v >= V) return;
  const int h = st[v].hd;
  if ((uint32_t)h >= (uint32_t)V) return;                 // (never)
  const uint8_t d = cdrop[h];
  if (d) dropped[v >> 1] = d;
}

// REMOVED | DROPPED for every kept arc with an end on a dropped read (the arc's only writer)
__global__ __launch_bounds__(256) void k_clean_arcs(pw_graph_arc* __restrict__ arcs, long long n_arcs, const uint8_t* __restrict__ dropped,
                                                    long long n_reads) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n_arcs) return;
  const int f = arcs[i].flags;
  if (f & PW_ARC_REMOVED) return;
  const long long a = arcs[i].v >> 1, b = arcs[i].w >> 1;
  if ((unsigned long long)a >= (unsigned long long)n_reads || (unsigned long long)b >= (unsigned long long)n_reads) return;      // (never)
  if (dropped[a] | dropped[b]) arcs[i].flags = f | PW_ARC_REMOVED | PW_ARC_DROPPED;
}

hipError_t clean_round(GraphState& g, int cur, int64_t n_arcs, const pw_graph_clean_params& c, hipStream_t st) {
  const int V = (int)g.V;
  const size_t nV = (size_t)V;
  if (!V) return hipSuccess;
  CL_TRY(g.d_cflag.ensure(nV)); CL_TRY(g.d_cdrop.ensure(nV)); CL_TRY(g.d_ctail.ensure(nV)); CL_TRY(g.d_cs.ensure(nV)); CL_TRY(g.d_cz.ensure(nV));
  const dim3 vgrid = rows_grid((uint64_t)V);
  const long long* rows = (const long long*)g.d_rows.cp();
  CL_TRY(hipMemsetAsync(g.d_cflag.p, 0, nV, st));
  CL_TRY(hipMemsetAsync(g.d_cdrop.p, 0, nV, st));
  hipLaunchKernelGGL(k_clean_cand, vgrid, kBlock256, 0, st, g.d_arcs.cp(), g.d_chain[cur].cp(), g.d_succ.cp(), g.d_cut.cp(), g.d_contained.cp(),
                     g.d_dropped.cp(), g.d_out.cp(), g.d_one.cp(), V, (int)c.max_tip_reads, (int)c.max_bubble_reads, g.d_cflag.p, g.d_ctail.p,
                     g.d_cs.p, g.d_cz.p);
  CL_TRY(hipGetLastError());
  if (c.max_tip_reads > 0) {
    hipLaunchKernelGGL(k_clean_tips, vgrid, kBlock256, 0, st, g.d_arcs.cp(), rows, g.d_chain[cur].cp(), g.d_cflag.cp(), g.d_ctail.cp(),
                       g.d_hcnt.cp(), g.d_hmin.cp(), V, g.d_cdrop.p);
    CL_TRY(hipGetLastError());
  }
  if (c.max_bubble_reads > 0) {
    hipLaunchKernelGGL(k_clean_bubbles, vgrid, kBlock256, 0, st, g.d_arcs.cp(), rows, g.d_cflag.cp(), g.d_cs.cp(), g.d_cz.cp(), g.d_hcnt.cp(),
                       g.d_hmin.cp(), V, g.d_cdrop.p);
    CL_TRY(hipGetLastError());
  }
  hipLaunchKernelGGL(k_clean_drop, vgrid, kBlock256, 0, st, g.d_chain[cur].cp(), g.d_cdrop.cp(), V, g.d_dropped.p);
  CL_TRY(hipGetLastError());
  if (n_arcs > 0) {
    hipLaunchKernelGGL(k_clean_arcs, rows_grid((uint64_t)n_arcs), kBlock256, 0, st, g.d_arcs.p, (long long)n_arcs, g.d_dropped.cp(),
                       (long long)g.n_reads);
    CL_TRY(hipGetLastError());
  }
  return hipSuccess;
}

}  // namespace pw

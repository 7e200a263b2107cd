// pw_graph.hip -- K17: the overlap graph (include/pw_graph.h holds the contract: records, classification, arcs, transitive
// reduction, unitigs, contig letters).  One thread per record, arc or vertex everywhere except in two kernels:
//   - k_graph_reduce, the hot one: one wavefront per vertex v with at least two arcs.  For every arc v -> w of v's row (a
//     uniform loop) the lanes go across the row of w, 64 arcs w -> x per pass, and look the target x up in v's own row:
//     a binary search in the row's (v << 32 | w) keys, sorted a second time by target, then every arc v -> x of the equal
//     range (a key may repeat) is tested and marked with a 32-bit atomic OR of a constant.  Rows longer than a wavefront
//     are the same loops running longer, on either side.  Nothing is read that another wavefront writes but the flag
//     dwords, and those are only ever ORed: the marks do not depend on arrival order.
//   - k_graph_contig_write: one wavefront per member copies (or reverse-complements) the member's advance letters.
// Heads, ranks, offsets and component minima come from pointer doubling over the chain predecessors: k_graph_double, one
// launch per round on ping-pong buffers, the round count fixed from the number of vertices alone.  A vertex that has
// reached no head after the last round lies on a cycle, and its `m` is then the cycle's smallest vertex: k_graph_cut cuts
// the link entering that vertex and the doubling runs once more.  The last member of every chain (k_graph_tails) hands
// the member count, the length and the smallest vertex to its head; heads and members are placed by two exclusive scans.
// No kernel waits for another workgroup: every dependency is a launch boundary on the stream.  No LDS, no scratch.
// The decomposition (graph_chains: out, chain links, doubling, cut, tails) runs once for the unitigs and, before that, once
// per cleaning round (K19, pw_clean.hip), then without marking the links; tails and heads skip contained and dropped reads.
// The arc sort (stable: the contract's order relies on it), the sort by target, the scans and the row index (a lower
// bound of v << 32 in the sorted keys) are rocPRIM's, through rocprim_run.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <cstring>
#include <rocprim/rocprim.hpp>

#include "../../include/pw_graph.h"
#include "../../include/pw_txsum.h"
#include "pw_graph_launch.h"

static_assert(sizeof(pw_graph_overlap) == 40, "overlap record must be 40 bytes");
static_assert(sizeof(pw_graph_params) == 32, "parameter record must be 32 bytes");
static_assert(sizeof(pw_graph_arc) == 24, "arc record must be 24 bytes");
static_assert(sizeof(pw_unitig) == 32, "unitig record must be 32 bytes");
static_assert(sizeof(pw_unitig_member) == 16, "member record must be 16 bytes");
static_assert(sizeof(pw::GraphChain) == 24, "doubling state must be 24 bytes");

namespace pw {

namespace {

#define GR_TRY(call) do { const hipError_t e_ = (call); if (e_ != hipSuccess) return e_; } while (0)

// The classification of include/pw_graph.h, rule by rule.
__device__ __forceinline__ int gr_classify(const pw_graph_overlap& r, int la, int lb, const pw_graph_params& p) {
  if (r.n_ops == 0) return PW_OVL_NONE;
  const long long sa = (long long)r.a_end - r.a_beg, sb = (long long)r.b_end - r.b_beg;
  if ((sa < sb ? sa : sb) < (long long)p.min_overlap || (double)r.n_match < p.min_identity * (double)r.n_ops) return PW_OVL_WEAK;
  const long long ta = (long long)la - r.a_end, tb = (long long)lb - r.b_end;
  const long long ext = (long long)(r.a_beg < r.b_beg ? r.a_beg : r.b_beg) + (ta < tb ? ta : tb);
  const long long span = sa > sb ? sa : sb;
  const double x = (double)p.max_hang, y = (double)span * p.int_frac;
  if ((double)ext > (y < x ? y : x)) return PW_OVL_INTERNAL;
  if (r.a_beg <= r.b_beg && ta <= tb) return PW_OVL_A_CONTAINED;
  if (r.a_beg >= r.b_beg && ta >= tb) return PW_OVL_B_CONTAINED;
  return r.a_beg > r.b_beg ? PW_OVL_A_TO_B : PW_OVL_B_TO_A;
}

// the advance of member v: the len of its chain link (the cut link of a cycle's last member included), else its read length
__device__ __forceinline__ int gr_advance(int v, const int32_t* __restrict__ succ, const int32_t* __restrict__ adv,
                                          const int32_t* __restrict__ lens) {
  return succ[v] >= 0 ? adv[v] : lens[v >> 1];
}

struct RowKey {
  __host__ __device__ uint64_t operator()(uint64_t v) const { return v << 32; }
};

}  // namespace

// Records [0, n) of a batch behind the records that are there: pair k's result and summary, its reads from stage[3][n].
__global__ __launch_bounds__(256) void k_graph_from_batch(const Result* __restrict__ results, const pw_tx_summary* __restrict__ sums,
                                                          const int32_t* __restrict__ stage, int n, pw_graph_overlap* __restrict__ out) {
  const int k = (int)(blockIdx.x * 256 + threadIdx.x);
  if (k >= n) return;
  pw_graph_overlap r = {stage[k], stage[n + k], stage[2 * n + k], PW_OVL_NONE, 0, 0, 0, 0, 0, 0};
  const pw_tx_summary s = sums[k];
  if (s.flags & PW_TXSUM_DONE) {
    const Result res = results[k];
    r.a_beg = res.origin_idx; r.a_end = res.origin_idx + s.n_match + s.n_subst + s.n_del;
    r.b_beg = res.mutant_idx; r.b_end = res.mutant_idx + s.n_match + s.n_subst + s.n_ins;
    r.n_match = s.n_match; r.n_ops = s.n_match + s.n_subst + s.n_ins + s.n_del;
  }
  out[k] = r;
}

// cls of every record; the contained flags (zeroed before) get plain byte stores of the constant 1
__global__ __launch_bounds__(256) void k_graph_classify(pw_graph_overlap* __restrict__ recs, long long n, const int32_t* __restrict__ lens,
                                                        pw_graph_params p, uint8_t* __restrict__ contained) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const pw_graph_overlap r = recs[i];
  const int cls = gr_classify(r, lens[r.a], lens[r.b], p);
  recs[i].cls = cls;
  if (cls == PW_OVL_A_CONTAINED) contained[r.a] = 1;
  else if (cls == PW_OVL_B_CONTAINED) contained[r.b] = 1;
}

// cnt[i] = 1 for a record that gives arcs (the scan's input)
__global__ __launch_bounds__(256) void k_graph_arc_count(const pw_graph_overlap* __restrict__ recs, long long n,
                                                         const uint8_t* __restrict__ contained, unsigned long long* __restrict__ cnt) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const pw_graph_overlap& r = recs[i];
  cnt[i] = (r.cls == PW_OVL_A_TO_B || r.cls == PW_OVL_B_TO_A) && !contained[r.a] && !contained[r.b];
}

// The arc and the twin of the t-th arc-giving record at gen[2t], gen[2t + 1], with their sort keys and positions.
__global__ __launch_bounds__(256) void k_graph_arcs(const pw_graph_overlap* __restrict__ recs, long long n, const int32_t* __restrict__ lens,
                                                    const unsigned long long* __restrict__ cnt, const unsigned long long* __restrict__ off,
                                                    long long n_arcs, pw_graph_arc* __restrict__ gen, unsigned long long* __restrict__ keys,
                                                    uint32_t* __restrict__ idx) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n || !cnt[i]) return;
  const long long g = 2 * (long long)off[i];
  if (g + 1 >= n_arcs) return;                            // (never: the table was allocated from this scan's total)
  const pw_graph_overlap r = recs[i];
  const int va = 2 * r.a, vb = 2 * r.b + r.strand;
  const int ta = lens[r.a] - r.a_end, tb = lens[r.b] - r.b_end;
  const int sa = r.a_end - r.a_beg, sb = r.b_end - r.b_beg;
  pw_graph_arc x, y;
  if (r.cls == PW_OVL_A_TO_B) {
    x = {va, vb, r.a_beg - r.b_beg, sa, (int32_t)i, 0};
    y = {vb ^ 1, va + 1, tb - ta, sb, (int32_t)i, 0};
  } else {
    x = {vb, va, r.b_beg - r.a_beg, sb, (int32_t)i, 0};
    y = {va + 1, vb ^ 1, ta - tb, sa, (int32_t)i, 0};
  }
  gen[g] = x; gen[g + 1] = y;
  keys[g] = ((unsigned long long)(uint32_t)x.v << 32) | (uint32_t)x.len;
  keys[g + 1] = ((unsigned long long)(uint32_t)y.v << 32) | (uint32_t)y.len;
  idx[g] = (uint32_t)g; idx[g + 1] = (uint32_t)(g + 1);
}

// The sorted table: arcs[s] = gen[idx_s[s]]; pos = the inverse of idx_s; the keys and values of the sort by target.
__global__ __launch_bounds__(256) void k_graph_gather(const pw_graph_arc* __restrict__ gen, const uint32_t* __restrict__ idx_s, long long n_arcs,
                                                      pw_graph_arc* __restrict__ arcs, uint32_t* __restrict__ pos,
                                                      unsigned long long* __restrict__ tkeys, uint32_t* __restrict__ tval) {
  const long long s = (long long)blockIdx.x * 256 + threadIdx.x;
  if (s >= n_arcs) return;
  const uint32_t g = idx_s[s];
  if (g >= (unsigned long long)n_arcs) return;            // (never: a permutation)
  const pw_graph_arc a = gen[g];
  arcs[s] = a;
  pos[g] = (uint32_t)s;
  tkeys[s] = ((unsigned long long)(uint32_t)a.v << 32) | (uint32_t)a.w;
  tval[s] = (uint32_t)s;
}

// Transitive reduction: one wavefront per vertex (see the top of the file).  tkeys / tarc: the arcs sorted by (v, w) and
// their indices in the arc table; row v of both is [rows[v], rows[v + 1]).
__global__ __launch_bounds__(64) void k_graph_reduce(pw_graph_arc* __restrict__ arcs, const long long* __restrict__ rows,
                                                     const unsigned long long* __restrict__ tkeys, const uint32_t* __restrict__ tarc,
                                                     int V, int fuzz) {
  const int v = (int)blockIdx.x;
  const int lane = (int)(threadIdx.x & 63u);
  const long long r0 = rows[v], r1 = rows[v + 1];
  if (r1 - r0 < 2) return;                                // (uniform)
  const long long top = (long long)arcs[r1 - 1].len + fuzz;        // the row ascends in len: no sum above this marks anything
  for (long long i = r0; i < r1; i++) {
    const int w = arcs[i].w;
    const long long len1 = arcs[i].len;
    if ((uint32_t)w >= (uint32_t)V) continue;             // (never: vertices come from validated read indices)
    const long long s0 = rows[w], s1 = rows[w + 1];
    for (long long j = s0 + lane; j < s1; j += 64) {
      const int x = arcs[j].w;
      const long long sum = len1 + arcs[j].len;
      if (x == w || sum > top) continue;
      const unsigned long long key = ((unsigned long long)(uint32_t)v << 32) | (uint32_t)x;
      for (long long k = r0 + lower_bound_dev(tkeys + r0, r1 - r0, key); k < r1 && tkeys[k] == key; k++) {
        const uint32_t t = tarc[k];
        if (sum <= (long long)arcs[t].len + fuzz) atomicOr((unsigned int*)&arcs[t].flags, (unsigned int)PW_ARC_REDUCED);
      }
    }
  }
}

// REMOVED: the arc or its twin (the arc generated beside it) is reduced
__global__ __launch_bounds__(256) void k_graph_twins(pw_graph_arc* __restrict__ arcs, const uint32_t* __restrict__ idx_s,
                                                     const uint32_t* __restrict__ pos, long long n_arcs) {
  const long long s = (long long)blockIdx.x * 256 + threadIdx.x;
  if (s >= n_arcs) return;
  const uint32_t t = pos[idx_s[s] ^ 1u];
  if (t >= (unsigned long long)n_arcs) return;            // (never)
  if ((arcs[s].flags | arcs[t].flags) & PW_ARC_REDUCED) atomicOr((unsigned int*)&arcs[s].flags, (unsigned int)PW_ARC_REMOVED);
}

// out[v] = kept arcs leaving v; one[v] = the last of them
__global__ __launch_bounds__(256) void k_graph_out(const pw_graph_arc* __restrict__ arcs, const long long* __restrict__ rows, int V,
                                                   uint32_t* __restrict__ out, int32_t* __restrict__ one) {
  const int v = (int)(blockIdx.x * 256 + threadIdx.x);
  if (v >= V) return;
  uint32_t n = 0;
  int32_t last = -1;
  for (long long i = rows[v]; i < rows[v + 1]; i++)
    if (!(arcs[i].flags & PW_ARC_REMOVED)) { n++; last = (int32_t)i; }
  out[v] = n; one[v] = last;
}

// Chain links: succ / adv of every vertex; pred (filled with -1 before) of the link's target -- one writer: out(w ^ 1) == 1.
// mark == 0 (the decomposition of a cleaning round): the links get no PW_ARC_CHAIN.
__global__ __launch_bounds__(256) void k_graph_chain(pw_graph_arc* __restrict__ arcs, const uint32_t* __restrict__ out,
                                                     const int32_t* __restrict__ one, int V, int mark, int32_t* __restrict__ succ,
                                                     int32_t* __restrict__ pred, int32_t* __restrict__ adv) {
  const int v = (int)(blockIdx.x * 256 + threadIdx.x);
  if (v >= V) return;
  int s = -1, a = 0;
  if (out[v] == 1) {
    const int32_t i = one[v];
    const int w = arcs[i].w;
    if ((uint32_t)w < (uint32_t)V && out[w ^ 1] == 1 && w != v && w != (v ^ 1)) {
      s = w; a = arcs[i].len;
      pred[w] = v;
      if (mark) arcs[i].flags |= PW_ARC_CHAIN;            // (the arc's only writer in this launch)
    }
  }
  succ[v] = s; adv[v] = a;
}

// Round 0 of the doubling: one link up, unless the vertex has no predecessor or its link is cut.
__global__ __launch_bounds__(256) void k_graph_chain_init(const int32_t* __restrict__ pred, const int32_t* __restrict__ adv,
                                                          const uint8_t* __restrict__ cut, int V, GraphChain* __restrict__ st) {
  const int v = (int)(blockIdx.x * 256 + threadIdx.x);
  if (v >= V) return;
  const int p = cut[v] ? -1 : pred[v];
  GraphChain c;
  if (p >= 0) c = {(uint64_t)(uint32_t)adv[p], p, p, 1u, p < v ? p : v};
  else c = {0, -1, v, 0u, v};
  st[v] = c;
}

// One round: the state of the ancestor nxt is appended to the vertex's own.
__global__ __launch_bounds__(256) void k_graph_double(const GraphChain* __restrict__ in, GraphChain* __restrict__ out, int V) {
  const int v = (int)(blockIdx.x * 256 + threadIdx.x);
  if (v >= V) return;
  GraphChain c = in[v];
  if (c.nxt >= 0) {
    const GraphChain q = in[c.nxt];
    c.o += q.o; c.d += q.d; c.m = q.m < c.m ? q.m : c.m; c.hd = q.hd; c.nxt = q.nxt;
  }
  out[v] = c;
}

// A vertex that reached no head lies on a cycle and m is the cycle's smallest vertex: that vertex heads it.
__global__ __launch_bounds__(256) void k_graph_cut(const GraphChain* __restrict__ st, int V, uint8_t* __restrict__ cut) {
  const int v = (int)(blockIdx.x * 256 + threadIdx.x);
  if (v >= V) return;
  if (st[v].nxt >= 0 && st[v].m == v) cut[v] = 1;
}

// The last member of every chain writes, at its head: the members, the length, the smallest vertex.
__global__ __launch_bounds__(256) void k_graph_tails(const GraphChain* __restrict__ st, const int32_t* __restrict__ succ,
                                                     const int32_t* __restrict__ adv, const uint8_t* __restrict__ cut,
                                                     const uint8_t* __restrict__ contained, const uint8_t* __restrict__ dropped,
                                                     const int32_t* __restrict__ lens, int V, int32_t* __restrict__ hcnt,
                                                     int32_t* __restrict__ hmin, unsigned long long* __restrict__ hlen) {
  const int v = (int)(blockIdx.x * 256 + threadIdx.x);
  if (v >= V || (contained[v >> 1] | dropped[v >> 1])) return;      // (live vertices only)
  const int s = succ[v];
  if (s >= 0 && !cut[s]) return;
  const GraphChain c = st[v];
  if (c.nxt >= 0 || (uint32_t)c.hd >= (uint32_t)V) return;         // (never after the cut: every chain has a head)
  hcnt[c.hd] = (int32_t)c.d + 1;
  hmin[c.hd] = c.m;
  hlen[c.hd] = c.o + (uint32_t)gr_advance(v, succ, adv, lens);
}

// flag[v] = 1 for the head of a kept unitig, mcnt[v] = its members (the inputs of the two scans)
__global__ __launch_bounds__(256) void k_graph_heads(const GraphChain* __restrict__ st, const uint8_t* __restrict__ contained,
                                                     const uint8_t* __restrict__ dropped, const int32_t* __restrict__ hcnt,
                                                     const int32_t* __restrict__ hmin, int V,
                                                     unsigned long long* __restrict__ flag, unsigned long long* __restrict__ mcnt) {
  const int v = (int)(blockIdx.x * 256 + threadIdx.x);
  if (v >= V) return;
  const GraphChain c = st[v];
  const bool keep = !(contained[v >> 1] | dropped[v >> 1]) && c.nxt < 0 && c.d == 0 && !(hmin[v] & 1);
  flag[v] = keep; mcnt[v] = keep ? (unsigned long long)hcnt[v] : 0ull;
}

// Every member of a kept unitig writes its record; the head writes the unitig's.
__global__ __launch_bounds__(256) void k_graph_emit(const GraphChain* __restrict__ st, const unsigned long long* __restrict__ flag,
                                                    const unsigned long long* __restrict__ uoff, const unsigned long long* __restrict__ moff,
                                                    const int32_t* __restrict__ succ, const int32_t* __restrict__ adv,
                                                    const uint8_t* __restrict__ cut, const int32_t* __restrict__ lens,
                                                    const int32_t* __restrict__ hcnt, const unsigned long long* __restrict__ hlen, int V,
                                                    long long n_unitigs, long long n_members, pw_unitig* __restrict__ unitigs,
                                                    pw_unitig_member* __restrict__ members, int32_t* __restrict__ mem_uid) {
  const int v = (int)(blockIdx.x * 256 + threadIdx.x);
  if (v >= V) return;
  const GraphChain c = st[v];
  if (c.nxt >= 0 || (uint32_t)c.hd >= (uint32_t)V || !flag[c.hd]) return;
  const long long u = (long long)uoff[c.hd], at = (long long)moff[c.hd] + c.d;
  if (u >= n_unitigs || at >= n_members) return;          // (never: both tables were allocated from these scans' totals)
  members[at] = {v, gr_advance(v, succ, adv, lens), (int64_t)c.o};
  mem_uid[at] = (int32_t)u;
  if (v == c.hd) unitigs[u] = {(int64_t)moff[v], (int64_t)hlen[v], hcnt[v], v, (int32_t)cut[v], 0};
}

// lens[u] = the letters of contig u (the scan's input)
__global__ __launch_bounds__(256) void k_graph_contig_count(const pw_unitig* __restrict__ unitigs, long long n, unsigned long long* __restrict__ lens) {
  const long long u = (long long)blockIdx.x * 256 + threadIdx.x;
  if (u < n) lens[u] = (unsigned long long)unitigs[u].length;
}

// One wavefront per member: the first `advance` letters of its oriented read at its offset in its contig.  comp: 256 bytes.
__global__ __launch_bounds__(64) void k_graph_contig_write(const pw_unitig_member* __restrict__ members, const int32_t* __restrict__ mem_uid,
                                                           const unsigned long long* __restrict__ coff, const uint8_t* __restrict__ letters,
                                                           const long long* __restrict__ roff, const int32_t* __restrict__ rlens,
                                                           const uint8_t* __restrict__ comp, uint8_t* __restrict__ out) {
  const long long m = blockIdx.x;
  const int lane = (int)(threadIdx.x & 63u);
  const pw_unitig_member mem = members[m];
  const int u = mem_uid[m], r = mem.vertex >> 1, n = rlens[r];
  const unsigned long long at = coff[u] + (unsigned long long)mem.offset, end = coff[u + 1];
  const uint8_t* __restrict__ src = letters + roff[r];
  const int cnt = mem.advance < n ? mem.advance : n;      // (never past the read)
  for (int i = lane; i < cnt; i += 64) {
    if (at + i >= end) break;                             // (never past the contig's own stretch of the output)
    out[at + i] = (mem.vertex & 1) ? comp[src[n - 1 - i]] : src[i];
  }
}

hipError_t graph_reserve(GraphState& g, int64_t extra, hipStream_t st) {
  const size_t need = (size_t)(g.n_recs + extra);
  if (g.d_recs.p && need <= g.d_recs.cap) return hipSuccess;
  DeviceArray<pw_graph_overlap> grown;
  GR_TRY(grown.ensure(need > 2 * g.d_recs.cap ? need : 2 * g.d_recs.cap));
  if (g.n_recs) GR_TRY(hipMemcpyAsync(grown.p, g.d_recs.p, grown.bytes((size_t)g.n_recs), hipMemcpyDeviceToDevice, st));
  g.d_recs = std::move(grown);                            // (the old block goes with `grown`: hipFree waits for the copy)
  return hipSuccess;
}

hipError_t launch_graph_from_batch(GraphState& g, const Result* results, const void* summaries, int n, hipStream_t st) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_graph_from_batch, rows_grid((uint64_t)n), kBlock256, 0, st, results, (const pw_tx_summary*)summaries, g.d_stage.cp(), n,
                     g.d_recs.p + g.n_recs);
  return hipGetLastError();
}

namespace {

hipError_t exclusive_sums(GraphState& g, const uint64_t* in, uint64_t* out, size_t n, hipStream_t st) {
  return rocprim_run(g.tmp, [&](void* t, size_t& b) {
    return rocprim::exclusive_scan(t, b, in, out, (uint64_t)0, n, rocprim::plus<uint64_t>(), st);
  });
}

// the doubling over the chain predecessors, the cut links left out; the final state is in d_chain[*cur]
hipError_t chain_ranks(GraphState& g, int rounds, int* cur, hipStream_t st) {
  const int V = (int)g.V;
  const dim3 grid = rows_grid((uint64_t)V);
  hipLaunchKernelGGL(k_graph_chain_init, grid, kBlock256, 0, st, g.d_pred.cp(), g.d_adv.cp(), g.d_cut.cp(), V, g.d_chain[0].p);
  GR_TRY(hipGetLastError());
  int c = 0;
  for (int r = 0; r < rounds; r++, c ^= 1) {
    hipLaunchKernelGGL(k_graph_double, grid, kBlock256, 0, st, g.d_chain[c].cp(), g.d_chain[c ^ 1].p, V);
    GR_TRY(hipGetLastError());
  }
  *cur = c;
  return hipSuccess;
}

}  // namespace

namespace {

// The UNITIGS decomposition over the live vertices, up to what every chain's tail hands its head: out / one, the chain
// links (with PW_ARC_CHAIN when mark is set), ranks by doubling, the cycles cut at their smallest vertex, the ranks redone,
// hcnt / hmin / hlen.  The final doubling state is in d_chain[*cur].
hipError_t graph_chains(GraphState& g, int mark, int* cur, hipStream_t st) {
  const int V = (int)g.V;
  const size_t nV = (size_t)V;
  const dim3 vgrid = rows_grid((uint64_t)V);
  hipLaunchKernelGGL(k_graph_out, vgrid, kBlock256, 0, st, g.d_arcs.cp(), (const long long*)g.d_rows.cp(), V, g.d_out.p, g.d_one.p);
  GR_TRY(hipGetLastError());
  GR_TRY(hipMemsetAsync(g.d_pred.p, 0xff, g.d_pred.bytes(nV), st));
  GR_TRY(hipMemsetAsync(g.d_cut.p, 0, nV, st));
  hipLaunchKernelGGL(k_graph_chain, vgrid, kBlock256, 0, st, g.d_arcs.p, g.d_out.cp(), g.d_one.cp(), V, mark, g.d_succ.p, g.d_pred.p, g.d_adv.p);
  GR_TRY(hipGetLastError());
  int rounds = 1;                                         // ceil(log2(V)) + 1: fixed from the number of vertices alone
  while (((int64_t)1 << (rounds - 1)) < V) rounds++;
  GR_TRY(chain_ranks(g, rounds, cur, st));
  hipLaunchKernelGGL(k_graph_cut, vgrid, kBlock256, 0, st, g.d_chain[*cur].cp(), V, g.d_cut.p);
  GR_TRY(hipGetLastError());
  GR_TRY(chain_ranks(g, rounds, cur, st));
  hipLaunchKernelGGL(k_graph_tails, vgrid, kBlock256, 0, st, g.d_chain[*cur].cp(), g.d_succ.cp(), g.d_adv.cp(), g.d_cut.cp(), g.d_contained.cp(),
                     g.d_dropped.cp(), g.d_lens.cp(), V, g.d_hcnt.p, g.d_hmin.p, g.d_hlen.as<unsigned long long>());
  return hipGetLastError();
}

}  // namespace

hipError_t graph_build(GraphState& g, const pw_graph_params& p, const pw_graph_clean_params& clean, hipStream_t st) {
  const int64_t n = g.n_recs, V = g.V;
  const size_t nV = (size_t)V;
  g.built = false; g.has_contigs = false;
  // ---- classification, contained flags, the arc count ----
  const size_t scan_n = (size_t)(n > V ? n : V) + 1;
  GR_TRY(g.d_contained.ensure((size_t)g.n_reads));
  GR_TRY(g.d_dropped.ensure((size_t)g.n_reads));
  GR_TRY(g.d_cnt.ensure(scan_n));
  GR_TRY(g.d_off.ensure(scan_n));
  if (g.n_reads) GR_TRY(hipMemsetAsync(g.d_contained.p, 0, (size_t)g.n_reads, st));
  if (g.n_reads) GR_TRY(hipMemsetAsync(g.d_dropped.p, 0, (size_t)g.n_reads, st));
  GR_TRY(hipMemsetAsync(g.d_cnt.p + n, 0, 8, st));
  if (n) {
    hipLaunchKernelGGL(k_graph_classify, rows_grid((uint64_t)n), kBlock256, 0, st, g.d_recs.p, (long long)n, g.d_lens.cp(), p, g.d_contained.p);
    GR_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_graph_arc_count, rows_grid((uint64_t)n), kBlock256, 0, st, g.d_recs.cp(), (long long)n, g.d_contained.cp(),
                       g.d_cnt.as<unsigned long long>());
    GR_TRY(hipGetLastError());
  }
  GR_TRY(exclusive_sums(g, g.d_cnt.cp(), g.d_off.p, (size_t)n + 1, st));
  uint64_t givers = 0;                                    // the arc table is allocated from the counted total
  GR_TRY(hipMemcpyAsync(&givers, g.d_off.p + n, 8, hipMemcpyDeviceToHost, st));
  GR_TRY(hipStreamSynchronize(st));
  const int64_t A = 2 * (int64_t)givers;
  const size_t nA = (size_t)A;
  // ---- arcs, the stable sort on (v, len), the row index, the sort by target ----
  GR_TRY(g.d_gen.ensure(nA)); GR_TRY(g.d_arcs.ensure(nA));
  GR_TRY(g.d_keys.ensure(nA)); GR_TRY(g.d_keys_s.ensure(nA));
  GR_TRY(g.d_idx.ensure(nA)); GR_TRY(g.d_idx_s.ensure(nA)); GR_TRY(g.d_pos.ensure(nA)); GR_TRY(g.d_tarc.ensure(nA));
  GR_TRY(g.d_rows.ensure(nV + 1));
  const int vbits = 32 + bits_for((uint64_t)(V > 0 ? V - 1 : 0));
  if (A) {
    hipLaunchKernelGGL(k_graph_arcs, rows_grid((uint64_t)n), kBlock256, 0, st, g.d_recs.cp(), (long long)n, g.d_lens.cp(),
                       g.d_cnt.as<const unsigned long long>(), g.d_off.as<const unsigned long long>(), (long long)A, g.d_gen.p,
                       g.d_keys.as<unsigned long long>(), g.d_idx.p);
    GR_TRY(hipGetLastError());
    GR_TRY(rocprim_run(g.tmp, [&](void* t, size_t& b) {
      return rocprim::radix_sort_pairs(t, b, g.d_keys.cp(), g.d_keys_s.p, g.d_idx.cp(), g.d_idx_s.p, nA, 0u, (unsigned)vbits, st);
    }));
    hipLaunchKernelGGL(k_graph_gather, rows_grid((uint64_t)A), kBlock256, 0, st, g.d_gen.cp(), g.d_idx_s.cp(), (long long)A, g.d_arcs.p, g.d_pos.p,
                       g.d_keys.as<unsigned long long>(), g.d_idx.p);
    GR_TRY(hipGetLastError());
    const auto needles = rocprim::make_transform_iterator(rocprim::make_counting_iterator<uint64_t>(0), RowKey());
    GR_TRY(rocprim_run(g.tmp, [&](void* t, size_t& b) {
      return rocprim::lower_bound(t, b, g.d_keys_s.cp(), needles, g.d_rows.p, nA, nV + 1, rocprim::less<uint64_t>(), st);
    }));
    GR_TRY(rocprim_run(g.tmp, [&](void* t, size_t& b) {
      return rocprim::radix_sort_pairs(t, b, g.d_keys.cp(), g.d_keys_s.p, g.d_idx.cp(), g.d_tarc.p, nA, 0u, (unsigned)vbits, st);
    }));
  } else {
    GR_TRY(hipMemsetAsync(g.d_rows.p, 0, g.d_rows.bytes(nV + 1), st));
  }
  // ---- reduction, twins, chain links ----
  GR_TRY(g.d_out.ensure(nV)); GR_TRY(g.d_one.ensure(nV)); GR_TRY(g.d_succ.ensure(nV)); GR_TRY(g.d_pred.ensure(nV)); GR_TRY(g.d_adv.ensure(nV));
  GR_TRY(g.d_cut.ensure(nV)); GR_TRY(g.d_chain[0].ensure(nV)); GR_TRY(g.d_chain[1].ensure(nV));
  GR_TRY(g.d_hcnt.ensure(nV)); GR_TRY(g.d_hmin.ensure(nV)); GR_TRY(g.d_hlen.ensure(nV));
  GR_TRY(g.d_mcnt.ensure(nV + 1)); GR_TRY(g.d_moff.ensure(nV + 1));
  uint64_t n_unitigs = 0, n_members = 0;
  if (V) {
    const dim3 vgrid = rows_grid((uint64_t)V);
    if (A) {
      if (!g.ev_reduce0.e) { GR_TRY(g.ev_reduce0.create()); GR_TRY(g.ev_reduce1.create()); }
      GR_TRY(hipEventRecord(g.ev_reduce0.e, st));
      hipLaunchKernelGGL(k_graph_reduce, dim3((unsigned)V), dim3(64), 0, st, g.d_arcs.p, (const long long*)g.d_rows.cp(),
                         g.d_keys_s.as<const unsigned long long>(), g.d_tarc.cp(), (int)V, (int)p.fuzz);
      GR_TRY(hipGetLastError());
      GR_TRY(hipEventRecord(g.ev_reduce1.e, st));
      hipLaunchKernelGGL(k_graph_twins, rows_grid((uint64_t)A), kBlock256, 0, st, g.d_arcs.p, g.d_idx_s.cp(), g.d_pos.cp(), (long long)A);
      GR_TRY(hipGetLastError());
    }
    // ---- cleaning: a fixed number of rounds, each on a decomposition of its own that marks no chain link ----
    int cur = 0;
    const int clean_rounds = (clean.max_tip_reads > 0 || clean.max_bubble_reads > 0) && A ? clean.rounds : 0;
    for (int r = 0; r < clean_rounds; r++) {
      GR_TRY(graph_chains(g, 0, &cur, st));
      GR_TRY(clean_round(g, cur, A, clean, st));
    }
    // ---- unitigs: ranks by doubling, the cycles cut at their smallest vertex, the ranks redone ----
    GR_TRY(graph_chains(g, 1, &cur, st));
    GR_TRY(hipMemsetAsync(g.d_cnt.p + V, 0, 8, st));
    GR_TRY(hipMemsetAsync(g.d_mcnt.p + V, 0, 8, st));
    hipLaunchKernelGGL(k_graph_heads, vgrid, kBlock256, 0, st, g.d_chain[cur].cp(), g.d_contained.cp(), g.d_dropped.cp(), g.d_hcnt.cp(), g.d_hmin.cp(), (int)V,
                       g.d_cnt.as<unsigned long long>(), g.d_mcnt.as<unsigned long long>());
    GR_TRY(hipGetLastError());
    GR_TRY(exclusive_sums(g, g.d_cnt.cp(), g.d_off.p, nV + 1, st));
    GR_TRY(exclusive_sums(g, g.d_mcnt.cp(), g.d_moff.p, nV + 1, st));
    GR_TRY(hipMemcpyAsync(&n_unitigs, g.d_off.p + V, 8, hipMemcpyDeviceToHost, st));
    GR_TRY(hipMemcpyAsync(&n_members, g.d_moff.p + V, 8, hipMemcpyDeviceToHost, st));
    GR_TRY(hipStreamSynchronize(st));                     // the unitig and member tables are allocated from the counted totals
    GR_TRY(g.d_unitigs.ensure((size_t)n_unitigs)); GR_TRY(g.d_members.ensure((size_t)n_members)); GR_TRY(g.d_mem_uid.ensure((size_t)n_members));
    hipLaunchKernelGGL(k_graph_emit, vgrid, kBlock256, 0, st, g.d_chain[cur].cp(), g.d_cnt.as<const unsigned long long>(),
                       g.d_off.as<const unsigned long long>(), g.d_moff.as<const unsigned long long>(), g.d_succ.cp(), g.d_adv.cp(), g.d_cut.cp(),
                       g.d_lens.cp(), g.d_hcnt.cp(), g.d_hlen.as<const unsigned long long>(), (int)V, (long long)n_unitigs, (long long)n_members,
                       g.d_unitigs.p, g.d_members.p, g.d_mem_uid.p);
    GR_TRY(hipGetLastError());
  } else {
    GR_TRY(g.d_unitigs.ensure(0)); GR_TRY(g.d_members.ensure(0)); GR_TRY(g.d_mem_uid.ensure(0));
  }
  GR_TRY(hipStreamSynchronize(st));
  g.reduce_ms = -1;
  if (A && V) {
    float ms = 0;
    GR_TRY(hipEventElapsedTime(&ms, g.ev_reduce0.e, g.ev_reduce1.e));
    g.reduce_ms = ms;
  }
  g.n_arcs = A; g.n_unitigs = (int64_t)n_unitigs; g.n_members = (int64_t)n_members; g.built = true;
  return hipSuccess;
}

// d_roff and d_comp are uploaded by the caller.  Count, scan, wait, allocate, write.
hipError_t graph_contigs(GraphState& g, const uint8_t* letters, hipStream_t st) {
  const int64_t U = g.n_unitigs;
  g.has_contigs = false;
  GR_TRY(g.d_cnt.ensure((size_t)U + 1 > g.d_cnt.cap ? (size_t)U + 1 : g.d_cnt.cap));
  GR_TRY(g.d_coff.ensure((size_t)U + 1));
  GR_TRY(hipMemsetAsync(g.d_cnt.p + U, 0, 8, st));
  if (U) {
    hipLaunchKernelGGL(k_graph_contig_count, rows_grid((uint64_t)U), kBlock256, 0, st, g.d_unitigs.cp(), (long long)U, g.d_cnt.as<unsigned long long>());
    GR_TRY(hipGetLastError());
  }
  GR_TRY(exclusive_sums(g, g.d_cnt.cp(), g.d_coff.p, (size_t)U + 1, st));
  uint64_t total = 0;
  GR_TRY(hipMemcpyAsync(&total, g.d_coff.p + U, 8, hipMemcpyDeviceToHost, st));
  GR_TRY(hipStreamSynchronize(st));
  GR_TRY(g.d_cletters.ensure((size_t)total));
  if (g.n_members) {
    hipLaunchKernelGGL(k_graph_contig_write, dim3((unsigned)g.n_members), dim3(64), 0, st, g.d_members.cp(), g.d_mem_uid.cp(),
                       g.d_coff.as<const unsigned long long>(), letters, (const long long*)g.d_roff.cp(), g.d_lens.cp(), g.d_comp.cp(), g.d_cletters.p);
    GR_TRY(hipGetLastError());
  }
  GR_TRY(hipStreamSynchronize(st));
  g.contig_total = (int64_t)total; g.has_contigs = true;
  return hipSuccess;
}

int64_t graph_device_bytes(const GraphState& g) {
  size_t b = g.tmp.cap;
  auto add = [&b](const auto& a) { if (a.p) b += a.bytes(a.cap); };
  add(g.d_lens); add(g.d_recs); add(g.d_stage); add(g.d_contained); add(g.d_cnt); add(g.d_off); add(g.d_mcnt); add(g.d_moff);
  add(g.d_gen); add(g.d_arcs); add(g.d_keys); add(g.d_keys_s); add(g.d_idx); add(g.d_idx_s); add(g.d_pos); add(g.d_tarc);
  add(g.d_rows); add(g.d_out); add(g.d_one); add(g.d_succ); add(g.d_pred); add(g.d_adv); add(g.d_cut); add(g.d_chain[0]); add(g.d_chain[1]);
  add(g.d_hcnt); add(g.d_hmin); add(g.d_hlen); add(g.d_dropped); add(g.d_cflag); add(g.d_cdrop); add(g.d_ctail); add(g.d_cs); add(g.d_cz); add(g.d_unitigs); add(g.d_members); add(g.d_mem_uid); add(g.d_roff); add(g.d_comp);
  add(g.d_coff); add(g.d_cletters);
  return (int64_t)b;
}

}  // namespace pw

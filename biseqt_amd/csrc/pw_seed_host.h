// pw_seed_host.h -- host code shared by the pairwise seed index (pw_seeds.hip), the N-way one (pw_mseeds.hip) and the
// query-batched one (pw_qseeds.hip), around the kernels of pw_seed_kernels.h: the word space L^k and its sort key, encode +
// sort of one sequence's k-mers, the direct-address table decision, the row-limit refusal, event timing, and the
// neighbourhood graph from its sorted points on -- CSR tail, read-backs, connected components.  Everything lives in an
// anonymous namespace and reports through `sink`, as PW_HIP_CHECK does: each translation unit keeps its own thread_local
// error channel.  The functions that take a handle `x` read its `device` and its SeedGraph `g` (the components its two
// events as well).  Device memory is typed (DeviceArray<T>, pw_hip_host.h); only the k-mer keys, 4 or 8 bytes wide by
// WordSpace::key32, and rocPRIM's scratch are DeviceBuffers: the function templates on the key type K name the type at the use.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <algorithm>
#include <functional>
#include <string>
#include <rocprim/rocprim.hpp>

#include "pw_hip_host.h"
#include "pw_seed_kernels.h"

namespace {

using ErrSink = void (*)(const std::string&);

// Between two recorded events: the milliseconds from ev0 to `stream`'s present end, which this waits for.
int elapsed(ErrSink sink, const DeviceEvent& ev0, const DeviceEvent& ev1, hipStream_t stream, float* ms) {
  PW_HIP_CHECK(sink, hipEventRecord(ev1.e, stream));
  PW_HIP_CHECK(sink, hipEventSynchronize(ev1.e));
  PW_HIP_CHECK(sink, hipEventElapsedTime(ms, ev0.e, ev1.e));
  PW_HIP_CHECK(sink, hipGetLastError());
  return 0;
}

// ---- the word space ---------------------------------------------------------------------------------------
// kinv = L^k, one past the largest k-mer (and the masked key of K5a); bits = the sort width; key32: L^k fits 32 bits, 4-byte
// keys.
struct WordSpace { int L = 0, k = 0, bits = 0; bool key32 = false; uint64_t kinv = 0; };

// The two range checks every create makes first ...
int check_word(ErrSink sink, int alphabet_len, int wordlen) {
  if (alphabet_len < 1 || alphabet_len > 36) { sink("alphabet_len must be 1..36 (kmers.py:266)"); return -1; }
  if (wordlen < 1 || wordlen > 31) { sink("wordlen must be 1..31 (kmers.py:269)"); return -1; }
  return 0;
}
// ... and, behind whatever its caller checks in between, the one that L^k fits: the masked key is L^k itself.  Sort width:
// the largest key that occurs -- L^k - 1, or L^k when mask sets are given (`masked`; for DNA words without masks that is
// 2k bits: k = 12 sorts in three 8-bit passes instead of four).
int word_space(ErrSink sink, int alphabet_len, int wordlen, bool masked, WordSpace* ws) {
  long double lk = 1; for (int i = 0; i < wordlen; i++) lk *= alphabet_len;
  if (lk >= (long double)(1ull << 62)) { sink("alphabet_len ^ wordlen must be below 2^62"); return -1; }
  ws->L = alphabet_len; ws->k = wordlen;
  ws->kinv = 1; for (int i = 0; i < wordlen; i++) ws->kinv *= (uint64_t)alphabet_len;
  ws->bits = bits_for(masked ? ws->kinv : (ws->kinv > 1 ? ws->kinv - 1 : 1));
  ws->key32 = ws->kinv < 0xffffffffull;
  return 0;
}

// ---- row totals -------------------------------------------------------------------------------------------
struct SatAdd {
  __host__ __device__ uint64_t operator()(uint64_t a, uint64_t b) const { const uint64_t s = a + b; return s < a ? ~0ull : s; }
};
// -1 and the refusal when the table would hold more than max_rows rows; `total` may have saturated (SatAdd) at 2^64 - 1
int check_row_limit(ErrSink sink, unsigned long long total, int64_t max_rows) {
  if (total <= (unsigned long long)max_rows) return 0;
  char msg[200];
  if (total == ~0ull)
    snprintf(msg, sizeof msg, "the seeds table would hold at least 2^64 - 1 rows (limit %lld): raise the word length", (long long)max_rows);
  else
    snprintf(msg, sizeof msg, "the seeds table would hold %llu rows (limit %lld): raise max_rows or the word length", total, (long long)max_rows);
  sink(msg);
  return -1;
}

// ---- K5a + sort -------------------------------------------------------------------------------------------
// (k-mer, position) of seq[0, n), nk = n - k + 1 of them, sorted by k-mer into keys_out / pos_out from element `at` on -- a
// stable LSD radix sort, so positions stay ascending inside a k-mer.  The outputs grow to hold at + nk elements (at least
// one), the caller's staging buffers to nk: a caller that fills one buffer piece by piece sizes all of them first.
template <typename K>
int encode_sort(ErrSink sink, const WordSpace& ws, const MaskSets& ms, const uint8_t* seq, int64_t n, int64_t nk,
                DeviceBuffer& keys_in, DeviceArray<uint32_t>& pos_in, DeviceBuffer& tmp, DeviceBuffer& keys_out,
                DeviceArray<uint32_t>& pos_out, int64_t at, hipStream_t st) {
  const size_t nout = (size_t)std::max<int64_t>(at + std::max<int64_t>(nk, 0), 1);
  PW_HIP_CHECK(sink, keys_out.ensure(nout * sizeof(K))); PW_HIP_CHECK(sink, pos_out.ensure(nout));
  if (nk <= 0) return 0;
  PW_HIP_CHECK(sink, keys_in.ensure((size_t)nk * sizeof(K))); PW_HIP_CHECK(sink, pos_in.ensure((size_t)nk));
  hipLaunchKernelGGL((k_encode<K>), rows_grid((uint64_t)nk), kBlock256, 0, st, seq, n, ws.k, ws.L, ws.kinv, ms, keys_in.as<K>(), pos_in.p);
  PW_HIP_CHECK(sink, rocprim_run(tmp, [&](void* t, size_t& b) {
    return rocprim::radix_sort_pairs(t, b, keys_in.as<const K>(), keys_out.as<K>() + at, pos_in.cp(), pos_out.p + at, (size_t)nk, 0u,
                                     (unsigned)ws.bits, st);
  }));
  return 0;
}

// ---- K5b's direct-address table ---------------------------------------------------------------------------
// The table pays when the key space is small and dense enough: at most 2^26 keys (256 MB of table) and on average no more
// than 64 keys between two consecutive elements of `other` (k_table_fill walks those gaps serially).
bool table_pays(const WordSpace& ws, int64_t n_other) {
  return ws.key32 && n_other > 0 && ws.kinv <= (1ull << 26) && ws.kinv / (uint64_t)n_other <= 64;
}
template <typename K>
int table_fill(ErrSink sink, const WordSpace& ws, const K* other, int64_t n_other, DeviceArray<uint32_t>& tab, hipStream_t st) {
  PW_HIP_CHECK(sink, tab.ensure((size_t)(ws.kinv + 2)));
  hipLaunchKernelGGL((k_table_fill<K>), rows_grid((uint64_t)n_other + 1), kBlock256, 0, st, other, n_other, ws.kinv, tab.p);
  return 0;
}

// ---- the neighbourhood graph (K7, K9e, K10d) from its sorted points on --------------------------------------
// keys / order: the points' sort keys, sorted, and the point each belongs to; cnt / off / adj: CSR (off 64-bit, n + 1
// entries).  npts / edges: -1 until a graph_build has succeeded.
struct SeedGraph { DeviceArray<uint64_t> keys, off; DeviceArray<uint32_t> order, cnt, adj; int64_t npts = -1, edges = -1; };

std::string before_graph_build(const char* entry) {      // entry = "<api>_graph_<what>"
  const std::string s(entry);
  return s + " before a successful " + s.substr(0, s.find("_graph_")) + "_graph_build";
}

// The caller's n keys `kin` (values `vin`: the point numbers) sorted over `bits` bits into g.keys / g.order; the count
// pass that follows writes g.cnt.  All on the null stream, as everything of the graph.
int graph_sort(ErrSink sink, SeedGraph& g, DeviceBuffer& tmp, const DeviceArray<uint64_t>& kin, const DeviceArray<uint32_t>& vin, int64_t n,
               int bits) {
  PW_HIP_CHECK(sink, g.keys.ensure((size_t)n)); PW_HIP_CHECK(sink, g.order.ensure((size_t)n));
  PW_HIP_CHECK(sink, g.cnt.ensure((size_t)n)); PW_HIP_CHECK(sink, g.off.ensure((size_t)n + 1));
  PW_HIP_CHECK(sink, rocprim_run(tmp, [&](void* t, size_t& b) {
    return rocprim::radix_sort_pairs(t, b, kin.cp(), g.keys.p, vin.cp(), g.order.p, (size_t)n, 0u, (unsigned)bits,
                                     (hipStream_t) nullptr);
  }));
  return 0;
}

// Behind the caller's count pass: offsets = exclusive scan of the counts, widened to 64 bits in `wide` (n x 8 bytes of the
// caller's), one 8-byte read-back of the total, off[n], adj sized, then fill_pass() -- the caller's FILL = true launch, 0 or
// -1 -- when there is an edge at all.  Returns the number of edges, which the caller records once its own synchronisation
// has succeeded, or -1.  (Not a template on the callable: as an ordinary function it leaves the order in which a translation
// unit's kernels are emitted, and so their fingerprints, as they were.)
int64_t graph_finish(ErrSink sink, SeedGraph& g, DeviceBuffer& tmp, DeviceArray<unsigned long long>& scalar, uint64_t* wide, int64_t n,
                     const std::function<int()>& fill_pass) {
  hipLaunchKernelGGL(k_widen, rows_grid((uint64_t)n), kBlock256, 0, nullptr, g.cnt.p, n, wide);
  PW_HIP_CHECK(sink, rocprim_run(tmp, [&](void* t, size_t& b) {
    return rocprim::exclusive_scan(t, b, (const uint64_t*)wide, g.off.p, (uint64_t)0, (size_t)n, rocprim::plus<uint64_t>(), (hipStream_t) nullptr);
  }));
  hipLaunchKernelGGL(k_total, dim3(1), dim3(64), 0, nullptr, g.off.p, wide, n, scalar.p);
  unsigned long long total = 0;
  PW_HIP_CHECK(sink, hipMemcpy(&total, scalar.p, sizeof total, hipMemcpyDeviceToHost));
  if (total >= (1ull << 32)) { sink("the neighbourhood graph has more than 2^32 edges: use a smaller radius"); return -1; }
  PW_HIP_CHECK(sink, hipMemcpy(g.off.p + n, &total, sizeof total, hipMemcpyHostToDevice));
  PW_HIP_CHECK(sink, g.adj.ensure((size_t)std::max<unsigned long long>(total, 1)));
  if (total && fill_pass() != 0) return -1;
  return (int64_t)total;
}

template <typename X>
int graph_counts_to_host(ErrSink sink, const char* entry, const X* x, int32_t* counts, int64_t cap) {
  if (!x || x->g.edges < 0) { sink(before_graph_build(entry)); return -1; }
  if (cap < x->g.npts) { sink(std::string(entry) + ": capacity too small"); return -1; }
  PW_HIP_CHECK(sink, hipSetDevice(x->device));
  if (x->g.npts) PW_HIP_CHECK(sink, hipMemcpy(counts, x->g.cnt.p, x->g.cnt.bytes((size_t)x->g.npts), hipMemcpyDeviceToHost));
  return 0;
}

template <typename X>
int graph_fetch_to_host(ErrSink sink, const char* entry, const X* x, int64_t* offsets, int32_t* neighbours) {
  if (!x || x->g.edges < 0) { sink(before_graph_build(entry)); return -1; }
  PW_HIP_CHECK(sink, hipSetDevice(x->device));
  if (x->g.npts == 0) { offsets[0] = 0; return 0; }
  PW_HIP_CHECK(sink, hipMemcpy(offsets, x->g.off.p, x->g.off.bytes((size_t)x->g.npts + 1), hipMemcpyDeviceToHost));
  if (x->g.edges) PW_HIP_CHECK(sink, hipMemcpy(neighbours, x->g.adj.p, x->g.adj.bytes((size_t)x->g.edges), hipMemcpyDeviceToHost));
  return 0;
}

// Connected components of the available points: labels[v] = the smallest point of v's component, -1 where avail[v] is 0.
// ms: where the device time goes (between the handle's two events), rounds: where the number of hook rounds goes; either
// may be null.
template <typename X>
int graph_components(ErrSink sink, const char* entry, const X* x, const uint8_t* avail, int32_t* labels, float* ms, int* rounds) {
  if (!x || x->g.edges < 0) { sink(before_graph_build(entry)); return -1; }
  const SeedGraph& g = x->g;
  const int64_t n = g.npts;
  if (rounds) *rounds = 0;
  if (n == 0) return 0;
  PW_HIP_CHECK(sink, hipSetDevice(x->device));
  DeviceArray<uint8_t> av; DeviceArray<int> par, flag;
  if (upload(sink, av, avail, (size_t)n) != 0) return -1;
  PW_HIP_CHECK(sink, par.ensure((size_t)n)); PW_HIP_CHECK(sink, flag.ensure(1));
  if (ms) PW_HIP_CHECK(sink, hipEventRecord(x->ev0.e, nullptr));
  const dim3 grid = rows_grid((uint64_t)n), blk = kBlock256;
  hipLaunchKernelGGL(k_cc_init, grid, blk, 0, nullptr, av.p, n, par.p);
  for (int it = 0; it < 10000; it++) {            // every round at least halves the number of roots still to merge
    PW_HIP_CHECK(sink, hipMemsetAsync(flag.p, 0, flag.bytes(1), nullptr));
    hipLaunchKernelGGL(k_cc_hook, grid, blk, 0, nullptr, g.off.p, g.cnt.p, g.adj.p, n, par.p, flag.p);
    hipLaunchKernelGGL(k_cc_compress, grid, blk, 0, nullptr, n, par.p);
    int changed = 0;
    PW_HIP_CHECK(sink, hipMemcpy(&changed, flag.p, sizeof changed, hipMemcpyDeviceToHost));
    if (rounds) *rounds = it + 1;
    if (!changed) break;
  }
  if (ms && elapsed(sink, x->ev0, x->ev1, nullptr, ms) != 0) return -1;
  PW_HIP_CHECK(sink, hipMemcpy(labels, par.p, par.bytes((size_t)n), hipMemcpyDeviceToHost));
  return 0;
}

}  // namespace

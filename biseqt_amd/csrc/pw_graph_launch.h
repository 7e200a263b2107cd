// pw_graph_launch.h -- what pwlib_api.cpp (the C surface of include/pw_graph.h: validation, the error channel, the host
// copies) sees of pw_graph.hip (K17: the kernels, rocPRIM's sort, scans and row index, and the stage sequences that count,
// wait, allocate and write).  GraphState owns every device array of a graph; the stage functions return a HIP error.
#ifndef PW_GRAPH_LAUNCH_H
#define PW_GRAPH_LAUNCH_H

#include <hip/hip_runtime_api.h>
#include <stdint.h>

#include "../../include/pw_graph.h"
#include "pw_hip_host.h"
#include "pw_types.h"

namespace pw {

// One vertex of the pointer doubling (k_graph_double): after a round, nxt is the ancestor 2^round links up the chain, or
// -1 once the head is passed; hd the farthest ancestor reached (the head, once nxt is -1); d the links and o the advances
// between the vertex and hd; m the smallest vertex from the vertex up to hd.  (Unsigned sums: on a cycle they wrap, and
// are thrown away.)
struct GraphChain {
  uint64_t o;
  int32_t nxt, hd;
  uint32_t d;
  int32_t m;
};                                       // 24 bytes

struct GraphState {
  int device = 0;
  int64_t n_reads = 0, V = 0;
  DeviceArray<int32_t> d_lens;           // [n_reads]
  DeviceArray<pw_graph_overlap> d_recs;  // [n_recs]; grows by doubling, the old records copied over
  int64_t n_recs = 0;
  DeviceArray<int32_t> d_stage;          // pw_batch_graph_add: [3][n] read a, read b, strand of the batch's pairs
  // ---- the last build ----
  bool built = false;
  int64_t n_arcs = 0, n_unitigs = 0, n_members = 0;
  DeviceEvent ev_reduce0, ev_reduce1;    // around k_graph_reduce; created by the first build that has arcs
  double reduce_ms = -1;
  DeviceArray<uint8_t> d_contained;      // [n_reads]
  DeviceArray<uint64_t> d_cnt, d_off;    // [max(n_recs, V) + 1]: a scan's input and output (arc-giving records; heads)
  DeviceArray<uint64_t> d_mcnt, d_moff;  // [V + 1]: members per kept head and their exclusive sums
  DeviceArray<pw_graph_arc> d_gen, d_arcs;               // [n_arcs]: in generation order / sorted
  DeviceArray<uint64_t> d_keys, d_keys_s;                // [n_arcs]: v << 32 | len, then v << 32 | w; in and out of the sorts
  DeviceArray<uint32_t> d_idx, d_idx_s, d_pos, d_tarc;   // [n_arcs]: generation position (in, sorted), its inverse, arcs by target
  DeviceArray<int64_t> d_rows;           // [V + 1]
  DeviceArray<uint32_t> d_out;           // [V]: kept arcs leaving v
  DeviceArray<int32_t> d_one, d_succ, d_pred, d_adv;     // [V]: a kept arc of v (the one, when out == 1); chain links; len of v's link
  DeviceArray<uint8_t> d_cut;            // [V]: the link entering v is cut (v heads a cycle)
  DeviceArray<GraphChain> d_chain[2];    // [V]: ping-pong
  DeviceArray<int32_t> d_hcnt, d_hmin;   // [V]: per head, written by its tail: members, smallest vertex
  DeviceArray<uint64_t> d_hlen;          // [V]: ... and the unitig's length
  // ---- cleaning (K19, pw_clean.hip); d_dropped is all zero after a build without it, the rest is allocated by the first round ----
  DeviceArray<uint8_t> d_dropped;        // [n_reads]: 0, 1 (tip), 2 (bubble)
  DeviceArray<uint8_t> d_cflag;          // [V]: per head: 1 tip candidate, 2 bubble candidate
  DeviceArray<uint8_t> d_cdrop;          // [V]: per head: the component is dropped as a tip (1) or as a bubble (2)
  DeviceArray<int32_t> d_ctail, d_cs, d_cz;              // [V]: per head: the tail; of a bubble candidate the source s and the sink z
  DeviceArray<pw_unitig> d_unitigs;      // [n_unitigs]
  DeviceArray<pw_unitig_member> d_members;               // [n_members]
  DeviceArray<int32_t> d_mem_uid;        // [n_members]: the member's unitig
  // ---- the last pw_graph_contigs ----
  bool has_contigs = false;
  int64_t contig_total = 0;
  DeviceArray<int64_t> d_roff;           // [n_reads]
  DeviceArray<uint8_t> d_comp;           // [256]: the complement table padded with the identity
  DeviceArray<uint64_t> d_coff;          // [n_unitigs + 1]
  DeviceArray<uint8_t> d_cletters;       // [contig_total]
  DeviceBuffer tmp;                      // rocPRIM's scratch
};

// d_recs grown to hold `extra` more records, the first n_recs kept (a device copy on `st` when the array moves)
hipError_t graph_reserve(GraphState& g, int64_t extra, hipStream_t st);
// records [n_recs, n_recs + n) from a batch (d_stage holds a, b, strand); summaries: pw_tx_summary[n] on the device
hipError_t launch_graph_from_batch(GraphState& g, const Result* results, const void* summaries, int n, hipStream_t st);
// c.rounds cleaning rounds between the twins and the unitigs; none when c.rounds == 0 or both maxima are 0
hipError_t graph_build(GraphState& g, const pw_graph_params& p, const pw_graph_clean_params& c, hipStream_t st);
// pw_clean.hip (K19): one cleaning round on the decomposition that graph_build left in d_out, d_one, d_succ, d_cut, d_hcnt,
// d_hmin and d_chain[cur]: candidates, tips, bubbles, d_dropped, and REMOVED | DROPPED on the n_arcs arcs.  Asynchronous on `st`.
hipError_t clean_round(GraphState& g, int cur, int64_t n_arcs, const pw_graph_clean_params& c, hipStream_t st);
hipError_t graph_contigs(GraphState& g, const uint8_t* letters, hipStream_t st);
int64_t graph_device_bytes(const GraphState& g);

}  // namespace pw
#endif

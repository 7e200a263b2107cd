// pw_consensus_launch.h -- what pwlib_api.cpp (the C surface of include/pw_consensus.h: validation, the error channel, the
// host copies) sees of pw_consensus.hip (K18: the kernels, rocPRIM's scans and the stage sequences that count, wait,
// allocate and write).  ConsState owns every device array of the consensus stage of one graph; the graph itself is
// reached through GraphState (pw_graph_launch.h) and only ever read.  The stage functions return a HIP error.
#ifndef PW_CONSENSUS_LAUNCH_H
#define PW_CONSENSUS_LAUNCH_H

#include <hip/hip_runtime_api.h>
#include <stdint.h>

#include "../../include/pw_consensus.h"
#include "pw_graph_launch.h"
#include "pw_hip_host.h"

namespace pw {

// One read of the pointer doubling (k_cons_double): the read in orientation rel begins at off in the forward frame of read
// f, d containment links up its chain; nxt is the read to look at next (f's parent chain), or -1 once f is no contained
// read.  (On a cycle the sums grow by at most 2^32 per link covered -- below 2^63 after the fixed rounds -- and are thrown
// away.)
struct ConsChain {
  int64_t off;
  int32_t f, nxt, rel, d;
};                                       // 24 bytes

struct ConsState {
  // ---- the last pw_graph_place ----
  bool placed = false;
  DeviceArray<uint64_t> d_best;          // [n_reads]: n_match << 32 | ~index of the parent record; 0 = none
  DeviceArray<ConsChain> d_chain[2];     // [n_reads]: ping-pong
  DeviceArray<int32_t> d_first;          // [n_reads]: the lowest member index of the read
  DeviceArray<pw_cons_place> d_place;    // [n_reads]
  // ---- the last pw_graph_consensus_layout ----
  bool has_layout = false;
  int64_t n_tasks = 0, n_cols = 0, arena_bytes = 0;
  DeviceArray<int64_t> d_roff;           // [n_reads]
  DeviceArray<uint8_t> d_comp;           // [256]: the complement table padded with the identity
  DeviceArray<uint64_t> d_ulen, d_cstart;                // [n_unitigs + 1]: padded contig lengths and their exclusive sums
  DeviceArray<uint64_t> d_tcnt, d_toff, d_msz, d_moff;   // [n_reads + 1]: tasks per read, frame bytes per read, their sums
  DeviceArray<uint32_t> d_flag;          // [1]: a contig of 2^31 letters or more was seen
  DeviceArray<pw_cons_task> d_tasks;     // [n_tasks]
  DeviceArray<uint8_t> d_arena;          // [arena_bytes + 16]
  DeviceBuffer tmp;                      // rocPRIM's scratch
};

hipError_t cons_place(const GraphState& g, ConsState& c, hipStream_t st);
// d_roff and d_comp are uploaded by the caller, the graph has its contig letters.  *too_long: a contig has 2^31 letters or
// more, and nothing was laid out.
hipError_t cons_layout(const GraphState& g, ConsState& c, const uint8_t* letters, int32_t slack, double drift, bool* too_long,
                       hipStream_t st);
// The two arena writers of cons_layout on their own (pw_rounds.hip lays the later rounds out with them): contig u of
// coff[u + 1] - coff[u] letters from cletters[coff[u] ..] at c.d_cstart[u] with 255 behind it, and the mutant frames of
// c.d_tasks from c.d_roff and c.d_comp.  c.d_arena is allocated and zeroed by the caller.
hipError_t cons_arena_contigs(ConsState& c, const uint8_t* cletters, const uint64_t* coff, int64_t n_unitigs, int64_t n_cols, hipStream_t st);
hipError_t cons_arena_mutants(const GraphState& g, ConsState& c, const uint8_t* letters, int64_t n_tasks, int64_t arena_bytes, hipStream_t st);
int64_t cons_device_bytes(const ConsState& c);

}  // namespace pw
#endif

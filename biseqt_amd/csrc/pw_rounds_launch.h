// pw_rounds_launch.h -- what pwlib_api.cpp (the C surface of include/pw_rounds.h: validation, the error channel, the host
// copies) sees of pw_rounds.hip (K20: the kernels, rocPRIM's scans and the stage sequences).  ColumnPolish owns the
// per-column arrays of one pileup's column polish, RoundState the positions and lengths of the current round of one graph;
// the graph's consensus arrays (ConsState, pw_consensus_launch.h) are rewritten by the relayout as the layout writes them.
#ifndef PW_ROUNDS_LAUNCH_H
#define PW_ROUNDS_LAUNCH_H

#include <hip/hip_runtime_api.h>
#include <stdint.h>

#include "../../include/pw_rounds.h"
#include "pw_consensus_launch.h"
#include "pw_hip_host.h"

namespace pw {

constexpr int kRoundChunk = 256;         // columns per workgroup of the column polish

// One workgroup of the column polish: columns [chunk * 256, chunk * 256 + 256) of read `read`.
struct RoundBlock { int32_t read, chunk; };

struct ColumnPolish {
  bool valid = false;                    // the last polish of the pileup was by columns
  DeviceArray<RoundBlock> d_blocks;      // [n_blocks]
  DeviceArray<uint8_t> d_e;              // [n_cols + 1]: letters per column, the last one 0
  DeviceArray<uint64_t> d_word;          // [n_cols]: a column's first eight letters, a byte each (columns in a read only)
  DeviceArray<uint8_t> d_ninth;          // [n_cols]: its ninth
  DeviceArray<uint64_t> d_colmap;        // [n_cols + 1]
};

struct RoundState {
  int round = 0;                         // 1 after a layout, + 1 per relayout
  bool have = false;                     // d_pos / d_len[cur] hold the current round's values
  int cur = 0;
  DeviceArray<int64_t> d_pos;            // [n_reads]
  DeviceArray<int64_t> d_len[2];         // [n_unitigs]: ping-pong
  DeviceArray<uint8_t> d_pol;            // the relayout's copy of the polished letters ...
  DeviceArray<uint64_t> d_poff;          // ... and of their n_unitigs + 1 offsets
};

// e, the kept letters and the zeroed statistics summed up; colmap = the exclusive sums of e; offsets from colmap.
hipError_t round_polish_count(ColumnPolish& cp, const uint32_t* counts, const uint32_t* ins, const uint8_t* letters, const int64_t* roff,
                              const int32_t* rlen, int64_t n_blocks, int64_t n_reads, int64_t n_cols, int L, int J, uint32_t min_depth,
                              uint64_t* offsets, pw_polish_stats* stats, DeviceBuffer& tmp, hipStream_t st);
hipError_t round_polish_write(const ColumnPolish& cp, const int64_t* roff, const int32_t* rlen, int64_t n_blocks, uint64_t total, uint8_t* out,
                              hipStream_t st);
// pos and lengths of round 1 from the placements and the unitigs, once per layout
hipError_t round_init(const GraphState& g, const ConsState& c, RoundState& r, hipStream_t st);
// *refused: 1 a contig of 2^31 letters or more, 2 the offsets disagree with colmap; nothing was laid out then.
hipError_t round_relayout(const GraphState& g, ConsState& c, RoundState& r, const uint8_t* polished, const uint64_t* poffs,
                          const uint64_t* colmap, const uint8_t* letters, int32_t slack, double drift, int* refused, hipStream_t st);
int64_t round_device_bytes(const RoundState& r);

}  // namespace pw
#endif

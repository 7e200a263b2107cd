// pw_cons_window.h -- the window of a placed read on its contig (include/pw_consensus.h, TASKS): the one definition that the
// layout of the first round (pw_consensus.hip, K18) and of the later rounds (pw_rounds.hip, K20) both compile.
#ifndef PW_CONS_WINDOW_H
#define PW_CONS_WINDOW_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/pw_consensus.h"

namespace pw {

// The window of a placed read of l letters on a contig of `length` letters; false: the read has no task.
__device__ __forceinline__ bool co_window(const pw_cons_place& p, int l, long long length, int slack, double drift, long long& lo,
                                          long long& hi, long long& radius) {
  if (p.unitig < 0 || l <= 0) return false;
  const long long pos = p.pos, end = pos + l;
  if (!((pos > 0 ? pos : 0) < (end < length ? end : length))) return false;
  radius = (long long)slack + (long long)((double)l * drift);
  lo = pos - radius; lo = (lo > 0 ? lo : 0) & ~3ll;
  hi = end + radius; hi = hi < length ? hi : length;
  return true;
}

}  // namespace pw
#endif

// pw_polish_column.h -- the POLISHING rule of include/pw_polish.h for one column, the one definition that the per-read polish
// (pw_polish.hip, K16) and the per-column polish (pw_rounds.hip, K20) both compile.
#ifndef PW_POLISH_COLUMN_H
#define PW_POLISH_COLUMN_H

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace pw {

// What one column emits (include/pw_polish.h, POLISHING): emit(letter) for each of its 0 .. 1 + J letters, in order;
// returns the statistics of the column as kept | substituted << 8 | deleted << 16 | inserted << 24.
template <typename Emit>
__device__ __forceinline__ uint32_t po_column(const uint32_t* __restrict__ row, const uint32_t* __restrict__ irow, int s, int L, int J,
                                              uint32_t min_depth, Emit&& emit) {
  unsigned long long depth = 0;
  uint32_t best = 0, call = 0;
  for (int ch = 0; ch <= L; ch++) {                     // letters, then DEL; a tie stays with the lower channel
    const uint32_t c = row[ch];
    depth += c;
    if (c > best) { best = c; call = (uint32_t)ch; }
  }
  if (depth < (unsigned long long)min_depth) { emit((uint8_t)s); return 1u; }
  uint32_t st;
  if (call == (uint32_t)L) st = 1u << 16;
  else { emit((uint8_t)call); st = call == (uint32_t)s ? 1u : 1u << 8; }
  for (int j = 0; j < J; j++) {
    unsigned long long nj = 0;
    uint32_t bj = 0, cj = 0;
    for (int y = 0; y < L; y++) {
      const uint32_t c = irow[j * L + y];
      nj += c;
      if (c > bj) { bj = c; cj = (uint32_t)y; }
    }
    if (!(2ull * nj > depth)) break;
    emit((uint8_t)cj);
    st += 1u << 24;
  }
  return st;
}

}  // namespace pw
#endif

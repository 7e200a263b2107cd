// pw_complement.h -- the complement table of a stranded call, shared by overlap band selection (pw_overlap.hip), the k-mer
// table (pw_kmers.hip) and the query-batched seed index (pw_qseeds.hip): the host check, the copy to the device and the kernels' LDS copy.  The table
// is alphabet_len <= 36 bytes, complement[c] for every letter c: a permutation of the alphabet that is its own inverse.
// Each C API keeps its own error channel: `sink` takes the message (as PW_HIP_CHECK's).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include <string>

#include "pw_hip_host.h"

// The complement table of a call in LDS (alphabet_len <= 36 bytes), read by every thread of the block.
__device__ __forceinline__ void load_complement(const uint8_t* __restrict__ comp, int L, uint8_t* s_comp) {
  if ((int)threadIdx.x < 36) s_comp[threadIdx.x] = (int)threadIdx.x < L ? comp[threadIdx.x] : (uint8_t)0;
  __syncthreads();
}

// complement[c] for c < L: a permutation of the alphabet that is its own inverse
template <typename Sink>
int check_complement(Sink&& sink, const uint8_t* comp, int L) {
  if (L < 1 || L > 36) return 0;                       // (the caller's own checks report the alphabet)
  bool ok = comp != nullptr;
  for (int c = 0; ok && c < L; c++) ok = comp[c] < L && comp[comp[c]] == c;
  if (!ok) { sink(std::string("complement must be alphabet_len bytes with complement[complement[c]] == c for every letter")); return -1; }
  return 0;
}

// the complement table on the device (36 bytes, zero padded): copied before the call returns, or, given a stream (null
// included), by hipMemcpyAsync on it (upload, pw_hip_host.h)
template <typename Sink>
int upload_complement(Sink&& sink, const uint8_t* comp, int L, DeviceArray<uint8_t>& d_comp) {
  uint8_t padded[36] = {0};
  memcpy(padded, comp, (size_t)L);
  return upload(sink, d_comp, padded, sizeof padded);
}
template <typename Sink>
int upload_complement(Sink&& sink, const uint8_t* comp, int L, DeviceArray<uint8_t>& d_comp, hipStream_t st) {
  uint8_t padded[36] = {0};
  memcpy(padded, comp, (size_t)L);
  return upload(sink, d_comp, padded, sizeof padded, st);
}

// pw_kmer_encode.h -- what the two translation units that index a whole READ SET share: overlap band selection (pw_overlap.hip,
// K9) and the k-mer table (pw_kmers.hip).  Device code: the k-mer of a position in either strand (kmer_fwd, kmer_rc) and the
// read encoders K9a / K9a'.  Host code: the argument checks of the all-pairs entry points (check_args) and the two rocPRIM
// helpers every stage of both goes through (sort_pairs, scan_u64), over typed device arrays (DeviceArray<T>, pw_hip_host.h: the
// element types are rocPRIM's template arguments).  Everything lives in an anonymous namespace: each
// translation unit gets its own copy of the kernels and reports through its own error channel (`sink`, as PW_HIP_CHECK's).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <cstring>
#include <string>
#include <rocprim/rocprim.hpp>

#include "pw_complement.h"
#include "pw_hip_host.h"

namespace {

// the k-mer s[0], s[1], ... s[k - 1], in base L
__device__ __forceinline__ uint64_t kmer_fwd(const uint8_t* __restrict__ s, int k, int L) {
  uint64_t v = 0;
  for (int t = 0; t < k; t++) v = v * (uint64_t)L + s[t];
  return v;
}
// The k-mer at position q of rc(read), never materialised: comp(read[len - 1 - q]), comp(read[len - 2 - q]), ... -- read
// backwards from the forward letters, s_last = &read[len - 1 - q].  q <= len - k, so s_last[-t] stays inside the read.
__device__ __forceinline__ uint64_t kmer_rc(const uint8_t* __restrict__ s_last, int k, int L, const uint8_t* s_comp) {
  uint64_t v = 0;
  for (int t = 0; t < k; t++) v = v * (uint64_t)L + s_comp[s_last[-t]];
  return v;
}

// K9a: k-mer of every position of every read; value = (read << 32) | pos.  rstart[r] = first k-mer index of read r.
__global__ __launch_bounds__(256) void k_enc_reads(const uint8_t* __restrict__ arena, const uint64_t* __restrict__ roff,
                                                   const uint64_t* __restrict__ rstart, int64_t nreads, int64_t total, int k, int L,
                                                   uint64_t* __restrict__ keys, uint64_t* __restrict__ vals) {
  const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (g >= total) return;
  const int64_t r = upper_bound_dev<uint64_t>(rstart, nreads + 1, (uint64_t)g) - 1;
  const uint32_t q = (uint32_t)(g - (int64_t)rstart[r]);
  keys[g] = kmer_fwd(arena + roff[r] + q, k, L);
  vals[g] = ((uint64_t)r << 32) | q;
}
// K9a': entry q of read r is the k-mer at position q of rc(read r) (kmer_rc).
// Generated in ascending (read, q), so inside a run of equal k-mers the stable sort leaves (read, q) ascending.
__global__ __launch_bounds__(256) void k_enc_reads_rc(const uint8_t* __restrict__ arena, const uint64_t* __restrict__ roff,
                                                      const int32_t* __restrict__ rlen, const uint64_t* __restrict__ rstart,
                                                      int64_t nreads, int64_t total, int k, int L, const uint8_t* __restrict__ comp,
                                                      uint64_t* __restrict__ keys, uint64_t* __restrict__ vals) {
  __shared__ uint8_t s_comp[36];
  load_complement(comp, L, s_comp);
  const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (g >= total) return;
  const int64_t r = upper_bound_dev<uint64_t>(rstart, nreads + 1, (uint64_t)g) - 1;
  const uint32_t q = (uint32_t)(g - (int64_t)rstart[r]);
  keys[g] = kmer_rc(arena + roff[r] + (uint64_t)(rlen[r] - 1) - q, k, L, s_comp);
  vals[g] = ((uint64_t)r << 32) | q;
}

// n (key, value) pairs stably sorted by the low `bits` bits of the key
template <typename K, typename V>
hipError_t sort_pairs(DeviceBuffer& tmp, const DeviceArray<K>& kin, DeviceArray<K>& kout, const DeviceArray<V>& vin, DeviceArray<V>& vout,
                      size_t n, int bits, hipStream_t stream = nullptr) {
  return rocprim_run(tmp, [&](void* t, size_t& b) {
    return rocprim::radix_sort_pairs(t, b, kin.cp(), kout.p, vin.cp(), vout.p, n, 0u, (unsigned)bits, stream);
  });
}
// out[i] = in[0] + ... + in[i - 1].  Ordinary functions, not a template on the input's type: rocPRIM's scan is instantiated
// here, ahead of the including unit's own, and the unit's kernels keep their order and fingerprints.  (unsigned long long: as rocPRIM wrote the counts)
hipError_t scan_u64(DeviceBuffer& tmp, const uint64_t* in, DeviceArray<uint64_t>& out, size_t n, hipStream_t stream) {
  return rocprim_run(tmp, [&](void* t, size_t& b) {
    return rocprim::exclusive_scan(t, b, in, out.p, (uint64_t)0, n, rocprim::plus<uint64_t>(), stream);
  });
}
hipError_t scan_u64(DeviceBuffer& tmp, const DeviceArray<uint64_t>& in, DeviceArray<uint64_t>& out, size_t n, hipStream_t stream = nullptr) {
  return scan_u64(tmp, in.cp(), out, n, stream);
}
hipError_t scan_u64(DeviceBuffer& tmp, const DeviceArray<unsigned long long>& in, DeviceArray<uint64_t>& out, size_t n,
                    hipStream_t stream = nullptr) {
  return scan_u64(tmp, in.as<const uint64_t>(), out, n, stream);
}

// The argument checks of the entry points that take a read set or a pair list, in this order: word range, counts and
// pointers (bad_args), coefficients, shard (bad_shard), L^k, reads inside the arena (outside(i) for i < n), letters inside
// the alphabet.  kbits: the width of the k-mer keys, the bits of L^k - 1.  L^k = 2^62 is accepted here (pw_seeds_create
// refuses it: its masked key is L^k).
template <typename Sink, typename Outside>
int check_args(Sink&& sink, int L, int k, bool bad_args, double len_coeff, double radius_coeff, double word_p_null, bool bad_shard,
               int64_t n, Outside outside, const uint8_t* arena, uint64_t arena_bytes, int* kbits) {
  if (L < 1 || L > 36 || k < 1 || k > 31) { sink("alphabet_len 1..36, wordlen 1..31"); return -1; }
  if (bad_args) { sink("bad arguments"); return -1; }
  if (!(len_coeff > 0) || !(radius_coeff > 0) || !(word_p_null > 0)) { sink("coefficients must be positive"); return -1; }
  if (bad_shard) { sink("bad shard"); return -1; }
  uint64_t kmax = 1;
  for (int i = 0; i < k; i++) { if (kmax > (1ull << 62) / (uint64_t)L) { sink("alphabet_len ^ wordlen must be below 2^62"); return -1; } kmax *= (uint64_t)L; }
  *kbits = bits_for(kmax - 1);
  for (int64_t i = 0; i < n; i++) if (outside(i)) { sink("a read lies outside the arena"); return -1; }
  for (uint64_t i = 0; i < arena_bytes; i++) if (arena[i] >= L) { sink("letter outside the alphabet"); return -1; }
  return 0;
}

}  // namespace

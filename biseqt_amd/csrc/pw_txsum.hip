// pw_txsum.hip -- K11: alignment summaries (include/pw_txsum.h).  One wavefront per transcript reduces the op bytes the
// traceback left in HBM to a 48-byte record: letter counts, gap runs, first / last match and the letters the ends in front
// of the first and behind the last match consume.  No atomics, no LDS: every lane keeps its own partial results over the
// dwords it reads, the wavefront combines them with shuffles, lane 0 writes the record with three 16-byte stores.  A long
// transcript (a strip-pipeline pair: 10^5 ops) is the same wavefront looping; nothing is split over blocks, so the result
// does not depend on the launch.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/pw_txsum.h"
#include "pw_launch.h"

static_assert(sizeof(pw_tx_summary) == 48, "summary record must be 48 bytes");

namespace pw {

namespace {

// 0x80 in every byte of w that equals the byte of c4 (the idiom of k_trace_fixup, pw_trace.hip)
__device__ __forceinline__ uint32_t tx_bytes_equal(uint32_t w, uint32_t c4) {
  const uint32_t v = w ^ c4;
  const uint32_t t = (v & 0x7f7f7f7fu) + 0x7f7f7f7fu;
  return ~(t | v | 0x7f7f7f7fu);
}
constexpr uint32_t kM4 = 0x4d4d4d4du, kS4 = 0x53535353u, kI4 = 0x49494949u, kD4 = 0x44444444u;

__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}
__device__ __forceinline__ int wave_min(int v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) { const int o = __shfl_xor(v, off, 64); v = o < v ? o : v; }
  return v;
}
__device__ __forceinline__ int wave_max(int v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) { const int o = __shfl_xor(v, off, 64); v = o > v ? o : v; }
  return v;
}

// The bytes ops[a, b) handed to f(w, pos) four at a time: w holds ops[pos .. pos + 3], the lowest address in the low byte.
// Bytes up to the first aligned dword and behind the last one are read one by one, as k_trace_fixup reads them, and come
// alone in the low byte of a w whose other bytes are 0 -- no letter.  Every lane takes every 64th dword.
template <typename F>
__device__ __forceinline__ void tx_scan(const uint8_t* __restrict__ ops, int a, int b, int lane, F&& f) {
  const int len = b - a;
  if (len <= 0) return;
  const uint8_t* p = ops + a;
  int head = (int)((4u - (uint32_t)((uintptr_t)p & 3u)) & 3u);          // bytes up to the first aligned dword
  head = head < len ? head : len;
  if (lane < head) f((uint32_t)p[lane], a + lane);
  const int nwords = (len - head) >> 2;
  const uint32_t* pw4 = (const uint32_t*)(p + head);
  for (int q = lane; q < nwords; q += 64) f(pw4[q], a + head + 4 * q);
  const int tail0 = head + 4 * nwords;
  if (tail0 + lane < len) f((uint32_t)p[tail0 + lane], a + tail0 + lane);
}

// The summary of ops[0, n), n > 0, in every lane of the wavefront.
__device__ __forceinline__ pw_tx_summary tx_summarize(const uint8_t* __restrict__ ops, int n, int lane) {
  int nM = 0, nS = 0, nI = 0, nD = 0, nG = 0, first = 0x7fffffff, last = -1;
  tx_scan(ops, 0, n, lane, [&](uint32_t w, int pos) {
    const uint32_t eM = tx_bytes_equal(w, kM4), eS = tx_bytes_equal(w, kS4), eI = tx_bytes_equal(w, kI4), eD = tx_bytes_equal(w, kD4);
    nM += __popc(eM); nS += __popc(eS); nI += __popc(eI); nD += __popc(eD);
    if (eI | eD) {
      // a gap byte opens a run when the byte in front of it is another letter: the dword's bytes shifted up by one, with the
      // byte in front of the dword -- read directly; it does not exist at position 0 -- in the low byte
      const uint32_t before = (w << 8) | (pos > 0 ? (uint32_t)ops[pos - 1] : 0u);
      nG += __popc(eI & ~tx_bytes_equal(before, kI4)) + __popc(eD & ~tx_bytes_equal(before, kD4));
    }
    if (eM) {
      const int lo = pos + ((__ffs((int)eM) - 1) >> 3), hi = pos + ((31 - __clz((int)eM)) >> 3);
      first = lo < first ? lo : first;
      last = hi > last ? hi : last;
    }
  });
  pw_tx_summary s;
  s.n_match = wave_sum(nM); s.n_subst = wave_sum(nS); s.n_ins = wave_sum(nI); s.n_del = wave_sum(nD); s.n_gaps = wave_sum(nG);
  first = wave_min(first); last = wave_max(last);
  s.head_origin = s.head_mutant = s.tail_origin = s.tail_mutant = 0;
  s.flags = PW_TXSUM_DONE;
  if (last < 0) { s.first_match = -1; s.last_match = -1; return s; }      // (uniform: no 'M', no second pass)
  s.first_match = first; s.last_match = last;
  int hO = 0, hM = 0, tO = 0, tM = 0;
  tx_scan(ops, 0, first, lane, [&](uint32_t w, int) {
    const int cS = __popc(tx_bytes_equal(w, kS4));
    hO += cS + __popc(tx_bytes_equal(w, kD4)); hM += cS + __popc(tx_bytes_equal(w, kI4));
  });
  tx_scan(ops, last + 1, n, lane, [&](uint32_t w, int) {
    const int cS = __popc(tx_bytes_equal(w, kS4));
    tO += cS + __popc(tx_bytes_equal(w, kD4)); tM += cS + __popc(tx_bytes_equal(w, kI4));
  });
  if (first > 0) { s.head_origin = wave_sum(hO); s.head_mutant = wave_sum(hM); }
  if (last + 1 < n) { s.tail_origin = wave_sum(tO); s.tail_mutant = wave_sum(tM); }
  return s;
}

// The record of a pair without a summarised transcript.
__device__ __forceinline__ pw_tx_summary tx_none() {
  pw_tx_summary s;
  s.n_match = s.n_subst = s.n_ins = s.n_del = s.n_gaps = 0;
  s.first_match = s.last_match = -1;
  s.head_origin = s.head_mutant = s.tail_origin = s.tail_mutant = 0;
  s.flags = 0;
  return s;
}

// 48 bytes, 16-byte aligned (the buffers come from hipMalloc, 48 = 3 * 16): three 16-byte vector stores of one lane
__device__ __forceinline__ void tx_store(pw_tx_summary* __restrict__ out, const pw_tx_summary& s) {
  int4* o = (int4*)out;
  o[0] = make_int4(s.n_match, s.n_subst, s.n_ins, s.n_del);
  o[1] = make_int4(s.n_gaps, s.first_match, s.last_match, s.head_origin);
  o[2] = make_int4(s.head_mutant, s.tail_origin, s.tail_mutant, s.flags);
}

}  // namespace

// over a batch's slots: the ops of a pair are right-aligned in its slot (any byte alignment), as k_trace_fixup and k_tx_pack
// address them
__global__ __launch_bounds__(64) void k_tx_summary(const PairDesc* __restrict__ pairs, const Result* __restrict__ results,
                                                   const uint8_t* __restrict__ slots, pw_tx_summary* __restrict__ out) {
  const int pair = (int)blockIdx.x;
  const int lane = (int)(threadIdx.x & 63u);
  const Result r = results[pair];
  const bool ok = (r.status & ST_TRACED) && !(r.status & (ST_EMPTY | ST_PANICK | ST_BADPATH)) && r.tx_len > 0;
  pw_tx_summary s = tx_none();
  if (ok) {
    const PairDesc& pd = pairs[pair];
    s = tx_summarize(slots + pd.tx_off + pd.tx_cap - r.tx_len, r.tx_len, lane);
  }
  if (lane == 0) tx_store(out + pair, s);
}

// over a packed buffer and its offsets (the layout of pw_batch_pack_transcripts)
__global__ __launch_bounds__(64) void k_tx_summary_packed(const uint8_t* __restrict__ ops, const unsigned long long* __restrict__ offsets,
                                                          pw_tx_summary* __restrict__ out) {
  const int64_t k = (int64_t)blockIdx.x;
  const int lane = (int)(threadIdx.x & 63u);
  const unsigned long long o0 = offsets[k], o1 = offsets[k + 1];
  pw_tx_summary s = tx_none();
  if (o1 > o0) s = tx_summarize(ops + o0, (int)(o1 - o0), lane);
  if (lane == 0) tx_store(out + k, s);
}

hipError_t launch_tx_summary(const PairDesc* pairs, const Result* results, const uint8_t* slots, int n, void* out, hipStream_t st) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_tx_summary, dim3((unsigned)n), dim3(64), 0, st, pairs, results, slots, (pw_tx_summary*)out);
  return hipGetLastError();
}

hipError_t launch_tx_summary_packed(const uint8_t* ops, const uint64_t* offsets, int n, void* out, hipStream_t st) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_tx_summary_packed, dim3((unsigned)n), dim3(64), 0, st, ops, (const unsigned long long*)offsets, (pw_tx_summary*)out);
  return hipGetLastError();
}

}  // namespace pw

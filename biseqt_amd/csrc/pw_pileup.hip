// pw_pileup.hip -- K13: pileups (include/pw_pileup.h).  k_pileup_add: one wavefront per pair scatters the op bytes the
// traceback left in HBM into per-column counts of the pair's origin, with 32-bit integer atomic adds without return (the
// counts are integers: the result does not depend on the order of arrival).  k_pileup_call: one thread per column turns
// its row of counts into an 8-byte site record.
//
// k_pileup_add reads the ALIGNED dwords that hold the transcript, as K12 does (pw_cigar.hip): dword q sits in lane
// q % 64 of pass q / 64 whatever the transcript's first address is, so the order of the lanes is the order of the ops;
// the first and the last dword may hold bytes of a neighbour and are read byte by byte, the bytes outside come as 0 -- no
// op.  Per pass of 256 bytes every lane counts the origin-consuming ('M', 'S', 'D') and the mutant-consuming ('M', 'S',
// 'I') ops of its dword, both counts travel in one register (16 bits each: a pass holds at most 256 of either) through one
// inclusive prefix sum of the wavefront, and two running totals are carried from pass to pass: that gives every op its
// column and its mutant letter.  A long transcript (a strip-pipeline pair: 10^5 ops) is the same wavefront looping;
// nothing is split over blocks.  No LDS, no scratch.
//
// Consecutive ops of a wavefront fall on consecutive columns, so one atomic wave-instruction touches 64 neighbouring rows
// of (alphabet_len + 2) dwords, one dword in each.  There is no pre-aggregation stage: wavefronts that pile onto the same
// columns meet in the L2's atomic units (measured: DESIGN.md, "Pileups").
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/pw_pileup.h"
#include "pw_launch.h"

static_assert(sizeof(pw_pileup_site) == 8, "site record must be 8 bytes");

namespace pw {

namespace {

// 0x80 in every byte of w that equals the byte of c4 (the idiom of k_trace_fixup, pw_trace.hip; tx_bytes_equal of K11)
__device__ __forceinline__ uint32_t pu_bytes_equal(uint32_t w, uint32_t c4) {
  const uint32_t v = w ^ c4;
  const uint32_t t = (v & 0x7f7f7f7fu) + 0x7f7f7f7fu;
  return ~(t | v | 0x7f7f7f7fu);
}
constexpr uint32_t kM4 = 0x4d4d4d4du, kS4 = 0x53535353u, kI4 = 0x49494949u, kD4 = 0x44444444u;

// a pair with a transcript to pile up: the predicate of k_tx_summary
__device__ __forceinline__ bool pu_has_ops(const Result& r) {
  return (r.status & ST_TRACED) && !(r.status & (ST_EMPTY | ST_PANICK | ST_BADPATH)) && r.tx_len > 0;
}

}  // namespace

// counts: uint32_t[n_cols][L + 2].  col0: frame start per pair, or null for o_off - arena_first.  A pair whose origin frame
// does not lie inside [0, n_cols) adds nothing, so no op needs a range check against the buffer; an op is still dropped
// when it would leave its own frames (a transcript the traceback wrote never does).
__global__ __launch_bounds__(64) void k_pileup_add(const PairDesc* __restrict__ pairs, const Result* __restrict__ results,
                                                   const uint8_t* __restrict__ slots, const uint8_t* __restrict__ arena,
                                                   const long long* __restrict__ col0, long long arena_first,
                                                   uint32_t* __restrict__ counts, long long n_cols, int L) {
  const int pair = (int)blockIdx.x;
  const int lane = (int)(threadIdx.x & 63u);
  const Result r = results[pair];
  if (!pu_has_ops(r)) return;
  const PairDesc& pd = pairs[pair];
  const int X = pd.X, Y = pd.Y;
  const long long f = col0 ? col0[pair] : (long long)pd.o_off - arena_first;
  if (f < 0 || f + X > n_cols) return;                  // (uniform)
  const int stride = L + 2;
  uint32_t* __restrict__ rows = counts + f * stride;    // row 0 = the frame's first letter
  const uint8_t* __restrict__ mut = arena + pd.m_off;
  const int n = r.tx_len;
  const uint8_t* ops = slots + pd.tx_off + pd.tx_cap - n;
  const int mis = (int)((uintptr_t)ops & 3u);
  const uint8_t* p0 = ops - mis;                        // 4-byte aligned; op k is byte mis + k of p0
  const int nq = (mis + n + 3) >> 2;
  int O = r.origin_idx, Q = r.mutant_idx;               // frame positions of the pass's first op
  for (int q0 = 0; q0 < nq; q0 += 64) {                 // (uniform: every lane takes part in the shuffles)
    const int q = q0 + lane;
    const int lo = 4 * q - mis;                         // the op in byte 0 of the dword
    uint32_t w = 0, prev = 0;
    if (q < nq) {
      if (lo >= 0 && lo + 4 <= n) w = *(const uint32_t*)(p0 + 4 * (int64_t)q);
      else {
#pragma unroll
        for (int j = 0; j < 4; j++)
          if (lo + j >= 0 && lo + j < n) w |= (uint32_t)p0[4 * (int64_t)q + j] << (8 * j);
      }
      if (lo > 0 && lo <= n) prev = (uint32_t)p0[4 * (int64_t)q - 1];       // the op in front of the dword (0: none)
    }
    const uint32_t eMS = pu_bytes_equal(w, kM4) | pu_bytes_equal(w, kS4), eD = pu_bytes_equal(w, kD4), eI = pu_bytes_equal(w, kI4);
    const uint32_t ev = eI & ~pu_bytes_equal((w << 8) | prev, kI4);          // an 'I' behind anything but an 'I': an event
    const uint32_t v = (uint32_t)__popc(eMS | eD) | ((uint32_t)__popc(eMS | eI) << 16);
    uint32_t incl = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const uint32_t u = __shfl_up(incl, off, 64);
      if (lane >= off) incl += u;
    }
    const uint32_t total = __shfl(incl, 63, 64);
    int o = O + (int)((incl - v) & 0xffffu), m = Q + (int)((incl - v) >> 16);
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const uint32_t bit = 0x80u << (8 * j);
      if (eMS & bit) {
        if ((uint32_t)o < (uint32_t)X && (uint32_t)m < (uint32_t)Y) {
          const int y = (int)mut[m];
          if (y < L) atomicAdd(rows + (int64_t)o * stride + y, 1u);
        }
        o++; m++;
      } else if (eD & bit) {
        if ((uint32_t)o < (uint32_t)X) atomicAdd(rows + (int64_t)o * stride + L, 1u);
        o++;
      } else if (eI & bit) {
        if ((ev & bit) && o > r.origin_idx && (uint32_t)(o - 1) < (uint32_t)X) atomicAdd(rows + (int64_t)(o - 1) * stride + L + 1, 1u);
        m++;
      }
    }
    O += (int)(total & 0xffffu); Q += (int)(total >> 16);
  }
}

// One thread per column: consecutive threads read consecutive rows, so a wavefront reads one contiguous stretch of counts.
__global__ __launch_bounds__(256) void k_pileup_call(const uint32_t* __restrict__ counts, const uint8_t* __restrict__ ref,
                                                     long long n_cols, int L, uint32_t min_depth, pw_pileup_site* __restrict__ sites) {
  const long long col = (long long)blockIdx.x * 256 + threadIdx.x;
  if (col >= n_cols) return;
  const uint32_t* __restrict__ row = counts + col * (L + 2);
  uint32_t depth = 0, best = 0, call = 0;
  for (int ch = 0; ch <= L; ch++) {                     // letters, then DEL; a tie stays with the lower channel
    const uint32_t c = row[ch];
    depth += c;
    if (c > best) { best = c; call = (uint32_t)ch; }
  }
  const uint32_t ins = row[L + 1];
  const bool covered = depth >= min_depth;
  if (!covered || depth == 0) call = 255u;
  const uint32_t rl = ref ? (uint32_t)ref[col] : 255u;
  uint32_t flags = 0;
  if (covered) {
    flags = PW_PILEUP_COVERED;
    if (ref && call != rl) flags |= PW_PILEUP_DIFFERS;
    if (2ull * ins > (unsigned long long)depth) flags |= PW_PILEUP_INSERT;
  }
  ((uint2*)sites)[col] = make_uint2(depth, call | (rl << 8) | (flags << 16));
}

hipError_t launch_pileup_add(const PairDesc* pairs, const Result* results, const uint8_t* slots, const uint8_t* arena, int n,
                             const int64_t* col0, int64_t arena_first, uint32_t* counts, int64_t n_cols, int L, hipStream_t st) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_pileup_add, dim3((unsigned)n), dim3(64), 0, st, pairs, results, slots, arena, (const long long*)col0,
                     (long long)arena_first, counts, (long long)n_cols, L);
  return hipGetLastError();
}

hipError_t launch_pileup_call(const uint32_t* counts, const uint8_t* ref, int64_t n_cols, int L, uint32_t min_depth, void* sites,
                              hipStream_t st) {
  if (n_cols <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_pileup_call, dim3((unsigned)((n_cols + 255) / 256)), dim3(256), 0, st, counts, ref, (long long)n_cols, L, min_depth,
                     (pw_pileup_site*)sites);
  return hipGetLastError();
}

}  // namespace pw

// pw_polish.hip -- K16: read correction (include/pw_polish.h).  k_polish_add: one wavefront per pair and side scatters the
// op bytes the traceback left in HBM into the per-column counts AND the insertion plane of the pair's origin, of its mutant,
// or of its mutant read backwards.  k_polish_letters: the self vote, one thread per column.  k_polish_count, an exclusive
// scan over the reads, k_polish_write: the polished reads, one wavefront per read.
//
// k_polish_add has the shape of k_pileup_add (pw_pileup.hip): the ALIGNED dwords of the transcript, dword q in lane q % 64
// of pass q / 64, byte masks, the origin- and the mutant-consuming ops of a dword counted into one register (16 bits each)
// and carried through one inclusive prefix sum of the wavefront per pass of 256 bytes.  Three things are new.
//   - The side.  The mutant side is the origin side of the swapped pair: the 'D' and the 'I' masks change places (a uniform
//     select) and the two frames change roles.
//   - The reversal.  A reversed side walks the transcript from its last op: pass by pass the dwords come from the end and
//     their bytes are swapped, which turns the aligned bytes into the same stream with another misalignment,
//     4 * nq - mis - n.  The letters of the other frame are the origin's read backwards through the complement table; the
//     table is 32 bytes of kernel arguments (scalar registers), a letter picks its byte with seven selects.  The totals o(n)
//     and m(n) that the start indices need come from a counting pass of the same wavefront over the same dwords.
//   - The slot of an inserted letter.  The index of an 'I' within its run is m - (m at the run's first op), and the run's
//     first op is the one behind the latest op that is no 'I'.  m is monotone, so "the m behind the latest non-'I' op in
//     front of this lane" is an inclusive max scan of the wavefront, shifted by one lane, with the maximum of all earlier
//     passes carried along: a run may straddle dwords, lanes and passes.  An 'I' whose index is 0 is the insertion EVENT.
// No LDS, no scratch; every count is an atomic add without return.  The per-pair frame test is the only guard against
// columns outside the buffers: an op is still dropped when it would leave its own frames.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <cstring>
#include <rocprim/rocprim.hpp>

#include "../../include/pw_polish.h"
#include "pw_hip_host.h"
#include "pw_launch.h"
#include "pw_polish_column.h"

static_assert(sizeof(pw_polish_stats) == 16, "statistics record must be 16 bytes");

namespace pw {

namespace {

// 0x80 in every byte of w that equals the byte of c4 (pu_bytes_equal of pw_pileup.hip)
__device__ __forceinline__ uint32_t po_bytes_equal(uint32_t w, uint32_t c4) {
  const uint32_t v = w ^ c4;
  const uint32_t t = (v & 0x7f7f7f7fu) + 0x7f7f7f7fu;
  return ~(t | v | 0x7f7f7f7fu);
}
constexpr uint32_t kM4 = 0x4d4d4d4du, kS4 = 0x53535353u, kI4 = 0x49494949u, kD4 = 0x44444444u;

__device__ __forceinline__ bool po_has_ops(const Result& r) {
  return (r.status & ST_TRACED) && !(r.status & (ST_EMPTY | ST_PANICK | ST_BADPATH)) && r.tx_len > 0;
}

// complement[y] for y < 32 out of the eight dwords of the table (uniform values: no indexed access, so no scratch)
__device__ __forceinline__ int po_complement(const PolishComplement& c, int y) {
  const uint32_t a0 = (y & 4) ? c.w[1] : c.w[0], a1 = (y & 4) ? c.w[3] : c.w[2], a2 = (y & 4) ? c.w[5] : c.w[4], a3 = (y & 4) ? c.w[7] : c.w[6];
  const uint32_t b0 = (y & 8) ? a1 : a0, b1 = (y & 8) ? a3 : a2;
  return (int)((((y & 16) ? b1 : b0) >> (8 * (y & 3))) & 0xffu);
}

// Dword q of the op stream of a pair (forward: aligned dword q; reversed: aligned dword nq - 1 - q, bytes swapped); bytes
// outside the transcript come as 0 -- no op.  p0: the aligned base; op k sits in byte mis + k of p0.
__device__ __forceinline__ uint32_t po_stream_dword(const uint8_t* p0, int mis, int n, int nq, int q, bool rev) {
  const int pq = rev ? nq - 1 - q : q;
  const int lo = 4 * pq - mis;
  uint32_t w = 0;
  if (lo >= 0 && lo + 4 <= n) w = *(const uint32_t*)(p0 + 4 * (int64_t)pq);
  else {
#pragma unroll
    for (int j = 0; j < 4; j++)
      if (lo + j >= 0 && lo + j < n) w |= (uint32_t)p0[4 * (int64_t)pq + j] << (8 * j);
  }
  return rev ? __builtin_bswap32(w) : w;
}

}  // namespace

// counts: uint32_t[n_cols][L + 2]; ins: uint32_t[n_cols][J][L] or null (J = 0).  Block (pair, y): side side0 + y, 0 the
// origin's and 1 the mutant's.  ocol0 / mcol0: frame starts per pair, or null for o_off / m_off - arena_first.  reversed:
// a byte per pair or null.  A side whose frame does not lie inside [0, n_cols) adds nothing.
__global__ __launch_bounds__(64) void k_polish_add(const PairDesc* __restrict__ pairs, const Result* __restrict__ results,
                                                   const uint8_t* __restrict__ slots, const uint8_t* __restrict__ arena,
                                                   const long long* __restrict__ ocol0, const long long* __restrict__ mcol0,
                                                   const uint8_t* __restrict__ reversed, PolishComplement comp, long long arena_first,
                                                   uint32_t* __restrict__ counts, uint32_t* __restrict__ ins, long long n_cols, int L,
                                                   int J, int side0) {
  const int pair = (int)blockIdx.x;
  const int lane = (int)(threadIdx.x & 63u);
  const bool mside = (side0 + (int)blockIdx.y) != 0;
  const Result r = results[pair];
  if (!po_has_ops(r)) return;
  const PairDesc& pd = pairs[pair];
  const bool rev = mside && reversed && reversed[pair];
  // TX: the frame whose columns are written; UX: the frame the letters come from
  const int TX = mside ? pd.Y : pd.X, UX = mside ? pd.X : pd.Y;
  const long long f = mside ? (mcol0 ? mcol0[pair] : (long long)pd.m_off - arena_first)
                            : (ocol0 ? ocol0[pair] : (long long)pd.o_off - arena_first);
  if (f < 0 || f + TX > n_cols) return;                 // (uniform)
  const int stride = L + 2;
  uint32_t* __restrict__ rows = counts + f * stride;    // row 0 = the frame's first letter
  uint32_t* __restrict__ irows = ins ? ins + f * (long long)J * L : nullptr;
  const uint8_t* __restrict__ oth = arena + (mside ? pd.o_off : pd.m_off);
  const int n = r.tx_len;
  const uint8_t* ops = slots + pd.tx_off + pd.tx_cap - n;
  const int pmis = (int)((uintptr_t)ops & 3u);
  const uint8_t* p0 = ops - pmis;                       // 4-byte aligned; op k is byte pmis + k of p0
  const int nq = (pmis + n + 3) >> 2;
  int O = mside ? r.mutant_idx : r.origin_idx, Q = mside ? r.origin_idx : r.mutant_idx;   // frame positions of the pass's first op
  if (rev) {                                            // (uniform) the counting pass: o(n) and m(n)
    uint32_t on = 0, mn = 0;                            // (apart: a long transcript passes 16 bits)
    for (int q = lane; q < nq; q += 64) {
      const uint32_t w = po_stream_dword(p0, pmis, n, nq, q, false);
      const uint32_t eMS = po_bytes_equal(w, kM4) | po_bytes_equal(w, kS4);
      on += (uint32_t)__popc(eMS | po_bytes_equal(w, kD4));
      mn += (uint32_t)__popc(eMS | po_bytes_equal(w, kI4));
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { on += __shfl_xor(on, off, 64); mn += __shfl_xor(mn, off, 64); }
    O = pd.Y - (r.mutant_idx + (int)mn);
    Q = pd.X - (r.origin_idx + (int)on);
  }
  const int O0 = O;
  int RS = Q;                                           // m at the first op of the I run that reaches into this pass
  for (int q0 = 0; q0 < nq; q0 += 64) {                 // (uniform: every lane takes part in the shuffles)
    const int q = q0 + lane;
    const uint32_t w = q < nq ? po_stream_dword(p0, pmis, n, nq, q, rev) : 0u;
    const uint32_t eMS = po_bytes_equal(w, kM4) | po_bytes_equal(w, kS4);
    const uint32_t d4 = po_bytes_equal(w, kD4), i4 = po_bytes_equal(w, kI4);
    const uint32_t eD = mside ? i4 : d4, eI = mside ? d4 : i4;
    const uint32_t mcons = eMS | eI;
    const uint32_t v = (uint32_t)__popc(eMS | eD) | ((uint32_t)__popc(mcons) << 16);
    uint32_t incl = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const uint32_t u = __shfl_up(incl, off, 64);
      if (lane >= off) incl += u;
    }
    const uint32_t total = __shfl(incl, 63, 64);
    const int mrel = (int)((incl - v) >> 16);           // mutant-consuming ops of the pass in front of this dword
    // 1 + the pass-relative m behind the lane's last byte that is no 'I'; 0 when all four are
    const uint32_t nonI = ~eI & 0x80808080u;
    uint32_t last = nonI ? 1u + (uint32_t)mrel + (uint32_t)__popc(mcons & (0xffffffffu >> (__clz((int)nonI) & ~7))) : 0u;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const uint32_t u = __shfl_up(last, off, 64);
      if (lane >= off) last = max(last, u);
    }
    const uint32_t before = __shfl_up(last, 1, 64), all = __shfl(last, 63, 64);
    int rs = (lane > 0 && before) ? Q + (int)before - 1 : RS;
    int o = O + (int)((incl - v) & 0xffffu), m = Q + mrel;
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const uint32_t bit = 0x80u << (8 * j);
      if (eI & bit) {
        const int idx = m - rs;
        if (o > O0 && (uint32_t)(o - 1) < (uint32_t)TX) {
          if (idx == 0) atomicAdd(rows + (int64_t)(o - 1) * stride + L + 1, 1u);
          if (idx < J && (uint32_t)m < (uint32_t)UX) {
            int y = (int)oth[rev ? UX - 1 - m : m];
            if (rev && y < L) y = po_complement(comp, y);
            if (y < L) atomicAdd(irows + ((int64_t)(o - 1) * J + idx) * L + y, 1u);
          }
        }
        m++;
      } else {
        if (eMS & bit) {
          if ((uint32_t)o < (uint32_t)TX && (uint32_t)m < (uint32_t)UX) {
            int y = (int)oth[rev ? UX - 1 - m : m];
            if (rev && y < L) y = po_complement(comp, y);
            if (y < L) atomicAdd(rows + (int64_t)o * stride + y, 1u);
          }
          o++; m++;
        } else if (eD & bit) {
          if ((uint32_t)o < (uint32_t)TX) atomicAdd(rows + (int64_t)o * stride + L, 1u);
          o++;
        }
        rs = m;
      }
    }
    if (all) RS = Q + (int)all - 1;
    O += (int)(total & 0xffffu); Q += (int)(total >> 16);
  }
}

// The self vote: one thread per column.
__global__ __launch_bounds__(256) void k_polish_letters(uint32_t* __restrict__ counts, const uint8_t* __restrict__ letters, long long lo,
                                                        long long hi, int L, uint32_t weight) {
  const long long c = lo + (long long)blockIdx.x * 256 + threadIdx.x;
  if (c >= hi) return;
  const int y = (int)letters[c - lo];
  if (y < L) atomicAdd(counts + c * (L + 2) + y, weight);
}

// One wavefront per read: lens[read] = the letters it emits, stats[read] its record.  (lens is uint64: the scan's input.)
__global__ __launch_bounds__(64) void k_polish_count(const uint32_t* __restrict__ counts, const uint32_t* __restrict__ ins,
                                                     const uint8_t* __restrict__ letters, const long long* __restrict__ roff,
                                                     const int* __restrict__ rlen, int L, int J, uint32_t min_depth,
                                                     unsigned long long* __restrict__ lens, pw_polish_stats* __restrict__ stats) {
  const long long read = blockIdx.x;
  const int lane = (int)(threadIdx.x & 63u);
  const long long off = roff[read];
  const int n = rlen[read];
  uint32_t len = 0, kept = 0, subst = 0, del = 0, insd = 0;
  for (int x = lane; x < n; x += 64) {
    const long long col = off + x;
    const uint32_t st = po_column(counts + col * (L + 2), ins ? ins + col * (long long)J * L : nullptr, (int)letters[col], L, J, min_depth,
                                  [&](uint8_t) { len++; });
    kept += st & 0xffu; subst += (st >> 8) & 0xffu; del += (st >> 16) & 0xffu; insd += st >> 24;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    len += __shfl_xor(len, o, 64); kept += __shfl_xor(kept, o, 64); subst += __shfl_xor(subst, o, 64);
    del += __shfl_xor(del, o, 64); insd += __shfl_xor(insd, o, 64);
  }
  if (lane == 0) {
    lens[read] = len;
    ((uint4*)stats)[read] = make_uint4(kept, subst, del, insd);
  }
}

// One wavefront per read: every column's letters at out[offsets[read] + the letters of the columns in front], through one
// prefix sum of the wavefront per pass of 64 columns.
__global__ __launch_bounds__(64) void k_polish_write(const uint32_t* __restrict__ counts, const uint32_t* __restrict__ ins,
                                                     const uint8_t* __restrict__ letters, const long long* __restrict__ roff,
                                                     const int* __restrict__ rlen, int L, int J, uint32_t min_depth,
                                                     const unsigned long long* __restrict__ offsets, uint8_t* __restrict__ out) {
  const long long read = blockIdx.x;
  const int lane = (int)(threadIdx.x & 63u);
  const long long off = roff[read];
  const int n = rlen[read];
  const unsigned long long end = offsets[read + 1];
  unsigned long long base = offsets[read];
  for (int x0 = 0; x0 < n; x0 += 64) {                  // (uniform: every lane takes part in the shuffles)
    const int x = x0 + lane;
    const long long col = off + x;
    uint32_t len = 0, ninth = 0;
    unsigned long long word = 0;                        // the column's first eight letters, a byte each; at most 1 + 8
    if (x < n)
      po_column(counts + col * (L + 2), ins ? ins + col * (long long)J * L : nullptr, (int)letters[col], L, J, min_depth,
                [&](uint8_t y) {
                  if (len < 8) word |= (unsigned long long)y << (8 * len); else ninth = y;
                  len++;
                });
    uint32_t incl = len;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const uint32_t u = __shfl_up(incl, o, 64);
      if (lane >= o) incl += u;
    }
    const uint32_t total = __shfl(incl, 63, 64);
    unsigned long long at = base + (incl - len);
    for (uint32_t k = 0; k < len; k++)                  // (never past the read's own stretch of the output)
      if (at + k < end) out[at + k] = (uint8_t)(k < 8 ? (uint32_t)(word >> (8 * k)) & 0xffu : ninth);
    base += total;
  }
}

hipError_t launch_polish_add(const PairDesc* pairs, const Result* results, const uint8_t* slots, const uint8_t* arena, int n, int sides,
                             const int64_t* ocol0, const int64_t* mcol0, const uint8_t* reversed, const PolishComplement& comp,
                             int64_t arena_first, uint32_t* counts, uint32_t* ins, int64_t n_cols, int L, int J, hipStream_t st) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_polish_add, dim3((unsigned)n, sides == 3 ? 2u : 1u), dim3(64), 0, st, pairs, results, slots, arena,
                     (const long long*)ocol0, (const long long*)mcol0, reversed, comp, (long long)arena_first, counts, ins, (long long)n_cols, L,
                     ins ? J : 0, sides == 2 ? 1 : 0);
  return hipGetLastError();
}

hipError_t launch_polish_letters(uint32_t* counts, const uint8_t* letters, int64_t lo, int64_t hi, int L, uint32_t weight, hipStream_t st) {
  if (hi <= lo) return hipSuccess;
  hipLaunchKernelGGL(k_polish_letters, rows_grid((uint64_t)(hi - lo)), kBlock256, 0, st, counts, letters, (long long)lo, (long long)hi, L, weight);
  return hipGetLastError();
}

// lens[n + 1] (the last one zeroed here) -> offsets[n + 1] = their exclusive sums, [n] the total
hipError_t launch_polish_count(const uint32_t* counts, const uint32_t* ins, const uint8_t* letters, const int64_t* roff, const int32_t* rlen,
                               int64_t n, int L, int J, uint32_t min_depth, uint64_t* lens, uint64_t* offsets, void* stats, DeviceBuffer& tmp,
                               hipStream_t st) {
  hipError_t e = hipMemsetAsync(lens + n, 0, 8, st);
  if (e != hipSuccess) return e;
  if (n > 0) {
    hipLaunchKernelGGL(k_polish_count, dim3((unsigned)n), dim3(64), 0, st, counts, ins, letters, (const long long*)roff, rlen, L, ins ? J : 0,
                       min_depth, (unsigned long long*)lens, (pw_polish_stats*)stats);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  return rocprim_run(tmp, [&](void* t, size_t& b) {
    return rocprim::exclusive_scan(t, b, (const uint64_t*)lens, offsets, (uint64_t)0, (size_t)n + 1, rocprim::plus<uint64_t>(), st);
  });
}

hipError_t launch_polish_write(const uint32_t* counts, const uint32_t* ins, const uint8_t* letters, const int64_t* roff, const int32_t* rlen,
                               int64_t n, int L, int J, uint32_t min_depth, const uint64_t* offsets, uint8_t* out, hipStream_t st) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_polish_write, dim3((unsigned)n), dim3(64), 0, st, counts, ins, letters, (const long long*)roff, rlen, L, ins ? J : 0,
                     min_depth, (const unsigned long long*)offsets, out);
  return hipGetLastError();
}

}  // namespace pw

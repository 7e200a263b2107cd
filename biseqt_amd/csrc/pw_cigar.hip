// pw_cigar.hip -- K12: CIGARs (include/pw_cigar.h).  One wavefront per transcript turns the op bytes the traceback left in
// HBM into runs, one dword (length << 4 | op) per maximal stretch of one op class.  K12a counts the runs of every
// transcript, one workgroup turns the counts into exclusive offsets, K12b writes every run at offsets[pair] + its index.
// No atomics, no LDS in K12a / K12b: a run's index and length come from prefix operations of the wavefront over the run
// starts of its 64 dwords, and from two numbers carried from one 256-byte pass to the next.  A long transcript (a
// strip-pipeline pair: 10^5 ops) is the same wavefront looping; nothing is split over blocks, so the result does not
// depend on the launch.
//
// The wavefront reads the ALIGNED dwords that hold the transcript: dword q sits in lane q % 64 of pass q / 64, whatever
// the transcript's first address is, so the order of the lanes is the order of the ops.  The first and the last dword may
// hold bytes of a neighbour; those two are read byte by byte, the bytes outside come as 0 -- no letter.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/pw_cigar.h"
#include "pw_launch.h"

namespace pw {

namespace {

// 0x80 in every byte of w that equals the byte of c4 (the idiom of k_trace_fixup, pw_trace.hip)
__device__ __forceinline__ uint32_t cg_bytes_equal(uint32_t w, uint32_t c4) {
  const uint32_t v = w ^ c4;
  const uint32_t t = (v & 0x7f7f7f7fu) + 0x7f7f7f7fu;
  return ~(t | v | 0x7f7f7f7fu);
}

// The op class of every byte of w: the byte itself in the extended form (fold == 0); in the classic form (fold == 'M' ^ 'S')
// every 'S' becomes 'M', so that neighbouring 'M' and 'S' stretches are one run.
constexpr uint32_t kFoldClassic = 0x4du ^ 0x53u;
__device__ __forceinline__ uint32_t cg_class(uint32_t w, uint32_t fold) { return w ^ ((cg_bytes_equal(w, 0x53535353u) >> 7) * fold); }

// BAM's op code of a class byte
__device__ __forceinline__ uint32_t cg_op(uint32_t c, uint32_t fold) {
  return c == 0x49u ? (uint32_t)PW_CIGAR_OP_I : c == 0x44u ? (uint32_t)PW_CIGAR_OP_D : c == 0x53u ? (uint32_t)PW_CIGAR_OP_X
       : fold ? (uint32_t)PW_CIGAR_OP_M : (uint32_t)PW_CIGAR_OP_EQ;
}

// The transcript ops[0, n), n > 0, as aligned dwords: p0 = ops - mis is 4-byte aligned, op k is byte mis + k of p0, nq dwords.
struct CgView {
  const uint8_t* p0;
  int mis, n, nq;
  __device__ __forceinline__ CgView(const uint8_t* ops, int n_) : p0(ops - ((uintptr_t)ops & 3u)), mis((int)((uintptr_t)ops & 3u)), n(n_), nq((mis + n_ + 3) >> 2) {}
};

// 0x80 in every byte of dword q that is an op of the transcript and starts a run: the first op, or an op whose class differs
// from the class of the op in front of it.  *before: the classes shifted up by one byte, i.e. in byte j the class of the op
// in front of byte j (the dword trick tx_summarize, pw_txsum.hip, uses for gap runs).  q >= nq gives 0.
__device__ __forceinline__ uint32_t cg_starts(const CgView& v, int q, uint32_t fold, uint32_t* before) {
  const int lo = 4 * q - v.mis;                        // the op in byte 0 of the dword
  uint32_t w = 0, in = 0;
  if (lo >= 0 && lo + 4 <= v.n) { w = *(const uint32_t*)(v.p0 + 4 * (int64_t)q); in = 0x80808080u; }
  else {
#pragma unroll
    for (int j = 0; j < 4; j++)
      if (lo + j >= 0 && lo + j < v.n) { w |= (uint32_t)v.p0[4 * (int64_t)q + j] << (8 * j); in |= 0x80u << (8 * j); }
  }
  w = cg_class(w, fold);
  const uint32_t prev = lo > 0 && lo <= v.n ? (uint32_t)v.p0[4 * (int64_t)q - 1] : 0u;     // (0: no letter -- op 0 starts a run)
  *before = (w << 8) | cg_class(prev, fold);
  return ~cg_bytes_equal(w, *before) & in;
}

// K12a: the number of runs of ops[0, n), n > 0, in every lane
__device__ __forceinline__ uint32_t cg_count(const uint8_t* __restrict__ ops, int n, int lane, uint32_t fold) {
  const CgView v(ops, n);
  int c = 0;
  for (int q = lane; q < v.nq; q += 64) { uint32_t before; c += __popc(cg_starts(v, q, fold, &before)); }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) c += __shfl_xor(c, off, 64);
  return (uint32_t)c;
}

// K12b: the runs of ops[0, n), n > 0, to out[0 .. runs).  A run is written by the lane that holds the start of the NEXT run:
// there the run's last op is the byte in front (its class is in `before`), its index is the number of starts so far minus
// one, and its length is the distance to the latest start in front.  Per pass of 64 dwords:
//   - index: exclusive sum scan of the starts per lane (0 .. 4, three ballots, one per bit of the count) plus the starts of
//     the passes before (`done`);
//   - latest start in front of a lane: exclusive max scan of the lanes' last start positions -- positions grow with the
//     lane, so it is the last start of the nearest lane below that has one (a ballot and one shuffle) -- or the latest
//     start of the passes before (`last`).
// The last run ends with the transcript: lane 0 writes it.
__device__ __forceinline__ void cg_write(const uint8_t* __restrict__ ops, int n, int lane, uint32_t fold, uint32_t* __restrict__ out) {
  const CgView v(ops, n);
  const unsigned long long below = (1ull << lane) - 1ull;
  int done = 0, last = 0;
  for (int q0 = 0; q0 < v.nq; q0 += 64) {                 // (uniform: every lane takes part in the ballots and the shuffles)
    const int q = q0 + lane;
    uint32_t before;
    const uint32_t s = cg_starts(v, q, fold, &before);
    const int c = __popc(s);
    const unsigned long long b0 = __ballot(c & 1), b1 = __ballot(c & 2), b2 = __ballot(c & 4), any = b0 | b1 | b2;
    int r = done + __popcll(b0 & below) + 2 * __popcll(b1 & below) + 4 * __popcll(b2 & below);
    const int lo = 4 * q - v.mis;
    const int mine = lo + ((31 - __clz((int)s)) >> 3);   // position of this lane's last start (meaningless without one)
    const unsigned long long under = any & below;
    int prev = __shfl(mine, under ? 63 - __clzll((long long)under) : lane, 64);
    if (!under) prev = last;
#pragma unroll
    for (int j = 0; j < 4; j++)
      if (s & (0x80u << (8 * j))) {
        const int p = lo + j;
        if (r > 0) out[r - 1] = ((uint32_t)(p - prev) << 4) | cg_op((before >> (8 * j)) & 0xffu, fold);
        prev = p;
        r++;
      }
    done += __popcll(b0) + 2 * __popcll(b1) + 4 * __popcll(b2);
    if (any) last = __shfl(mine, 63 - __clzll((long long)any), 64);
  }
  if (lane == 0) out[done - 1] = ((uint32_t)(n - last) << 4) | cg_op(cg_class((uint32_t)ops[n - 1], fold), fold);
}

// a pair with a transcript to encode: the predicate of k_tx_summary
__device__ __forceinline__ bool cg_has_ops(const Result& r) {
  return (r.status & ST_TRACED) && !(r.status & (ST_EMPTY | ST_PANICK | ST_BADPATH)) && r.tx_len > 0;
}

}  // namespace

// over a batch's slots: the ops of a pair are right-aligned in its slot (any byte alignment), as k_tx_summary addresses them.
// counts[pair] is a uint64: k_cigar_offsets scans the array in place.
__global__ __launch_bounds__(64) void k_cigar_count(const PairDesc* __restrict__ pairs, const Result* __restrict__ results,
                                                    const uint8_t* __restrict__ slots, uint32_t fold, unsigned long long* __restrict__ counts) {
  const int pair = (int)blockIdx.x;
  const int lane = (int)(threadIdx.x & 63u);
  const Result r = results[pair];
  uint32_t c = 0;
  if (cg_has_ops(r)) {
    const PairDesc& pd = pairs[pair];
    c = cg_count(slots + pd.tx_off + pd.tx_cap - r.tx_len, r.tx_len, lane, fold);
  }
  if (lane == 0) counts[pair] = c;
}

__global__ __launch_bounds__(64) void k_cigar_write(const PairDesc* __restrict__ pairs, const Result* __restrict__ results,
                                                    const uint8_t* __restrict__ slots, uint32_t fold,
                                                    const unsigned long long* __restrict__ offsets, uint32_t* __restrict__ runs) {
  const int pair = (int)blockIdx.x;
  const int lane = (int)(threadIdx.x & 63u);
  const Result r = results[pair];
  if (!cg_has_ops(r)) return;
  const PairDesc& pd = pairs[pair];
  cg_write(slots + pd.tx_off + pd.tx_cap - r.tx_len, r.tx_len, lane, fold, runs + offsets[pair]);
}

// over a packed buffer and its offsets (the layout of pw_batch_pack_transcripts)
__global__ __launch_bounds__(64) void k_cigar_count_packed(const uint8_t* __restrict__ ops, const unsigned long long* __restrict__ offsets,
                                                           uint32_t fold, unsigned long long* __restrict__ counts) {
  const int64_t k = (int64_t)blockIdx.x;
  const int lane = (int)(threadIdx.x & 63u);
  const unsigned long long o0 = offsets[k], o1 = offsets[k + 1];
  uint32_t c = 0;
  if (o1 > o0) c = cg_count(ops + o0, (int)(o1 - o0), lane, fold);
  if (lane == 0) counts[k] = c;
}

__global__ __launch_bounds__(64) void k_cigar_write_packed(const uint8_t* __restrict__ ops, const unsigned long long* __restrict__ offsets,
                                                           uint32_t fold, const unsigned long long* __restrict__ run_offsets,
                                                           uint32_t* __restrict__ runs) {
  const int64_t k = (int64_t)blockIdx.x;
  const int lane = (int)(threadIdx.x & 63u);
  const unsigned long long o0 = offsets[k], o1 = offsets[k + 1];
  if (o1 > o0) cg_write(ops + o0, (int)(o1 - o0), lane, fold, runs + run_offsets[k]);
}

// counts[0, n) -> exclusive prefix sums in place, a[n] = total: the scheme of k_tx_offsets (pw_trace.hip) -- one workgroup, a
// chunk per thread, the chunk sums scanned in LDS.  In place: every thread reads an element of its own chunk before it
// overwrites it, and no other thread touches that chunk.
__global__ __launch_bounds__(1024) void k_cigar_offsets(unsigned long long* __restrict__ a, int n) {
  __shared__ unsigned long long part[1024];
  const int t = (int)threadIdx.x;
  const int per = (n + 1023) / 1024;
  const int64_t k0 = (int64_t)t * per, k1 = k0 + per < n ? k0 + per : n;
  unsigned long long s = 0;
  for (int64_t k = k0; k < k1; k++) s += a[k];
  part[t] = s;
  __syncthreads();
  for (int off = 1; off < 1024; off <<= 1) {              // inclusive scan of the chunk sums
    const unsigned long long u = t >= off ? part[t - off] : 0ull;
    __syncthreads();
    part[t] += u;
    __syncthreads();
  }
  unsigned long long run = t > 0 ? part[t - 1] : 0ull;
  for (int64_t k = k0; k < k1; k++) {
    const unsigned long long c = a[k];
    a[k] = run;
    run += c;
  }
  if (t == 1023) a[n] = part[1023];
}

namespace {
uint32_t fold_of(int form) { return form == PW_CIGAR_CLASSIC ? kFoldClassic : 0u; }
}  // namespace

hipError_t launch_cigar_count(const PairDesc* pairs, const Result* results, const uint8_t* slots, int n, int form, uint64_t* offsets,
                              hipStream_t st) {
  if (n > 0) {
    hipLaunchKernelGGL(k_cigar_count, dim3((unsigned)n), dim3(64), 0, st, pairs, results, slots, fold_of(form), (unsigned long long*)offsets);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(k_cigar_offsets, dim3(1), dim3(1024), 0, st, (unsigned long long*)offsets, n > 0 ? n : 0);
  return hipGetLastError();
}

hipError_t launch_cigar_write(const PairDesc* pairs, const Result* results, const uint8_t* slots, int n, int form, const uint64_t* offsets,
                              uint32_t* runs, hipStream_t st) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_cigar_write, dim3((unsigned)n), dim3(64), 0, st, pairs, results, slots, fold_of(form), (const unsigned long long*)offsets, runs);
  return hipGetLastError();
}

hipError_t launch_cigar_count_packed(const uint8_t* ops, const uint64_t* offsets, int n, int form, uint64_t* run_offsets, hipStream_t st) {
  if (n > 0) {
    hipLaunchKernelGGL(k_cigar_count_packed, dim3((unsigned)n), dim3(64), 0, st, ops, (const unsigned long long*)offsets, fold_of(form),
                       (unsigned long long*)run_offsets);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(k_cigar_offsets, dim3(1), dim3(1024), 0, st, (unsigned long long*)run_offsets, n > 0 ? n : 0);
  return hipGetLastError();
}

hipError_t launch_cigar_write_packed(const uint8_t* ops, const uint64_t* offsets, int n, int form, const uint64_t* run_offsets, uint32_t* runs,
                                     hipStream_t st) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_cigar_write_packed, dim3((unsigned)n), dim3(64), 0, st, ops, (const unsigned long long*)offsets, fold_of(form),
                     (const unsigned long long*)run_offsets, runs);
  return hipGetLastError();
}

}  // namespace pw

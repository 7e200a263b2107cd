// pw_minimizer.h -- window-minimizer sampling of the k-mer positions of a READ SET, shared by the two translation units that
// index one: overlap band selection (pw_overlap.hip, K9) and the k-mer table (pw_kmers.hip).  Included behind pw_kmer_encode.h,
// whose kmer_fwd / kmer_rc give the keys; everything lives in an anonymous namespace, as there.
//
// THE RULE (include/pw_kmers.h states it in full).  x(p) is the key of the k-mer at position p of a read with n positions,
// x'(p) the key of its reverse complement; the order value is h(p) = mix(x(p)), or mix(min(x(p), x'(p))) under the canonical
// order (any strand selection but PW_STRAND_PLUS).  With ww = min(window, n), p is selected when some window of ww consecutive
// positions of the read contains p and h(p) equals its minimum -- every position that attains a minimum, no tie is broken:
// lg = the consecutive positions left of p with h >= h(p), rg the same to the right, both stopping at the read's ends and at
// ww - 1; p is selected exactly when lg + rg + 1 >= ww.
//
//   K15a k_mini_count   over the flat position space g of K9a (k_enc_reads): a workgroup stages the order values of its 256
//                       positions and of a halo of window - 1 on each side in LDS, every key computed once per staged position;
//                       a thread walks left and right from its own position inside its own read (it knows its read's ends: a
//                       halo position of a neighbouring read is never looked at).  Each wavefront writes its 64 flags as one
//                       word of the selection bitmap and their number: 16 bytes per 64 positions, nothing per position
//        scan           exclusive sum of the words' counts = the row of every word's first selected position
//   K15b k_mini_emit    one thread per position; a selected one writes its row (key = x(p), never the order value; hit =
//                       (read << 32) | p) at its rank: rows come out in ascending (read, pos) and the stable sort by k-mer
//                       leaves runs ordered as the unsampled encoders do.  <REV>: the reverse-strand index.  Under the
//                       canonical order the selected set of rc(read) is the mirror image n - 1 - p of the read's own, so the
//                       same flags give its rows: key x'(p) = the k-mer at q = n - 1 - p of rc(read), hit (read << 32) | q, in
//                       ascending (read, q) -- descending p inside a read, at starts[r] + starts[r + 1] - 1 - rank
//   K15c k_mini_starts  one thread per read: the sampled forward rows before it (a binary search of the forward hits, which
//                       ascend); starts[n_reads] = all of them
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pw_hip_host.h"
#include "pw_kmer_encode.h"

namespace {

constexpr int kMiniMaxWindow = 128;
constexpr int kMiniTile = 256 + 2 * (kMiniMaxWindow - 1);      // staged order values per workgroup

// a bijection of the 64-bit integers (the finaliser of splitmix64 behind its increment): equal order values mean equal keys,
// and the added constant keeps key 0 -- the homopolymer of letter 0 -- from being the minimum of every window
__device__ __forceinline__ uint64_t mini_mix(uint64_t x) {
  uint64_t z = x + 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// the order value of flat position g (0 <= g < total); r, q, n: its read, its position in it, the read's positions
template <bool CANON>
__device__ __forceinline__ uint64_t mini_order(const uint8_t* __restrict__ arena, const uint64_t* __restrict__ roff,
                                               const uint64_t* __restrict__ rstart, int64_t nreads, int64_t g, int k, int L,
                                               const uint8_t* __restrict__ comp, int64_t& r, uint32_t& q, uint32_t& n) {
  r = upper_bound_dev<uint64_t>(rstart, nreads + 1, (uint64_t)g) - 1;
  q = (uint32_t)(g - (int64_t)rstart[r]);
  n = (uint32_t)(rstart[r + 1] - rstart[r]);
  const uint8_t* s = arena + roff[r] + q;
  uint64_t x = kmer_fwd(s, k, L);
  if (CANON) { const uint64_t y = kmer_rc(s + (k - 1), k, L, comp); x = y < x ? y : x; }
  return mini_mix(x);
}

// K15a.  bits[j], wcnt[j]: the flags and the selected count of positions [64 j, 64 j + 64), j < ceil(total / 64).
// LDS index t <-> flat position 256 blockIdx.x - (window - 1) + t; a thread's own position sits at t = tid + window - 1.
template <bool CANON>
__global__ __launch_bounds__(256) void k_mini_count(const uint8_t* __restrict__ arena, const uint64_t* __restrict__ roff,
                                                    const uint64_t* __restrict__ rstart, int64_t nreads, int64_t total, int k, int L,
                                                    int window, const uint8_t* __restrict__ comp, uint64_t* __restrict__ bits,
                                                    uint64_t* __restrict__ wcnt) {
  __shared__ uint64_t s_h[kMiniTile];
  const int tid = (int)threadIdx.x, halo = window - 1;
  const int64_t g0 = (int64_t)blockIdx.x * 256, g = g0 + tid;
  int64_t r = 0; uint32_t q = 0, n = 0;
  if (g < total) s_h[tid + halo] = mini_order<CANON>(arena, roff, rstart, nreads, g, k, L, comp, r, q, n);
  if (tid < 2 * halo) {                                // the halo: window - 1 positions left of the block, then right of it
    const int t = tid < halo ? tid : 256 + tid;
    const int64_t gh = g0 - halo + t;
    int64_t rh; uint32_t qh, nh;
    if (gh >= 0 && gh < total) s_h[t] = mini_order<CANON>(arena, roff, rstart, nreads, gh, k, L, comp, rh, qh, nh);
  }
  __syncthreads();
  bool sel = false;
  if (g < total) {
    const int ww = n < (uint32_t)window ? (int)n : window;
    const int lmax = q < (uint32_t)(ww - 1) ? (int)q : ww - 1;                      // the read's first position, or ww - 1
    const int rmax = n - 1 - q < (uint32_t)(ww - 1) ? (int)(n - 1 - q) : ww - 1;    // its last one
    const int t = tid + halo;
    const uint64_t h = s_h[t];
    int lg = 0, rg = 0;
    while (lg < lmax && s_h[t - lg - 1] >= h) lg++;
    while (rg < rmax && lg + rg + 1 < ww && s_h[t + rg + 1] >= h) rg++;
    sel = lg + rg + 1 >= ww;
  }
  const unsigned long long word = __ballot(sel);
  const int64_t j = g0 / 64 + (tid >> 6);
  if ((tid & 63) == 0 && j * 64 < total) { bits[j] = (uint64_t)word; wcnt[j] = (uint64_t)__popcll(word); }
}

// K15b.  woff: the exclusive sum of wcnt.  REV: starts = the sampled forward rows before every read (K15c).
template <bool REV>
__global__ __launch_bounds__(256) void k_mini_emit(const uint8_t* __restrict__ arena, const uint64_t* __restrict__ roff,
                                                   const uint64_t* __restrict__ rstart, int64_t nreads, int64_t total, int k, int L,
                                                   const uint8_t* __restrict__ comp, const uint64_t* __restrict__ bits,
                                                   const uint64_t* __restrict__ woff, const uint64_t* __restrict__ starts,
                                                   uint64_t* __restrict__ keys, uint64_t* __restrict__ vals) {
  const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (g >= total) return;
  const uint64_t word = bits[g >> 6];
  const int lane = (int)(g & 63);
  if (!(word >> lane & 1ull)) return;
  const uint64_t i = woff[g >> 6] + (uint64_t)__popcll(word & ((1ull << lane) - 1ull));
  const int64_t r = upper_bound_dev<uint64_t>(rstart, nreads + 1, (uint64_t)g) - 1;
  const uint32_t p = (uint32_t)(g - (int64_t)rstart[r]);
  const uint8_t* s = arena + roff[r] + p;
  if (REV) {
    const uint32_t n = (uint32_t)(rstart[r + 1] - rstart[r]);
    const uint64_t o = starts[r] + starts[r + 1] - 1ull - i;
    keys[o] = kmer_rc(s + (k - 1), k, L, comp);
    vals[o] = ((uint64_t)r << 32) | (n - 1u - p);
  } else {
    keys[i] = kmer_fwd(s, k, L);
    vals[i] = ((uint64_t)r << 32) | p;
  }
}

// K15c.  fvals: the hits of the sampled forward rows in (read, pos) order, as K15b wrote them.
__global__ __launch_bounds__(256) void k_mini_starts(const uint64_t* __restrict__ fvals, int64_t rows, int64_t nreads,
                                                     uint64_t* __restrict__ starts) {
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (r > nreads) return;
  starts[r] = (uint64_t)lower_bound_dev<uint64_t>(fvals, rows, (uint64_t)r << 32);
}

// The host side of the stage.  count() runs K15a and the scan and WAITS for the number of rows (the index behind it is sized
// by it); emit() and read_starts() only launch.  The reads (arena, roff, rstart: the UNSAMPLED first position of every read,
// n_reads + 1 entries) are the caller's device arrays.
struct MiniSample {
  DeviceArray<uint64_t> bits, wcnt, woff, starts;
  uint64_t positions = 0, rows = 0;                    // forward positions before / after sampling

  // the stage's own memory for `total` positions of n_reads reads (count() calls it; ahead of a timed region, call it first)
  template <typename Sink>
  int reserve(Sink&& sink, int64_t n_reads, uint64_t total) {
    const size_t words = (size_t)((total + 63) / 64);
    PW_HIP_CHECK(sink, bits.ensure(words)); PW_HIP_CHECK(sink, wcnt.ensure(words)); PW_HIP_CHECK(sink, woff.ensure(words));
    PW_HIP_CHECK(sink, starts.ensure((size_t)n_reads + 1));
    return 0;
  }
  template <typename Sink>
  int count(Sink&& sink, DeviceBuffer& tmp, const uint8_t* arena, const uint64_t* roff, const uint64_t* rstart, int64_t n_reads,
            uint64_t total, int k, int L, int window, bool canonical, const uint8_t* comp, hipStream_t st) {
    const size_t words = (size_t)((total + 63) / 64);
    positions = total; rows = 0;
    if (reserve(sink, n_reads, total) != 0) return -1;
    auto* const kernel = canonical ? k_mini_count<true> : k_mini_count<false>;
    hipLaunchKernelGGL(kernel, rows_grid(total), kBlock256, 0, st, arena, roff, rstart, n_reads, (int64_t)total, k, L, window, comp, bits.p,
                       wcnt.p);
    PW_HIP_CHECK(sink, scan_u64(tmp, wcnt, woff, words, st));
    uint64_t last[2] = {0, 0};
    PW_HIP_CHECK(sink, hipMemcpyAsync(&last[0], woff.p + (words - 1), sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    PW_HIP_CHECK(sink, hipMemcpyAsync(&last[1], wcnt.p + (words - 1), sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    PW_HIP_CHECK(sink, hipStreamSynchronize(st));
    PW_HIP_CHECK(sink, hipGetLastError());
    rows = last[0] + last[1];
    return 0;
  }
  // the sampled rows of one strand into keys / vals (`rows` entries each); the reverse strand after read_starts()
  void emit(bool reverse, const uint8_t* arena, const uint64_t* roff, const uint64_t* rstart, int64_t n_reads, int k, int L,
            const uint8_t* comp, uint64_t* keys, uint64_t* vals, hipStream_t st) const {
    auto* const kernel = reverse ? k_mini_emit<true> : k_mini_emit<false>;
    hipLaunchKernelGGL(kernel, rows_grid(positions), kBlock256, 0, st, arena, roff, rstart, n_reads, (int64_t)positions, k, L, comp, bits.cp(),
                       woff.cp(), starts.cp(), keys, vals);
  }
  // starts[r] = the sampled forward rows of the reads before r, from the forward hits emit(false) wrote
  void read_starts(const uint64_t* fvals, int64_t n_reads, hipStream_t st) {
    hipLaunchKernelGGL(k_mini_starts, rows_grid((uint64_t)n_reads + 1), kBlock256, 0, st, fvals, (int64_t)rows, n_reads, starts.p);
  }
};

}  // namespace

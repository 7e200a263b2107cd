// pw_overlap.hip -- overlap band selection for many read pairs at once (C ABI: include/pw_overlap.h).
//
//   K8a k_enc_batch   k-mer of every position of every pair's S (or T) read, key = (pair << kbits) | k-mer
//       sort          both sides by key (rocPRIM radix sort, stable: positions ascending inside a k-mer)
//   K8b k_join_hist   one thread per sorted S element: its run of equal keys on the T side; every (i, j) of the run
//                     is one seed: atomicAdd into the pair's per-diagonal histogram (rows are never written), the
//                     pair's row count, and atomicMin of the element index (-> the first row in table order)
//   K8c k_band_select one workgroup per pair: prefix sums of the histogram, then for every occupied diagonal the
//                     window of diagonals within 1 on the axis d / r(d) (the reference's own floating-point
//                     predicate; d / r(d) is monotone in d), n(d), w(d); block reduction to the best diagonal, the
//                     tie count and the seed count of its band
//   K8d k_band_small  at most 64 seeds: one wavefront per pair, from the seed list
//   K8e k_band_medium 65 .. 2048 seeds (all-pairs path): one workgroup per pair, from the seed list in LDS
// K8c, K8d and K8e differ only in how they count the seeds of a window: the window (ov_window), the score (band_w), the order
// of two diagonals (better), the tie rule (tie_threshold, ties) and the record (band_record) exist once; records are byte-identical.
// All floating point is IEEE double in the reference's operation order (compiled with -ffp-contract=off).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <cstring>
#include <algorithm>
#include <string>
#include <vector>
#include <rocprim/rocprim.hpp>

#include "../../include/pw_overlap.h"
#include "pw_complement.h"
#include "pw_hip_host.h"
#include "pw_kmer_encode.h"
#include "pw_minimizer.h"

namespace {

thread_local std::string g_err;
thread_local double g_ms = 0.0;
void set_err(const std::string& s) { g_err = s; }
#define CHECK(call) PW_HIP_CHECK(set_err, call)

struct DPair { uint64_t s_off, t_off; int32_t s_len, t_len; uint64_t hbase; };   // hbase: start of its histogram

// side 0: S reads, side 1: T reads.  start[p] = index of pair p's first k-mer on this side (start[n] = total).
__global__ __launch_bounds__(256) void k_enc_batch(const uint8_t* __restrict__ arena, const DPair* __restrict__ pairs,
                                                   const uint64_t* __restrict__ start, int64_t npairs, int64_t total, int side,
                                                   int k, int L, int kbits, uint64_t* __restrict__ keys, uint32_t* __restrict__ pos) {
  const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (g >= total) return;
  const int64_t p = upper_bound_dev<uint64_t>(start, npairs + 1, (uint64_t)g) - 1;
  const DPair pr = pairs[p];
  const uint32_t q = (uint32_t)(g - (int64_t)start[p]);
  keys[g] = ((uint64_t)p << kbits) | kmer_fwd(arena + (side ? pr.t_off : pr.s_off) + q, k, L);
  pos[g] = q;
}

// K8a', stranded pair list: the T side where strand[p] != 0 encodes T = rc(read) (kmer_rc).
// Entries are generated in ascending q, so the stable sort keeps positions of T ascending inside a k-mer.
__global__ __launch_bounds__(256) void k_enc_batch_rc(const uint8_t* __restrict__ arena, const DPair* __restrict__ pairs,
                                                      const uint64_t* __restrict__ start, int64_t npairs, int64_t total,
                                                      const uint8_t* __restrict__ strand, const uint8_t* __restrict__ comp,
                                                      int k, int L, int kbits, uint64_t* __restrict__ keys, uint32_t* __restrict__ pos) {
  __shared__ uint8_t s_comp[36];
  load_complement(comp, L, s_comp);
  const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (g >= total) return;
  const int64_t p = upper_bound_dev<uint64_t>(start, npairs + 1, (uint64_t)g) - 1;
  const DPair pr = pairs[p];
  const uint32_t q = (uint32_t)(g - (int64_t)start[p]);
  const uint64_t v = strand[p] ? kmer_rc(arena + pr.t_off + (uint64_t)(pr.t_len - 1) - q, k, L, s_comp)
                               : kmer_fwd(arena + pr.t_off + q, k, L);
  keys[g] = ((uint64_t)p << kbits) | v;
  pos[g] = q;
}

__global__ __launch_bounds__(256) void k_join_hist(const uint64_t* __restrict__ ks, const uint32_t* __restrict__ ps, int64_t ns,
                                                   const uint64_t* __restrict__ kt, const uint32_t* __restrict__ pt, int64_t nt,
                                                   const DPair* __restrict__ pairs, int kbits, uint32_t* __restrict__ hist,
                                                   unsigned long long* __restrict__ nrows, uint32_t* __restrict__ first_e,
                                                   int32_t* __restrict__ dlist /* [npairs][64]: the diagonals of a pair's first 64 seeds */) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= ns) return;
  const uint64_t key = ks[e];
  const int64_t lo = lower_bound_dev<uint64_t>(kt, nt, key);
  if (lo >= nt || kt[lo] != key) return;
  const int64_t hi = upper_bound_dev<uint64_t>(kt, nt, key);
  const int64_t p = (int64_t)(key >> kbits);
  const DPair pr = pairs[p];
  const int i = (int)ps[e];
  uint32_t* __restrict__ h = hist + pr.hbase + pr.t_len;      // h[d], d = -t_len .. s_len
  const unsigned long long slot0 = atomicAdd(&nrows[p], (unsigned long long)(hi - lo));
  for (int64_t t = lo; t < hi; t++) {
    const int d = i - (int)pt[t];
    atomicAdd(&h[d], 1u);
    const unsigned long long slot = slot0 + (unsigned long long)(t - lo);
    if (slot < 64ull) dlist[p * 64 + (int64_t)slot] = d;      // pairs with <= 64 seeds are scored from this list (K8d)
  }
  atomicMin(&first_e[p], (uint32_t)e);                        // (fewer than 2^32 k-mers per chunk, checked by the host)
}

struct BandConst { double q, C, p0; };
__device__ __forceinline__ int ov_len(int d, int ls, int lt, double q) {
  const int wall = (ls - d < lt ? ls - d : lt) + (d < 0 ? d : 0);
  return (int)ceil(q * (double)wall);
}
__device__ __forceinline__ int ov_rad(int L, double C) {
  const int r = (int)ceil(C * sqrt((double)L));
  return r < 1 ? 1 : r;
}
__device__ __forceinline__ double ov_x(int d, int ls, int lt, BandConst c) {
  return (double)d / (double)ov_rad(ov_len(d, ls, lt, c.q), c.C);
}

// ---- what the three scoring kernels share -------------------------------------------------------------------------
// L, r and the window [first, last] of diagonals within 1 of d on the axis d / r(d).  Both predicates are monotone in d'
// (what the binary searches of the first version relied on), so the same two boundaries are found by walking from a
// guess -- d -+ r, where they are unless r(d') changes in between: a handful of evaluations of x(d') instead of 2 x 14.
__device__ __forceinline__ void ov_window(int d, int ls, int lt, BandConst c, int& L, int& r, int& first, int& last) {
  L = ov_len(d, ls, lt, c.q); r = ov_rad(L, c.C);
  const double x = (double)d / (double)r;
  first = d - r < -lt ? -lt : d - r;                   // smallest d' in [-lt, d] with x - x(d') <= 1
  if (x - ov_x(first, ls, lt, c) <= 1.0) { while (first > -lt && x - ov_x(first - 1, ls, lt, c) <= 1.0) first--; }
  else { do first++; while (first < d && !(x - ov_x(first, ls, lt, c) <= 1.0)); }
  last = d + r > ls ? ls : d + r;                      // largest d' in [d, ls] with x(d') - x <= 1
  if (ov_x(last, ls, lt, c) - x <= 1.0) { while (last < ls && ov_x(last + 1, ls, lt, c) - x <= 1.0) last++; }
  else { do last--; while (last > d && !(ov_x(last, ls, lt, c) - x <= 1.0)); }
}
// w(d) of a diagonal with n neighbours in its window: the seeds above the 2 r L p0 expected by chance, per letter
__device__ __forceinline__ double band_w(int n, int r, int L, double p0) {
  const long long area = 2ll * r * L;
  return ((double)(n + 1) - (double)area * p0) / (double)L;
}
// Which of two diagonals wins: the larger w, then the smaller d; d == kNoDiag is no diagonal at all and loses to any.
constexpr int kNoDiag = 0x7fffffff;
struct Best { double w; int d; };
__device__ __forceinline__ bool better(Best a, Best b) {
  return a.d != kNoDiag && (b.d == kNoDiag || a.w > b.w || (a.w == b.w && a.d < b.d));
}
// The tie rule.  p = min(w^(1/k), 1): everything at or above 1 ties, below it whatever is within 1e-9 relative of the best;
// where no w is positive every p is 0 and every occupied diagonal ties.
__device__ __forceinline__ double tie_threshold(double wbest) {
  const double wcap = wbest >= 1.0 ? 1.0 : wbest;
  return wcap - fabs(wcap) * 1e-9;
}
__device__ __forceinline__ bool ties(double wbest, double thr, double w) { return wbest <= 0.0 || w >= thr; }
// The best of a workgroup's 256 candidates, to every thread (s_w, s_d: 256 entries each).
__device__ __forceinline__ Best block_best(Best mine, double* s_w, int* s_d, int tid) {
  s_w[tid] = mine.w; s_d[tid] = mine.d;
  __syncthreads();
  for (int off = 128; off >= 1; off >>= 1) {
    if (tid < off) {
      const Best o{s_w[tid + off], s_d[tid + off]};
      if (better(o, Best{s_w[tid], s_d[tid]})) { s_w[tid] = o.w; s_d[tid] = o.d; }
    }
    __syncthreads();
  }
  const Best b{s_w[0], s_d[0]};
  __syncthreads();
  return b;
}
// N sums over a workgroup's 256 threads in one tree, to every thread (s: N x 256 entries).
template <int N>
__device__ __forceinline__ void block_sum(int (&v)[N], int* s, int tid) {
  for (int i = 0; i < N; i++) s[256 * i + tid] = v[i];
  __syncthreads();
  for (int off = 128; off >= 1; off >>= 1) {
    for (int i = 0; i < N; i++) if (tid < off) s[256 * i + tid] += s[256 * i + tid + off];
    __syncthreads();
  }
  for (int i = 0; i < N; i++) v[i] = s[256 * i];
}
// A diagonal as the record reports it -- the best one, or the first row's: n(d), L(d), r(d) and the seeds of [d - r, d + r].
struct BandSide { int d, n, len, r, band; };
__device__ __forceinline__ pw_overlap_band band_record(int64_t n_seeds, double w_best, int tie, BandSide best, BandSide first) {
  pw_overlap_band o;
  memset(&o, 0, sizeof o);
  o.n_seeds = n_seeds; o.w_best = w_best; o.tie = tie;
  o.d_best = best.d; o.n_best = best.n; o.len_best = best.len; o.r_best = best.r; o.band_best = best.band;
  o.d_first = first.d; o.n_first = first.n; o.len_first = first.len; o.r_first = first.r; o.band_first = first.band;
  return o;
}

// one workgroup per pair
__global__ __launch_bounds__(256) void k_band_select(const DPair* __restrict__ pairs, uint32_t* hist,
                                                     const unsigned long long* __restrict__ nrows, const int32_t* __restrict__ d_first,
                                                     uint64_t hist_first, int small_max, BandConst c, pw_overlap_band* __restrict__ out) {
  __shared__ uint32_t s_sum[256];
  __shared__ double s_w[256];
  __shared__ int s_d[256], s_cnt[256];
  // the occupied diagonals of the pair, in no particular order: the seeds of a true overlap sit on a few dozen neighbouring
  // diagonals, i.e. in the chunks of one or two threads -- evaluating them where they are found left 254 threads idle
  // (0.5 ms per pair); listed first, they are dealt round-robin
  constexpr int kMaxOcc = 8192;
  __shared__ int s_occ[kMaxOcc];
  __shared__ int s_nocc;
  const int p = (int)blockIdx.x, tid = (int)threadIdx.x;
  const DPair pr = pairs[p];
  const int ls = pr.s_len, lt = pr.t_len, nd = ls + lt + 1;
  uint32_t* h = hist + (pr.hbase - hist_first);        // `hist` starts at counter hist_first; index dd = d + lt
  const int64_t n_seeds = (int64_t)nrows[p];
  if (n_seeds == 0) { if (tid == 0) out[p] = band_record(0, 0.0, 0, BandSide{}, BandSide{}); return; }
  if (n_seeds <= small_max) return;                    // the sparse kernel (k_band_small) scores these
  // ---- inclusive prefix sums in place: every thread owns a contiguous chunk ----
  const int chunk = (nd + 255) / 256;
  const int b = tid * chunk, e = b + chunk < nd ? b + chunk : nd;
  uint32_t sum = 0;
  for (int dd = b; dd < e; dd++) sum += h[dd];
  s_sum[tid] = sum;
  __syncthreads();
  for (int off = 1; off < 256; off <<= 1) {
    const uint32_t v = tid >= off ? s_sum[tid - off] : 0u;
    __syncthreads();
    s_sum[tid] += v;
    __syncthreads();
  }
  if (tid == 0) s_nocc = 0;
  __syncthreads();
  uint32_t run = tid ? s_sum[tid - 1] : 0u;
  for (int dd = b; dd < e; dd++) {
    const uint32_t v = h[dd];
    run += v; h[dd] = run;
    if (v) { const int q = atomicAdd(&s_nocc, 1); if (q < kMaxOcc) s_occ[q] = dd; }
  }
  __threadfence_block();
  __syncthreads();
  const int nocc = s_nocc;
  const bool listed = nocc <= kMaxOcc;                 // else: every thread walks its own chunk (as before)
  auto pre = [&](int dd) -> uint32_t { return dd < 0 ? 0u : h[dd < nd ? dd : nd - 1]; };
  // neighbours of a seed on diagonal d and the score of its band
  auto eval = [&](int d, int& n, int& L, int& r) -> double {
    int first, last;
    ov_window(d, ls, lt, c, L, r, first, last);
    n = (int)(pre(last + lt) - pre(first + lt - 1)) - 1;
    return band_w(n, r, L, c.p0);
  };
  constexpr int kKeep = 4;                             // scores of this thread's first diagonals, kept for pass 2
  double wkeep[kKeep];
  // f(d, it) for every occupied diagonal of this thread; it < kKeep numbers the first ones of a listed pair
  auto each_occupied = [&](auto&& f) {
    if (listed) { int it = 0; for (int q = tid; q < nocc; q += 256, it++) f(s_occ[q] - lt, it); }
    else { for (int dd = b; dd < e; dd++) if (pre(dd) != pre(dd - 1)) f(dd - lt, kKeep); }
  };
  // ---- pass 1: the best occupied diagonal ----
  Best mine{0.0, kNoDiag};
  each_occupied([&](int d, int it) {
    int n, L, r;
    const double w = eval(d, n, L, r);
    if (it < kKeep) wkeep[it] = w;
    if (better(Best{w, d}, mine)) mine = Best{w, d};
  });
  const Best best = block_best(mine, s_w, s_d, tid);
  // ---- pass 2: how many occupied diagonals could reach the same p ----
  int tie[1] = {0};
  const double thr = tie_threshold(best.w);
  each_occupied([&](int d, int it) {
    int n, L, r;
    tie[0] += ties(best.w, thr, it < kKeep ? wkeep[it] : eval(d, n, L, r)) ? 1 : 0;
  });
  block_sum(tie, s_cnt, tid);
  if (tid == 0) {
    // the best diagonal, and the diagonal of the first row of the table (k-mer asc, i asc, j asc)
    BandSide side[2];
    for (int i = 0; i < 2; i++) {
      const int d = i ? d_first[p] : best.d;
      int n, L, r;
      (void)eval(d, n, L, r);
      side[i] = BandSide{d, n, L, r, (int)(pre(d + r + lt) - pre(d - r + lt - 1))};
    }
    out[p] = band_record(n_seeds, best.w, tie[0], side[0], side[1]);
  }
}

// pair-list path: the first row = the first sorted S element with a match, paired with the first j of its run
__global__ __launch_bounds__(256) void k_first_d(const uint32_t* __restrict__ first_e, int64_t npairs, const uint64_t* __restrict__ ks,
                                                 const uint32_t* __restrict__ ps, const uint64_t* __restrict__ kt,
                                                 const uint32_t* __restrict__ pt, int64_t nt, int32_t* __restrict__ d_first) {
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= npairs) return;
  const uint32_t fe = first_e[p];
  if (fe == 0xffffffffu) { d_first[p] = 0; return; }
  const int64_t lo = lower_bound_dev<uint64_t>(kt, nt, ks[fe]);
  d_first[p] = (int)ps[fe] - (int)pt[lo];
}

// ---- all reads against all reads through ONE index (K9) -----------------------------------------------------------
// (K9a and K9a', the read encoders, live in pw_kmer_encode.h: the k-mer table of pw_kmers.hip is built by the same two)
// K9b: self join.  Inside a run of equal k-mers the entries are ordered by (read, pos); element e pairs with every
// later entry of a DIFFERENT read: those start at fs[e].
// CAP (pw_overlap_all_pairs_capped): a k-mer whose run [lo, hi) holds more than max_occ entries is masked -- its entries get
// cnt[e] = 0, so its seeds are never expanded, sorted or grouped.  The run is counted over the WHOLE index, before the shard
// test, so every rank masks the same k-mers.  stats[0..2] += masked entries, masked runs (counted at their first entry),
// the seeds this rank's masked entries would have produced: one 64-bit integer atomic per wavefront and counter.
template <int N>
__device__ __forceinline__ void cap_tally(const unsigned long long (&t)[N], unsigned long long* __restrict__ stats) {
  for (int i = 0; i < N; i++) {
    unsigned long long v = t[i];
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_down(v, off, 64);
    if ((threadIdx.x & 63u) == 0 && v) atomicAdd(&stats[i], v);
  }
}
template <bool CAP>
__global__ __launch_bounds__(256) void k_self_count(const uint64_t* __restrict__ keys, const uint64_t* __restrict__ vals, int64_t n,
                                                    int shard_rank, int shard_world, uint32_t* __restrict__ fs, uint64_t* __restrict__ cnt,
                                                    uint32_t max_occ, unsigned long long* __restrict__ stats) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  unsigned long long tally[3] = {0, 0, 0};
  if (e < n) {
    // multi-GPU: the pairs (a, b), a < b, are dealt round-robin by a; every rank joins only its own share
    const bool mine = (int)((vals[e] >> 32) % (uint64_t)shard_world) == shard_rank;
    if (!mine) { fs[e] = (uint32_t)e; cnt[e] = 0; }
    if (mine || CAP) {
      const uint64_t key = keys[e];
      const int64_t hi = upper_bound_dev<uint64_t>(keys, n, key);
      bool masked = false;
      if (CAP) {
        const int64_t lo = lower_bound_dev<uint64_t>(keys, n, key);
        masked = (uint64_t)(hi - lo) > (uint64_t)max_occ;
        if (masked) { tally[0] = 1; tally[1] = lo == e ? 1 : 0; }
      }
      if (mine) {
        const uint64_t next_read = ((vals[e] >> 32) + 1) << 32;
        const int64_t f = e + 1 + lower_bound_dev<uint64_t>(vals + e + 1, hi - e - 1, next_read);
        fs[e] = (uint32_t)f;
        cnt[e] = masked ? 0ull : (uint64_t)(hi - f);
        if (masked) tally[2] = (unsigned long long)(hi - f);
      }
    }
  }
  if (CAP) cap_tally(tally, stats);
}
// one seed per thread: key = rank of the pair (ra < rb) = ra * nreads + rb, value = d = pos_a - pos_b.  Seeds are
// produced in (k-mer, i, j) order per pair, which a STABLE sort by the pair key keeps.
__global__ __launch_bounds__(256) void k_self_expand(const uint64_t* __restrict__ off, int64_t n, int64_t nseeds,
                                                     const uint64_t* __restrict__ vals, const uint32_t* __restrict__ fs,
                                                     uint64_t nreads, uint64_t* __restrict__ pkey, int32_t* __restrict__ dval) {
  const int64_t o = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (o >= nseeds) return;
  const int64_t e = upper_bound_dev<uint64_t>(off, n, (uint64_t)o) - 1;
  const int64_t f = (int64_t)fs[e] + (o - (int64_t)off[e]);
  const uint64_t va = vals[e], vb = vals[f];
  pkey[o] = (va >> 32) * nreads + (vb >> 32);
  dval[o] = (int32_t)(uint32_t)va - (int32_t)(uint32_t)vb;
}
// ---- both strands (K9'): a second index holds the k-mers of rc(read) for every read, computed from the forward letters ----
// K9b': forward element e of read a pairs with the forward entries (sel & 1) and the reverse entries (sel & 2) of every read
// b > a that hold the same k-mer: [ff[e], ff[e] + cf[e]) of the forward index, then [fr[e], ...) of the reverse index.
// A read is never joined with its own reverse complement, and no reverse entry plays the a side.
// CAP: occ(x) = the forward entries with the key + the reverse entries with the key, whatever `sel` joins -- count(x) of a k-mer
// table over both strands (pw_kmers.h).  x is masked exactly when rc(x) is, and the reverse index holds rc(x) as often as the
// forward index holds x: the masked reverse entries are as many as the masked forward ones, and a masked k-mer that only the
// reverse index holds is the reverse complement of a masked forward run without reverse entries -- both are counted from the
// forward entries alone (stats[1] += 2 for such a run).
template <bool CAP>
__global__ __launch_bounds__(256) void k_self_count_st(const uint64_t* __restrict__ keys, const uint64_t* __restrict__ vals, int64_t n,
                                                       const uint64_t* __restrict__ rkeys, const uint64_t* __restrict__ rvals, int sel,
                                                       int shard_rank, int shard_world, uint32_t* __restrict__ ff, uint32_t* __restrict__ cf,
                                                       uint32_t* __restrict__ fr, uint64_t* __restrict__ cnt, uint32_t max_occ,
                                                       unsigned long long* __restrict__ stats) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  unsigned long long tally[3] = {0, 0, 0};
  if (e < n) {
    const bool mine = (int)((vals[e] >> 32) % (uint64_t)shard_world) == shard_rank;
    uint32_t f_f = 0, c_f = 0, f_r = 0;
    uint64_t c = 0;
    if (mine || CAP) {
      const uint64_t key = keys[e];
      bool masked = false;
      if (CAP) {
        const int64_t flo = lower_bound_dev<uint64_t>(keys, n, key), fhi = upper_bound_dev<uint64_t>(keys, n, key);
        const int64_t rlo = lower_bound_dev<uint64_t>(rkeys, n, key), rhi = upper_bound_dev<uint64_t>(rkeys, n, key);
        masked = (uint64_t)(fhi - flo) + (uint64_t)(rhi - rlo) > (uint64_t)max_occ;
        if (masked) { tally[0] = 1; tally[1] = flo == e ? (rhi == rlo ? 2 : 1) : 0; }
      }
      if (mine) {
        const uint64_t next_read = ((vals[e] >> 32) + 1) << 32;
        if (sel & 1) {
          const int64_t hi = upper_bound_dev<uint64_t>(keys, n, key);
          const int64_t f = e + 1 + lower_bound_dev<uint64_t>(vals + e + 1, hi - e - 1, next_read);
          f_f = (uint32_t)f; c_f = (uint32_t)(hi - f);
          c += (uint64_t)(hi - f);
        }
        if (sel & 2) {
          const int64_t lo = lower_bound_dev<uint64_t>(rkeys, n, key);
          const int64_t hi = upper_bound_dev<uint64_t>(rkeys, n, key);
          const int64_t f = lo + lower_bound_dev<uint64_t>(rvals + lo, hi - lo, next_read);
          f_r = (uint32_t)f;
          c += (uint64_t)(hi - f);
        }
        if (masked) { tally[2] = c; f_f = 0; c_f = 0; f_r = 0; c = 0; }
      }
    }
    ff[e] = f_f; cf[e] = c_f; fr[e] = f_r; cnt[e] = c;
  }
  if (CAP) cap_tally(tally, stats);
}
// one seed per thread: key = 2 (ra * nreads + rb) + strand, value = d = pos_a - pos_b with pos_b in the frame of rc(rb) on the
// minus strand.  Per pair and strand the seeds come out in (k-mer, i, j) order, which the stable sort by the key keeps.
__global__ __launch_bounds__(256) void k_self_expand_st(const uint64_t* __restrict__ off, int64_t n, int64_t nseeds,
                                                        const uint64_t* __restrict__ vals, const uint64_t* __restrict__ rvals,
                                                        const uint32_t* __restrict__ ff, const uint32_t* __restrict__ cf,
                                                        const uint32_t* __restrict__ fr, uint64_t nreads,
                                                        uint64_t* __restrict__ pkey, int32_t* __restrict__ dval) {
  const int64_t o = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (o >= nseeds) return;
  const int64_t e = upper_bound_dev<uint64_t>(off, n, (uint64_t)o) - 1;
  const uint64_t t = (uint64_t)o - off[e];
  const uint64_t nf = cf[e];
  const uint64_t va = vals[e];
  const uint64_t vb = t < nf ? vals[(uint64_t)ff[e] + t] : rvals[(uint64_t)fr[e] + (t - nf)];
  pkey[o] = (((va >> 32) * nreads + (vb >> 32)) << 1) | (t < nf ? 0ull : 1ull);
  dval[o] = (int32_t)(uint32_t)va - (int32_t)(uint32_t)vb;
}
// per candidate pair (unique key u, seeds [soff[u], soff[u] + scount[u])): its reads, histogram base, first diagonal
// (ST = 1: the key carries the strand in its lowest bit, written to ps)
template <int ST>
__global__ __launch_bounds__(256) void k_cand_pairs(const uint64_t* __restrict__ ukeys, const uint64_t* __restrict__ soff,
                                                    const int32_t* __restrict__ dval, int64_t np, uint64_t nreads,
                                                    const uint64_t* __restrict__ roff, const int32_t* __restrict__ rlen,
                                                    const uint64_t* __restrict__ hbase, DPair* __restrict__ pairs,
                                                    int32_t* __restrict__ d_first, int32_t* __restrict__ pa, int32_t* __restrict__ pb,
                                                    uint8_t* __restrict__ ps) {
  const int64_t u = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (u >= np) return;
  const uint64_t key = ukeys[u] >> ST;
  const uint64_t a = key / nreads, b = key % nreads;
  pairs[u] = DPair{roff[a], roff[b], rlen[a], rlen[b], hbase[u]};
  d_first[u] = dval[soff[u]];
  pa[u] = (int32_t)a; pb[u] = (int32_t)b;
  if (ST) ps[u] = (uint8_t)(ukeys[u] & 1ull);
}
constexpr int kSmallPair = 64;     // pairs with at most this many seeds are scored by one wavefront, without a histogram
constexpr int kMediumPair = 2048;  // all-pairs path: up to this many seeds by one workgroup from the seed list (k_band_medium)
template <int ST>
__global__ __launch_bounds__(256) void k_pair_hsize(const uint64_t* __restrict__ ukeys, const unsigned long long* __restrict__ cnt,
                                                    int64_t np, uint64_t nreads, const int32_t* __restrict__ rlen,
                                                    uint64_t* __restrict__ hsize, int sparse_max) {
  const int64_t u = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (u >= np) return;
  const uint64_t key = ukeys[u] >> ST;
  hsize[u] = cnt[u] <= (unsigned long long)sparse_max ? 0ull : (uint64_t)rlen[key / nreads] + (uint64_t)rlen[key % nreads] + 1;
}
// seeds [s0, s1) belong to the pairs [u0, u1) of this chunk; hbase is relative to the chunk's first histogram entry
__global__ __launch_bounds__(256) void k_scatter_hist(const int32_t* __restrict__ dval, int64_t s0, int64_t s1,
                                                      const uint64_t* __restrict__ soff, int64_t u0, int64_t u1,
                                                      const DPair* __restrict__ pairs, uint64_t hchunk0, uint32_t* __restrict__ hist,
                                                      int sparse_max) {
  const int64_t o = s0 + (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (o >= s1) return;
  const int64_t u = u0 + upper_bound_dev<uint64_t>(soff + u0, u1 - u0, (uint64_t)o) - 1;
  if ((u + 1 < u1 ? soff[u + 1] : (uint64_t)s1) - soff[u] <= (uint64_t)sparse_max) return;     // no histogram for sparse pairs
  const DPair pr = pairs[u];
  atomicAdd(&hist[pr.hbase - hchunk0 + (uint64_t)(dval[o] + pr.t_len)], 1u);
}

// K8d: a pair with at most 64 seeds is scored by ONE wavefront straight from its seed list (lane l = seed l, in table
// order): the shared window, score, ordering and tie rule; the neighbour count by a shuffle loop over the lanes.
// Seeds of pair u: dval[soff[u] + l] in table order (all-pairs path, soff != nullptr) or dval[64 u + l] in arbitrary order
// with the first row's diagonal given in d_first (pair-list path).
__global__ __launch_bounds__(256) void k_band_small(const DPair* __restrict__ pairs, const uint64_t* __restrict__ soff,
                                                    const unsigned long long* __restrict__ cnt, const int32_t* __restrict__ dval,
                                                    const int32_t* __restrict__ d_first, int64_t np, BandConst c,
                                                    pw_overlap_band* __restrict__ out) {
  const int64_t u = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 6;
  const int l = (int)(threadIdx.x & 63u);
  if (u >= np) return;
  const int ns = (int)(cnt[u] > 64ull ? 65 : cnt[u]);
  if (ns > kSmallPair) return;
  const DPair pr = pairs[u];
  const int ls = pr.s_len, lt = pr.t_len;
  const bool valid = l < ns;
  const int d = valid ? dval[(soff ? soff[u] : (uint64_t)u * 64ull) + (uint64_t)l] : kNoDiag;
  if (ns == 0) return;
  int L = 1, r = 1, first = 0, last = 0;
  if (valid) ov_window(d, ls, lt, c, L, r, first, last);
  int n = -1; bool rep = valid;
  for (int j = 0; j < ns; j++) {
    const int dj = __shfl(d, j, 64);
    n += (valid && dj >= first && dj <= last) ? 1 : 0;
    rep = rep && !(j < l && dj == d);              // the first lane of every occupied diagonal represents it
  }
  const double w = valid ? band_w(n, r, L, c.p0) : 0.0;
  Best best{w, rep ? d : kNoDiag};                   // the best occupied diagonal: a butterfly over the representatives
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const Best o{__shfl_xor(best.w, off, 64), __shfl_xor(best.d, off, 64)};
    if (better(o, best)) best = o;
  }
  const double bw = best.w; const int bd = best.d;
  const unsigned long long tie_mask = __ballot(rep && ties(bw, tie_threshold(bw), w));
  const unsigned long long win_mask = __ballot(rep && d == bd);
  const int wl = __ffsll((long long)win_mask) - 1;
  const int rb = __shfl(r, wl, 64), Lb = __shfl(L, wl, 64), nb = __shfl(n, wl, 64);
  const int d0 = d_first ? d_first[u] : __shfl(d, 0, 64);
  const int fl = __ffsll((long long)__ballot(valid && d == d0)) - 1;      // a seed on the first row's diagonal
  const int r0 = __shfl(r, fl, 64), L0 = __shfl(L, fl, 64), n0 = __shfl(n, fl, 64);
  const unsigned long long band_b = __ballot(valid && d >= bd - rb && d <= bd + rb);
  const unsigned long long band_f = __ballot(valid && d >= d0 - r0 && d <= d0 + r0);
  if (l == 0)
    out[u] = band_record(ns, bw, (int)__popcll(tie_mask), BandSide{bd, nb, Lb, rb, (int)__popcll(band_b)},
                         BandSide{d0, n0, L0, r0, (int)__popcll(band_f)});
}

// K8e: a pair with 65 .. kMediumPair seeds is scored by ONE workgroup straight from its seed list in LDS (all-pairs path):
// the shared window, score, ordering and tie rule per occupied diagonal -- the neighbour count by a loop over the list instead
// of a prefix-summed histogram of |S| + |T| + 1 counters per pair (10 001 for 5 kb reads: reading and summing them was the
// bulk of the dense kernel's time, for the ~250 seeds of a true overlap).  The first seed of every occupied diagonal
// represents it.
__global__ __launch_bounds__(256) void k_list_medium(const unsigned long long* __restrict__ cnt, int64_t np, unsigned long long* __restrict__ n_list,
                                                     int64_t* __restrict__ list) {
  const int64_t u = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (u >= np) return;
  if (cnt[u] > (unsigned long long)kSmallPair && cnt[u] <= (unsigned long long)kMediumPair) list[atomicAdd(n_list, 1ull)] = u;
}
__global__ __launch_bounds__(256) void k_band_medium(const DPair* __restrict__ pairs, const int64_t* __restrict__ list,
                                                     const uint64_t* __restrict__ soff, const unsigned long long* __restrict__ cnt,
                                                     const int32_t* __restrict__ dval, const int32_t* __restrict__ d_first, BandConst c,
                                                     pw_overlap_band* __restrict__ out) {
  constexpr int PER = kMediumPair / 256;
  __shared__ int s_dv[kMediumPair];
  __shared__ double s_w[256];
  __shared__ int s_d[256], s_sum[3 * 256];
  __shared__ int s_best[3], s_first[3];
  const int64_t u = list[blockIdx.x];
  const int tid = (int)threadIdx.x;
  const int ns = (int)cnt[u];
  const DPair pr = pairs[u];
  const int ls = pr.s_len, lt = pr.t_len;
  const uint64_t base = soff[u];
  for (int l = tid; l < ns; l += 256) s_dv[l] = dval[base + (uint64_t)l];
  __syncthreads();
  const int d0 = d_first[u];
  double wq[PER];
  unsigned repmask = 0;
  Best mine{0.0, kNoDiag};
#pragma unroll
  for (int q = 0; q < PER; q++) {
    const int l = tid + 256 * q;
    wq[q] = 0.0;
    if (l < ns) {
      const int d = s_dv[l];
      int L, r, first, last;
      ov_window(d, ls, lt, c, L, r, first, last);
      int n = -1; bool rp = true;
      for (int j = 0; j < ns; j++) {
        const int dj = s_dv[j];
        n += (dj >= first && dj <= last) ? 1 : 0;
        rp = rp && !(j < l && dj == d);
      }
      const double w = band_w(n, r, L, c.p0);
      wq[q] = w;
      if (rp) {
        repmask |= 1u << q;
        if (better(Best{w, d}, mine)) mine = Best{w, d};
      }
      if (d == d0 && rp) { s_first[0] = n; s_first[1] = L; s_first[2] = r; }       // (one representative per diagonal)
    }
  }
  const Best best = block_best(mine, s_w, s_d, tid);
  const double wbest = best.w; const int dbest = best.d;
  const double thr = tie_threshold(wbest);
  int sum[3] = {0, 0, 0};                                                           // ties, seeds of the best band, of the first row's
#pragma unroll
  for (int q = 0; q < PER; q++) {
    const int l = tid + 256 * q;
    if (l < ns && (repmask >> q & 1u)) {
      sum[0] += ties(wbest, thr, wq[q]) ? 1 : 0;
      if (s_dv[l] == dbest) {                                                       // the best diagonal's representative
        int L, r, first, last;
        ov_window(dbest, ls, lt, c, L, r, first, last);
        int n = -1;
        for (int j = 0; j < ns; j++) n += (s_dv[j] >= first && s_dv[j] <= last) ? 1 : 0;
        s_best[0] = n; s_best[1] = L; s_best[2] = r;
      }
    }
  }
  __syncthreads();
  const int rb = s_best[2], r0 = s_first[2];
  for (int l = tid; l < ns; l += 256) {
    const int d = s_dv[l];
    sum[1] += (d >= dbest - rb && d <= dbest + rb) ? 1 : 0;
    sum[2] += (d >= d0 - r0 && d <= d0 + r0) ? 1 : 0;
  }
  block_sum(sum, s_sum, tid);
  if (tid == 0)
    out[u] = band_record(ns, wbest, sum[0], BandSide{dbest, s_best[0], s_best[1], rb, sum[1]},
                         BandSide{d0, s_first[0], s_first[1], r0, sum[2]});
}

// ---- host helpers: everything runs on the null stream --------------------------------------------------------------
// strand (host, one byte per pair of the chunk) and d_comp are null on the forward-only path
int run_chunk(const uint8_t* d_arena, const pw_read_pair* pairs, int64_t n, int L, int k, int kbits, BandConst bc,
              pw_overlap_band* out, hipEvent_t ev0, hipEvent_t ev1, float* ms, const uint8_t* strand = nullptr,
              const uint8_t* d_comp = nullptr) {
  std::vector<DPair> hp((size_t)n);
  std::vector<uint64_t> ss((size_t)n + 1), ts((size_t)n + 1);
  uint64_t hb = 0, cs = 0, ct = 0;
  for (int64_t p = 0; p < n; p++) {
    hp[(size_t)p] = DPair{pairs[p].s_off, pairs[p].t_off, pairs[p].s_len, pairs[p].t_len, hb};
    hb += (uint64_t)pairs[p].s_len + (uint64_t)pairs[p].t_len + 1;
    ss[(size_t)p] = cs; ts[(size_t)p] = ct;
    cs += pairs[p].s_len >= k ? (uint64_t)(pairs[p].s_len - k + 1) : 0;
    ct += pairs[p].t_len >= k ? (uint64_t)(pairs[p].t_len - k + 1) : 0;
  }
  ss[(size_t)n] = cs; ts[(size_t)n] = ct;
  DeviceArray<DPair> dp; DeviceArray<uint64_t> dss, dts, kin, ksb, ktb; DeviceArray<uint32_t> pin, psb, ptb, hist, first;
  DeviceArray<uint8_t> dstrand; DeviceArray<unsigned long long> rows; DeviceArray<int32_t> dlist, dfirst;     // dlist: 64 diagonals per pair
  DeviceArray<pw_overlap_band> dout; DeviceBuffer tmp;
  CHECK(kin.ensure((size_t)std::max(cs, ct))); CHECK(pin.ensure((size_t)std::max(cs, ct)));
  CHECK(ksb.ensure((size_t)cs)); CHECK(psb.ensure((size_t)cs)); CHECK(ktb.ensure((size_t)ct)); CHECK(ptb.ensure((size_t)ct));
  CHECK(hist.ensure((size_t)hb)); CHECK(rows.ensure((size_t)n)); CHECK(first.ensure((size_t)n));
  CHECK(dout.ensure((size_t)n)); CHECK(dlist.ensure(64 * (size_t)n));
  if (upload(set_err, dp, hp.data(), (size_t)n) != 0 || upload(set_err, dss, ss.data(), (size_t)n + 1) != 0 ||
      upload(set_err, dts, ts.data(), (size_t)n + 1) != 0 || (strand && upload(set_err, dstrand, strand, (size_t)n) != 0))
    return -1;
  CHECK(hipEventRecord(ev0, nullptr));
  CHECK(hipMemsetAsync(hist.p, 0, hist.bytes((size_t)hb), nullptr));
  CHECK(hipMemsetAsync(rows.p, 0, rows.bytes((size_t)n), nullptr));
  CHECK(hipMemsetAsync(first.p, 0xff, first.bytes((size_t)n), nullptr));
  const int pbits = bits_for((uint64_t)n);
  for (int side = 0; side < 2; side++) {
    const uint64_t tot = side ? ct : cs;
    if (tot == 0) continue;
    if (side && strand)
      hipLaunchKernelGGL(k_enc_batch_rc, rows_grid(tot), kBlock256, 0, nullptr, d_arena, dp.p, dts.p, n, (int64_t)tot, dstrand.p, d_comp, k,
                         L, kbits, kin.p, pin.p);
    else
      hipLaunchKernelGGL(k_enc_batch, rows_grid(tot), kBlock256, 0, nullptr, d_arena, dp.p, side ? dts.p : dss.p, n, (int64_t)tot, side, k, L,
                         kbits, kin.p, pin.p);
    CHECK(sort_pairs(tmp, kin, side ? ktb : ksb, pin, side ? ptb : psb, (size_t)tot, kbits + pbits));
  }
  if (cs && ct)
    hipLaunchKernelGGL(k_join_hist, rows_grid(cs), kBlock256, 0, nullptr, ksb.p, psb.p, (int64_t)cs, ktb.p, ptb.p, (int64_t)ct, dp.p, kbits,
                       hist.p, rows.p, first.p, dlist.p);
  CHECK(dfirst.ensure((size_t)n));
  hipLaunchKernelGGL(k_first_d, rows_grid((uint64_t)n), kBlock256, 0, nullptr, first.p, n, ksb.p, psb.p, ktb.p, ptb.p, (int64_t)ct, dfirst.p);
  hipLaunchKernelGGL(k_band_small, rows_grid((uint64_t)n * 64), kBlock256, 0, nullptr, dp.p, (const uint64_t*)nullptr, rows.p, dlist.p,
                     dfirst.p, n, bc, dout.p);
  hipLaunchKernelGGL(k_band_select, dim3((unsigned)n), kBlock256, 0, nullptr, dp.p, hist.p, rows.p, dfirst.p, (uint64_t)0, kSmallPair, bc,
                     dout.p);
  CHECK(hipEventRecord(ev1, nullptr));
  CHECK(hipMemcpy(out, dout.p, dout.bytes((size_t)n), hipMemcpyDeviceToHost));
  CHECK(hipGetLastError());
  float t = 0.f;
  CHECK(hipEventElapsedTime(&t, ev0, ev1));
  *ms += t;
  return 0;
}

// ---- all reads against all reads (K9): one call, stage by stage on the null stream ----------------------------------------
// sel: 1 forward pairs only (d_comp and pair_strand unused: the kernels and keys of the unstranded call), 2 minus pairs only,
// 3 both.  With sel != 1 a second index of the same size holds the reverse-strand k-mers and the pair key carries the strand.
// The buffers are listed under the stage that fills them; all of them live until the call returns, so none is freed between
// the two events.
struct AllPairs {
  const uint8_t* d_arena; const uint8_t* d_comp;
  int64_t R; int L, k, kbits, sel, shard_rank, shard_world; int64_t max_pairs; BandConst bc;
  uint32_t max_occ;                                    // 0: no cap, K9b / K9b' as they always were
  int window;                                          // above 1: the index holds the window minimizers only (pw_minimizer.h)
  MiniSample mini;                                     // (window > 1) the selection: K15a's bitmap and ranks, the reads' sampled starts
  uint64_t positions = 0;                              // forward positions of the read set: K before sampling
  pw_overlap_cap_stats cap{};                          // (max_occ != 0) filled by self_join
  DeviceArray<unsigned long long> dstats;              // the three counters of the cap
  bool st = false;                                     // sel != 1
  uint64_t K = 0, NS = 0;                              // k-mers per index, seeds
  unsigned long long NP = 0;                           // candidate pairs
  const dim3 blk = kBlock256;
  DeviceArray<uint64_t> droff, drstart; DeviceArray<int32_t> drlen; DeviceBuffer tmp;   // the reads (run); rocPRIM's scratch, one for the whole call
  DeviceArray<uint64_t> kin, vin, ks, vs, kr, vr;      // build_index: staging, the forward index, the reverse-strand index
  DeviceArray<uint32_t> fs, fr, cf; DeviceArray<uint64_t> cnt, off, pk_in, pk; DeviceArray<int32_t> dv_in, dv;   // self_join: (pair key, d) per seed
  DeviceArray<uint64_t> uk, soff, hsize, hbase; DeviceArray<unsigned long long> uc, nruns;                       // group_pairs: the candidate pairs
  DeviceArray<DPair> dpairs; DeviceArray<int32_t> dfirst, dpa, dpb; DeviceArray<uint8_t> dps;
  DeviceArray<pw_overlap_band> dout; DeviceArray<uint32_t> hist;                                                 // score_tiers: the records

  // Stage 1, once per strand: K9a (K9a' for the reverse strand) into kin / vin, then the stable sort by k-mer.
  // Sampled: K15b writes the selected rows of the strand instead (the reverse strand from the same flags, after K15c).
  int build_index(bool reverse) {
    if (window > 1) {
      mini.emit(reverse, d_arena, droff.p, drstart.p, R, k, L, d_comp, kin.p, vin.p, nullptr);
      if (!reverse && st) mini.read_starts(vin.p, R, nullptr);     // K15c, while vin holds the forward hits in (read, pos) order
    } else if (reverse)
      hipLaunchKernelGGL(k_enc_reads_rc, rows_grid(K), blk, 0, nullptr, d_arena, droff.p, drlen.p, drstart.p, R, (int64_t)K, k, L, d_comp,
                         kin.p, vin.p);
    else
      hipLaunchKernelGGL(k_enc_reads, rows_grid(K), blk, 0, nullptr, d_arena, droff.p, drstart.p, R, (int64_t)K, k, L, kin.p, vin.p);
    CHECK(sort_pairs(tmp, kin, reverse ? kr : ks, vin, reverse ? vr : vs, (size_t)K, kbits));
    return 0;
  }

  // Stage 2: the self join (K9b, K9b') to seeds -> (pair key, d), stably sorted by the pair key.  NS stays 0 when no two reads
  // share a k-mer.
  int self_join() {
    const dim3 gK = rows_grid(K);
    const bool capped = max_occ != 0;
    if (capped) { CHECK(dstats.ensure(3)); CHECK(hipMemsetAsync(dstats.p, 0, dstats.bytes(3), nullptr)); }
    auto* const count_kernel = capped ? k_self_count<true> : k_self_count<false>;
    auto* const count_st_kernel = capped ? k_self_count_st<true> : k_self_count_st<false>;
    if (st)
      hipLaunchKernelGGL(count_st_kernel, gK, blk, 0, nullptr, ks.p, vs.p, (int64_t)K, kr.p, vr.p, sel, shard_rank, shard_world, fs.p, cf.p,
                         fr.p, cnt.p, max_occ, dstats.p);
    else
      hipLaunchKernelGGL(count_kernel, gK, blk, 0, nullptr, ks.p, vs.p, (int64_t)K, shard_rank, shard_world, fs.p, cnt.p, max_occ, dstats.p);
    CHECK(scan_u64(tmp, cnt, off, (size_t)K));
    uint64_t last_off = 0, last_cnt = 0;
    CHECK(hipMemcpy(&last_off, off.p + (K - 1), sizeof last_off, hipMemcpyDeviceToHost));
    CHECK(hipMemcpy(&last_cnt, cnt.p + (K - 1), sizeof last_cnt, hipMemcpyDeviceToHost));
    NS = last_off + last_cnt;
    if (capped) {
      unsigned long long t[3];
      CHECK(hipMemcpy(t, dstats.p, sizeof t, hipMemcpyDeviceToHost));
      // (both strands: the reverse index holds as many masked entries as the forward one, see K9b')
      cap = pw_overlap_cap_stats{(st ? 2 : 1) * K, (st ? 2 : 1) * t[0], t[1], NS, t[2]};
    }
    if (NS == 0) return 0;
    if (NS >= (1ull << 32)) { set_err("more than 2^32 seeds between the reads: use a longer word"); return -1; }
    CHECK(pk_in.ensure((size_t)NS)); CHECK(dv_in.ensure((size_t)NS)); CHECK(pk.ensure((size_t)NS)); CHECK(dv.ensure((size_t)NS));
    if (st)
      hipLaunchKernelGGL(k_self_expand_st, rows_grid(NS), blk, 0, nullptr, off.p, (int64_t)K, (int64_t)NS, vs.p, vr.p, fs.p, cf.p, fr.p,
                         (uint64_t)R, pk_in.p, dv_in.p);
    else
      hipLaunchKernelGGL(k_self_expand, rows_grid(NS), blk, 0, nullptr, off.p, (int64_t)K, (int64_t)NS, vs.p, fs.p, (uint64_t)R, pk_in.p,
                         dv_in.p);
    const int pbits = bits_for((uint64_t)R * (uint64_t)R) + (st ? 1 : 0);       // (the strand bit below the pair rank)
    CHECK(sort_pairs(tmp, pk_in, pk, dv_in, dv, (size_t)NS, pbits));
    return 0;
  }

  // Stage 3: the sorted seeds grouped into candidate pairs -- unique pair keys with their seed counts, then seed offsets,
  // histogram bases and DPairs.
  int group_pairs() {
    CHECK(uk.ensure((size_t)NS)); CHECK(uc.ensure((size_t)NS)); CHECK(nruns.ensure(1));
    CHECK(rocprim_run(tmp, [&](void* t, size_t& b) {
      return rocprim::run_length_encode(t, b, pk.cp(), (unsigned int)NS, uk.p, uc.p, nruns.p, (hipStream_t) nullptr);
    }));
    CHECK(hipMemcpy(&NP, nruns.p, sizeof NP, hipMemcpyDeviceToHost));
    if ((int64_t)NP > max_pairs) {
      char msg[160];
      snprintf(msg, sizeof msg, "%llu pairs of reads share a seed (capacity %lld): raise max_pairs or the word length", NP, (long long)max_pairs);
      set_err(msg);
      return -1;
    }
    if (st) CHECK(dps.ensure((size_t)NP));
    CHECK(soff.ensure((size_t)NP)); CHECK(hsize.ensure((size_t)NP)); CHECK(hbase.ensure((size_t)NP));
    CHECK(dpairs.ensure((size_t)NP)); CHECK(dfirst.ensure((size_t)NP)); CHECK(dpa.ensure((size_t)NP));
    CHECK(dpb.ensure((size_t)NP));
    const dim3 gP = rows_grid(NP);
    CHECK(scan_u64(tmp, uc, soff, (size_t)NP));
    auto* const hsize_kernel = st ? k_pair_hsize<1> : k_pair_hsize<0>;
    auto* const cand_kernel = st ? k_cand_pairs<1> : k_cand_pairs<0>;
    hipLaunchKernelGGL(hsize_kernel, gP, blk, 0, nullptr, uk.p, uc.p, (int64_t)NP, (uint64_t)R, drlen.p, hsize.p, kMediumPair);
    CHECK(scan_u64(tmp, hsize, hbase, (size_t)NP));
    hipLaunchKernelGGL(cand_kernel, gP, blk, 0, nullptr, uk.p, soff.p, dv.p, (int64_t)NP, (uint64_t)R, droff.p, drlen.p, hbase.p, dpairs.p,
                       dfirst.p, dpa.p, dpb.p, dps.p);
    return 0;
  }

  // Stage 4: every candidate pair's record, by the tier its seed count puts it in.
  int score_tiers() {
    const dim3 gP = rows_grid(NP);
    CHECK(dout.ensure((size_t)NP));
    hipLaunchKernelGGL(k_band_small, rows_grid(NP * 64), blk, 0, nullptr, dpairs.p, soff.p, uc.p, dv.p, (const int32_t*)nullptr, (int64_t)NP,
                       bc, dout.p);
    // pairs with 65 .. kMediumPair seeds: one workgroup each, from the seed list
    {
      DeviceArray<int64_t> mlist; DeviceArray<unsigned long long> mcount;
      CHECK(mlist.ensure((size_t)NP)); CHECK(mcount.ensure(1));
      CHECK(hipMemsetAsync(mcount.p, 0, mcount.bytes(1), nullptr));
      hipLaunchKernelGGL(k_list_medium, gP, blk, 0, nullptr, uc.p, (int64_t)NP, mcount.p, mlist.p);
      unsigned long long NM = 0;
      CHECK(hipMemcpy(&NM, mcount.p, sizeof NM, hipMemcpyDeviceToHost));
      if (NM) hipLaunchKernelGGL(k_band_medium, dim3((unsigned)NM), blk, 0, nullptr, dpairs.p, mlist.p, soff.p, uc.p, dv.p, dfirst.p, bc, dout.p);
      CHECK(hipDeviceSynchronize());                      // (mlist is freed at the end of this scope)
    }
    // chunks of pairs whose histograms fit 2^30 counters (none at all when no pair has more than kMediumPair seeds)
    uint64_t last_base = 0, last_size = 0;
    if (NP) {
      CHECK(hipMemcpy(&last_base, hbase.p + (NP - 1), sizeof last_base, hipMemcpyDeviceToHost));
      CHECK(hipMemcpy(&last_size, hsize.p + (NP - 1), sizeof last_size, hipMemcpyDeviceToHost));
    }
    const bool any_hist = last_base + last_size > 0;
    const size_t NPh = any_hist ? (size_t)NP : 0;
    std::vector<uint64_t> h_hbase(NPh), h_soff(NPh), h_hsize(NPh);
    if (any_hist) {
      CHECK(hipMemcpy(h_hbase.data(), hbase.p, hbase.bytes(NPh), hipMemcpyDeviceToHost));
      CHECK(hipMemcpy(h_soff.data(), soff.p, soff.bytes(NPh), hipMemcpyDeviceToHost));
      CHECK(hipMemcpy(h_hsize.data(), hsize.p, hsize.bytes(NPh), hipMemcpyDeviceToHost));
    }
    const uint64_t cap = 1ull << 30;
    for (uint64_t u0 = 0; any_hist && u0 < NP;) {
      uint64_t u1 = u0, tot = 0;
      while (u1 < NP && (u1 == u0 || tot + h_hsize[(size_t)u1] <= cap)) { tot += h_hsize[(size_t)u1]; u1++; }
      if (tot == 0) { u0 = u1; continue; }                 // no pair of this chunk needs a histogram
      CHECK(hist.ensure((size_t)tot));
      CHECK(hipMemsetAsync(hist.p, 0, hist.bytes((size_t)tot), nullptr));
      const uint64_t s0 = h_soff[(size_t)u0], s1 = u1 < NP ? h_soff[(size_t)u1] : NS;
      hipLaunchKernelGGL(k_scatter_hist, rows_grid(s1 - s0), blk, 0, nullptr, dv.p, (int64_t)s0, (int64_t)s1, soff.p, (int64_t)u0, (int64_t)u1,
                         dpairs.p, h_hbase[(size_t)u0], hist.p, kMediumPair);
      hipLaunchKernelGGL(k_band_select, dim3((unsigned)(u1 - u0)), blk, 0, nullptr, dpairs.p + u0, hist.p, uc.p + u0, dfirst.p + u0,
                         h_hbase[(size_t)u0], kMediumPair, bc, dout.p + u0);
      u0 = u1;
    }
    return 0;
  }

  int run(const uint64_t* read_off, const int32_t* read_len, int32_t* pair_a, int32_t* pair_b, uint8_t* pair_strand, pw_overlap_band* out,
          int64_t* n_out, float* ms) {
    st = sel != 1;
    std::vector<uint64_t> rstart((size_t)R + 1);
    for (int64_t r = 0; r < R; r++) { rstart[(size_t)r] = K; K += read_len[r] >= k ? (uint64_t)(read_len[r] - k + 1) : 0; }
    rstart[(size_t)R] = K;
    *n_out = 0;
    if (K == 0) return 0;
    if (K >= (1ull << 32)) {
      set_err(st ? "more than 2^32 k-mers in one index: split the read set (with the reverse strand the index holds twice the entries, "
                   "2^32 per strand)"
                 : "more than 2^32 k-mers in one index: split the read set");
      return -1;
    }
    positions = K;
    DeviceEvent ev0, ev1, evs0, evs1;
    CHECK(ev0.create()); CHECK(ev1.create());
    auto upload_reads = [&]() -> int {
      return upload(set_err, droff, read_off, (size_t)R) != 0 || upload(set_err, drlen, read_len, (size_t)R) != 0 ||
                     upload(set_err, drstart, rstart.data(), (size_t)R + 1) != 0
                 ? -1 : 0;
    };
    float ms_sample = 0.f;
    if (window > 1) {
      // The selection comes first: K15a, its scan, and the host waits for the number of rows, which becomes K -- the index and
      // everything behind it are sized by it.  Timed by its own pair of events, so that still no allocation is timed.
      CHECK(evs0.create()); CHECK(evs1.create());
      if (mini.reserve(set_err, R, K) != 0 || upload_reads() != 0) return -1;
      CHECK(hipEventRecord(evs0.e, nullptr));
      if (mini.count(set_err, tmp, d_arena, droff.p, drstart.p, R, K, k, L, window, st, d_comp, nullptr) != 0) return -1;
      CHECK(hipEventRecord(evs1.e, nullptr));
      CHECK(hipEventSynchronize(evs1.e));
      CHECK(hipEventElapsedTime(&ms_sample, evs0.e, evs1.e));
      K = mini.rows;
    }
    // what the forward strand needs is allocated before the first event: no allocation of it is timed
    CHECK(kin.ensure((size_t)K)); CHECK(vin.ensure((size_t)K)); CHECK(ks.ensure((size_t)K)); CHECK(vs.ensure((size_t)K));
    CHECK(fs.ensure((size_t)K)); CHECK(cnt.ensure((size_t)K)); CHECK(off.ensure((size_t)K));
    if (window <= 1 && upload_reads() != 0) return -1;
    CHECK(hipEventRecord(ev0.e, nullptr));
    if (build_index(false) != 0) return -1;
    if (st) {
      CHECK(kr.ensure((size_t)K)); CHECK(vr.ensure((size_t)K)); CHECK(fr.ensure((size_t)K)); CHECK(cf.ensure((size_t)K));
      if (build_index(true) != 0) return -1;
    }
    if (self_join() != 0) return -1;
    if (NS == 0) return 0;
    if (group_pairs() != 0 || score_tiers() != 0) return -1;
    CHECK(hipEventRecord(ev1.e, nullptr));
    CHECK(hipMemcpy(out, dout.p, dout.bytes((size_t)NP), hipMemcpyDeviceToHost));
    CHECK(hipMemcpy(pair_a, dpa.p, dpa.bytes((size_t)NP), hipMemcpyDeviceToHost));
    CHECK(hipMemcpy(pair_b, dpb.p, dpb.bytes((size_t)NP), hipMemcpyDeviceToHost));
    if (st) CHECK(hipMemcpy(pair_strand, dps.p, (size_t)NP, hipMemcpyDeviceToHost));
    CHECK(hipGetLastError());
    CHECK(hipEventElapsedTime(ms, ev0.e, ev1.e));
    *ms += ms_sample;
    *n_out = (int64_t)NP;
    return 0;
  }
};

// the complement of a call (pw_complement.h), refusals into this API's error channel; an alphabet out of range passes here:
// check_args reports it
int check_complement(const uint8_t* comp, int L) { return ::check_complement(set_err, comp, L); }

// the arena on `device`, with 64 bytes of slack behind the last read
int upload_arena(int device, const uint8_t* arena, uint64_t arena_bytes, DeviceArray<uint8_t>& d_arena) {
  CHECK(hipSetDevice(device));
  CHECK(d_arena.ensure((size_t)arena_bytes + 64));
  return upload(set_err, d_arena, arena, (size_t)arena_bytes);
}

int upload_complement(const uint8_t* comp, int L, DeviceArray<uint8_t>& d_comp) { return ::upload_complement(set_err, comp, L, d_comp); }

// both all-pairs entry points; stranded: pair_strand is required and the strand selection and the complement are checked
// first (the complement only where the selection needs it), then everything in check_args' order
int all_pairs(int device, const uint8_t* arena, uint64_t arena_bytes, const uint64_t* read_off, const int32_t* read_len,
              int64_t n_reads, int alphabet_len, int wordlen, double len_coeff, double radius_coeff, double word_p_null,
              bool stranded, const uint8_t* complement, int strands, int shard_rank, int shard_world, int64_t max_pairs,
              int32_t* pair_a, int32_t* pair_b, uint8_t* pair_strand, pw_overlap_band* out, int64_t* n_out, uint32_t max_occ = 0,
              pw_overlap_cap_stats* stats = nullptr, int window = 0, pw_overlap_sample_stats* sample = nullptr) {
  if (stats) memset(stats, 0, sizeof *stats);
  if (sample) memset(sample, 0, sizeof *sample);
  if (window < 0 || window > kMiniMaxWindow) { set_err("window must be 0..128"); return -1; }
  if (stranded) {
    if (strands < PW_STRAND_PLUS || strands > PW_STRAND_BOTH) { set_err("strands must be 1 (+), 2 (-) or 3 (both)"); return -1; }
    if (strands != PW_STRAND_PLUS && check_complement(complement, alphabet_len) != 0) return -1;
  }
  int kbits = 0;
  if (check_args(set_err, alphabet_len, wordlen,
                 n_reads < 0 || n_reads >= (1ll << 31) || !n_out || (n_reads && (!read_off || !read_len)) || (stranded && !pair_strand),
                 len_coeff, radius_coeff, word_p_null, shard_world < 1 || shard_rank < 0 || shard_rank >= shard_world, n_reads,
                 [&](int64_t r) { return read_len[r] < 0 || read_off[r] + (uint64_t)read_len[r] > arena_bytes; },
                 arena, arena_bytes, &kbits) != 0)
    return -1;
  g_ms = 0.0; *n_out = 0;
  if (n_reads < 2) return 0;
  DeviceArray<uint8_t> d_arena, d_comp;
  if (upload_arena(device, arena, arena_bytes, d_arena) != 0) return -1;
  if (strands != PW_STRAND_PLUS && upload_complement(complement, alphabet_len, d_comp) != 0) return -1;
  float ms = 0.f;
  AllPairs job{d_arena.p, d_comp.p, n_reads, alphabet_len, wordlen, kbits, strands, shard_rank, shard_world,
               max_pairs, BandConst{len_coeff, radius_coeff, word_p_null}, max_occ, window};
  const int rc = job.run(read_off, read_len, pair_a, pair_b, pair_strand, out, n_out, &ms);
  if (stats) *stats = job.cap;                         // (what the join counted, also where a refusal followed it)
  if (sample) *sample = pw_overlap_sample_stats{job.positions, job.K};
  if (rc == 0 && stranded && strands == PW_STRAND_PLUS) memset(pair_strand, 0, (size_t)*n_out);
  g_ms = (double)ms;
  return rc;
}

// both pair-list entry points (strand == nullptr: every T as given, the complement is not read)
int bands(int device, const uint8_t* arena, uint64_t arena_bytes, const pw_read_pair* pairs, int64_t n_pairs, int alphabet_len,
          int wordlen, double len_coeff, double radius_coeff, double word_p_null, const uint8_t* complement, const uint8_t* strand,
          pw_overlap_band* out) {
  static_assert(sizeof(pw_overlap_band) == 64, "pw_overlap_band is 64 bytes");
  int kbits = 0;
  if (check_args(set_err, alphabet_len, wordlen, n_pairs < 0 || (n_pairs && (!pairs || !out)), len_coeff, radius_coeff, word_p_null, false,
                 n_pairs, [&](int64_t p) {
                   const pw_read_pair& r = pairs[p];
                   return r.s_len < 0 || r.t_len < 0 || r.s_off + (uint64_t)r.s_len > arena_bytes || r.t_off + (uint64_t)r.t_len > arena_bytes;
                 }, arena, arena_bytes, &kbits) != 0)
    return -1;
  g_ms = 0.0;
  if (n_pairs == 0) return 0;
  DeviceArray<uint8_t> d_arena, d_comp;
  if (upload_arena(device, arena, arena_bytes, d_arena) != 0) return -1;
  if (strand && upload_complement(complement, alphabet_len, d_comp) != 0) return -1;
  DeviceEvent ev0, ev1;
  CHECK(ev0.create()); CHECK(ev1.create());
  // chunks: at most 2^31 histogram entries, 2^31 k-mers per side and pair ids that fit beside the k-mer
  const uint64_t lim = 1ull << 31;
  const int64_t max_pairs_bits = 62 - kbits;
  float ms = 0.f;
  int rc = 0;
  for (int64_t p0 = 0; p0 < n_pairs && rc == 0;) {
    uint64_t hb = 0, cs = 0, ct = 0; int64_t p1 = p0;
    while (p1 < n_pairs) {
      const uint64_t h = (uint64_t)pairs[p1].s_len + (uint64_t)pairs[p1].t_len + 1;
      if (p1 > p0 && (hb + h > lim || cs + (uint64_t)pairs[p1].s_len > lim || ct + (uint64_t)pairs[p1].t_len > lim ||
                      (max_pairs_bits < 40 && (p1 - p0 + 1) >= (1ll << max_pairs_bits)))) break;
      hb += h; cs += (uint64_t)pairs[p1].s_len; ct += (uint64_t)pairs[p1].t_len; p1++;
    }
    rc = run_chunk(d_arena.p, pairs + p0, p1 - p0, alphabet_len, wordlen, kbits, BandConst{len_coeff, radius_coeff, word_p_null}, out + p0,
                   ev0.e, ev1.e, &ms, strand ? strand + p0 : nullptr, d_comp.p);
    p0 = p1;
  }
  g_ms = (double)ms;
  return rc;
}

// rc frames: one thread per letter
__global__ __launch_bounds__(256) void k_revcomp_frames(uint8_t* __restrict__ arena, const uint64_t* __restrict__ src,
                                                        const uint64_t* __restrict__ dst, const uint64_t* __restrict__ start,
                                                        int64_t n, int64_t total, const uint8_t* __restrict__ comp, int L) {
  __shared__ uint8_t s_comp[36];
  load_complement(comp, L, s_comp);
  const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (g >= total) return;
  const int64_t f = upper_bound_dev<uint64_t>(start, n + 1, (uint64_t)g) - 1;
  const uint64_t q = (uint64_t)g - start[f], len = start[f + 1] - start[f];
  arena[dst[f] + q] = s_comp[arena[src[f] + (len - 1 - q)]];
}

}  // namespace

extern "C" {

int pw_overlap_all_pairs(int device, const uint8_t* arena, uint64_t arena_bytes, const uint64_t* read_off, const int32_t* read_len,
                         int64_t n_reads, int alphabet_len, int wordlen, double len_coeff, double radius_coeff, double word_p_null,
                         int shard_rank, int shard_world, int64_t max_pairs, int32_t* pair_a, int32_t* pair_b, pw_overlap_band* out,
                         int64_t* n_out) {
  return all_pairs(device, arena, arena_bytes, read_off, read_len, n_reads, alphabet_len, wordlen, len_coeff, radius_coeff, word_p_null,
                   false, nullptr, PW_STRAND_PLUS, shard_rank, shard_world, max_pairs, pair_a, pair_b, nullptr, out, n_out);
}

int pw_overlap_all_pairs_stranded(int device, const uint8_t* arena, uint64_t arena_bytes, const uint64_t* read_off,
                                  const int32_t* read_len, int64_t n_reads, int alphabet_len, int wordlen, double len_coeff,
                                  double radius_coeff, double word_p_null, const uint8_t* complement, int strands, int shard_rank,
                                  int shard_world, int64_t max_pairs, int32_t* pair_a, int32_t* pair_b, uint8_t* pair_strand,
                                  pw_overlap_band* out, int64_t* n_out) {
  return all_pairs(device, arena, arena_bytes, read_off, read_len, n_reads, alphabet_len, wordlen, len_coeff, radius_coeff, word_p_null,
                   true, complement, strands, shard_rank, shard_world, max_pairs, pair_a, pair_b, pair_strand, out, n_out);
}

int pw_overlap_all_pairs_capped(int device, const uint8_t* arena, uint64_t arena_bytes, const uint64_t* read_off,
                                const int32_t* read_len, int64_t n_reads, int alphabet_len, int wordlen, double len_coeff,
                                double radius_coeff, double word_p_null, const uint8_t* complement, int strands, int shard_rank,
                                int shard_world, int64_t max_pairs, int32_t* pair_a, int32_t* pair_b, uint8_t* pair_strand,
                                pw_overlap_band* out, int64_t* n_out, uint32_t max_occ, pw_overlap_cap_stats* stats) {
  return all_pairs(device, arena, arena_bytes, read_off, read_len, n_reads, alphabet_len, wordlen, len_coeff, radius_coeff, word_p_null,
                   true, complement, strands, shard_rank, shard_world, max_pairs, pair_a, pair_b, pair_strand, out, n_out, max_occ, stats);
}

int pw_overlap_all_pairs_sampled(int device, const uint8_t* arena, uint64_t arena_bytes, const uint64_t* read_off,
                                 const int32_t* read_len, int64_t n_reads, int alphabet_len, int wordlen, double len_coeff,
                                 double radius_coeff, double word_p_null, const uint8_t* complement, int strands, int shard_rank,
                                 int shard_world, int64_t max_pairs, int32_t* pair_a, int32_t* pair_b, uint8_t* pair_strand,
                                 pw_overlap_band* out, int64_t* n_out, uint32_t max_occ, pw_overlap_cap_stats* stats, int window,
                                 pw_overlap_sample_stats* sample) {
  return all_pairs(device, arena, arena_bytes, read_off, read_len, n_reads, alphabet_len, wordlen, len_coeff, radius_coeff, word_p_null,
                   true, complement, strands, shard_rank, shard_world, max_pairs, pair_a, pair_b, pair_strand, out, n_out, max_occ, stats,
                   window, sample);
}

void* pw_overlap_arena_upload(int device, const uint8_t* host_arena, uint64_t bytes, uint64_t total_bytes, int64_t n_frames,
                              const uint64_t* src_off, const uint64_t* dst_off, const int32_t* len, const uint8_t* complement,
                              int alphabet_len) {
  auto refuse = [](const char* m) -> void* { set_err(m); return nullptr; };
  if (alphabet_len < 1 || alphabet_len > 36) return refuse("alphabet_len 1..36");
  if (check_complement(complement, alphabet_len) != 0) return nullptr;
  if (n_frames < 0 || total_bytes < bytes || (bytes && !host_arena) || (n_frames && (!src_off || !dst_off || !len))) return refuse("bad arguments");
  std::vector<uint64_t> start((size_t)n_frames + 1);
  uint64_t total = 0, floor = bytes;                   // frames ascending, disjoint, behind the uploaded letters
  for (int64_t f = 0; f < n_frames; f++) {
    if (len[f] < 0 || src_off[f] + (uint64_t)len[f] > bytes) return refuse("a read lies outside the arena");
    if (dst_off[f] % 4 != 0) return refuse("frames must start on a 4-byte boundary of the arena");
    if (dst_off[f] < floor || dst_off[f] + (uint64_t)len[f] > total_bytes)
      return refuse("reverse-complement frames must ascend without overlap between the uploaded letters and total_bytes");
    for (int32_t i = 0; i < len[f]; i++)
      if (host_arena[src_off[f] + (uint64_t)i] >= alphabet_len) return refuse("letter outside the alphabet");
    floor = dst_off[f] + (uint64_t)len[f];
    start[(size_t)f] = total; total += (uint64_t)len[f];
  }
  start[(size_t)n_frames] = total;
  auto run = [&](void* p) -> int {
    CHECK(hipMemset((uint8_t*)p + bytes, 0, (size_t)(total_bytes - bytes) + 16));
    if (bytes) CHECK(hipMemcpy(p, host_arena, (size_t)bytes, hipMemcpyHostToDevice));
    if (total == 0) return 0;
    DeviceArray<uint64_t> dsrc, ddst, dstart; DeviceArray<uint8_t> d_comp;
    const size_t nf = (size_t)n_frames;
    if (upload(set_err, dsrc, src_off, nf) != 0 || upload(set_err, ddst, dst_off, nf) != 0 || upload(set_err, dstart, start.data(), nf + 1) != 0)
      return -1;
    if (upload_complement(complement, alphabet_len, d_comp) != 0) return -1;
    hipLaunchKernelGGL(k_revcomp_frames, rows_grid(total), kBlock256, 0, nullptr, (uint8_t*)p, dsrc.p, ddst.p, dstart.p, n_frames,
                       (int64_t)total, d_comp.p, alphabet_len);
    CHECK(hipGetLastError());
    CHECK(hipDeviceSynchronize());
    return 0;
  };
  void* p = nullptr;
  if (hipSetDevice(device) != hipSuccess || hipMalloc(&p, (size_t)total_bytes + 16) != hipSuccess) {
    (void)hipGetLastError();
    return refuse("pw_overlap_arena_upload: allocation failed");
  }
  if (run(p) != 0) { (void)hipFree(p); return nullptr; }
  return p;
}

int pw_overlap_arena_read(int device, const void* dev_arena, uint64_t off, uint64_t bytes, uint8_t* host_out) {
  if (!dev_arena || (bytes && !host_out)) { set_err("bad arguments"); return -1; }
  CHECK(hipSetDevice(device));
  if (bytes) CHECK(hipMemcpy(host_out, (const uint8_t*)dev_arena + off, (size_t)bytes, hipMemcpyDeviceToHost));
  return 0;
}

const char* pw_overlap_last_error(void) { return g_err.c_str(); }
double pw_overlap_last_ms(void) { return g_ms; }

int pw_overlap_bands(int device, const uint8_t* arena, uint64_t arena_bytes, const pw_read_pair* pairs, int64_t n_pairs,
                     int alphabet_len, int wordlen, double len_coeff, double radius_coeff, double word_p_null,
                     pw_overlap_band* out) {
  return bands(device, arena, arena_bytes, pairs, n_pairs, alphabet_len, wordlen, len_coeff, radius_coeff, word_p_null, nullptr, nullptr,
               out);
}

int pw_overlap_bands_stranded(int device, const uint8_t* arena, uint64_t arena_bytes, const pw_read_pair* pairs, int64_t n_pairs,
                              int alphabet_len, int wordlen, double len_coeff, double radius_coeff, double word_p_null,
                              const uint8_t* complement, const uint8_t* strand, pw_overlap_band* out) {
  if (strand) {
    if (check_complement(complement, alphabet_len) != 0) return -1;
    for (int64_t p = 0; p < n_pairs; p++) if (strand[p] > 1) { set_err("strand flags must be 0 (+) or 1 (-)"); return -1; }
  }
  return bands(device, arena, arena_bytes, pairs, n_pairs, alphabet_len, wordlen, len_coeff, radius_coeff, word_p_null, complement, strand,
               out);
}

}  // extern "C"

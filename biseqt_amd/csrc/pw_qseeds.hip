// pw_qseeds.hip -- exact-match k-mer seeds of many queries against one reference sequence on gfx950 (C ABI:
// include/pw_qseeds.h).
//
// The reference's in-memory Word-Blot (blot.py:582-700) keeps the hits of ONE sequence per k-mer and scans each query
// left to right; its experiments call it in a loop over hundreds of short queries.  Here the loop is gone: every kernel
// below runs once over the positions, rows or boxes of ALL queries, so the number of launches and host round trips does
// not depend on the number of queries.
//   create            K5a k_encode + one stable radix sort of the reference's (k-mer, position), once per handle; for
//                     small key spaces K5b's direct-address table start[key] (k_table_fill) as well
//   K10a k_qmatch     one thread per query position in (q, j) order: the query it falls in (a windowed search over the
//                     queries' first positions), its k-mer -- none when fewer than k letters are left IN THAT QUERY --
//                     and that k-mer's run in the sorted reference (table, or two binary searches as K5b) -> rows it
//                     contributes; a saturating exclusive scan -> row offsets
//   K10a' k_qmatch_stranded  the same with a strand per listed query: a minus entry IS rc(query), and the thread at its
//                     position j' forms the k-mer from the forward letters read backwards, complemented through a table in
//                     LDS -- rc(query) is never materialised for seeding.  Everything behind K10a works on listed queries
//                     and does not know about strands
//   K10b k_qexpand    one thread per row (K5c's windowed search): (q, d, a) = (q, i - j, i + j).  Threads are in (q, j)
//                     order and a run's positions ascend (the sort is stable), so rows come out in (q, j, i) order by
//                     construction -- the order the in-memory classes list their seeds in -- with no sort of the queries
//   K10c k_qcount     seed counts of many (query, d band, a band) boxes: one wavefront per box walks the rows of the
//                     box's own query only, a ballot per 64 rows, no atomics
//   K10d k_qgraph_*   the neighbourhood graph: one radix sort of the points by (q, d, a); a query's points then occupy
//                     the same index range as its rows.  One thread per point narrows that range to the admissible
//                     diagonals (K7's test on the scaled axis) and binary-searches the a window of each; a count pass,
//                     a scan, a fill pass (CSR)
//       k_cc_*        connected components of the available rows (pw_seed_kernels.h); edges never cross queries
// All of it is memory- and latency-bound: binary searches and row traffic, no arithmetic to speak of.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <algorithm>
#include <string>
#include <vector>
#include <rocprim/rocprim.hpp>

#include "../../include/pw_qseeds.h"
#include "pw_complement.h"
#include "pw_seed_host.h"

namespace {

thread_local std::string g_err;
void set_err(const std::string& s) { g_err = s; }
#define CHECK(call) PW_HIP_CHECK(set_err, call)

// (SatAdd: pw_seed_host.h; bits_for: pw_hip_host.h)

// ---- K10a -----------------------------------------------------------------------------------------------
// pstart[q] = number of positions of the queries before q (pstart[nq] = npos); position t belongs to the last query whose
// pstart is <= t (empty queries share their successor's pstart and are never chosen).  The workgroup's window of queries
// comes from two searches over all of pstart, then every thread searches inside it.
template <typename K>
__global__ __launch_bounds__(256) void k_qmatch(const uint8_t* __restrict__ arena, const int64_t* __restrict__ qoff,
                                                const int32_t* __restrict__ qlen, const int64_t* __restrict__ pstart, int64_t nq,
                                                int64_t npos, int k, int L, const K* __restrict__ rkeys, int64_t nkr,
                                                const uint32_t* __restrict__ tab, uint32_t* __restrict__ qid,
                                                uint32_t* __restrict__ lo_out, uint64_t* __restrict__ cnt, int* __restrict__ bad) {
  __shared__ int64_t win[2];
  const int64_t t0 = (int64_t)blockIdx.x * 256;
  const int64_t tlast = (t0 + 256 < npos ? t0 + 256 : npos) - 1;
  if (threadIdx.x == 0) win[0] = upper_bound_dev<int64_t>(pstart, nq + 1, t0) - 1;
  if (threadIdx.x == 64) win[1] = upper_bound_dev<int64_t>(pstart, nq + 1, tlast) - 1;
  __syncthreads();
  const int64_t t = t0 + threadIdx.x;
  if (t >= npos) return;
  const int64_t q = win[0] + upper_bound_dev<int64_t>(pstart + win[0], win[1] - win[0] + 1, t) - 1;
  const int64_t j = t - pstart[q];
  const int64_t len = qlen[q];
  qid[t] = (uint32_t)q;
  uint64_t c = 0;
  uint32_t lo32 = 0;
  if (j + k <= len) {                             // fewer than k letters left in this query: no k-mer here
    const uint8_t* __restrict__ s = arena + qoff[q] + j;
    uint64_t v = 0;
    bool ok = true;
    for (int i = 0; i < k; i++) {
      const uint32_t ch = s[i];
      ok = ok && ch < (uint32_t)L;
      v = v * (uint64_t)L + ch;
    }
    if (!ok) *bad = 1;
    else {
      const K key = (K)v;
      int64_t lo, hi;
      if (tab != nullptr) { lo = tab[v]; hi = tab[v + 1]; }
      else { lo = lower_bound_dev<K>(rkeys, nkr, key); hi = lo + upper_bound_dev<K>(rkeys + lo, nkr - lo, key); }
      lo32 = (uint32_t)lo;
      c = (uint64_t)(hi - lo);
    }
  } else if (j < len) {                           // the tail of a query still holds letters: they are validated too
    if (arena[qoff[q] + j] >= (uint32_t)L) *bad = 1;
  }
  lo_out[t] = lo32;
  cnt[t] = c;
}
// K10a', one strand per listed query: entry q with strand[q] != 0 is T = rc(query q), and position j' of T is letter
// len - 1 - j' of the query, complemented.  The k-mer at j' is comp(s[len - 1 - j']), comp(s[len - 2 - j']), ... : the letters
// [len - j' - k, len - j') of the query read backwards, so nothing below offsets[q] is touched; a tail position
// (j' > len - k) validates its own letter len - 1 - j', and so every letter of the query is validated on either strand.
// Wavefronts hold entries of both strands side by side: ONE loop serves both, each thread with its own first letter and
// step, and the complement is a select behind a table read every lane makes (the table in LDS, as pw_overlap.hip's).
template <typename K>
__global__ __launch_bounds__(256) void k_qmatch_stranded(const uint8_t* __restrict__ arena, const int64_t* __restrict__ qoff,
                                                         const int32_t* __restrict__ qlen, const int64_t* __restrict__ pstart,
                                                         const uint8_t* __restrict__ strand, const uint8_t* __restrict__ comp,
                                                         int64_t nq, int64_t npos, int k, int L, const K* __restrict__ rkeys,
                                                         int64_t nkr, const uint32_t* __restrict__ tab, uint32_t* __restrict__ qid,
                                                         uint32_t* __restrict__ lo_out, uint64_t* __restrict__ cnt,
                                                         int* __restrict__ bad) {
  __shared__ int64_t win[2];
  __shared__ uint8_t s_comp[36];
  const int64_t t0 = (int64_t)blockIdx.x * 256;
  const int64_t tlast = (t0 + 256 < npos ? t0 + 256 : npos) - 1;
  if (threadIdx.x == 0) win[0] = upper_bound_dev<int64_t>(pstart, nq + 1, t0) - 1;
  if (threadIdx.x == 64) win[1] = upper_bound_dev<int64_t>(pstart, nq + 1, tlast) - 1;
  load_complement(comp, L, s_comp);               // (its barrier publishes the window too)
  const int64_t t = t0 + threadIdx.x;
  if (t >= npos) return;
  const int64_t q = win[0] + upper_bound_dev<int64_t>(pstart + win[0], win[1] - win[0] + 1, t) - 1;
  const int64_t j = t - pstart[q];                // position in the listed sequence: of rc(query) for a minus entry
  const int64_t len = qlen[q];
  const bool minus = strand[q] != 0;
  const uint8_t* __restrict__ s = arena + qoff[q] + (minus ? len - 1 - j : j);   // this position's own letter
  const int64_t step = minus ? -1 : 1;
  qid[t] = (uint32_t)q;
  uint64_t c = 0;
  uint32_t lo32 = 0;
  if (j + k <= len) {                             // fewer than k letters left in this entry: no k-mer here
    uint64_t v = 0;
    bool ok = true;
    for (int i = 0; i < k; i++) {
      const uint32_t ch = s[i * step];
      ok = ok && ch < (uint32_t)L;
      const uint32_t cc = s_comp[ch < (uint32_t)L ? ch : 0u];
      v = v * (uint64_t)L + (minus ? cc : ch);
    }
    if (!ok) *bad = 1;
    else {
      const K key = (K)v;
      int64_t lo, hi;
      if (tab != nullptr) { lo = tab[v]; hi = tab[v + 1]; }
      else { lo = lower_bound_dev<K>(rkeys, nkr, key); hi = lo + upper_bound_dev<K>(rkeys + lo, nkr - lo, key); }
      lo32 = (uint32_t)lo;
      c = (uint64_t)(hi - lo);
    }
  } else if (j < len) {                           // the tail of an entry still holds letters: they are validated too
    if (s[0] >= (uint32_t)L) *bad = 1;
  }
  lo_out[t] = lo32;
  cnt[t] = c;
}
// scalar[0] = the row total (saturated), row_off[q] = first row of query q, row_off[nq] = total
__global__ __launch_bounds__(256) void k_qoffsets(const uint64_t* __restrict__ off, const uint64_t* __restrict__ cnt, int64_t npos,
                                                  const int64_t* __restrict__ pstart, int64_t nq,
                                                  unsigned long long* __restrict__ scalar, uint64_t* __restrict__ row_off) {
  const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (q > nq) return;
  const uint64_t total = npos > 0 ? SatAdd()(off[npos - 1], cnt[npos - 1]) : 0ull;
  if (q == 0) scalar[0] = total;
  const int64_t p = pstart[q];
  row_off[q] = p < npos ? off[p] : total;
}

// ---- K10b -----------------------------------------------------------------------------------------------
// As K5c: kExpRows rows per workgroup, the workgroup's window of positions found by two searches over all offsets, then
// ~10 cache-resident steps per row.
constexpr int kExpRows = 2048;
__global__ __launch_bounds__(256) void k_qexpand(const uint64_t* __restrict__ off, int64_t npos, int64_t nrows,
                                                 const uint32_t* __restrict__ qid, const int64_t* __restrict__ pstart,
                                                 const uint32_t* __restrict__ lo_in, const uint32_t* __restrict__ rpos,
                                                 int32_t* __restrict__ rows) {
  __shared__ int64_t win[2];
  const int64_t o0 = (int64_t)blockIdx.x * kExpRows;
  const int64_t olast = (o0 + kExpRows < nrows ? o0 + kExpRows : nrows) - 1;
  if (threadIdx.x == 0) win[0] = upper_bound_dev<uint64_t>(off, npos, (uint64_t)o0) - 1;
  if (threadIdx.x == 64) win[1] = upper_bound_dev<uint64_t>(off, npos, (uint64_t)olast) - 1;
  __syncthreads();
  const int64_t e0 = win[0], nwin = win[1] - win[0] + 1;
#pragma unroll 1
  for (int it = 0; it < kExpRows / 256; it++) {
    const int64_t o = o0 + it * 256 + threadIdx.x;
    if (o >= nrows) return;
    const int64_t e = e0 + upper_bound_dev<uint64_t>(off + e0, nwin, (uint64_t)o) - 1;      // last position whose first row is <= o
    const int64_t r = o - (int64_t)off[e];
    const uint32_t q = qid[e];
    const int32_t j = (int32_t)(e - pstart[q]);
    const int32_t i = (int32_t)rpos[(int64_t)lo_in[e] + r];
    rows[o * 3] = (int32_t)q; rows[o * 3 + 1] = i - j; rows[o * 3 + 2] = i + j;
  }
}

// ---- K10c -----------------------------------------------------------------------------------------------
// One wavefront per box: the rows of the box's query are contiguous, so nothing else is read.
__global__ __launch_bounds__(256) void k_qcount(const int32_t* __restrict__ rows, const uint64_t* __restrict__ row_off, int64_t nq,
                                                int64_t nboxes, const int32_t* __restrict__ bq, const int32_t* __restrict__ dmin,
                                                const int32_t* __restrict__ dmax, const int32_t* __restrict__ amin,
                                                const int32_t* __restrict__ amax, unsigned long long* __restrict__ counts) {
  const int64_t b = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= nboxes) return;
  const int lane = (int)(threadIdx.x & 63u);
  const int64_t q = bq[b];
  unsigned long long c = 0;
  if (q >= 0 && q < nq) {
    const int32_t d0 = dmin[b], d1 = dmax[b], a0 = amin[b], a1 = amax[b];
    const int64_t r1 = (int64_t)row_off[q + 1];
    for (int64_t base = (int64_t)row_off[q]; base < r1; base += 64) {
      const int64_t o = base + lane;
      bool ok = false;
      if (o < r1) {
        const int32_t d = rows[o * 3 + 1], a = rows[o * 3 + 2];
        ok = d >= d0 && d <= d1 && a >= a0 && a <= a1;
      }
      c += (unsigned long long)__popcll(__ballot(ok));
    }
  }
  if (lane == 0) counts[b] = c;
}

// ---- K10d -----------------------------------------------------------------------------------------------
// Key: query | d + d_off | a, abits for a, dbits for the diagonal, the query above them; all fields non-negative.
struct KeyLayout { int abits, dbits, d_off; };
__device__ __forceinline__ uint64_t make_key(const KeyLayout kl, uint64_t q, uint64_t dq, uint64_t a) {
  return (q << (kl.dbits + kl.abits)) | (dq << kl.abits) | a;
}
__global__ __launch_bounds__(256) void k_qgraph_keys(const int32_t* __restrict__ rows, int64_t n, KeyLayout kl,
                                                     uint64_t* __restrict__ keys, uint32_t* __restrict__ vals) {
  const int64_t o = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (o >= n) return;
  keys[o] = make_key(kl, (uint64_t)(uint32_t)rows[o * 3], (uint64_t)(uint32_t)(rows[o * 3 + 1] + kl.d_off), (uint64_t)(uint32_t)rows[o * 3 + 2]);
  vals[o] = (uint32_t)o;
}
// One thread per point in (q, d, a) order; the sorted points of query q are [row_off[q], row_off[q + 1]).  The admission
// test on the scaled axis is the KD-tree's own, fl(|fl(d c) - fl(d' c)|) <= R, as K7's; on each admitted diagonal the points
// with |a - a'| <= R form one contiguous piece.  Diagonals ascend, so every search starts where the last one ended.
template <bool FILL>
__global__ __launch_bounds__(256) void k_qgraph_scan(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ order, int64_t n,
                                                     const uint64_t* __restrict__ row_off, KeyLayout kl, int nd, double c, double R,
                                                     int win, uint32_t* __restrict__ cnt, const uint64_t* __restrict__ off,
                                                     uint32_t* __restrict__ adj) {
  const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (s >= n) return;
  const uint64_t key = keys[s];
  const uint32_t o = order[s];
  const uint64_t amask = (1ull << kl.abits) - 1, dmask = (1ull << kl.dbits) - 1;
  const uint64_t qq = key >> (kl.dbits + kl.abits);
  const int dq = (int)((key >> kl.abits) & dmask);
  const int64_t a = (int64_t)(key & amask);
  const double X = (double)(dq - kl.d_off) * c;
  const int64_t ra = (int64_t)floor(R);           // |a - a'| <= R for integers
  const int64_t alo = a - ra < 0 ? 0 : a - ra, ahi = a + ra > (int64_t)amask ? (int64_t)amask : a + ra;
  uint64_t w = FILL ? off[o] : 0;
  uint32_t total = 0;
  const int d0 = dq - win < 0 ? 0 : dq - win, d1 = dq + win > nd - 1 ? nd - 1 : dq + win;
  const int64_t qb = (int64_t)row_off[qq], qe = (int64_t)row_off[qq + 1];
  int64_t wlo = qb + lower_bound_dev<uint64_t>(keys + qb, qe - qb, make_key(kl, qq, (uint64_t)d0, 0));
  const int64_t whi = wlo + upper_bound_dev<uint64_t>(keys + wlo, qe - wlo, make_key(kl, qq, (uint64_t)d1, amask));
  for (int dd = d0; dd <= d1 && wlo < whi; dd++) {
    const double Xp = (double)(dd - kl.d_off) * c;
    if (!(fabs(X - Xp) <= R)) continue;
    const int64_t lo = wlo + lower_bound_dev<uint64_t>(keys + wlo, whi - wlo, make_key(kl, qq, (uint64_t)dd, (uint64_t)alo));
    const int64_t hi = lo + upper_bound_dev<uint64_t>(keys + lo, whi - lo, make_key(kl, qq, (uint64_t)dd, (uint64_t)ahi));
    if (!FILL) total += (uint32_t)(hi - lo);
    else for (int64_t t = lo; t < hi; t++) { const uint32_t v = order[t]; if (v != o) adj[w++] = v; }
    wlo = hi;
  }
  if (!FILL) cnt[o] = total - 1;                  // its own entry is removed (blot.py:371-372)
}

}  // namespace

struct pw_qseed_index {
  int device = 0;
  WordSpace ws;
  bool has_tab = false;                 // the direct-address table is filled
  int64_t nR = 0, nkR = 0, nq = -1, npos = 0, nrows = -1, max_qlen = 0;
  DeviceArray<uint8_t> dref; DeviceBuffer rkeys; DeviceArray<uint32_t> rpos, tab;      // the reference: filled by create (rkeys: uint32_t or uint64_t by ws.key32)
  DeviceArray<uint8_t> arena; DeviceArray<int64_t> meta; DeviceArray<uint32_t> qid, lo;  // the queries: filled by build (meta: build_queries has the layout)
  DeviceArray<uint64_t> cnt, off, row_off; DeviceArray<int32_t> rows;                 // ... rows: (query, i, j) each
  DeviceArray<unsigned long long> scalar; DeviceBuffer tmp;                           // [the row total | the bad-letter flag]; rocPRIM's scratch
  DeviceArray<uint8_t> comp;                                                  // the complement of a stranded build
  SeedGraph g;                                                                // neighbourhood graph (K10d); g.npts: the rows
  int cc_rounds = 0;
  DeviceEvent ev0, ev1;
  float ms_build = 0.f, ms_graph = 0.f, ms_cc = 0.f, ms_count = 0.f;
};

// encode + sort the reference, fill the table: everything of pw_qseeds_create that depends on the key type
template <typename K>
static int index_reference(pw_qseed_index* x) {
  DeviceBuffer keys_in; DeviceArray<uint32_t> pos_in;
  const MaskSets none = {};
  if (encode_sort<K>(set_err, x->ws, none, x->dref.p, x->nR, x->nkR, keys_in, pos_in, x->tmp, x->rkeys, x->rpos, 0, nullptr) != 0) return -1;
  if (x->nkR <= 0) return 0;
  if (table_pays(x->ws, x->nkR)) {
    if (table_fill<K>(set_err, x->ws, x->rkeys.as<const K>(), x->nkR, x->tab, nullptr) != 0) return -1;
    x->has_tab = true;
  }
  CHECK(hipDeviceSynchronize());                  // (keys_in / pos_in are freed on return)
  CHECK(hipGetLastError());
  return 0;
}

// the flag a match kernel raises at a letter outside the alphabet: an int in the second word of `scalar`
static int* bad_letter_flag(pw_qseed_index* x) { return reinterpret_cast<int*>(x->scalar.p + 1); }

template <typename K>
static void launch_match(pw_qseed_index* x, const uint8_t* arena, hipStream_t st) {
  const int64_t* meta = x->meta.p;                                 // [offsets nq | pstart nq + 1 | lengths nq (int32)]
  hipLaunchKernelGGL((k_qmatch<K>), rows_grid((uint64_t)x->npos), kBlock256, 0, st, arena, meta, (const int32_t*)(meta + 2 * x->nq + 1),
                     meta + x->nq, x->nq, x->npos, x->ws.k, x->ws.L, x->rkeys.as<const K>(), x->nkR, x->has_tab ? x->tab.p : nullptr,
                     x->qid.p, x->lo.p, x->cnt.p, bad_letter_flag(x));
}

template <typename K>
static void launch_match_stranded(pw_qseed_index* x, const uint8_t* arena, hipStream_t st) {
  const int64_t* meta = x->meta.p;                                 // [... | strands nq (uint8)] behind launch_match's block
  const int32_t* dlen = (const int32_t*)(meta + 2 * x->nq + 1);
  hipLaunchKernelGGL((k_qmatch_stranded<K>), rows_grid((uint64_t)x->npos), kBlock256, 0, st, arena, meta, dlen, meta + x->nq,
                     (const uint8_t*)(meta + 2 * x->nq + 1 + (x->nq + 1) / 2 + 1), x->comp.p, x->nq, x->npos, x->ws.k, x->ws.L,
                     x->rkeys.as<const K>(), x->nkR, x->has_tab ? x->tab.p : nullptr, x->qid.p, x->lo.p, x->cnt.p, bad_letter_flag(x));
}

// both build entry points.  strand == nullptr: pw_qseeds_build, every query as given, the complement is not read.
static int build_queries(pw_qseed_index* x, const uint8_t* arena, uint64_t arena_bytes, int arena_on_device, const int64_t* offsets,
                 const int32_t* lengths, const uint8_t* strand, const uint8_t* complement, int64_t n_queries, int64_t max_rows,
                 void* stream) {
  if (!x) { set_err("null index"); return -1; }
  if (n_queries < 0 || n_queries >= (1ll << 31)) { set_err("n_queries out of range"); return -1; }
  if (n_queries > 0 && (!offsets || !lengths)) { set_err("null offsets / lengths"); return -1; }
  if (arena_bytes > 0 && !arena) { set_err("null arena pointer"); return -1; }
  hipStream_t st = (hipStream_t)stream;
  if (max_rows <= 0) max_rows = 1ll << 30;
  max_rows = std::min<int64_t>(max_rows, (1ll << 31) - 1);
  x->nrows = -1; x->nq = -1; x->g.edges = -1; x->g.npts = -1;
  const int64_t nq = n_queries;
  bool any_minus = false;                         // (none: the unstranded kernels, and the complement is not read)
  for (int64_t q = 0; strand && q < nq; q++) {
    if (strand[q] > 1) { set_err("strand " + std::to_string(q) + " must be 0 (as given) or 1 (reverse complement)"); return -1; }
    any_minus = any_minus || strand[q] == 1;
  }
  if (any_minus && check_complement(set_err, complement, x->ws.L) != 0) return -1;
  // [offsets nq | pstart nq + 1 | lengths nq (int32) | strands nq (uint8), a stranded build's] in one block: one copy to
  // the device
  const size_t strand_at = (size_t)(2 * nq + 1 + (nq + 1) / 2 + 1);
  std::vector<int64_t> meta(strand_at + (any_minus ? (size_t)(nq + 7) / 8 : 0));
  if (any_minus) memcpy(meta.data() + strand_at, strand, (size_t)nq);
  int64_t npos = 0, max_qlen = 0;
  int32_t* hl = (int32_t*)(meta.data() + 2 * nq + 1);
  for (int64_t q = 0; q < nq; q++) {
    if (lengths[q] < 0 || offsets[q] < 0 || (uint64_t)offsets[q] + (uint64_t)lengths[q] > arena_bytes) {
      set_err("query " + std::to_string(q) + " lies outside the arena"); return -1;
    }
    meta[(size_t)q] = offsets[q];
    meta[(size_t)(nq + q)] = npos;
    hl[q] = lengths[q];
    npos += lengths[q];
    max_qlen = std::max<int64_t>(max_qlen, lengths[q]);
    if (npos >= (1ll << 31)) { set_err("the queries' lengths must sum to less than 2^31"); return -1; }
  }
  meta[(size_t)(2 * nq)] = npos;
  CHECK(hipSetDevice(x->device));
  CHECK(x->meta.ensure(meta.size()));
  CHECK(x->row_off.ensure((size_t)nq + 1));
  if (any_minus && upload_complement(set_err, complement, x->ws.L, x->comp) != 0) return -1;
  CHECK(hipEventRecord(x->ev0.e, st));            // (the build's time includes its copies to the device)
  const uint8_t* darena = arena;
  if (!arena_on_device) {
    CHECK(x->arena.ensure((size_t)arena_bytes + 64));
    if (upload(set_err, x->arena, arena, (size_t)arena_bytes, st) != 0) return -1;
    darena = x->arena.p;
  }
  if (upload(set_err, x->meta, meta.data(), meta.size(), st) != 0) return -1;
  CHECK(hipMemsetAsync(x->scalar.p, 0, x->scalar.bytes(2), st));
  x->npos = npos; x->max_qlen = max_qlen;
  const size_t np1 = (size_t)std::max<int64_t>(npos, 1);
  CHECK(x->qid.ensure(np1)); CHECK(x->lo.ensure(np1)); CHECK(x->cnt.ensure(np1)); CHECK(x->off.ensure(np1));
  x->nq = nq;                                     // (launch_match reads it; reset below on failure)
  if (npos > 0) {
    if (!any_minus) { if (x->ws.key32) launch_match<uint32_t>(x, darena, st); else launch_match<uint64_t>(x, darena, st); }
    else if (x->ws.key32) launch_match_stranded<uint32_t>(x, darena, st);
    else launch_match_stranded<uint64_t>(x, darena, st);
    CHECK(rocprim_run(x->tmp, [&](void* t, size_t& b) {
      return rocprim::exclusive_scan(t, b, x->cnt.cp(), x->off.p, (uint64_t)0, (size_t)npos, SatAdd(), st);
    }));
  }
  const int64_t* dmeta = x->meta.p;
  hipLaunchKernelGGL(k_qoffsets, rows_grid((uint64_t)nq + 1), kBlock256, 0, st, x->off.p, x->cnt.p, npos, dmeta + nq, nq, x->scalar.p,
                     x->row_off.p);
  unsigned long long res[2] = {0, 0};             // row total, bad-letter flag
  CHECK(hipMemcpyAsync(res, x->scalar.p, sizeof res, hipMemcpyDeviceToHost, st));
  CHECK(hipStreamSynchronize(st));
  x->nq = -1;
  if ((int)res[1] != 0) { set_err("letter outside the alphabet in a query"); return -1; }
  const unsigned long long total = res[0];
  if (check_row_limit(set_err, total, max_rows) != 0) return -1;
  CHECK(x->rows.ensure((size_t)std::max<unsigned long long>(total, 1) * 3));
  if (total > 0)
    hipLaunchKernelGGL(k_qexpand, dim3((unsigned)((total + kExpRows - 1) / kExpRows)), kBlock256, 0, st, x->off.p, npos, (int64_t)total,
                       x->qid.p, dmeta + nq, x->lo.p, x->rpos.p, x->rows.p);
  if (elapsed(set_err, x->ev0, x->ev1, st, &x->ms_build) != 0) return -1;
  x->nq = nq; x->nrows = (int64_t)total;
  return 0;
}

extern "C" {

const char* pw_qseeds_last_error(void) { return g_err.c_str(); }

pw_qseed_index* pw_qseeds_create(int device, const uint8_t* ref, int64_t n_ref, int alphabet_len, int wordlen) {
  WordSpace ws;
  if (check_word(set_err, alphabet_len, wordlen) != 0 || word_space(set_err, alphabet_len, wordlen, false, &ws) != 0) return nullptr;
  if (n_ref < 0 || n_ref >= (1ll << 31)) { set_err("reference length out of range (below 2^31)"); return nullptr; }
  if (n_ref > 0 && !ref) { set_err("null reference pointer"); return nullptr; }
  for (int64_t i = 0; i < n_ref; i++) if (ref[i] >= alphabet_len) { set_err("letter outside the alphabet in the reference"); return nullptr; }
  if (hipSetDevice(device) != hipSuccess) { set_err("hipSetDevice failed"); return nullptr; }
  pw_qseed_index* x = new pw_qseed_index();
  x->device = device; x->ws = ws;
  x->nR = n_ref; x->nkR = n_ref >= wordlen ? n_ref - wordlen + 1 : 0;
  if (x->dref.ensure((size_t)n_ref + 64) != hipSuccess || x->scalar.ensure(2) != hipSuccess || x->ev0.create() != hipSuccess ||
      x->ev1.create() != hipSuccess) {
    set_err("device allocation failed"); delete x; return nullptr;
  }
  if (n_ref && hipMemcpy(x->dref.p, ref, (size_t)n_ref, hipMemcpyHostToDevice) != hipSuccess) {
    set_err("copy of the reference to the device failed"); delete x; return nullptr;
  }
  if ((x->ws.key32 ? index_reference<uint32_t>(x) : index_reference<uint64_t>(x)) != 0) { delete x; return nullptr; }
  return x;
}

int pw_qseeds_build(pw_qseed_index* x, const uint8_t* arena, uint64_t arena_bytes, int arena_on_device, const int64_t* offsets,
                    const int32_t* lengths, int64_t n_queries, int64_t max_rows, void* stream) {
  return build_queries(x, arena, arena_bytes, arena_on_device, offsets, lengths, nullptr, nullptr, n_queries, max_rows, stream);
}

int pw_qseeds_build_stranded(pw_qseed_index* x, const uint8_t* arena, uint64_t arena_bytes, int arena_on_device, const int64_t* offsets,
                             const int32_t* lengths, const uint8_t* strand, const uint8_t* complement, int64_t n_queries,
                             int64_t max_rows, void* stream) {
  return build_queries(x, arena, arena_bytes, arena_on_device, offsets, lengths, strand, complement, n_queries, max_rows, stream);
}

int64_t pw_qseeds_num_queries(const pw_qseed_index* x) { return x ? x->nq : -1; }
int64_t pw_qseeds_num_rows(const pw_qseed_index* x) { return x ? x->nrows : -1; }
const int32_t* pw_qseeds_rows_device(const pw_qseed_index* x) { return (x && x->nrows >= 0) ? x->rows.p : nullptr; }
double pw_qseeds_build_ms(const pw_qseed_index* x) { return x ? (double)x->ms_build : -1.0; }
double pw_qseeds_graph_ms(const pw_qseed_index* x) { return x ? (double)x->ms_graph : -1.0; }
double pw_qseeds_components_ms(const pw_qseed_index* x) { return x ? (double)x->ms_cc : -1.0; }
double pw_qseeds_count_ms(const pw_qseed_index* x) { return x ? (double)x->ms_count : -1.0; }
int pw_qseeds_components_rounds(const pw_qseed_index* x) { return x ? x->cc_rounds : -1; }

int pw_qseeds_rows(const pw_qseed_index* x, int32_t* rows, int64_t cap) {
  if (!x || x->nrows < 0) { set_err("pw_qseeds_rows before a successful pw_qseeds_build"); return -1; }
  if (cap < x->nrows) { set_err("pw_qseeds_rows: capacity too small"); return -1; }
  CHECK(hipSetDevice(x->device));
  if (x->nrows) CHECK(hipMemcpy(rows, x->rows.p, x->rows.bytes((size_t)x->nrows * 3), hipMemcpyDeviceToHost));
  return 0;
}

int pw_qseeds_row_offsets(const pw_qseed_index* x, int64_t* row_offsets) {
  if (!x || x->nrows < 0) { set_err("pw_qseeds_row_offsets before a successful pw_qseeds_build"); return -1; }
  CHECK(hipSetDevice(x->device));
  CHECK(hipMemcpy(row_offsets, x->row_off.p, x->row_off.bytes((size_t)x->nq + 1), hipMemcpyDeviceToHost));
  return 0;
}

int pw_qseeds_count_boxes(const pw_qseed_index* xc, int64_t n_boxes, const int32_t* q, const int32_t* dmin, const int32_t* dmax,
                          const int32_t* amin, const int32_t* amax, int64_t* counts) {
  pw_qseed_index* x = const_cast<pw_qseed_index*>(xc);
  if (!x || x->nrows < 0) { set_err("pw_qseeds_count_boxes before a successful pw_qseeds_build"); return -1; }
  if (n_boxes < 0 || n_boxes >= (1ll << 31)) { set_err("n_boxes out of range"); return -1; }
  if (n_boxes == 0) return 0;
  for (int64_t b = 0; b < n_boxes; b++)
    if (q[b] < 0 || q[b] >= x->nq) { set_err("box " + std::to_string(b) + " names a query that does not exist"); return -1; }
  CHECK(hipSetDevice(x->device));
  const size_t nb = (size_t)n_boxes;
  std::vector<int32_t> h(nb * 5);                 // the five bound arrays in one block: one copy to the device
  const int32_t* src[5] = {q, dmin, dmax, amin, amax};
  for (int f = 0; f < 5; f++) memcpy(h.data() + f * nb, src[f], nb * sizeof(int32_t));
  DeviceArray<int32_t> dbox; DeviceArray<unsigned long long> dcnt;
  CHECK(dbox.ensure(h.size())); CHECK(dcnt.ensure(nb));
  if (upload(set_err, dbox, h.data(), h.size()) != 0) return -1;
  CHECK(hipEventRecord(x->ev0.e, nullptr));
  const int32_t* d = dbox.p;
  hipLaunchKernelGGL(k_qcount, dim3((unsigned)((n_boxes + 3) / 4)), kBlock256, 0, nullptr, x->rows.p, x->row_off.p, x->nq, n_boxes, d, d + nb,
                     d + 2 * nb, d + 3 * nb, d + 4 * nb, dcnt.p);
  if (elapsed(set_err, x->ev0, x->ev1, nullptr, &x->ms_count) != 0) return -1;
  CHECK(hipMemcpy(counts, dcnt.p, dcnt.bytes(nb), hipMemcpyDeviceToHost));
  return 0;
}

int64_t pw_qseeds_graph_build(pw_qseed_index* x, double d_coeff, double radius) {
  if (!x || x->nrows < 0) { set_err("pw_qseeds_graph_build before a successful pw_qseeds_build"); return -1; }
  if (!(d_coeff > 0) || !(radius >= 0)) { set_err("d_coeff must be positive and radius non-negative"); return -1; }
  SeedGraph& g = x->g;
  g.edges = -1;
  CHECK(hipSetDevice(x->device));
  const int64_t n = g.npts = x->nrows;
  if (n == 0) { g.edges = 0; x->ms_graph = 0.f; return 0; }
  // d = i - j lies in (-max query length, nR): bucket d + max_qlen in [0, nd); a = i + j below nR + max_qlen
  const int64_t nd = x->nR + x->max_qlen + 1;
  KeyLayout kl;
  kl.d_off = (int)x->max_qlen;
  kl.dbits = bits_for((uint64_t)(nd - 1));
  kl.abits = bits_for((uint64_t)(x->nR + x->max_qlen));
  const int qbits = bits_for((uint64_t)std::max<int64_t>(x->nq - 1, 1));
  if (qbits + kl.dbits + kl.abits > 64) {
    char msg[200];
    snprintf(msg, sizeof msg, "the graph's sort key needs %d + %d + %d bits (query, diagonal, antidiagonal): more than 64; "
             "use fewer queries per call", qbits, kl.dbits, kl.abits);
    set_err(msg);
    return -1;
  }
  CHECK(hipEventRecord(x->ev0.e, nullptr));
  const double wd = floor(radius / d_coeff) + 2;
  const int win = wd > (double)nd ? (int)nd : (int)wd;
  DeviceArray<uint64_t> kin; DeviceArray<uint32_t> vin;      // kin: the sort keys, then graph_finish's widened counts
  CHECK(kin.ensure((size_t)n)); CHECK(vin.ensure((size_t)n));
  const dim3 grid = rows_grid((uint64_t)n), blk = kBlock256;
  hipLaunchKernelGGL(k_qgraph_keys, grid, blk, 0, nullptr, x->rows.p, n, kl, kin.p, vin.p);
  if (graph_sort(set_err, g, x->tmp, kin, vin, n, qbits + kl.dbits + kl.abits) != 0) return -1;
  hipLaunchKernelGGL((k_qgraph_scan<false>), grid, blk, 0, nullptr, g.keys.p, g.order.p, n, x->row_off.p, kl, (int)nd, d_coeff, radius, win,
                     g.cnt.p, (const uint64_t*)nullptr, (uint32_t*)nullptr);
  const int64_t total = graph_finish(set_err, g, x->tmp, x->scalar, kin.p, n, [&] {
    hipLaunchKernelGGL((k_qgraph_scan<true>), grid, blk, 0, nullptr, g.keys.p, g.order.p, n, x->row_off.p, kl, (int)nd, d_coeff, radius, win,
                       (uint32_t*)nullptr, g.off.p, g.adj.p);
    return 0;
  });
  if (total < 0) return -1;
  if (elapsed(set_err, x->ev0, x->ev1, nullptr, &x->ms_graph) != 0) return -1;
  g.edges = total;
  return total;
}

int pw_qseeds_graph_counts(const pw_qseed_index* x, int32_t* counts, int64_t cap) {
  return graph_counts_to_host(set_err, "pw_qseeds_graph_counts", x, counts, cap);
}

int pw_qseeds_graph_fetch(const pw_qseed_index* x, int64_t* offsets, int32_t* neighbours) {
  return graph_fetch_to_host(set_err, "pw_qseeds_graph_fetch", x, offsets, neighbours);
}

int pw_qseeds_graph_components(const pw_qseed_index* xc, const uint8_t* avail, int32_t* labels) {
  pw_qseed_index* x = const_cast<pw_qseed_index*>(xc);
  return graph_components(set_err, "pw_qseeds_graph_components", x, avail, labels, x ? &x->ms_cc : nullptr, x ? &x->cc_rounds : nullptr);
}

void pw_qseeds_destroy(pw_qseed_index* x) {
  if (!x) return;
  (void)hipSetDevice(x->device);
  delete x;
}

}  // extern "C"

// pw_seeds.hip -- exact-match k-mer seeds of one pair of sequences on gfx950 (C ABI: include/pw_seeds.h).
//
// What the reference does with SQLite tables and Python generators (kmers.py:437-509, seeds.py:117-237) is a
// sort-merge join:
//   K5a k_encode   one thread per position: the k-mer as an integer in base L (kmers.py:164-210), or the
//                  "masked" key L^k when its letter set equals a mask set (kmers.py:232-236)
//       sort       (k-mer, position) of S and of T by k-mer -- stable LSD radix sort (rocPRIM), so positions stay
//                  ascending inside a k-mer, which is the reference's (seqid, pos) hit order
//   K5b k_match    one thread per sorted S element: its run of equal k-mers in T (two binary searches) -> the
//                  number of rows it contributes; exclusive scan -> row offsets
//   K5c k_expand   one thread per row: (d, a) = (i - j, i + j).  Rows come out in the reference's rowid order
//                  (k-mer asc, i asc, j asc) by construction, with no further sort
//   K5d k_count    COUNT(*) in a (d, a) band: predicate + wave reduction + one atomic per wave
// A self comparison (seeds.py:33,141-143) joins S with itself: per k-mer run the pairs i < j in combination
// order, then the trivial pairs -- an element contributes the pairs with the later elements of its run, and the
// LAST element of a run contributes the run's trivial rows.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <cstring>
#include <string>
#include <vector>
#include <rocprim/rocprim.hpp>

#include "../../include/pw_seeds.h"
#include "pw_seed_host.h"

namespace {

thread_local std::string g_err;
void set_err(const std::string& s) { g_err = s; }
#define CHECK(call) PW_HIP_CHECK(set_err, call)

// (K5a k_encode, the CSR components k_cc_*, k_widen and k_total: pw_seed_kernels.h; the host code around them: pw_seed_host.h)

// ---- K5b ------------------------------------------------------------------------------------------------
// other = sorted keys of T (or of S itself for a self comparison).  Two ways to find an element's run [lo, hi) in it:
//   * a direct-address table tab[key] = first index of `key` in `other` (k_table_fill) when the key space is small
//     (DNA, k <= 13: <= 256 MB of table, resident in the Infinity Cache): S is sorted too, so neighbouring threads read
//     neighbouring table entries -- two coalesced 4-byte reads instead of 2 log2(n) dependent ones;
//   * two binary searches otherwise.
template <typename K>
__global__ __launch_bounds__(256) void k_match(const K* __restrict__ ks, int64_t ns,
                                               const K* __restrict__ other, int64_t no, uint64_t kinv,
                                               int self, const uint32_t* __restrict__ tab, uint32_t* __restrict__ lo_out,
                                               uint64_t* __restrict__ cnt) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= ns) return;
  const K key = ks[e];
  if ((uint64_t)key >= kinv) { lo_out[e] = 0; cnt[e] = 0; return; }
  int64_t lo, hi;
  if (tab != nullptr) { lo = tab[(uint64_t)key]; hi = tab[(uint64_t)key + 1]; }
  else { lo = lower_bound_dev<K>(other, no, key); hi = upper_bound_dev<K>(other, no, key); }
  lo_out[e] = (uint32_t)lo;
  if (!self) cnt[e] = (uint64_t)(hi - lo);
  else cnt[e] = (uint64_t)(hi - 1 - e) + (e == hi - 1 ? (uint64_t)(hi - lo) : 0ull);
}
// (k_table_fill, which fills tab: pw_seed_kernels.h)

// ---- K5c ------------------------------------------------------------------------------------------------
// One thread per row, kExpRows rows per workgroup.  The element a row belongs to is found by a binary search over the
// row offsets -- inside the window of elements that the workgroup's rows span (two searches per workgroup over the whole
// array, then ~10 cache-resident steps per row instead of log2(n) scattered ones).
constexpr int kExpRows = 2048;
template <typename K>
__global__ __launch_bounds__(256) void k_expand(const uint64_t* __restrict__ off, int64_t ns, int64_t nrows,
                                                const uint32_t* __restrict__ ps, const uint32_t* __restrict__ po,
                                                const uint32_t* __restrict__ lo_in, const K* __restrict__ ks,
                                                int self, int2* __restrict__ rows) {
  __shared__ int64_t win[2];
  const int64_t o0 = (int64_t)blockIdx.x * kExpRows;
  const int64_t olast = (o0 + kExpRows < nrows ? o0 + kExpRows : nrows) - 1;
  if (threadIdx.x == 0) win[0] = upper_bound_dev<uint64_t>(off, ns, (uint64_t)o0) - 1;
  if (threadIdx.x == 64) win[1] = upper_bound_dev<uint64_t>(off, ns, (uint64_t)olast) - 1;
  __syncthreads();
  const int64_t e0 = win[0], nwin = win[1] - win[0] + 1;
#pragma unroll 1
  for (int q = 0; q < kExpRows / 256; q++) {
    const int64_t o = o0 + q * 256 + threadIdx.x;
    if (o >= nrows) return;
    const int64_t e = e0 + upper_bound_dev<uint64_t>(off + e0, nwin, (uint64_t)o) - 1;      // last element whose first row is <= o
    const int64_t r = o - (int64_t)off[e];
    int32_t i, j;
    if (!self) {
      i = (int32_t)ps[e];
      j = (int32_t)po[(int64_t)lo_in[e] + r];
    } else {
      // the run of e is [lo, hi): e pairs with e + 1 .. hi - 1; the last element of the run then lists (x, x)
      const int64_t lo = lo_in[e];
      const K key = ks[e];
      const bool last = e + 1 >= ns || ks[e + 1] != key;
      if (!last) { i = (int32_t)ps[e]; j = (int32_t)ps[e + 1 + r]; }
      else { i = (int32_t)ps[lo + r]; j = i; }
    }
    rows[o] = make_int2(i - j, i + j);
  }
}

// ---- K5d ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_count(const int2* __restrict__ rows, int64_t nrows, int have_d, int dmin,
                                               int dmax, int have_a, int amin, int amax,
                                               unsigned long long* __restrict__ out) {
  unsigned long long c = 0;
  for (int64_t o = (int64_t)blockIdx.x * 256 + threadIdx.x; o < nrows; o += (int64_t)gridDim.x * 256) {
    const int2 r = rows[o];
    const bool ok = (!have_d || (r.x >= dmin && r.x <= dmax)) && (!have_a || (r.y >= amin && r.y <= amax));
    c += ok ? 1ull : 0ull;
  }
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) c += __shfl_xor(c, s, 64);
  if ((threadIdx.x & 63u) == 0 && c) atomicAdd(out, c);
}

// ---- K6: neighbours on the scaled diagonal axis (blot.py:521-527) -------------------------------------------
__global__ __launch_bounds__(256) void k_scale(const int2* __restrict__ rows, int64_t nrows, const double* __restrict__ radius,
                                               int nT, double* __restrict__ x) {
  const int64_t o = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (o >= nrows) return;
  const int d = rows[o].x;
  x[o] = (double)d / radius[d + nT];
}
// xs sorted ascending.  The two predicates are the KD-tree's own test fl(|x - x'|) <= 1, one side each; both are
// monotone along xs (rounding is monotone), so a binary search on the predicate itself is exact.
__global__ __launch_bounds__(256) void k_neigh(const double* __restrict__ x, const double* __restrict__ xs, int64_t nrows,
                                               int32_t* __restrict__ counts) {
  const int64_t o = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (o >= nrows) return;
  const double v = x[o];
  int64_t lo = 0, hi = nrows;                     // first index with v - xs[idx] <= 1
  while (lo < hi) { const int64_t mid = (lo + hi) >> 1; if (!(v - xs[mid] <= 1.0)) lo = mid + 1; else hi = mid; }
  const int64_t first = lo;
  lo = 0; hi = nrows;                             // first index with NOT (xs[idx] - v <= 1)
  while (lo < hi) { const int64_t mid = (lo + hi) >> 1; if (xs[mid] - v <= 1.0) lo = mid + 1; else hi = mid; }
  counts[o] = (int32_t)(lo - first - 1);
}

// Self comparison: the seeds a WordBlot iterates are SeedIndex.seeds(exclude_trivial=True) (seeds.py:186-197): every
// non-trivial row (i < j, d < 0) followed by its mirror image, trivial rows (d = 0) dropped.
__global__ __launch_bounds__(256) void k_self_flag(const int2* __restrict__ rows, int64_t n, uint64_t* __restrict__ flag) {
  const int64_t o = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (o < n) flag[o] = rows[o].x != 0 ? 1ull : 0ull;
}
__global__ __launch_bounds__(256) void k_self_points(const int2* __restrict__ rows, int64_t n, const uint64_t* __restrict__ pos,
                                                     int2* __restrict__ pts) {
  const int64_t o = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (o >= n) return;
  const int2 r = rows[o];
  if (r.x == 0) return;
  pts[2 * pos[o]] = r;
  pts[2 * pos[o] + 1] = make_int2(-r.x, r.y);
}

// ---- K7: the neighbourhood graph of the seeds (blot.py:343-374) and its connected components (:452-468) ----------
__global__ __launch_bounds__(256) void k_graph_keys(const int2* __restrict__ rows, int64_t n, int nT, uint64_t* __restrict__ keys,
                                                    uint32_t* __restrict__ vals) {
  const int64_t o = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (o >= n) return;
  const int2 r = rows[o];
  keys[o] = ((uint64_t)(uint32_t)(r.x + nT) << 32) | (uint32_t)r.y;
  vals[o] = (uint32_t)o;
}
// One thread per seed in (d, a) order.  For every diagonal d' that passes the KD-tree's test on the scaled axis,
// fl(|fl(d c) - fl(d' c)|) <= R, the seeds with |a - a'| <= R form one contiguous piece of that diagonal's run.
template <bool FILL>
__global__ __launch_bounds__(256) void k_graph_scan(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ order, int64_t n,
                                                    const uint32_t* __restrict__ dstart, int nd, int nT, double c, double R, int win,
                                                    uint32_t* __restrict__ cnt, const uint64_t* __restrict__ off,
                                                    uint32_t* __restrict__ adj) {
  const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (s >= n) return;
  const uint64_t key = keys[s];
  const uint32_t o = order[s];
  const int q = (int)(key >> 32);
  const int64_t a = (int64_t)(uint32_t)key;
  const double X = (double)(q - nT) * c;
  const int64_t ra = (int64_t)floor(R);           // |a - a'| <= R for integers
  uint64_t w = FILL ? off[o] : 0;
  uint32_t total = 0;
  const int q0 = q - win < 0 ? 0 : q - win, q1 = q + win > nd - 1 ? nd - 1 : q + win;
  for (int qq = q0; qq <= q1; qq++) {
    const double Xp = (double)(qq - nT) * c;
    if (!(fabs(X - Xp) <= R)) continue;
    const int64_t b = dstart[qq], e = dstart[qq + 1];
    if (b == e) continue;
    const int64_t alo = a - ra < 0 ? 0 : a - ra, ahi = a + ra;
    const uint64_t klo = ((uint64_t)(uint32_t)qq << 32) | (uint64_t)alo;
    const uint64_t khi = ((uint64_t)(uint32_t)qq << 32) | (uint64_t)(ahi > 0xffffffffll ? 0xffffffffll : ahi);
    const int64_t lo = b + lower_bound_dev<uint64_t>(keys + b, e - b, klo);
    const int64_t hi = b + upper_bound_dev<uint64_t>(keys + b, e - b, khi);
    if (!FILL) total += (uint32_t)(hi - lo);
    else for (int64_t t = lo; t < hi; t++) { const uint32_t v = order[t]; if (v != o) adj[w++] = v; }
  }
  if (!FILL) cnt[o] = total - 1;                  // its own entry is removed (blot.py:371-372)
}
}  // namespace

struct pw_seed_index {
  int device = 0, self = 0;
  WordSpace ws;
  DeviceArray<uint32_t> tab;            // direct-address table of the join (small key spaces)
  int64_t nS = 0, nT = 0, nkS = 0, nkT = 0, nrows = -1;
  MaskSets ms;
  DeviceArray<uint8_t> dS, dT; DeviceBuffer keys_in, keys_s, keys_t, tmp;      // (the keys: uint32_t or uint64_t by ws.key32; rocPRIM's scratch)
  DeviceArray<uint32_t> pos_in, pos_s, pos_t, lo; DeviceArray<uint64_t> cnt, off; DeviceArray<int2> rows;
  DeviceArray<unsigned long long> scalar;         // [the row total | pw_seeds_count's counter]
  SeedGraph g;                          // neighbourhood graph (K7); g.npts: the rows, or the mirrored non-trivial rows of a self comparison
  DeviceArray<uint32_t> g_dstart; DeviceArray<int2> g_pts;
  DeviceEvent ev0, ev1;
  float ms_build = 0.f;
};

// encode + sort both sequences, join them: everything of pw_seeds_build that depends on the key type
template <typename K>
static int build_join(pw_seed_index* x, hipStream_t st, int64_t ns, bool count_only, unsigned long long total) {
  const WordSpace& ws = x->ws;
  if (count_only) {
    if (encode_sort<K>(set_err, ws, x->ms, x->dS.p, x->nS, x->nkS, x->keys_in, x->pos_in, x->tmp, x->keys_s, x->pos_s, 0, st) != 0)
      return -1;
    if (!x->self && encode_sort<K>(set_err, ws, x->ms, x->dT.p, x->nT, x->nkT, x->keys_in, x->pos_in, x->tmp, x->keys_t, x->pos_t, 0, st) != 0)
      return -1;
    if (ns <= 0) return 0;
    const K* other = x->self ? x->keys_s.as<const K>() : x->keys_t.as<const K>();
    const int64_t no = x->self ? ns : x->nkT;
    const uint32_t* tab = nullptr;
    if (table_pays(ws, no)) {
      if (table_fill<K>(set_err, ws, other, no, x->tab, st) != 0) return -1;
      tab = x->tab.p;
    }
    hipLaunchKernelGGL((k_match<K>), rows_grid((uint64_t)ns), kBlock256, 0, st, x->keys_s.as<const K>(), ns, other, no, ws.kinv, x->self, tab,
                       x->lo.p, x->cnt.p);
    return 0;
  }
  hipLaunchKernelGGL((k_expand<K>), dim3((unsigned)((total + kExpRows - 1) / kExpRows)), kBlock256, 0, st, x->off.p, ns, (int64_t)total,
                     x->pos_s.p, x->self ? x->pos_s.p : x->pos_t.p, x->lo.p, x->keys_s.as<const K>(), x->self, x->rows.p);
  return 0;
}

// the device copies of S and T (64 bytes of slack behind each), and the events that time pw_seeds_build
static int to_device(pw_seed_index* x, const uint8_t* S, const uint8_t* T) {
  CHECK(x->dS.ensure((size_t)x->nS + 64));
  if (upload(set_err, x->dS, S, (size_t)x->nS) != 0) return -1;
  if (!x->self) {
    CHECK(x->dT.ensure((size_t)x->nT + 64));
    if (upload(set_err, x->dT, T, (size_t)x->nT) != 0) return -1;
  }
  CHECK(x->ev0.create()); CHECK(x->ev1.create());
  return 0;
}

extern "C" {

const char* pw_seeds_last_error(void) { return g_err.c_str(); }

pw_seed_index* pw_seeds_create(int device, const uint8_t* S, int64_t nS, const uint8_t* T, int64_t nT,
                               int alphabet_len, int wordlen, const uint64_t* mask_sets, int n_masks,
                               int self_comp) {
  if (check_word(set_err, alphabet_len, wordlen) != 0) return nullptr;
  if (n_masks < 0 || n_masks > kMaxMasks) { set_err("at most 16 mask sets"); return nullptr; }
  if (nS < 0 || nT < 0 || nS >= (1ll << 31) || nT >= (1ll << 31)) { set_err("sequence length out of range"); return nullptr; }
  WordSpace ws;
  if (word_space(set_err, alphabet_len, wordlen, n_masks > 0, &ws) != 0) return nullptr;
  for (int64_t i = 0; i < nS; i++) if (S[i] >= alphabet_len) { set_err("letter outside the alphabet in S"); return nullptr; }
  if (self_comp < 0) self_comp = (nS == nT && (nS == 0 || memcmp(S, T, (size_t)nS) == 0)) ? 1 : 0;
  if (!self_comp) for (int64_t i = 0; i < nT; i++) if (T[i] >= alphabet_len) { set_err("letter outside the alphabet in T"); return nullptr; }
  if (hipSetDevice(device) != hipSuccess) { set_err("hipSetDevice failed"); return nullptr; }
  pw_seed_index* x = new pw_seed_index();
  x->device = device; x->ws = ws; x->self = self_comp;
  x->nS = nS; x->nT = self_comp ? nS : nT;
  x->nkS = nS >= wordlen ? nS - wordlen + 1 : 0;
  x->nkT = self_comp ? x->nkS : (nT >= wordlen ? nT - wordlen + 1 : 0);
  x->ms.n = n_masks;
  for (int i = 0; i < kMaxMasks; i++) x->ms.set[i] = i < n_masks ? mask_sets[i] : 0;
  if (to_device(x, S, T) != 0) { delete x; return nullptr; }
  return x;
}

int pw_seeds_build(pw_seed_index* x, int64_t max_rows, void* stream) {
  if (!x) { set_err("null index"); return -1; }
  hipStream_t st = (hipStream_t)stream;
  CHECK(hipSetDevice(x->device));
  if (max_rows <= 0) max_rows = (1ll << 31) - 1;
  x->nrows = -1; x->g.edges = -1; x->g.npts = -1;
  CHECK(hipEventRecord(x->ev0.e, st));
  const int64_t ns = x->nkS;
  CHECK(x->scalar.ensure(2));
  if (ns > 0) { CHECK(x->lo.ensure((size_t)ns)); CHECK(x->cnt.ensure((size_t)ns)); CHECK(x->off.ensure((size_t)ns)); }
  if ((x->ws.key32 ? build_join<uint32_t>(x, st, ns, true, 0) : build_join<uint64_t>(x, st, ns, true, 0)) != 0) return -1;
  unsigned long long total = 0;
  if (ns > 0) {
    CHECK(rocprim_run(x->tmp, [&](void* t, size_t& b) {
      return rocprim::exclusive_scan(t, b, x->cnt.cp(), x->off.p, (uint64_t)0, (size_t)ns, rocprim::plus<uint64_t>(), st);
    }));
    hipLaunchKernelGGL(k_total, dim3(1), dim3(64), 0, st, x->off.p, x->cnt.p, ns, x->scalar.p);
    CHECK(hipMemcpyAsync(&total, x->scalar.p, sizeof total, hipMemcpyDeviceToHost, st));
    CHECK(hipStreamSynchronize(st));
  }
  if (check_row_limit(set_err, total, max_rows) != 0) return -1;    // (a sum of at most nS * nT: never saturated)
  CHECK(x->rows.ensure((size_t)std::max<unsigned long long>(total, 1)));
  if (total > 0 && (x->ws.key32 ? build_join<uint32_t>(x, st, ns, false, total) : build_join<uint64_t>(x, st, ns, false, total)) != 0) return -1;
  if (elapsed(set_err, x->ev0, x->ev1, st, &x->ms_build) != 0) return -1;
  x->nrows = (int64_t)total;
  return 0;
}

int64_t pw_seeds_num_rows(const pw_seed_index* x) { return x ? x->nrows : -1; }
int pw_seeds_is_self(const pw_seed_index* x) { return x ? x->self : -1; }
const int32_t* pw_seeds_rows_device(const pw_seed_index* x) { return (x && x->nrows >= 0) ? x->rows.as<const int32_t>() : nullptr; }
double pw_seeds_build_ms(const pw_seed_index* x) { return x ? (double)x->ms_build : -1.0; }
int64_t pw_seeds_algorithmic_bytes(const pw_seed_index* x) {
  if (!x || x->nrows < 0) return -1;
  return x->nS + (x->self ? 0 : x->nT) + 8 * x->nrows;
}

int pw_seeds_rows(const pw_seed_index* x, int32_t* da, int64_t cap) {
  if (!x || x->nrows < 0) { set_err("pw_seeds_rows before a successful pw_seeds_build"); return -1; }
  if (cap < x->nrows) { set_err("pw_seeds_rows: capacity too small"); return -1; }
  CHECK(hipSetDevice(x->device));
  if (x->nrows) CHECK(hipMemcpy(da, x->rows.p, x->rows.bytes((size_t)x->nrows), hipMemcpyDeviceToHost));
  return 0;
}

int64_t pw_seeds_count(const pw_seed_index* x, int have_d, int32_t dmin, int32_t dmax, int have_a, int32_t amin,
                       int32_t amax) {
  if (!x || x->nrows < 0) { set_err("pw_seeds_count before a successful pw_seeds_build"); return -1; }
  if (!have_d && !have_a) return x->nrows;
  if (x->nrows == 0) return 0;
  CHECK(hipSetDevice(x->device));
  unsigned long long* out = x->scalar.p + 1;
  CHECK(hipMemsetAsync(out, 0, sizeof *out, nullptr));
  const int64_t blocks = std::min<int64_t>((x->nrows + 255) / 256, 256 * 16);
  hipLaunchKernelGGL(k_count, dim3((unsigned)blocks), kBlock256, 0, nullptr, x->rows.p, x->nrows, have_d, dmin, dmax, have_a, amin, amax, out);
  unsigned long long c = 0;
  CHECK(hipMemcpy(&c, out, sizeof c, hipMemcpyDeviceToHost));
  return (int64_t)c;
}

int64_t pw_seeds_kmers(const pw_seed_index* x, int which, int64_t* out, int64_t cap) {
  if (!x) { set_err("null index"); return -1; }
  const bool t = which != 0 && !x->self;
  const int64_t n = t ? x->nT : x->nS, nk = t ? x->nkT : x->nkS;
  if (cap < nk) { set_err("pw_seeds_kmers: capacity too small"); return -1; }
  if (nk <= 0) return 0;
  CHECK(hipSetDevice(x->device));
  DeviceArray<uint64_t> keys; DeviceArray<uint32_t> pos;
  CHECK(keys.ensure((size_t)nk)); CHECK(pos.ensure((size_t)nk));
  hipLaunchKernelGGL((k_encode<uint64_t>), rows_grid((uint64_t)nk), kBlock256, 0, nullptr, t ? x->dT.p : x->dS.p, n, x->ws.k, x->ws.L,
                     x->ws.kinv, x->ms, keys.p, pos.p);
  std::vector<uint64_t> h((size_t)nk);
  CHECK(hipMemcpy(h.data(), keys.p, keys.bytes((size_t)nk), hipMemcpyDeviceToHost));
  for (int64_t i = 0; i < nk; i++) out[i] = h[(size_t)i] >= x->ws.kinv ? -1 : (int64_t)h[(size_t)i];
  return nk;
}

int pw_seeds_band_neighbours(const pw_seed_index* xc, const double* radius, int64_t n_radius, int32_t* counts, int64_t cap) {
  pw_seed_index* x = const_cast<pw_seed_index*>(xc);
  if (!x || x->nrows < 0) { set_err("pw_seeds_band_neighbours before a successful pw_seeds_build"); return -1; }
  if (x->self) { set_err("pw_seeds_band_neighbours is not defined for a self comparison"); return -1; }
  if (n_radius != x->nS + x->nT + 1) { set_err("radius table must hold nS + nT + 1 entries (d = -nT .. nS)"); return -1; }
  if (cap < x->nrows) { set_err("pw_seeds_band_neighbours: capacity too small"); return -1; }
  for (int64_t i = 0; i < n_radius; i++) if (!(radius[i] > 0)) { set_err("band radii must be positive"); return -1; }
  const int64_t n = x->nrows;
  if (n == 0) return 0;
  CHECK(hipSetDevice(x->device));
  DeviceArray<double> rad, xu, xs; DeviceArray<int32_t> cn;
  CHECK(rad.ensure((size_t)n_radius)); CHECK(xu.ensure((size_t)n)); CHECK(xs.ensure((size_t)n)); CHECK(cn.ensure((size_t)n));
  if (upload(set_err, rad, radius, (size_t)n_radius) != 0) return -1;
  hipLaunchKernelGGL(k_scale, rows_grid((uint64_t)n), kBlock256, 0, nullptr, x->rows.p, n, rad.p, (int)x->nT, xu.p);
  CHECK(rocprim_run(x->tmp, [&](void* t, size_t& b) {
    return rocprim::radix_sort_keys(t, b, xu.cp(), xs.p, (size_t)n, 0u, 64u, (hipStream_t) nullptr);
  }));
  hipLaunchKernelGGL(k_neigh, rows_grid((uint64_t)n), kBlock256, 0, nullptr, xu.p, xs.p, n, cn.p);
  CHECK(hipMemcpy(counts, cn.p, cn.bytes((size_t)n), hipMemcpyDeviceToHost));
  return 0;
}

int64_t pw_seeds_graph_build(pw_seed_index* x, double d_coeff, double radius) {
  if (!x || x->nrows < 0) { set_err("pw_seeds_graph_build before a successful pw_seeds_build"); return -1; }
  if (!(d_coeff > 0) || !(radius >= 0)) { set_err("d_coeff must be positive and radius non-negative"); return -1; }
  SeedGraph& g = x->g;
  g.edges = -1; g.npts = -1;
  CHECK(hipSetDevice(x->device));
  const int2* pts = x->rows.p;
  int64_t n = x->nrows;
  if (x->self && n > 0) {
    // the point list of a self comparison: non-trivial rows and their mirror images, in table order
    DeviceArray<uint64_t> flag, pos;              // (freed at the end of this block)
    CHECK(flag.ensure((size_t)n)); CHECK(pos.ensure((size_t)n));
    const dim3 g = rows_grid((uint64_t)n), bl = kBlock256;
    hipLaunchKernelGGL(k_self_flag, g, bl, 0, nullptr, x->rows.p, n, flag.p);
    CHECK(rocprim_run(x->tmp, [&](void* t, size_t& b) {
      return rocprim::exclusive_scan(t, b, flag.cp(), pos.p, (uint64_t)0, (size_t)n, rocprim::plus<uint64_t>(), (hipStream_t) nullptr);
    }));
    uint64_t lp = 0, lf = 0;
    CHECK(hipMemcpy(&lp, pos.p + (n - 1), sizeof lp, hipMemcpyDeviceToHost));
    CHECK(hipMemcpy(&lf, flag.p + (n - 1), sizeof lf, hipMemcpyDeviceToHost));
    const int64_t np = (int64_t)(2 * (lp + lf));
    CHECK(x->g_pts.ensure((size_t)std::max<int64_t>(np, 1)));
    hipLaunchKernelGGL(k_self_points, g, bl, 0, nullptr, x->rows.p, n, pos.p, x->g_pts.p);
    CHECK(hipDeviceSynchronize());
    pts = x->g_pts.p; n = np;
  }
  g.npts = n;
  if (n == 0) { g.edges = 0; return 0; }
  const int64_t nd = x->nS + x->nT + 1;
  const double wd = floor(radius / d_coeff) + 2;
  const int win = wd > (double)nd ? (int)nd : (int)wd;
  DeviceArray<uint64_t> kin; DeviceArray<uint32_t> vin;      // kin: the sort keys, then graph_finish's widened counts
  CHECK(kin.ensure((size_t)n)); CHECK(vin.ensure((size_t)n)); CHECK(x->g_dstart.ensure((size_t)nd + 1));
  const dim3 grid = rows_grid((uint64_t)n), blk = kBlock256;
  hipLaunchKernelGGL(k_graph_keys, grid, blk, 0, nullptr, pts, n, (int)x->nT, kin.p, vin.p);
  if (graph_sort(set_err, g, x->tmp, kin, vin, n, 32 + bits_for((uint64_t)nd)) != 0) return -1;
  hipLaunchKernelGGL(k_graph_dstart, rows_grid((uint64_t)nd + 1), blk, 0, nullptr, g.keys.p, n, nd, x->g_dstart.p);
  hipLaunchKernelGGL((k_graph_scan<false>), grid, blk, 0, nullptr, g.keys.p, g.order.p, n, x->g_dstart.p, (int)nd, (int)x->nT, d_coeff, radius,
                     win, g.cnt.p, (const uint64_t*)nullptr, (uint32_t*)nullptr);
  const int64_t total = graph_finish(set_err, g, x->tmp, x->scalar, kin.p, n, [&] {
    hipLaunchKernelGGL((k_graph_scan<true>), grid, blk, 0, nullptr, g.keys.p, g.order.p, n, x->g_dstart.p, (int)nd, (int)x->nT, d_coeff, radius,
                       win, (uint32_t*)nullptr, g.off.p, g.adj.p);
    return 0;
  });
  if (total < 0) return -1;
  CHECK(hipDeviceSynchronize());                  // (no event timing: the pairwise ABI has no graph_ms)
  CHECK(hipGetLastError());
  g.edges = total;
  return total;
}

int64_t pw_seeds_graph_num_points(const pw_seed_index* x) { return (x && x->g.edges >= 0) ? x->g.npts : -1; }

int pw_seeds_graph_points(const pw_seed_index* x, int32_t* da, int64_t cap) {
  if (!x || x->g.edges < 0) { set_err("pw_seeds_graph_points before a successful pw_seeds_graph_build"); return -1; }
  if (cap < x->g.npts) { set_err("pw_seeds_graph_points: capacity too small"); return -1; }
  CHECK(hipSetDevice(x->device));
  if (x->g.npts) CHECK(hipMemcpy(da, x->self ? x->g_pts.p : x->rows.p, x->rows.bytes((size_t)x->g.npts), hipMemcpyDeviceToHost));
  return 0;
}

int pw_seeds_graph_counts(const pw_seed_index* x, int32_t* counts, int64_t cap) {
  return graph_counts_to_host(set_err, "pw_seeds_graph_counts", x, counts, cap);
}

int pw_seeds_graph_fetch(const pw_seed_index* x, int64_t* offsets, int32_t* neighbours) {
  return graph_fetch_to_host(set_err, "pw_seeds_graph_fetch", x, offsets, neighbours);
}

int pw_seeds_graph_components(const pw_seed_index* x, const uint8_t* avail, int32_t* labels) {
  return graph_components(set_err, "pw_seeds_graph_components", x, avail, labels, nullptr, nullptr);      // (neither timed nor counted)
}

void pw_seeds_destroy(pw_seed_index* x) {
  if (!x) return;
  (void)hipSetDevice(x->device);
  delete x;
}

}  // extern "C"

// pw_mseeds.hip -- exact-match k-mer seeds shared by N = 2 .. 16 sequences on gfx950 (C ABI: include/pw_mseeds.h).
//
// The reference enumerates the seeds of WordBlotMultipleFast in Python (blot.py:1040-1071: per k-mer the product of its
// hit lists) and finds neighbours with a cKDTree (blot.py:833-868).  Here the same is a sort-merge join, generalised:
//   K9a k_encode      one thread per position of every sequence (pw_seed_kernels.h; no mask), then one stable radix sort
//                     of (k-mer, position) per sequence, so positions stay ascending inside a k-mer
//   K9b k_mjoin       one thread per sorted element of sequence 0; the first of each k-mer run finds that k-mer's run in
//                     every other sequence (two binary searches each) -> rows = product of the N run lengths, saturating
//                     at 2^64 - 1; a saturating exclusive scan -> row offsets
//   K9c k_mexpand     one thread per row: the row's k-mer by a windowed binary search over the offsets, then the row
//                     index inside the k-mer decoded in mixed radix (sequence N-1 fastest) -> (d_1 .. d_{N-1}, a).
//                     Rows come out in itertools.product order by construction, with no further sort
//   K9d k_mcount      hyper-box counts for up to 64 boxes per workgroup row: a row is read once per 64 boxes, the
//                     predicate goes through a ballot into LDS counters, one 64-bit atomic per box and workgroup
//   K9e k_mgraph_*    the neighbourhood graph: points sorted by (d_1, a) as K7 does, gathered into a sorted copy, one
//                     thread per point scans the admissible d_1 runs, binary-searches the a window in each and tests
//                     d_2 .. d_{N-1} per candidate; a count pass, a scan, a fill pass (CSR)
//       k_cc_*        connected components of the available rows (pw_seed_kernels.h)
// All of it is memory- and latency-bound: binary searches and row traffic, no arithmetic to speak of.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <algorithm>
#include <string>
#include <rocprim/rocprim.hpp>

#include "../../include/pw_mseeds.h"
#include "pw_seed_host.h"

namespace {

thread_local std::string g_err;
void set_err(const std::string& s) { g_err = s; }
#define CHECK(call) PW_HIP_CHECK(set_err, call)

constexpr int kMaxSeqs = 16;
// Where every sequence's sorted k-mers start in the concatenated key / position arrays, and how many there are.
struct SeqOffsets { int64_t koff[kMaxSeqs + 1]; };

__device__ __forceinline__ uint64_t sat_mul(uint64_t a, uint64_t b) { return __umul64hi(a, b) ? ~0ull : a * b; }
// (SatAdd: pw_seed_host.h)

// ---- K9b ------------------------------------------------------------------------------------------------
// lo[s * nk0 + e] / rl[s * nk0 + e]: start and length of the run of e's k-mer in sequence s (filled for run starts only).
template <typename K>
__global__ __launch_bounds__(256) void k_mjoin(const K* __restrict__ keys, SeqOffsets so, int n, uint32_t* __restrict__ lo,
                                               uint32_t* __restrict__ rl, uint64_t* __restrict__ cnt) {
  const int64_t nk0 = so.koff[1];
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= nk0) return;
  const K key = keys[e];
  if (e > 0 && keys[e - 1] == key) { cnt[e] = 0; return; }
  const int64_t run0 = upper_bound_dev<K>(keys + e, nk0 - e, key);
  lo[e] = (uint32_t)e; rl[e] = (uint32_t)run0;
  uint64_t prod = (uint64_t)run0;
  for (int s = 1; s < n && prod; s++) {
    const K* ks = keys + so.koff[s];
    const int64_t ns = so.koff[s + 1] - so.koff[s];
    const int64_t l = lower_bound_dev<K>(ks, ns, key), h = l + upper_bound_dev<K>(ks + l, ns - l, key);
    lo[s * nk0 + e] = (uint32_t)l; rl[s * nk0 + e] = (uint32_t)(h - l);
    prod = sat_mul(prod, (uint64_t)(h - l));
  }
  cnt[e] = prod;
}
__global__ void k_total_sat(const uint64_t* __restrict__ off, const uint64_t* __restrict__ cnt, int64_t ns,
                            unsigned long long* __restrict__ out) {
  if (threadIdx.x == 0 && blockIdx.x == 0) out[0] = ns > 0 ? SatAdd()(off[ns - 1], cnt[ns - 1]) : 0ull;
}

// ---- K9c ------------------------------------------------------------------------------------------------
// As K5c: kExpRows rows per workgroup, the workgroup's window of elements found by two searches over all offsets, then
// ~10 cache-resident steps per row.  The row count is below 2^31 (pw_mseeds_build refuses more), so the mixed-radix
// decode runs in 32 bits.
constexpr int kExpRows = 2048;
template <int N>
__global__ __launch_bounds__(256) void k_mexpand(const uint64_t* __restrict__ off, int64_t nk0, int64_t nrows,
                                                 const uint32_t* __restrict__ pos, SeqOffsets so,
                                                 const uint32_t* __restrict__ lo, const uint32_t* __restrict__ rl,
                                                 int32_t* __restrict__ rows) {
  __shared__ int64_t win[2];
  const int64_t o0 = (int64_t)blockIdx.x * kExpRows;
  const int64_t olast = (o0 + kExpRows < nrows ? o0 + kExpRows : nrows) - 1;
  if (threadIdx.x == 0) win[0] = upper_bound_dev<uint64_t>(off, nk0, (uint64_t)o0) - 1;
  if (threadIdx.x == 64) win[1] = upper_bound_dev<uint64_t>(off, nk0, (uint64_t)olast) - 1;
  __syncthreads();
  const int64_t e0 = win[0], nwin = win[1] - win[0] + 1;
#pragma unroll 1
  for (int q = 0; q < kExpRows / 256; q++) {
    const int64_t o = o0 + q * 256 + threadIdx.x;
    if (o >= nrows) return;
    const int64_t e = e0 + upper_bound_dev<uint64_t>(off + e0, nwin, (uint64_t)o) - 1;
    uint32_t r = (uint32_t)(o - (int64_t)off[e]);
    int32_t p[N];
#pragma unroll
    for (int s = N - 1; s >= 1; s--) {
      const uint32_t len = rl[s * nk0 + e];
      const uint32_t qt = r / len, idx = r - qt * len;
      r = qt;
      p[s] = (int32_t)pos[so.koff[s] + lo[s * nk0 + e] + idx];
    }
    p[0] = (int32_t)pos[e + r];
    int32_t a = 0;
#pragma unroll
    for (int s = 0; s < N; s++) a += p[s];
    int32_t* out = rows + o * N;
#pragma unroll
    for (int s = 1; s < N; s++) out[s - 1] = p[0] - p[s];
    out[N - 1] = a;
  }
}

// ---- K9d ------------------------------------------------------------------------------------------------
// grid.y walks the boxes 64 at a time; box b's bounds are lo / hi / have[b N .. b N + N).
constexpr int kBoxChunk = 64;
template <int N>
__global__ __launch_bounds__(256) void k_mcount(const int32_t* __restrict__ rows, int64_t nrows, int64_t nboxes,
                                                const int32_t* __restrict__ lo, const int32_t* __restrict__ hi,
                                                const uint8_t* __restrict__ have, unsigned long long* __restrict__ counts) {
  __shared__ uint32_t c[kBoxChunk];
  const int64_t b0 = (int64_t)blockIdx.y * kBoxChunk;
  const int nb = (int)(nboxes - b0 < kBoxChunk ? nboxes - b0 : kBoxChunk);
  if (threadIdx.x < kBoxChunk) c[threadIdx.x] = 0;
  __syncthreads();
  for (int64_t base = (int64_t)blockIdx.x * 256; base < nrows; base += (int64_t)gridDim.x * 256) {
    const int64_t o = base + threadIdx.x;
    const bool valid = o < nrows;
    int32_t v[N];
#pragma unroll
    for (int k = 0; k < N; k++) v[k] = valid ? rows[o * N + k] : 0;
    for (int b = 0; b < nb; b++) {
      const int64_t bb = (b0 + b) * N;
      bool ok = valid;
#pragma unroll
      for (int k = 0; k < N; k++) ok = ok && (!have[bb + k] || (v[k] >= lo[bb + k] && v[k] <= hi[bb + k]));
      const uint64_t m = __ballot(ok);
      if ((threadIdx.x & 63u) == 0 && m) atomicAdd(&c[b], (uint32_t)__popcll(m));
    }
  }
  __syncthreads();
  if ((int)threadIdx.x < nb && c[threadIdx.x]) atomicAdd(&counts[b0 + threadIdx.x], (unsigned long long)c[threadIdx.x]);
}

// ---- K9e ------------------------------------------------------------------------------------------------
// Keys as K7's: (d_1 + nd_off) in the high word, a in the low word; d_1 + nd_off >= 0 and a >= 0 for every row.
__global__ __launch_bounds__(256) void k_mgraph_keys(const int32_t* __restrict__ rows, int64_t n, int N, int nd_off,
                                                     uint64_t* __restrict__ keys, uint32_t* __restrict__ vals) {
  const int64_t o = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (o >= n) return;
  keys[o] = ((uint64_t)(uint32_t)(rows[o * N] + nd_off) << 32) | (uint32_t)rows[o * N + N - 1];
  vals[o] = (uint32_t)o;
}
// the rows in (d_1, a) order, so that the candidates of one d_1 run are contiguous
__global__ __launch_bounds__(256) void k_mgraph_gather(const int32_t* __restrict__ rows, const uint32_t* __restrict__ order, int64_t n,
                                                       int N, int32_t* __restrict__ srows) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= n) return;
  const int64_t o = order[t];
  for (int k = 0; k < N; k++) srows[t * N + k] = rows[o * N + k];
}
// One thread per point in (d_1, a) order.  For every d_1 bucket that passes the KD-tree's test on the scaled axis,
// fl(|fl(d c) - fl(d' c)|) <= R, the points with |a - a'| <= R are one contiguous piece of the bucket; each candidate
// there is then held to the same test on d_2 .. d_{N-1}.
template <int N, bool FILL>
__global__ __launch_bounds__(256) void k_mgraph_scan(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ order,
                                                     const int32_t* __restrict__ srows, int64_t n,
                                                     const uint32_t* __restrict__ dstart, int nd, int nd_off, double c, double R,
                                                     int win, uint32_t* __restrict__ cnt, const uint64_t* __restrict__ off,
                                                     uint32_t* __restrict__ adj) {
  const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (s >= n) return;
  const uint64_t key = keys[s];
  const uint32_t o = order[s];
  const int q = (int)(key >> 32);
  const int64_t a = (int64_t)(uint32_t)key;
  const double X = (double)(q - nd_off) * c;
  double Xk[N > 2 ? N - 2 : 1];
#pragma unroll
  for (int k = 1; k < N - 1; k++) Xk[k - 1] = (double)srows[s * N + k] * c;
  const int64_t ra = (int64_t)floor(R);           // |a - a'| <= R for integers
  uint64_t w = FILL ? off[o] : 0;
  uint32_t total = 0;
  const int q0 = q - win < 0 ? 0 : q - win, q1 = q + win > nd - 1 ? nd - 1 : q + win;
  for (int qq = q0; qq <= q1; qq++) {
    const double Xp = (double)(qq - nd_off) * c;
    if (!(fabs(X - Xp) <= R)) continue;
    const int64_t b = dstart[qq], e = dstart[qq + 1];
    if (b == e) continue;
    const int64_t alo = a - ra < 0 ? 0 : a - ra, ahi = a + ra;
    const uint64_t klo = ((uint64_t)(uint32_t)qq << 32) | (uint64_t)alo;
    const uint64_t khi = ((uint64_t)(uint32_t)qq << 32) | (uint64_t)(ahi > 0xffffffffll ? 0xffffffffll : ahi);
    const int64_t lo = b + lower_bound_dev<uint64_t>(keys + b, e - b, klo);
    const int64_t hi = b + upper_bound_dev<uint64_t>(keys + b, e - b, khi);
    for (int64_t t = lo; t < hi; t++) {
      bool ok = true;
#pragma unroll
      for (int k = 1; k < N - 1; k++) ok = ok && fabs(Xk[k - 1] - (double)srows[t * N + k] * c) <= R;
      if (!ok) continue;
      if (!FILL) total++;
      else { const uint32_t v = order[t]; if (v != o) adj[w++] = v; }
    }
  }
  if (!FILL) cnt[o] = total - 1;                  // its own entry is removed (blot.py:864-866)
}

// One launch of a kernel templated on the number of sequences N = 2 .. 16.
#define PW_MSEEDS_FOR_N(n, LAUNCH)                                                                        \
  switch (n) {                                                                                            \
    case 2: LAUNCH(2); break;   case 3: LAUNCH(3); break;   case 4: LAUNCH(4); break;                     \
    case 5: LAUNCH(5); break;   case 6: LAUNCH(6); break;   case 7: LAUNCH(7); break;                     \
    case 8: LAUNCH(8); break;   case 9: LAUNCH(9); break;   case 10: LAUNCH(10); break;                   \
    case 11: LAUNCH(11); break; case 12: LAUNCH(12); break; case 13: LAUNCH(13); break;                   \
    case 14: LAUNCH(14); break; case 15: LAUNCH(15); break; case 16: LAUNCH(16); break;                   \
    default: set_err("n_seqs out of range"); return -1;                                                   \
  }

}  // namespace

struct pw_mseed_index {
  int device = 0, n = 0;
  WordSpace ws;
  int64_t len[kMaxSeqs] = {}, soff[kMaxSeqs + 1] = {}, nrows = -1;
  SeqOffsets so = {};
  DeviceArray<uint8_t> dseq; DeviceBuffer keys_in, keys, tmp;      // (the keys: uint32_t or uint64_t by ws.key32; rocPRIM's scratch)
  DeviceArray<uint32_t> pos_in, pos, lo, rl; DeviceArray<uint64_t> cnt, off;
  DeviceArray<int32_t> rows; DeviceArray<unsigned long long> scalar;   // rows: n indices each
  SeedGraph g;                          // neighbourhood graph (K9e); g.npts: the rows
  DeviceArray<int32_t> g_srows; DeviceArray<uint32_t> g_dstart;
  DeviceEvent ev0, ev1;
  float ms_build = 0.f, ms_graph = 0.f, ms_cc = 0.f, ms_count = 0.f;
};

// encode + sort every sequence, join on sequence 0: everything of pw_mseeds_build that depends on the key type
template <typename K>
static int build_join(pw_mseed_index* x, hipStream_t st) {
  const int64_t nk_all = x->so.koff[x->n], nk0 = x->so.koff[1];
  int64_t nk_max = 1;
  for (int s = 0; s < x->n; s++) nk_max = std::max(nk_max, x->so.koff[s + 1] - x->so.koff[s]);
  // every sequence sorts into its own piece of keys / pos through one pair of staging buffers: all sized here
  CHECK(x->keys.ensure((size_t)std::max<int64_t>(nk_all, 1) * sizeof(K))); CHECK(x->pos.ensure((size_t)std::max<int64_t>(nk_all, 1)));
  CHECK(x->keys_in.ensure((size_t)nk_max * sizeof(K))); CHECK(x->pos_in.ensure((size_t)nk_max));
  const MaskSets none = {};
  for (int s = 0; s < x->n; s++)
    if (encode_sort<K>(set_err, x->ws, none, x->dseq.p + x->soff[s], x->len[s], x->so.koff[s + 1] - x->so.koff[s], x->keys_in, x->pos_in,
                       x->tmp, x->keys, x->pos, x->so.koff[s], st) != 0)
      return -1;
  hipLaunchKernelGGL((k_mjoin<K>), rows_grid((uint64_t)nk0), kBlock256, 0, st, x->keys.as<const K>(), x->so, x->n, x->lo.p, x->rl.p, x->cnt.p);
  return 0;
}

extern "C" {

const char* pw_mseeds_last_error(void) { return g_err.c_str(); }

pw_mseed_index* pw_mseeds_create(int device, const uint8_t* const* seqs, const int64_t* lens, int n_seqs,
                                 int alphabet_len, int wordlen) {
  if (n_seqs < 2 || n_seqs > kMaxSeqs) { set_err("n_seqs must be 2..16"); return nullptr; }
  WordSpace ws;
  if (check_word(set_err, alphabet_len, wordlen) != 0 || word_space(set_err, alphabet_len, wordlen, false, &ws) != 0) return nullptr;
  int64_t total = 0;
  for (int s = 0; s < n_seqs; s++) {             // all lengths first: nothing is read before they are known to be sane
    if (lens[s] < 0) { set_err("negative sequence length"); return nullptr; }
    total += lens[s];
    if (total >= (1ll << 31)) { set_err("the sequences' lengths must sum to less than 2^31"); return nullptr; }
    if (lens[s] > 0 && !seqs[s]) { set_err("null sequence pointer"); return nullptr; }
  }
  for (int s = 0; s < n_seqs; s++) {
    for (int64_t i = 0; i < lens[s]; i++)
      if (seqs[s][i] >= alphabet_len) { set_err("letter outside the alphabet in sequence " + std::to_string(s)); return nullptr; }
  }
  if (hipSetDevice(device) != hipSuccess) { set_err("hipSetDevice failed"); return nullptr; }
  pw_mseed_index* x = new pw_mseed_index();
  x->device = device; x->ws = ws; x->n = n_seqs;
  for (int s = 0; s < n_seqs; s++) {
    x->len[s] = lens[s];
    x->soff[s + 1] = x->soff[s] + lens[s];
    x->so.koff[s + 1] = x->so.koff[s] + (lens[s] >= wordlen ? lens[s] - wordlen + 1 : 0);
  }
  for (int s = n_seqs; s < kMaxSeqs; s++) x->so.koff[s + 1] = x->so.koff[n_seqs];
  if (x->dseq.ensure((size_t)total + 64) != hipSuccess || x->ev0.create() != hipSuccess || x->ev1.create() != hipSuccess) {
    set_err("device allocation failed"); delete x; return nullptr;
  }
  for (int s = 0; s < n_seqs; s++)
    if (lens[s] && hipMemcpy(x->dseq.p + x->soff[s], seqs[s], (size_t)lens[s], hipMemcpyHostToDevice) != hipSuccess) {
      set_err("copy of the sequences to the device failed"); delete x; return nullptr;
    }
  return x;
}

int pw_mseeds_build(pw_mseed_index* x, int64_t max_rows, void* stream) {
  if (!x) { set_err("null index"); return -1; }
  hipStream_t st = (hipStream_t)stream;
  CHECK(hipSetDevice(x->device));
  // default: the rows (4 N bytes each) within 16 GB; never above 2^31 - 1 rows (int32 row indices in the graph)
  if (max_rows <= 0) max_rows = (16ll << 30) / (4ll * x->n);
  max_rows = std::min<int64_t>(max_rows, (1ll << 31) - 1);
  x->nrows = -1; x->g.edges = -1; x->g.npts = -1;
  CHECK(hipEventRecord(x->ev0.e, st));
  CHECK(x->scalar.ensure(2));
  const int64_t nk0 = x->so.koff[1];
  bool empty = false;
  for (int s = 0; s < x->n; s++) empty |= x->so.koff[s + 1] == x->so.koff[s];
  unsigned long long total = 0;
  if (!empty) {
    CHECK(x->lo.ensure((size_t)nk0 * x->n)); CHECK(x->rl.ensure((size_t)nk0 * x->n));
    CHECK(x->cnt.ensure((size_t)nk0)); CHECK(x->off.ensure((size_t)nk0));
    if ((x->ws.key32 ? build_join<uint32_t>(x, st) : build_join<uint64_t>(x, st)) != 0) return -1;
    CHECK(rocprim_run(x->tmp, [&](void* t, size_t& b) {
      return rocprim::exclusive_scan(t, b, x->cnt.cp(), x->off.p, (uint64_t)0, (size_t)nk0, SatAdd(), st);
    }));
    hipLaunchKernelGGL(k_total_sat, dim3(1), dim3(64), 0, st, x->off.p, x->cnt.p, nk0, x->scalar.p);
    CHECK(hipMemcpyAsync(&total, x->scalar.p, sizeof total, hipMemcpyDeviceToHost, st));
    CHECK(hipStreamSynchronize(st));
  }
  if (check_row_limit(set_err, total, max_rows) != 0) return -1;
  CHECK(x->rows.ensure((size_t)std::max<unsigned long long>(total, 1) * x->n));
  if (total > 0) {
    const dim3 g((unsigned)((total + kExpRows - 1) / kExpRows)), b = kBlock256;
#define PW_LAUNCH_EXPAND(N_) \
  hipLaunchKernelGGL((k_mexpand<N_>), g, b, 0, st, x->off.p, nk0, (int64_t)total, x->pos.p, x->so, x->lo.p, x->rl.p, x->rows.p)
    PW_MSEEDS_FOR_N(x->n, PW_LAUNCH_EXPAND)
#undef PW_LAUNCH_EXPAND
  }
  if (elapsed(set_err, x->ev0, x->ev1, st, &x->ms_build) != 0) return -1;
  x->nrows = (int64_t)total;
  return 0;
}

int pw_mseeds_num_seqs(const pw_mseed_index* x) { return x ? x->n : -1; }
int64_t pw_mseeds_num_rows(const pw_mseed_index* x) { return x ? x->nrows : -1; }
const int32_t* pw_mseeds_rows_device(const pw_mseed_index* x) { return (x && x->nrows >= 0) ? x->rows.p : nullptr; }
double pw_mseeds_build_ms(const pw_mseed_index* x) { return x ? (double)x->ms_build : -1.0; }
double pw_mseeds_graph_ms(const pw_mseed_index* x) { return x ? (double)x->ms_graph : -1.0; }
double pw_mseeds_components_ms(const pw_mseed_index* x) { return x ? (double)x->ms_cc : -1.0; }
double pw_mseeds_count_ms(const pw_mseed_index* x) { return x ? (double)x->ms_count : -1.0; }
int64_t pw_mseeds_algorithmic_bytes(const pw_mseed_index* x) {
  if (!x || x->nrows < 0) return -1;
  return x->soff[x->n] + 4ll * x->n * x->nrows;
}

int pw_mseeds_rows(const pw_mseed_index* x, int32_t* rows, int64_t cap) {
  if (!x || x->nrows < 0) { set_err("pw_mseeds_rows before a successful pw_mseeds_build"); return -1; }
  if (cap < x->nrows) { set_err("pw_mseeds_rows: capacity too small"); return -1; }
  CHECK(hipSetDevice(x->device));
  if (x->nrows) CHECK(hipMemcpy(rows, x->rows.p, x->rows.bytes((size_t)x->nrows * x->n), hipMemcpyDeviceToHost));
  return 0;
}

int pw_mseeds_count_many(const pw_mseed_index* xc, int64_t n_boxes, const int32_t* lo, const int32_t* hi, const uint8_t* have,
                         int64_t* counts) {
  pw_mseed_index* x = const_cast<pw_mseed_index*>(xc);
  if (!x || x->nrows < 0) { set_err("pw_mseeds_count_many before a successful pw_mseeds_build"); return -1; }
  if (n_boxes < 0) { set_err("n_boxes must be non-negative"); return -1; }
  if (n_boxes == 0) return 0;
  if (n_boxes > (int64_t)kBoxChunk * 65535) { set_err("at most 64 * 65535 boxes per call"); return -1; }
  CHECK(hipSetDevice(x->device));
  const size_t nb = (size_t)n_boxes * x->n;
  DeviceArray<int32_t> dlo, dhi; DeviceArray<uint8_t> dhave; DeviceArray<unsigned long long> dcnt;
  CHECK(dlo.ensure(nb)); CHECK(dhi.ensure(nb)); CHECK(dhave.ensure(nb)); CHECK(dcnt.ensure((size_t)n_boxes));
  if (upload(set_err, dlo, lo, nb) != 0 || upload(set_err, dhi, hi, nb) != 0 || upload(set_err, dhave, have, nb) != 0) return -1;
  CHECK(hipMemsetAsync(dcnt.p, 0, dcnt.bytes((size_t)n_boxes), nullptr));
  CHECK(hipEventRecord(x->ev0.e, nullptr));
  if (x->nrows > 0) {
    const dim3 g((unsigned)std::min<int64_t>((x->nrows + 255) / 256, 1024), (unsigned)((n_boxes + kBoxChunk - 1) / kBoxChunk)), b = kBlock256;
#define PW_LAUNCH_COUNT(N_) hipLaunchKernelGGL((k_mcount<N_>), g, b, 0, nullptr, x->rows.p, x->nrows, n_boxes, dlo.p, dhi.p, dhave.p, dcnt.p)
    PW_MSEEDS_FOR_N(x->n, PW_LAUNCH_COUNT)
#undef PW_LAUNCH_COUNT
  }
  if (elapsed(set_err, x->ev0, x->ev1, nullptr, &x->ms_count) != 0) return -1;
  CHECK(hipMemcpy(counts, dcnt.p, dcnt.bytes((size_t)n_boxes), hipMemcpyDeviceToHost));
  return 0;
}

int64_t pw_mseeds_graph_build(pw_mseed_index* x, double d_coeff, double radius) {
  if (!x || x->nrows < 0) { set_err("pw_mseeds_graph_build before a successful pw_mseeds_build"); return -1; }
  if (!(d_coeff > 0) || !(radius >= 0)) { set_err("d_coeff must be positive and radius non-negative"); return -1; }
  SeedGraph& g = x->g;
  g.edges = -1;
  CHECK(hipSetDevice(x->device));
  const int64_t n = g.npts = x->nrows;
  if (n == 0) { g.edges = 0; x->ms_graph = 0.f; return 0; }
  CHECK(hipEventRecord(x->ev0.e, nullptr));
  const int N = x->n;
  // d_1 = i_1 - i_2 lies in (-len_2, len_1): bucket q = d_1 + len_2 in [0, nd)
  const int nd_off = (int)x->len[1];
  const int64_t nd = x->len[0] + x->len[1] + 1;
  const double wd = floor(radius / d_coeff) + 2;
  const int win = wd > (double)nd ? (int)nd : (int)wd;
  DeviceArray<uint64_t> kin; DeviceArray<uint32_t> vin;      // kin: the sort keys, then graph_finish's widened counts
  CHECK(kin.ensure((size_t)n)); CHECK(vin.ensure((size_t)n));
  CHECK(x->g_srows.ensure((size_t)n * N)); CHECK(x->g_dstart.ensure((size_t)nd + 1));
  const dim3 grid = rows_grid((uint64_t)n), blk = kBlock256;
  hipLaunchKernelGGL(k_mgraph_keys, grid, blk, 0, nullptr, x->rows.p, n, N, nd_off, kin.p, vin.p);
  if (graph_sort(set_err, g, x->tmp, kin, vin, n, 32 + bits_for((uint64_t)nd)) != 0) return -1;
  hipLaunchKernelGGL(k_mgraph_gather, grid, blk, 0, nullptr, x->rows.p, g.order.p, n, N, x->g_srows.p);
  hipLaunchKernelGGL(k_graph_dstart, rows_grid((uint64_t)nd + 1), blk, 0, nullptr, g.keys.p, n, nd, x->g_dstart.p);
  // the count pass (FILL_ = false: cnt) and the fill pass (off -> adj)
  uint32_t* const no_counts = nullptr; uint32_t* const no_adj = nullptr; const uint64_t* const no_off = nullptr;
#define PW_LAUNCH_SCAN(N_, FILL_, CNT_, OFF_, ADJ_)                                                                              \
  hipLaunchKernelGGL((k_mgraph_scan<N_, FILL_>), grid, blk, 0, nullptr, g.keys.p, g.order.p, x->g_srows.p, n, x->g_dstart.p, (int)nd, \
                     nd_off, d_coeff, radius, win, CNT_, OFF_, ADJ_)
#define PW_LAUNCH_COUNT_PASS(N_) PW_LAUNCH_SCAN(N_, false, g.cnt.p, no_off, no_adj)
#define PW_LAUNCH_FILL_PASS(N_) PW_LAUNCH_SCAN(N_, true, no_counts, g.off.p, g.adj.p)
  PW_MSEEDS_FOR_N(N, PW_LAUNCH_COUNT_PASS)
  const int64_t total = graph_finish(set_err, g, x->tmp, x->scalar, kin.p, n, [&]() -> int {
    PW_MSEEDS_FOR_N(N, PW_LAUNCH_FILL_PASS)
    return 0;
  });
#undef PW_LAUNCH_FILL_PASS
#undef PW_LAUNCH_COUNT_PASS
#undef PW_LAUNCH_SCAN
  if (total < 0) return -1;
  if (elapsed(set_err, x->ev0, x->ev1, nullptr, &x->ms_graph) != 0) return -1;
  g.edges = total;
  return total;
}

int pw_mseeds_graph_counts(const pw_mseed_index* x, int32_t* counts, int64_t cap) {
  return graph_counts_to_host(set_err, "pw_mseeds_graph_counts", x, counts, cap);
}

int pw_mseeds_graph_fetch(const pw_mseed_index* x, int64_t* offsets, int32_t* neighbours) {
  return graph_fetch_to_host(set_err, "pw_mseeds_graph_fetch", x, offsets, neighbours);
}

int pw_mseeds_graph_components(const pw_mseed_index* xc, const uint8_t* avail, int32_t* labels) {
  pw_mseed_index* x = const_cast<pw_mseed_index*>(xc);
  return graph_components(set_err, "pw_mseeds_graph_components", x, avail, labels, x ? &x->ms_cc : nullptr, nullptr);
}

void pw_mseeds_destroy(pw_mseed_index* x) {
  if (!x) return;
  (void)hipSetDevice(x->device);
  delete x;
}

}  // extern "C"

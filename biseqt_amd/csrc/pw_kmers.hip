// pw_kmers.hip -- the k-mer table of a whole read set and the questions asked of it (C ABI: include/pw_kmers.h).
//
//   K9a  k_enc_reads      (pw_kmer_encode.h, shared with pw_overlap.hip) k-mer of every position of every read, hit = (read << 32) | pos
//   K9a' k_enc_reads_rc   ... of the reverse complement of every read, behind the forward rows (PW_STRAND_BOTH)
//   K14a k_kmers_tag      the strand bit of the reverse rows' hits
//        sort             by k-mer (rocPRIM radix sort, stable: the rows were generated in (strand, read, pos) order and keep it
//                         inside a k-mer)
//   K14b k_kmers_heads    one thread per row: 1 where a run of equal keys starts
//        scan             exclusive sum of the heads = the rank of every row's run
//   K14c k_kmers_runs     one thread per row: a run head writes its key and its first row; the last row writes the number of
//                         runs D and the end of the table: run u is [ustart[u], ustart[u + 1])
//   K14d k_kmers_spectrum grid-stride over the runs: histogram of min(count, max_mult) in LDS, flushed once per workgroup
//   K14e k_kmers_lookup   one thread per query: a binary search over the D distinct keys
//   K14f k_kmers_occ      one thread per row: a forward row writes its run's length to (read, pos)
// A SAMPLED table (pw_kmers_build_sampled, window > 1) holds the window minimizers only: K15a-c of pw_minimizer.h stand in for
// the encoders, everything from the sort on is the same, and K15d k_mini_occ stands in for K14f.
// Everything is asynchronous on the stream of the build; the number of runs stays on the device until a call returns host
// data.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <cstring>
#include <algorithm>
#include <string>
#include <vector>
#include <rocprim/rocprim.hpp>

#include "../../include/pw_kmers.h"
#include "pw_complement.h"
#include "pw_hip_host.h"
#include "pw_kmer_encode.h"
#include "pw_minimizer.h"

namespace {

thread_local std::string g_err;
thread_local double g_ms = 0.0;
void set_err(const std::string& s) { g_err = s; }
#define CHECK(call) PW_HIP_CHECK(set_err, call)

constexpr uint64_t kStrandBit = 1ull << 31;

// K14a: hits of the reverse rows carry strand 1
__global__ __launch_bounds__(256) void k_kmers_tag(uint64_t* __restrict__ vals, int64_t n) {
  const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (g < n) vals[g] |= kStrandBit;
}

// K14b: head[g] = 1 where row g starts a run of equal keys
__global__ __launch_bounds__(256) void k_kmers_heads(const uint64_t* __restrict__ keys, int64_t n, uint64_t* __restrict__ head) {
  const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (g >= n) return;
  head[g] = (g == 0 || keys[g] != keys[g - 1]) ? 1ull : 0ull;
}

// K14c: rank[g] = the run heads before row g.  ukeys / ustart hold up to n / n + 1 entries.
__global__ __launch_bounds__(256) void k_kmers_runs(const uint64_t* __restrict__ keys, const uint64_t* __restrict__ head,
                                                    const uint64_t* __restrict__ rank, int64_t n, uint64_t* __restrict__ ukeys,
                                                    uint64_t* __restrict__ ustart, unsigned long long* __restrict__ n_runs) {
  const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (g >= n) return;
  const uint64_t u = rank[g];
  if (head[g]) { ukeys[u] = keys[g]; ustart[u] = (uint64_t)g; }
  if (g == n - 1) { ustart[u + head[g]] = (uint64_t)n; *n_runs = u + head[g]; }
}

__device__ __forceinline__ uint32_t run_count(const uint64_t* __restrict__ ustart, int64_t u) {
  const uint64_t c = ustart[u + 1] - ustart[u];
  return c > 0xffffffffull ? 0xffffffffu : (uint32_t)c;
}

// K14d: hist[min(count, max_mult)] += 1 per run.  Bins below kSpectrumBins are counted in LDS (32-bit: a workgroup sees
// fewer than 2^32 runs) and flushed once per workgroup with one 64-bit atomic per occupied bin; the few runs of a larger
// multiplicity go to HBM directly.
constexpr int kSpectrumBins = 4096;
__global__ __launch_bounds__(256) void k_kmers_spectrum(const uint64_t* __restrict__ ustart, const unsigned long long* __restrict__ n_runs,
                                                        uint32_t max_mult, unsigned long long* __restrict__ hist) {
  __shared__ uint32_t s_h[kSpectrumBins];
  const int tid = (int)threadIdx.x;
  for (int b = tid; b < kSpectrumBins; b += 256) s_h[b] = 0;
  __syncthreads();
  const int64_t D = (int64_t)*n_runs;
  for (int64_t u = (int64_t)blockIdx.x * 256 + tid; u < D; u += (int64_t)gridDim.x * 256) {
    const uint32_t c = run_count(ustart, u), m = c < max_mult ? c : max_mult;
    if (m < (uint32_t)kSpectrumBins) atomicAdd(&s_h[m], 1u);
    else atomicAdd(&hist[m], 1ull);
  }
  __syncthreads();
  const int top = (int)(max_mult < (uint32_t)kSpectrumBins - 1 ? max_mult : (uint32_t)kSpectrumBins - 1);
  for (int b = tid; b <= top; b += 256)
    if (s_h[b]) atomicAdd(&hist[b], (unsigned long long)s_h[b]);
}

// K14e: counts[i] = count(q[i]), 0 where the key is absent; starts (may be null): the first row of its run
__global__ __launch_bounds__(256) void k_kmers_lookup(const uint64_t* __restrict__ ukeys, const uint64_t* __restrict__ ustart,
                                                      const unsigned long long* __restrict__ n_runs, const uint64_t* __restrict__ q,
                                                      int64_t n, uint32_t* __restrict__ counts, uint64_t* __restrict__ starts) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int64_t D = (int64_t)*n_runs;
  const uint64_t key = q[i];
  const int64_t u = lower_bound_dev<uint64_t>(ukeys, D, key);
  const bool found = u < D && ukeys[u] == key;
  counts[i] = found ? run_count(ustart, u) : 0u;
  if (starts) starts[i] = found ? ustart[u] : 0ull;
}

// K14f: the run of row g is the last one that starts at or before it; rstart[r] = the forward rows of the reads before r
__global__ __launch_bounds__(256) void k_kmers_occ(const uint64_t* __restrict__ hits, int64_t n, const uint64_t* __restrict__ ustart,
                                                   const unsigned long long* __restrict__ n_runs, const uint64_t* __restrict__ rstart,
                                                   uint32_t* __restrict__ occ) {
  const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (g >= n) return;
  const uint64_t v = hits[g];
  if (v & kStrandBit) return;
  const int64_t D = (int64_t)*n_runs;
  const int64_t u = upper_bound_dev<uint64_t>(ustart, D, (uint64_t)g) - 1;
  occ[rstart[v >> 32] + (v & (kStrandBit - 1))] = run_count(ustart, u);
}

// K15d: K14f of a sampled table.  fhits: the hits of the sampled forward rows in (read, pos) order (they ascend): the place of
// a forward row among them is where its run's length goes.
__global__ __launch_bounds__(256) void k_mini_occ(const uint64_t* __restrict__ hits, int64_t n, const uint64_t* __restrict__ ustart,
                                                  const unsigned long long* __restrict__ n_runs, const uint64_t* __restrict__ fhits,
                                                  int64_t n_fwd, uint32_t* __restrict__ occ) {
  const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (g >= n) return;
  const uint64_t v = hits[g];
  if (v & kStrandBit) return;
  const int64_t D = (int64_t)*n_runs;
  const int64_t u = upper_bound_dev<uint64_t>(ustart, D, (uint64_t)g) - 1;
  occ[lower_bound_dev<uint64_t>(fhits, n_fwd, v)] = run_count(ustart, u);
}

}  // namespace

struct pw_kmer_index {
  int device = 0, L = 0, k = 0, kbits = 0, strands = 0;
  bool built = false;
  int64_t R = 0;
  uint64_t K = 0, N = 0;                               // forward rows, rows
  uint64_t P = 0;                                      // forward positions: K, more where the table is sampled
  bool sampled = false;                                // built with a window above 1
  MiniSample mini; DeviceArray<uint64_t> fhits;        // (sampled) the selection; the forward hits in (read, pos) order
  int64_t D = -1;                                      // distinct keys; -1: still on the device (n_runs)
  hipStream_t stream = nullptr;
  DeviceArray<uint8_t> arena, comp; DeviceArray<uint64_t> roff, rstart; DeviceArray<int32_t> rlen;     // the reads
  DeviceArray<uint64_t> kin, vin, keys, hits;          // staging (after the sort: run heads, ranks), the sorted table
  DeviceArray<uint64_t> ukeys, ustart; DeviceArray<unsigned long long> n_runs; DeviceBuffer tmp;        // the runs; rocPRIM's scratch
  DeviceEvent bev0, bev1, qev0, qev1;                  // the build, a query
};

namespace {

// waits for the build where its number of runs is still on the device; its device time becomes pw_kmers_last_ms()
int finish_build(pw_kmer_index* x) {
  CHECK(hipSetDevice(x->device));
  if (x->D >= 0) return 0;
  unsigned long long d = 0;
  CHECK(hipMemcpyAsync(&d, x->n_runs.p, sizeof d, hipMemcpyDeviceToHost, x->stream));
  CHECK(hipStreamSynchronize(x->stream));
  CHECK(hipGetLastError());
  float ms = 0.f;
  CHECK(hipEventElapsedTime(&ms, x->bev0.e, x->bev1.e));
  g_ms = (double)ms;
  x->D = (int64_t)d;
  return 0;
}
int ready(pw_kmer_index* x, const char* entry) {
  if (!x || !x->built) { set_err(std::string(entry) + " before a successful pw_kmers_build"); return -1; }
  return finish_build(x);
}
int query_begin(pw_kmer_index* x) { CHECK(hipEventRecord(x->qev0.e, x->stream)); return 0; }
int query_end(pw_kmer_index* x) {
  CHECK(hipEventRecord(x->qev1.e, x->stream));
  CHECK(hipStreamSynchronize(x->stream));
  CHECK(hipGetLastError());
  float ms = 0.f;
  CHECK(hipEventElapsedTime(&ms, x->qev0.e, x->qev1.e));
  g_ms = (double)ms;
  return 0;
}
// counts / first rows of n host keys (starts may be null)
int lookup(pw_kmer_index* x, const uint64_t* keys, int64_t n, uint32_t* counts_out, uint64_t* starts_out) {
  DeviceArray<uint64_t> dq, ds; DeviceArray<uint32_t> dc;
  CHECK(dc.ensure((size_t)n));
  if (starts_out) CHECK(ds.ensure((size_t)n));
  if (upload(set_err, dq, keys, (size_t)n, x->stream) != 0 || query_begin(x) != 0) return -1;
  hipLaunchKernelGGL(k_kmers_lookup, rows_grid((uint64_t)n), kBlock256, 0, x->stream, x->ukeys.p, x->ustart.p, x->n_runs.p, dq.p, n, dc.p,
                     ds.p);
  if (query_end(x) != 0) return -1;
  CHECK(hipMemcpy(counts_out, dc.p, dc.bytes((size_t)n), hipMemcpyDeviceToHost));
  if (starts_out) CHECK(hipMemcpy(starts_out, ds.p, ds.bytes((size_t)n), hipMemcpyDeviceToHost));
  return 0;
}

// the staged rows (kin, vin) -> the sorted table and its runs; ends the build's timing
int sort_and_runs(pw_kmer_index* x, int kbits) {
  const hipStream_t st = x->stream;
  const uint64_t N = x->N;
  CHECK(sort_pairs(x->tmp, x->kin, x->keys, x->vin, x->hits, (size_t)N, kbits, st));
  // the staging buffers are free again: run heads in kin, their ranks in vin
  hipLaunchKernelGGL(k_kmers_heads, rows_grid(N), kBlock256, 0, st, x->keys.p, (int64_t)N, x->kin.p);
  CHECK(scan_u64(x->tmp, x->kin, x->vin, (size_t)N, st));
  hipLaunchKernelGGL(k_kmers_runs, rows_grid(N), kBlock256, 0, st, x->keys.p, x->kin.p, x->vin.p, (int64_t)N, x->ukeys.p, x->ustart.p,
                     x->n_runs.p);
  CHECK(hipEventRecord(x->bev1.e, st));
  CHECK(hipGetLastError());
  x->built = true;
  return 0;
}

// The build of a sampled table, from the uploads on (x->K holds the unsampled forward positions on entry).  The order value
// is canonical exactly when the table holds both strands.  K15a and its scan run first and the host waits for the row count:
// the table's buffers are sized by it, not by the positions.
int build_sampled(pw_kmer_index* x, const uint8_t* arena, uint64_t arena_bytes, const uint64_t* read_off, const int32_t* read_len,
                  const std::vector<uint64_t>& rstart, const uint8_t* complement, int window) {
  const hipStream_t st = x->stream;
  const bool both = x->strands == PW_STRAND_BOTH;
  const int64_t R = x->R;
  const uint64_t P = x->P;
  if (upload(set_err, x->arena, arena, (size_t)arena_bytes, st) != 0 || upload(set_err, x->roff, read_off, (size_t)R, st) != 0 ||
      upload(set_err, x->rlen, read_len, (size_t)R, st) != 0 || upload(set_err, x->rstart, rstart.data(), (size_t)R + 1, st) != 0)
    return -1;
  if (both && upload_complement(set_err, complement, x->L, x->comp, st) != 0) return -1;
  CHECK(x->n_runs.ensure(1));
  CHECK(hipStreamSynchronize(st));                     // the host arrays are the caller's again
  CHECK(hipEventRecord(x->bev0.e, st));
  if (x->mini.count(set_err, x->tmp, x->arena.p, x->roff.p, x->rstart.p, R, P, x->k, x->L, window, both, x->comp.p, st) != 0) return -1;
  const uint64_t K = x->mini.rows, N = both ? 2 * K : K;
  x->K = K; x->N = N;
  CHECK(x->kin.ensure((size_t)N)); CHECK(x->vin.ensure((size_t)N)); CHECK(x->keys.ensure((size_t)N)); CHECK(x->hits.ensure((size_t)N));
  CHECK(x->ukeys.ensure((size_t)N)); CHECK(x->ustart.ensure((size_t)N + 1)); CHECK(x->fhits.ensure((size_t)K));
  x->mini.emit(false, x->arena.p, x->roff.p, x->rstart.p, R, x->k, x->L, x->comp.p, x->kin.p, x->vin.p, st);
  CHECK(hipMemcpyAsync(x->fhits.p, x->vin.p, x->fhits.bytes((size_t)K), hipMemcpyDeviceToDevice, st));
  x->mini.read_starts(x->fhits.p, R, st);
  if (both) {
    x->mini.emit(true, x->arena.p, x->roff.p, x->rstart.p, R, x->k, x->L, x->comp.p, x->kin.p + K, x->vin.p + K, st);
    hipLaunchKernelGGL(k_kmers_tag, rows_grid(K), kBlock256, 0, st, x->vin.p + K, (int64_t)K);
  }
  return sort_and_runs(x, x->kbits);
}

int build(pw_kmer_index* x, const uint8_t* arena, uint64_t arena_bytes, const uint64_t* read_off, const int32_t* read_len,
          int64_t n_reads, int strands, const uint8_t* complement, hipStream_t st, int window = 1) {
  if (!x) { set_err("bad arguments"); return -1; }
  if (strands != PW_STRAND_PLUS && strands != PW_STRAND_BOTH) { set_err("strands must be 1 (+) or 3 (both)"); return -1; }
  if (window < 1 || window > kMiniMaxWindow) { set_err("window must be 1..128"); return -1; }
  if (strands == PW_STRAND_BOTH && check_complement(set_err, complement, x->L) != 0) return -1;
  int kbits = 0;
  if (check_args(set_err, x->L, x->k, n_reads < 0 || n_reads >= (1ll << 31) || (n_reads && (!read_off || !read_len)) || (arena_bytes && !arena),
                 1., 1., 1., false, n_reads,
                 [&](int64_t r) { return read_len[r] < 0 || read_off[r] + (uint64_t)read_len[r] > arena_bytes; }, arena, arena_bytes,
                 &kbits) != 0)
    return -1;
  const bool both = strands == PW_STRAND_BOTH;
  std::vector<uint64_t> rstart((size_t)n_reads + 1);
  uint64_t K = 0;
  for (int64_t r = 0; r < n_reads; r++) { rstart[(size_t)r] = K; K += read_len[r] >= x->k ? (uint64_t)(read_len[r] - x->k + 1) : 0; }
  rstart[(size_t)n_reads] = K;
  if (K >= (1ull << 32)) {
    set_err(both ? "more than 2^32 k-mers in one index: split the read set (with the reverse strand the index holds twice the entries, "
                   "2^32 per strand)"
                 : "more than 2^32 k-mers in one index: split the read set");
    return -1;
  }
  CHECK(hipSetDevice(x->device));
  x->built = false;
  if (x->stream != st && x->D < 0 && x->N) CHECK(hipStreamSynchronize(x->stream));    // (a build still running on another stream)
  uint64_t N = both ? 2 * K : K;
  x->stream = st; x->strands = strands; x->R = n_reads; x->K = K; x->P = K; x->N = N; x->D = N ? -1 : 0;
  x->sampled = window > 1 && N != 0;
  if (N == 0) { x->built = true; return 0; }
  if (x->sampled) return build_sampled(x, arena, arena_bytes, read_off, read_len, rstart, complement, window);
  CHECK(x->kin.ensure((size_t)N)); CHECK(x->vin.ensure((size_t)N)); CHECK(x->keys.ensure((size_t)N)); CHECK(x->hits.ensure((size_t)N));
  CHECK(x->ukeys.ensure((size_t)N)); CHECK(x->ustart.ensure((size_t)N + 1)); CHECK(x->n_runs.ensure(1));
  if (upload(set_err, x->arena, arena, (size_t)arena_bytes, st) != 0 || upload(set_err, x->roff, read_off, (size_t)n_reads, st) != 0 ||
      upload(set_err, x->rlen, read_len, (size_t)n_reads, st) != 0 ||
      upload(set_err, x->rstart, rstart.data(), (size_t)n_reads + 1, st) != 0)
    return -1;
  if (both && upload_complement(set_err, complement, x->L, x->comp, st) != 0) return -1;
  CHECK(hipStreamSynchronize(st));                     // the host arrays (rstart among them) are the caller's again
  CHECK(hipEventRecord(x->bev0.e, st));
  hipLaunchKernelGGL(k_enc_reads, rows_grid(K), kBlock256, 0, st, x->arena.p, x->roff.p, x->rstart.p, n_reads, (int64_t)K, x->k, x->L,
                     x->kin.p, x->vin.p);
  if (both) {
    hipLaunchKernelGGL(k_enc_reads_rc, rows_grid(K), kBlock256, 0, st, x->arena.p, x->roff.p, x->rlen.p, x->rstart.p, n_reads, (int64_t)K,
                       x->k, x->L, x->comp.p, x->kin.p + K, x->vin.p + K);
    hipLaunchKernelGGL(k_kmers_tag, rows_grid(K), kBlock256, 0, st, x->vin.p + K, (int64_t)K);
  }
  return sort_and_runs(x, kbits);
}

}  // namespace

extern "C" {

pw_kmer_index* pw_kmers_create(int device, int alphabet_len, int wordlen) {
  int kbits = 0;
  if (check_args(set_err, alphabet_len, wordlen, false, 1., 1., 1., false, 0, [](int64_t) { return false; }, nullptr, 0, &kbits) != 0)
    return nullptr;
  pw_kmer_index* x = new pw_kmer_index;
  x->device = device; x->L = alphabet_len; x->k = wordlen; x->kbits = kbits;
  auto init = [&]() -> int {
    CHECK(hipSetDevice(device));
    CHECK(x->bev0.create()); CHECK(x->bev1.create()); CHECK(x->qev0.create()); CHECK(x->qev1.create());
    return 0;
  };
  if (init() != 0) { delete x; return nullptr; }
  return x;
}

int pw_kmers_build(pw_kmer_index* x, const uint8_t* arena, uint64_t arena_bytes, const uint64_t* read_off, const int32_t* read_len,
                   int64_t n_reads, int strands, const uint8_t* complement, void* stream) {
  return build(x, arena, arena_bytes, read_off, read_len, n_reads, strands, complement, (hipStream_t)stream);
}

int pw_kmers_build_sampled(pw_kmer_index* x, const uint8_t* arena, uint64_t arena_bytes, const uint64_t* read_off, const int32_t* read_len,
                           int64_t n_reads, int strands, const uint8_t* complement, int window, void* stream) {
  return build(x, arena, arena_bytes, read_off, read_len, n_reads, strands, complement, (hipStream_t)stream, window);
}

int64_t pw_kmers_num_positions(const pw_kmer_index* x) { return x && x->built ? (int64_t)x->P : -1; }

int pw_kmers_rows(pw_kmer_index* x, uint64_t* keys_out, uint64_t* hits_out, int64_t cap) {
  if (ready(x, "pw_kmers_rows") != 0) return -1;
  if (cap < (int64_t)x->N) { set_err("pw_kmers_rows: capacity too small"); return -1; }
  if (x->N == 0) return 0;
  if (!keys_out || !hits_out) { set_err("bad arguments"); return -1; }
  CHECK(hipMemcpy(keys_out, x->keys.p, x->keys.bytes((size_t)x->N), hipMemcpyDeviceToHost));
  CHECK(hipMemcpy(hits_out, x->hits.p, x->hits.bytes((size_t)x->N), hipMemcpyDeviceToHost));
  return 0;
}

int pw_kmers_read_starts(pw_kmer_index* x, uint64_t* out) {
  if (ready(x, "pw_kmers_read_starts") != 0) return -1;
  if (!out) { set_err("bad arguments"); return -1; }
  const size_t n = (size_t)x->R + 1;
  if (x->N == 0) { std::fill(out, out + n, 0ull); return 0; }
  CHECK(hipMemcpy(out, x->sampled ? x->mini.starts.p : x->rstart.p, n * sizeof(uint64_t), hipMemcpyDeviceToHost));
  return 0;
}

int64_t pw_kmers_num_entries(const pw_kmer_index* x) { return x && x->built ? (int64_t)x->N : -1; }

int64_t pw_kmers_num_distinct(const pw_kmer_index* x) {
  pw_kmer_index* m = const_cast<pw_kmer_index*>(x);    // (the handle's cache of a number the device holds)
  return ready(m, "pw_kmers_num_distinct") != 0 ? -1 : m->D;
}

int pw_kmers_distinct(pw_kmer_index* x, uint64_t* keys_out, uint32_t* counts_out, int64_t cap) {
  if (ready(x, "pw_kmers_distinct") != 0) return -1;
  if (cap < x->D) { set_err("pw_kmers_distinct: capacity too small"); return -1; }
  if (x->D == 0) return 0;
  if (!keys_out || !counts_out) { set_err("bad arguments"); return -1; }
  std::vector<uint64_t> start((size_t)x->D + 1);
  CHECK(hipMemcpy(keys_out, x->ukeys.p, x->ukeys.bytes((size_t)x->D), hipMemcpyDeviceToHost));
  CHECK(hipMemcpy(start.data(), x->ustart.p, x->ustart.bytes((size_t)x->D + 1), hipMemcpyDeviceToHost));
  for (int64_t u = 0; u < x->D; u++) counts_out[u] = (uint32_t)std::min<uint64_t>(start[(size_t)u + 1] - start[(size_t)u], 0xffffffffull);
  return 0;
}

int pw_kmers_lookup(pw_kmer_index* x, const uint64_t* keys, int64_t n, uint32_t* counts_out) {
  if (ready(x, "pw_kmers_lookup") != 0) return -1;
  if (n < 0 || (n && (!keys || !counts_out))) { set_err("bad arguments"); return -1; }
  if (n == 0) return 0;
  if (x->D == 0) { std::fill(counts_out, counts_out + n, 0u); return 0; }
  return lookup(x, keys, n, counts_out, nullptr);
}

int pw_kmers_hits(pw_kmer_index* x, uint64_t key, uint64_t* hits_out, int64_t cap, int64_t* n_out) {
  if (ready(x, "pw_kmers_hits") != 0) return -1;
  if (!n_out || cap < 0 || (cap && !hits_out)) { set_err("bad arguments"); return -1; }
  *n_out = 0;
  if (x->D == 0) return 0;
  uint32_t count = 0; uint64_t start = 0;
  if (lookup(x, &key, 1, &count, &start) != 0) return -1;
  *n_out = (int64_t)count;
  if ((int64_t)count > cap) {
    char msg[160];
    snprintf(msg, sizeof msg, "pw_kmers_hits: the k-mer has %u hits (capacity %lld)", count, (long long)cap);
    set_err(msg);
    return -1;
  }
  if (count) CHECK(hipMemcpy(hits_out, x->hits.p + start, x->hits.bytes(count), hipMemcpyDeviceToHost));
  return 0;
}

int pw_kmers_spectrum(pw_kmer_index* x, int max_mult, uint64_t* hist_out) {
  if (ready(x, "pw_kmers_spectrum") != 0) return -1;
  if (max_mult < 1 || max_mult > 65536) { set_err("max_mult must be 1..65536"); return -1; }
  if (!hist_out) { set_err("bad arguments"); return -1; }
  DeviceArray<unsigned long long> dh;
  const size_t bins = (size_t)max_mult + 1, bytes = dh.bytes(bins);
  memset(hist_out, 0, bytes);
  if (x->D == 0) return 0;
  CHECK(dh.ensure(bins));
  CHECK(hipMemsetAsync(dh.p, 0, bytes, x->stream));
  if (query_begin(x) != 0) return -1;
  // a fixed grid: every workgroup flushes its LDS histogram once, whatever the table's size
  const unsigned blocks = (unsigned)std::min<uint64_t>(((uint64_t)x->D + 255) / 256, 2048);
  hipLaunchKernelGGL(k_kmers_spectrum, dim3(blocks), kBlock256, 0, x->stream, x->ustart.p, x->n_runs.p, (uint32_t)max_mult, dh.p);
  if (query_end(x) != 0) return -1;
  CHECK(hipMemcpy(hist_out, dh.p, bytes, hipMemcpyDeviceToHost));
  return 0;
}

int pw_kmers_occurrences(pw_kmer_index* x, uint32_t* occ_out) {
  if (ready(x, "pw_kmers_occurrences") != 0) return -1;
  if (x->K == 0) return 0;
  if (!occ_out) { set_err("bad arguments"); return -1; }
  DeviceArray<uint32_t> docc;
  CHECK(docc.ensure((size_t)x->K));
  if (query_begin(x) != 0) return -1;
  if (x->sampled)
    hipLaunchKernelGGL(k_mini_occ, rows_grid(x->N), kBlock256, 0, x->stream, x->hits.p, (int64_t)x->N, x->ustart.p, x->n_runs.p, x->fhits.p,
                       (int64_t)x->K, docc.p);
  else
    hipLaunchKernelGGL(k_kmers_occ, rows_grid(x->N), kBlock256, 0, x->stream, x->hits.p, (int64_t)x->N, x->ustart.p, x->n_runs.p, x->rstart.p,
                       docc.p);
  if (query_end(x) != 0) return -1;
  CHECK(hipMemcpy(occ_out, docc.p, docc.bytes((size_t)x->K), hipMemcpyDeviceToHost));
  return 0;
}

void pw_kmers_destroy(pw_kmer_index* x) {
  if (!x) return;
  (void)hipSetDevice(x->device);
  if (x->built && x->N) (void)hipStreamSynchronize(x->stream);
  delete x;
}

double pw_kmers_last_ms(void) { return g_ms; }
const char* pw_kmers_last_error(void) { return g_err.c_str(); }

}  // extern "C"

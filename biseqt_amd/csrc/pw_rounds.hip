// pw_rounds.hip -- K20: iterated contig consensus (include/pw_rounds.h holds the contract: the column polish and its
// coordinate map, the remap of the placements, the relayout).
//   - The column polish (k_round_count, k_round_offsets, k_round_write): one lane per column, one workgroup per chunk of 256
//     columns of one read; the host lists the chunks, so no kernel searches for its read.  The count pass runs the rule of
//     K16 (pw_polish_column.h, the one definition) once per column and keeps what it emitted -- a byte for the count, a
//     64-bit word for the first eight letters and a byte for the ninth -- so that the write pass reads 9 + 8 bytes a column
//     and no counter.  Between them one exclusive scan (rocPRIM, through rocprim_run) over the n_cols + 1 counts IS the
//     coordinate map.  The statistics of a read are wavefront sums and one integer atomic add per field and wavefront into
//     zeroed records: integer sums do not depend on arrival order.
//   - The relayout (k_round_init, k_round_remap, k_round_lengths, k_round_task_count, k_round_task_write): one thread per
//     read or contig.  A position is remapped with one or two reads of the map; the tasks are the tasks of K18 with the
//     lengths and positions taken from arrays (the window is the one definition of pw_cons_window.h); the arena is written
//     by K18's own two writers (pw_consensus_launch.h) from the polished letters.
// No kernel waits for another workgroup: every dependency is a launch boundary on the stream.  No LDS, no scratch.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <cstring>
#include <rocprim/rocprim.hpp>

#include "../../include/pw_rounds.h"
#include "pw_cons_window.h"
#include "pw_polish_column.h"
#include "pw_rounds_launch.h"

static_assert(sizeof(pw::RoundBlock) == 8, "chunk record must be 8 bytes");
static_assert(pw::kRoundChunk == 256, "the column kernels are written for chunks of 256 columns");

namespace pw {

namespace {

#define RD_TRY(call) do { const hipError_t e_ = (call); if (e_ != hipSuccess) return e_; } while (0)

struct RoundWiden {
  __host__ __device__ uint64_t operator()(uint8_t v) const { return (uint64_t)v; }
};

hipError_t round_sums(DeviceBuffer& tmp, const uint64_t* in, uint64_t* out, size_t n, hipStream_t st) {
  return rocprim_run(tmp, [&](void* t, size_t& b) {
    return rocprim::exclusive_scan(t, b, in, out, (uint64_t)0, n, rocprim::plus<uint64_t>(), st);
  });
}

}  // namespace

// One lane per column of a read: e[col], the column's letters (word, ninth) and the read's statistics.  stats is zeroed
// before; columns outside every read keep the zero that e was filled with.
__global__ __launch_bounds__(256) void k_round_count(const uint32_t* __restrict__ counts, const uint32_t* __restrict__ ins,
                                                     const uint8_t* __restrict__ letters, const long long* __restrict__ roff,
                                                     const int* __restrict__ rlen, const RoundBlock* __restrict__ blocks, int L, int J,
                                                     uint32_t min_depth, uint8_t* __restrict__ e, unsigned long long* __restrict__ word,
                                                     uint8_t* __restrict__ ninth, pw_polish_stats* __restrict__ stats) {
  const RoundBlock b = blocks[blockIdx.x];
  const long long x = (long long)b.chunk * 256 + threadIdx.x;
  uint32_t st = 0;
  if (x < (long long)rlen[b.read]) {
    const long long col = roff[b.read] + x;
    uint32_t len = 0, nin = 0;
    unsigned long long w = 0;
    st = po_column(counts + col * (L + 2), ins ? ins + col * (long long)J * L : nullptr, (int)letters[col], L, J, min_depth,
                   [&](uint8_t y) {
                     if (len < 8) w |= (unsigned long long)y << (8 * len); else nin = y;
                     len++;
                   });
    e[col] = (uint8_t)len;
    word[col] = w;
    ninth[col] = (uint8_t)nin;
  }
  uint32_t kept = st & 0xffu, subst = (st >> 8) & 0xffu, del = (st >> 16) & 0xffu, insd = st >> 24;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {                      // (every lane takes part: the columns past the read's end add 0)
    kept += __shfl_xor(kept, o, 64); subst += __shfl_xor(subst, o, 64);
    del += __shfl_xor(del, o, 64); insd += __shfl_xor(insd, o, 64);
  }
  if ((threadIdx.x & 63u) == 0) {
    pw_polish_stats* s = stats + b.read;
    if (kept) atomicAdd(&s->kept, kept);
    if (subst) atomicAdd(&s->substituted, subst);
    if (del) atomicAdd(&s->deleted, del);
    if (insd) atomicAdd(&s->inserted, insd);
  }
}

// offsets[r] = colmap[roff[r]], offsets[n_reads] = colmap[n_cols]
__global__ __launch_bounds__(256) void k_round_offsets(const unsigned long long* __restrict__ colmap, const long long* __restrict__ roff,
                                                       long long n_reads, long long n_cols, unsigned long long* __restrict__ offsets) {
  const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
  if (r > n_reads) return;
  long long c = r < n_reads ? roff[r] : n_cols;
  c = c < 0 ? 0 : (c > n_cols ? n_cols : c);              // (never: the offsets are validated on the host)
  offsets[r] = colmap[c];
}

// One lane per column of a read: the letters the count pass kept, at colmap[col].
__global__ __launch_bounds__(256) void k_round_write(const uint8_t* __restrict__ e, const unsigned long long* __restrict__ word,
                                                     const uint8_t* __restrict__ ninth, const unsigned long long* __restrict__ colmap,
                                                     const long long* __restrict__ roff, const int* __restrict__ rlen,
                                                     const RoundBlock* __restrict__ blocks, unsigned long long total, uint8_t* __restrict__ out) {
  const RoundBlock b = blocks[blockIdx.x];
  const long long x = (long long)b.chunk * 256 + threadIdx.x;
  if (x >= (long long)rlen[b.read]) return;
  const long long col = roff[b.read] + x;
  const uint32_t len = e[col];
  if (!len) return;
  const unsigned long long at = colmap[col], w = word[col];
  const uint32_t nin = len > 8 ? ninth[col] : 0u;
  for (uint32_t k = 0; k < len; k++)                       // (never past the output: it was allocated from this scan's total)
    if (at + k < total) out[at + k] = (uint8_t)(k < 8 ? (uint32_t)(w >> (8 * k)) & 0xffu : nin);
}

// Round 1: the positions of the placements and the lengths of the build.
__global__ __launch_bounds__(256) void k_round_init(const pw_cons_place* __restrict__ place, const pw_unitig* __restrict__ unitigs,
                                                    long long n_reads, long long n_unitigs, long long* __restrict__ pos,
                                                    long long* __restrict__ len) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i < n_reads) pos[i] = place[i].pos;
  if (i < n_unitigs) len[i] = unitigs[i].length;
}

// ROUND REMAP of include/pw_rounds.h, in place: len and cstart are the CURRENT layout's.
__global__ __launch_bounds__(256) void k_round_remap(const pw_cons_place* __restrict__ place, const long long* __restrict__ len,
                                                     const unsigned long long* __restrict__ cstart, const unsigned long long* __restrict__ colmap,
                                                     long long n_reads, long long n_unitigs, long long* __restrict__ pos) {
  const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
  if (r >= n_reads) return;
  const int u = place[r].unitig;
  if (u < 0 || u >= n_unitigs) return;
  const long long x = pos[r];
  if (x < 0) return;
  const long long n = len[u];
  const unsigned long long cs = cstart[u], base = colmap[cs];
  pos[r] = x <= n ? (long long)(colmap[cs + (unsigned long long)x] - base) : (long long)(colmap[cs + (unsigned long long)n] - base) + (x - n);
}

// n'_u, its padded size (the scan's input) and the flags: 1 a contig of 2^31 letters or more, 2 the polished offsets
// disagree with the map.
__global__ __launch_bounds__(256) void k_round_lengths(const long long* __restrict__ len, const unsigned long long* __restrict__ cstart,
                                                       const unsigned long long* __restrict__ colmap, const unsigned long long* __restrict__ poff,
                                                       long long n_unitigs, long long* __restrict__ len_new, unsigned long long* __restrict__ ulen,
                                                       uint32_t* __restrict__ flag) {
  const long long u = (long long)blockIdx.x * 256 + threadIdx.x;
  if (u >= n_unitigs) return;
  const unsigned long long cs = cstart[u];
  const unsigned long long n = colmap[cs + (unsigned long long)len[u]] - colmap[cs];
  len_new[u] = (long long)n;
  ulen[u] = (n + 3) & ~3ull;
  if (n >= (1ull << 31)) atomicOr(flag, 1u);
  if (poff[u + 1] - poff[u] != n) atomicOr(flag, 2u);
}

// k_cons_task_count of K18 with the position and the length from the round's arrays
__global__ __launch_bounds__(256) void k_round_task_count(const pw_cons_place* __restrict__ place, const long long* __restrict__ pos,
                                                          const int32_t* __restrict__ lens, const long long* __restrict__ len, int n_reads,
                                                          long long n_unitigs, int slack, double drift, unsigned long long* __restrict__ tcnt,
                                                          unsigned long long* __restrict__ msz) {
  const int r = (int)(blockIdx.x * 256 + threadIdx.x);
  if (r >= n_reads) return;
  pw_cons_place p = place[r];
  p.pos = pos[r];
  const int l = lens[r];
  long long lo, hi, radius;
  const bool has = p.unitig >= 0 && p.unitig < n_unitigs && co_window(p, l, len[p.unitig], slack, drift, lo, hi, radius);
  tcnt[r] = has;
  msz[r] = has ? ((unsigned long long)l + 15) / 16 * 16 + 16 : 0ull;
}

// k_cons_task_write of K18 likewise
__global__ __launch_bounds__(256) void k_round_task_write(const pw_cons_place* __restrict__ place, const long long* __restrict__ pos,
                                                          const int32_t* __restrict__ lens, const long long* __restrict__ len,
                                                          const unsigned long long* __restrict__ cstart, const unsigned long long* __restrict__ tcnt,
                                                          const unsigned long long* __restrict__ toff, const unsigned long long* __restrict__ moff,
                                                          long long base, long long n_tasks, int n_reads, int slack, double drift,
                                                          pw_cons_task* __restrict__ tasks) {
  const int r = (int)(blockIdx.x * 256 + threadIdx.x);
  if (r >= n_reads || !tcnt[r]) return;
  const long long t = (long long)toff[r];
  if (t >= n_tasks) return;                                 // (never: the table was allocated from this scan's total)
  pw_cons_place p = place[r];
  p.pos = pos[r];
  const int l = lens[r];
  long long lo, hi, radius;
  if (!co_window(p, l, len[p.unitig], slack, drift, lo, hi, radius)) return;      // (never: tcnt says it has one)
  const long long d0 = p.pos - lo, win = hi - lo;
  const long long dmin = d0 - radius > -(long long)l ? d0 - radius : -(long long)l;
  const long long dmax = d0 + radius < win ? d0 + radius : win;
  tasks[t] = {(int64_t)cstart[p.unitig] + lo, base + (int64_t)moff[r], r, (int32_t)win, (int32_t)dmin, (int32_t)dmax, p.rev, 0};
}

hipError_t round_polish_count(ColumnPolish& cp, const uint32_t* counts, const uint32_t* ins, const uint8_t* letters, const int64_t* roff,
                              const int32_t* rlen, int64_t n_blocks, int64_t n_reads, int64_t n_cols, int L, int J, uint32_t min_depth,
                              uint64_t* offsets, pw_polish_stats* stats, DeviceBuffer& tmp, hipStream_t st) {
  const size_t nC = (size_t)n_cols;
  RD_TRY(cp.d_e.ensure(nC + 1)); RD_TRY(cp.d_word.ensure(nC)); RD_TRY(cp.d_ninth.ensure(nC)); RD_TRY(cp.d_colmap.ensure(nC + 1));
  RD_TRY(hipMemsetAsync(cp.d_e.p, 0, nC + 1, st));
  if (n_reads) RD_TRY(hipMemsetAsync(stats, 0, sizeof(pw_polish_stats) * (size_t)n_reads, st));
  if (n_blocks) {
    hipLaunchKernelGGL(k_round_count, dim3((unsigned)n_blocks), kBlock256, 0, st, counts, ins, letters, (const long long*)roff, rlen,
                       cp.d_blocks.cp(), L, ins ? J : 0, min_depth, cp.d_e.p, cp.d_word.as<unsigned long long>(), cp.d_ninth.p, stats);
    RD_TRY(hipGetLastError());
  }
  RD_TRY(rocprim_run(tmp, [&](void* t, size_t& b) {
    return rocprim::exclusive_scan(t, b, rocprim::make_transform_iterator(cp.d_e.cp(), RoundWiden()), cp.d_colmap.p, (uint64_t)0, nC + 1,
                                   rocprim::plus<uint64_t>(), st);
  }));
  hipLaunchKernelGGL(k_round_offsets, rows_grid((uint64_t)n_reads + 1), kBlock256, 0, st, cp.d_colmap.as<const unsigned long long>(),
                     (const long long*)roff, (long long)n_reads, (long long)n_cols, (unsigned long long*)offsets);
  return hipGetLastError();
}

hipError_t round_polish_write(const ColumnPolish& cp, const int64_t* roff, const int32_t* rlen, int64_t n_blocks, uint64_t total, uint8_t* out,
                              hipStream_t st) {
  if (n_blocks <= 0 || total == 0) return hipSuccess;
  hipLaunchKernelGGL(k_round_write, dim3((unsigned)n_blocks), kBlock256, 0, st, cp.d_e.cp(), cp.d_word.as<const unsigned long long>(),
                     cp.d_ninth.cp(), cp.d_colmap.as<const unsigned long long>(), (const long long*)roff, rlen, cp.d_blocks.cp(),
                     (unsigned long long)total, out);
  return hipGetLastError();
}

hipError_t round_init(const GraphState& g, const ConsState& c, RoundState& r, hipStream_t st) {
  const int64_t R = g.n_reads, U = g.n_unitigs;
  r.have = false;
  RD_TRY(r.d_pos.ensure((size_t)R)); RD_TRY(r.d_len[0].ensure((size_t)U)); RD_TRY(r.d_len[1].ensure((size_t)U));
  r.cur = 0;
  if (R || U) {
    hipLaunchKernelGGL(k_round_init, rows_grid((uint64_t)(R > U ? R : U)), kBlock256, 0, st, c.d_place.cp(), g.d_unitigs.cp(), (long long)R,
                       (long long)U, (long long*)r.d_pos.p, (long long*)r.d_len[0].p);
    RD_TRY(hipGetLastError());
  }
  RD_TRY(hipStreamSynchronize(st));
  r.have = true;
  return hipSuccess;
}

hipError_t round_relayout(const GraphState& g, ConsState& c, RoundState& r, const uint8_t* polished, const uint64_t* poffs,
                          const uint64_t* colmap, const uint8_t* letters, int32_t slack, double drift, int* refused, hipStream_t st) {
  const int64_t R = g.n_reads, U = g.n_unitigs;
  const size_t nR = (size_t)R, nU = (size_t)U;
  *refused = 0;
  if (!r.have) RD_TRY(round_init(g, c, r, st));
  c.has_layout = false;
  // ---- the caller's arrays: the letters and their offsets are copied, the map is consumed by the two kernels below ----
  uint64_t ptotal = 0;
  RD_TRY(hipMemcpyAsync(&ptotal, poffs + U, 8, hipMemcpyDeviceToHost, st));
  RD_TRY(hipStreamSynchronize(st));
  RD_TRY(r.d_pol.ensure((size_t)ptotal)); RD_TRY(r.d_poff.ensure(nU + 1));
  if (ptotal) RD_TRY(hipMemcpyAsync(r.d_pol.p, polished, (size_t)ptotal, hipMemcpyDeviceToDevice, st));
  RD_TRY(hipMemcpyAsync(r.d_poff.p, poffs, 8 * (nU + 1), hipMemcpyDeviceToDevice, st));
  // ---- positions, lengths and the padded contig starts of the next round ----
  const long long* len_old = (const long long*)r.d_len[r.cur].cp();
  long long* len_new = (long long*)r.d_len[r.cur ^ 1].p;
  RD_TRY(hipMemsetAsync(c.d_ulen.p + U, 0, 8, st));
  RD_TRY(hipMemsetAsync(c.d_flag.p, 0, 4, st));
  if (R) {
    hipLaunchKernelGGL(k_round_remap, rows_grid((uint64_t)R), kBlock256, 0, st, c.d_place.cp(), len_old, c.d_cstart.as<const unsigned long long>(),
                       (const unsigned long long*)colmap, (long long)R, (long long)U, (long long*)r.d_pos.p);
    RD_TRY(hipGetLastError());
  }
  if (U) {
    hipLaunchKernelGGL(k_round_lengths, rows_grid((uint64_t)U), kBlock256, 0, st, len_old, c.d_cstart.as<const unsigned long long>(),
                       (const unsigned long long*)colmap, r.d_poff.as<const unsigned long long>(), (long long)U, len_new,
                       c.d_ulen.as<unsigned long long>(), c.d_flag.p);
    RD_TRY(hipGetLastError());
  }
  r.have = false;                                           // (the positions are the next round's from here; a failure leaves no layout)
  RD_TRY(round_sums(c.tmp, c.d_ulen.cp(), c.d_cstart.p, nU + 1, st));
  // ---- the task count and the frames' sizes ----
  RD_TRY(hipMemsetAsync(c.d_tcnt.p + R, 0, 8, st));
  RD_TRY(hipMemsetAsync(c.d_msz.p + R, 0, 8, st));
  if (R) {
    hipLaunchKernelGGL(k_round_task_count, rows_grid((uint64_t)R), kBlock256, 0, st, c.d_place.cp(), (const long long*)r.d_pos.cp(), g.d_lens.cp(),
                       (const long long*)len_new, (int)R, (long long)U, (int)slack, drift, c.d_tcnt.as<unsigned long long>(),
                       c.d_msz.as<unsigned long long>());
    RD_TRY(hipGetLastError());
  }
  RD_TRY(round_sums(c.tmp, c.d_tcnt.cp(), c.d_toff.p, nR + 1, st));
  RD_TRY(round_sums(c.tmp, c.d_msz.cp(), c.d_moff.p, nR + 1, st));
  uint64_t n_cols = 0, n_tasks = 0, frames = 0;
  uint32_t flag = 0;
  RD_TRY(hipMemcpyAsync(&n_cols, c.d_cstart.p + U, 8, hipMemcpyDeviceToHost, st));
  RD_TRY(hipMemcpyAsync(&n_tasks, c.d_toff.p + R, 8, hipMemcpyDeviceToHost, st));
  RD_TRY(hipMemcpyAsync(&frames, c.d_moff.p + R, 8, hipMemcpyDeviceToHost, st));
  RD_TRY(hipMemcpyAsync(&flag, c.d_flag.p, 4, hipMemcpyDeviceToHost, st));
  RD_TRY(hipStreamSynchronize(st));                         // the task table and the arena are allocated from the counted totals
  if (flag) { *refused = (flag & 1u) ? 1 : 2; return hipSuccess; }
  const uint64_t base = (n_cols + 15) & ~(uint64_t)15, arena_bytes = base + frames + 16;
  RD_TRY(c.d_tasks.ensure((size_t)n_tasks));
  RD_TRY(c.d_arena.ensure((size_t)arena_bytes + 16));
  RD_TRY(hipMemsetAsync(c.d_arena.p, 0, (size_t)arena_bytes + 16, st));
  if (n_tasks) {
    hipLaunchKernelGGL(k_round_task_write, rows_grid((uint64_t)R), kBlock256, 0, st, c.d_place.cp(), (const long long*)r.d_pos.cp(), g.d_lens.cp(),
                       (const long long*)len_new, c.d_cstart.as<const unsigned long long>(), c.d_tcnt.as<const unsigned long long>(),
                       c.d_toff.as<const unsigned long long>(), c.d_moff.as<const unsigned long long>(), (long long)base, (long long)n_tasks,
                       (int)R, (int)slack, drift, c.d_tasks.p);
    RD_TRY(hipGetLastError());
  }
  RD_TRY(cons_arena_contigs(c, r.d_pol.cp(), r.d_poff.cp(), U, (int64_t)n_cols, st));
  RD_TRY(cons_arena_mutants(g, c, letters, (int64_t)n_tasks, (int64_t)arena_bytes, st));
  RD_TRY(hipStreamSynchronize(st));
  c.n_tasks = (int64_t)n_tasks; c.n_cols = (int64_t)n_cols; c.arena_bytes = (int64_t)arena_bytes; c.has_layout = true;
  r.cur ^= 1; r.have = true; r.round++;
  return hipSuccess;
}

int64_t round_device_bytes(const RoundState& r) {
  size_t b = 0;
  auto add = [&b](const auto& a) { if (a.p) b += a.bytes(a.cap); };
  add(r.d_pos); add(r.d_len[0]); add(r.d_len[1]); add(r.d_pol); add(r.d_poff);
  return (int64_t)b;
}

}  // namespace pw

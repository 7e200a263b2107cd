// pw_consensus.hip -- K18: the consensus stage's layout (include/pw_consensus.h holds the contract: placements, tasks, the
// consensus arena).  The graph is read through GraphState (pw_graph_launch.h) and never written.  One thread per record,
// read, member, unitig or arena dword everywhere except in k_cons_arena_mutants, where one wavefront per task copies (or
// reverse-complements) the task's read into its mutant frame, a dword of four letters per lane and step.
//   - Parent selection (k_cons_parent): one 64-bit atomic max per containment record, of n_match << 32 | ~index; the winner
//     does not depend on arrival order.
//   - Chains (k_cons_chain_init, k_cons_double): pointer doubling over the parent links, one launch per round on ping-pong
//     buffers, the round count fixed from the number of reads alone.  A read that has reached no member after the last
//     round lies on, or leads into, a containment cycle and stays unplaced.
//   - Roots (k_cons_roots, k_cons_place): every member offers its index to its read with a 32-bit atomic min -- the lowest
//     member index wins -- and every read composes its chain with the winner of its root.
//   - Tasks (k_cons_contig_pad, k_cons_task_count, k_cons_task_write): counted, scanned (rocPRIM, through rocprim_run), the
//     totals waited for, the arrays allocated from them, then written.
//   - The arena (k_cons_arena_contigs, k_cons_arena_mutants): the contig letters at their padded starts with 255 between
//     them; the mutant frames behind.
// No kernel waits for another workgroup: every dependency is a launch boundary on the stream.  No LDS, no scratch.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <cstring>
#include <rocprim/rocprim.hpp>

#include "../../include/pw_consensus.h"
#include "pw_consensus_launch.h"
#include "pw_cons_window.h"

static_assert(sizeof(pw_cons_place) == 24, "placement record must be 24 bytes");
static_assert(sizeof(pw_cons_task) == 40, "task record must be 40 bytes");
static_assert(sizeof(pw::ConsChain) == 24, "doubling state must be 24 bytes");

namespace pw {

namespace {

#define CO_TRY(call) do { const hipError_t e_ = (call); if (e_ != hipSuccess) return e_; } while (0)

// The composition of include/pw_consensus.h: a child (rel_c, off_c) of lc letters on a read of lp letters that is itself
// placed with (rel_p, off_p).
__device__ __forceinline__ void co_compose(int rel_p, long long off_p, int lp, int lc, int& rel_c, long long& off_c) {
  if (rel_p == 0) { off_c = off_p + off_c; }
  else { off_c = off_p + (long long)lp - off_c - (long long)lc; rel_c ^= 1; }
}

}  // namespace

// best[c] of the read a containment record contains, and of a dropped read that a dovetail record joins to a live one: the
// largest n_match << 32 | ~index (best is zeroed before).  A dropped read is never contained, so the two kinds of offer never
// meet in one entry.
__global__ __launch_bounds__(256) void k_cons_parent(const pw_graph_overlap* __restrict__ recs, long long n, long long n_reads,
                                                     const uint8_t* __restrict__ contained, const uint8_t* __restrict__ dropped,
                                                     unsigned long long* __restrict__ best) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const pw_graph_overlap& r = recs[i];
  const int cls = r.cls;
  if (cls < PW_OVL_A_CONTAINED) return;
  if ((unsigned long long)r.a >= (unsigned long long)n_reads || (unsigned long long)r.b >= (unsigned long long)n_reads) return;      // (never: read indices are validated when a record is added)
  int c;
  if (cls == PW_OVL_A_CONTAINED) c = r.a;
  else if (cls == PW_OVL_B_CONTAINED) c = r.b;
  else {                                                    // a dovetail: the dropped side hangs on the live side
    const bool live_a = !(contained[r.a] | dropped[r.a]), live_b = !(contained[r.b] | dropped[r.b]);
    if (dropped[r.a] && live_b) c = r.a;
    else if (dropped[r.b] && live_a) c = r.b;
    else return;
  }
  atomicMax(&best[c], ((unsigned long long)(uint32_t)r.n_match << 32) | (uint32_t)~(uint32_t)i);
}

// Round 0 of the doubling: a contained read stands on its parent, one link up; every other read on itself.
__global__ __launch_bounds__(256) void k_cons_chain_init(const pw_graph_overlap* __restrict__ recs, long long n_recs,
                                                         const unsigned long long* __restrict__ best, const int32_t* __restrict__ lens,
                                                         int n_reads, ConsChain* __restrict__ st) {
  const int r = (int)(blockIdx.x * 256 + threadIdx.x);
  if (r >= n_reads) return;
  ConsChain c = {0, r, -1, 0, 0};
  const unsigned long long key = best[r];
  const uint32_t i = ~(uint32_t)key;
  if (key != 0 && (long long)i < n_recs) {
    const pw_graph_overlap rec = recs[i];
    const bool a_child = rec.a == r;                        // (A_CONTAINED, or the dropped read of a dovetail; a != b)
    const int parent = a_child ? rec.b : rec.a;
    if ((uint32_t)parent < (uint32_t)n_reads) {             // (always)
      const long long delta = a_child ? (long long)rec.b_beg - rec.a_beg : (long long)rec.a_beg - rec.b_beg;
      const long long off = (a_child && rec.strand) ? (long long)lens[rec.b] - delta - (long long)lens[rec.a] : delta;
      c = {off, parent, parent, rec.strand ? 1 : 0, 1};
    }
  }
  st[r] = c;
}

// One round: the state of the read nxt is appended to the read's own.
__global__ __launch_bounds__(256) void k_cons_double(const ConsChain* __restrict__ in, ConsChain* __restrict__ out,
                                                     const int32_t* __restrict__ lens, int n_reads) {
  const int r = (int)(blockIdx.x * 256 + threadIdx.x);
  if (r >= n_reads) return;
  ConsChain c = in[r];
  if (c.nxt >= 0 && c.nxt < n_reads) {
    const ConsChain q = in[c.nxt];
    int rel = c.rel;
    long long off = c.off;
    co_compose(q.rel, q.off, lens[c.f], lens[r], rel, off);
    c = {off, q.f, q.nxt, rel, c.d + q.d};
  }
  out[r] = c;
}

// first[r] = the lowest member index of read r (filled with 0x7f7f7f7f before)
__global__ __launch_bounds__(256) void k_cons_roots(const pw_unitig_member* __restrict__ members, long long n_members, long long n_reads,
                                                    int32_t* __restrict__ first) {
  const long long m = (long long)blockIdx.x * 256 + threadIdx.x;
  if (m >= n_members) return;
  const int r = members[m].vertex >> 1;
  if ((unsigned long long)r >= (unsigned long long)n_reads) return;  // (never)
  atomicMin(&first[r], (int32_t)m);
}

// Every read composes its chain with the member record of its root.
__global__ __launch_bounds__(256) void k_cons_place(const ConsChain* __restrict__ st, const int32_t* __restrict__ first,
                                                    const pw_unitig_member* __restrict__ members, const int32_t* __restrict__ mem_uid,
                                                    const int32_t* __restrict__ lens, int n_reads, long long n_members,
                                                    pw_cons_place* __restrict__ place) {
  const int r = (int)(blockIdx.x * 256 + threadIdx.x);
  if (r >= n_reads) return;
  const ConsChain c = st[r];
  pw_cons_place p = {-1, 0, 0, 0, 0};
  if (c.nxt < 0 && (uint32_t)c.f < (uint32_t)n_reads) {
    const long long m = first[c.f];
    if (m < n_members) {
      const pw_unitig_member mem = members[m];
      int rel = c.rel;
      long long off = c.off;
      co_compose(mem.vertex & 1, (long long)mem.offset, lens[c.f], lens[r], rel, off);
      p = {mem_uid[m], rel, off, c.f, c.d};
    }
  }
  place[r] = p;
}

// ulen[u] = the letters of contig u rounded up to a multiple of 4 (the scan's input); flag: a contig of 2^31 letters or more
__global__ __launch_bounds__(256) void k_cons_contig_pad(const pw_unitig* __restrict__ unitigs, long long n, unsigned long long* __restrict__ ulen,
                                                         uint32_t* __restrict__ flag) {
  const long long u = (long long)blockIdx.x * 256 + threadIdx.x;
  if (u >= n) return;
  const long long len = unitigs[u].length;
  ulen[u] = (unsigned long long)((len + 3) & ~3ll);
  if (len < 0 || len >= (1ll << 31)) atomicOr(flag, 1u);
}

// tcnt[r] = 1 for a read with a task, msz[r] = the bytes of its mutant frame (the inputs of the two scans)
__global__ __launch_bounds__(256) void k_cons_task_count(const pw_cons_place* __restrict__ place, const int32_t* __restrict__ lens,
                                                         const pw_unitig* __restrict__ unitigs, int n_reads, long long n_unitigs, int slack,
                                                         double drift, unsigned long long* __restrict__ tcnt, unsigned long long* __restrict__ msz) {
  const int r = (int)(blockIdx.x * 256 + threadIdx.x);
  if (r >= n_reads) return;
  const pw_cons_place p = place[r];
  const int l = lens[r];
  long long lo, hi, radius;
  const bool has = p.unitig >= 0 && p.unitig < n_unitigs && co_window(p, l, unitigs[p.unitig].length, slack, drift, lo, hi, radius);
  tcnt[r] = has;
  msz[r] = has ? ((unsigned long long)l + 15) / 16 * 16 + 16 : 0ull;
}

// The task of every read that has one, at its scanned position.
__global__ __launch_bounds__(256) void k_cons_task_write(const pw_cons_place* __restrict__ place, const int32_t* __restrict__ lens,
                                                         const pw_unitig* __restrict__ unitigs, const unsigned long long* __restrict__ cstart,
                                                         const unsigned long long* __restrict__ tcnt, const unsigned long long* __restrict__ toff,
                                                         const unsigned long long* __restrict__ moff, long long base, long long n_tasks,
                                                         int n_reads, int slack, double drift, pw_cons_task* __restrict__ tasks) {
  const int r = (int)(blockIdx.x * 256 + threadIdx.x);
  if (r >= n_reads || !tcnt[r]) return;
  const long long t = (long long)toff[r];
  if (t >= n_tasks) return;                                 // (never: the table was allocated from this scan's total)
  const pw_cons_place p = place[r];
  const int l = lens[r];
  long long lo, hi, radius;
  if (!co_window(p, l, unitigs[p.unitig].length, slack, drift, lo, hi, radius)) return;      // (never: tcnt says it has one)
  const long long d0 = p.pos - lo, win = hi - lo;
  const long long dmin = d0 - radius > -(long long)l ? d0 - radius : -(long long)l;
  const long long dmax = d0 + radius < win ? d0 + radius : win;
  tasks[t] = {(int64_t)cstart[p.unitig] + lo, base + (int64_t)moff[r], r, (int32_t)win, (int32_t)dmin, (int32_t)dmax, p.rev, 0};
}

// One thread per dword of the columns [0, n_cols): contig u at cstart[u], 255 behind its last letter.
__global__ __launch_bounds__(256) void k_cons_arena_contigs(const uint8_t* __restrict__ cletters, const unsigned long long* __restrict__ coff,
                                                            const unsigned long long* __restrict__ cstart, long long n_unitigs, long long n_cols,
                                                            uint8_t* __restrict__ arena) {
  const long long w = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long col = 4 * w;
  if (col >= n_cols || n_unitigs <= 0) return;
  long long u = upper_bound_dev(cstart, n_unitigs + 1, (unsigned long long)col) - 1;
  u = u < 0 ? 0 : (u >= n_unitigs ? n_unitigs - 1 : u);
  const unsigned long long src = coff[u], len = coff[u + 1] - src, x = (unsigned long long)col - cstart[u];
  uint32_t word = 0;
#pragma unroll
  for (int k = 0; k < 4; k++) word |= (uint32_t)(x + k < len ? cletters[src + x + k] : (uint8_t)255) << (8 * k);
  *reinterpret_cast<uint32_t*>(arena + col) = word;
}

// One wavefront per task: the read as stored, or reverse-complemented, at mut_off; four letters per lane and step, the
// letters past the read's end 0.  comp: 256 bytes.
__global__ __launch_bounds__(64) void k_cons_arena_mutants(const pw_cons_task* __restrict__ tasks, const uint8_t* __restrict__ letters,
                                                           const long long* __restrict__ roff, const int32_t* __restrict__ lens,
                                                           const uint8_t* __restrict__ comp, long long arena_bytes, uint8_t* __restrict__ arena) {
  const pw_cons_task t = tasks[blockIdx.x];
  const int lane = (int)(threadIdx.x & 63u);
  const int l = lens[t.read];
  const uint8_t* __restrict__ src = letters + roff[t.read];
  for (int i = 4 * lane; i < l; i += 256) {
    if (t.mut_off + i + 4 > arena_bytes) break;             // (never: the arena was allocated from the frames' scanned sizes)
    uint32_t word = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const int x = i + k;
      if (x < l) word |= (uint32_t)(t.rev ? comp[src[l - 1 - x]] : src[x]) << (8 * k);
    }
    *reinterpret_cast<uint32_t*>(arena + t.mut_off + i) = word;
  }
}

namespace {

hipError_t cons_sums(ConsState& c, const uint64_t* in, uint64_t* out, size_t n, hipStream_t st) {
  return rocprim_run(c.tmp, [&](void* t, size_t& b) {
    return rocprim::exclusive_scan(t, b, in, out, (uint64_t)0, n, rocprim::plus<uint64_t>(), st);
  });
}

}  // namespace

hipError_t cons_place(const GraphState& g, ConsState& c, hipStream_t st) {
  const int64_t R = g.n_reads, n = g.n_recs, M = g.n_members;
  const size_t nR = (size_t)R;
  c.placed = false; c.has_layout = false;
  CO_TRY(c.d_best.ensure(nR)); CO_TRY(c.d_chain[0].ensure(nR)); CO_TRY(c.d_chain[1].ensure(nR));
  CO_TRY(c.d_first.ensure(nR)); CO_TRY(c.d_place.ensure(nR));
  if (R) {
    const dim3 rgrid = rows_grid((uint64_t)R);
    CO_TRY(hipMemsetAsync(c.d_best.p, 0, c.d_best.bytes(nR), st));
    CO_TRY(hipMemsetAsync(c.d_first.p, 0x7f, c.d_first.bytes(nR), st));
    if (n) {
      hipLaunchKernelGGL(k_cons_parent, rows_grid((uint64_t)n), kBlock256, 0, st, g.d_recs.cp(), (long long)n, (long long)R,
                         g.d_contained.cp(), g.d_dropped.cp(), c.d_best.as<unsigned long long>());
      CO_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL(k_cons_chain_init, rgrid, kBlock256, 0, st, g.d_recs.cp(), (long long)n, c.d_best.as<const unsigned long long>(),
                       g.d_lens.cp(), (int)R, c.d_chain[0].p);
    CO_TRY(hipGetLastError());
    int rounds = 1;                                         // ceil(log2(max(R, 2))) + 1: fixed from the number of reads alone
    while (((int64_t)1 << rounds) < R) rounds++;
    rounds++;
    int cur = 0;
    for (int k = 0; k < rounds; k++, cur ^= 1) {
      hipLaunchKernelGGL(k_cons_double, rgrid, kBlock256, 0, st, c.d_chain[cur].cp(), c.d_chain[cur ^ 1].p, g.d_lens.cp(), (int)R);
      CO_TRY(hipGetLastError());
    }
    if (M) {
      hipLaunchKernelGGL(k_cons_roots, rows_grid((uint64_t)M), kBlock256, 0, st, g.d_members.cp(), (long long)M, (long long)R, c.d_first.p);
      CO_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL(k_cons_place, rgrid, kBlock256, 0, st, c.d_chain[cur].cp(), c.d_first.cp(), g.d_members.cp(), g.d_mem_uid.cp(),
                       g.d_lens.cp(), (int)R, (long long)M, c.d_place.p);
    CO_TRY(hipGetLastError());
  }
  CO_TRY(hipStreamSynchronize(st));
  c.placed = true;
  return hipSuccess;
}

hipError_t cons_arena_contigs(ConsState& c, const uint8_t* cletters, const uint64_t* coff, int64_t n_unitigs, int64_t n_cols, hipStream_t st) {
  if (n_cols <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_cons_arena_contigs, rows_grid((uint64_t)n_cols / 4), kBlock256, 0, st, cletters, (const unsigned long long*)coff,
                     c.d_cstart.as<const unsigned long long>(), (long long)n_unitigs, (long long)n_cols, c.d_arena.p);
  return hipGetLastError();
}

hipError_t cons_arena_mutants(const GraphState& g, ConsState& c, const uint8_t* letters, int64_t n_tasks, int64_t arena_bytes, hipStream_t st) {
  if (n_tasks <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_cons_arena_mutants, dim3((unsigned)n_tasks), dim3(64), 0, st, c.d_tasks.cp(), letters, (const long long*)c.d_roff.cp(),
                     g.d_lens.cp(), c.d_comp.cp(), (long long)arena_bytes, c.d_arena.p);
  return hipGetLastError();
}

hipError_t cons_layout(const GraphState& g, ConsState& c, const uint8_t* letters, int32_t slack, double drift, bool* too_long,
                       hipStream_t st) {
  const int64_t R = g.n_reads, U = g.n_unitigs;
  const size_t nR = (size_t)R, nU = (size_t)U;
  c.has_layout = false; *too_long = false;
  // ---- the padded contig starts ----
  CO_TRY(c.d_ulen.ensure(nU + 1)); CO_TRY(c.d_cstart.ensure(nU + 1)); CO_TRY(c.d_flag.ensure(1));
  CO_TRY(hipMemsetAsync(c.d_ulen.p + U, 0, 8, st));
  CO_TRY(hipMemsetAsync(c.d_flag.p, 0, 4, st));
  if (U) {
    hipLaunchKernelGGL(k_cons_contig_pad, rows_grid((uint64_t)U), kBlock256, 0, st, g.d_unitigs.cp(), (long long)U,
                       c.d_ulen.as<unsigned long long>(), c.d_flag.p);
    CO_TRY(hipGetLastError());
  }
  CO_TRY(cons_sums(c, c.d_ulen.cp(), c.d_cstart.p, nU + 1, st));
  // ---- the task count and the frames' sizes ----
  CO_TRY(c.d_tcnt.ensure(nR + 1)); CO_TRY(c.d_toff.ensure(nR + 1)); CO_TRY(c.d_msz.ensure(nR + 1)); CO_TRY(c.d_moff.ensure(nR + 1));
  CO_TRY(hipMemsetAsync(c.d_tcnt.p + R, 0, 8, st));
  CO_TRY(hipMemsetAsync(c.d_msz.p + R, 0, 8, st));
  if (R) {
    hipLaunchKernelGGL(k_cons_task_count, rows_grid((uint64_t)R), kBlock256, 0, st, c.d_place.cp(), g.d_lens.cp(), g.d_unitigs.cp(), (int)R,
                       (long long)U, (int)slack, drift, c.d_tcnt.as<unsigned long long>(), c.d_msz.as<unsigned long long>());
    CO_TRY(hipGetLastError());
  }
  CO_TRY(cons_sums(c, c.d_tcnt.cp(), c.d_toff.p, nR + 1, st));
  CO_TRY(cons_sums(c, c.d_msz.cp(), c.d_moff.p, nR + 1, st));
  uint64_t n_cols = 0, n_tasks = 0, frames = 0;
  uint32_t flag = 0;
  CO_TRY(hipMemcpyAsync(&n_cols, c.d_cstart.p + U, 8, hipMemcpyDeviceToHost, st));
  CO_TRY(hipMemcpyAsync(&n_tasks, c.d_toff.p + R, 8, hipMemcpyDeviceToHost, st));
  CO_TRY(hipMemcpyAsync(&frames, c.d_moff.p + R, 8, hipMemcpyDeviceToHost, st));
  CO_TRY(hipMemcpyAsync(&flag, c.d_flag.p, 4, hipMemcpyDeviceToHost, st));
  CO_TRY(hipStreamSynchronize(st));                         // the task table and the arena are allocated from the counted totals
  if (flag) { *too_long = true; return hipSuccess; }
  const uint64_t base = (n_cols + 15) & ~(uint64_t)15, arena_bytes = base + frames + 16;
  CO_TRY(c.d_tasks.ensure((size_t)n_tasks));
  CO_TRY(c.d_arena.ensure((size_t)arena_bytes + 16));
  CO_TRY(hipMemsetAsync(c.d_arena.p, 0, (size_t)arena_bytes + 16, st));
  if (n_tasks) {
    hipLaunchKernelGGL(k_cons_task_write, rows_grid((uint64_t)R), kBlock256, 0, st, c.d_place.cp(), g.d_lens.cp(), g.d_unitigs.cp(),
                       c.d_cstart.as<const unsigned long long>(), c.d_tcnt.as<const unsigned long long>(),
                       c.d_toff.as<const unsigned long long>(), c.d_moff.as<const unsigned long long>(), (long long)base, (long long)n_tasks,
                       (int)R, (int)slack, drift, c.d_tasks.p);
    CO_TRY(hipGetLastError());
  }
  CO_TRY(cons_arena_contigs(c, g.d_cletters.cp(), g.d_coff.cp(), U, (int64_t)n_cols, st));
  CO_TRY(cons_arena_mutants(g, c, letters, (int64_t)n_tasks, (int64_t)arena_bytes, st));
  CO_TRY(hipStreamSynchronize(st));
  c.n_tasks = (int64_t)n_tasks; c.n_cols = (int64_t)n_cols; c.arena_bytes = (int64_t)arena_bytes; c.has_layout = true;
  return hipSuccess;
}

int64_t cons_device_bytes(const ConsState& c) {
  size_t b = c.tmp.cap;
  auto add = [&b](const auto& a) { if (a.p) b += a.bytes(a.cap); };
  add(c.d_best); add(c.d_chain[0]); add(c.d_chain[1]); add(c.d_first); add(c.d_place); add(c.d_roff); add(c.d_comp); add(c.d_ulen);
  add(c.d_cstart); add(c.d_tcnt); add(c.d_toff); add(c.d_msz); add(c.d_moff); add(c.d_flag); add(c.d_tasks); add(c.d_arena);
  return (int64_t)b;
}

}  // namespace pw

// pwlib_api.cpp -- host side of libpwlib (pwlib.so): the batch C ABI of include/pw_batch.h and, on
// top of it, the four drop-in functions of include/pwlib.h (reference biseqt/pwlib/pw.c).
//
// Everything that computes runs in the gfx950 kernels of pw_device.h / pw_trace.hip; this file plans
// (pw_plan.h), moves bytes and launches.  There is no CPU fallback: what the kernels do not support is
// reported as an error.
#include <hip/hip_runtime.h>
#include <math.h>
#include <cmath>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <chrono>
#include <memory>
#include <mutex>
#include <thread>
#include <vector>
#include <unordered_set>

#include "../../include/pw_batch.h"
#include "../../include/pw_txsum.h"
#include "../../include/pw_cigar.h"
#include "../../include/pw_pileup.h"
#include "../../include/pw_polish.h"
#include "../../include/pw_graph.h"
#include "../../include/pw_consensus.h"
#include "../../include/pw_rounds.h"
#include "pw_launch.h"
#include "pw_plan.h"
#include "pw_model.h"
#include "pw_hip_host.h"
#include "pw_complement.h"
#include "pw_graph_launch.h"
#include "pw_consensus_launch.h"
#include "pw_rounds_launch.h"
#define PW_FN inline
#include "pw_strip.h"
#include <atomic>

extern "C" {
#include "../../include/pwlib.h"
}

static_assert(sizeof(pw::Result) == 32 && sizeof(pw_result) == 32, "result record must be 32 bytes");
static_assert(sizeof(pw::PairDesc) == 96, "PairDesc layout");

namespace {
int env_int(const char* name, int dflt);

// A small cache of the big device buffers (tie-mask planes, transcript slots): freeing and re-allocating tens of GB per
// batch stalls in the driver for seconds at a time (measured in the config-4 alignment stage).  Buffers of at least
// 1 MB are kept on pw_batch_destroy, per device up to PWLIB_POOL_GB (default: a quarter of the device's memory; 0
// disables), and handed to the next batch on that device that fits.  pw_pool_trim() releases everything.
struct PoolEntry { void* p; size_t bytes; int device; };
std::mutex g_pool_mutex;
std::vector<PoolEntry> g_pool;
constexpr int kMaxDevices = 64;
size_t g_pool_held[kMaxDevices] = {0};     // bytes parked per device
size_t g_pool_cap[kMaxDevices] = {0};      // 0 = not computed yet

// Cap of the bytes parked on one device: PWLIB_POOL_GB if set (0 disables the pool), otherwise a quarter of the
// device's memory (72 GB on an MI355X), read once per device -- and, at the moment a buffer is parked, never more than
// half of what is FREE on the device then (parked bytes included): several processes sharing a device, or another
// allocator in this process (torch, RCCL), then see the pool shrink instead of an out-of-memory error.
size_t pool_cap(int device) {
  if (device < 0 || device >= kMaxDevices) return 0;
  if (g_pool_cap[device] == 0) {
    const char* v = getenv("PWLIB_POOL_GB");
    size_t cap;
    if (v && *v) cap = (size_t)atoi(v) << 30;
    else {
      size_t fr = 0, tot = 0;
      cap = (hipMemGetInfo(&fr, &tot) == hipSuccess) ? tot / 4 : ((size_t)16 << 30);
    }
    g_pool_cap[device] = cap + 1;            // + 1: "computed" even when the cap itself is 0
  }
  return g_pool_cap[device] - 1;
}
// ... the free-memory half of the rule (the caller holds no lock; the device is current)
size_t pool_room_now(int device, size_t held) {
  static const bool fixed = [] { const char* v = getenv("PWLIB_POOL_GB"); return v && *v; }();
  const size_t cap = pool_cap(device);
  if (fixed) return cap;
  size_t fr = 0, tot = 0;
  if (hipMemGetInfo(&fr, &tot) != hipSuccess) return cap;
  return std::min(cap, (fr + held) / 2);
}

void* pool_take(int device, size_t bytes, size_t* got) {
  std::lock_guard<std::mutex> lk(g_pool_mutex);
  int best = -1;
  // a parked buffer may be up to 25 % (+ 1 MB) larger than asked for: batches of one chunked job differ by less
  for (int i = 0; i < (int)g_pool.size(); i++)
    if (g_pool[i].device == device && g_pool[i].bytes >= bytes && g_pool[i].bytes <= bytes + bytes / 4 + (1u << 20) &&
        (best < 0 || g_pool[i].bytes < g_pool[best].bytes)) best = i;
  if (best < 0) return nullptr;
  void* p = g_pool[best].p; *got = g_pool[best].bytes;
  if (device >= 0 && device < kMaxDevices) g_pool_held[device] -= g_pool[best].bytes;
  g_pool.erase(g_pool.begin() + best);
  return p;
}
// (the caller has made sure no kernel still uses p: ~pw_batch synchronises first)
void pool_give(int device, void* p, size_t bytes) {
  if (!p) return;
  if (device >= 0 && device < kMaxDevices && bytes >= (1u << 20)) {
    size_t held_now;
    { std::lock_guard<std::mutex> lk(g_pool_mutex); held_now = g_pool_held[device]; }
    const size_t cap = pool_room_now(device, held_now);
    std::lock_guard<std::mutex> lk(g_pool_mutex);
    if (g_pool_held[device] + bytes <= cap && g_pool.size() < 64) {
      g_pool.push_back(PoolEntry{p, bytes, device});
      g_pool_held[device] += bytes;
      return;
    }
  }
  (void)hipFree(p);
}
void pool_drop(int device /* < 0: every device */) {
  std::vector<PoolEntry> drop;
  {
    std::lock_guard<std::mutex> lk(g_pool_mutex);
    std::vector<PoolEntry> keep;
    for (auto& e : g_pool) (device < 0 || e.device == device ? drop : keep).push_back(e);
    g_pool.swap(keep);
    for (int d = 0; d < kMaxDevices; d++) if (device < 0 || d == device) g_pool_held[d] = 0;
  }
  int cur = 0;
  (void)hipGetDevice(&cur);
  for (auto& d : drop) { (void)hipSetDevice(d.device); (void)hipFree(d.p); }
  (void)hipSetDevice(cur);
}
hipError_t pool_alloc(int device, void** p, size_t bytes, size_t* got) {
  // size classes, 8 per octave: consecutive batches of similar size then reuse each other's buffers
  if (bytes >= (1u << 20)) {
    int lg = 0; while ((bytes >> (lg + 1)) != 0) lg++;
    const size_t step = (size_t)1 << (lg - 3);
    bytes = (bytes + step - 1) / step * step;
  }
  *p = pool_take(device, bytes, got);
  if (*p) return hipSuccess;
  *got = bytes;
  hipError_t e = hipMalloc(p, bytes);
  if (e != hipSuccess) {           // out of memory with buffers parked in the pool: release them and retry once
    (void)hipGetLastError();
    pool_drop(device);
    e = hipMalloc(p, bytes);
  }
  return e;
}

// A buffer of the pool: taken through pool_alloc, handed back by pool_give when its owner goes (or when it is allocated
// again).  The owner makes sure that no kernel still uses it by then.
template <typename T>
struct PoolBuffer {
  int device = -1;
  T* p = nullptr;
  size_t bytes = 0;
  PoolBuffer() = default;
  PoolBuffer(PoolBuffer&& o) noexcept : device(o.device), p(std::exchange(o.p, nullptr)), bytes(std::exchange(o.bytes, 0)) {}
  PoolBuffer& operator=(PoolBuffer&& o) noexcept { std::swap(device, o.device); std::swap(p, o.p); std::swap(bytes, o.bytes); return *this; }
  ~PoolBuffer() { pool_give(device, p, bytes); }
  hipError_t alloc(int dev, size_t want) {
    pool_give(device, std::exchange(p, nullptr), bytes);
    device = dev;
    void* q = nullptr;
    const hipError_t e = pool_alloc(dev, &q, want, &bytes);
    if (e == hipSuccess) p = (T*)q;
    return e;
  }
};

thread_local std::string g_err;

int fail(const std::string& msg) { g_err = msg; return -1; }

#define HIP_TRY(expr) PW_HIP_CHECK(fail, expr)

struct BkClass {
  int bk = 0;
  int nw = 1;                   // wavefronts per pair (> 1: multi-wavefront kernel for wide bands)
  std::vector<int32_t> order;   // pair indices, largest table first
  DeviceArray<int32_t> d_order; // [order.size()]
};

}  // namespace

struct pw_batch {
  int device = 0;
  int32_t n = 0;
  uint32_t flags = 0;
  int mode = 0, type = 0, L = 0;
  double go = 0, ge = 0;
  std::vector<double> subst;
  bool simple = false, use_f64 = false;
  double plan_ms = 0;
  pw::PlanKnobs knobs;                   // the planner's environment knobs, read by batch_plan
  int scale_shift = 0;                   // dyadic scaling: every score is held times 2^scale_shift by the integer kernels
  double score_mul = 1.0;                // 2^-scale_shift: what the kernels multiply a reported score with
  int variant = 0, brule = 0, endrule = 0, gosign = 0;
  std::vector<pw_pair> pairs;
  std::vector<pw::Plan> plans;
  std::vector<pw::PairDesc> descs;
  std::vector<BkClass> classes;
  std::vector<pw::WaveDesc> waves;      // lane-packed kernel: one per wavefront
  std::vector<int32_t> strips;          // standard-mode pairs wider than a workgroup: the strip pipeline (K2c, pw_strip.h)
  std::vector<uint32_t> strip_ctl_init;                   // per strip pair: the 16 dwords its control block starts from
  PoolBuffer<uint64_t> d_fifo; size_t fifo_bytes = 0;   // FIFO rows of the largest strip pair (pairs run one after another)
  DeviceArray<pw::StripBest> d_sbest;    // [max strips]
  DeviceArray<uint32_t> d_ctl;           // [strip pairs][16]: control blocks (work queue head, abort flag, ..)
  std::vector<int32_t> tiled;           // pairs that go through the time-blocked tiled kernel (K2b)
  DeviceBuffer d_state[2];               // their per-diagonal state in the score type (int32_t or double), double buffered (shared: pairs run one after another)
  int32_t st_pitch = 0;
  int packed_seg = 0, packed_rule = 0, packed_nw = 1;     // packed_nw: wavefronts per pair (K2a with the 16-bit body)
  int packed_mat = 0;                                     // the packed kernel reads a substitution matrix (WaveFill16<.., MAT>)
  int ramp_free = 0;                                      // ... and runs its start and end blocks on the steady body (pw_plan.h, ramp_free)
  int stamp_group = 1;                                    // ... and stamps the running best once per this many blocks (pw_plan.h, stamp_group)
  int lds_feed = 0;                                       // ... and reads its letters from LDS (pw_plan.h, lds_feed)
  int pair_keys = 0;                                      // ... and keeps one running-best key per two cells (pw_plan.h, pair_keys)
  int lds_exchange = 0;                                   // ... and hands its lane-crossing offers on through LDS (pw_plan.h, lds_exchange)
  DeviceArray<pw::WaveDesc> d_waves;     // [waves.size()]
  int64_t cells = 0, alg_bytes = 0;
  // device (~pw_batch releases all of it)
  bool on_device = false;                // batch_alloc ran: a batch that only planned makes no HIP call when it goes
  PoolBuffer<uint8_t> arena; uint64_t arena_bytes = 0;
  uint8_t* d_arena = nullptr;            // the arena the kernels read: `arena`, or the caller's (pw_batch_share_arena)
  bool arena_shared = false;             // PW_FLAG_SHARED_ARENA: the batch owns no arena
  PoolBuffer<pw::PairDesc> d_pairs;
  PoolBuffer<uint32_t> d_masks; uint64_t mask_words = 0;
  DeviceBuffer d_hdump; uint64_t h_elems = 0;   // int32_t or double score planes (PW_FLAG_DUMP_SCORES)
  PoolBuffer<pw::Result> d_results;
  PoolBuffer<uint8_t> d_tx; uint64_t tx_bytes = 0;
  DeviceBuffer d_subst;                  // int32_t or double [L][L]
  DeviceArray<int32_t> d_ends;           // [n][2]: pw_batch_traceback_from
  PoolBuffer<uint8_t> d_txpacked;        // pw_batch_pack_transcripts: the ops back to back
  DeviceArray<uint64_t> d_txoffsets;     // [n + 1]
  PoolBuffer<pw_tx_summary> d_summaries; // pw_batch_summarize: allocated on its first call
  uint64_t trace_seq = 0, summary_seq = 0;   // tracebacks so far / the one the summaries were taken after
  DeviceArray<uint64_t> d_cigoffsets;    // pw_batch_cigars: [n + 1], allocated on its first call
  PoolBuffer<uint32_t> d_cigruns;        // ... and the runs; grows to the largest total seen
  uint64_t cigar_room = 0, cigar_total = 0, cigar_seq = 0;   // runs d_cigruns holds / the last total / the traceback it describes
  int cigar_form = -1;
  hipStream_t cigar_stream = nullptr;    // the stream of the last pw_batch_cigars
  DeviceArray<int64_t> d_col0;           // pw_batch_pileup_add: [n] frame starts, allocated on its first call with a col0
  std::vector<int64_t> h_col0;           // ... and the host copy they are uploaded from
  DeviceArray<int64_t> d_sides_col0;     // pw_batch_pileup_add_sides: [2][n] frame starts of the origin and the mutant side
  DeviceArray<uint8_t> d_reversed;       // ... [n] reversal bytes
  std::vector<int64_t> h_sides_col0;     // ... and the host copies they are uploaded from
  std::vector<uint8_t> h_reversed;
  DeviceEvent ev_fill0, ev_fill1, ev_tr0, ev_tr1;
  bool fill_timed = false, trace_timed = false;
  // scores as the caller gave them (batch_plan may scale b->subst / go / ge by a power of two)
  std::vector<double> subst_in; double go_in = 0, ge_in = 0;
  // Strip pairs whose pipeline gave up waiting (PW_ST_BADPATH with no end cell) are solved again by a batch of one with the
  // strips disabled (repair_strip_pair); the replacement lives as long as the batch and serves every later traceback
  std::vector<std::pair<int32_t, std::unique_ptr<pw_batch>>> repaired;
  // one event per stream the batch was launched on, re-recorded behind every launch sequence: destroying the batch waits
  // for exactly these (not for the device: other batches' streams keep running)
  std::vector<std::pair<hipStream_t, DeviceEvent>> done_events;
  bool traced = false, traced_from = false;          // what the last traceback call was (a repaired pair repeats it)
  std::vector<int32_t> last_ends;
  ~pw_batch();
};

// The members free themselves when the body is done; the body makes that safe.  The pool's buffers are parked for the
// next batch, not freed (freeing would synchronise by itself), and pool_give reads the free memory of the current device:
// the batch's device is selected, and nothing that was launched for THIS batch may still read or write them -- the events
// recorded behind its launches, stream by stream (a device-wide synchronisation would stall every other batch in flight).
pw_batch::~pw_batch() {
  repaired.clear();
  if (!on_device) return;
  (void)hipSetDevice(device);
  for (auto& se : done_events) (void)hipEventSynchronize(se.second.e);
}

namespace {

// The planner's environment knobs (pw_plan.h, PlanKnobs), read once per batch.
pw::PlanKnobs plan_knobs() {
  auto on = [](const char* name) { return env_int(name, 0) != 0; };
  pw::PlanKnobs k;
  k.no_dyadic = on("PWLIB_NO_DYADIC");
  k.latency_mode = env_int("PWLIB_LATENCY_MODE", -1);
  k.no_packed_mat = on("PWLIB_NO_PACKED_MAT");
  k.no_packed_anchored = on("PWLIB_NO_PACKED_ANCHORED");
  k.no_packed_overlap = on("PWLIB_NO_PACKED_OVERLAP");
  k.no_packed_mw = on("PWLIB_NO_PACKED_MW");
  k.no_strip = on("PWLIB_NO_STRIP");
  k.no_small_strip = on("PWLIB_NO_SMALL_STRIP");
  k.strip_no_byte_rows = on("PWLIB_STRIP_NO_BYTE_ROWS");
  k.no_small_tiled = on("PWLIB_NO_SMALL_TILED");
  k.mw_wide_lanes = on("PWLIB_MW_WIDE_LANES");
  k.simple_as_matrix = env_int("PWLIB_SIMPLE_AS_MATRIX", -1);
  k.no_scaled16 = on("PWLIB_NO_SCALED16");
  k.ramp_blocks = on("PWLIB_RAMP_BLOCKS");
  k.stamp_group1 = env_int("PWLIB_STAMP_GROUP", 0) == 1;
  k.no_lds_feed = env_int("PWLIB_LDS_FEED", 1) == 0;
  k.no_pair_keys = env_int("PWLIB_PAIR_KEYS", 1) == 0;
  k.no_lds_exchange = env_int("PWLIB_LDS_EXCHANGE", 1) == 0;
  const char* bk = getenv("PWLIB_PACKED_BK");
  if (bk && *bk) { k.packed_bk_forced = true; k.packed_bk = atoi(bk); k.packed_bk_seg = strchr(bk, 's') != nullptr; }
  return k;
}

// The arguments of pw_batch_create / pw_plan_only, checked in this order, copied into b.  A NULL score matrix is one of
// pw_plan_only's bad arguments; pw_batch_create reports it with the alphabet.
int batch_inputs(pw_batch* b, bool plan_only, const pw_scoring* sc, int32_t n_pairs, const pw_pair* pairs, uint64_t arena_bytes,
                 uint32_t flags) {
  if (!sc || n_pairs < 0 || (n_pairs > 0 && !pairs) || (plan_only && !sc->subst))
    return fail(plan_only ? "pw_plan_only: bad arguments" : "pw_batch_create: bad arguments");
  if (sc->mode != pw::STD_MODE && sc->mode != pw::BANDED_MODE) return fail("unknown alignment mode");
  if (sc->type < 0 || sc->type > (sc->mode == pw::STD_MODE ? 6 : 2)) return fail("unknown alignment type");
  if (sc->alphabet_len < 1 || sc->alphabet_len > 256 || !sc->subst) return fail("alphabet_len must be 1..256 with a score matrix");
  b->n = n_pairs; b->flags = flags;
  b->mode = sc->mode; b->type = sc->type; b->L = sc->alphabet_len; b->go = sc->go; b->ge = sc->ge;
  b->subst.assign(sc->subst, sc->subst + (size_t)b->L * b->L);
  b->subst_in = b->subst; b->go_in = b->go; b->ge_in = b->ge;
  b->pairs.assign(pairs, pairs + n_pairs);
  b->arena_bytes = arena_bytes;
  return 0;
}

// The packed 16-bit body: consecutive (similar length) pairs share a wavefront (p16.seg), one WaveDesc per wavefront
void plan_waves(pw_batch* b, const pw::PackedLayout& p16) {
  const int ppw = p16.seg ? 64 / p16.nl : 1;
  BkClass& c = b->classes[0];
  for (size_t i = 0; i < c.order.size(); i += ppw) {
    pw::WaveDesc wd;
    memset(&wd, 0, sizeof wd);
    wd.first = (int32_t)i; wd.count = (int32_t)std::min<size_t>(ppw, c.order.size() - i);
    wd.nl = (p16.seg || p16.nw > 1) ? p16.nl : 64;      // lanes per pair in the wave / workgroup (the mask plane rows stay p16.nl wide)
    wd.nblocks = 0; wd.steady_b0 = 0; wd.steady_b1 = 0x7fffffff;
    for (int q = 0; q < wd.count; q++) {
      const pw::PairDesc& d = b->descs[c.order[i + q]];
      wd.nblocks = std::max(wd.nblocks, d.nblocks);
      wd.steady_b0 = std::max(wd.steady_b0, d.steady_b0);
      wd.steady_b1 = std::min(wd.steady_b1, d.steady_b1);
    }
    if (wd.steady_b1 < wd.steady_b0) wd.steady_b1 = wd.steady_b0;
    b->waves.push_back(wd);
  }
}

// Planning: host arithmetic only (dptable_init per pair, score type, kernel variant and geometry, launch classes) -- no
// device call, so pw_plan_only can run it anywhere.  batch_alloc then creates the device buffers it sized.  The rules that
// choose the kernels are pure functions shared with the CPU lane emulator (pw_plan.h); this function gathers their inputs.
int batch_plan(pw_batch* b) {
  const double t_build0 = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
  // ---- scoring analysis (PW_FLAG_FORCE_F64 and PWLIB_NO_DYADIC=1 keep fractional scores as given) ----
  const int L = b->L;
  const pw::PlanKnobs& kn = b->knobs = plan_knobs();
  const pw::ScoreSummary sc = pw::summarise_scores(L, b->subst.data(), b->go, b->ge, !(b->flags & PW_FLAG_FORCE_F64) && !kn.no_dyadic);
  if (!sc.finite) return fail("substitution scores must be finite");
  b->simple = sc.simple;
  if (sc.scale_shift) {
    const double f = (double)(1 << sc.scale_shift);
    for (auto& v : b->subst) v *= f;
    b->go *= f; b->ge *= f;
    b->scale_shift = sc.scale_shift; b->score_mul = 1.0 / f;
  }
  pw::plan_rules(b->mode, b->type, &b->brule, &b->endrule);
  b->gosign = b->go < 0 ? -1 : (b->go > 0 ? 1 : 0);
  // ---- pass 1: per-pair plans (dptable_init arithmetic) and batch statistics ----
  int64_t maxspan = 0, maxmin = 0; int maxnd = 0; int64_t sumnd = 0; int nsolv = 0;
  // a batch of few pairs: kernels that take the pairs one after another (strips, tiles: each pair gets the whole chip)
  // against kernels that take all of them at once -- estimated times of both from the one table of pw_model.h
  const pw::PlanModel& model = pw::kPlanModel;
  pw::BatchEstimates est;
  int min_x = 0x7fffffff;
  b->plans.resize(b->n); b->descs.resize(b->n);
  uint64_t mask_words = 0, h_elems = 0, tx_bytes = 0;
  for (int32_t k = 0; k < b->n; k++) {
    const pw_pair& p = b->pairs[k];
    if (p.origin_len < 0 || p.mutant_len < 0) return fail("negative sequence length");
    if (p.origin_off + (uint64_t)p.origin_len > b->arena_bytes || p.mutant_off + (uint64_t)p.mutant_len > b->arena_bytes)
      return fail("pair frame outside the arena");
    if ((int64_t)p.origin_len + p.mutant_len > (1 << 30)) return fail("sequences too long");
    if ((p.origin_off & 3) || (p.mutant_off & 3)) return fail("frames must start on a 4-byte boundary of the arena");
    pw::Plan pl = pw::plan_problem(b->mode, b->type, p.origin_len, p.mutant_len, p.dmin, p.dmax);
    b->plans[k] = pl;
    pw::PairDesc d;
    memset(&d, 0, sizeof d);
    d.o_off = p.origin_off; d.m_off = p.mutant_off;
    d.X = p.origin_len; d.Y = p.mutant_len;
    d.solvable = (pl.rc == 0 && pl.ndiag > 0) ? 1 : 0;
    d.tx_off = tx_bytes;
    d.tx_cap = p.origin_len + p.mutant_len + 1;
    tx_bytes += ((uint64_t)d.tx_cap + 15) / 16 * 16;
    if (d.solvable) {
      d.dmin = pl.dmin; d.ndiag = pl.ndiag; d.s0 = pl.s0; d.nblocks = pl.nblocks;
      d.steady_b0 = pl.steady_b0; d.steady_b1 = pl.steady_b1;
      d.h_pitch = std::min(p.origin_len, p.mutant_len) + 1;
      b->cells += pl.cells;
      b->alg_bytes += pl.cells / 2 + p.origin_len + p.mutant_len + 32;
      maxspan = std::max<int64_t>(maxspan, (int64_t)p.origin_len + p.mutant_len + 2);
      maxmin = std::max<int64_t>(maxmin, std::min(p.origin_len, p.mutant_len));
      maxnd = std::max(maxnd, pl.ndiag); sumnd += pl.ndiag; nsolv++;
      est.add_pair(model, (double)pl.nblocks * 16.0 /* anti-diagonals of the (banded) table */, pl.ndiag);
      min_x = std::min(min_x, (int)p.origin_len);
      if (b->mode == pw::STD_MODE) est.add_std_pair(model, p.origin_len, p.mutant_len, pl.ndiag);
    }
    b->descs[k] = d;
  }
  // the reference's -INT_MAX floor (pw_plan.h, reaches_reference_floor): refused, not silently diverged from
  {
    const double f = (double)(1 << sc.scale_shift);            // (b->go, b->ge, sc.smin: times 2^scale_shift)
    const double gstep = pw::floor_gap_step(b->go, b->ge) / f, smin = sc.smin / f;
    for (int32_t k = 0; k < b->n; k++) {
      const pw::PairDesc& d = b->descs[k];
      if (d.solvable && pw::reaches_reference_floor(b->brule, d.ndiag == 1 && b->mode == pw::BANDED_MODE, gstep, smin,
                                                    (int64_t)d.X + d.Y + 2))
        return fail("scores too low for this alignment type: (X + Y + 2) * (the most a gap step, or on a one-diagonal band a "
                    "substitution, can lower a score) must stay below INT_MAX, where the reference floors gap candidates and "
                    "end cells at -INT_MAX (not reproduced)");
    }
  }
  // ---- score type and kernel variant ----
  // int32 is exact iff every score is an integer and no partial sum can leave +-2^27 (pw_wave.h)
  b->use_f64 = (b->flags & PW_FLAG_FORCE_F64) || !sc.integral || (double)maxspan * sc.maxabs >= (double)(1 << 27);
  const bool bany = b->brule == pw::BRULE_ANY;
  const bool track = b->endrule == pw::END_STD_LOCAL || b->endrule == pw::END_BANDED_LOCAL;
  // A substitution matrix needs no kernel of its own: the wavefront kernels read every substitution score from a table in
  // LDS (pw_wave.h, TAB), the packed kernels take small integer matrices as rows of bytes (pw_plan.h).  The generic kernel is
  // left with what is decided at run time: go > 0, the score-plane dump, and alphabets beyond the LDS copy (32 letters).
  if ((b->flags & (PW_FLAG_FORCE_GENERIC | PW_FLAG_DUMP_SCORES)) || b->go > 0 || L > 32) b->variant = pw::VAR_GENERIC;
  else if (bany) b->variant = pw::VAR_FAST_ANY_TRACK;
  else if (track) b->variant = pw::VAR_FAST_TRACK;
  else b->variant = pw::VAR_FAST;
  // latency mode: with at most 256 pairs the batch is a few hundred wavefronts on a 1024-SIMD chip, so the time is
  // the length of one pair's dependency chain, not throughput (PWLIB_LATENCY_MODE=0 / 1 overrides)
  const bool latency_mode = kn.latency_mode >= 0 ? kn.latency_mode != 0 : nsolv <= 256;
  // the strip pipeline takes standard-mode pairs with match / mismatch scores or a matrix of signed bytes (pw_strip.h, BROW),
  // scores within +-2^25 (it tracks a row's best as 32 * H + step)
  const bool strips_serve = b->mode == pw::STD_MODE && !kn.no_strip && !(b->flags & (PW_FLAG_DUMP_SCORES | PW_FLAG_NO_STRIP)) &&
                            (double)maxspan * sc.maxabs < (double)(1 << 25) &&
                            (sc.simple || (sc.integral && L <= 4 && sc.smax <= 127 && sc.smin >= -128 && !kn.strip_no_byte_rows));
  // (a few standard-mode pairs: the strips, one pair after another, when they are estimated to finish before the 16-bit body
  //  on several wavefronts per pair would -- tests/micro/few_pairs.py: 2 kb x 2 kb, one pair 0.6 ms on the strips, 1.5 ms
  //  there; four pairs 2.3 ms and 1.6 ms)
  const bool strips_win = latency_mode && strips_serve && min_x >= 127 && !kn.no_small_strip && est.strips_beat_packed_workgroups(model);
  // ---- the packed 16-bit body (pw_wave.h, WaveFill16): admission and lane layout ----
  const int rule = b->variant == pw::VAR_GENERIC ? -1 : pw::packed_rule(b->brule, b->endrule);
  const pw::PackedAdmission adm = pw::admit_packed(rule, sc, L, b->go, b->ge, maxmin, maxnd, maxspan, kn);
  pw::PackedLayout p16;
  if (adm.rule >= 0 && !b->use_f64 && nsolv > 0 && !(b->flags & (PW_FLAG_NO_PACKED16 | PW_FLAG_FORCE_TILED | PW_FLAG_FORCE_STRIP))) {
    // bands wider than one wavefront holds, many pairs (standard-mode tables of 1 .. 8 kb, say): a workgroup per pair
    if (maxnd > 2048) {
      if (maxnd <= 64 * pw::kMaxWavesPerPair * 32 && !kn.no_packed_mw && !strips_win) p16 = pw::packed_workgroup_layout(maxnd);
    } else {
      p16 = pw::packed_lane_layout(maxnd, sumnd, nsolv, latency_mode, strips_win, kn, model);
    }
  }
  if (p16.bk) {
    b->variant = pw::VAR_FAST16;
    b->packed_seg = p16.seg; b->packed_nw = p16.nw;
    b->packed_mat = pw::packed_matrix_form(adm, p16, sc.simple, kn);
    b->packed_rule = adm.x4 && (!b->packed_mat || adm.x4_matrix) ? 3 : adm.rule;   // rule 0, scores below 2048: every score times 4
    b->ramp_free = pw::ramp_free(b->packed_rule, b->packed_mat != 0, b->go, b->ge, sc.smin, kn);
    b->stamp_group = pw::stamp_group(b->packed_rule, b->packed_mat != 0, p16.bk, p16.seg != 0, p16.nw, b->ramp_free != 0, kn);
    b->lds_feed = pw::lds_feed(b->stamp_group, kn) ? 1 : 0;
    b->pair_keys = pw::pair_keys(b->lds_feed != 0, b->subst.data(), L, b->go, b->ge, kn) ? 1 : 0;
    b->lds_exchange = pw::lds_exchange(b->pair_keys != 0, kn) ? 1 : 0;
  }
  // ---- pass 2: kernel geometry per pair (pw_plan.h, pair_layout), mask planes, launch classes ----
  pw::PairRules pr;
  pr.strips = strips_serve && !b->use_f64 && b->variant != pw::VAR_GENERIC && b->variant != pw::VAR_FAST16 &&
              !(b->flags & PW_FLAG_FORCE_TILED);
  pr.all_strips = (b->flags & PW_FLAG_FORCE_STRIP) != 0;
  pr.few_strips = latency_mode && !kn.no_small_strip && est.strips_beat_workgroups(model);
  pr.all_tiled = (b->flags & PW_FLAG_FORCE_TILED) != 0;
  pr.few_tiled = latency_mode && !(b->flags & PW_FLAG_DUMP_SCORES) && !kn.no_small_tiled && est.tiles_beat_workgroups(model, b->use_f64);
  pr.latency_mode = latency_mode; pr.f64 = b->use_f64; pr.wide_lanes = kn.mw_wide_lanes;
  pr.packed_bk = p16.bk; pr.packed_nl = p16.nl;
  for (int32_t k = 0; k < b->n; k++) {
    pw::PairDesc& d = b->descs[k];
    if (!d.solvable) continue;
    const pw::PairLayout lay = pw::pair_layout(d.ndiag, d.X, pr);
    d.bk = lay.bk; d.nl = lay.nl;
    d.mask_off = mask_words;
    d.h_off = h_elems;
    if (lay.kind == pw::PAIR_STRIPS) {
      // rows in strips of 64, a pipeline of wavefronts
      const int nstrips = pw::strip_count(d.X), nkq = pw::strip_nkq(d.Y);
      d.layout = 1;
      mask_words += (uint64_t)nstrips * nkq * 64 * 4;
      b->strips.push_back(k);
      b->fifo_bytes = std::max<size_t>(b->fifo_bytes, (size_t)nstrips * (size_t)pw::strip_fifo_pitch(d.Y) * sizeof(uint64_t));
      continue;
    }
    if (lay.kind == pw::PAIR_TILED && (b->flags & PW_FLAG_DUMP_SCORES)) return fail("the score plane is not available for tiled (very wide) tables");
    mask_words += (uint64_t)(d.nblocks + 1) * lay.nl * lay.bk;   // + one spare row: the branch-free stores of idle lanes land there
    if (b->flags & PW_FLAG_DUMP_SCORES) h_elems += (uint64_t)d.ndiag * d.h_pitch;
    if (lay.kind == pw::PAIR_TILED) { b->tiled.push_back(k); b->st_pitch = std::max(b->st_pitch, (d.ndiag + 63) / 64 * 64); continue; }
    size_t ci = 0;
    for (; ci < b->classes.size(); ci++) if (b->classes[ci].bk == lay.bk && b->classes[ci].nw == lay.nw) break;
    if (ci == b->classes.size()) { b->classes.emplace_back(); b->classes.back().bk = lay.bk; b->classes.back().nw = lay.nw; }
    b->classes[ci].order.push_back(k);
  }
  for (auto& c : b->classes)
    std::stable_sort(c.order.begin(), c.order.end(), [&](int32_t x, int32_t y) {
      return b->descs[x].nblocks > b->descs[y].nblocks;
    });
  if (b->variant == pw::VAR_FAST16) plan_waves(b, p16);
  b->mask_words = mask_words; b->h_elems = h_elems; b->tx_bytes = tx_bytes;
  b->arena_shared = (b->flags & PW_FLAG_SHARED_ARENA) != 0;
  b->plan_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count() - t_build0;
  return 0;
}

int batch_alloc(pw_batch* b) {
  const int L = b->L;
  const uint64_t mask_words = b->mask_words, h_elems = b->h_elems, tx_bytes = b->tx_bytes;
  // ---- device buffers ----
  const bool tim = env_int("PWLIB_TIMING", 0) != 0;
  auto tnow = []() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
  const double t_plan = tnow();
  const int dev = b->device;
  b->on_device = true;
  HIP_TRY(hipSetDevice(dev));
  if (!b->arena_shared) {
    HIP_TRY(b->arena.alloc(dev, b->arena_bytes + 16));   // kernels read whole dwords: slack past the last frame
    b->d_arena = b->arena.p;
  }
  HIP_TRY(b->d_pairs.alloc(dev, sizeof(pw::PairDesc) * std::max<int32_t>(b->n, 1)));
  HIP_TRY(b->d_masks.alloc(dev, 4 * mask_words + 64));   // slack: the walker reads whole 16-byte groups
  HIP_TRY(b->d_results.alloc(dev, sizeof(pw::Result) * std::max<int32_t>(b->n, 1)));
  HIP_TRY(b->d_tx.alloc(dev, std::max<uint64_t>(tx_bytes, 16)));
  const size_t esz = b->use_f64 ? 8 : 4;
  if (h_elems) HIP_TRY(b->d_hdump.ensure(esz * h_elems));
  HIP_TRY(b->d_subst.ensure(esz * (size_t)L * L));
  if (b->use_f64) {
    HIP_TRY(hipMemcpy(b->d_subst.p, b->subst.data(), 8 * (size_t)L * L, hipMemcpyHostToDevice));
  } else {
    std::vector<int32_t> si((size_t)L * L);
    for (size_t i = 0; i < si.size(); i++) si[i] = (int32_t)b->subst[i];
    HIP_TRY(hipMemcpy(b->d_subst.p, si.data(), 4 * si.size(), hipMemcpyHostToDevice));
  }
  if (b->n) HIP_TRY(hipMemcpy(b->d_pairs.p, b->descs.data(), sizeof(pw::PairDesc) * b->n, hipMemcpyHostToDevice));
  if (!b->strips.empty()) {
    int maxs = 0;
    for (int32_t k : b->strips) maxs = std::max(maxs, pw::strip_count(b->descs[k].X));
    HIP_TRY(b->d_fifo.alloc(dev, b->fifo_bytes));
    // granules are recognised by their epoch tag: whatever the (possibly recycled) buffer holds must never look like one
    HIP_TRY(hipMemset(b->d_fifo.p, 0, b->fifo_bytes));
    HIP_TRY(b->d_sbest.ensure((size_t)maxs));
    HIP_TRY(b->d_ctl.ensure(b->strips.size() * 16));
  }
  if (!b->tiled.empty())
    for (DeviceBuffer& st : b->d_state) HIP_TRY(st.ensure((size_t)5 * b->st_pitch * sizeof(double)));   // (room for either score type)
  if (!b->waves.empty() && upload(fail, b->d_waves, b->waves.data(), b->waves.size()) != 0) return -1;
  for (auto& c : b->classes)
    if (upload(fail, c.d_order, c.order.data(), c.order.size()) != 0) return -1;
  {  // records of pairs no kernel will touch
    std::vector<pw::Result> init(std::max<int32_t>(b->n, 1));
    for (auto& r : init) { r.score = 0; r.opt_i = r.opt_j = -1; r.origin_idx = r.mutant_idx = 0; r.tx_len = 0; r.status = 0; }
    HIP_TRY(hipMemcpy(b->d_results.p, init.data(), sizeof(pw::Result) * init.size(), hipMemcpyHostToDevice));
  }
  if (b->flags & PW_FLAG_PROFILE)
    for (DeviceEvent* ev : {&b->ev_fill0, &b->ev_fill1, &b->ev_tr0, &b->ev_tr1}) HIP_TRY(ev->create());
  if (tim && b->n > 1000) fprintf(stderr, "pwlib timing: batch of %d pairs: planning %.1f ms, device buffers + descriptors %.1f ms\n", b->n, b->plan_ms, tnow() - t_plan);
  return 0;
}

// Records "everything launched for this batch on `st` so far" (see pw_batch::done_events).
int mark_done(pw_batch* b, hipStream_t st) {
  for (auto& se : b->done_events)
    if (se.first == st) { HIP_TRY(hipEventRecord(se.second.e, st)); return 0; }
  DeviceEvent ev;
  HIP_TRY(hipEventCreateWithFlags(&ev.e, hipEventDisableTiming));
  b->done_events.emplace_back(st, std::move(ev));
  HIP_TRY(hipEventRecord(b->done_events.back().second.e, st));
  return 0;
}

std::atomic<uint32_t> g_strip_epoch{1};

// XCC ids present on a device (the strip pipeline keeps runs of consecutive strips on one XCD): counted once per device
// by a census kernel.  xcc_queue[id] = queue index or -1; returns the number of queues (0 on error).
int xcc_queues(int device, int32_t* xcc_queue) {
  static std::mutex mu;
  static int cached_n[kMaxDevices] = {0};
  static int32_t cached_map[kMaxDevices][8];
  std::lock_guard<std::mutex> lk(mu);
  if (device < 0 || device >= kMaxDevices) return 0;
  if (cached_n[device] == 0) {
    DeviceArray<uint32_t> d; uint32_t h[8] = {0};
    if (d.ensure(8) != hipSuccess || hipMemset(d.p, 0, sizeof h) != hipSuccess ||
        pw::launch_xcc_census(d.p, nullptr) != hipSuccess || hipMemcpy(h, d.p, sizeof h, hipMemcpyDeviceToHost) != hipSuccess)
      return 0;
    int n = 0;
    for (int i = 0; i < 8; i++) cached_map[device][i] = h[i] ? n++ : -1;
    cached_n[device] = n;
  }
  memcpy(xcc_queue, cached_map[device], sizeof cached_map[device]);
  return cached_n[device];
}

// The strip kernel's byte rows (pw_strip.h, BROW): at most 4 letters, every score an integer that fits a signed byte
bool strip_byte_rows_ok(const pw_batch* b) {
  if (b->L > 4 || b->knobs.strip_no_byte_rows) return false;
  for (double v : b->subst) if (v != std::floor(v) || v < -128 || v > 127) return false;
  return true;
}

// K2c: the strip pairs of a batch, one after another (each one fills the chip by itself)
int launch_strip_fills(pw_batch* b, hipStream_t st) {
  static const int workers = std::max(1, env_int("PWLIB_STRIP_WAVES", 1024));
  static const int lds_kb = std::max(0, env_int("PWLIB_STRIP_LDS_KB", 0));
  size_t q = 0;
  if (b->strip_ctl_init.size() != 16 * b->strips.size()) b->strip_ctl_init.assign(16 * b->strips.size(), 0u);
  for (int32_t k : b->strips) {
    const pw::PairDesc& d = b->descs[k];
    pw::StripParams a;
    memset(&a, 0, sizeof a);
    a.arena = b->d_arena; a.o_off = d.o_off; a.m_off = d.m_off;
    a.fifo = b->d_fifo.p; a.masks = b->d_masks.p + d.mask_off; a.sbest = b->d_sbest.p;
    a.ctl = b->d_ctl.p + 16 * q++;
    a.result = b->d_results.p + k;
    a.X = d.X; a.Y = d.Y;
    a.nstrips = pw::strip_count(d.X); a.nkq = pw::strip_nkq(d.Y);
    a.fifo_pitch = pw::strip_fifo_pitch(d.Y);
    uint32_t e = g_strip_epoch.fetch_add(1) & 0xffffffu;          // 24 bits: the tag's other 8 are the column's low bits
    if (e == 0) e = g_strip_epoch.fetch_add(1) & 0xffffffu;
    a.epoch = e;
    a.brule = b->brule; a.endrule = b->endrule;
    a.match = (int32_t)b->subst[0]; a.mismatch = (int32_t)(b->L > 1 ? b->subst[1] : b->subst[0]);
    a.go = (int32_t)b->go; a.ge = (int32_t)b->ge;
    a.score_mul = b->score_mul;
    a.spin_limit = env_int("PWLIB_STRIP_SPIN_LIMIT", 1 << 21);
    a.nq = xcc_queues(b->device, a.xcc_queue);
    if (a.nq <= 0) return fail("could not determine the XCDs of the device");
    a.run_len = std::max(1, env_int("PWLIB_STRIP_RUN", std::max(1, workers / a.nq)));
    const bool track = b->endrule != pw::END_CORNER;
    // tuning aid: PWLIB_STRIP_TRACE=<file> dumps per-strip clock stamps (100 MHz; [8 + i]: shader-clock counts at the same points) of the first strip pair: dequeue, set-up
    // done, first granules seen, steps 64 / 96 reached, end; [7] = XCC id | workgroup << 8
    const char* trace = getenv("PWLIB_STRIP_TRACE");
    DeviceArray<uint64_t> stamps;                                  // 16 per strip
    if (trace && *trace && q == 1) {
      HIP_TRY(stamps.ensure((size_t)a.nstrips * 16));
      HIP_TRY(hipMemset(stamps.p, 0, stamps.bytes((size_t)a.nstrips * 16)));
      a.stamps = stamps.p;
    }
    const bool byte_rows = strip_byte_rows_ok(b);
    if (!byte_rows && !b->simple) return fail("internal: a substitution matrix on the strips needs their byte rows");
    // (the 16 dwords the control block starts from: zeros and, behind them, the byte rows; kept in the batch until it dies)
    uint32_t* ci = b->strip_ctl_init.data() + 16 * (q - 1);
    uint32_t rows[4] = {0u, 0u, 0u, 0u};
    if (byte_rows)
      for (int o = 0; o < 4; o++)
        for (int m = 0; m < 4; m++)
          if (o < b->L && m < b->L) rows[o] |= ((uint32_t)(int32_t)b->subst[(size_t)o * b->L + m] & 0xffu) << (8 * m);
    // (written once per batch in effect: every solve stores the same values, also while an earlier copy may still be reading them)
    for (int z = 0; z < 16; z++) ci[z] = (z >= pw::kStripRows && z < pw::kStripRows + 4) ? rows[z - pw::kStripRows] : 0u;
    HIP_TRY(pw::launch_strip_fill(a, track, byte_rows, ci, workers, lds_kb << 10, st));
    if (stamps.p) {
      std::vector<uint64_t> h((size_t)a.nstrips * 16);
      HIP_TRY(hipStreamSynchronize(st));
      HIP_TRY(hipMemcpy(h.data(), stamps.p, stamps.bytes(h.size()), hipMemcpyDeviceToHost));
      if (FILE* f = fopen(trace, "wb")) { fwrite(h.data(), 8, h.size(), f); fclose(f); }
    }
  }
  return 0;
}

// The fields every fill kernel reads
template <typename T>
pw::FillParams<T> fill_params(const pw_batch* b) {
  pw::FillParams<T> a;
  memset(&a, 0, sizeof a);
  a.pairs = b->d_pairs.p; a.arena = b->d_arena; a.masks = b->d_masks.p; a.results = b->d_results.p;
  a.npairs = b->n; a.L = b->L; a.brule = b->brule; a.endrule = b->endrule;
  a.banded = b->mode == pw::BANDED_MODE;
  a.match = (T)b->subst[0]; a.mismatch = (T)(b->L > 1 ? b->subst[1] : b->subst[0]);
  a.go = (T)b->go; a.ge = (T)b->ge;
  a.score_mul = b->score_mul;
  return a;
}

template <typename T>
int launch_all_fills(pw_batch* b, hipStream_t st) {
  pw::FillParams<T> a = fill_params<T>(b);
  a.hdump = b->d_hdump.as<T>(); a.subst = b->d_subst.as<const T>();
  for (auto& c : b->classes) {
    a.order = c.d_order.p;
    if (c.nw > 1) HIP_TRY(pw::launch_fill_mw(a, b->variant, c.bk, c.nw, (int)c.order.size(), st));
    else HIP_TRY(pw::launch_fill(a, b->variant, c.bk, (int)c.order.size(), st));
  }
  // K2b: tiled pairs, one after another; per pair one launch per time block, then the end-cell search
  a.order = nullptr;
  a.st_pitch = b->st_pitch;
  for (int32_t k : b->tiled) {
    const pw::PairDesc& d = b->descs[k];
    const int ntiles = (d.nl + pw::kTileCentralLanes - 1) / pw::kTileCentralLanes;
    int cur = 0;
    for (int tb = 0; tb < d.nblocks; tb += pw::kTileBlocks) {
      a.tile_b0 = tb; a.tile_nb = std::min(pw::kTileBlocks, d.nblocks - tb);
      a.st_in = b->d_state[cur].as<const T>(); a.st_out = b->d_state[cur ^ 1].as<T>();
      HIP_TRY(pw::launch_tile(a, b->variant, (int)k, ntiles, st));
      cur ^= 1;
    }
    a.st_in = b->d_state[cur].as<const T>();
    HIP_TRY(pw::launch_tile_finish(a, (int)k, st));
  }
  return 0;
}

int launch_packed_fill(pw_batch* b, hipStream_t st) {
  pw::FillParams<int32_t> a = fill_params<int32_t>(b);
  a.order = b->classes[0].d_order.p; a.waves = b->d_waves.p;
  if (b->packed_mat) pw::packed_matrix_rows(b->subst.data(), b->L, b->packed_rule == 3, a.mat_rows, &a.mat_bias);
  a.ramp_free = b->ramp_free;
  if (b->packed_nw > 1) HIP_TRY(pw::launch_fill16_mw(a, b->classes[0].bk, b->packed_rule, b->packed_mat, b->packed_nw, (int)b->waves.size(), st));
  else if (b->lds_exchange) HIP_TRY(pw::launch_fill16x(a, (int)b->waves.size(), st));
  else if (b->pair_keys) HIP_TRY(pw::launch_fill16p(a, (int)b->waves.size(), st));
  else if (b->lds_feed) HIP_TRY(pw::launch_fill16l(a, (int)b->waves.size(), st));
  else if (b->stamp_group == 4) HIP_TRY(pw::launch_fill16g(a, (int)b->waves.size(), st));
  else HIP_TRY(pw::launch_fill16(a, b->classes[0].bk, b->packed_seg, b->packed_rule, b->packed_mat, (int)b->waves.size(), st));
  return 0;
}

}  // namespace

extern "C" {

const char* pw_last_error(void) { return g_err.c_str(); }

void pw_pool_trim(void) { pool_drop(-1); }

int pw_device_memory(int device, uint64_t* free_bytes, uint64_t* total_bytes) {
  size_t fr = 0, tot = 0;
  HIP_TRY(hipSetDevice(device));
  HIP_TRY(hipMemGetInfo(&fr, &tot));
  if (free_bytes) *free_bytes = fr;
  if (total_bytes) *total_bytes = tot;
  return 0;
}

int pw_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

pw_batch* pw_batch_create(int device, const pw_scoring* sc, int32_t n_pairs, const pw_pair* pairs,
                          uint64_t arena_bytes, uint32_t flags) {
  std::unique_ptr<pw_batch> b(new pw_batch());
  b->device = device;
  if (batch_inputs(b.get(), false, sc, n_pairs, pairs, arena_bytes, flags) != 0 || batch_plan(b.get()) != 0 ||
      batch_alloc(b.get()) != 0)
    return nullptr;
  return b.release();
}

void pw_batch_destroy(pw_batch* b) { delete b; }

int pw_plan_only(const pw_scoring* sc, int32_t n_pairs, const pw_pair* pairs, uint64_t arena_bytes, uint32_t flags,
                 char* kernel, int32_t kernel_cap, int32_t* info) {
  pw_batch b;
  b.device = -1;
  if (batch_inputs(&b, true, sc, n_pairs, pairs, arena_bytes, flags) != 0 || batch_plan(&b) != 0) return -1;
  if (kernel && kernel_cap > 0) { strncpy(kernel, pw_batch_kernel_name(&b), (size_t)kernel_cap - 1); kernel[kernel_cap - 1] = 0; }
  if (info) {
    int64_t one = 0, wg = 0;
    for (const auto& c : b.classes) (c.nw > 1 || (b.variant == pw::VAR_FAST16 && b.packed_nw > 1) ? wg : one) += (int64_t)c.order.size();
    info[0] = b.use_f64 ? 1 : 0; info[1] = b.scale_shift; info[2] = (int32_t)one; info[3] = (int32_t)wg;
    info[4] = (int32_t)b.tiled.size(); info[5] = (int32_t)b.strips.size();
    info[6] = b.variant == pw::VAR_FAST16 ? b.packed_rule : -1; info[7] = (b.packed_mat ? 1 : 0) | (b.ramp_free ? 2 : 0) | (b.stamp_group == 4 ? 4 : 0) | (b.lds_feed ? 8 : 0) | (b.pair_keys ? 16 : 0) | (b.lds_exchange ? 32 : 0);
  }
  return 0;
}

int pw_batch_init_rc(const pw_batch* b, int32_t k) { return (k < 0 || k >= b->n) ? -1 : b->plans[k].rc; }

int pw_batch_band(const pw_batch* b, int32_t k, int32_t* dmin, int32_t* dmax, int32_t* num_rows) {
  if (k < 0 || k >= b->n) return -1;
  if (dmin) *dmin = b->plans[k].dmin;
  if (dmax) *dmax = b->plans[k].dmax;
  if (num_rows) *num_rows = b->plans[k].num_rows;
  return b->plans[k].clamped;
}

int64_t pw_batch_pair_cells(const pw_batch* b, int32_t k) { return (k < 0 || k >= b->n) ? -1 : b->plans[k].cells; }
int64_t pw_batch_cells(const pw_batch* b) { return b->cells; }
int64_t pw_batch_algorithmic_bytes(const pw_batch* b) { return b->alg_bytes; }
int pw_batch_score_type(const pw_batch* b) { return b->use_f64 ? 1 : 0; }

const char* pw_batch_kernel_name(const pw_batch* b) {
  static thread_local char name[96];
  int bk = 0, nw = 1; size_t most = 0;
  for (const auto& c : b->classes) if (c.order.size() > most) { most = c.order.size(); bk = c.bk; nw = c.nw; }
  if (b->classes.empty() && b->tiled.empty() && !b->strips.empty()) {
    snprintf(name, sizeof name, "k_fill_strip<%s> x row strips", b->endrule != pw::END_CORNER ? "true" : "false");
    return name;
  }
  if (b->classes.empty() && !b->tiled.empty()) { snprintf(name, sizeof name, "k_fill_tile<%s> x time blocks", b->use_f64 ? "double" : "int"); return name; }
  const char* t = b->use_f64 ? "double" : "int";
  if (nw > 1) { snprintf(name, sizeof name, "k_fill_mw<%s, %d, ...> x %d wavefronts", t, bk, nw); return name; }
  switch (b->variant) {
    case pw::VAR_FAST16:
      if (b->packed_nw > 1) snprintf(name, sizeof name, "k_fill16_mw<%d, %d> x %d wavefronts", bk, b->packed_rule, b->packed_nw);
      else if (b->packed_rule == 3) snprintf(name, sizeof name, "k_fill16<%d, %s> x4", bk, b->packed_seg ? "true" : "false");
      else if (b->packed_rule) snprintf(name, sizeof name, "k_fill16<%d, %s, %d>", bk, b->packed_seg ? "true" : "false", b->packed_rule);
      else snprintf(name, sizeof name, "k_fill16<%d, %s>", bk, b->packed_seg ? "true" : "false");
      if (b->packed_mat) strncat(name, " matrix", sizeof name - strlen(name) - 1);
      break;
    case pw::VAR_FAST_ANY_TRACK: snprintf(name, sizeof name, "k_fill<%s, %d, true, true, false>", t, bk); break;
    case pw::VAR_FAST_TRACK: snprintf(name, sizeof name, "k_fill<%s, %d, false, true, false>", t, bk); break;
    case pw::VAR_FAST: snprintf(name, sizeof name, "k_fill<%s, %d, false, false, false>", t, bk); break;
    default: snprintf(name, sizeof name, "k_fill<%s, %d, false, true, true>", t, bk); break;
  }
  return name;
}

void* pw_arena_upload(int device, const uint8_t* host, uint64_t bytes) {
  void* p = nullptr;
  if (hipSetDevice(device) != hipSuccess || hipMalloc(&p, bytes + 16) != hipSuccess) { (void)hipGetLastError(); fail("pw_arena_upload: allocation failed"); return nullptr; }
  if (hipMemset((uint8_t*)p + bytes, 0, 16) != hipSuccess || (bytes && hipMemcpy(p, host, bytes, hipMemcpyHostToDevice) != hipSuccess)) {
    (void)hipGetLastError(); (void)hipFree(p); fail("pw_arena_upload: copy failed"); return nullptr;
  }
  return p;
}
void pw_arena_free(int device, void* p) { if (p) { (void)hipSetDevice(device); (void)hipFree(p); } }
int pw_batch_share_arena(pw_batch* b, void* dev) {
  if (!b->arena_shared) return fail("pw_batch_share_arena: the batch was not created with PW_FLAG_SHARED_ARENA");
  if (!dev) return fail("pw_batch_share_arena: null arena");
  b->d_arena = (uint8_t*)dev;
  return 0;
}

int pw_batch_upload_arena(pw_batch* b, const uint8_t* host, uint64_t bytes) {
  if (b->arena_shared) return fail("the batch shares a caller-owned arena (PW_FLAG_SHARED_ARENA): nothing to upload");
  if (bytes > b->arena_bytes) return fail("arena upload larger than the arena");
  HIP_TRY(hipSetDevice(b->device));
  if (bytes) HIP_TRY(hipMemcpy(b->d_arena, host, bytes, hipMemcpyHostToDevice));
  return 0;
}

void* pw_batch_arena_device(pw_batch* b) { return b->d_arena; }

void* pw_host_alloc(uint64_t bytes) {
  void* p = nullptr;
  if (hipHostMalloc(&p, bytes ? bytes : 1, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); fail("hipHostMalloc failed"); return nullptr; }
  return p;
}
void pw_host_free(void* p) { if (p) (void)hipHostFree(p); }

int pw_batch_upload_arena_async(pw_batch* b, const uint8_t* host, uint64_t bytes, void* stream) {
  if (b->arena_shared) return fail("the batch shares a caller-owned arena (PW_FLAG_SHARED_ARENA): nothing to upload");
  if (bytes > b->arena_bytes) return fail("arena upload larger than the arena");
  HIP_TRY(hipSetDevice(b->device));
  if (bytes) HIP_TRY(hipMemcpyAsync(b->d_arena, host, bytes, hipMemcpyHostToDevice, (hipStream_t)stream));
  return mark_done(b, (hipStream_t)stream);
}
int pw_batch_results_async(pw_batch* b, pw_result* out, void* stream) {
  HIP_TRY(hipSetDevice(b->device));
  if (b->n) HIP_TRY(hipMemcpyAsync(out, b->d_results.p, sizeof(pw_result) * (size_t)b->n, hipMemcpyDeviceToHost, (hipStream_t)stream));
  return mark_done(b, (hipStream_t)stream);
}
int pw_batch_transcripts_async(pw_batch* b, uint8_t* out, void* stream) {
  HIP_TRY(hipSetDevice(b->device));
  if (b->tx_bytes) HIP_TRY(hipMemcpyAsync(out, b->d_tx.p, b->tx_bytes, hipMemcpyDeviceToHost, (hipStream_t)stream));
  return mark_done(b, (hipStream_t)stream);
}

int pw_batch_solve(pw_batch* b, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  if (b->arena_shared && !b->d_arena) return fail("pw_batch_solve: the batch was created with PW_FLAG_SHARED_ARENA and has no arena yet");
  HIP_TRY(hipSetDevice(b->device));
  b->traced = false; b->traced_from = false;
  if (!b->repaired.empty()) {          // a new solve: the strips get another chance
    HIP_TRY(hipDeviceSynchronize());
    b->repaired.clear();
  }
  if (b->flags & PW_FLAG_PROFILE) HIP_TRY(hipEventRecord(b->ev_fill0.e, st));
  int rc = b->variant == pw::VAR_FAST16 ? launch_packed_fill(b, st)
           : b->use_f64 ? launch_all_fills<double>(b, st) : launch_all_fills<int32_t>(b, st);
  if (rc == 0 && !b->strips.empty()) rc = launch_strip_fills(b, st);
  if (rc != 0) return rc;
  if (b->flags & PW_FLAG_PROFILE) { HIP_TRY(hipEventRecord(b->ev_fill1.e, st)); b->fill_timed = true; }
  return mark_done(b, st);
}

static pw_batch* repaired_sub(pw_batch* b, int32_t k) {
  for (auto& r : b->repaired) if (r.first == k) return r.second.get();
  return nullptr;
}

// The replacement of a repaired strip pair repeats the batch's last traceback call; its record and transcript slot (same
// capacity, ops right-aligned) are copied over the pair's own, device to device, on the same stream.
static int replay_trace(pw_batch* b, int32_t k, pw_batch* sub, hipStream_t st) {
  if (b->traced_from) {
    const int32_t e[2] = {b->last_ends[2 * (size_t)k], b->last_ends[2 * (size_t)k + 1]};
    if (pw_batch_traceback_from(sub, e, st) != 0) return -1;
  } else if (pw_batch_traceback(sub, st) != 0) return -1;
  const pw::PairDesc& d = b->descs[k];
  HIP_TRY(hipMemcpyAsync(b->d_results.p + k, sub->d_results.p, sizeof(pw::Result), hipMemcpyDeviceToDevice, st));
  HIP_TRY(hipMemcpyAsync(b->d_tx.p + d.tx_off, sub->d_tx.p + sub->descs[0].tx_off, (size_t)d.tx_cap, hipMemcpyDeviceToDevice, st));
  return 0;
}

// A strip pair whose pipeline was abandoned (a wavefront waited longer than PWLIB_STRIP_SPIN_LIMIT polls for the strip above
// it: a starved or contended device) is solved once more inside the library, as a batch of one that shares the arena and
// may not use the strips (tiled or workgroup kernels).  Synchronous; called from pw_batch_results.
static int repair_strip_pair(pw_batch* b, int32_t k) {
  pw_scoring sc;
  sc.mode = b->mode; sc.type = b->type; sc.alphabet_len = b->L; sc.subst = b->subst_in.data(); sc.go = b->go_in; sc.ge = b->ge_in;
  const uint32_t keep = b->flags & (PW_FLAG_FORCE_F64 | PW_FLAG_FORCE_GENERIC | PW_FLAG_NO_PACKED16);
  std::unique_ptr<pw_batch> owned(pw_batch_create(b->device, &sc, 1, &b->pairs[k], b->arena_bytes,
                                                  keep | PW_FLAG_SHARED_ARENA | PW_FLAG_NO_STRIP));
  pw_batch* sub = owned.get();
  if (!sub) return -1;
  if (!sub->strips.empty()) return fail("internal: the replacement of a strip pair took the strips again");
  if (pw_batch_share_arena(sub, b->d_arena) != 0 || pw_batch_solve(sub, nullptr) != 0) return -1;
  b->repaired.emplace_back(k, std::move(owned));
  if (b->traced) { b->trace_seq++; if (replay_trace(b, k, sub, nullptr) != 0) return -1; }
  else HIP_TRY(hipMemcpyAsync(b->d_results.p + k, sub->d_results.p, sizeof(pw::Result), hipMemcpyDeviceToDevice, nullptr));
  HIP_TRY(hipStreamSynchronize(nullptr));
  static const bool verbose = env_int("PWLIB_TIMING", 0) != 0;
  if (verbose) fprintf(stderr, "pwlib: strip pipeline of pair %d abandoned; solved again on %s\n", (int)k, pw_batch_kernel_name(sub));
  return 0;
}

static int do_trace(pw_batch* b, const int32_t* d_ends, hipStream_t st) {
  pw::TraceParams p;
  memset(&p, 0, sizeof p);
  p.pairs = b->d_pairs.p; p.arena = b->d_arena; p.masks = b->d_masks.p; p.results = b->d_results.p;
  p.transcripts = b->d_tx.p; p.npairs = b->n; p.gosign = b->gosign;
  p.banded = b->mode == pw::BANDED_MODE; p.ends = d_ends;
  // long transcripts (strip-pipeline pairs) are fixed up by several wavefronts each: ~2000 ops per segment
  if (!b->strips.empty()) {
    int64_t longest = 0;
    for (int32_t k : b->strips) longest = std::max<int64_t>(longest, b->descs[k].tx_cap);
    p.fix_segments = (int32_t)std::min<int64_t>(256, std::max<int64_t>(1, longest / 2048));
  }
  b->trace_seq++;                      // (summaries taken before this traceback are stale: pw_txsum.h)
  if (b->flags & PW_FLAG_PROFILE) HIP_TRY(hipEventRecord(b->ev_tr0.e, st));
  for (int32_t k : b->strips) {        // strip-layout pairs: one wavefront each (before the fix-up pass below)
    if (repaired_sub(b, k)) continue;  // (its mask plane is that of an abandoned fill: the replacement walks its own)
    const pw::PairDesc& d = b->descs[k];
    pw::StripTraceParams sp;
    memset(&sp, 0, sizeof sp);
    sp.masks = b->d_masks.p + d.mask_off; sp.result = b->d_results.p + k; sp.tx = b->d_tx.p + d.tx_off;
    sp.ends = d_ends ? d_ends + 2 * k : nullptr;
    sp.X = d.X; sp.Y = d.Y; sp.nkq = pw::strip_nkq(d.Y); sp.tx_cap = d.tx_cap; sp.gosign = b->gosign;
    HIP_TRY(pw::launch_strip_trace(sp, st));
  }
  HIP_TRY(pw::launch_trace(p, st));
  for (auto& r : b->repaired) if (replay_trace(b, r.first, r.second.get(), st) != 0) return -1;
  if (b->flags & PW_FLAG_PROFILE) { HIP_TRY(hipEventRecord(b->ev_tr1.e, st)); b->trace_timed = true; }
  return mark_done(b, st);
}

int pw_batch_traceback(pw_batch* b, void* stream) {
  HIP_TRY(hipSetDevice(b->device));
  b->traced = true; b->traced_from = false;
  return do_trace(b, nullptr, (hipStream_t)stream);
}

int pw_batch_traceback_from(pw_batch* b, const int32_t* ends_ij, void* stream) {
  HIP_TRY(hipSetDevice(b->device));
  hipStream_t st = (hipStream_t)stream;
  HIP_TRY(b->d_ends.ensure(2 * (size_t)std::max<int32_t>(b->n, 1)));
  // validate on the host: an end cell outside the table would send the walker out of the mask plane
  for (int32_t k = 0; k < b->n; k++) {
    if (!b->descs[k].solvable) continue;
    const int i = ends_ij[2 * k], j = ends_ij[2 * k + 1];
    if (i < 0 && j < 0) continue;
    const pw::Plan& pl = b->plans[k];
    const int X = b->pairs[k].origin_len, Y = b->pairs[k].mutant_len;
    bool ok;
    if (b->mode == pw::STD_MODE) ok = i >= 0 && i <= X && j >= 0 && j <= Y;
    else ok = i >= 0 && i < pl.num_rows && j >= 0 && j < pw::plan_len(X, Y, pl.dmin + i);
    if (!ok) return fail("traceback end cell outside the table");
  }
  // The copy reads the batch's own pageable copy: the caller's array is consumed here, also where it is page-locked (a copy
  // from such memory reads it when the stream gets there).  That the copy below is done with last_ends when it returns --
  // the next call assigns to it again -- is the runtime's rule for pageable sources (hipMemcpyAsync returns once a pageable
  // buffer is staged), at any size; the tests see it at 64 pairs only.
  b->last_ends.assign(ends_ij, ends_ij + 2 * (size_t)b->n);
  HIP_TRY(hipMemcpyAsync(b->d_ends.p, b->last_ends.data(), b->d_ends.bytes(2 * (size_t)b->n), hipMemcpyHostToDevice, st));
  b->traced = true; b->traced_from = true;
  return do_trace(b, b->d_ends.p, st);
}

int pw_batch_sync(pw_batch* b, void* stream) {
  HIP_TRY(hipSetDevice(b->device));
  HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
  return 0;
}

void* pw_batch_results_device(pw_batch* b) { return b->d_results.p; }
void* pw_batch_transcripts_device(pw_batch* b) { return b->d_tx.p; }
uint64_t pw_batch_transcripts_bytes(const pw_batch* b) { return b->tx_bytes; }

int pw_batch_tx_slot(const pw_batch* b, int32_t k, uint64_t* off, int32_t* cap) {
  if (k < 0 || k >= b->n) return -1;
  if (off) *off = b->descs[k].tx_off;
  if (cap) *cap = b->descs[k].tx_cap;
  return 0;
}

int pw_batch_results(pw_batch* b, pw_result* out) {
  HIP_TRY(hipSetDevice(b->device));
  if (b->n) HIP_TRY(hipMemcpy(out, b->d_results.p, sizeof(pw_result) * (size_t)b->n, hipMemcpyDeviceToHost));
  // (the D2H copy above has waited for everything launched on the default stream; callers that launched on another stream
  //  synchronise it first, as for any read of the records)
  for (int32_t k : b->strips)
    if ((out[k].status & PW_ST_BADPATH) && out[k].opt_i < 0 && !repaired_sub(b, k)) {
      if (env_int("PWLIB_NO_STRIP_REPAIR", 0))
        return fail("the strip pipeline of a wide pair was abandoned (a wavefront waited too long for the strip above it)");
      if (repair_strip_pair(b, k) != 0)
        return fail("the strip pipeline of a wide pair was abandoned and solving the pair again without it failed: " + std::string(g_err));
      HIP_TRY(hipMemcpy(out + k, b->d_results.p + k, sizeof(pw_result), hipMemcpyDeviceToHost));
    }
  return 0;
}

int pw_batch_transcripts(pw_batch* b, uint8_t* out) {
  HIP_TRY(hipSetDevice(b->device));
  if (b->tx_bytes) HIP_TRY(hipMemcpy(out, b->d_tx.p, b->tx_bytes, hipMemcpyDeviceToHost));
  return 0;
}

int pw_batch_pack_transcripts(pw_batch* b, void* stream) {
  HIP_TRY(hipSetDevice(b->device));
  if (!b->d_txoffsets.p) {
    HIP_TRY(b->d_txpacked.alloc(b->device, std::max<uint64_t>(b->tx_bytes, 16)));
    HIP_TRY(b->d_txoffsets.ensure((size_t)b->n + 1));
  }
  HIP_TRY(pw::launch_tx_pack(b->d_pairs.p, b->d_results.p, b->d_tx.p, b->n, b->d_txoffsets.p, b->d_txpacked.p,
                             (hipStream_t)stream));
  return mark_done(b, (hipStream_t)stream);
}
void* pw_batch_packed_device(pw_batch* b) { return b->d_txpacked.p; }
void* pw_batch_packed_offsets_device(pw_batch* b) { return b->d_txoffsets.p; }
int pw_batch_packed_total_async(pw_batch* b, uint64_t* host_out, void* stream) {
  if (!b->d_txoffsets.p) return fail("pw_batch_packed_total_async before pw_batch_pack_transcripts");
  HIP_TRY(hipSetDevice(b->device));
  HIP_TRY(hipMemcpyAsync(host_out, b->d_txoffsets.p + b->n, sizeof *host_out, hipMemcpyDeviceToHost, (hipStream_t)stream));
  return mark_done(b, (hipStream_t)stream);
}
int pw_batch_packed(pw_batch* b, uint8_t* out, uint64_t cap, uint64_t* offsets_out) {
  if (!b->d_txoffsets.p) return fail("pw_batch_packed before pw_batch_pack_transcripts");
  HIP_TRY(hipSetDevice(b->device));
  std::vector<uint64_t> off((size_t)b->n + 1);
  HIP_TRY(hipMemcpy(off.data(), b->d_txoffsets.p, b->d_txoffsets.bytes(off.size()), hipMemcpyDeviceToHost));
  if (offsets_out) memcpy(offsets_out, off.data(), 8 * off.size());
  if (out) {
    if (off[b->n] > cap) return fail("packed transcripts: buffer too small");
    if (off[b->n]) HIP_TRY(hipMemcpy(out, b->d_txpacked.p, off[b->n], hipMemcpyDeviceToHost));
  }
  return 0;
}

// ---- alignment summaries (include/pw_txsum.h; kernel in pw_txsum.hip) ----
int pw_batch_summarize(pw_batch* b, void* stream) {
  if (!b->traced) return fail("pw_batch_summarize before a traceback of the batch");
  HIP_TRY(hipSetDevice(b->device));
  if (!b->d_summaries.p) HIP_TRY(b->d_summaries.alloc(b->device, sizeof(pw_tx_summary) * (size_t)std::max<int32_t>(b->n, 1)));
  HIP_TRY(pw::launch_tx_summary(b->d_pairs.p, b->d_results.p, b->d_tx.p, b->n, b->d_summaries.p, (hipStream_t)stream));
  b->summary_seq = b->trace_seq;
  return mark_done(b, (hipStream_t)stream);
}
void* pw_batch_summaries_device(pw_batch* b) { return b->d_summaries.p; }
int pw_batch_summaries_async(pw_batch* b, pw_tx_summary* out, void* stream) {
  if (!b->d_summaries.p) return fail("pw_batch_summaries_async before pw_batch_summarize");
  HIP_TRY(hipSetDevice(b->device));
  if (b->n) HIP_TRY(hipMemcpyAsync(out, b->d_summaries.p, sizeof(pw_tx_summary) * (size_t)b->n, hipMemcpyDeviceToHost, (hipStream_t)stream));
  return mark_done(b, (hipStream_t)stream);
}
int pw_batch_summaries(pw_batch* b, pw_tx_summary* out) {
  if (!b->traced) return fail("pw_batch_summaries before a traceback of the batch");
  // (as for pw_batch_results: callers that launched on another stream synchronise it first)
  if ((!b->d_summaries.p || b->summary_seq != b->trace_seq) && pw_batch_summarize(b, nullptr) != 0) return -1;
  HIP_TRY(hipSetDevice(b->device));
  if (b->n) HIP_TRY(hipMemcpy(out, b->d_summaries.p, sizeof(pw_tx_summary) * (size_t)b->n, hipMemcpyDeviceToHost));
  return 0;
}
int pw_tx_summarize_packed(int device, const uint8_t* ops, const uint64_t* offsets, int64_t n, pw_tx_summary* out) {
  if (n < 0 || n > INT32_MAX) return fail("pw_tx_summarize_packed: transcript count out of range");
  if (n == 0) return 0;
  if (!offsets || !out) return fail("pw_tx_summarize_packed: null offsets or output");
  for (int64_t k = 0; k < n; k++) {
    if (offsets[k + 1] < offsets[k]) return fail("pw_tx_summarize_packed: offsets must ascend");
    if (offsets[k + 1] - offsets[k] > (uint64_t)INT32_MAX) return fail("pw_tx_summarize_packed: a transcript of 2^31 ops or more");
  }
  const uint64_t total = offsets[n];
  if (total && !ops) return fail("pw_tx_summarize_packed: null ops with a non-zero total");
  HIP_TRY(hipSetDevice(device));
  DeviceArray<uint8_t> d_ops; DeviceArray<uint64_t> d_off; DeviceArray<pw_tx_summary> d_out;
  HIP_TRY(d_ops.ensure((size_t)total));
  HIP_TRY(d_off.ensure((size_t)n + 1));
  HIP_TRY(d_out.ensure((size_t)n));
  if (upload(fail, d_ops, ops, (size_t)total) != 0 || upload(fail, d_off, offsets, (size_t)n + 1) != 0) return -1;
  HIP_TRY(pw::launch_tx_summary_packed(d_ops.p, d_off.p, (int)n, d_out.p, nullptr));
  HIP_TRY(hipMemcpy(out, d_out.p, d_out.bytes((size_t)n), hipMemcpyDeviceToHost));
  return 0;
}

// ---- CIGARs (include/pw_cigar.h; kernels in pw_cigar.hip) ----
namespace {
bool cigar_form_ok(int form) { return form == PW_CIGAR_EXTENDED || form == PW_CIGAR_CLASSIC; }
}  // namespace
int pw_batch_cigars(pw_batch* b, int form, void* stream) {
  if (!b->traced) return fail("pw_batch_cigars before a traceback of the batch");
  if (!cigar_form_ok(form)) return fail("pw_batch_cigars: unknown form (PW_CIGAR_EXTENDED or PW_CIGAR_CLASSIC)");
  for (const pw::PairDesc& d : b->descs)
    if ((int64_t)d.tx_cap >= (int64_t)PW_CIGAR_MAX_LEN) return fail("pw_batch_cigars: a transcript slot of 2^28 bytes or more (run lengths are 28 bits)");
  const hipStream_t st = (hipStream_t)stream;
  HIP_TRY(hipSetDevice(b->device));
  // (the offsets are rewritten in place: a write kernel of an earlier call on ANOTHER stream may still read them)
  if (b->d_cigoffsets.p && st != b->cigar_stream)
    for (auto& se : b->done_events) HIP_TRY(hipEventSynchronize(se.second.e));
  b->cigar_stream = st;
  HIP_TRY(b->d_cigoffsets.ensure((size_t)b->n + 1));
  HIP_TRY(pw::launch_cigar_count(b->d_pairs.p, b->d_results.p, b->d_tx.p, b->n, form, b->d_cigoffsets.p, st));
  // the one blocking read: the total sizes the run buffer
  uint64_t total = 0;
  HIP_TRY(hipMemcpyAsync(&total, b->d_cigoffsets.p + b->n, sizeof total, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  if (!b->d_cigruns.p || total > b->cigar_room) {
    // (a write of an earlier call may still run on another stream: the old buffer goes back to the pool only behind it)
    for (auto& se : b->done_events) HIP_TRY(hipEventSynchronize(se.second.e));
    HIP_TRY(b->d_cigruns.alloc(b->device, 4 * (size_t)std::max<uint64_t>(total, 4)));
    b->cigar_room = std::max<uint64_t>(total, 4);
  }
  HIP_TRY(pw::launch_cigar_write(b->d_pairs.p, b->d_results.p, b->d_tx.p, b->n, form, b->d_cigoffsets.p, b->d_cigruns.p, st));
  b->cigar_total = total; b->cigar_seq = b->trace_seq; b->cigar_form = form;
  return mark_done(b, st);
}
void* pw_batch_cigar_runs_device(pw_batch* b) { return b->d_cigruns.p; }
void* pw_batch_cigar_offsets_device(pw_batch* b) { return b->d_cigoffsets.p; }
uint64_t pw_batch_cigar_total(const pw_batch* b) { return b->d_cigoffsets.p ? b->cigar_total : 0; }
int pw_batch_cigar(pw_batch* b, int form, uint32_t* runs_out, uint64_t cap, uint64_t* offsets_out) {
  if (!b->traced) return fail("pw_batch_cigar before a traceback of the batch");
  if (!cigar_form_ok(form)) return fail("pw_batch_cigar: unknown form (PW_CIGAR_EXTENDED or PW_CIGAR_CLASSIC)");
  // (as for pw_batch_results: callers that launched on another stream synchronise it first)
  if ((!b->d_cigruns.p || b->cigar_seq != b->trace_seq || b->cigar_form != form) && pw_batch_cigars(b, form, nullptr) != 0) return -1;
  if (runs_out && b->cigar_total > cap) return fail("pw_batch_cigar: run buffer too small");
  HIP_TRY(hipSetDevice(b->device));
  if (offsets_out) HIP_TRY(hipMemcpy(offsets_out, b->d_cigoffsets.p, b->d_cigoffsets.bytes((size_t)b->n + 1), hipMemcpyDeviceToHost));
  if (runs_out && b->cigar_total) HIP_TRY(hipMemcpy(runs_out, b->d_cigruns.p, 4 * (size_t)b->cigar_total, hipMemcpyDeviceToHost));
  return 0;
}
int pw_tx_cigar_packed(int device, const uint8_t* ops, const uint64_t* offsets, int64_t n, int form, uint32_t* runs_out, uint64_t cap,
                       uint64_t* run_offsets_out) {
  if (n < 0 || n > INT32_MAX) return fail("pw_tx_cigar_packed: transcript count out of range");
  if (!cigar_form_ok(form)) return fail("pw_tx_cigar_packed: unknown form (PW_CIGAR_EXTENDED or PW_CIGAR_CLASSIC)");
  if (n == 0) return 0;
  if (!offsets || !run_offsets_out) return fail("pw_tx_cigar_packed: null offsets or output");
  for (int64_t k = 0; k < n; k++) {
    if (offsets[k + 1] < offsets[k]) return fail("pw_tx_cigar_packed: offsets must ascend");
    if (offsets[k + 1] - offsets[k] >= (uint64_t)PW_CIGAR_MAX_LEN) return fail("pw_tx_cigar_packed: a transcript of 2^28 ops or more");
  }
  const uint64_t total = offsets[n];
  if (total && !ops) return fail("pw_tx_cigar_packed: null ops with a non-zero total");
  for (uint64_t k = offsets[0]; k < total; k++)
    if (ops[k] != 'M' && ops[k] != 'S' && ops[k] != 'I' && ops[k] != 'D')
      return fail("pw_tx_cigar_packed: byte " + std::to_string(k) + " is none of M, S, I, D");
  HIP_TRY(hipSetDevice(device));
  DeviceArray<uint8_t> d_ops; DeviceArray<uint64_t> d_off, d_roff; DeviceArray<uint32_t> d_runs;
  HIP_TRY(d_ops.ensure((size_t)total));
  HIP_TRY(d_off.ensure((size_t)n + 1));
  HIP_TRY(d_roff.ensure((size_t)n + 1));
  if (upload(fail, d_ops, ops, (size_t)total) != 0 || upload(fail, d_off, offsets, (size_t)n + 1) != 0) return -1;
  HIP_TRY(pw::launch_cigar_count_packed(d_ops.p, d_off.p, (int)n, form, d_roff.p, nullptr));
  std::vector<uint64_t> roff((size_t)n + 1);
  HIP_TRY(hipMemcpy(roff.data(), d_roff.p, d_roff.bytes(roff.size()), hipMemcpyDeviceToHost));
  if (runs_out) {
    if (roff[n] > cap) return fail("pw_tx_cigar_packed: run buffer too small");
    HIP_TRY(d_runs.ensure((size_t)roff[n]));
    HIP_TRY(pw::launch_cigar_write_packed(d_ops.p, d_off.p, (int)n, form, d_roff.p, d_runs.p, nullptr));
    if (roff[n]) HIP_TRY(hipMemcpy(runs_out, d_runs.p, d_runs.bytes((size_t)roff[n]), hipMemcpyDeviceToHost));
  }
  memcpy(run_offsets_out, roff.data(), 8 * roff.size());
  return 0;
}

// ---- pileups (include/pw_pileup.h; kernels in pw_pileup.hip) ----
struct pw_pileup {
  int device = 0;
  int64_t n_cols = 0;
  int L = 0;
  DeviceArray<uint32_t> d_counts;        // [n_cols][L + 2]
  DeviceArray<pw_pileup_site> d_sites;   // [n_cols]: allocated by the first pw_pileup_call
  size_t row() const { return (size_t)(L + 2); }                         // counters per column
  size_t count_bytes() const { return d_counts.bytes((size_t)n_cols * row()); }
  // include/pw_polish.h: the insertion plane of pw_pileup_create_ins and the results of the last pw_pileup_polish
  int J = 0;                             // ins_slots; 0: no plane
  DeviceArray<uint32_t> d_ins;           // [n_cols][J][L]
  size_t ins_row() const { return (size_t)J * (size_t)L; }
  size_t ins_bytes() const { return d_ins.bytes((size_t)n_cols * ins_row()); }
  bool polished = false;
  int64_t polish_reads = 0, polish_total = 0;
  DeviceArray<int64_t> d_roff;           // [n_reads]
  DeviceArray<int32_t> d_rlen;           // [n_reads]
  DeviceArray<uint64_t> d_plens, d_poffs;   // [n_reads + 1]: emitted lengths, their exclusive sums
  DeviceArray<pw_polish_stats> d_pstats; // [n_reads]
  DeviceArray<uint8_t> d_pletters;       // [polish_total]
  DeviceBuffer polish_tmp;               // rocPRIM's scratch
  std::vector<int64_t> h_roff; std::vector<int32_t> h_rlen;
  pw::ColumnPolish col;                  // include/pw_rounds.h: the per-column arrays of pw_pileup_polish_columns
  std::vector<pw::RoundBlock> h_blocks;
};

pw_pileup* pw_pileup_create(int device, int64_t n_cols, int alphabet_len) {
  if (alphabet_len < 1 || alphabet_len > 32) { fail("pw_pileup_create: alphabet_len must be 1..32"); return nullptr; }
  if (n_cols < 0 || n_cols > ((int64_t)1 << 36)) { fail("pw_pileup_create: n_cols out of range"); return nullptr; }
  std::unique_ptr<pw_pileup> p(new pw_pileup);
  p->device = device; p->n_cols = n_cols; p->L = alphabet_len;
  if (hipSetDevice(device) != hipSuccess || p->d_counts.ensure((size_t)n_cols * p->row()) != hipSuccess ||
      hipMemset(p->d_counts.p, 0, std::max<size_t>(p->count_bytes(), 16)) != hipSuccess) {
    (void)hipGetLastError();
    fail("pw_pileup_create: allocation failed");
    return nullptr;
  }
  return p.release();
}
void pw_pileup_destroy(pw_pileup* p) {
  if (!p) return;
  (void)hipSetDevice(p->device);         // (hipFree waits for the device: no kernel still writes the counts)
  delete p;
}
int pw_pileup_clear(pw_pileup* p, void* stream) {
  if (!p) return fail("pw_pileup_clear: null pileup");
  HIP_TRY(hipSetDevice(p->device));
  if (p->count_bytes()) HIP_TRY(hipMemsetAsync(p->d_counts.p, 0, p->count_bytes(), (hipStream_t)stream));
  if (p->J && p->ins_bytes()) HIP_TRY(hipMemsetAsync(p->d_ins.p, 0, p->ins_bytes(), (hipStream_t)stream));
  return 0;
}
int pw_batch_pileup_add(pw_batch* b, pw_pileup* p, const int64_t* col0, int64_t arena_first, void* stream) {
  if (!b || !p) return fail("pw_batch_pileup_add: null batch or pileup");
  if (!b->traced) return fail("pw_batch_pileup_add before a traceback of the batch");
  if (b->device != p->device) return fail("pw_batch_pileup_add: the batch and the pileup live on different devices");
  if (p->L < 1 || p->L > 32) return fail("pw_batch_pileup_add: alphabet_len must be 1..32");
  const hipStream_t st = (hipStream_t)stream;
  HIP_TRY(hipSetDevice(b->device));
  const int64_t* d_col0 = nullptr;
  if (col0 && b->n) {
    // (the staging buffer is rewritten in place: an add of an earlier call on ANOTHER stream may still read it)
    if (b->d_col0.p) for (auto& se : b->done_events) if (se.first != st) HIP_TRY(hipEventSynchronize(se.second.e));
    b->h_col0.assign(col0, col0 + (size_t)b->n);           // (the caller's array is consumed here: see pw_batch_traceback_from)
    if (upload(fail, b->d_col0, b->h_col0.data(), (size_t)b->n, st) != 0) return -1;
    d_col0 = b->d_col0.p;
  }
  HIP_TRY(pw::launch_pileup_add(b->d_pairs.p, b->d_results.p, b->d_tx.p, b->d_arena, b->n, d_col0, arena_first, p->d_counts.p, p->n_cols,
                                p->L, st));
  return mark_done(b, st);
}
void* pw_pileup_counts_device(pw_pileup* p) { return p ? p->d_counts.p : nullptr; }
int pw_pileup_counts(pw_pileup* p, int64_t lo, int64_t hi, uint32_t* host_out) {
  if (!p) return fail("pw_pileup_counts: null pileup");
  if (lo < 0 || hi < lo || hi > p->n_cols) return fail("pw_pileup_counts: columns outside the pileup");
  if (hi == lo) return 0;
  if (!host_out) return fail("pw_pileup_counts: null output");
  HIP_TRY(hipSetDevice(p->device));
  const size_t row = p->row();
  HIP_TRY(hipMemcpy(host_out, p->d_counts.p + row * (size_t)lo, p->d_counts.bytes(row * (size_t)(hi - lo)), hipMemcpyDeviceToHost));
  return 0;
}
int pw_pileup_set_counts(pw_pileup* p, int64_t lo, int64_t hi, const uint32_t* host_in) {
  if (!p) return fail("pw_pileup_set_counts: null pileup");
  if (lo < 0 || hi < lo || hi > p->n_cols) return fail("pw_pileup_set_counts: columns outside the pileup");
  if (hi == lo) return 0;
  if (!host_in) return fail("pw_pileup_set_counts: null input");
  HIP_TRY(hipSetDevice(p->device));
  const size_t row = p->row();
  HIP_TRY(hipMemcpy(p->d_counts.p + row * (size_t)lo, host_in, p->d_counts.bytes(row * (size_t)(hi - lo)), hipMemcpyHostToDevice));
  return 0;
}
int pw_pileup_call(pw_pileup* p, const uint8_t* ref_letters_device, uint32_t min_depth, void* stream) {
  if (!p) return fail("pw_pileup_call: null pileup");
  HIP_TRY(hipSetDevice(p->device));
  if (!p->d_sites.p) HIP_TRY(p->d_sites.ensure((size_t)p->n_cols));
  HIP_TRY(pw::launch_pileup_call(p->d_counts.p, ref_letters_device, p->n_cols, p->L, min_depth, p->d_sites.p,
                                 (hipStream_t)stream));
  return 0;
}
void* pw_pileup_sites_device(pw_pileup* p) { return p ? p->d_sites.p : nullptr; }
int pw_pileup_sites(pw_pileup* p, int64_t lo, int64_t hi, pw_pileup_site* host_out) {
  if (!p) return fail("pw_pileup_sites: null pileup");
  if (!p->d_sites.p) return fail("pw_pileup_sites before pw_pileup_call");
  if (lo < 0 || hi < lo || hi > p->n_cols) return fail("pw_pileup_sites: columns outside the pileup");
  if (hi == lo) return 0;
  if (!host_out) return fail("pw_pileup_sites: null output");
  HIP_TRY(hipSetDevice(p->device));
  HIP_TRY(hipMemcpy(host_out, p->d_sites.p + lo, p->d_sites.bytes((size_t)(hi - lo)), hipMemcpyDeviceToHost));
  return 0;
}

// ---- read correction (include/pw_polish.h; kernels in pw_polish.hip) ----
pw_pileup* pw_pileup_create_ins(int device, int64_t n_cols, int alphabet_len, int ins_slots) {
  if (ins_slots < 1 || ins_slots > PW_POLISH_MAX_SLOTS) { fail("pw_pileup_create_ins: ins_slots must be 1..8"); return nullptr; }
  std::unique_ptr<pw_pileup> p(pw_pileup_create(device, n_cols, alphabet_len));
  if (!p) return nullptr;
  p->J = ins_slots;
  if (p->d_ins.ensure((size_t)n_cols * p->ins_row()) != hipSuccess || hipMemset(p->d_ins.p, 0, std::max<size_t>(p->ins_bytes(), 16)) != hipSuccess) {
    (void)hipGetLastError();
    (void)hipSetDevice(device);
    fail("pw_pileup_create_ins: allocation failed");
    return nullptr;
  }
  return p.release();
}
int pw_pileup_ins_slots(const pw_pileup* p) { return p ? p->J : 0; }
void* pw_pileup_ins_counts_device(pw_pileup* p) { return p && p->J ? p->d_ins.p : nullptr; }
int pw_pileup_ins_counts(pw_pileup* p, int64_t lo, int64_t hi, uint32_t* host_out) {
  if (!p) return fail("pw_pileup_ins_counts: null pileup");
  if (!p->J) return fail("pw_pileup_ins_counts: the pileup has no insertion plane (pw_pileup_create_ins)");
  if (lo < 0 || hi < lo || hi > p->n_cols) return fail("pw_pileup_ins_counts: columns outside the pileup");
  if (hi == lo) return 0;
  if (!host_out) return fail("pw_pileup_ins_counts: null output");
  HIP_TRY(hipSetDevice(p->device));
  const size_t row = p->ins_row();
  HIP_TRY(hipMemcpy(host_out, p->d_ins.p + row * (size_t)lo, p->d_ins.bytes(row * (size_t)(hi - lo)), hipMemcpyDeviceToHost));
  return 0;
}
int pw_batch_pileup_add_sides(pw_batch* b, pw_pileup* p, int sides, const int64_t* origin_col0, const int64_t* mutant_col0,
                              const uint8_t* reversed, const uint8_t* complement, int complement_len, int64_t arena_first, void* stream) {
  if (sides < PW_SIDE_ORIGIN || sides > PW_SIDE_BOTH) return fail("pw_batch_pileup_add_sides: sides must be 1 (origin), 2 (mutant) or 3 (both)");
  if (!b || !p) return fail("pw_batch_pileup_add_sides: null batch or pileup");
  if (!b->traced) return fail("pw_batch_pileup_add_sides before a traceback of the batch");
  if (b->device != p->device) return fail("pw_batch_pileup_add_sides: the batch and the pileup live on different devices");
  if (p->L < 1 || p->L > 32) return fail("pw_batch_pileup_add_sides: alphabet_len must be 1..32");
  const size_t n = (size_t)b->n;
  bool any_rev = false;
  if (reversed && (sides & PW_SIDE_MUTANT)) for (size_t k = 0; k < n && !any_rev; k++) any_rev = reversed[k] != 0;
  pw::PolishComplement comp = {{0, 0, 0, 0, 0, 0, 0, 0}};
  if (any_rev) {
    if (!complement) return fail("pw_batch_pileup_add_sides: reversed pairs need a complement");
    if (complement_len != p->L) return fail("pw_batch_pileup_add_sides: complement_len must be the pileup's alphabet_len");
    if (check_complement(fail, complement, p->L) != 0) return -1;
    memcpy(comp.w, complement, (size_t)p->L);
  }
  const hipStream_t st = (hipStream_t)stream;
  HIP_TRY(hipSetDevice(b->device));
  const int64_t *d_o = nullptr, *d_m = nullptr;
  const uint8_t* d_rev = nullptr;
  if (n && (origin_col0 || mutant_col0 || any_rev)) {
    // (the staging buffers are rewritten in place: an add of an earlier call on ANOTHER stream may still read them)
    if (b->d_sides_col0.p || b->d_reversed.p) for (auto& se : b->done_events) if (se.first != st) HIP_TRY(hipEventSynchronize(se.second.e));
    b->h_sides_col0.assign(2 * n, 0);                        // (the caller's arrays are consumed here: see pw_batch_traceback_from)
    if (origin_col0) std::copy(origin_col0, origin_col0 + n, b->h_sides_col0.begin());
    if (mutant_col0) std::copy(mutant_col0, mutant_col0 + n, b->h_sides_col0.begin() + n);
    if (origin_col0 || mutant_col0) {
      if (upload(fail, b->d_sides_col0, b->h_sides_col0.data(), 2 * n, st) != 0) return -1;
      if (origin_col0) d_o = b->d_sides_col0.p;
      if (mutant_col0) d_m = b->d_sides_col0.p + n;
    }
    if (any_rev) {
      b->h_reversed.assign(reversed, reversed + n);
      if (upload(fail, b->d_reversed, b->h_reversed.data(), n, st) != 0) return -1;
      d_rev = b->d_reversed.p;
    }
  }
  HIP_TRY(pw::launch_polish_add(b->d_pairs.p, b->d_results.p, b->d_tx.p, b->d_arena, b->n, sides, d_o, d_m, d_rev, comp, arena_first,
                                p->d_counts.p, p->J ? p->d_ins.p : nullptr, p->n_cols, p->L, p->J, st));
  return mark_done(b, st);
}
int pw_pileup_add_letters(pw_pileup* p, const uint8_t* letters_device, int64_t lo, int64_t hi, uint32_t weight, void* stream) {
  if (!p) return fail("pw_pileup_add_letters: null pileup");
  if (lo < 0 || hi < lo || hi > p->n_cols) return fail("pw_pileup_add_letters: columns outside the pileup");
  if (hi == lo) return 0;
  if (!letters_device) return fail("pw_pileup_add_letters: null letters");
  HIP_TRY(hipSetDevice(p->device));
  HIP_TRY(pw::launch_polish_letters(p->d_counts.p, letters_device, lo, hi, p->L, weight, (hipStream_t)stream));
  return 0;
}
int pw_pileup_polish(pw_pileup* p, const uint8_t* letters_device, const int64_t* read_offs, const int32_t* read_lens, int64_t n_reads,
                     uint32_t min_depth, void* stream) {
  if (!p) return fail("pw_pileup_polish: null pileup");
  if (n_reads < 0 || n_reads > INT32_MAX || (n_reads > 0 && (!read_offs || !read_lens))) return fail("pw_pileup_polish: bad read arrays");
  bool letters_needed = false;
  for (int64_t r = 0; r < n_reads; r++) {
    if (read_lens[r] < 0 || read_offs[r] < 0 || read_offs[r] > p->n_cols || read_lens[r] > p->n_cols - read_offs[r])
      return fail("pw_pileup_polish: read " + std::to_string(r) + " lies outside the pileup");
    letters_needed = letters_needed || read_lens[r] > 0;
  }
  if (letters_needed && !letters_device) return fail("pw_pileup_polish: null letters");
  const hipStream_t st = (hipStream_t)stream;
  const size_t n = (size_t)n_reads;
  HIP_TRY(hipSetDevice(p->device));
  p->polished = false; p->col.valid = false;
  p->h_roff.assign(read_offs, read_offs + n);                // (the caller's arrays are consumed here)
  p->h_rlen.assign(read_lens, read_lens + n);
  if (upload(fail, p->d_roff, p->h_roff.data(), n, st) != 0 || upload(fail, p->d_rlen, p->h_rlen.data(), n, st) != 0) return -1;
  HIP_TRY(p->d_plens.ensure(n + 1));
  HIP_TRY(p->d_poffs.ensure(n + 1));
  HIP_TRY(p->d_pstats.ensure(n));
  const uint32_t* ins = p->J ? p->d_ins.p : nullptr;
  HIP_TRY(pw::launch_polish_count(p->d_counts.p, ins, letters_device, p->d_roff.p, p->d_rlen.p, n_reads, p->L, p->J, min_depth, p->d_plens.p,
                                  p->d_poffs.p, p->d_pstats.p, p->polish_tmp, st));
  uint64_t total = 0;                                        // the output is allocated from the counted total
  HIP_TRY(hipMemcpyAsync(&total, p->d_poffs.p + n, 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  HIP_TRY(p->d_pletters.ensure((size_t)total));
  HIP_TRY(pw::launch_polish_write(p->d_counts.p, ins, letters_device, p->d_roff.p, p->d_rlen.p, n_reads, p->L, p->J, min_depth, p->d_poffs.p,
                                  p->d_pletters.p, st));
  HIP_TRY(hipStreamSynchronize(st));                         // (the call is synchronous: it has waited for the total already)
  p->polish_reads = n_reads; p->polish_total = (int64_t)total; p->polished = true;
  return 0;
}
int64_t pw_pileup_polished_total(pw_pileup* p) {
  if (!p) return fail("pw_pileup_polished_total: null pileup");
  if (!p->polished) return fail("pw_pileup_polished_total before pw_pileup_polish");
  return p->polish_total;
}
int pw_pileup_polished_offsets(pw_pileup* p, int64_t* host_out) {
  if (!p) return fail("pw_pileup_polished_offsets: null pileup");
  if (!p->polished) return fail("pw_pileup_polished_offsets before pw_pileup_polish");
  if (!host_out) return fail("pw_pileup_polished_offsets: null output");
  HIP_TRY(hipSetDevice(p->device));
  HIP_TRY(hipMemcpy(host_out, p->d_poffs.p, p->d_poffs.bytes((size_t)p->polish_reads + 1), hipMemcpyDeviceToHost));
  return 0;
}
int pw_pileup_polished_letters(pw_pileup* p, uint8_t* host_out) {
  if (!p) return fail("pw_pileup_polished_letters: null pileup");
  if (!p->polished) return fail("pw_pileup_polished_letters before pw_pileup_polish");
  if (p->polish_total == 0) return 0;
  if (!host_out) return fail("pw_pileup_polished_letters: null output");
  HIP_TRY(hipSetDevice(p->device));
  HIP_TRY(hipMemcpy(host_out, p->d_pletters.p, (size_t)p->polish_total, hipMemcpyDeviceToHost));
  return 0;
}
int pw_pileup_polished_stats(pw_pileup* p, pw_polish_stats* host_out) {
  if (!p) return fail("pw_pileup_polished_stats: null pileup");
  if (!p->polished) return fail("pw_pileup_polished_stats before pw_pileup_polish");
  if (p->polish_reads == 0) return 0;
  if (!host_out) return fail("pw_pileup_polished_stats: null output");
  HIP_TRY(hipSetDevice(p->device));
  HIP_TRY(hipMemcpy(host_out, p->d_pstats.p, p->d_pstats.bytes((size_t)p->polish_reads), hipMemcpyDeviceToHost));
  return 0;
}
void* pw_pileup_polished_letters_device(pw_pileup* p) {
  if (!p || !p->polished) { fail("pw_pileup_polished_letters_device before pw_pileup_polish"); return nullptr; }
  return p->d_pletters.p;
}
void* pw_pileup_polished_offsets_device(pw_pileup* p) {
  if (!p || !p->polished) { fail("pw_pileup_polished_offsets_device before pw_pileup_polish"); return nullptr; }
  return p->d_poffs.p;
}

// ---- the column polish (include/pw_rounds.h; kernels and stage sequences in pw_rounds.hip) ----
int pw_pileup_polish_columns(pw_pileup* p, const uint8_t* letters_device, const int64_t* read_offs, const int32_t* read_lens, int64_t n_reads,
                             uint32_t min_depth, void* stream) {
  if (!p) return fail("pw_pileup_polish_columns: null pileup");
  if (n_reads < 0 || n_reads > INT32_MAX || (n_reads > 0 && (!read_offs || !read_lens))) return fail("pw_pileup_polish_columns: bad read arrays");
  bool letters_needed = false;
  int64_t n_blocks = 0;
  for (int64_t r = 0; r < n_reads; r++) {
    if (read_lens[r] < 0 || read_offs[r] < 0 || read_offs[r] > p->n_cols || read_lens[r] > p->n_cols - read_offs[r])
      return fail("pw_pileup_polish_columns: read " + std::to_string(r) + " lies outside the pileup");
    if (r > 0 && read_offs[r] < read_offs[r - 1])
      return fail("pw_pileup_polish_columns: read " + std::to_string(r) + " is not in column order");
    if (r > 0 && read_offs[r - 1] + read_lens[r - 1] > read_offs[r])
      return fail("pw_pileup_polish_columns: read " + std::to_string(r) + " overlaps read " + std::to_string(r - 1));
    letters_needed = letters_needed || read_lens[r] > 0;
    n_blocks += ((int64_t)read_lens[r] + pw::kRoundChunk - 1) / pw::kRoundChunk;
  }
  if (letters_needed && !letters_device) return fail("pw_pileup_polish_columns: null letters");
  if (n_blocks > INT32_MAX) return fail("pw_pileup_polish_columns: more than 2^31 chunks of columns");
  const hipStream_t st = (hipStream_t)stream;
  const size_t n = (size_t)n_reads;
  HIP_TRY(hipSetDevice(p->device));
  p->polished = false; p->col.valid = false;
  p->h_roff.assign(read_offs, read_offs + n);                // (the caller's arrays are consumed here)
  p->h_rlen.assign(read_lens, read_lens + n);
  p->h_blocks.clear();
  p->h_blocks.reserve((size_t)n_blocks);
  for (int64_t r = 0; r < n_reads; r++)                      // one workgroup per 256 columns of a read: no kernel searches for its read
    for (int32_t k = 0; (int64_t)k * pw::kRoundChunk < read_lens[r]; k++) p->h_blocks.push_back({(int32_t)r, k});
  if (upload(fail, p->d_roff, p->h_roff.data(), n, st) != 0 || upload(fail, p->d_rlen, p->h_rlen.data(), n, st) != 0 ||
      upload(fail, p->col.d_blocks, p->h_blocks.data(), (size_t)n_blocks, st) != 0)
    return -1;
  HIP_TRY(p->d_poffs.ensure(n + 1));
  HIP_TRY(p->d_pstats.ensure(n));
  const uint32_t* ins = p->J ? p->d_ins.p : nullptr;
  HIP_TRY(pw::round_polish_count(p->col, p->d_counts.p, ins, letters_device, p->d_roff.p, p->d_rlen.p, n_blocks, n_reads, p->n_cols, p->L, p->J,
                                 min_depth, p->d_poffs.p, p->d_pstats.p, p->polish_tmp, st));
  uint64_t total = 0;                                        // the output is allocated from the counted total
  HIP_TRY(hipMemcpyAsync(&total, p->col.d_colmap.p + p->n_cols, 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  HIP_TRY(p->d_pletters.ensure((size_t)total));
  HIP_TRY(pw::round_polish_write(p->col, p->d_roff.p, p->d_rlen.p, n_blocks, total, p->d_pletters.p, st));
  HIP_TRY(hipStreamSynchronize(st));                         // (the call is synchronous: it has waited for the total already)
  p->polish_reads = n_reads; p->polish_total = (int64_t)total; p->polished = true; p->col.valid = true;
  return 0;
}
void* pw_pileup_colmap_device(pw_pileup* p) {
  if (!p || !p->polished || !p->col.valid) { fail("pw_pileup_colmap_device before pw_pileup_polish_columns"); return nullptr; }
  return p->col.d_colmap.p;
}
int pw_pileup_colmap(pw_pileup* p, int64_t lo, int64_t hi, uint64_t* host_out) {
  if (!p) return fail("pw_pileup_colmap: null pileup");
  if (!p->polished || !p->col.valid) return fail("pw_pileup_colmap before pw_pileup_polish_columns");
  if (lo < 0 || hi < lo || hi > p->n_cols + 1) return fail("pw_pileup_colmap: entries outside 0 .. n_cols + 1");
  if (hi == lo) return 0;
  if (!host_out) return fail("pw_pileup_colmap: null output");
  HIP_TRY(hipSetDevice(p->device));
  HIP_TRY(hipMemcpy(host_out, p->col.d_colmap.p + lo, p->col.d_colmap.bytes((size_t)(hi - lo)), hipMemcpyDeviceToHost));
  return 0;
}

// ---- the overlap graph (include/pw_graph.h; kernels and stage sequences in pw_graph.hip) ----
struct pw_graph {
  pw::GraphState s;
  pw::ConsState c;                       // the consensus stage (include/pw_consensus.h; pw_consensus.hip)
  pw::RoundState r;                      // its later rounds (include/pw_rounds.h; pw_rounds.hip)
  std::vector<int32_t> lens;             // [n_reads]
  std::unordered_set<uint64_t> keys;     // (a * n_reads + b) * 2 + strand of every record
  std::string duplicate;                 // the first duplicate key, in words; pw_graph_build reports it
  std::vector<int32_t> h_stage;          // pw_batch_graph_add: the host copy d_stage is uploaded from
  std::vector<int64_t> h_roff;           // pw_graph_contigs: ... and d_roff
};

namespace {

// what both add paths refuse of (a, b, strand), and the duplicate keys they remember for the build
int graph_check_key(const char* who, pw_graph* g, int64_t k, int64_t a, int64_t b, int64_t strand) {
  const int64_t R = g->s.n_reads;
  if (a < 0 || a >= R || b < 0 || b >= R) return fail(std::string(who) + ": record " + std::to_string(k) + " names a read outside the graph");
  if (a == b) return fail(std::string(who) + ": record " + std::to_string(k) + " pairs read " + std::to_string(a) + " with itself");
  if (strand != 0 && strand != 1) return fail(std::string(who) + ": record " + std::to_string(k) + " has a strand other than 0 / 1");
  return 0;
}
void graph_note_key(pw_graph* g, int64_t a, int64_t b, int64_t strand) {
  if (!g->keys.insert((uint64_t)((a * g->s.n_reads + b) * 2 + strand)).second && g->duplicate.empty())
    g->duplicate = "(" + std::to_string(a) + ", " + std::to_string(b) + ", " + std::to_string(strand) + ")";
}

}  // namespace

pw_graph* pw_graph_create(int device, int64_t n_reads, const int32_t* read_lens) {
  if (n_reads < 0 || n_reads > ((int64_t)1 << 28)) { fail("pw_graph_create: n_reads out of range"); return nullptr; }
  if (n_reads > 0 && !read_lens) { fail("pw_graph_create: null read lengths"); return nullptr; }
  for (int64_t r = 0; r < n_reads; r++)
    if (read_lens[r] < 0) { fail("pw_graph_create: read " + std::to_string(r) + " has a negative length"); return nullptr; }
  std::unique_ptr<pw_graph> g(new pw_graph);
  g->s.device = device; g->s.n_reads = n_reads; g->s.V = 2 * n_reads;
  g->lens.assign(read_lens, read_lens + n_reads);
  if (hipSetDevice(device) != hipSuccess || upload(fail, g->s.d_lens, g->lens.data(), (size_t)n_reads) != 0) {
    fail("pw_graph_create: allocation failed");
    return nullptr;
  }
  return g.release();
}
void pw_graph_free(pw_graph* g) {
  if (!g) return;
  (void)hipSetDevice(g->s.device);
  delete g;
}
int64_t pw_graph_num_overlaps(const pw_graph* g) { return g ? g->s.n_recs : 0; }
int64_t pw_graph_device_bytes(const pw_graph* g) { return g ? pw::graph_device_bytes(g->s) + pw::cons_device_bytes(g->c) + pw::round_device_bytes(g->r) : 0; }

int pw_graph_add_overlaps(pw_graph* g, const pw_graph_overlap* recs, int64_t n) {
  if (!g) return fail("pw_graph_add_overlaps: null graph");
  if (n < 0 || g->s.n_recs + n > ((int64_t)1 << 30)) return fail("pw_graph_add_overlaps: record count out of range");
  if (n == 0) return 0;
  if (!recs) return fail("pw_graph_add_overlaps: null records");
  for (int64_t k = 0; k < n; k++) {
    const pw_graph_overlap& r = recs[k];
    if (graph_check_key("pw_graph_add_overlaps", g, k, r.a, r.b, r.strand) != 0) return -1;
    const int la = g->lens[(size_t)r.a], lb = g->lens[(size_t)r.b];
    if (r.a_beg < 0 || r.a_beg > r.a_end || r.a_end > la || r.b_beg < 0 || r.b_beg > r.b_end || r.b_end > lb)
      return fail("pw_graph_add_overlaps: record " + std::to_string(k) + " has an interval outside its read");
    if (r.n_match < 0 || r.n_match > r.n_ops) return fail("pw_graph_add_overlaps: record " + std::to_string(k) + " has not 0 <= n_match <= n_ops");
  }
  HIP_TRY(hipSetDevice(g->s.device));
  HIP_TRY(pw::graph_reserve(g->s, n, nullptr));
  std::vector<pw_graph_overlap> tmp(recs, recs + n);
  for (auto& r : tmp) r.cls = PW_OVL_NONE;
  HIP_TRY(hipMemcpy(g->s.d_recs.p + g->s.n_recs, tmp.data(), sizeof(pw_graph_overlap) * (size_t)n, hipMemcpyHostToDevice));
  for (int64_t k = 0; k < n; k++) graph_note_key(g, recs[k].a, recs[k].b, recs[k].strand);
  g->s.n_recs += n;
  return 0;
}

int pw_batch_graph_add(pw_batch* b, pw_graph* g, const int32_t* read_a, const int32_t* read_b, const uint8_t* strand, void* stream) {
  if (!b || !g) return fail("pw_batch_graph_add: null batch or graph");
  if (!b->traced) return fail("pw_batch_graph_add before a traceback of the batch");
  if (b->device != g->s.device) return fail("pw_batch_graph_add: the batch and the graph live on different devices");
  const int64_t n = b->n;
  if (g->s.n_recs + n > ((int64_t)1 << 30)) return fail("pw_batch_graph_add: record count out of range");
  if (n == 0) return 0;
  if (!read_a || !read_b) return fail("pw_batch_graph_add: null read indices");
  for (int64_t k = 0; k < n; k++) {
    if (graph_check_key("pw_batch_graph_add", g, k, read_a[k], read_b[k], strand ? strand[k] : 0) != 0) return -1;
    if (b->pairs[(size_t)k].origin_len != g->lens[(size_t)read_a[k]] || b->pairs[(size_t)k].mutant_len != g->lens[(size_t)read_b[k]])
      return fail("pw_batch_graph_add: the frames of pair " + std::to_string(k) + " are not the whole reads " + std::to_string(read_a[k]) +
                  " and " + std::to_string(read_b[k]));
  }
  const hipStream_t st = (hipStream_t)stream;
  if ((!b->d_summaries.p || b->summary_seq != b->trace_seq) && pw_batch_summarize(b, stream) != 0) return -1;
  HIP_TRY(hipSetDevice(b->device));
  HIP_TRY(pw::graph_reserve(g->s, n, st));
  HIP_TRY(hipStreamSynchronize(st));                         // (the staging array is rewritten in place: the last add has read it)
  g->h_stage.resize(3 * (size_t)n);                          // (the caller's arrays are consumed here)
  for (int64_t k = 0; k < n; k++) {
    g->h_stage[(size_t)k] = read_a[k]; g->h_stage[(size_t)(n + k)] = read_b[k]; g->h_stage[(size_t)(2 * n + k)] = strand ? strand[k] : 0;
  }
  if (upload(fail, g->s.d_stage, g->h_stage.data(), 3 * (size_t)n, st) != 0) return -1;
  HIP_TRY(pw::launch_graph_from_batch(g->s, b->d_results.p, b->d_summaries.p, (int)n, st));
  for (int64_t k = 0; k < n; k++) graph_note_key(g, read_a[k], read_b[k], strand ? strand[k] : 0);
  g->s.n_recs += n;
  return mark_done(b, st);
}

int pw_graph_build(pw_graph* g, const pw_graph_params* p, void* stream) { return pw_graph_build_clean(g, p, nullptr, stream); }

int pw_graph_build_clean(pw_graph* g, const pw_graph_params* p, const pw_graph_clean_params* c, void* stream) {
  static_assert(sizeof(pw_graph_clean_params) == 16, "cleaning parameter record must be 16 bytes");
  if (!g || !p) return fail("pw_graph_build: null graph or parameters");
  if (c && (c->max_tip_reads < 0 || c->max_bubble_reads < 0)) return fail("pw_graph_build_clean: max_tip_reads and max_bubble_reads must not be negative");
  if (c && (c->rounds < 0 || c->rounds > 8)) return fail("pw_graph_build_clean: rounds must lie in 0 .. 8");
  const pw_graph_clean_params clean = c ? *c : pw_graph_clean_params{0, 0, 0, 0};
  if (!g->duplicate.empty()) return fail("pw_graph_build: duplicate overlap key " + g->duplicate);
  if (!std::isfinite(p->int_frac) || !std::isfinite(p->min_identity)) return fail("pw_graph_build: int_frac and min_identity must be finite");
  if (p->max_hang < 0 || p->min_overlap < 0 || p->fuzz < 0) return fail("pw_graph_build: max_hang, min_overlap and fuzz must not be negative");
  HIP_TRY(hipSetDevice(g->s.device));
  g->c.placed = false; g->c.has_layout = false;              // (a build drops every consensus result)
  HIP_TRY(pw::graph_build(g->s, *p, clean, (hipStream_t)stream));
  return 0;
}

int64_t pw_graph_num_arcs(pw_graph* g) { return g && g->s.built ? g->s.n_arcs : fail("pw_graph_num_arcs before pw_graph_build"); }
int64_t pw_graph_num_unitigs(pw_graph* g) { return g && g->s.built ? g->s.n_unitigs : fail("pw_graph_num_unitigs before pw_graph_build"); }
double pw_graph_reduce_ms(pw_graph* g) { return g && g->s.built ? g->s.reduce_ms : -1.; }
int64_t pw_graph_num_members(pw_graph* g) { return g && g->s.built ? g->s.n_members : fail("pw_graph_num_members before pw_graph_build"); }

namespace {

extern "C++" {
template <class T, class U>
int graph_copy_out(const char* who, pw_graph* g, bool ready, const DeviceArray<T>& arr, int64_t count, U* host_out) {
  if (!g) return fail(std::string(who) + ": null graph");
  if (!ready) return fail(std::string(who) + " before pw_graph_build");
  if (count == 0) return 0;
  if (!host_out) return fail(std::string(who) + ": null output");
  static_assert(sizeof(T) == sizeof(U), "host and device records have one size");
  HIP_TRY(hipSetDevice(g->s.device));
  HIP_TRY(hipMemcpy(host_out, arr.p, arr.bytes((size_t)count), hipMemcpyDeviceToHost));
  return 0;
}
template <class T>
void* graph_device_ptr(const char* who, pw_graph* g, bool ready, const DeviceArray<T>& arr) {
  if (!g || !ready) { fail(std::string(who) + " before pw_graph_build"); return nullptr; }
  return arr.p;
}
}  // extern "C++"

}  // namespace

int pw_graph_overlaps(pw_graph* g, pw_graph_overlap* out) { if (!g) return fail("pw_graph_overlaps: null graph"); return graph_copy_out("pw_graph_overlaps", g, true, g->s.d_recs, g->s.n_recs, out); }
int pw_graph_contained(pw_graph* g, uint8_t* out) { if (!g) return fail("pw_graph_contained: null graph"); return graph_copy_out("pw_graph_contained", g, g && g->s.built, g->s.d_contained, g->s.n_reads, out); }
int pw_graph_dropped(pw_graph* g, uint8_t* out) { if (!g) return fail("pw_graph_dropped: null graph"); return graph_copy_out("pw_graph_dropped", g, g && g->s.built, g->s.d_dropped, g->s.n_reads, out); }
void* pw_graph_dropped_device(pw_graph* g) { if (!g) { fail("pw_graph_dropped_device: null graph"); return nullptr; } return graph_device_ptr("pw_graph_dropped_device", g, g && g->s.built, g->s.d_dropped); }
int pw_graph_arcs(pw_graph* g, pw_graph_arc* out) { if (!g) return fail("pw_graph_arcs: null graph"); return graph_copy_out("pw_graph_arcs", g, g && g->s.built, g->s.d_arcs, g->s.n_arcs, out); }
int pw_graph_rows(pw_graph* g, int64_t* out) { if (!g) return fail("pw_graph_rows: null graph"); return graph_copy_out("pw_graph_rows", g, g && g->s.built, g->s.d_rows, g->s.V + 1, out); }
int pw_graph_unitigs(pw_graph* g, pw_unitig* out) { if (!g) return fail("pw_graph_unitigs: null graph"); return graph_copy_out("pw_graph_unitigs", g, g && g->s.built, g->s.d_unitigs, g->s.n_unitigs, out); }
int pw_graph_members(pw_graph* g, pw_unitig_member* out) { if (!g) return fail("pw_graph_members: null graph"); return graph_copy_out("pw_graph_members", g, g && g->s.built, g->s.d_members, g->s.n_members, out); }
void* pw_graph_overlaps_device(pw_graph* g) { if (!g) { fail("pw_graph_overlaps_device: null graph"); return nullptr; } return graph_device_ptr("pw_graph_overlaps_device", g, true, g->s.d_recs); }
void* pw_graph_contained_device(pw_graph* g) { if (!g) { fail("pw_graph_contained_device: null graph"); return nullptr; } return graph_device_ptr("pw_graph_contained_device", g, g && g->s.built, g->s.d_contained); }
void* pw_graph_arcs_device(pw_graph* g) { if (!g) { fail("pw_graph_arcs_device: null graph"); return nullptr; } return graph_device_ptr("pw_graph_arcs_device", g, g && g->s.built, g->s.d_arcs); }
void* pw_graph_rows_device(pw_graph* g) { if (!g) { fail("pw_graph_rows_device: null graph"); return nullptr; } return graph_device_ptr("pw_graph_rows_device", g, g && g->s.built, g->s.d_rows); }
void* pw_graph_unitigs_device(pw_graph* g) { if (!g) { fail("pw_graph_unitigs_device: null graph"); return nullptr; } return graph_device_ptr("pw_graph_unitigs_device", g, g && g->s.built, g->s.d_unitigs); }
void* pw_graph_members_device(pw_graph* g) { if (!g) { fail("pw_graph_members_device: null graph"); return nullptr; } return graph_device_ptr("pw_graph_members_device", g, g && g->s.built, g->s.d_members); }

int pw_graph_contigs(pw_graph* g, const uint8_t* letters_device, const int64_t* read_offs, const uint8_t* complement, int complement_len,
                     void* stream) {
  if (!g) return fail("pw_graph_contigs: null graph");
  if (!g->s.built) return fail("pw_graph_contigs before pw_graph_build");
  if (complement && (complement_len < 1 || complement_len > 256)) return fail("pw_graph_contigs: complement_len must be 1..256");
  const int64_t R = g->s.n_reads;
  if (R > 0 && !read_offs) return fail("pw_graph_contigs: null read offsets");
  for (int64_t r = 0; r < R; r++)
    if (read_offs[r] < 0) return fail("pw_graph_contigs: read " + std::to_string(r) + " has a negative offset");
  if (g->s.n_members > 0 && !letters_device) return fail("pw_graph_contigs: null letters");
  const hipStream_t st = (hipStream_t)stream;
  HIP_TRY(hipSetDevice(g->s.device));
  uint8_t table[256];
  for (int c = 0; c < 256; c++) table[c] = complement && c < complement_len ? complement[c] : (uint8_t)c;
  g->h_roff.assign(read_offs, read_offs + R);                // (the caller's array is consumed here)
  if (upload(fail, g->s.d_roff, g->h_roff.data(), (size_t)R, st) != 0) return -1;
  HIP_TRY(g->s.d_comp.ensure(256));
  HIP_TRY(hipMemcpy(g->s.d_comp.p, table, 256, hipMemcpyHostToDevice));
  g->c.has_layout = false;                                   // (the consensus arena holds the letters of an earlier call)
  HIP_TRY(pw::graph_contigs(g->s, letters_device, st));
  return 0;
}
int64_t pw_graph_contig_total(pw_graph* g) {
  return g && g->s.has_contigs ? g->s.contig_total : fail("pw_graph_contig_total before pw_graph_contigs");
}
int pw_graph_contig_offsets(pw_graph* g, int64_t* out) {
  if (!g || !g->s.has_contigs) return fail("pw_graph_contig_offsets before pw_graph_contigs");
  if (!out) return fail("pw_graph_contig_offsets: null output");
  HIP_TRY(hipSetDevice(g->s.device));
  HIP_TRY(hipMemcpy(out, g->s.d_coff.p, g->s.d_coff.bytes((size_t)g->s.n_unitigs + 1), hipMemcpyDeviceToHost));
  return 0;
}
int pw_graph_contig_letters(pw_graph* g, uint8_t* out) {
  if (!g || !g->s.has_contigs) return fail("pw_graph_contig_letters before pw_graph_contigs");
  if (g->s.contig_total == 0) return 0;
  if (!out) return fail("pw_graph_contig_letters: null output");
  HIP_TRY(hipSetDevice(g->s.device));
  HIP_TRY(hipMemcpy(out, g->s.d_cletters.p, (size_t)g->s.contig_total, hipMemcpyDeviceToHost));
  return 0;
}
void* pw_graph_contig_letters_device(pw_graph* g) {
  if (!g || !g->s.has_contigs) { fail("pw_graph_contig_letters_device before pw_graph_contigs"); return nullptr; }
  return g->s.d_cletters.p;
}
void* pw_graph_contig_offsets_device(pw_graph* g) {
  if (!g || !g->s.has_contigs) { fail("pw_graph_contig_offsets_device before pw_graph_contigs"); return nullptr; }
  return g->s.d_coff.p;
}

// ---- the consensus stage (include/pw_consensus.h; kernels and stage sequences in pw_consensus.hip) ----
int pw_graph_place(pw_graph* g, void* stream) {
  if (!g) return fail("pw_graph_place: null graph");
  if (!g->s.built) return fail("pw_graph_place before pw_graph_build");
  HIP_TRY(hipSetDevice(g->s.device));
  HIP_TRY(pw::cons_place(g->s, g->c, (hipStream_t)stream));
  return 0;
}
int pw_graph_placements(pw_graph* g, pw_cons_place* out) {
  if (!g || !g->s.built || !g->c.placed) return fail("pw_graph_placements before pw_graph_place");
  if (g->s.n_reads == 0) return 0;
  if (!out) return fail("pw_graph_placements: null output");
  HIP_TRY(hipSetDevice(g->s.device));
  HIP_TRY(hipMemcpy(out, g->c.d_place.p, g->c.d_place.bytes((size_t)g->s.n_reads), hipMemcpyDeviceToHost));
  return 0;
}
void* pw_graph_placements_device(pw_graph* g) {
  if (!g || !g->s.built || !g->c.placed) { fail("pw_graph_placements_device before pw_graph_place"); return nullptr; }
  return g->c.d_place.p;
}

int pw_graph_consensus_layout(pw_graph* g, const uint8_t* letters_device, const int64_t* read_offs, const uint8_t* complement,
                              int complement_len, int32_t slack, double drift, void* stream) {
  if (!g) return fail("pw_graph_consensus_layout: null graph");
  if (!g->s.built) return fail("pw_graph_consensus_layout before pw_graph_build");
  if (slack < 0) return fail("pw_graph_consensus_layout: slack must not be negative");
  if (!std::isfinite(drift) || drift < 0 || drift > 1048576.) return fail("pw_graph_consensus_layout: drift must be finite and lie in 0 .. 2^20");
  if (complement && (complement_len < 1 || complement_len > 256)) return fail("pw_graph_consensus_layout: complement_len must be 1..256");
  const int64_t R = g->s.n_reads;
  if (R > 0 && !read_offs) return fail("pw_graph_consensus_layout: null read offsets");
  for (int64_t r = 0; r < R; r++)
    if (read_offs[r] < 0) return fail("pw_graph_consensus_layout: read " + std::to_string(r) + " has a negative offset");
  const hipStream_t st = (hipStream_t)stream;
  HIP_TRY(hipSetDevice(g->s.device));
  if (!g->c.placed) HIP_TRY(pw::cons_place(g->s, g->c, st));
  if (!g->s.has_contigs && pw_graph_contigs(g, letters_device, read_offs, complement, complement_len, stream) != 0) return -1;
  g->c.has_layout = false;
  bool any = false;                                          // a read of at least one letter: the frames are read from the letters
  for (int64_t r = 0; r < R && !any; r++) any = g->lens[r] > 0;
  if (any && !letters_device) return fail("pw_graph_consensus_layout: null letters");
  uint8_t table[256];
  for (int c = 0; c < 256; c++) table[c] = complement && c < complement_len ? complement[c] : (uint8_t)c;
  g->h_roff.assign(read_offs, read_offs + R);                // (the caller's array is consumed here)
  if (upload(fail, g->c.d_roff, g->h_roff.data(), (size_t)R, st) != 0) return -1;
  HIP_TRY(g->c.d_comp.ensure(256));
  HIP_TRY(hipMemcpy(g->c.d_comp.p, table, 256, hipMemcpyHostToDevice));
  bool too_long = false;
  HIP_TRY(pw::cons_layout(g->s, g->c, letters_device, slack, drift, &too_long, st));
  if (too_long) return fail("pw_graph_consensus_layout: a contig has 2^31 letters or more");
  g->r.round = 1; g->r.have = false;                         // (include/pw_rounds.h: a layout is round 1)
  return 0;
}
int64_t pw_graph_cons_num_tasks(pw_graph* g) {
  return g && g->s.built && g->c.has_layout ? g->c.n_tasks : fail("pw_graph_cons_num_tasks before pw_graph_consensus_layout");
}
int64_t pw_graph_cons_num_cols(pw_graph* g) {
  return g && g->s.built && g->c.has_layout ? g->c.n_cols : fail("pw_graph_cons_num_cols before pw_graph_consensus_layout");
}
int64_t pw_graph_cons_arena_bytes(pw_graph* g) {
  return g && g->s.built && g->c.has_layout ? g->c.arena_bytes : fail("pw_graph_cons_arena_bytes before pw_graph_consensus_layout");
}
int pw_graph_cons_cstart(pw_graph* g, int64_t* out) {
  if (!g || !g->s.built || !g->c.has_layout) return fail("pw_graph_cons_cstart before pw_graph_consensus_layout");
  if (!out) return fail("pw_graph_cons_cstart: null output");
  HIP_TRY(hipSetDevice(g->s.device));
  HIP_TRY(hipMemcpy(out, g->c.d_cstart.p, g->c.d_cstart.bytes((size_t)g->s.n_unitigs + 1), hipMemcpyDeviceToHost));
  return 0;
}
int pw_graph_cons_tasks(pw_graph* g, pw_cons_task* out) {
  if (!g || !g->s.built || !g->c.has_layout) return fail("pw_graph_cons_tasks before pw_graph_consensus_layout");
  if (g->c.n_tasks == 0) return 0;
  if (!out) return fail("pw_graph_cons_tasks: null output");
  HIP_TRY(hipSetDevice(g->s.device));
  HIP_TRY(hipMemcpy(out, g->c.d_tasks.p, g->c.d_tasks.bytes((size_t)g->c.n_tasks), hipMemcpyDeviceToHost));
  return 0;
}
void* pw_graph_cons_cstart_device(pw_graph* g) {
  if (!g || !g->s.built || !g->c.has_layout) { fail("pw_graph_cons_cstart_device before pw_graph_consensus_layout"); return nullptr; }
  return g->c.d_cstart.p;
}
void* pw_graph_cons_tasks_device(pw_graph* g) {
  if (!g || !g->s.built || !g->c.has_layout) { fail("pw_graph_cons_tasks_device before pw_graph_consensus_layout"); return nullptr; }
  return g->c.d_tasks.p;
}
void* pw_graph_cons_arena_device(pw_graph* g) {
  if (!g || !g->s.built || !g->c.has_layout) { fail("pw_graph_cons_arena_device before pw_graph_consensus_layout"); return nullptr; }
  return g->c.d_arena.p;
}

// ---- the later rounds of the consensus (include/pw_rounds.h; kernels and stage sequences in pw_rounds.hip) ----
int pw_graph_consensus_relayout(pw_graph* g, const uint8_t* polished_device, const uint64_t* polished_offsets_device,
                                const uint64_t* colmap_device, const uint8_t* letters_device, const int64_t* read_offs,
                                const uint8_t* complement, int complement_len, int32_t slack, double drift, void* stream) {
  if (!g) return fail("pw_graph_consensus_relayout: null graph");
  if (!g->s.built || !g->c.has_layout) return fail("pw_graph_consensus_relayout before pw_graph_consensus_layout");
  if (slack < 0) return fail("pw_graph_consensus_relayout: slack must not be negative");
  if (!std::isfinite(drift) || drift < 0 || drift > 1048576.) return fail("pw_graph_consensus_relayout: drift must be finite and lie in 0 .. 2^20");
  if (complement && (complement_len < 1 || complement_len > 256)) return fail("pw_graph_consensus_relayout: complement_len must be 1..256");
  if (!polished_offsets_device || !colmap_device) return fail("pw_graph_consensus_relayout: null offsets or colmap");
  if (g->c.n_cols > 0 && !polished_device) return fail("pw_graph_consensus_relayout: null polished letters");
  const int64_t R = g->s.n_reads;
  if (R > 0 && !read_offs) return fail("pw_graph_consensus_relayout: null read offsets");
  for (int64_t r = 0; r < R; r++)
    if (read_offs[r] < 0) return fail("pw_graph_consensus_relayout: read " + std::to_string(r) + " has a negative offset");
  bool any = false;                                          // a read of at least one letter: the frames are read from the letters
  for (int64_t r = 0; r < R && !any; r++) any = g->lens[r] > 0;
  if (any && !letters_device) return fail("pw_graph_consensus_relayout: null letters");
  const hipStream_t st = (hipStream_t)stream;
  HIP_TRY(hipSetDevice(g->s.device));
  uint8_t table[256];
  for (int c = 0; c < 256; c++) table[c] = complement && c < complement_len ? complement[c] : (uint8_t)c;
  g->h_roff.assign(read_offs, read_offs + R);                // (the caller's array is consumed here)
  if (upload(fail, g->c.d_roff, g->h_roff.data(), (size_t)R, st) != 0) return -1;
  HIP_TRY(g->c.d_comp.ensure(256));
  HIP_TRY(hipMemcpy(g->c.d_comp.p, table, 256, hipMemcpyHostToDevice));
  int refused = 0;
  HIP_TRY(pw::round_relayout(g->s, g->c, g->r, polished_device, polished_offsets_device, colmap_device, letters_device, slack, drift, &refused,
                             st));
  if (refused == 1) return fail("pw_graph_consensus_relayout: a contig has 2^31 letters or more");
  if (refused) return fail("pw_graph_consensus_relayout: the polished offsets disagree with colmap about a contig's length");
  return 0;
}
int pw_graph_cons_round(pw_graph* g) {
  return g && g->s.built && g->c.has_layout ? g->r.round : fail("pw_graph_cons_round before pw_graph_consensus_layout");
}
int pw_graph_cons_positions(pw_graph* g, int64_t* out) {
  if (!g || !g->s.built || !g->c.has_layout) return fail("pw_graph_cons_positions before pw_graph_consensus_layout");
  if (g->s.n_reads == 0) return 0;
  if (!out) return fail("pw_graph_cons_positions: null output");
  HIP_TRY(hipSetDevice(g->s.device));
  if (!g->r.have) HIP_TRY(pw::round_init(g->s, g->c, g->r, nullptr));
  HIP_TRY(hipMemcpy(out, g->r.d_pos.p, g->r.d_pos.bytes((size_t)g->s.n_reads), hipMemcpyDeviceToHost));
  return 0;
}
int pw_graph_cons_lengths(pw_graph* g, int64_t* out) {
  if (!g || !g->s.built || !g->c.has_layout) return fail("pw_graph_cons_lengths before pw_graph_consensus_layout");
  if (g->s.n_unitigs == 0) return 0;
  if (!out) return fail("pw_graph_cons_lengths: null output");
  HIP_TRY(hipSetDevice(g->s.device));
  if (!g->r.have) HIP_TRY(pw::round_init(g->s, g->c, g->r, nullptr));
  HIP_TRY(hipMemcpy(out, g->r.d_len[g->r.cur].p, g->r.d_len[0].bytes((size_t)g->s.n_unitigs), hipMemcpyDeviceToHost));
  return 0;
}

int pw_batch_scores(pw_batch* b, int32_t k, double* out, int64_t n) {
  if (!(b->flags & PW_FLAG_DUMP_SCORES) || k < 0 || k >= b->n || !b->descs[k].solvable) return fail("no score plane");
  const pw::PairDesc& d = b->descs[k];
  const int64_t want = (int64_t)d.ndiag * d.h_pitch;
  if (n < want) return fail("score buffer too small");
  HIP_TRY(hipSetDevice(b->device));
  if (b->use_f64) {
    HIP_TRY(hipMemcpy(out, b->d_hdump.as<double>() + d.h_off, 8 * (size_t)want, hipMemcpyDeviceToHost));
    for (int64_t i = 0; i < want; i++) out[i] *= b->score_mul;          // (dyadic scaling on f64 as well: a power of two)
  } else {
    std::vector<int32_t> tmp((size_t)want);
    HIP_TRY(hipMemcpy(tmp.data(), b->d_hdump.as<int32_t>() + d.h_off, 4 * (size_t)want, hipMemcpyDeviceToHost));
    for (int64_t i = 0; i < want; i++) out[i] = (double)tmp[(size_t)i] * b->score_mul;
  }
  return 0;
}

int pw_batch_masks(pw_batch* b, int32_t k, uint8_t* out, int64_t n) {
  if (k < 0 || k >= b->n || !b->descs[k].solvable) return fail("no mask plane for this pair");
  if (pw_batch* sub = repaired_sub(b, k)) return pw_batch_masks(sub, 0, out, n);   // (the replacement's plane is the live one)
  const pw::PairDesc& d = b->descs[k];
  if (n < b->plans[k].cells) return fail("mask buffer too small");
  const uint64_t words = d.layout == 1 ? (uint64_t)pw::strip_count(d.X) * pw::strip_nkq(d.Y) * 64 * 4
                                       : (uint64_t)(d.nblocks + 1) * d.nl * d.bk;
  std::vector<uint32_t> plane((size_t)words);
  HIP_TRY(hipSetDevice(b->device));
  HIP_TRY(hipMemcpy(plane.data(), b->d_masks.p + d.mask_off, 4 * (size_t)words, hipMemcpyDeviceToHost));
  pw::mask_table(d, plane.data(), b->mode == pw::BANDED_MODE, out);
  return 0;
}

int pw_batch_table(pw_batch* b, int32_t k, double* out, int64_t n) {
  if (!(b->flags & PW_FLAG_DUMP_SCORES) || k < 0 || k >= b->n || !b->descs[k].solvable) return fail("no score plane");
  if (b->mode != pw::STD_MODE) return fail("pw_batch_table: standard mode only");
  const pw::PairDesc& d = b->descs[k];
  const int64_t want = (int64_t)(d.X + 1) * (d.Y + 1);
  if (n < want) return fail("table buffer too small");
  HIP_TRY(hipSetDevice(b->device));
  DeviceArray<double> dev;
  HIP_TRY(dev.ensure((size_t)want));
  const void* plane = b->use_f64 ? (const void*)(b->d_hdump.as<double>() + d.h_off) : (const void*)(b->d_hdump.as<int32_t>() + d.h_off);
  HIP_TRY(pw::launch_table_rowmajor(plane, b->use_f64, d.X, d.Y, d.h_pitch, b->score_mul, dev.p, nullptr));
  HIP_TRY(hipMemcpy(out, dev.p, dev.bytes((size_t)want), hipMemcpyDeviceToHost));
  return 0;
}

float pw_batch_fill_ms(pw_batch* b) {
  if (!b->fill_timed) return -1.f;
  float ms = -1.f;
  (void)hipSetDevice(b->device);
  if (hipEventSynchronize(b->ev_fill1.e) != hipSuccess) return -1.f;
  if (hipEventElapsedTime(&ms, b->ev_fill0.e, b->ev_fill1.e) != hipSuccess) return -1.f;
  return ms;
}

float pw_batch_trace_ms(pw_batch* b) {
  if (!b->trace_timed) return -1.f;
  float ms = -1.f;
  (void)hipSetDevice(b->device);
  if (hipEventSynchronize(b->ev_tr1.e) != hipSuccess) return -1.f;
  if (hipEventElapsedTime(&ms, b->ev_tr0.e, b->ev_tr1.e) != hipSuccess) return -1.f;
  return ms;
}

}  // extern "C"

// =================================================================================================
// The four drop-in functions (include/pwlib.h): one problem per dptable, solved as a batch of one.
// =================================================================================================
namespace {

const uint64_t kMagic = 0x70776c69622d6869ull;   // "pwlib-hi"

// Lives immediately in front of the row-pointer array T->cells points at.
struct Hidden {
  uint64_t magic;
  pw_batch* batch;
  dpcell* cell_slab;          // all rows, back to back (NULL for huge tables: lazy)
  dpcell* opt_row;            // lazy tables: the one row that holds the optimal cell
  bool lazy;
  alnchoice* choice_slab;     // materialised choices
  int64_t ncells;
  int L;
  int dmin_c;
  std::vector<alignment*>* alns;
};

Hidden* hidden_of(dptable* T) {
  if (!T || !T->cells) return nullptr;
  Hidden* h = (Hidden*)((char*)T->cells - sizeof(Hidden));
  return h->magic == kMagic ? h : nullptr;
}

int env_int(const char* name, int dflt) {
  const char* v = getenv(name);
  return (v && *v) ? atoi(v) : dflt;
}

}  // namespace

extern "C" {

int dptable_init(dptable* T) {
  if (!T || !T->prob || !T->prob->frame || !T->prob->scores) return -1;
  alnprob* prob = T->prob;
  alnframe* fr = prob->frame;
  const int X = fr->origin_range.j - fr->origin_range.i, Y = fr->mutant_range.j - fr->mutant_range.i;
  if (prob->mode != STD_MODE && prob->mode != BANDED_MODE) {
    printf("Panick in %s (%d): %s\n", "pwlib", __LINE__, "Shouldn't have happened!");   // pw.c:22-23 exits here
    return -1;
  }
  if (X < 0 || Y < 0) { fprintf(stderr, "pwlib: negative frame length\n"); return -1; }
  if (prob->max_new_mins > 0) {
    fprintf(stderr, "pwlib: max_new_mins > 0 is not supported (the reference reads uninitialised memory there)\n");
    return -1;
  }
  int type, dmin = 0, dmax = 0;
  if (prob->mode == STD_MODE) type = (int)prob->std_params->type;
  else { type = (int)prob->banded_params->type; dmin = prob->banded_params->dmin; dmax = prob->banded_params->dmax; }
  pw::Plan pl = pw::plan_problem((int)prob->mode, type, X, Y, dmin, dmax);
  if (prob->mode == BANDED_MODE) {
    if (pl.clamped) {   // _pw_internals.c:32-35: message on stdout, caller's struct updated
      printf("Band [%d, %d] exceeds table limits, reduced it to [%d, %d].\n", dmin, dmax, pl.dmin, pl.dmax);
      prob->banded_params->dmin = pl.dmin; prob->banded_params->dmax = pl.dmax;
    }
    if (pl.rc != 0) {
      if (type == B_GLOBAL && (X - Y > pl.dmax || X - Y < pl.dmin || (int64_t)pl.dmax * pl.dmin > 0))
        printf("End points not within band for global alignment!\n");            // :41
      else printf("Invalid band: [%d, %d]!\n", pl.dmin, pl.dmax);                // :47
      return -1;
    }
  }
  {  // the reference's -INT_MAX floor (pw_plan.h, reaches_reference_floor), as far as init can tell: it reads the frame
     // lengths only (the alphabet is the letters' to say), so here the gap scores; dptable_solve's planner adds the
     // substitution scores of one-diagonal bands and refuses there
    const double gstep = pw::floor_gap_step(prob->scores->gap_open_score, prob->scores->gap_extend_score);
    if (pw::reaches_reference_floor(pl.brule, false, gstep, 0.0, (int64_t)X + Y + 2)) {
      fprintf(stderr, "pwlib: (X + Y + 2) * -(ge + min(go, 0)) = %.17g reaches the reference's -INT_MAX floor of gap "
              "candidates and end cells (not reproduced); refusing\n", ((double)X + Y + 2) * gstep);
      return -1;
    }
  }
  if (pl.ndiag > (1 << 21)) {
    fprintf(stderr, "pwlib: %d diagonals exceed the widest GPU fill kernel (%d); refusing (no CPU fallback)\n",
            pl.ndiag, 1 << 21);
    return -1;
  }
  T->num_rows = pl.num_rows;
  T->row_lens = (int*)malloc(sizeof(int) * (size_t)std::max(pl.num_rows, 1));
  char* blk = (char*)malloc(sizeof(Hidden) + sizeof(dpcell*) * (size_t)std::max(pl.num_rows, 1));
  if (!T->row_lens || !blk) { fprintf(stderr, "pwlib: out of memory\n"); free(T->row_lens); free(blk); return -1; }
  Hidden* h = (Hidden*)blk;
  h->magic = kMagic; h->batch = nullptr; h->choice_slab = nullptr; h->L = 0; h->dmin_c = pl.dmin;
  h->alns = new std::vector<alignment*>();
  h->ncells = pl.cells;
  // Tables beyond 2^26 cells (1 GiB of dpcell) do not get their cells on the host: the row-pointer array is
  // there, rows are NULL, and dptable_solve allocates only the row of the optimal cell (what pw.py:272 reads).
  h->lazy = pl.cells > ((int64_t)1 << 26);
  h->opt_row = nullptr;
  h->cell_slab = h->lazy ? nullptr : (dpcell*)calloc((size_t)std::max<int64_t>(pl.cells, 1), sizeof(dpcell));   // all empty (:64-74)
  if (!h->lazy && !h->cell_slab) { fprintf(stderr, "pwlib: out of memory\n"); delete h->alns; free(T->row_lens); free(blk); return -1; }
  T->cells = (dpcell**)(blk + sizeof(Hidden));
  int64_t off = 0;
  for (int i = 0; i < pl.num_rows; i++) {
    const int len = prob->mode == STD_MODE ? Y + 1 : pw::plan_len(X, Y, pl.dmin + i);
    T->row_lens[i] = len;
    T->cells[i] = h->lazy ? nullptr : h->cell_slab + off;
    off += len;
  }
  return 0;
}

void dptable_free(dptable* T) {
  Hidden* h = hidden_of(T);
  if (!h) return;
  pw_batch_destroy(h->batch);
  for (alignment* a : *h->alns) { free(a->transcript); free(a); }
  delete h->alns;
  free(h->choice_slab);
  free(h->cell_slab);
  free(h->opt_row);
  h->magic = 0;
  free((char*)T->cells - sizeof(Hidden));
  free(T->row_lens);
  T->cells = NULL; T->row_lens = NULL; T->num_rows = -1;
}

intpair dptable_solve(dptable* T) {
  const intpair none = {-1, -1};
  Hidden* h = hidden_of(T);
  if (!h) { fprintf(stderr, "pwlib: dptable_solve on an uninitialised table\n"); return none; }
  alnprob* prob = T->prob;
  alnframe* fr = prob->frame;
  const int X = fr->origin_range.j - fr->origin_range.i, Y = fr->mutant_range.j - fr->mutant_range.i;
  if (T->num_rows <= 0) return none;
  // letters -> one byte each; the alphabet size is not part of the ABI: use the largest letter seen
  const size_t moff = ((size_t)X + 3) / 4 * 4;     // frames start on 4-byte boundaries
  std::vector<uint8_t> arena(moff + (size_t)Y + 16, 0);
  int maxlet = 0;
  for (int i = 0; i < X; i++) { const int c = fr->origin[fr->origin_range.i + i]; if (c < 0 || c > 255) { fprintf(stderr, "pwlib: letter %d out of range 0..255\n", c); return none; } arena[i] = (uint8_t)c; maxlet = std::max(maxlet, c); }
  for (int i = 0; i < Y; i++) { const int c = fr->mutant[fr->mutant_range.i + i]; if (c < 0 || c > 255) { fprintf(stderr, "pwlib: letter %d out of range 0..255\n", c); return none; } arena[moff + i] = (uint8_t)c; maxlet = std::max(maxlet, c); }
  const int L = maxlet + 1;
  std::vector<double> subst((size_t)L * L);
  for (int i = 0; i < L; i++) for (int j = 0; j < L; j++) subst[(size_t)i * L + j] = prob->scores->subst_scores[i][j];
  pw_scoring sc;
  sc.mode = (int)prob->mode;
  sc.type = prob->mode == STD_MODE ? (int)prob->std_params->type : (int)prob->banded_params->type;
  sc.alphabet_len = L; sc.subst = subst.data();
  sc.go = prob->scores->gap_open_score; sc.ge = prob->scores->gap_extend_score;
  pw_pair pr;
  pr.origin_off = 0; pr.mutant_off = (uint64_t)moff; pr.origin_len = X; pr.mutant_len = Y;
  pr.dmin = prob->mode == BANDED_MODE ? prob->banded_params->dmin : 0;
  pr.dmax = prob->mode == BANDED_MODE ? prob->banded_params->dmax : 0;
  const bool timing = env_int("PWLIB_TIMING", 0) != 0;
  auto now = []() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
  const double t_a = now();
  // the full table (host: 48 B per cell) is materialised for tables up to 2^24 cells; beyond that only the
  // optimal cell is (table_scores-style callers need PWLIB_NO_TABLE unset and a table that size)
  const bool want_table = prob->mode == STD_MODE && !env_int("PWLIB_NO_TABLE", 0) && h->ncells <= (1 << 24);
  if (h->batch) { pw_batch_destroy(h->batch); h->batch = nullptr; }
  h->batch = pw_batch_create(env_int("PWLIB_DEVICE", 0), &sc, 1, &pr, arena.size(), want_table ? PW_FLAG_DUMP_SCORES : 0);
  if (!h->batch) { fprintf(stderr, "pwlib: %s\n", pw_last_error()); return none; }
  pw_result res;
  if (pw_batch_upload_arena(h->batch, arena.data(), arena.size()) != 0 || pw_batch_solve(h->batch, nullptr) != 0 ||
      pw_batch_sync(h->batch, nullptr) != 0 || pw_batch_results(h->batch, &res) != 0) {
    fprintf(stderr, "pwlib: %s\n", pw_last_error());
    return none;
  }
  const double t_b = now();
  double t_plane = 0.0;
  // ---- materialise what the reference's callers read out of C memory ----
  free(h->choice_slab); h->choice_slab = nullptr;
  if (want_table) {
    // every cell's choices[0].score (Aligner.table_scores, pw.py:278-285): the table comes back row-major
    double* table = (double*)malloc(sizeof(double) * (size_t)h->ncells);
    h->choice_slab = (alnchoice*)malloc(sizeof(alnchoice) * (size_t)h->ncells);
    if (!table || !h->choice_slab) { fprintf(stderr, "pwlib: out of memory\n"); free(table); return none; }
    if (pw_batch_table(h->batch, 0, table, h->ncells) != 0) { fprintf(stderr, "pwlib: %s\n", pw_last_error()); free(table); return none; }
    t_plane = now() - t_b;
    const int mins_cd = prob->max_new_mins;
    // 48 bytes per cell of freshly allocated host memory: first touch and stores are spread over a few threads
    auto fill_cells = [&](int64_t c0, int64_t c1) {
      for (int64_t c = c0; c < c1; c++) {
        alnchoice* ch = &h->choice_slab[c];
        ch->op = 0; ch->score = table[c]; ch->base = NULL; ch->mins_cd = mins_cd; ch->cur_min = 0;
        h->cell_slab[c].num_choices = 1; h->cell_slab[c].choices = ch;
      }
    };
    const int nth = h->ncells >= (1 << 16) ? std::max(1, std::min(8, (int)std::thread::hardware_concurrency())) : 1;
    if (nth <= 1) fill_cells(0, h->ncells);
    else {
      std::vector<std::thread> th;
      const int64_t per = (h->ncells + nth - 1) / nth;
      for (int t = 0; t < nth; t++) {
        const int64_t c0 = t * per, c1 = std::min<int64_t>(h->ncells, c0 + per);
        if (c0 < c1) th.emplace_back(fill_cells, c0, c1);
      }
      for (auto& t : th) t.join();
    }
    free(table);
  } else if (res.opt_i >= 0 && res.opt_j >= 0) {
    if (h->lazy) {
      free(h->opt_row);
      h->opt_row = (dpcell*)calloc((size_t)T->row_lens[res.opt_i], sizeof(dpcell));
      if (!h->opt_row) { fprintf(stderr, "pwlib: out of memory\n"); return none; }
      T->cells[res.opt_i] = h->opt_row;
    }
    h->choice_slab = (alnchoice*)calloc(1, sizeof(alnchoice));
    if (!h->choice_slab) { fprintf(stderr, "pwlib: out of memory\n"); return none; }
    h->choice_slab->score = res.score; h->choice_slab->base = NULL; h->choice_slab->mins_cd = prob->max_new_mins;
    T->cells[res.opt_i][res.opt_j].num_choices = 1;
    T->cells[res.opt_i][res.opt_j].choices = h->choice_slab;
  }
  if (timing) fprintf(stderr, "pwlib timing: create+upload+solve+sync %.2f ms, materialise %.2f ms (score plane D2H %.2f ms)\n", t_b - t_a, now() - t_b, t_plane);
  intpair opt = {res.opt_i, res.opt_j};
  return opt;
}

}  // extern "C"

namespace {

// The end cell's score when no table holds it: the walk IS the reference's chain of base choices (the predecessor rule,
// pw_wave.h trace_walk), whose scores the reference builds forward from the start cell's B choice (score 0):
// M / S add subst[o][m] (_pw_internals.c:234), D / I add ge and then go unless the op before was the same (:268-278).
// Same operations in the same order as the reference: bit-exact in doubles.
double walk_score(const dptable* T, const char* tx, int x, int y) {
  const alnframe* fr = T->prob->frame;
  const alnscores* sc = T->prob->scores;
  double s = 0.0;
  char prev = 'B';
  for (const char* c = tx; *c; c++) {
    if (*c == 'M' || *c == 'S') {
      s = s + sc->subst_scores[fr->origin[fr->origin_range.i + x]][fr->mutant[fr->mutant_range.i + y]];
      x++; y++;
    } else {
      s = s + sc->gap_extend_score;
      if (*c != prev) s = s + sc->gap_open_score;
      if (*c == 'D') x++; else y++;
    }
    prev = (*c == 'S') ? 'M' : *c;
  }
  return s;
}

}  // namespace

extern "C" {

alignment* dptable_traceback(dptable* T, intpair end) {
  Hidden* h = hidden_of(T);
  if (!h || !h->batch) { fprintf(stderr, "pwlib: dptable_traceback before dptable_solve\n"); return NULL; }
  const int32_t ends[2] = {end.i, end.j};
  pw_result res;
  if (pw_batch_traceback_from(h->batch, ends, nullptr) != 0 || pw_batch_sync(h->batch, nullptr) != 0 ||
      pw_batch_results(h->batch, &res) != 0) {
    fprintf(stderr, "pwlib: %s\n", pw_last_error());
    return NULL;
  }
  if (!(res.status & PW_ST_TRACED)) return NULL;
  if (res.status & PW_ST_PANICK) {   // the reference exits the process here (pw.c:132-134)
    printf("Panick in %s (%d): %s\n", "pwlib", __LINE__, "Shouldn't have happened!");
    return NULL;
  }
  if (res.tx_len == 0) return NULL;  // empty transcript (pw.c:135-138)
  uint64_t off; int32_t cap;
  pw_batch_tx_slot(h->batch, 0, &off, &cap);
  std::vector<uint8_t> tx(pw_batch_transcripts_bytes(h->batch));
  if (pw_batch_transcripts(h->batch, tx.data()) != 0) { fprintf(stderr, "pwlib: %s\n", pw_last_error()); return NULL; }
  alignment* a = (alignment*)malloc(sizeof(alignment));
  a->transcript = (char*)malloc((size_t)res.tx_len + 1);
  memcpy(a->transcript, tx.data() + off + cap - res.tx_len, (size_t)res.tx_len);
  a->transcript[res.tx_len] = 0;
  a->origin_idx = res.origin_idx + T->prob->frame->origin_range.i;
  a->mutant_idx = res.mutant_idx + T->prob->frame->mutant_range.i;
  // score of the END cell given (pw.c:148): the solve score for the optimal cell, the materialised
  // table for any other cell (standard mode), otherwise unknown
  if (end.i == res.opt_i && end.j == res.opt_j) a->score = res.score;
  else if (T->cells[end.i] && T->cells[end.i][end.j].num_choices > 0) a->score = T->cells[end.i][end.j].choices[0].score;
  else a->score = walk_score(T, a->transcript, res.origin_idx, res.mutant_idx);
  h->alns->push_back(a);
  return a;
}

}  // extern "C"

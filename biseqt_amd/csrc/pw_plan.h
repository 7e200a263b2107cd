// pw_plan.h -- host-side planning of one alignment problem: the arithmetic of the reference's
// dptable_init (table dimensions, band clamp, feasibility: _pw_internals.c:8-62) plus the geometry the
// wavefront kernel needs (step range, steady-phase blocks, begin / end rules); and the rules that choose a batch's
// kernels (score analysis, the packed 16-bit admission, lane and per-pair layouts).  Pure C++, no HIP: shared by the
// product library and by the CPU lane emulator in tests/emu.
#ifndef PW_PLAN_H
#define PW_PLAN_H

#include <math.h>
#include <stdint.h>
#include <stdlib.h>

#include <algorithm>

#include "pw_model.h"
#include "pw_types.h"

namespace pw {

struct Plan {
  int rc;              // 0, or -1 exactly where the reference's dptable_init returns -1
  int clamped;         // the band was reduced to the table limits (_pw_internals.c:29-36)
  int dmin, dmax;      // band after the clamp (STD mode: -Y, X)
  int num_rows;        // dptable.num_rows: X + 1 (STD) or 1 + dmax - dmin (banded)
  int64_t cells;       // cells the reference allocates = the GCUPS denominator
  int ndiag;
  int s0, nblocks, steady_b0, steady_b1;
  int brule, endrule;
};

static inline int plan_len(int X, int Y, int d) {       // cells on diagonal d (_pw_internals.c:56)
  return 1 + (d > 0 ? 0 : d) + (X - d > Y ? Y : X - d);
}

// sum over d = dmin .. dmax of plan_len(X, Y, d) in closed form (dmin <= dmax, -Y <= dmin, dmax <= X): three
// arithmetic series -- the number of diagonals, min(d, 0) over the negative ones, min(X - d, Y) split at d = X - Y.
static inline int64_t plan_series(int64_t a, int64_t b) { return a > b ? 0 : (a + b) * (b - a + 1) / 2; }   // a + ... + b
static inline int64_t plan_band_cells(int X, int Y, int dmin, int dmax) {
  const int64_t n = (int64_t)dmax - dmin + 1;
  int64_t cells = n;
  cells += plan_series(dmin, dmax < -1 ? dmax : -1);                      // min(d, 0)
  const int64_t k = (int64_t)X - Y;                                       // X - d > Y  <=>  d < k
  const int64_t lo_end = dmax < k - 1 ? dmax : k - 1;                     // d in [dmin, lo_end]: min = Y
  if (lo_end >= dmin) cells += (lo_end - dmin + 1) * (int64_t)Y;
  const int64_t hi_beg = dmin > k ? dmin : k;                             // d in [hi_beg, dmax]: min = X - d
  if (hi_beg <= dmax) cells += (dmax - hi_beg + 1) * (int64_t)X - plan_series(hi_beg, dmax);
  return cells;
}

// Begin rule (_alnchoice_B, _pw_internals.c:161-209) and end rule (:303-414) of an alignment type.
static inline void plan_rules(int mode, int type, int* brule, int* endrule) {
  if (mode == STD_MODE) {
    *brule = (type == LOCAL || type == END_ANCHORED) ? BRULE_ANY
             : (type == OVERLAP || type == END_ANCHORED_OVERLAP) ? BRULE_EDGE : BRULE_ORIGIN;
    *endrule = (type == GLOBAL || type == END_ANCHORED || type == END_ANCHORED_OVERLAP) ? END_CORNER
               : (type == OVERLAP || type == START_ANCHORED_OVERLAP) ? END_STD_OVERLAP : END_STD_LOCAL;
  } else {
    *brule = type == B_LOCAL ? BRULE_ANY : type == B_OVERLAP ? BRULE_EDGE : BRULE_ORIGIN;
    *endrule = type == B_GLOBAL ? END_CORNER : type == B_OVERLAP ? END_BANDED_OVERLAP : END_BANDED_LOCAL;
  }
}

static inline Plan plan_problem(int mode, int type, int X, int Y, int dmin_in, int dmax_in) {
  Plan p;
  p.rc = 0; p.clamped = 0; p.cells = 0; p.ndiag = 0;
  p.s0 = 0; p.nblocks = 0; p.steady_b0 = 0; p.steady_b1 = 0;
  plan_rules(mode, type, &p.brule, &p.endrule);
  if (mode == STD_MODE) {
    p.dmin = -Y; p.dmax = X; p.num_rows = X + 1;
    p.cells = (int64_t)(X + 1) * (int64_t)(Y + 1);
  } else {
    int dmin = dmin_in, dmax = dmax_in;
    if (dmax > X || dmin < -Y) {                       // :29-36
      dmax = dmax > X ? X : dmax;
      dmin = dmin < -Y ? -Y : dmin;
      p.clamped = 1;
    }
    p.dmin = dmin; p.dmax = dmax;
    const int dend = X - Y;
    if (type == B_GLOBAL && (dend > dmax || dend < dmin || (int64_t)dmax * dmin > 0)) { p.rc = -1; return p; }  // :38-43
    p.num_rows = 1 + dmax - dmin;
    if (p.num_rows < 0) { p.rc = -1; return p; }       // :46-49
    if (p.num_rows == 0) { p.ndiag = 0; return p; }    // an empty table: the reference goes on with zero rows
    p.cells = plan_band_cells(X, Y, dmin, dmax);
  }
  p.ndiag = 1 + p.dmax - p.dmin;
  // first / last anti-diagonal that holds an in-band cell
  const int amin = p.dmin > 0 ? p.dmin : (p.dmax < 0 ? -p.dmax : 0);          // min |d|
  int s_last = 0, tf_max = 0, tl_min = 0x7fffffff;
  p.s0 = amin - (((amin - p.dmin) % 2 + 2) % 2);        // s0 == dmin (mod 2), s0 <= amin
  // |d| is maximal at a band end; tlast(d) = |d| + 2 (len(d) - 1) is piecewise linear in d with
  // breakpoints at 0 and X - Y, so its extrema sit at the band ends or at those breakpoints.
  const int cand[4] = {p.dmin, p.dmax, 0, X - Y};
  for (int k = 0; k < 4; k++) {
    const int d = cand[k];
    if (d < p.dmin || d > p.dmax) continue;
    const int ad = d < 0 ? -d : d;
    const int tl = ad + 2 * (plan_len(X, Y, d) - 1);
    if (tl > s_last) s_last = tl;
    if (ad - p.s0 > tf_max) tf_max = ad - p.s0;
    if (tl - p.s0 < tl_min) tl_min = tl - p.s0;
  }
  const int nsteps = s_last - p.s0 + 1;
  p.nblocks = (nsteps + 15) / 16;
  // block b is steady iff every in-band diagonal holds its FIRST cell strictly before step 16 b (first
  // cells carry the begin rule and have missing predecessors) and none has ended before step 16 b + 15
  p.steady_b0 = tf_max / 16 + 1;
  p.steady_b1 = (tl_min + 1) / 16;
  if (p.steady_b1 > p.nblocks) p.steady_b1 = p.nblocks;
  if (p.steady_b1 < p.steady_b0) p.steady_b1 = p.steady_b0;
  return p;
}

// ---- kernel selection: the pure part of the batch planner (pwlib_api.cpp, batch_plan) ----

// Fill-kernel variants (template switches of WaveFill, pw_wave.h).
enum { VAR_FAST_ANY_TRACK = 0,  // begin anywhere + per-diagonal best: LOCAL, B_LOCAL (END_ANCHORED rides along)
       VAR_FAST_TRACK = 1,      // begin at origin/edges + per-diagonal best: START_ANCHORED
       VAR_FAST = 2,            // begin at origin/edges, end on the table edge: GLOBAL, *OVERLAP, B_GLOBAL, B_OVERLAP
       VAR_GENERIC = 3,         // substitution matrix / go > 0 / score-plane dump: everything at run time
       VAR_FAST16 = 4 };        // packed 16-bit (LOCAL / B_LOCAL, B_OVERLAP, B_GLOBAL), several pairs per wavefront (launch_fill16)

static const int kSupportedBK[] = {2, 4, 8, 16, 32};             // diagonals per lane of the 32-bit / f64 kernels
static const int kNumSupportedBK = 5;
static const int kNarrowMwBK[] = {4, 8, 16}, kWideMwBK[] = {8, 16, 32};   // ... their workgroups: a few pairs / wide bands
static const int kPackedBK[] = {4, 8, 12, 16, 20, 24, 28, 32};   // diagonals per lane of the packed 16-bit kernels
static const int kNumPackedBK = 8;
static const int kMaxWavesPerPair = 8;                           // wavefronts of a workgroup that takes one pair
// tiled single-pair kernel (K2b): tiles of kTileCentralDiags diagonals + ghosts, time blocks of kTileBlocks blocks
// (geometry overridable at build time for tuning runs: -DPW_TILE_LANES= -DPW_TILE_BK= -DPW_TILE_GHOST= -DPW_TILE_BLOCKS=)
#ifndef PW_TILE_LANES
#define PW_TILE_LANES 256
#endif
#ifndef PW_TILE_BK
#define PW_TILE_BK 2
#endif
#ifndef PW_TILE_GHOST
#define PW_TILE_GHOST 64
#endif
#ifndef PW_TILE_BLOCKS
#define PW_TILE_BLOCKS (PW_TILE_GHOST * PW_TILE_BK / 16)
#endif
static const int kTileBKHost = PW_TILE_BK, kTileCentralLanes = PW_TILE_LANES - 2 * PW_TILE_GHOST, kTileBlocks = PW_TILE_BLOCKS;

// The fewest diagonals per lane among `bk` (ascending) with which `waves` wavefronts cover ndiag diagonals, or 0.
static inline int narrowest_bk(int ndiag, const int* bk, int n, int waves) {
  for (int i = 0; i < n; i++) if ((int64_t)64 * waves * bk[i] >= ndiag) return bk[i];
  return 0;
}

static inline bool plan_integral(double v) { return v == floor(v) && fabs(v) < 1e9; }

// What the planner needs to know of a scoring.  Every score value below is of the scores the kernels hold: times
// 2^scale_shift.
struct ScoreSummary {
  bool finite;            // every substitution score is finite
  bool integral;          // every score (go, ge too) is an integer
  bool simple;            // match / mismatch scoring: subst[i][j] = i == j ? mt : mm
  int scale_shift;
  double mt, mm;          // subst[0][0], subst[0][1] (L = 1: the match score both)
  double smin, smax;      // the worst and the best substitution (any may be: the API accepts mismatch > match, and a matrix)
  double maxabs;          // the largest |score| of subst, go, ge, go + ge
};

// Dyadic scaling (allow_dyadic): scores that are all multiples of 2^-k (k <= 10; e.g. config 5's extension scores
// 0.25 / -1 / 0 / -1, reference experiments/blot_stats.py:365-372) are held times 2^k and run on the integer kernels.  Every
// partial sum of such scores is exact in the reference's doubles (the planner keeps them far below 2^53 / 2^k), scaling by a
// power of two preserves every comparison and tie, and the kernels report value * 2^-k, which is exact again: bit-identical
// results, no f64 kernel.  The caller scales its own copies of the scores by 2^scale_shift.
static inline ScoreSummary summarise_scores(int L, const double* subst, double go, double ge, bool allow_dyadic) {
  ScoreSummary s{};                                        // (all zero: what a non-finite scoring leaves)
  s.finite = true; s.simple = true;
  s.integral = plan_integral(go) && plan_integral(ge);
  s.maxabs = std::max(fabs(go), std::max(fabs(ge), fabs(go + ge)));
  const double mt0 = subst[0], mm0 = L > 1 ? subst[1] : subst[0];
  for (int i = 0; i < L * L; i++) {
    const double v = subst[i];
    if (!(v == v) || fabs(v) > 1e300) { s.finite = false; return s; }
    s.integral = s.integral && plan_integral(v);
    s.maxabs = std::max(s.maxabs, fabs(v));
    if (v != (i / L == i % L ? mt0 : mm0)) s.simple = false;
  }
  if (!s.integral && allow_dyadic && s.maxabs < 1e6) {
    for (int sh = 1; sh <= 10 && !s.scale_shift; sh++) {
      const double f = (double)(1 << sh);
      bool ok = plan_integral(go * f) && plan_integral(ge * f);
      for (int i = 0; ok && i < L * L; i++) ok = plan_integral(subst[i] * f);
      if (ok) s.scale_shift = sh;
    }
    if (s.scale_shift) { s.integral = true; s.maxabs *= (double)(1 << s.scale_shift); }
  }
  const double f = (double)(1 << s.scale_shift);
  s.mt = mt0 * f; s.mm = mm0 * f;
  s.smin = s.smax = s.mt;
  for (int i = 0; i < L * L; i++) { s.smax = std::max(s.smax, subst[i] * f); s.smin = std::min(s.smin, subst[i] * f); }
  if (s.simple) { s.smax = std::max(s.mt, s.mm); s.smin = std::min(s.mt, s.mm); }      // (L = 1: the mismatch score never occurs)
  return s;
}

// The reference starts every gap candidate's maximum at -INT_MAX (_pw_internals.c:267) and so does the end-cell search of
// OVERLAP / B_OVERLAP (:320, :381): a candidate at or below it is floored there (with choices[0] as its base), a cell at
// or below it is never an end cell.  The kernels do not reproduce that floor, so the planner refuses the problems that could
// reach it.  What decides it is the lowest cell MAXIMUM, not the lowest path: a gap candidate out of cell c is at least
// max(c) + ge + min(go, 0), and an end cell's score is its maximum.  Every cell that holds a choice has one out of a
// predecessor that holds one (or the begin candidate 0), so max(x, y) >= -(x + y) * h, where h bounds the loss per unit of
// x + y over the steps that are always there:
//   * standard mode, and bands of 2+ diagonals: every cell but the first has a gap predecessor in the table / band (the
//     band holds diagonal d - 1 or d + 1), so h = gap_step = max(0, -(ge + min(go, 0))) -- the substitution scores do not
//     matter, however low;
//   * a band of one diagonal: substitutions only, h = max(gap_step, -smin).
// A candidate or end cell is at most X + Y + 1 steps from (0, 0): maxspan * h < INT_MAX (maxspan = X + Y + 2, scores in the
// CALLER's units, not times 2^scale_shift) keeps every one above the floor.  Begin-anywhere rules (LOCAL, END_ANCHORED,
// B_LOCAL) are never affected: every cell holds the begin candidate 0, so a floored candidate is never kept.
static inline double floor_gap_step(double go, double ge) { return std::max(0.0, -(ge + std::min(go, 0.0))); }
static inline bool reaches_reference_floor(int brule, bool one_diagonal, double gap_step, double smin, int64_t maxspan) {
  const double h = one_diagonal ? std::max(gap_step, -smin) : gap_step;
  return brule != BRULE_ANY && (double)maxspan * h >= 2147483647.0;
}

// The planner's environment knobs (tuning and A/B runs), read once per batch (pwlib_api.cpp, plan_knobs).  The defaults
// are the planner's own choices; the CPU lane emulator and the tests use them.
struct PlanKnobs {
  bool no_dyadic = false;           // PWLIB_NO_DYADIC=1: fractional scores stay as given (f64 kernels)
  int latency_mode = -1;            // PWLIB_LATENCY_MODE=0 / 1: instead of "at most 256 solvable pairs"
  bool no_packed_mat = false;       // PWLIB_NO_PACKED_MAT=1: no matrix form of the packed kernels
  bool no_packed_anchored = false;  // PWLIB_NO_PACKED_ANCHORED=1: no packed rules 4, 5
  bool no_packed_overlap = false;   // PWLIB_NO_PACKED_OVERLAP=1: no packed rules 1, 2, 5
  bool no_packed_mw = false;        // PWLIB_NO_PACKED_MW=1: no packed workgroups
  bool no_strip = false;            // PWLIB_NO_STRIP=1: no strip pipeline
  bool no_small_strip = false;      // PWLIB_NO_SMALL_STRIP=1: the strips only for pairs wider than a workgroup
  bool strip_no_byte_rows = false;  // PWLIB_STRIP_NO_BYTE_ROWS=1: the strips take match / mismatch scores only
  bool no_small_tiled = false;      // PWLIB_NO_SMALL_TILED=1: the tiles only for pairs wider than a workgroup
  bool mw_wide_lanes = false;       // PWLIB_MW_WIDE_LANES=1: many wide pairs on 32 diagonals per lane
  int simple_as_matrix = -1;        // PWLIB_SIMPLE_AS_MATRIX=0 / 1: match / mismatch in the packed matrix form never / always
  bool no_scaled16 = false;         // PWLIB_NO_SCALED16=1: no scores-times-4 form (rule 3)
  bool ramp_blocks = false;         // PWLIB_RAMP_BLOCKS=1: blocks in which diagonals start or end keep their own bodies (ramp_free)
  bool stamp_group1 = false;        // PWLIB_STAMP_GROUP=1: the running best stamped per block, never per four (stamp_group)
  bool no_lds_feed = false;         // PWLIB_LDS_FEED=0: the grouped kernel keeps its edge-lane feeders (lds_feed)
  bool no_pair_keys = false;        // PWLIB_PAIR_KEYS=0: one running-best key per cell, the kernel k_fill16l (pair_keys)
  bool no_lds_exchange = false;     // PWLIB_LDS_EXCHANGE=0: the offers cross lanes by DPP moves, the kernel k_fill16p (lds_exchange)
  bool packed_bk_forced = false;   // PWLIB_PACKED_BK="<bk>" or "<bk>s": the packed lane width (s: lane packing)
  int packed_bk = 0;
  bool packed_bk_seg = false;
};

// The packed 16-bit body's RULE (pw_wave.h, WaveFill16) for a begin / end rule, -1 where there is none: 0 begin anywhere,
// end at the best cell (LOCAL, B_LOCAL); 1 the overlap begin or end (B_OVERLAP, OVERLAP, START_ANCHORED_OVERLAP --
// begins at (0, 0) --, END_ANCHORED_OVERLAP -- ends at (X, Y) --: begin and end rule read at run time); 2 begin at (0, 0),
// end at (X, Y) (GLOBAL on the band [-Y, X], B_GLOBAL); 4 END_ANCHORED (begin anywhere, the captured last cell of one
// diagonal, nothing tracked); 5 START_ANCHORED (begin at (0, 0), end at the first best cell, which must beat 0).  Rule 3 is
// rule 0 with every score times 4 (admit_packed).
static inline int packed_rule(int brule, int endrule) {
  const bool local_end = endrule == END_STD_LOCAL || endrule == END_BANDED_LOCAL;
  const bool overlap_end = endrule == END_BANDED_OVERLAP || endrule == END_STD_OVERLAP;
  if (brule == BRULE_ANY) return local_end ? 0 : endrule == END_CORNER ? 4 : -1;
  if (brule == BRULE_ORIGIN) return endrule == END_STD_LOCAL ? 5 : endrule == END_STD_OVERLAP ? 1 : endrule == END_CORNER ? 2 : -1;
  if (brule == BRULE_EDGE) return overlap_end || endrule == END_CORNER ? 1 : -1;
  return -1;
}

// An integer substitution matrix over at most 4 letters goes into the packed kernels as rows of bytes (WaveFill16<.., MAT>,
// _alnchoice_M reads subst_scores[o][m], _pw_internals.c:217-245): bytes subst - min, at most 127 (times 4 in the
// scores-times-4 form, x4), and min <= 0 -- letters outside a sequence score the minimum and must not lift a cell that has
// not started.  Match / mismatch scores over 2 .. 4 letters are such a matrix too.
static inline bool packed_matrix_bytes_ok(const ScoreSummary& s, int L, bool x4) {
  return L >= 2 && L <= 4 && s.integral && s.smin <= 0 && (x4 ? 4 : 1) * (s.smax - s.smin) <= 127;
}

// ... the rows themselves: rows[o] holds scale * (subst[o][m] - min) in byte m = 0 .. 3 from the low byte up (scale 4 in
// the scores-times-4 form), *bias = scale * -min; letters beyond L never occur.  `subst` as the kernels hold it.
static inline void packed_matrix_rows(const double* subst, int L, bool x4, uint32_t rows[4], int32_t* bias) {
  const int scale = x4 ? 4 : 1;
  double smin = subst[0];
  for (int i = 0; i < L * L; i++) smin = std::min(smin, subst[i]);
  for (int o = 0; o < 4; o++) {
    uint32_t row = 0;
    for (int m = 0; m < 4; m++)
      if (o < L && m < L) row |= (uint32_t)(scale * (int)(subst[(size_t)o * L + m] - smin)) << (8 * m);
    rows[o] = row;
  }
  *bias = scale * (int)(-smin);
}

struct PackedAdmission {
  int rule = -1;               // the body's RULE; -1: not admitted
  bool force_matrix = false;   // match / mismatch scores that must take the matrix form
  bool matrix_ok = false;      // ... that may take it (where it measured faster: packed_matrix_form)
  bool x4 = false;             // rule 0 may hold every score times 4 (rule 3) -- in the matrix form only if x4_matrix too
  bool x4_matrix = false;
};

// Admission of a batch to the packed 16-bit body: `rule` from packed_rule (-1: none, or a kernel variant without it), the
// scores as the kernels hold them, the batch's largest min(X, Y), band (diagonals) and X + Y + 2.  Each bound keeps one
// running value of the body inside the part of the 16-bit range its scheme leaves it.
static inline PackedAdmission admit_packed(int rule, const ScoreSummary& s, int L, double go, double ge, int64_t maxmin,
                                           int maxnd, int64_t maxspan, const PlanKnobs& kn) {
  PackedAdmission a;
  const bool bytes = !kn.no_packed_mat && packed_matrix_bytes_ok(s, L, false);
  if (rule < 0 || (!s.simple && (rule > 2 || !bytes))) return a;       // (the matrix form: rules 0 .. 3)
  // The packed kernels keep cells that have not started (and cells beyond a diagonal's end) at a shallow 16-bit sentinel,
  // pinned from below by a maximum; what keeps them from creeping UP is that letters outside a sequence "match nothing" and
  // that scores nothing -- true only while the mismatch score (what the plain form gives such letters; with one letter the
  // match score) is <= 0.  With mismatch > 0, which the API accepts, a diagonal that waits ~1400 steps for its first cell
  // starts from a positive phantom score (found by the fuzz on a 3673-diagonal band, scores 1 / 6 / -5 / -2: a wrong end
  // cell, and the walk from it left the mask plane).  Such scores take the matrix form where it applies (its off-table
  // letters score the matrix MINIMUM, required <= 0) and the 32-bit kernels otherwise.
  if (s.simple && s.mm > 0) {
    if (rule > 2 || !bytes) return a;
    a.force_matrix = true;
  }
  if (rule >= 4 && kn.no_packed_anchored) return a;
  const double best = (double)maxmin * std::max(0.0, s.smax);      // no cell scores above min(X, Y) best substitutions
  bool fits;
  // rules 0, 4 (scores >= 0): the best score stays below the 8192 of the shallow sentinel -- the first diagonal above the
  // band is computed like any other and its offer into the band is lowered by only that much, so no score, in or out of the
  // band, may reach it (regression: test_band_edge_never_leaks_long_pairs)
  if (rule == 0 || rule == 4) fits = best <= 8000;
  else {
    // rules 1, 2, 5: scores go negative and the sentinel is -24000.  The lowest real score stays above the values derived
    // from the sentinel (<= -24000 + 100): the lowest in-band cell is the straight run down its own diagonal from the table
    // edge (min(X, Y) substitutions) -- for B_GLOBAL after the gap run from (0, 0) to that diagonal
    const double lowest = (double)maxmin * std::max(0.0, -s.smin) + fabs(go) + fabs(ge) * (maxnd + 2);
    fits = lowest <= 23000 && !kn.no_packed_overlap;
    // ... and the highest one below int16's top -- rule 5 below 8192, the range of its running-best key
    fits = fits && best <= (rule == 5 ? 8000 : 30000);
  }
  // every score within +-100: one step moves a running value by at most that much, the margin the bounds above leave;
  // X + Y + 2 < 32000: steps are counted in signed 16 bits; go, ge <= 0: gaps only lower a score (the bounds above count
  // substitutions only)
  if (!fits || s.maxabs > 100 || maxspan >= 32000 || go > 0 || ge > 0) return a;
  a.rule = rule;
  a.matrix_ok = s.simple && rule <= 2 && bytes;
  // rule 3 holds every score times 4: the best score times 4 stays below the same 8192
  a.x4 = rule == 0 && best <= 2047 && !kn.no_scaled16;
  a.x4_matrix = packed_matrix_bytes_ok(s, L, true);
  return a;
}

// ramp_free: whether the packed body that runs one loop per kind of block (WaveFill16::SPLIT: the matrix form of rule 0 and
// of its scores-times-4 twin, rule 3) may run the blocks in which diagonals start or end on the STEADY body, which neither
// withholds the begin candidate from cells that have not started nor masks cells beyond a diagonal's end out of the running
// best.  `rule` and `matrix` as the batch runs (PackedAdmission, packed_matrix_form); go, ge, smin as the kernels hold them
// (integers; admit_packed already requires go <= 0, ge <= 0, packed_matrix_bytes_ok smin <= 0).  True iff
//     ge < 0,   ge + go < 0,   smin < 0.
// Start ramp.  The in-band slots start at H = 0 instead of the sentinel.  A virtual cell (one with a negative coordinate)
// has only virtual predecessors.  Letters outside a sequence score smin <= 0 and every gap offer is H + ge (+ go) < H, so by
// induction a virtual cell's candidates are <= 0 and, with the begin candidate, it stays EXACTLY 0 -- what such a cell
// counts as in the running best today.  A real cell sees from a virtual predecessor a diagonal candidate 0 + smin <= 0,
// which cannot lift it above the begin candidate it holds anyway (the packed plane stores no M bit), and a gap offer
// ge + go < 0, which never equals its own H >= 0: no D or I bit is set that the sentinel would not have set.  Every in-band
// diagonal predecessor is >= 0 from block 0 on, which is all the steady body's saturating subtract asks, and 0 lies inside
// the [0, 8191] the body's 32-bit diagonal add requires of H (pw_wave.h, cellpair).
// End ramp.  Cells beyond a diagonal's end stay in the running best.  The letters they read are outside a sequence and
// score as such: the steady loop then replaces the feed letters outside the sequences in EVERY block that is fed one, because a letter
// beyond a sequence's end is fed long before the band reads it, in blocks that are still steady (pw_wave.h, RAMPF).  So
// each of their candidates is a predecessor's H plus smin < 0 or
// plus at most ge < 0, or the begin candidate 0: by induction over the steps such a cell holds at most max(0, G - 1), G the
// best in-table score.  If G > 0 no such cell reaches G: a slot whose diagonal holds an in-table G cell keeps that cell (the
// key's stamp moves only on a strict rise of the score), a slot that reports a cell beyond its end reports less than G and
// loses the end-cell reduction.  If G = 0 no score rises at all, no stamp is written and every diagonal reports its first
// cell as before.  The tie nibbles of such cells go where they went before: mask slots no walk visits.
static inline bool ramp_free(int rule, bool matrix, double go, double ge, double smin, const PlanKnobs& kn) {
  return (rule == 0 || rule == 3) && matrix && !kn.ramp_blocks && ge < 0 && ge + go < 0 && smin < 0;
}

// stamp_group: the blocks per stamp of the running best (pw_wave.h, WaveFill16, GRP).  4 -- the grouped kernel k_fill16g --
// exactly for packed rule 3, matrix form, 8 diagonals per lane, one pair per wavefront (no lane packing), one wavefront per
// pair, with ramp_free (the kernel holds the steady loop alone); 1 otherwise, and under PWLIB_STAMP_GROUP=1.  No admission
// bound of its own: the grouped key 8 (4 score) + (31 - cell) needs 4 score <= 8188, and rule 3 is admitted only with
// min(X, Y) max(subst) <= 2047 (admit_packed, x4), which is that bound.
static inline int stamp_group(int rule, bool matrix, int bk, bool seg, int nw, bool ramp_free_on, const PlanKnobs& kn) {
  return (rule == 3 && matrix && bk == 8 && !seg && nw == 1 && ramp_free_on && !kn.stamp_group1) ? 4 : 1;
}

// lds_feed: whether the grouped kernel reads the matrix rows and selector dwords of its letters from two rings in LDS
// (pw_wave.h, WaveFill16, LDSF: the kernel k_fill16l) instead of passing them through the lanes from scalar feeders.  Exactly
// where stamp_group says 4 -- the same form, ramp_free among its conditions: the rings hold every letter outside a sequence
// already replaced -- and not under PWLIB_LDS_FEED=0, which keeps k_fill16g.  No admission bound of its own: the rings hold
// what the feeders deliver, letter for letter.
static inline bool lds_feed(int stamp_group_, const PlanKnobs& kn) { return stamp_group_ == 4 && !kn.no_lds_feed; }

// pair_keys: whether the kernel that reads its letters from LDS keeps ONE running-best key per two consecutive cells of a slot
// and finds out in the end-cell search which of the two held the best (pw_wave.h, WaveFill16, PAIRK: the kernel k_fill16p).
// Exactly where lds_feed says so, and only with ge < 0, go <= 0 and no substitution score equal to 0 (`subst` as the kernels
// hold it, L x L): then the best cell of the table kept the diagonal move alone on a positive substitution score, which is
// what tells the second cell of a pair from the first (the argument is at WaveFill16::pairk).  Not under PWLIB_PAIR_KEYS=0,
// which keeps k_fill16l.
static inline bool pair_keys(bool lds_feed_, const double* subst, int L, double go, double ge, const PlanKnobs& kn) {
  if (!lds_feed_ || kn.no_pair_keys || !(ge < 0) || !(go <= 0)) return false;
  for (int i = 0; i < L * L; i++)
    if (subst[i] == 0) return false;
  return true;
}

// lds_exchange: whether that kernel hands the two offers that cross lanes on through LDS instead of a DPP move and a
// v_alignbit each (pw_wave.h, WaveFill16, XLDS: the kernel k_fill16x).  Exactly where pair_keys says so: the values are the
// same ones, bit for bit, so there is no bound of its own.  Not under PWLIB_LDS_EXCHANGE=0, which keeps k_fill16p.
static inline bool lds_exchange(bool pair_keys_, const PlanKnobs& kn) { return pair_keys_ && !kn.no_lds_exchange; }

struct PackedLayout { int bk = 0, nl = 0, seg = 0, nw = 1; };   // bk = 0: none; seg: several pairs per wavefront

// The packed 16-bit body on a workgroup of up to 8 wavefronts per pair, as few diagonals per lane as 8 wavefronts allow.
static inline PackedLayout packed_workgroup_layout(int maxnd) {
  PackedLayout l;
  l.bk = narrowest_bk(maxnd, kPackedBK, kNumPackedBK, kMaxWavesPerPair);
  if (l.bk) { l.nw = (maxnd + 64 * l.bk - 1) / (64 * l.bk); l.nl = 64 * l.nw; }
  return l;
}

// The packed body's layout for bands one wavefront holds (maxnd <= 2048): diagonals per lane and pairs per wavefront.  One
// pair per wave keeps the pair descriptor in scalar registers (measured ~7 % cheaper per cell); several pairs per wave (lane
// packing) keep more of the 64 x BK diagonal slots busy.  Each layout is priced (pw_model.h): what a slot-step costs at that
// lane width (the wide lanes pay for their registers) / the share of busy slots x a factor for the last, partly filled round
// of wavefronts over the SIMDs.  Round 3 found config 4's overlap batches -- bands of 9 .. 111 diagonals, 20 000 pairs -- on
// 28 diagonals per lane (69 % of the slots busy, but 1250 wavefronts on 1024 SIMDs: 7.4 ms) where 8 per lane take 4.9 ms;
// with 50 000 pairs per batch 16 per lane win (profiles/round3_n_lane_width.txt).  Packing is taken when it is priced 5 %
// below one pair per wavefront.
static inline PackedLayout packed_lane_layout(int maxnd, int64_t sumnd, int nsolv, bool latency_mode, bool strips_win,
                                              const PlanKnobs& kn, const PlanModel& model) {
  const bool forced = kn.packed_bk_forced;
  const double meannd = (double)sumnd / nsolv;
  double cost1 = 1e300, costp = 1e300; int bk1 = 0, bkp = 0, nlp = 0;
  for (int i = 0; i < kNumPackedBK; i++) {
    const int bk = kPackedBK[i];
    if (forced && kn.packed_bk != bk) continue;
    const int nl = (maxnd + bk - 1) / bk;
    if (nl > 64) continue;
    if (!bk1) {                                                             // smallest BK that fits: one pair per wavefront
      bk1 = bk;
      cost1 = model.one_pair_discount * model.seg_slot_cost[i] * last_round_factor((double)nsolv) / (meannd / (64.0 * bk));
    }
    const int ppw = 64 / nl;
    const int64_t nwv = ((int64_t)nsolv + ppw - 1) / ppw;
    // (packing must leave at least one wavefront per SIMD: 20 000 pairs with a 21-diagonal band packed 64 to a wavefront are
    //  313 wavefronts with 12 cells per lane and step -- 0.69 ms against 0.41 ms for 10 to a wavefront)
    const bool enough = forced || nwv >= 1024;
    const double cp = model.seg_slot_cost[i] * last_round_factor((double)nwv) / ((double)ppw * meannd / (64.0 * bk));
    if (ppw >= 2 && enough && cp < costp - 1e-9) { costp = cp; bkp = bk; nlp = nl; }      // ties: the narrower lanes
  }
  const bool want_seg = bkp && (!bk1 || costp < 0.95 * cost1 || (forced && kn.packed_bk_seg));
  // pairs that fit one wavefront side by side at the narrowest lanes
  const int ppw1 = bk1 ? std::max(1, 64 / ((maxnd + bk1 - 1) / bk1)) : 1;
  PackedLayout l;
  if ((latency_mode || nsolv < 1024 * ppw1) && bk1 && !forced) {
    // fewer wavefronts than SIMDs (side by side): the time is one wavefront's chain of steps, so as few diagonals per
    // lane as the band allows -- several pairs side by side where they fit, which changes the number of wavefronts, not
    // the chain (2 kb pairs, band radius 20: 1.41 -> 0.49 ms; radius 50: 0.87 -> 0.49 ms).  Round 3 (found by
    // tests/micro/planner_check.py): this also holds for 1024 ... 1024 x ppw1 pairs, which used to fall between the two
    // rules and ran one pair per wavefront, two wavefronts per SIMD -- 2000 pairs of 1 kb with a 21-diagonal band
    // 0.48 ms, side by side 0.37 ms.
    l.bk = bk1; l.nl = (maxnd + bk1 - 1) / bk1; l.seg = 64 / l.nl >= 2 ? 1 : 0;
  }
  else if (want_seg) { l.bk = bkp; l.nl = nlp; l.seg = 1; }
  else if (bk1) { l.bk = bk1; l.nl = (maxnd + bk1 - 1) / bk1; }
  // one pair per wavefront with 16+ diagonals per lane is a long serial chain: small batches go multi-wavefront --
  // the strips if they win, else the 16-bit body on up to 8 wavefronts with 4 or 8 diagonals per lane
  if (latency_mode && l.bk >= 16 && !l.seg) {
    l = PackedLayout();
    if (!strips_win && !forced && !kn.no_packed_mw) l = packed_workgroup_layout(maxnd);
    if (l.nw <= 1) l = PackedLayout();                                      // (one wavefront would do: not this case)
  }
  return l;
}

// Whether the admitted body takes the matrix form on its layout.  Match / mismatch scoring over at most 4 letters IS a
// matrix, and the matrix form's cell pair is shorter -- one v_perm_b32 instead of xor, min and
// multiply-add, and under the local rule the bias comes off with a saturating subtract that makes the maximum with the begin
// candidate 0 unnecessary -- at the price of registers (3 wavefronts per SIMD instead of 5).  Taken where an A/B on the GPU
// showed it faster (tests/micro/ab_simple_matrix.py, profiles/round3_h_ab_simple_matrix.txt): the local rule at 8 diagonals
// per lane, one pair per wavefront (config 2's shape: 3.50 -> 3.29 ms) and at 16 (2.23 -> 2.15 ms), standard-mode GLOBAL at
// 32 per lane (4.38 -> 4.27 ms); slower lane-packed (+4 %) and under the overlap rule (+4 %).
static inline bool packed_matrix_form(const PackedAdmission& adm, const PackedLayout& l, bool simple, const PlanKnobs& kn) {
  const bool measured = !l.seg && l.nw <= 1 && (((l.bk == 8 || l.bk == 16) && adm.rule == 0) || (l.bk == 32 && adm.rule == 2));
  return !simple || adm.force_matrix || (adm.matrix_ok && (kn.simple_as_matrix > 0 || (kn.simple_as_matrix < 0 && measured)));
}

enum { PAIR_WAVES = 0, PAIR_TILED, PAIR_STRIPS };
struct PairLayout { int kind = PAIR_WAVES, bk = 0, nl = 64, nw = 1; };
// What every pair of a batch shares in the choice of its kernel.
struct PairRules {
  bool strips;        // the strip pipeline serves the batch (standard mode, integer scores it takes, ...)
  bool all_strips;    // PW_FLAG_FORCE_STRIP
  bool few_strips;    // latency mode, and the strips of all pairs one after another beat the slowest workgroup
  bool all_tiled;     // PW_FLAG_FORCE_TILED
  bool few_tiled;     // latency mode, and the tiles of all pairs one after another beat the slowest workgroup
  bool latency_mode, f64, wide_lanes;
  int packed_bk, packed_nl;                 // the packed 16-bit body's layout (packed_bk = 0: not on it)
};

// The kernel of one solvable pair: the strips, the tiles, or wavefronts (one, or a workgroup of nw) of bk diagonals per lane.
static inline PairLayout pair_layout(int ndiag, int X, const PairRules& r) {
  PairLayout l;
  // the strips always for tables wider than a workgroup holds; for batches of a few pairs (latency mode) when the strips of
  // all pairs, one pair after another, are estimated to finish before the slowest workgroup would (2 kb x 2 kb: 0.6 ms per
  // pair against 13.6 ms for one workgroup of 32-diagonal lanes -- up to 16 such pairs; 1 kb x 1 kb: 0.3 ms against 1.0 ms
  // -- up to 2), for tables that span at least two strips
  if (r.strips && (r.all_strips || ndiag > 2048 * kMaxWavesPerPair || (r.few_strips && X >= 127))) { l.kind = PAIR_STRIPS; return l; }
  if (r.packed_bk) { l.bk = r.packed_bk; l.nl = r.packed_nl; return l; }
  // a few pairs with bands wider than a wavefront holds, not served by the strips (f64 scores, a substitution matrix,
  // go > 0, banded): the tiles when all pairs, one after another, are estimated to finish before the slowest workgroup; and
  // tables wider than a workgroup holds
  if (r.all_tiled || ndiag > 2048 * kMaxWavesPerPair || (r.few_tiled && ndiag > 1024)) {
    l.kind = PAIR_TILED; l.bk = kTileBKHost; l.nl = (ndiag + l.bk - 1) / l.bk;
    return l;
  }
  l.bk = narrowest_bk(ndiag, kSupportedBK, kNumSupportedBK, 1);
  if (l.bk == 0) {
    // wider than one wavefront holds: a workgroup of nw wavefronts, 2048 diagonals each -- in latency mode as many
    // wavefronts as a workgroup takes, with as few diagonals per lane as that allows (2 kb x 2 kb: 8 x 8 instead of
    // 2 x 32 diagonals per lane); also with many pairs: at 32 diagonals per lane the kernel spills 1.4 - 3 KB of registers
    // per lane (300 pairs of 10 kb with a 3001-diagonal band: 208 ms with 2 x 32, measured below with 6 x 8)
    if (r.latency_mode || !r.wide_lanes) l.bk = narrowest_bk(ndiag, kWideMwBK, 3, kMaxWavesPerPair);
    if (l.bk == 0) l.bk = 32;
  } else if ((r.latency_mode && l.bk >= 16) || (r.f64 && l.bk >= 32)) {
    // a handful of pairs cannot fill the chip anyway: spread each over up to 8 wavefronts with few diagonals per lane (the
    // step count is fixed by X + Y; the work per step shrinks 4-8x, the exchange costs ~0.3 us); f64 with 32 diagonals per
    // lane needs more registers than a wavefront has (3000 pairs with a 1201-diagonal band take 166 ms on one wavefront each,
    // 47 ms on five wavefronts of 4 diagonals per lane)
    if (const int bk = narrowest_bk(ndiag, kNarrowMwBK, 3, kMaxWavesPerPair)) l.bk = bk;
  } else {
    return l;
  }
  l.nw = (ndiag + 64 * l.bk - 1) / (64 * l.bk);
  l.nl = 64 * l.nw;
  return l;
}

}  // namespace pw
#endif

// pw_wave.h -- the per-lane program of the banded anti-diagonal wavefront fill ("K1") and of the
// traceback walker ("K4").
//
// What it computes: the reference's dptable_solve (biseqt/pwlib/pw.c:47-114) with its move
// generators (_pw_internals.c:161-299) and end-cell search (:303-414), restated as
// (H, 4-bit ordered tie mask) per cell, and dptable_traceback (pw.c:116-151)
// restated over the tie masks.
//
// How it is laid out on a 64-lane CDNA wavefront (one wavefront per sequence pair):
//   * band coordinates: diagonal d = x - y, anti-diagonal s = x + y.  Lane l owns the BK (even)
//     consecutive diagonals dd = l*BK .. l*BK+BK-1 (dd = d - dmin); their running state
//     (H, the gap offers U/L, mask accumulator, best-so-far) lives in registers.
//   * a step advances one anti-diagonal; slot j holds a cell on the steps t == j (mod 2), so each
//     step a lane updates R = BK/2 independent cells in place: the diagonal predecessor is the slot's
//     own previous value, the up/left predecessors are the neighbouring slots' values from the
//     previous step.  Only the two block-edge values cross lanes, one DPP wave shift per step.
//   * the sequences stream through the lanes systolically: origin letters move towards lower lanes,
//     mutant letters towards higher lanes, one DPP shift per step; the edge lanes are fed from the
//     sequence arena with wave-uniform loads.
//   * every 16 steps each slot has accumulated 8 tie masks = one dword; the wave stores them with
//     16-byte-per-lane, 1 KiB-contiguous stores (layout: pw_types.h, mask_word_index).
//
// The file is written against a tiny platform policy P (lane id and count, shifts by one lane, shuffles,
// broadcast across the wavefronts of a workgroup) so
// that the very same lane program is compiled by hipcc into the gfx950 kernels (pw_kernels.hip) and
// by g++ into a 64-fiber lockstep emulator used only by the CPU tests (tests/emu).  PW_FN is the
// function qualifier each side supplies.
#ifndef PW_WAVE_H
#define PW_WAVE_H

#ifndef PW_FN
#error "PW_FN must be defined by the includer"
#endif

#include "pw_types.h"
#if !defined(__HIPCC__)
#include <stdlib.h>
#endif

namespace pw {

template <typename T> struct ScoreTraits;
template <> struct ScoreTraits<int32_t> {
  static constexpr bool is_int = true;
  // "no such predecessor".  Real scores are kept within +-2^27 by the host planner, so a sentinel
  // (even after a few thousand additions of small scores) never reaches a real score, and the sum of
  // two sentinels still fits an int32.
  PW_FN static int32_t neg() { return -(1 << 28); }
  PW_FN static int32_t zero_blk() { return 0; }
  // (the forms the floating-point path uses; for integers they are the plain expressions)
  PW_FN static int32_t max2(int32_t a, int32_t b) { return a > b ? a : b; }
  PW_FN static int32_t gap_offer(bool kept, int32_t go, int32_t A) { return kept ? A : A + go; }
};
template <> struct ScoreTraits<double> {
  static constexpr bool is_int = false;
  PW_FN static double neg() { return -1.0e300; }
  PW_FN static double zero_blk() { return -0.0; }   // x + (-0.0) == x bit for bit, also for x = +-0
  // The larger of two (finite) scores as ONE instruction (v_max_f64) instead of compare + two selects.  Same value as the
  // reference's "replace when strictly greater" (pw.c:92-103); only the sign of a zero may differ (documented exception).
  PW_FN static double max2(double a, double b) { return __builtin_fmax(a, b); }
  // A gap offer out of a cell whose own score + ge is `A`: A + go unless the same gap op is kept in the cell
  // (_pw_internals.c:268-278), as ONE fused multiply-add on a 0.0 / 1.0 factor whose high dword is the only thing selected:
  // fma(1, go, A) = round(go + A), the reference's (H + ge) + go; fma(0, go, A) = A.  Exact, no double rounding: the
  // product is 0 or go itself.  (Compare + add + two 32-bit selects otherwise.)
  union D2I_ { double d; int32_t i[2]; };
  PW_FN static double gap_offer(bool kept, double go, double A) {
    D2I_ f; f.i[0] = 0; f.i[1] = kept ? 0 : 0x3ff00000;
    return __builtin_fma(f.d, go, A);
  }
};

// ---- cross-lane moves for any score type, built on the platform's 32-bit wave shifts -----------
template <class P> PW_FN int32_t xshr1(int32_t v, int32_t old) { return P::shr1(v, old); }
template <class P> PW_FN int32_t xshl1(int32_t v, int32_t old) { return P::shl1(v, old); }
template <class P> PW_FN uint32_t xshr1(uint32_t v, uint32_t old) { return (uint32_t)P::shr1((int32_t)v, (int32_t)old); }
template <class P> PW_FN uint32_t xshl1(uint32_t v, uint32_t old) { return (uint32_t)P::shl1((int32_t)v, (int32_t)old); }
union D2I { double d; int32_t i[2]; };
template <class P> PW_FN double xshr1(double v, double old) {
  D2I a, o, r; a.d = v; o.d = old;
  r.i[0] = P::shr1(a.i[0], o.i[0]); r.i[1] = P::shr1(a.i[1], o.i[1]);
  return r.d;
}
template <class P> PW_FN double xshl1(double v, double old) {
  D2I a, o, r; a.d = v; o.d = old;
  r.i[0] = P::shl1(a.i[0], o.i[0]); r.i[1] = P::shl1(a.i[1], o.i[1]);
  return r.d;
}
// A score and a 32-bit word moved by one lane in ONE exchange (policies whose shifts cross wavefronts through
// LDS pay one barrier for the group instead of two per value; `phase` alternates their LDS slots).
template <class P, int N> PW_FN void xshrv(int32_t (&v)[N], const int32_t (&old)[N], int phase) {
  if constexpr (P::kBatchedShifts) P::template shrv<N>(v, old, phase);
  else {
#pragma unroll
    for (int i = 0; i < N; i++) v[i] = P::shr1(v[i], old[i]);
  }
}
template <class P, int N> PW_FN void xshlv(int32_t (&v)[N], const int32_t (&old)[N], int phase) {
  if constexpr (P::kBatchedShifts) P::template shlv<N>(v, old, phase);
  else {
#pragma unroll
    for (int i = 0; i < N; i++) v[i] = P::shl1(v[i], old[i]);
  }
}
template <class P, bool LEFT> PW_FN void xshift_pair(int32_t& s, int32_t sold, uint32_t& w, uint32_t wold, int phase) {
  int32_t v[2] = {s, (int32_t)w}; const int32_t o[2] = {sold, (int32_t)wold};
  if (LEFT) xshlv<P, 2>(v, o, phase); else xshrv<P, 2>(v, o, phase);
  s = v[0]; w = (uint32_t)v[1];
}
template <class P, bool LEFT> PW_FN void xshift_pair(double& s, double sold, uint32_t& w, uint32_t wold, int phase) {
  D2I a, b; a.d = s; b.d = sold;
  if constexpr (!P::kBatchedShifts) {
    // Every caller passes "no such predecessor" as the edge lane's value, and such a value only has to be hugely negative:
    // its HIGH dword decides that.  So the low dword moves with a zero-filling shift (no copy of a constant in front of the
    // DPP move), the high dword with the constant.
    a.i[0] = LEFT ? P::shl1z(a.i[0]) : P::shr1z(a.i[0]);
    a.i[1] = LEFT ? P::shl1(a.i[1], b.i[1]) : P::shr1(a.i[1], b.i[1]);
    w = (uint32_t)(LEFT ? P::shl1((int32_t)w, (int32_t)wold) : P::shr1((int32_t)w, (int32_t)wold));
    s = a.d;
    return;
  }
  int32_t v[3] = {a.i[0], a.i[1], (int32_t)w}; const int32_t o[3] = {b.i[0], b.i[1], (int32_t)wold};
  if (LEFT) xshlv<P, 3>(v, o, phase); else xshrv<P, 3>(v, o, phase);
  a.i[0] = v[0]; a.i[1] = v[1]; s = a.d; w = (uint32_t)v[2];
}
template <class P> PW_FN int32_t xshfl_xor(int32_t v, int m) { return P::shfl_xor(v, m); }
template <class P> PW_FN double xshfl_xor(double v, int m) {
  D2I a, r; a.d = v;
  r.i[0] = P::shfl_xor(a.i[0], m); r.i[1] = P::shfl_xor(a.i[1], m);
  return r.d;
}
template <class P> PW_FN uint64_t xshfl_xor(uint64_t v, int m) {
  uint32_t lo = (uint32_t)P::shfl_xor((int32_t)(uint32_t)v, m);
  uint32_t hi = (uint32_t)P::shfl_xor((int32_t)(uint32_t)(v >> 32), m);
  return ((uint64_t)hi << 32) | lo;
}

template <class P> PW_FN int32_t xwave_bcast(int32_t v, int w) { return P::wave_bcast(v, w); }
template <class P> PW_FN double xwave_bcast(double v, int w) {
  D2I a, r; a.d = v;
  r.i[0] = P::wave_bcast(a.i[0], w); r.i[1] = P::wave_bcast(a.i[1], w);
  return r.d;
}
template <class P> PW_FN uint64_t xwave_bcast(uint64_t v, int w) {
  const uint32_t lo = (uint32_t)P::wave_bcast((int32_t)(uint32_t)v, w);
  const uint32_t hi = (uint32_t)P::wave_bcast((int32_t)(uint32_t)(v >> 32), w);
  return ((uint64_t)hi << 32) | lo;
}

PW_FN int32_t pw_clampi(int32_t v, int32_t lo, int32_t hi) { return v < lo ? lo : (v > hi ? hi : v); }

// =================================================================================================
// K1: fill one pair.  Template switches:
//   BK       diagonals per lane (even); the wave covers 64*BK diagonals
//   BANY     an alignment may begin anywhere (LOCAL, END_ANCHORED, B_LOCAL)         [fast kernels]
//   TRACK    keep the first best cell of every diagonal (needed by the *LOCAL end rules)
//   GENERIC  everything at run time: substitution matrix lookup, begin rule, sign of the gap-open
//            score, optional dump of the score plane.  (BANY/TRACK are ignored: TRACK is on.)
// =================================================================================================
template <class P, typename T, int BK, bool BANY, bool TRACK_, bool GENERIC>
struct WaveFill {
  static constexpr int R = BK / 2;
  static constexpr bool TRACK = TRACK_ || GENERIC;
  using Tr = ScoreTraits<T>;
  // TAB: the substitution score is READ from a table (LDS on the device) instead of selected by a letter comparison: one
  // add for the address and a read that does not occupy the vector ALU, against compare + select (+ a second select for a
  // 64-bit value).  It also makes ANY substitution matrix -- BLOSUM-style integer matrices over 20 letters, full log-odds
  // matrices -- exactly as cheap as match / mismatch scoring on these kernels (round 2 sent every matrix to the generic
  // kernel).  The letter windows hold byte offsets: the origin letter times the row size, the mutant letter times the
  // element size.  (Round 3; `false` restores the comparison for integer scores.)
  static constexpr bool TAB = true;

  // ---- uniform (per pair) ----
  const FillParams<T>& a;
  const PairDesc& pd;
  const T* sub_tab;           // substitution table (LDS on the device) for GENERIC
  const uint8_t* oseq;
  const uint8_t* mseq;
  int X, Y, ndiag, olast, mlast;

  // ---- per lane ----
  int lane;
  int njl;                    // slot j is inside the band iff j < njl
  int xbase, ybase;           // (x, y) of slot 0 on the even step of the current iteration
  T H[BK], U[BK], L[BK], blkL[BK], best[BK];
  int32_t bestT[BK];
  uint32_t m[BK];
  uint32_t ow[R], mw[R];

  PW_FN WaveFill(const FillParams<T>& a_, const PairDesc& pd_, const T* sub_tab_)
      : a(a_), pd(pd_), sub_tab(sub_tab_) {}

  // (the table sits in LDS -- always for the fast f64 kernels, whose planner admits alphabets of up to kMaxLdsL letters
  //  only; the generic kernels also take larger alphabets, from global memory, and ask at run time)
  uint32_t tab_handle = 0;      // the platform's handle of the LDS copy (P::tab_read)
  bool tab_in_lds = false;
  PW_FN T subst(uint32_t oc, uint32_t mc) const {
    if (TAB) {      // (pre-scaled letters: see TAB)
      if (!GENERIC) return P::template tab_read<T, true>(sub_tab, tab_handle, oc + mc, true);
      return P::template tab_read<T, false>(sub_tab, tab_handle, oc + mc, tab_in_lds);
    }
    return oc == mc ? a.match : a.mismatch;
  }
  PW_FN uint32_t osc() const { return TAB ? (uint32_t)a.L * (uint32_t)sizeof(T) : 1u; }
  PW_FN uint32_t msc() const { return TAB ? (uint32_t)sizeof(T) : 1u; }

  // One cell of slot J on step t (lane-local coordinates x, y).
  template <bool RAMP, int J>
  PW_FN void cell(T up, T left, T sub, int x, int y, int t) {
    const T hD = up, hI = left;
    const T hM = H[J] + sub;
    bool active = true;
    bool ball;
    if (RAMP) {
      active = (J < njl) && ((uint32_t)x <= (uint32_t)X) && ((uint32_t)y <= (uint32_t)Y);
      const int brule = GENERIC ? a.brule : (BANY ? (int)BRULE_ANY : a.brule);
      const bool edge = (x == 0) || (y == 0);
      const bool orig = (x == 0) && (y == 0);
      ball = (brule == BRULE_ANY) || (edge && (brule == BRULE_EDGE || orig));
    } else {
      ball = GENERIC ? (a.brule == BRULE_ANY) : BANY;   // no first cells in the steady phase
    }
    // maximum in the reference's candidate order B, D, I, M, later candidates replace only when
    // strictly greater (pw.c:92-103)
    T Hn;
    if (Tr::is_int) {
      Hn = hD > hI ? hD : hI;
      Hn = hM > Hn ? hM : Hn;
      const T b0 = ball ? T(0) : Tr::neg();
      Hn = b0 > Hn ? b0 : Hn;
    } else {
      // (an alignment that may not begin here: "no such predecessor" as the begin candidate, as the integer path does)
      const T b0 = ball ? T(0) : Tr::neg();
      Hn = Tr::max2(Tr::max2(Tr::max2(b0, hD), hI), hM);
    }
    const bool bB = ball && (Hn == T(0));
    const bool bD = (hD == Hn), bI = (hI == Hn), bM = (hM == Hn);
    // what this cell offers downwards (as a D predecessor) and rightwards (as an I predecessor):
    // _alnchoice_ID scans the kept choices, (H + ge) [+ go when the kept op differs], first strict max
    // (_pw_internals.c:268-278).  All kept choices share H, so only "is the same op kept" matters.
    const T A = Hn + a.ge;
    T Un, Ln;
    if (!GENERIC) {                 // go <= 0 guaranteed by the planner
      if (Tr::is_int) {
        const T gego = a.ge + a.go;
        Un = Hn + (bD ? a.ge : gego);
        Ln = Hn + (bI ? a.ge : gego) + blkL[J];
      } else {
        Un = Tr::gap_offer(bD, a.go, A);
        Ln = Tr::gap_offer(bI, a.go, A) + blkL[J];
      }
    } else {
      const T Bv = A + a.go;
      const T hi = A > Bv ? A : Bv;
      const bool oD = bB || bI || bM, oI = bB || bD || bM;   // some other op kept as well
      Un = bD ? (oD ? hi : A) : Bv;
      Ln = (bI ? (oI ? hi : A) : Bv) + blkL[J];
    }
    // the tie nibble (M, I, D, B from bit 3 down: MM, MI, MD, MB) is shifted into the slot's mask word one flag at a time:
    // on the device each P::shl1_in is ONE add-with-carry whose carry-in is the comparison's lane mask (m + m + flag), four
    // instructions per cell instead of four selects, the ORs and the shift
    if (RAMP) {
      m[J] = P::shl1_in(P::shl1_in(P::shl1_in(P::shl1_in(m[J], bM && active), bI && active), bD && active), bB && active);
      H[J] = active ? Hn : H[J];
      U[J] = active ? Un : U[J];
      L[J] = active ? Ln : L[J];
      if (TRACK) {
        const bool upd = active && (Hn > best[J]);
        best[J] = upd ? Hn : best[J];
        bestT[J] = upd ? t : bestT[J];
      }
    } else {
      m[J] = P::shl1_in(P::shl1_in(P::shl1_in(P::shl1_in(m[J], bM), bI), bD), bB);
      H[J] = Hn; U[J] = Un; L[J] = Ln;
      if (TRACK) {
        const bool upd = Hn > best[J];
        if (Tr::is_int) best[J] = upd ? Hn : best[J];
        else best[J] = Tr::max2(best[J], Hn);           // (one v_max_f64 instead of two selects)
        bestT[J] = upd ? t : bestT[J];
      }
    }
    if (GENERIC) {
      if (a.hdump != nullptr && active && (RAMP || J < njl)) {
        const int aa = x < y ? x : y;
        a.hdump[pd.h_off + (uint64_t)(lane * BK + J) * (uint64_t)pd.h_pitch + (uint64_t)aa] = Hn;
      }
    }
  }

  // compile-time loops over the slots of one parity
  // (AHEAD: the substitution scores of the step were read from the table a step earlier -- sE / sO, see iteration())
  template <bool RAMP, int I> struct EvenLoop {
    PW_FN static void run(WaveFill& w, T uin, int t) {
      w.template cell<RAMP, 2 * I>(I == 0 ? uin : w.U[(2 * I - 1 + BK) % BK], w.L[2 * I + 1],
                                   AHEAD ? w.sE[I] : w.subst(w.ow[I], w.mw[I]), w.xbase + I, w.ybase - I, t);
      EvenLoop<RAMP, I + 1>::run(w, uin, t);
    }
  };
  template <bool RAMP> struct EvenLoop<RAMP, R> { PW_FN static void run(WaveFill&, T, int) {} };
  template <bool RAMP, int I> struct OddLoop {
    PW_FN static void run(WaveFill& w, T lin, int t) {
      w.template cell<RAMP, 2 * I + 1>(w.U[2 * I], I == R - 1 ? lin : w.L[(2 * I + 2) % BK],
                                       AHEAD ? w.sO[I] : w.subst(w.ow[I], w.mw[I]), w.xbase + I + 1, w.ybase - I, t);
      OddLoop<RAMP, I + 1>::run(w, lin, t);
    }
  };
  template <bool RAMP> struct OddLoop<RAMP, R> { PW_FN static void run(WaveFill&, T, int) {} };

  // AHEAD (single-wavefront platforms): the letters do not depend on the arithmetic, so their two window moves run ahead of
  // it and every table read is issued a whole STEP before the cell that needs it -- the odd step's at the start of the even
  // step, the next even step's at the start of the odd step -- instead of a few instructions before (a table read takes
  // ~100 cycles; with two wavefronts per SIMD nothing else covers it).  Platforms whose shifts cross wavefronts through LDS
  // move a letter and a score in ONE exchange and keep the letters in step with the arithmetic.
  static constexpr bool AHEAD = TAB && !P::kBatchedShifts;
  T sE[AHEAD ? R : 1], sO[AHEAD ? R : 1];
  PW_FN static T shift_score_l(T v) { T r = v; uint32_t none = 0; xshift_pair<P, true>(r, Tr::neg(), none, 0u, 0); return r; }
  PW_FN static T shift_score_r(T v) { T r = v; uint32_t none = 0; xshift_pair<P, false>(r, Tr::neg(), none, 0u, 0); return r; }

  // One iteration = the even step 2*it and the odd step 2*it + 1.
  template <bool RAMP>
  PW_FN void iteration(int it, int k) {
    // even step: slot 0 takes its "up" offer from the previous lane's last slot (moved at the end of the
    // previous iteration, together with the mutant window)
    T uin = uin_next;
    if (P::kVirtualLanes) uin = lane == 0 ? Tr::neg() : uin;    // nothing lies below diagonal 0 of the band
    if constexpr (AHEAD) {
      // origin window as of the odd step (lane l takes lane l+1's lowest letter, the last lane is fed from the arena)
      {
        const uint32_t oin = (uint32_t)P::shl1((int32_t)ow[0], (int32_t)(feed_byte(fo_lo, fo_hi, k) * osc()));
#pragma unroll
        for (int i = 0; i + 1 < R; i++) ow[i] = ow[i + 1];
        ow[R - 1] = oin;
      }
#pragma unroll
      for (int i = 0; i < R; i++) sO[i] = subst(ow[i], mw[i]);           // the odd step's scores: a step ahead
      EvenLoop<RAMP, 0>::run(*this, uin, 2 * it);
      const T lin = shift_score_l(L[0]);
      // mutant window as of the next iteration (lane l takes lane l-1's highest letter, lane 0 is fed from the arena)
      {
        const uint32_t min_ = (uint32_t)P::shr1((int32_t)mw[R - 1], (int32_t)(feed_byte(fm_lo, fm_hi, k) * msc()));
#pragma unroll
        for (int i = R - 1; i > 0; i--) mw[i] = mw[i - 1];
        mw[0] = min_;
      }
#pragma unroll
      for (int i = 0; i < R; i++) sE[i] = subst(ow[i], mw[i]);           // the next even step's scores
      OddLoop<RAMP, 0>::run(*this, lin, 2 * it + 1);
      uin_next = shift_score_r(U[BK - 1]);
      xbase++; ybase++;
      return;
    }
    EvenLoop<RAMP, 0>::run(*this, uin, 2 * it);
    // one exchange to the left: the origin window moves on by one letter (lane l takes lane l+1's lowest
    // letter, the last lane is fed from the arena) and the last slot gets its "left" offer for the odd step
    T lin = L[0];
    {
      uint32_t oin = ow[0];
      xshift_pair<P, true>(lin, Tr::neg(), oin, feed_byte(fo_lo, fo_hi, k) * osc(), it & 1);
#pragma unroll
      for (int i = 0; i + 1 < R; i++) ow[i] = ow[i + 1];
      ow[R - 1] = oin;
    }
    OddLoop<RAMP, 0>::run(*this, lin, 2 * it + 1);
    // one exchange to the right: the mutant window moves on (lane l takes lane l-1's highest letter, lane 0
    // is fed from the arena) and the next even step's "up" offer travels with it
    {
      uint32_t min_ = mw[R - 1];
      uin_next = U[BK - 1];
      xshift_pair<P, false>(uin_next, Tr::neg(), min_, feed_byte(fm_lo, fm_hi, k) * msc(), it & 1);
#pragma unroll
      for (int i = R - 1; i > 0; i--) mw[i] = mw[i - 1];
      mw[0] = min_;
    }
    xbase++; ybase++;
  }

  // ---- edge-lane feeders (wave-uniform) ----------------------------------------------------------
  // The last lane needs origin letter o[xfeed_o + it] and lane 0 mutant letter m[yfeed_m + it] on
  // iteration `it`.  The 8 letters a block consumes per sequence are fetched as three aligned dwords ONE
  // BLOCK AHEAD (feed_issue) and funnel-shifted into two registers when the block starts (feed_commit),
  // so no iteration ever waits on memory.  Word indices are clamped: letters outside the sequence feed
  // only cells outside the table.
  T uin_next;                 // slot 0's "up" offer for the next even step
  int xfeed_o, yfeed_m;       // arena index the edge lanes are fed from at iteration 0
  int owlast, mwlast;         // last dword of each frame
  uint32_t fo_lo, fo_hi, fm_lo, fm_hi;                 // the current block's 8 + 8 letters
  uint32_t fo_n0, fo_n1, fo_n2, fm_n0, fm_n1, fm_n2;   // next block's raw dwords

  PW_FN static uint32_t feed_byte(uint32_t lo, uint32_t hi, int k) {
    return ((k < 4 ? lo : hi) >> (8 * (k & 3))) & 0xffu;
  }
  PW_FN static uint32_t funnel(uint32_t hi, uint32_t lo, int r) {
    return (uint32_t)(((((uint64_t)hi) << 32) | (uint64_t)lo) >> (8 * r));
  }
  PW_FN void feed_issue(int b) {
    // (wave-uniform indices into the read-only letter arena: scalar loads, which leave vmcnt to the mask stores)
    const int wo = (xfeed_o + 8 * b) >> 2, wm = (yfeed_m + 8 * b) >> 2;
    fo_n0 = P::const_dword(oseq, pw_clampi(wo, 0, owlast)); fo_n1 = P::const_dword(oseq, pw_clampi(wo + 1, 0, owlast));
    fo_n2 = P::const_dword(oseq, pw_clampi(wo + 2, 0, owlast));
    fm_n0 = P::const_dword(mseq, pw_clampi(wm, 0, mwlast)); fm_n1 = P::const_dword(mseq, pw_clampi(wm + 1, 0, mwlast));
    fm_n2 = P::const_dword(mseq, pw_clampi(wm + 2, 0, mwlast));
  }
  PW_FN void feed_commit(int b) {
    const int ro = (xfeed_o + 8 * b) & 3, rm = (yfeed_m + 8 * b) & 3;
    fo_lo = funnel(fo_n1, fo_n0, ro); fo_hi = funnel(fo_n2, fo_n1, ro);
    fm_lo = funnel(fm_n1, fm_n0, rm); fm_hi = funnel(fm_n2, fm_n1, rm);
  }

  // A block = 16 steps = 8 iterations = one mask dword per slot.  The steady body is fully unrolled (the
  // letter-window shifts become register renames); the predicated ramp body runs only at the two ends
  // of a pair and is kept rolled to bound code size and scalar-register pressure.
  template <bool RAMP>
  PW_FN void block(int b) {
    if (RAMP) {
#pragma unroll 1
      for (int k = 0; k < 8; k++) iteration<true>(8 * b + k, k);
    } else {
#pragma unroll
      for (int k = 0; k < 8; k++) iteration<false>(8 * b + k, k);
    }
  }

  PW_FN void store_masks(int b) {
    if (lane >= 0 && lane * BK < ndiag && P::central()) {
      uint32_t* dst = a.masks + pd.mask_off;
#pragma unroll
      for (int j = 0; j < BK; j++) dst[mask_word_index(BK, pd.nl, b, lane, j)] = m[j];
    }
  }

  PW_FN void init(int it0 = 0) {
    lane = P::lane();
    X = pd.X; Y = pd.Y; ndiag = pd.ndiag;
    oseq = a.arena + pd.o_off; mseq = a.arena + pd.m_off;
    olast = X > 0 ? X - 1 : 0; mlast = Y > 0 ? Y - 1 : 0;
    owlast = olast >> 2; mwlast = mlast >> 2;
    njl = lane < 0 ? 0 : ndiag - lane * BK;      // (tiles may carry virtual lanes below diagonal 0)
    uin_next = Tr::neg();
    // s0 == dmin (mod 2): e, f are exact
    const int e = (pd.s0 + pd.dmin) >> 1;       // x of diagonal dd = 0 on step t = 0
    const int f = (pd.s0 - pd.dmin) >> 1;       // y of diagonal dd = 0 on step t = 0
    xbase = e + it0 + lane * R;
    ybase = f + it0 - lane * R;
    xfeed_o = e + P::nlanes() * R - 1;          // letter o[xbase + R - 1] of a virtual lane beyond the last one
    yfeed_m = f - P::lane0() * R;               // letter m[ybase] of the first lane
#pragma unroll
    for (int j = 0; j < BK; j++) {
      H[j] = Tr::neg(); U[j] = Tr::neg(); L[j] = Tr::neg();
      best[j] = Tr::neg(); bestT[j] = 0; m[j] = 0;
      // the first diagonal above the band must never offer an insertion into the band
      blkL[j] = (lane * BK + j == ndiag) ? Tr::neg() : Tr::zero_blk();
    }
#pragma unroll
    for (int i = 0; i < R; i++) {
      ow[i] = (uint32_t)oseq[pw_clampi(xbase + i - 1, 0, olast)] * osc();
      mw[i] = (uint32_t)mseq[pw_clampi(ybase - i - 1, 0, mlast)] * msc();
    }
    if (AHEAD) {
#pragma unroll
      for (int i = 0; i < (AHEAD ? R : 1); i++) sE[i] = subst(ow[i], mw[i]);
    }
  }

  PW_FN void run() {
    init();
    feed_issue(0);
    for (int b = 0; b < pd.nblocks; b++) {
      feed_commit(b);
      if (b + 1 < pd.nblocks) feed_issue(b + 1);
      if (b >= pd.steady_b0 && b < pd.steady_b1) block<false>(b);
      else block<true>(b);
      store_masks(b);
    }
    finish();
  }

  // ---- K2b: one tile of a time-blocked, ghost-zone tiled fill (tables too wide for one workgroup) -------
  // The workgroup owns P::nlanes() - P::lane0() lanes of the band; the outer `ghost` lanes on each side are
  // recomputed copies of the neighbouring tiles' lanes.  Dependencies travel one diagonal per step, so after
  // tile_nb * 16 <= ghost * BK steps the centre lanes (P::central()) are still exact; only they store masks
  // and hand their state to the next time block.  State: [5][st_pitch] = H, U, L, best, bestT per diagonal.
  PW_FN void run_tile() {
    const int bb0 = a.tile_b0, bb1 = a.tile_b0 + a.tile_nb, pitch = a.st_pitch;
    lane = P::lane();
    ndiag = pd.ndiag;
    // steps on which this tile's in-band diagonals (ghost lanes included) hold their first / last cell
    int w4[4] = {-0x7fffffff, -0x7fffffff, -0x7fffffff, -0x7fffffff};   // max of: -tf, tf, -tl, tl
#pragma unroll
    for (int j = 0; j < BK; j++) {
      const int dd = lane * BK + j;
      if (lane >= 0 && dd < ndiag) {
        const int d = pd.dmin + dd;
        const int tf = (d < 0 ? -d : d) - pd.s0;
        const int tl = tf + 2 * ((d > 0 ? 0 : d) + (pd.X - d > pd.Y ? pd.Y : pd.X - d));
        w4[0] = -tf > w4[0] ? -tf : w4[0]; w4[1] = tf > w4[1] ? tf : w4[1];
        w4[2] = -tl > w4[2] ? -tl : w4[2]; w4[3] = tl > w4[3] ? tl : w4[3];
      }
    }
    P::wg_max4(w4);
    const int tfmin = -w4[0], tfmax = w4[1], tlmin = -w4[2], tlmax = w4[3];
    // the blocks of this time block in which any of them is live
    int bA = tfmin >> 4, bB = tlmax >> 4;
    if (w4[1] == -0x7fffffff) { bA = 1; bB = 0; }          // no diagonal of the band in this tile
    bA = bA < bb0 ? bb0 : bA; bB = bB > bb1 - 1 ? bb1 - 1 : bB;
    if (bA > bB) {
      // not started yet or already finished: the state passes through unchanged
      if (P::central()) {
#pragma unroll
        for (int j = 0; j < BK; j++) {
          const int dd = lane * BK + j;
          if (lane >= 0 && dd < ndiag) {
#pragma unroll
            for (int r = 0; r < 5; r++)
              a.st_out[r * pitch + dd] = bb0 > 0 ? a.st_in[r * pitch + dd] : (r == 4 ? T(0) : Tr::neg());
          }
        }
      }
      return;
    }
    init(8 * bA);
    if (bb0 > 0) {
#pragma unroll
      for (int j = 0; j < BK; j++) {
        const int dd = lane * BK + j;
        if (lane >= 0 && dd < ndiag) {
          H[j] = a.st_in[dd]; U[j] = a.st_in[pitch + dd]; L[j] = a.st_in[2 * pitch + dd];
          best[j] = a.st_in[3 * pitch + dd]; bestT[j] = (int32_t)a.st_in[4 * pitch + dd];
        }
      }
      uint32_t none = 0;
      uin_next = U[BK - 1];
      xshift_pair<P, false>(uin_next, Tr::neg(), none, 0u, 1);
    }
    feed_issue(bA);
    for (int b = bA; b <= bB; b++) {
      feed_commit(b);
      if (b < bB) feed_issue(b + 1);
      // steady: every diagonal of the tile started strictly before the block and none ends inside it
      if (16 * b > tfmax && 16 * b + 15 <= tlmin) block<false>(b);
      else block<true>(b);
      store_masks(b);
    }
    if (P::central()) {
#pragma unroll
      for (int j = 0; j < BK; j++) {
        const int dd = lane * BK + j;
        if (lane >= 0 && dd < ndiag) {
          a.st_out[dd] = H[j]; a.st_out[pitch + dd] = U[j]; a.st_out[2 * pitch + dd] = L[j];
          a.st_out[3 * pitch + dd] = best[j]; a.st_out[4 * pitch + dd] = (T)bestT[j];
        }
      }
    }
  }

  // ---- end-cell search: reduce (score desc, scan rank asc) over the in-band diagonals ----------
  PW_FN void finish() {
    const int endrule = a.endrule;
    T cs = Tr::neg(); uint64_t ck = ~(uint64_t)0; int cx = -1, cy = -1; bool have = false;
#pragma unroll
    for (int j = 0; j < BK; j++) {
      const int dd = lane * BK + j;
      const int d = pd.dmin + dd;
      const bool inband = dd < ndiag;
      // last cell of diagonal d
      const bool ends_right = d < X - Y;           // ends on the right column y = Y, else bottom row x = X
      const int lx = ends_right ? d + Y : X, ly = ends_right ? Y : X - d;
      T s; uint64_t k; int x, y; bool ok = inband;
      if (endrule == END_CORNER) {
        ok = ok && (d == X - Y); s = H[j]; k = 0; x = X; y = Y;
      } else if (endrule == END_STD_OVERLAP) {
        // row-major over last column (x < X) then last row: rank x for (x, Y), X + y for (X, y)
        s = H[j]; x = lx; y = ly; k = ends_right ? (uint64_t)(uint32_t)lx : (uint64_t)(uint32_t)(X + ly);
      } else if (endrule == END_BANDED_OVERLAP) {
        s = H[j]; x = lx; y = ly; k = (uint64_t)(uint32_t)dd;
      } else {
        // first best cell of the diagonal: step bestT -> index along the diagonal
        const int tfirst = (d < 0 ? -d : d) - pd.s0;
        const int aa = (bestT[j] - tfirst) >> 1;
        s = best[j]; x = aa + (d > 0 ? d : 0); y = aa - (d < 0 ? d : 0);
        if (endrule == END_STD_LOCAL) k = (uint64_t)(uint32_t)x * (uint64_t)(uint32_t)(Y + 1) + (uint64_t)(uint32_t)y;
        else k = ((uint64_t)(uint32_t)dd << 32) | (uint64_t)(uint32_t)aa;
      }
      const bool better = ok && (!have || s > cs || (s == cs && k < ck));
      if (better) { cs = s; ck = k; cx = x; cy = y; have = true; }
    }
    // butterfly over the 64 lanes
    int hv = have ? 1 : 0;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
      const T os = xshfl_xor<P>(cs, off);
      const uint64_t ok_ = xshfl_xor<P>(ck, off);
      const int ox = P::shfl_xor(cx, off), oy = P::shfl_xor(cy, off), oh = P::shfl_xor(hv, off);
      const bool take = oh && (!hv || os > cs || (os == cs && ok_ < ck));
      if (take) { cs = os; ck = ok_; cx = ox; cy = oy; hv = 1; }
    }
    // several wavefronts per pair (wide bands): reduce the per-wave winners the same way
    if (P::nwaves() > 1) {
      T bs = cs; uint64_t bk_ = ck; int bx = cx, by = cy, bh = 0;
      for (int wv = 0; wv < P::nwaves(); wv++) {
        const T os = xwave_bcast<P>(cs, wv);
        const uint64_t ok_ = xwave_bcast<P>(ck, wv);
        const int ox = P::wave_bcast(cx, wv), oy = P::wave_bcast(cy, wv), oh = P::wave_bcast(hv, wv);
        const bool take = oh && (!bh || os > bs || (os == bs && ok_ < bk_));
        if (take) { bs = os; bk_ = ok_; bx = ox; by = oy; bh = 1; }
      }
      cs = bs; ck = bk_; cx = bx; cy = by; hv = bh;
    }
    if (lane == 0) {
      Result r;
      r.score = (double)cs * a.score_mul;
      // table coordinates as dptable_solve returns them (_cellpos_from_xy, _pw_internals.c:87-98)
      r.opt_i = a.banded ? cx - cy - pd.dmin : cx;
      r.opt_j = a.banded ? (cx < cy ? cx : cy) : cy;
      r.origin_idx = 0; r.mutant_idx = 0; r.tx_len = 0; r.status = 0;
      // LOCAL / START_ANCHORED start from the score of cell (0,0), i.e. 0 (_pw_internals.c:342)
      if (!hv || (endrule == END_STD_LOCAL && !(cs > T(0)))) { r.opt_i = -1; r.opt_j = -1; r.score = 0.0; }
      a.results[pair_slot] = r;
    }
  }
  int pair_slot;
};

// =================================================================================================
// K1, packed 16-bit steady phase.
//
// Measured on gfx950 (profiles/round1_valu_issue_table.txt): only v_add/v_sub/v_xor/v_mov issue at the
// 2-cycle wave64 rate; v_max/v_min/v_cmp/v_cndmask, shifts, every VOP3 op, DPP and the packed VOP3P ops
// all take ~4 cycles.  The 32-bit cell update above is almost entirely 4-cycle ops, one cell each.  The
// packed form below does the same recurrence on TWO cells per 4-cycle v_pk_* op, with the tie bits
// obtained arithmetically (n = min(H - candidate, 1) is 0 iff the candidate is kept) instead of through
// compare -> select, so a steady-phase cell costs roughly half the issue cycles.
//
// Register layout: a lane's BK diagonals are split into a low and a high half-block of BK/2; slot j of the
// low half-block and slot j + BK/2 of the high one share a register (lo / hi 16 bits).  With that pairing
// the up / left neighbours of a register pair are again whole registers of the other parity; only the
// two block edges need one DPP wave shift + one v_alignbit per step.
//
// Blocks in which diagonals start or end run a slightly longer packed body (cellpair<EDGE = true>) that
// needs no predication at all -- see there.  Eligibility (host planner): LOCAL and B_LOCAL (begin anywhere,
// end anywhere: the end-cell search uses the tracked bests only), match/mismatch scoring, go <= 0, every
// score within +-100, min(X,Y) * max(match, mismatch, 0) <= 8000 (below the 8192-deep sentinel that blocks the first diagonal
// above the band), X + Y + 2 < 32000 (steps as signed 16-bit).
// =================================================================================================
// 16-byte group of the mask plane; an 8-byte store at any byte address
struct __attribute__((aligned(8))) U4 { uint32_t x, y, z, w; };
struct __attribute__((packed)) PackedU64 { uint64_t v; };   // an 8-byte store at any byte address
struct __attribute__((packed)) PackedU32 { uint32_t v; };   // a 4-byte load at any byte address

namespace pk {
#if defined(__HIP_DEVICE_COMPILE__)
// clang vector types: the backend selects v_pk_add_u16 / v_pk_sub_i16 / v_pk_max_i16 / v_pk_min_u16 /
// v_pk_mad_u16 itself and knows their latencies (inline asm would be padded with s_nop)
typedef short s2_t __attribute__((ext_vector_type(2)));
typedef unsigned short u2_t __attribute__((ext_vector_type(2)));
PW_FN s2_t as_s2(uint32_t v) { return __builtin_bit_cast(s2_t, v); }
PW_FN u2_t as_u2(uint32_t v) { return __builtin_bit_cast(u2_t, v); }
PW_FN uint32_t add(uint32_t a, uint32_t b) { return __builtin_bit_cast(uint32_t, (u2_t)(as_u2(a) + as_u2(b))); }
PW_FN uint32_t sub(uint32_t a, uint32_t b) { return __builtin_bit_cast(uint32_t, (u2_t)(as_u2(a) - as_u2(b))); }
// packed add where no half can carry: a plain 32-bit add.  Contract: no half of a in [0xff80, 0xffff], b a byte per half
PW_FN uint32_t add32(uint32_t a, uint32_t b) { return a + b; }
// unsigned saturating subtract per half: max(a - b, 0) (v_pk_sub_u16 ... clamp)
PW_FN uint32_t subsat(uint32_t a, uint32_t b) { return __builtin_bit_cast(uint32_t, __builtin_elementwise_sub_sat(as_u2(a), as_u2(b))); }
PW_FN uint32_t max(uint32_t a, uint32_t b) { return __builtin_bit_cast(uint32_t, __builtin_elementwise_max(as_s2(a), as_s2(b))); }
// NB min(x, 1) and (x >> 15) & c with LITERAL constants would be rewritten by the optimizer into compare +
// select per half (the very pattern this kernel avoids), and inline asm gets padded with s_nop by the
// hazard recogniser.  Callers therefore pass the constants in registers made opaque once (pk::opaque).
PW_FN uint32_t minu(uint32_t a, uint32_t b) { return __builtin_bit_cast(uint32_t, __builtin_elementwise_min(as_u2(a), as_u2(b))); }
PW_FN uint32_t maxu(uint32_t a, uint32_t b) { return __builtin_bit_cast(uint32_t, __builtin_elementwise_max(as_u2(a), as_u2(b))); }
// logical shift right per half by sh = (n, n) held in an opaque register
PW_FN uint32_t shru(uint32_t a, uint32_t sh) { return __builtin_bit_cast(uint32_t, (u2_t)(as_u2(a) >> as_u2(sh))); }
PW_FN uint32_t mad(uint32_t a, uint32_t b, uint32_t c) { return __builtin_bit_cast(uint32_t, (u2_t)(as_u2(a) * as_u2(b) + as_u2(c))); }
PW_FN uint32_t mins(uint32_t a, uint32_t b) { return __builtin_bit_cast(uint32_t, __builtin_elementwise_min(as_s2(a), as_s2(b))); }
PW_FN uint32_t align16(uint32_t hi, uint32_t lo) { return __builtin_amdgcn_alignbit(hi, lo, 16); }
// sign mask per half (0xffff where negative): arithmetic shift by sh15 = (15, 15) held in an opaque register
PW_FN uint32_t sign(uint32_t a, uint32_t sh15) { return __builtin_bit_cast(uint32_t, (s2_t)(as_s2(a) >> as_s2(sh15))); }
PW_FN uint32_t opaque(uint32_t v) { asm volatile("" : "+v"(v)); return v; }
PW_FN uint32_t opaque_su(uint32_t v) { asm volatile("" : "+s"(v)); return v; }   // a wave-uniform value, kept in a scalar register
PW_FN uint8_t* opaque_s(uint8_t* v) { asm volatile("" : "+s"(v)); return v; }   // a wave-uniform address, kept in scalar registers
// a copy of wave-uniform `src` into a scalar register of its own, in ONE statement with `pass`: what depends on `pass`
// afterwards comes behind the copy
PW_FN uint32_t copy_su(uint32_t src, uint32_t& pass) {
  uint32_t d;
  asm volatile("s_mov_b32 %0, %2" : "=&s"(d), "+s"(pass) : "s"(src));
  return d;
}
// 16 bytes to base + off in GLOBAL memory (an address that went through opaque_s has lost its address space, and a flat store
// would count against the scalar loads' counter as well)
PW_FN void store_global(uint8_t* base, uint32_t off, const U4& v) {
  typedef __attribute__((address_space(1))) uint8_t gbyte_t;
  typedef __attribute__((address_space(1))) U4 gu4_t;
  *(gu4_t*)((gbyte_t*)base + off) = v;
}
// v_perm_b32: byte i of the result is byte sel[i] of the 8 bytes {a (4 .. 7), b (0 .. 3)}; selector 8 .. 11 = the sign of
// byte 1 / 3 / 5 / 7 spread over the byte, 12 = 0x00, 13 and up = 0xff
PW_FN uint32_t perm(uint32_t a, uint32_t b, uint32_t sel) { return __builtin_amdgcn_perm(a, b, sel); }
#else
PW_FN uint32_t mk(uint32_t lo, uint32_t hi) { return (lo & 0xffffu) | (hi << 16); }
PW_FN int32_t sl(uint32_t v) { return (int16_t)(v & 0xffffu); }
PW_FN int32_t sh(uint32_t v) { return (int16_t)(v >> 16); }
PW_FN uint32_t add(uint32_t a, uint32_t b) { return mk((a & 0xffffu) + (b & 0xffffu), (a >> 16) + (b >> 16)); }
PW_FN uint32_t sub(uint32_t a, uint32_t b) { return mk((a & 0xffffu) - (b & 0xffffu), (a >> 16) - (b >> 16)); }
// add32's contract, checked here on the CPU only: no half of `a` lies in [0xff80, 0xffff] (b holds a byte per half, so no
// half carries into its neighbour).  Breaches are counted, not fatal: the CPU tests read and reset the count.
#if !defined(__HIPCC__)
inline unsigned& add32_breaches() { static unsigned n = 0; return n; }
PW_FN uint32_t add32(uint32_t a, uint32_t b) {
  if ((a & 0xffffu) >= 0xff80u || (a >> 16) >= 0xff80u) add32_breaches()++;
  return a + b;
}
#else
PW_FN uint32_t add32(uint32_t a, uint32_t b) { return a + b; }   // (the host pass of a device build: never run)
#endif
PW_FN uint32_t subsat(uint32_t a, uint32_t b) {
  const uint32_t al = a & 0xffffu, bl = b & 0xffffu, ah = a >> 16, bh = b >> 16;
  return mk(al > bl ? al - bl : 0u, ah > bh ? ah - bh : 0u);
}
PW_FN uint32_t max(uint32_t a, uint32_t b) { return mk((uint32_t)(sl(a) > sl(b) ? sl(a) : sl(b)), (uint32_t)(sh(a) > sh(b) ? sh(a) : sh(b))); }
PW_FN uint32_t minu(uint32_t a, uint32_t b) {
  const uint32_t al = a & 0xffffu, bl = b & 0xffffu, ah = a >> 16, bh = b >> 16;
  return mk(al < bl ? al : bl, ah < bh ? ah : bh);
}
PW_FN uint32_t mad(uint32_t a, uint32_t b, uint32_t c) {
  return mk((uint32_t)(sl(a) * sl(b) + sl(c)), (uint32_t)(sh(a) * sh(b) + sh(c)));
}
PW_FN uint32_t maxu(uint32_t a, uint32_t b) {
  const uint32_t al = a & 0xffffu, bl = b & 0xffffu, ah = a >> 16, bh = b >> 16;
  return mk(al > bl ? al : bl, ah > bh ? ah : bh);
}
PW_FN uint32_t shru(uint32_t a, uint32_t sh) { return mk((a & 0xffffu) >> (sh & 0xfu), (a >> 16) >> ((sh >> 16) & 0xfu)); }
PW_FN uint32_t mins(uint32_t a, uint32_t b) { return mk((uint32_t)(sl(a) < sl(b) ? sl(a) : sl(b)), (uint32_t)(sh(a) < sh(b) ? sh(a) : sh(b))); }
PW_FN uint32_t align16(uint32_t hi, uint32_t lo) { return (lo >> 16) | (hi << 16); }
PW_FN uint32_t sign(uint32_t a, uint32_t) { return mk(sl(a) < 0 ? 0xffffu : 0u, sh(a) < 0 ? 0xffffu : 0u); }
PW_FN uint32_t opaque(uint32_t v) { return v; }
PW_FN uint32_t opaque_su(uint32_t v) { return v; }
PW_FN uint8_t* opaque_s(uint8_t* v) { return v; }
PW_FN uint32_t copy_su(uint32_t src, uint32_t&) { return src; }
PW_FN void store_global(uint8_t* base, uint32_t off, const U4& v) { *(U4*)(base + off) = v; }
PW_FN uint32_t perm(uint32_t a, uint32_t b, uint32_t sel) {
  const uint64_t in = ((uint64_t)a << 32) | b;
  uint32_t r = 0;
  for (int i = 0; i < 4; i++) {
    const uint32_t c = (sel >> (8 * i)) & 0xffu;
    uint32_t v;
    if (c >= 13) v = 0xffu;
    else if (c == 12) v = 0u;
    else if (c >= 8) v = ((in >> (8 * (2 * (c - 8) + 1) + 7)) & 1u) ? 0xffu : 0u;
    else v = (uint32_t)(in >> (8 * c)) & 0xffu;
    r |= v << (8 * i);
  }
  return r;
}
#endif
PW_FN uint32_t both(int32_t v) { return ((uint32_t)v & 0xffffu) | ((uint32_t)v << 16); }
PW_FN uint32_t pack(int32_t lo, int32_t hi) { return ((uint32_t)lo & 0xffffu) | ((uint32_t)hi << 16); }
PW_FN int32_t lo_s(uint32_t v) { return (int32_t)(int16_t)(v & 0xffffu); }
PW_FN int32_t hi_s(uint32_t v) { return (int32_t)(int16_t)(v >> 16); }
}  // namespace pk
#if !defined(__HIPCC__)
// (the CPU emulator's library exports the count of pk::add32 contract breaches; reset = 1 clears it after reading)
extern "C" __attribute__((used, visibility("default"))) inline unsigned pw_pk_add32_breaches(int reset) {
  const unsigned n = pk::add32_breaches();
  if (reset) pk::add32_breaches() = 0;
  return n;
}
// Which body ran: blocks of one launch per kind of block (block16<EK>: 0 steady, 1 not started, 2 ended, 3 both), counted by
// lane 0 of the emulated wavefront or workgroup.  The emulator's harness fills FillParams without the planner, so the
// planner's ramp_free is handed to the lane program here: -1 as FillParams says, 0 / 1 for the launches that follow;
// PWLIB_RAMP_BLOCKS=1 turns it off as it does in the planner.
namespace pk {
inline unsigned* ramp_block_counts() { static unsigned n[4] = {0, 0, 0, 0}; return n; }
inline int& ramp_free_emu() { static int v = -1; return v; }
}  // namespace pk
extern "C" __attribute__((used, visibility("default"))) inline void pw_ramp_block_counts(unsigned* out, int reset) {
  for (int i = 0; i < 4; i++) { out[i] = pk::ramp_block_counts()[i]; if (reset) pk::ramp_block_counts()[i] = 0; }
}
extern "C" __attribute__((used, visibility("default"))) inline void pw_emu_ramp_free(int v) { pk::ramp_free_emu() = v; }
// The stamp group of the running best (WaveFill16, GRP) is a template constant on the device; the emulator's harness
// instantiates the five-argument form only, so here it is a run-time value: 4 runs the grouped form wherever the kernel's
// form allows it (WaveFill16::GOK, with ramp_free on), 1 or -1 the stamp per block.
namespace pk {
inline int& stamp_group_emu() { static int v = -1; return v; }
inline unsigned& group_stamps() { static unsigned n = 0; return n; }
}  // namespace pk
extern "C" __attribute__((used, visibility("default"))) inline void pw_emu_stamp_group(int v) { pk::stamp_group_emu() = v; }
// (the stamps written per group, counted by lane 0: one per four blocks and one for a last, shorter group)
extern "C" __attribute__((used, visibility("default"))) inline unsigned pw_group_stamps(int reset) {
  const unsigned n = pk::group_stamps();
  if (reset) pk::group_stamps() = 0;
  return n;
}
// The letter rings (WaveFill16, LDSF) are a template constant on the device too; here 1 runs them wherever the kernel's form
// allows it (WaveFill16::LOK, with ramp_free on), 0 or -1 the edge-lane feeders.  The emulated wavefront's LDS is the two
// rings below; a byte the restage step asks for outside its frame is counted with the feeders' breaches (pw_feed_breaches).
namespace pk {
inline int& lds_feed_emu() { static int v = -1; return v; }
inline unsigned& ring_restages() { static unsigned n = 0; return n; }
inline uint32_t* emu_ring() { static uint32_t r[2 * 528]; return r; }
}  // namespace pk
extern "C" __attribute__((used, visibility("default"))) inline void pw_emu_lds_feed(int v) { pk::lds_feed_emu() = v; }
// (the chunks of 64 letters staged, counted by lane 0: six in front of the loop and one per eight blocks run in full)
extern "C" __attribute__((used, visibility("default"))) inline unsigned pw_ring_restages(int reset) {
  const unsigned n = pk::ring_restages();
  if (reset) pk::ring_restages() = 0;
  return n;
}
// One running-best key per TWO cells (WaveFill16, PAIRK) is a template constant on the device as well; here 1 runs it wherever
// the grouped form runs (WaveFill16::grp4), 0 or -1 one key per cell.  finish() counts what it resolved: [slots resolved to the
// pair's first cell c, to its second cell c', the reported end cell resolved to c, to c'] -- slots that were stamped only.
namespace pk {
inline int& pair_keys_emu() { static int v = -1; return v; }
inline unsigned* pair_key_counts() { static unsigned n[4] = {0, 0, 0, 0}; return n; }
}  // namespace pk
extern "C" __attribute__((used, visibility("default"))) inline void pw_emu_pair_keys(int v) { pk::pair_keys_emu() = v; }
extern "C" __attribute__((used, visibility("default"))) inline void pw_pair_key_counts(unsigned* out, int reset) {
  for (int i = 0; i < 4; i++) { out[i] = pk::pair_key_counts()[i]; if (reset) pk::pair_key_counts()[i] = 0; }
}
// The packed kernels' edge-lane feeders, one pair per wavefront (WaveFill16::feed_issue): dwords the emulator's reader was
// asked for outside [0, wlast] of the frame it was reading (counted by every lane; must stay 0), and the blocks whose
// window took each path, counted by lane 0: [origin ahead, origin late, mutant ahead, mutant late].
namespace pk {
inline unsigned& feed_breaches() { static unsigned n = 0; return n; }
inline unsigned* feed_path_counts() { static unsigned n[4] = {0, 0, 0, 0}; return n; }
}  // namespace pk
extern "C" __attribute__((used, visibility("default"))) inline unsigned pw_feed_breaches(int reset) {
  const unsigned n = pk::feed_breaches();
  if (reset) pk::feed_breaches() = 0;
  return n;
}
extern "C" __attribute__((used, visibility("default"))) inline void pw_feed_path_counts(unsigned* out, int reset) {
  for (int i = 0; i < 4; i++) { out[i] = pk::feed_path_counts()[i]; if (reset) pk::feed_path_counts()[i] = 0; }
}
#endif

// The two offers of the packed kernels that cross lanes, one pair per wavefront.  Each is handed on where it is produced
// (TAKE = false: `own` goes to the neighbour, nothing is returned) and taken where it is consumed (TAKE = true): the register
// the cell pair reads, one half the lane's own value, the other half the neighbour's.
//   up offer:    (lane below's own.hi, own.lo)  -- handed on after the odd step, taken in front of the next even step
//   left offer:  (own.hi, next lane's own.lo)   -- handed on after the even step, taken in front of the odd step
// LDS = false: a DPP move into `carried`, whose edge lane (0 / 63) keeps what it held, and one v_alignbit.
// LDS = true (WaveFill16, XLDS; device only): no vector ALU work.  Two arrays of 64 + 1 dwords behind the letter rings,
// this lane's dword of the first at `xa`; the lane STORES its two halves where their readers want them -- ds_write_b16 and
// ds_write_b16_d16_hi, two halfwords side by side that straddle two dwords -- and takes its register as ONE aligned dword:
//   up:    own.lo -> high half of U[lane], own.hi -> low half of U[lane + 1];  taken: U[lane]      (U[0].lo: the seed)
//   left:  own.lo -> high half of L[lane], own.hi -> low half of L[lane + 1];  taken: L[lane + 1]  (L[64].hi: the seed)
// Every lane writes and reads its own words with its neighbour, 64 consecutive words: no bank conflict.  The workgroup is one
// wavefront and a wavefront's LDS operations complete in order, so a lane's read finds what the other lanes' stores of the same
// instruction left; the compiler sees plain stores and a load that may alias them and places the one wait the load needs.
// (The 16-bit LDS LOADS that write one half of a register and keep the other are not what this target gives: with SRAM ECC on
// they clear the other half, and the compiler never selects them for gfx950.  Stores have no such half to keep.)
static constexpr uint32_t kOfferWords = 65, kOfferLeft = 4u * kOfferWords;      // dwords per array; byte distance of L from U
template <class P, bool LDS, bool TAKE>
PW_FN uint32_t offer_up(uint32_t xa, uint32_t& carried, uint32_t own) {
  if constexpr (LDS) {
    if (TAKE) return P::lds_take32(xa);
    P::lds_put_halves(xa + 2u, own);
    return 0u;
  } else {
    if (TAKE) return pk::align16(own, carried);                 // (carried.hi, own.lo)
    carried = (uint32_t)P::shr1((int32_t)own, (int32_t)carried);
    return 0u;
  }
}
template <class P, bool LDS, bool TAKE>
PW_FN uint32_t offer_left(uint32_t xa, uint32_t& carried, uint32_t own) {
  if constexpr (LDS) {
    if (TAKE) return P::lds_take32(xa + kOfferLeft + 4u);
    P::lds_put_halves(xa + kOfferLeft + 2u, own);
    return 0u;
  } else {
    if (TAKE) return pk::align16(carried, own);                 // (own.hi, carried.lo)
    carried = (uint32_t)P::shl1((int32_t)own, (int32_t)carried);
    return 0u;
  }
}

// RULE selects the begin / end rules the kernel serves:
//   0  LOCAL / B_LOCAL            begin anywhere (B = 0 in every started cell), end = first best cell (tracked)
//   1  B_OVERLAP                  begin on the table edge (B = 0 only in the FIRST cell of a diagonal), end = the best
//                                 LAST cell of a diagonal
//   2  B_GLOBAL                   begin at (0, 0) only, end = cell (X, Y)
// Rules 1 and 2 have negative scores, so their sentinel is deeper (-24000; real scores stay within [-23000, 30000],
// see the host planner), the first diagonal above the band is silenced by clamping its offer (adding a second sentinel to a
// real score could wrap), every cell takes max(.., sentinel) -- which also pins cells before a diagonal's start and
// beyond its end -- and instead of tracking a best the value of each diagonal's last cell is captured.
//   4  END_ANCHORED (standard)   begin anywhere like rule 0 (scores >= 0, shallow sentinel), end = cell (X, Y): the last
//                                 cell of diagonal X - Y is captured, nothing is tracked
//   5  START_ANCHORED (standard) begin at (0, 0) only like rule 2 (negative scores, deep sentinel), end = the first best
//                                 cell anywhere, which must beat 0 (_pw_internals.c:342): the running best is tracked as a
//                                 key over max(H, 0), so real scores must stay within [-23000, 8000]
// CONTRACT of the plain (match / mismatch) form: letters outside a sequence never match, i.e. cells that have not started and
// cells beyond a diagonal's end take the MISMATCH score on their diagonal move -- which must be <= 0, or they creep up from
// the sentinel (the host planner admits the plain form only then; the matrix form scores such letters with the matrix minimum).
// MAT: the diagonal candidate takes its score from an integer substitution matrix of up to 4 x 4 letters instead of
// match / mismatch (_alnchoice_M, _pw_internals.c:217-245: subst_scores[o][m]).  The origin window then carries, per
// cell, the origin letter's ROW of the matrix -- four bytes subst[o][.] - min(subst) (times 4 under rule 3), at most 127
// each -- and the mutant window carries byte SELECTORS (0x0c00 | letter, + 4 in ONE half of a register, see FIXSEL): one
// v_perm_b32 looks up both cells of a pair.  Letters outside a sequence are the all-zero row / a selector that reads as
// 0x00: the matrix minimum, which the planner requires to be <= 0 ("matches nothing").
// GRP: the blocks per STAMP GROUP of the running best (1 or 4; stamp_best).  4 is a kernel of its own (k_fill16g) for the
// batches the planner's stamp_group (pw_plan.h) names; every other instantiation is the five-argument form.
// LDSF: the matrix rows and selector dwords of the letters are READ from two rings in LDS instead of travelling through the
// lanes (ring_read, restage); a kernel of its own (k_fill16l) for the batches the planner's lds_feed names.
// PAIRK: the running best takes ONE key per two consecutive cells of a slot, and finish() finds out which of the two held it
// (track_pair, second_of_pair); a kernel of its own (k_fill16p) for the batches the planner's pair_keys names.
// XLDS: the offers that cross lanes go through LDS instead of a DPP move and a v_alignbit each (offer_up, offer_left): bit 0 the
// up offer, bit 1 the left offer; a kernel of its own (k_fill16x) for the batches the planner's lds_exchange names.
template <class P, int BK, bool SEG, int RULE = 0, bool MAT = false, int GRP = 1, bool LDSF = false, bool PAIRK = false,
          int XLDS = 0>
struct WaveFill16 {
  // RULE 3 = rule 0 with every score held times 4 (admitted when the scores stay below 2048): a kept-or-not difference
  // of two running values is then 0 or at least 4, so min(x, 2) and min(x, 4) deliver the D and I tie bits already
  // weighted and the tie nibble is one three-operand add instead of two multiply-adds.
  static constexpr bool SC4 = RULE == 3;
  static constexpr int RL = SC4 ? 0 : RULE;
  static constexpr int SCL = SC4 ? 4 : 1;
  // what the rules are made of
  static constexpr bool ANYB = RL == 0 || RL == 4;   // an alignment may begin in every cell: scores >= 0, sentinel -8192
  static constexpr bool TRK = RL == 0 || RL == 5;    // the first best cell of every diagonal is tracked (as a key)
  static constexpr bool CAP = !TRK;                  // the value of every diagonal's last cell is captured instead
  static_assert(BK % 4 == 0, "packed layout needs an even number of cells per step");
  static constexpr int R = BK / 2;      // cells per lane and step
  static constexpr int RH = R / 2;      // packed registers per parity
#ifdef PW_FILL16_UNR
  static constexpr int UNR = PW_FILL16_UNR;                      // (A/B builds: build.py, PW_FILL16_UNR_OVERRIDE)
#else
  static constexpr int UNR = BK <= 8 ? 4 : (BK <= 16 ? 2 : 1);   // iterations unrolled per loop trip
#endif
  static constexpr int32_t NEG16 = ANYB ? -8192 : -24000;
  static constexpr uint32_t SENT_O = 0xfffeu, SENT_M = 0xffffu;   // letters outside a sequence: match nothing
  // MAT: selector codes of a mutant letter: 0x0c00 | letter reads the row that is v_perm_b32's second operand, + 4 the row
  // that is its first; outside the sequence the "letter" is 8, so the codes are 8 / 12, which both read as 0x00 under
  // either operand order (8 = the sign of a row byte, and row bytes stay below 128)
  static constexpr uint32_t MSEL = 0x0c00u, MOUT = 8u;
  // FIXSEL (two packed registers per parity, BK = 8): a mutant letter keeps ONE code all the way through the window.  A
  // letter walks MW[0].lo, MW[1].lo, MW[0].hi, MW[1].hi and on into the next lane's MW[0].lo, one place per iteration, so
  // the two letters of a register are always two iterations apart.  With the + 4 given once, to the letters fed on
  // iterations 2, 3 (mod 4) (sel4_fed), every register holds one code of each kind; which half holds the + 4 follows from
  // the iteration and the register alone (sel4_lo), and the cell pair passes the two rows to v_perm_b32 in that order.  The
  // iterations of a block are unrolled, so the order is fixed at compile time and nothing is left of the + 4 / - 4 that
  // otherwise repairs the spliced register on every iteration (MADJ).  Wider lanes (RH > 2) have letters RH iterations
  // apart and blocks that do not start on a multiple of 2 RH iterations: they keep the low half / high half codes and MADJ.
  static constexpr bool FIXSEL = MAT && RH == 2;
  PW_FN static uint32_t sel4_fed(int it) { return ((uint32_t)it >> 1) & 1u; }      // (it < 0: letters in the window at the start)
  PW_FN static bool sel4_lo(int k, int p) { return (((k + 7 - p) >> 1) & 1) != 0; }   // the low half of MW[p] on iteration k (mod 4)
  using Base = WaveFill<P, int32_t, BK, true, true, false>;       // only its static feeder helpers are used

  // SEG = true, lane packing: a wavefront holds `count` pairs side by side, `nl` lanes each (WaveDesc).
  // Everything that is per pair is then per LANE (pd is a per-lane copy); the DPP wave shifts still move
  // whole-wave, so the values that cross a pair boundary are replaced on the first / last lane of every
  // pair (sentinel offers, or the pair's own sequence feeder).
  // SEG = false: one pair per wavefront (wd.nl == 64); the descriptor is wave-uniform (scalar registers and
  // scalar loads) and the DPP `old` operand alone handles the two wave edges.
  const FillParams<int32_t>& a;
  const WaveDesc wd;
  PairDesc pd;
  int li;                               // lane within the pair
  bool valid, segfirst, seglast;
  int pair_slot;
  const uint8_t* oseq;
  const uint8_t* mseq;
  int X, Y, ndiag, owlast, mwlast, xfeed_o, yfeed_m;
  // the current block's 8 + 8 letters; the next block's raw dwords: the first, and the second and third as one 64-bit value
  // (what the two-dword load delivers; feed_commit shifts it in place)
  uint32_t fo_lo, fo_hi, fm_lo, fm_hi, fo_n0, fm_n0;
  uint64_t fo_n12, fm_n12;
  uint32_t fo_w, fm_w, fo_lim, fm_lim;  // !SEG: byte offset of the first dword of the block to come; the bound of the load ahead (feed_issue)

  // packed state: index p <-> even slots (2p, 2p + R) [E*] / odd slots (2p + 1, 2p + 1 + R) [O*]
  uint32_t HE[RH], UE[RH], LE[RH], HO[RH], UO[RH], LO[RH];
  // capturing rules: the value of every diagonal's last cell (bt unused); tracking rules: the running best lives in
  // kbE / kbO as a key and bt holds the stamp of where it was first reached (stamp_best)
  uint32_t bestE[RH], bestO[RH], btE[RH], btO[RH];
  uint32_t gebE[RH], gebO[RH];                          // ge (KEPT: + go) (+ the band-top block) per half
  uint32_t clE[RH], clO[RH];                            // RULE != 0: clamp of the "left" offer (sentinel for the slot above the band)
  uint32_t tfE[RH], tfO[RH], tlE[RH], tlO[RH];          // first / last step of each diagonal
  uint32_t accE[RH], accO[RH], acc2E[RH], acc2O[RH];    // tie nibbles, inverted unless KEPT: cells 0-3 / 4-7 of a block
  uint32_t OW[RH], MW[RH];
  uint32_t ROW[MAT ? R : 1];                            // MAT: the matrix row of every cell's origin letter
  uint32_t BIASV, MADJ;                                 // MAT: -min(subst) in both halves; the selector fix-up of the mutant window (!FIXSEL)
  uint32_t MR0, MR1, MR2, MR3;                          // MAT: the four rows of the matrix
  uint32_t ONE, SH15, C2, C4, C16, NDELTA, MATCHV, GOV, GOVI, NEGV, LIMV;
  // RULE 0, steady blocks: the running best of a slot as a key 8 H + (7 - cell within the block) -- one multiply-add and
  // one unsigned maximum per cell pair instead of maximum, compare, subtract and multiply-add (H <= 8191: the planner
  // admits scores up to 8000); carried from block to block and turned back into (best, step) once, in finish()
  uint32_t kbE[RH], kbO[RH], C8, SEVEN;
  // The two offers that cross lanes, as of the end of the previous exchange.  Only the DPP moves write them, and each move
  // takes the register's own previous value as its `old` operand: the edge lane that has no source (lane 0 / lane 63 of the
  // wavefront) keeps the sentinel it was given in run(), with no copy of the sentinel in front of every move.
  uint32_t up_prev;             // the lane below's last odd slot
  uint32_t left_next;           // the next lane's first even slot
  int phase_l, phase_r;         // LDS slot of the next exchange to the left / right (multi-wavefront platforms)
  // mask plane (pw_types.h, mask_word_index): this lane's dword in block 0 and the dwords per block -- the spare row and 0 for
  // lanes with nothing to store --, the spare row's first dword, the dwords per lane group
  uint32_t mrow0, mrow_step, mspare, mgroup;
  // The matrix form of the begin-anywhere rules runs one loop per kind of block (run()).  The match / mismatch form and the
  // rules that begin on the table edge keep the single loop that chooses a body per block: split, the former changes its
  // register profile (the BK = 8 body would fit one more wavefront per SIMD than build.py holds it to, a choice that wants
  // an A/B of its own), the latter lost wavefronts per SIMD or spilled scalar registers.
  static constexpr bool SPLIT = ANYB && MAT;
  // ... and, with every score held times 4, collects the tie bits as KEPT (1 = candidate kept), the form the plane stores: a
  // kept-or-not difference x is 0 or at least 4, so an unsigned saturating c - x is c where the candidate is kept and 0 where
  // not, for c = 1, 2, 4 -- the nibble's bits in place, and no "7 - nibble" per accumulator at the end of a block.  The gap
  // offers then start from (H + ge) + go and take go back where the same gap op is kept (run(): geb, GOV, GOVI); in 16-bit
  // wrap-around arithmetic that is the same value.
  static constexpr bool KEPT = SC4 && SPLIT;
  // ... and, one pair per wavefront, its mask stores take a wave-uniform base per lane group and one 32-bit byte offset per
  // lane.  (Elsewhere the BK / 4 addresses cost registers the body has no room for: the rules that begin on the table edge
  // spilled scalar registers, the match / mismatch body at 28 diagonals per lane lost its second wavefront per SIMD.)
  static constexpr bool SBASE = !SEG && SPLIT;
  // ... and, where the best is tracked (rules 0 and 3), takes the blocks in which diagonals start or end into the steady loop
  // when the planner says the scores allow it (pw_plan.h, ramp_free: the two proofs are there).  Then
  //   * the slots up to and including the first diagonal above the band start at H = 0 instead of the sentinel (run()): the
  //     cells before a diagonal's first stay exactly 0, so the steady body's saturating subtract (FLOOR0) and its 32-bit
  //     diagonal add hold from block 0 on.  Slot ndiag starts at 0 with them: the edge bodies lift it to 0 on step 0
  //     (tfirst_of), the steady body has no maximum with 0, and left at the sentinel it would take the band's offers
  //     H + ge + go -- small negative values, which the 32-bit add carries out of;
  //   * cells beyond a diagonal's end stay in the key (track_key<0> masks nothing): they hold less than the best;
  //   * the steady loop replaces the feed letters outside the sequences in EVERY block that is fed one (feed_commit), not
  //     only in the blocks in which diagonals start or end: a letter beyond a sequence's end is fed many blocks before the
  //     band's cells beyond the table read it -- the origin feed runs a whole wavefront of lanes ahead -- i.e. in blocks
  //     that are steady by the planner's bounds.  Left as loaded (a copy of the sequence's last letters) it would match,
  //     and a cell beyond a diagonal's end could then outscore the table.  The test is two scalar compares per block; the
  //     replacement itself, about 40 scalar instructions, runs only in the blocks that need it.
  // The three other loops stay for batches whose scores do not allow it.
  static constexpr bool RAMPF = SPLIT && TRK;
  // ... and, scores times 4, one pair per wavefront, 8 diagonals per lane, with ramp_free on, may stamp the running best once
  // per GROUP of four blocks (stamp_best).  On the device the group is the template constant and the grouped kernel is
  // launched for ramp_free batches only: it holds the steady loop alone.  The CPU emulator decides at run time
  // (pk::stamp_group_emu).
  static constexpr bool GOK = SC4 && SPLIT && TRK && !SEG && BK == 8;
  static_assert(GRP == 1 || (GRP == 4 && GOK), "a stamp group of 4: rule 3, matrix form, one pair per wavefront, 8 per lane");
#if defined(__HIPCC__)
  PW_FN static constexpr bool grp4() { return GRP == 4; }
#else
  bool grp4_rt = false;
  PW_FN bool grp4() const { return grp4_rt; }
#endif
  uint32_t kgE[RH], kgO[RH];    // grouped: the keys as they stood before the group
  uint32_t POS[8];              // grouped: 31 - cell within the group, in both halves, of the block's 8 iterations (wave-uniform)
  // PAIRK, one key per two cells (grouped form only).  The cells of iterations k and k + 1 (k even) of a slot are consecutive
  // cells c, c' of one diagonal; they share the key 8 max(H(c), H(c')) + (15 - pair within the group), taken on iteration
  // k + 1, where H(c) is still there as the cell pair's input: one signed maximum, one multiply-add and one unsigned maximum
  // per register and TWO iterations, against two multiply-adds and two unsigned maxima.  POS[0 .. 3] hold the codes of the
  // block's four pairs; the code takes four of the key's five low bits, so stamp_group reads key and stamp as before.
  // Which of the two cells held the maximum is lost, and recovered in finish() for the key that matters.  Let S > 0 be the best
  // score of the table, with ge < 0, go <= 0 and no substitution score 0 (the planner's pair_keys, pw_plan.h):
  //   * if H(c') = S, c' kept the diagonal move alone, on a substitution score s > 0: a kept D or I needs a predecessor of
  //     H >= S - ge > S, a kept B needs S = 0; so H(c) = S - s < S;
  //   * if c' kept the diagonal move alone on s > 0, then H(c') = H(c) + s > H(c) (no B kept: the floor at 0 did not act).
  // So where a pair's maximum is S, c' holds it iff the tie nibble of c' has none of B, D, I and the letters at c' score above
  // 0; otherwise c does, never both.  A slot whose own best is below S may resolve wrongly: it loses the end-cell search on its
  // score.  Cells before a diagonal's first and beyond its last hold less than S (pw_plan.h, ramp_free), so a pair that
  // straddles either end resolves to its in-table cell: letters outside a sequence score the matrix minimum, which is <= 0.
  static_assert(!PAIRK || (GRP == 4 && LDSF), "one key per two cells: the form of the kernel that reads its letters from LDS");
#if defined(__HIPCC__)
  PW_FN static constexpr bool pairk() { return PAIRK; }
#else
  PW_FN bool pairk() const { return pairk_rt; }
#endif
  // LDSF, letters from LDS.  What an iteration hands a lane -- the 4-byte matrix row of ONE origin letter (the new ROW[R - 1])
  // and the selector dword of ONE mutant letter (the new MW[0]: the letter's code in the low half, the code of the letter two
  // back in the high half; FIXSEL: a letter keeps one code, chosen by its index, sel4_fed) -- is a function of the sequences
  // alone.  The feeders rebuild both in scalar code block by block and the lanes pass them on, one DPP move and one copy of the
  // feed value each per iteration, plus the alignbit that splices the selector.  Here the wavefront keeps them EXPANDED in two
  // rings in LDS and every lane reads the two values it needs: one LDS read with an immediate offset each, no vector ALU work;
  // the lane exchanges shrink to the two offers.
  //   * ring offset u counts letters: origin letter e + u, mutant letter f - 256 + u (e, f: run()).  On iteration `it` lane l
  //     reads origin offset 4 l + 3 + it and mutant offset 256 - 4 l + it: a span of 256 offsets between lane 0 and lane 63.
  //   * a ring holds 512 offsets; offset u lives in slot s = u mod 512, word (s mod 4) * kRingRow + s / 4: four rows of 128
  //     words, so that the 64 lanes of a read, 4 slots apart, fall on 64 consecutive words (no bank conflict), each row with
  //     its first 4 words repeated behind it, so that a block's reads are immediates on ONE address per ring that moves on by
  //     two words per block and wraps with one AND (8 iterations reach at most 2 words past the row's end).
  //   * restaging, once per 8 blocks = 64 iterations = 64 letters per sequence (restage): behind the scalar branch of the
  //     stamp group, after the mask stores.  Lane l takes letter u0 + l of each sequence -- one byte load per sequence at a
  //     CLAMPED index (never a byte outside the frame), issued one section ahead and held in nx_o / nx_m --, expands it, with
  //     the letters outside a sequence replaced by the all-zero row / MOUT as feed_commit replaces them for ramp_free, and
  //     writes the row, the low half of its own selector dword and the high half of the dword two letters on.
  //   * at the start of section s (blocks 8 s ..) both rings hold offsets [64 s, 64 s + 384): the section reads origin offsets
  //     64 s + 3 .. 64 s + 318 and mutant offsets 64 s + 4 .. 64 s + 319.  The restage behind it writes [64 s + 384, 64 s + 448)
  //     (the selector's high halves up to 64 s + 449), slots that held offsets below 64 s - 62: read by nobody any more.
  // Runs where RAMPF does with ramp_free on (the steady loop alone; every letter outside a sequence replaced), one pair per
  // wavefront, 8 diagonals per lane.  On the device it is the template constant (k_fill16l); the CPU emulator decides at run time
  // (pk::lds_feed_emu) and may run it with either stamp group.
  static constexpr bool LOK = SPLIT && TRK && !SEG && BK == 8;
  static_assert(!LDSF || (LOK && GRP == 4), "letters from LDS: the grouped kernel's form");
  static constexpr int kRingRow = 132, kRingWords = 4 * kRingRow;      // words per row (128 + 4 repeated) and per ring
#if defined(__HIPCC__)
#define PW_IF_LDSF if constexpr (LDSF)
#else
  bool ldsf_rt = false;
#define PW_IF_LDSF if (ldsf_rt)
#endif
  // (the rings' per-lane state -- ring_h, ro, rm, nx_o, nx_m, fe, ff -- is declared at the end of the struct)
  // word c of the block's reads (the slot's distance from the lane's base, a constant in the unrolled block)
  PW_FN uint32_t ring_read(int which, uint32_t base, int c) const {
    const uint32_t w = (uint32_t)(which * kRingWords + (c & 3) * kRingRow + (c >> 2));
#if defined(__HIPCC__)
    return P::lds_read32(ring_h + base + 4u * w);
#else
    return pk::emu_ring()[w + (base >> 2)];
#endif
  }
  // half: -1 the whole word, 0 / 1 its low / high 16 bits
  PW_FN void ring_store(uint32_t w, uint32_t v, int half) {
#if defined(__HIPCC__)
    if (half < 0) P::lds_write32(ring_h + 4u * w, v);
    else P::lds_write16(ring_h + 4u * w + 2u * (uint32_t)half, v);
#else
    uint32_t& d = pk::emu_ring()[w];
    d = half < 0 ? v : (half == 0 ? ((d & 0xffff0000u) | (v & 0xffffu)) : ((d & 0xffffu) | (v << 16)));
#endif
  }
  PW_FN void ring_put(int which, uint32_t u, uint32_t v, int half) {
    const uint32_t s = u & 511u;
    const uint32_t w = (uint32_t)(which * kRingWords) + (s & 3u) * (uint32_t)kRingRow + (s >> 2);
    ring_store(w, v, half);
    if ((s >> 2) < 4u) ring_store(w + 128u, v, half);          // the row's first words again behind its end
  }
  PW_FN static void ring_sync() {
#if defined(__HIPCC__)
    P::lds_sync();
#else
    (void)P::shr1z(0);            // (the emulator's lanes meet at every exchange)
#endif
  }
  // letter idx of a frame of n letters, idx clamped into the frame (the CPU emulator counts a byte asked for outside it)
  PW_FN static uint32_t ring_letter(const uint8_t* seq, int idx, int n) {
    const int c = pw_clampi(idx, 0, n > 0 ? n - 1 : 0);
#if !defined(__HIPCC__)
    if (c < 0 || c >= (n > 0 ? n : 1)) { pk::feed_breaches()++; return 0xa5u; }
#endif
    return (uint32_t)seq[c];
  }
  PW_FN void stage_issue(int u0) {
    const int u = u0 + P::lane();
    nx_o = ring_letter(oseq, fe + u, X); nx_m = ring_letter(mseq, ff - 256 + u, Y);
  }
  PW_FN void stage_commit(int u0) {
#if !defined(__HIPCC__)
    if (P::lane() == 0) pk::ring_restages()++;                 // (the CPU emulator: chunks staged)
#endif
    const int u = u0 + P::lane();
    const uint32_t row = (uint32_t)(fe + u) < (uint32_t)X ? row_of(nx_o) : 0u;
    const uint32_t code = MSEL | (((uint32_t)(ff - 256 + u) < (uint32_t)Y ? nx_m : MOUT) + 4u * sel4_fed(u));   // (256 = 0 mod 4)
    ring_put(0, (uint32_t)u, row, -1);
    ring_put(1, (uint32_t)u, code, 0);
    ring_put(1, (uint32_t)u + 2u, code, 1);
  }
  // in front of the block loops: offsets [0, 384) of both rings, the loads of the first restage, the lanes' addresses
  PW_FN void ring_begin() {
#pragma unroll 1
    for (int c = 0; c < 6; c++) { stage_issue(64 * c); stage_commit(64 * c); }
    ring_sync();
    stage_issue(384);
    ro = 4u * (uint32_t)li; rm = 4u * (uint32_t)(64 - li);
  }
  // XLDS, in front of the block loops: the lane's address, and both arrays as the DPP moves' registers stand before the first
  // exchange -- U[0].lo is lane 0's up_prev, which no move ever writes, L[64].hi lane 63's left_next likewise (whole dwords
  // from every lane: the other halves are stored over before anyone reads them); then the up offer of iteration 0, which the
  // loop hands on at the end of the iteration before: every lane's UO[RH - 1] as it starts, whose high half is up_prev's.
  static constexpr bool XUP = (XLDS & 1) != 0, XLEFT = (XLDS & 2) != 0;
  static_assert(XLDS == 0 || (LDSF && XLDS <= 3), "offers through LDS: the form of the kernel that reads its letters from LDS");
  PW_FN void offers_begin() {
    if constexpr (XLDS != 0) {
      xch_a = ring_h + 4u * (uint32_t)(2 * kRingWords) + 4u * (uint32_t)P::lane();
      if (XUP) { P::lds_put32(xch_a, up_prev >> 16); offer_up<P, true, false>(xch_a, up_prev, UO[RH - 1]); }
      if (XLEFT) P::lds_put32(xch_a + kOfferLeft + 4u, left_next << 16);
    }
  }
  // behind the last block of section s
  PW_FN void restage(int s) {
    stage_commit(64 * s + 384);
    ring_sync();
    stage_issue(64 * s + 448);
  }
  // One pair per wavefront, matrix form, blocks unrolled in full: the rows of a block's 8 origin feed letters are selected
  // when the block starts (feed_commit), on bits read in place (row_bits) -- wave-uniform, scalar registers.
  static constexpr bool FROWS = MAT && !SEG && UNR == 4 && BK <= 8;
  uint32_t frow[FROWS ? 8 : 1];
  bool rf;                      // RAMPF and the planner's ramp_free
  uint32_t flimx, flimy;        // RAMPF: max(length - 7, 0) of each sequence (blocks_step)
  uint32_t mrowb;              // SBASE: the byte offset of this lane's dwords in the block to come
  uint8_t* mbase[BK / 4];       // SBASE: the plane's address plus the distance of lane group g

  PW_FN WaveFill16(const FillParams<int32_t>& a_, const WaveDesc& wd_) : a(a_), wd(wd_) {}

  // Two cells at once.  `acc` collects the INVERTED tie bits (1 = candidate not kept; KEPT: the bits themselves), 4 bits per
  // cell: bit 0 B, bit 1 D, bit 2 I; bit 3 (M) stays 0 -- with go <= 0 the walker never needs it: the first
  // kept op is M exactly when none of B, D, I is kept (pw_first_op).
  //
  // EDGE = false: steady phase, every in-band diagonal holds an in-table cell.
  // EDGE = true : blocks in which diagonals start or end.  No state is frozen; instead
  //   * a diagonal that has not started yet (cells with a negative coordinate) may not begin an alignment:
  //     its B candidate is the sentinel instead of 0.  Such cells have only sentinels as predecessors and
  //     letters outside the sequences match nothing, so they stay at the sentinel and in-table cells
  //     never pick them;
  //   * a diagonal that has ended keeps computing cells beyond the table; nothing in the table reads them
  //     (predecessors have smaller coordinates), their tie nibbles land in mask slots the walker never
  //     visits, and they are kept out of the running best by lowering them by 32767 first.
  // For RULE != 0: `bests` holds the captured value of the diagonal's LAST cell, `bts` is unused, `tf` is the step of
  // the one cell that may begin an alignment (32767 = none), `geb` is ge in both halves and `clampL` silences the
  // first diagonal above the band.
  // EK: 0 steady; bit 0: some diagonal of the wavefront has not started yet in this block; bit 1: some has ended (rules
  // 1 / 2 know steady and "edge" = 3 only).
  template <int EK>
  PW_FN void cellpair(uint32_t& Hs, uint32_t& Us, uint32_t& Ls, uint32_t& bests, uint32_t& bts, uint32_t geb,
                      uint32_t tf, uint32_t tl, uint32_t& acc, uint32_t up, uint32_t left, uint32_t oc,
                      uint32_t mc, uint32_t tv, uint32_t clampL = 0, uint32_t och = 0, bool lo4 = false) {
    constexpr bool EDGE = EK != 0;
    uint32_t hM;
    // (MAT, begin-anywhere rules outside the blocks where diagonals start: a started cell's score is never negative, so the
    //  bias comes off with an unsigned SATURATING subtract -- the diagonal candidate is max(H + subst, 0) already and the
    //  maximum with the begin candidate 0 below is not needed: one op less per cell pair.  Cells that have not started hold
    //  the sentinel, a large unsigned value that the subtract leaves alone.)
    constexpr bool FLOOR0 = MAT && ANYB && (EK & 1) == 0;
    if (MAT) {
      // oc / och: the matrix rows of the low / high cell's origin letter, mc: the two selectors; lo4 (FIXSEL): the low
      // half's selector is the one that carries the + 4
      //
      // Begin-anywhere rules: the diagonal add is a plain 32-bit add (v_add_u32, the 2-cycle issue class, instead of
      // v_pk_add_u16).  INVARIANT: no half of H lies in [0xff80, 0xffff] on entry; the addend is a row byte, 0 .. 127, in each
      // half, so no half carries into its neighbour and the bits are the packed add's.  A half of H is one of
      //   * a started cell's score, or a cell's beyond its diagonal's end: 0 .. 8191 -- admit_packed (pw_plan.h) holds
      //     min(X, Y) * max(subst) to 8000, to 2047 times 4 in the scores-times-4 form, and letters outside a sequence score
      //     the matrix minimum, which packed_matrix_bytes_ok requires to be <= 0; with ramp_free (RAMPF) also a cell before
      //     its diagonal's first: exactly 0;
      //   * the first diagonal above the band (slot ndiag): begins at step 0 (tfirst_of), so it is 0 .. 8191 like a started
      //     cell from its first update on.  (Left at the sentinel it took the in-band offers H + ge + go, small negative
      //     values, and carried into the slot it shares a register with.)  Its offers go out 8192 lower (blocked), below every
      //     started cell as before;
      //   * a cell that has not started, a slot further above the band, a lane without a pair: the sentinel -8192 plus what
      //     the substitutions of at most min(X, Y) in-table cells add, or an offer that came through slot ndiag -- at most
      //     8000 - 8192 = -192, i.e. 0xff40.  A positive mismatch score cannot lift them further: admit_packed sends such
      //     scores to this form, whose off-sequence letters score <= 0 (the creep commit 78c26ef bounded).  From below they
      //     are held by the maximum with the sentinel in the blocks where diagonals start, and elsewhere by the offers of
      //     their neighbours: slot ndiag + k stays at or above -8192 - k |go + ge|.  The planner's layouts leave at most 255
      //     spare slots and |go + ge| <= 100, so only the last ten of them could fall past -32768 and wrap round to this
      //     range, and only with every substitution on the way at -100 too; a layout forced wider (PWLIB_PACKED_BK) can.
      //     What then carries is one spare slot into another: the band reads neither except through slot ndiag's offers.
      // The rules that begin on the table edge hold negative scores: they keep the packed add.  The CPU emulation of
      // pk::add32 counts every breach of the invariant.
      const uint32_t sub2 = lo4 ? pk::perm(oc, och, mc) : pk::perm(och, oc, mc);
      const uint32_t hb = ANYB ? pk::add32(Hs, sub2) : pk::add(Hs, sub2);
      hM = FLOOR0 ? pk::subsat(hb, BIASV) : pk::sub(hb, BIASV);
    } else {
      const uint32_t ne = pk::minu(oc ^ mc, ONE);               // 0 where the letters match
      hM = pk::add(Hs, pk::mad(ne, NDELTA, MATCHV));
    }
    uint32_t Hn = pk::max(pk::max(up, left), hM);
    uint32_t nB;
    if (ANYB) {
      if (EK & 1) Hn = pk::max(Hn, pk::sign(pk::sub(tv, tf), SH15) & NEGV);   // B = 0 once started, sentinel before
      else if (!FLOOR0) Hn = pk::max(Hn, 0u);                    // B: an alignment may begin anywhere, score 0
      nB = KEPT ? pk::subsat(ONE, Hn) : pk::minu(Hn, ONE);       // (KEPT: a sentinel is a large unsigned value -- not kept)
    } else {
      // B = 0 in the one cell that may begin (step tf), the sentinel everywhere else
      const uint32_t Bc = EDGE ? pk::mad(pk::minu(tv ^ tf, ONE), NEGV, 0u) : NEGV;
      Hn = pk::max(Hn, Bc);
      nB = pk::minu(Hn ^ Bc, ONE);
    }
    // "is the candidate kept" only asks whether H == candidate: xor (a 2-cycle op) instead of a packed subtract
    const uint32_t nD = KEPT ? pk::subsat(C2, Hn ^ up) : pk::minu(Hn ^ up, SC4 ? C2 : ONE);       // SC4: 0 or 2
    const uint32_t nI = KEPT ? pk::subsat(C4, Hn ^ left) : pk::minu(Hn ^ left, SC4 ? C4 : ONE);   // SC4: 0 or 4
    const uint32_t hg = pk::add(Hn, geb);
    Us = pk::mad(nD, GOV, hg);                                   // (H + ge) + go unless a D choice is kept
    Ls = pk::mad(nI, GOVI, hg);
    if (!ANYB) Ls = pk::mins(Ls, clampL);
    // nibble = nB + 2 nD + 4 nI, appended to the accumulator: three packed multiply-adds
    if (SC4) acc = pk::mad(acc, C16, nB + nD + nI);             // (halves below 8: a plain 32-bit three-operand add)
    else acc = pk::mad(acc, C16, pk::mad(nI, C4, pk::mad(nD, C2, nB)));
    if (TRK) {
      // (the running best is kept as a key by iteration16)
    } else if (EK & 2) {
      const uint32_t e = pk::minu(tv ^ tl, ONE);                 // 0 in the diagonal's last cell
      bests = pk::mad(e, pk::sub(bests, Hn), Hn);                // e ? bests : Hn
    }
    Hs = Hn;
  }

  // The running best stays a key from block to block (kbE / kbO), with no re-seeding: a block goes on taking maxima into the
  // key as it stands (`kb0` = its value before the block).  What a block leaves behind besides the key is a STAMP of where the
  // best was first reached, 8 (block + 1) + 7 - cell, written only where the key's SCORE part (bits 3 and up) rose in this
  // block: the low bits are then 7 - the first cell of the block that reached the new score.  An equal score in a later
  // block can only raise the low bits; that is not a rise of the score part, no stamp is written, and the low bits are never
  // read again until the score part rises (which rewrites them).  Stamps only grow from block to block, so an unsigned
  // maximum keeps the latest; where the score did not rise the candidate is 0 * stamp + (0 .. 7), below every real stamp.
  // finish() turns key and stamp into score and step, once per pair.
  PW_FN void stamp_best(uint32_t& bts, uint32_t kb, uint32_t kb0, uint32_t blk8) {
    const uint32_t ch = pk::minu((kb ^ kb0) & ~SEVEN, ONE);      // 1 where the best strictly improved in this block
    bts = pk::maxu(bts, pk::mad(ch, blk8, kb & SEVEN));
  }
  // Grouped (grp4): the key is 8 H + (31 - cell within the GROUP of four blocks), H = 4 score <= 8188 under the times-4
  // admission (min(X, Y) max(subst) <= 2047), so 8 * 8188 + 31 = 65535 fills the 16 bits exactly; the score part is bits 5
  // and up, `kg` the key before the group, and the stamp 32 (group + 1) + 31 - cell -- at most 32 * 1024 + 31 for 4096
  // blocks -- is written once per group, behind a scalar branch (block16), and once more behind the loop for a last group of
  // fewer than four blocks (run()).  An equal score later never wins, for the reasons above restated for groups: within a
  // group a later cell has a smaller position code, so the unsigned maximum keeps the first; in a later group an equal score
  // can only raise the low bits; the low bits are read only in a group whose score part rose (ch = 1); and the key that made
  // it rise rewrote them with its own code, after which only smaller codes follow at that score in the group.  Stamps grow
  // from group to group; the candidate where nothing rose is 0 .. 31, below every real stamp.
  PW_FN void stamp_group(uint32_t g1) {
#if !defined(__HIPCC__)
    if (P::lane() == 0) pk::group_stamps()++;                 // (the CPU emulator: the grouped form ran)
#endif
    const uint32_t sv = pk::both((int32_t)(32u * g1));
#pragma unroll
    for (int p = 0; p < RH; p++) {
      const uint32_t chE = pk::minu((kbE[p] ^ kgE[p]) & 0xffe0ffe0u, ONE), chO = pk::minu((kbO[p] ^ kgO[p]) & 0xffe0ffe0u, ONE);
      btE[p] = pk::maxu(btE[p], pk::mad(chE, sv, kbE[p] & 0x001f001fu));
      btO[p] = pk::maxu(btO[p], pk::mad(chO, sv, kbO[p] & 0x001f001fu));
      kgE[p] = kbE[p]; kgO[p] = kbO[p];
    }
  }

  // HALF selects the accumulator set: iterations 0-3 of a block (cells 0-3 of every slot) or 4-7.
  // Rule 0: the slot's running best as a key (see kbE): cells of a diagonal that has not started hold the sentinel and
  // count as 0, cells beyond a diagonal's end are masked out -- neither can beat 8 best + 7.
  template <int EK>
  PW_FN void track_key(uint32_t& kb, uint32_t H, uint32_t tl, uint32_t tv, int k) {
    const uint32_t hk = (!ANYB || (EK & 1)) ? pk::max(H, 0u) : H;   // (rule 5: real scores go negative and count as 0)
    uint32_t key = grp4() ? pk::mad(hk, C8, POS[k]) : pk::mad(hk, SC4 ? C2 : C8, pk::both(7 - k));
    if (EK & 2) key &= ~pk::sign(pk::sub(tl, tv), SH15);
    kb = pk::maxu(kb, key);
  }
  // PAIRK, iteration k odd: `H0` is the slot's cell of iteration k - 1, `H` the one of iteration k (steady body only)
  PW_FN void track_pair(uint32_t& kb, uint32_t H0, uint32_t H, int k) {
    kb = pk::maxu(kb, pk::mad(pk::max(H0, H), C8, POS[(k >> 1) & 3]));
  }

  template <int EK, int HALF>
  PW_FN void iteration16(int it, int k) {
    constexpr bool EDGE = EK != 0;
    const uint32_t tv0 = pk::both(2 * it), tv1 = pk::both(2 * it + 1);
    // even step: slot 0 <- previous lane's last slot, slot R <- own slot R - 1
    {
      // (the lane below's last odd slot: moved at the end of the previous iteration, together with the mutant window)
      uint32_t prev = up_prev;
      if (SEG) prev = segfirst ? NEGV : prev;
      const uint32_t up0 = offer_up<P, XUP, true>(xch_a, prev, UO[RH - 1]);         // (prev.hi, own.lo)
#pragma unroll
      for (int p = 0; p < RH; p++)
      {
        const uint32_t h0 = HE[p];
        cellpair<EK>(HE[p], UE[p], LE[p], bestE[p], btE[p], gebE[p], tfE[p], tlE[p], HALF == 0 ? accE[p] : acc2E[p],
                     p == 0 ? up0 : UO[p == 0 ? 0 : p - 1], LO[p], MAT ? ROW[MAT ? p : 0] : OW[p], MW[p], tv0, clE[p],
                     MAT ? ROW[MAT ? p + RH : 0] : 0u, FIXSEL && sel4_lo(k, p));
        if (TRK) {
          if (pairk()) { if (k & 1) track_pair(kbE[p], h0, HE[p], k); }
          else track_key<EK>(kbE[p], HE[p], tlE[p], tv0, k);
        }
      }
    }
    // origin window moves on: last register <- (own first.hi, next lane's first.lo | the pair's feeder).
    // Only cells outside the table read letters outside a sequence; in steady blocks those are out-of-band
    // slots whose values nobody reads, so the range check is needed in EDGE blocks only.
    // The letter and the left offer of the odd step travel the same way: ONE exchange (platforms whose shifts cross
    // wavefronts through LDS pay one barrier for the pair).
    PW_IF_LDSF {
      // letters from LDS: only the left offer crosses lanes; the row of the letter that enters the window is read
      offer_left<P, XLEFT, false>(xch_a, left_next, LE[0]);
      const uint32_t nxt = ring_read(0, ro, 3 + k);
#pragma unroll
      for (int i = 0; i + 1 < (MAT ? R : 1); i++) ROW[i] = ROW[i + 1];
      ROW[MAT ? R - 1 : 0] = nxt;
    } else {
      // (MAT: feed_commit has already turned the letters outside the sequence into 0xff, whose row is 0 -- no range check
      //  here: on a wave-uniform feed it compiled to a branch per iteration, which serialises the packed ops)
      const int oi = xfeed_o + it;
      const uint32_t fb = Base::feed_byte(fo_lo, fo_hi, k);
      uint32_t feed = (!EDGE || (uint32_t)oi < (uint32_t)X) ? fb : SENT_O;
      if (MAT) feed = FROWS ? frow[FROWS ? k : 0] : row_of(fb);
      int32_t mv[2] = {(int32_t)(MAT ? ROW[0] : OW[0]), (int32_t)LE[0]};
      const int32_t mo[2] = {(int32_t)feed, (int32_t)left_next};
      xshlv<P, 2>(mv, mo, phase_l); phase_l ^= 1;
      uint32_t nxt = (uint32_t)mv[0];
      left_next = (uint32_t)mv[1];
      if (SEG) nxt = seglast ? feed : nxt;
      if (MAT) {
        // whole registers: the window of rows moves on by renaming
#pragma unroll
        for (int i = 0; i + 1 < (MAT ? R : 1); i++) ROW[i] = ROW[i + 1];
        ROW[MAT ? R - 1 : 0] = nxt;
      } else {
        const uint32_t last = pk::align16(nxt, OW[0]);
#pragma unroll
        for (int p = 0; p + 1 < RH; p++) OW[p] = OW[p + 1];
        OW[RH - 1] = last;
      }
    }
    // odd step: slot BK - 1 <- next lane's slot 0, slot R - 1 <- own slot R
    {
      uint32_t nxt = left_next;
      if (SEG) nxt = seglast ? NEGV : nxt;
      const uint32_t leftl = offer_left<P, XLEFT, true>(xch_a, nxt, LE[0]);              // (own.hi, next.lo)
#pragma unroll
      for (int p = 0; p < RH; p++)
      {
        const uint32_t h0 = HO[p];
        cellpair<EK>(HO[p], UO[p], LO[p], bestO[p], btO[p], gebO[p], tfO[p], tlO[p], HALF == 0 ? accO[p] : acc2O[p],
                     UE[p], p == RH - 1 ? leftl : LE[p == RH - 1 ? p : p + 1], MAT ? ROW[MAT ? p : 0] : OW[p], MW[p], tv1, clO[p],
                     MAT ? ROW[MAT ? p + RH : 0] : 0u, FIXSEL && sel4_lo(k, p));
        if (TRK) {
          if (pairk()) { if (k & 1) track_pair(kbO[p], h0, HO[p], k); }
          else track_key<EK>(kbO[p], HO[p], tlO[p], tv1, k);
        }
      }
    }
    // mutant window moves on: first register <- (previous lane's last.hi | the pair's feeder, own last.lo)
    PW_IF_LDSF {
      // letters from LDS: only the up offer crosses lanes; the first register's new value is read whole
      offer_up<P, XUP, false>(xch_a, up_prev, UO[RH - 1]);
      const uint32_t first = ring_read(1, rm, k);
#pragma unroll
      for (int p = RH - 1; p > 0; p--) MW[p] = MW[p - 1];
      MW[0] = first;
    } else {
      const int mi = yfeed_m + it;
      const uint32_t fbm = Base::feed_byte(fm_lo, fm_hi, k);
      // (MAT: the letter arrives in a high half and is moved to the low half of the first register below: high-half code,
      //  which MADJ repairs -- or, FIXSEL, the code it keeps; feed_commit has turned the letters outside the sequence into
      //  MOUT, so their codes are 8 / 12 by the same rule)
      const uint32_t feed = (MAT ? (MSEL | (fbm + 4u * (FIXSEL ? sel4_fed(k) : 1u)))
                                 : ((!EDGE || (uint32_t)mi < (uint32_t)Y) ? fbm : SENT_M)) << 16;
      // ... together with the up offer of the next iteration's even step (one exchange)
      int32_t mv[2] = {(int32_t)MW[RH - 1], (int32_t)UO[RH - 1]};
      const int32_t mo[2] = {(int32_t)feed, (int32_t)up_prev};
      xshrv<P, 2>(mv, mo, phase_r); phase_r ^= 1;
      uint32_t prv = (uint32_t)mv[0];
      up_prev = (uint32_t)mv[1];
      if (SEG) prv = segfirst ? feed : prv;
      uint32_t first = pk::align16(MW[RH - 1], prv);
      // MAT: what moved from a high half into the low one sheds its + 4, what moved from a low half into the high one gains
      // it (one 32-bit add: no half borrows, codes are 4 .. 12 in the low half here); FIXSEL: codes stay as they are
      if (MAT && !FIXSEL) first += MADJ;
#pragma unroll
      for (int p = RH - 1; p > 0; p--) MW[p] = MW[p - 1];
      MW[0] = first;
    }
  }

  template <int EK>
  PW_FN void block16(int b) {
#if !defined(__HIPCC__)
    if (P::lane() == 0) pk::ramp_block_counts()[EK]++;       // (the CPU emulator: which body ran)
#endif
#pragma unroll
    for (int p = 0; p < RH; p++) { accE[p] = 0; accO[p] = 0; acc2E[p] = 0; acc2O[p] = 0; }
    uint32_t kb0E[RH], kb0O[RH];
    if (TRK && !grp4()) {
#pragma unroll
      for (int p = 0; p < RH; p++) { kb0E[p] = kbE[p]; kb0O[p] = kbO[p]; }
    }
    // unroll depth: full for narrow lanes (the letter-window shifts become register renames), shallower for
    // wide ones, where the live state already fills the register file
#pragma clang loop unroll_count(UNR)
    for (int k = 0; k < 4; k++) iteration16<EK, 0>(8 * b + k, k);
#pragma clang loop unroll_count(UNR)
    for (int k = 4; k < 8; k++) iteration16<EK, 1>(8 * b + k, k);
    if (TRK && !grp4()) {
      const uint32_t blk8 = pk::both(8 * b + 8);
#pragma unroll
      for (int p = 0; p < RH; p++) {
        stamp_best(btE[p], kbE[p], kb0E[p], blk8);
        stamp_best(btO[p], kbO[p], kb0O[p], blk8);
      }
    }
    // 8 cells per slot -> one dword, first cell in the top nibble; un-invert: kept = 7 - (not kept), one subtract per
    // accumulator for both slots it holds (every nibble is at most 7: no borrows) -- KEPT: as collected.  Slots are gathered into their natural
    // order -- one v_perm_b32 per dword -- so that every group of 4 goes out as one 16-byte store.
    // Lanes with nothing to store (padding lanes, lanes beyond the plane's rows, blocks past the pair's last)
    // write into the plane's spare row (row `nblocks`, slot 0) instead of branching: a branch here splits the
    // unrolled block and serialises the packed ops (dependent VOP3P ops need a wait state between them).
    {
      uint32_t mwd[BK];
#pragma unroll
      for (int p = 0; p < RH; p++) {
        const uint32_t inv = KEPT ? 0u : 0x77777777u;
        const uint32_t kE = KEPT ? accE[p] : inv - accE[p], k2E = KEPT ? acc2E[p] : inv - acc2E[p];
        const uint32_t kO = KEPT ? accO[p] : inv - accO[p], k2O = KEPT ? acc2O[p] : inv - acc2O[p];
        mwd[2 * p] = pk::perm(kE, k2E, 0x05040100u);           // (kE.lo, k2E.lo)
        mwd[2 * p + R] = pk::perm(kE, k2E, 0x07060302u);       // (kE.hi, k2E.hi)
        mwd[2 * p + 1] = pk::perm(kO, k2O, 0x05040100u);
        mwd[2 * p + 1 + R] = pk::perm(kO, k2O, 0x07060302u);
      }
      if (!SBASE) {
        // mask_word_index(BK, nl, b, li, 4 g), or the spare row: a 32-bit dword index (run(): mrow0 / mrow_step / mspare); a
        // shorter pair of a lane-packed wavefront parks its stores in the spare row once its own blocks are done
        const uint32_t row = b < pd.nblocks ? mrow0 + (uint32_t)b * mrow_step : mspare;
        uint32_t* dst = a.masks + pd.mask_off;
#pragma unroll
        for (int g = 0; g < BK / 4; g++) {
          U4 v; v.x = mwd[4 * g]; v.y = mwd[4 * g + 1]; v.z = mwd[4 * g + 2]; v.w = mwd[4 * g + 3];
          *(U4*)(dst + (row + (uint32_t)g * mgroup)) = v;
        }
      } else {
        // One pair per wavefront runs exactly the pair's blocks (nblocks_run()), so no block is tested against the pair's
        // count; the lane's BYTE offset into the pair's plane is carried from block to block -- one add -- and the lane
        // group's distance sits in the wave-uniform base (mbase[g]): a store takes a scalar base and this one 32-bit
        // register, with no 64-bit address arithmetic per lane.  (A plane stays far below 4 GiB: at most 4096 blocks of
        // 512 lanes x 32 dwords.)
#pragma unroll
        for (int g = 0; g < BK / 4; g++) {
          U4 v; v.x = mwd[4 * g]; v.y = mwd[4 * g + 1]; v.z = mwd[4 * g + 2]; v.w = mwd[4 * g + 3];
          pk::store_global(mbase[g], mrowb, v);
        }
        mrowb += 4u * mrow_step;
      }
    }
    // Grouped: the position codes move on by a block (scalar registers); the last block of a group stamps, takes the keys as
    // the next group's "before" and starts the codes again -- behind ONE scalar branch, after the mask stores, so that the
    // unrolled body stays one basic block.
    if (TRK && grp4()) {
      // (PAIRK: four codes, 15 - pair within the group -- four pairs per block, sixteen per group)
      if (pairk()) {
#pragma unroll
        for (int k = 0; k < 4; k++) POS[k] -= 0x00040004u;
      } else {
#pragma unroll
        for (int k = 0; k < 8; k++) POS[k] -= 0x00080008u;
      }
      if ((b & 3) == 3) {
        stamp_group((uint32_t)(b >> 2) + 1u);
        if (pairk()) {
#pragma unroll
          for (int k = 0; k < 4; k++) POS[k] += 0x00100010u;
        } else {
#pragma unroll
          for (int k = 0; k < 8; k++) POS[k] += 0x00200020u;
        }
        PW_IF_LDSF { if ((b & 7) == 7) restage(b >> 3); }      // (the same branch serves both)
      }
    } else PW_IF_LDSF {
      if ((b & 7) == 7) restage(b >> 3);
    }
    // letters from LDS: both ring addresses move on by a block -- 8 slots, two words of a row
    PW_IF_LDSF { ro = (ro + 8u) & 511u; rm = (rm + 8u) & 511u; }
  }

  // One pair per wavefront (or workgroup): the indices are wave-uniform -- scalar loads, which leave vmcnt to the mask stores.
  // A block consumes 8 letters, so its 3-dword window (words w, w + 1, w + 2 of the frame, each clamped to 0 .. wlast) moves
  // on by exactly 2 dwords per block: the first word of a block's window IS the last word of the block before, clamped or
  // not.  The window's place is carried as a byte offset (fw = 4 w, + 8 per block), and
  //   * where the other two words are unclamped -- 0 <= w and w + 2 <= wlast, i.e. fw < 4 max(wlast - 1, 0) as UNSIGNED
  //     numbers (a negative offset is a huge one) -- they are loaded ONE BLOCK AHEAD by one two-dword load at an offset held
  //     in a scalar register (feed_issue), against three loads with a clamp and a 64-bit address each.  The load reads words
  //     w + 1 and w + 2 <= wlast: never a dword outside the frame's own (a caller-owned arena has nothing behind its last
  //     frame but 16 bytes of slack).  A frame of fewer than 3 dwords never qualifies;
  //   * elsewhere the block that needs the words fetches them itself, when it starts (feed_late, behind a branch in front of
  //     the body): the three clamped loads -- or, where the window lies past the frame's end or before its start altogether
  //     (w >= wlast or w + 2 <= 0), no load: all three words are the word carried over.  Loads are left for a pair's first
  //     block and the one or two blocks in which a window straddles an end of its sequence.
  // Each sequence decides for itself: a short one at its end does not send the long one down the slow path.
  PW_FN static uint64_t dwords(uint32_t lo, uint32_t hi) { return ((uint64_t)hi << 32) | lo; }
  PW_FN static void feed_count(int which) {
#if !defined(__HIPCC__)
    if (P::lane() == 0) pk::feed_path_counts()[which]++;       // (the CPU emulator: which path ran)
#endif
  }
  // The two readers.  On the device: scalar loads (P::const_dword; P::const_dword2, the two-dword load).  On the CPU emulator:
  // plain reads through the platform's const_dword that COUNT every dword asked for outside [0, wlast] of the frame
  // (pk::feed_breaches) and deliver a poison value for it instead of touching memory.
  PW_FN static uint32_t feed_dword(const uint8_t* base, int idx, int wlast) {
#if !defined(__HIPCC__)
    if (idx < 0 || idx > wlast) { pk::feed_breaches()++; return 0xa5a5a5a5u; }
#endif
    return P::const_dword(base, idx);
  }
  PW_FN static uint64_t feed_dword2(const uint8_t* base, uint32_t byte_off, int wlast) {
#if !defined(__HIPCC__)
    const int idx = (int)(byte_off + 4u) >> 2;
    if ((byte_off & 3u) != 0) pk::feed_breaches()++;
    return dwords(feed_dword(base, idx, wlast), feed_dword(base, idx + 1, wlast));
#else
    return P::const_dword2(base, byte_off);
#endif
  }
  PW_FN void feed_load3(const uint8_t* seq, int wlast, uint32_t fw, uint32_t& n0, uint64_t& n12) {
    const int w = (int)fw >> 2;
    n0 = feed_dword(seq, pw_clampi(w, 0, wlast), wlast);
    n12 = dwords(feed_dword(seq, pw_clampi(w + 1, 0, wlast), wlast), feed_dword(seq, pw_clampi(w + 2, 0, wlast), wlast));
  }
  PW_FN void feed_late(const uint8_t* seq, int wlast, uint32_t fw, uint32_t& n0, uint64_t& n12, int which) {
    const int w = (int)fw >> 2;
    feed_count(2 * which + 1);
    if (w >= wlast || w + 2 <= 0) { n0 = (uint32_t)(n12 >> 32); n12 = dwords(n0, n0); }
    else feed_load3(seq, wlast, fw, n0, n12);
  }
  PW_FN void feed_ahead(const uint8_t* seq, int wlast, uint32_t& fw, uint32_t flim, uint32_t& n0, uint64_t& n12, int which) {
    fw += 8u;
    if (fw < flim) {
      feed_count(2 * which);
      // (the copy of the word carried over comes BEFORE the load, which then lands in the registers it was copied from: the
      //  load's offset passes through the statement that makes the copy (pk::copy_su).  Scheduled first, the load took registers of
      //  its own and was waited for on the spot, to be copied into place.)
      n0 = pk::copy_su((uint32_t)(n12 >> 32), fw);
      n12 = feed_dword2(seq, fw, wlast);
    }
  }
  // FIRST: a pair's first block, in front of the block loops -- nothing is carried yet
  template <bool FIRST = false>
  PW_FN void feed_issue(int b) {
    if (!SEG) {
      if (FIRST) {
        feed_load3(oseq, owlast, fo_w, fo_n0, fo_n12); feed_load3(mseq, mwlast, fm_w, fm_n0, fm_n12);
      } else {
        feed_ahead(oseq, owlast, fo_w, fo_lim, fo_n0, fo_n12, 0); feed_ahead(mseq, mwlast, fm_w, fm_lim, fm_n0, fm_n12, 1);
      }
      return;
    }
    const uint32_t* o32 = (const uint32_t*)oseq;
    const uint32_t* m32 = (const uint32_t*)mseq;
    const int wo = (xfeed_o + 8 * b) >> 2, wm = (yfeed_m + 8 * b) >> 2;
    fo_n0 = o32[pw_clampi(wo, 0, owlast)]; fo_n12 = dwords(o32[pw_clampi(wo + 1, 0, owlast)], o32[pw_clampi(wo + 2, 0, owlast)]);
    fm_n0 = m32[pw_clampi(wm, 0, mwlast)]; fm_n12 = dwords(m32[pw_clampi(wm + 1, 0, mwlast)], m32[pw_clampi(wm + 2, 0, mwlast)]);
  }
  // bytes k = 0 .. 7 of the result are 0xff where i0 + k lies in [0, n), 0 elsewhere
  // (one pair per wavefront: the arguments are wave-uniform, and a clamp written as one expression is selected as a vector
  //  v_med3_i32 plus a v_readfirstlane_b32; split in two by an opaque scalar it stays s_max_i32 / s_min_i32)
  PW_FN static int clamp08(int v) {
    if (SEG) return pw_clampi(v, 0, 8);
    const int r = (int)pk::opaque_su((uint32_t)(v > 0 ? v : 0));
    return r < 8 ? r : 8;
  }
  PW_FN static uint64_t inside_bytes(int i0, int n) {
    const int lo = clamp08(-i0), hi = clamp08(n - i0);
    const uint64_t below_hi = hi >= 8 ? ~(uint64_t)0 : (((uint64_t)1 << (8 * hi)) - 1);
    const uint64_t below_lo = lo >= 8 ? ~(uint64_t)0 : (((uint64_t)1 << (8 * lo)) - 1);
    return below_hi & ~below_lo;
  }
  // MAT, blocks in which diagonals start or end (`edge`): the block's feed letters outside the sequences are replaced here,
  // once per block, by letters that encode "outside" (origin 0xff: row 0; mutant MOUT: selector 8 or 12) instead of a range
  // check per iteration.  Steady blocks keep the letters as loaded (only out-of-band slots read those beyond a sequence).
  // (The steady loop of RAMPF passes a run-time `edge`, see blocks_step: a branch around the replacement, in front of the
  // unrolled body -- wave-uniform with one pair per wavefront.  RT marks that call: the two paths join, and the high halves
  // are made opaque behind the join.)
  template <bool RT = false>
  PW_FN void feed_commit(int b, bool edge) {
    const int ro = (xfeed_o + 8 * b) & 3, rm = (yfeed_m + 8 * b) & 3;
    if (!SEG) {      // (a window the block before could not load ahead: feed_issue; the first block's is loaded, and stays)
      // (ONE branch in front of both: a test of its own per sequence opened the loop with a block of two instructions, which
      //  the block placement copied into the loop's closing block)
      const bool late_o = fo_w >= fo_lim, late_m = fm_w >= fm_lim;
      if (late_o | late_m) {
        if (late_o) feed_late(oseq, owlast, fo_w, fo_n0, fo_n12, 0);
        if (late_m) feed_late(mseq, mwlast, fm_w, fm_n0, fm_n12, 1);
      }
    }
    fo_lo = Base::funnel((uint32_t)fo_n12, fo_n0, ro); fo_hi = (uint32_t)(fo_n12 >> (8 * ro));
    fm_lo = Base::funnel((uint32_t)fm_n12, fm_n0, rm); fm_hi = (uint32_t)(fm_n12 >> (8 * rm));
    if (FROWS) {
#pragma unroll
      for (int k = 0; k < 8; k++) frow[k] = row_bits(fo_lo, fo_hi, k);
    }
    if (MAT && edge) {
      const uint64_t io = inside_bytes(xfeed_o + 8 * b, X), im = inside_bytes(yfeed_m + 8 * b, Y);
      const uint64_t m = (((((uint64_t)fm_hi) << 32) | fm_lo) & im) | ((0x0101010101010101ull * MOUT) & ~im);
      fm_lo = (uint32_t)m; fm_hi = (uint32_t)(m >> 32);
      if (FROWS) {
        // the rows are there already: a letter outside the sequence gets the all-zero row here, once per block, and the
        // selection per letter (row_bits) knows the four real rows only
        // (the halves apart and opaque: on the 64-bit value a test of the top byte became a 64-bit unsigned compare, which
        //  exists as a vector instruction only)
        const uint32_t io_lo = pk::opaque_su((uint32_t)io), io_hi = pk::opaque_su((uint32_t)(io >> 32));
#pragma unroll
        for (int k = 0; k < 8; k++) frow[k] = (((k < 4 ? io_lo : io_hi) >> (8 * (k & 3))) & 1u) ? frow[k] : 0u;
      } else {
        const uint64_t o = ((((uint64_t)fo_hi) << 32) | fo_lo) | ~io;
        fo_lo = (uint32_t)o; fo_hi = (uint32_t)(o >> 32);
      }
      // (seen as the halves of one 64-bit value, "the last letter is 0" became a 64-bit unsigned compare, which exists as a
      //  vector instruction only)
      if (!SEG && !RT) { if (!FROWS) fo_hi = pk::opaque_su(fo_hi); fm_hi = pk::opaque_su(fm_hi); }
    }
    if (MAT && !SEG && RT) { if (!FROWS) fo_hi = pk::opaque_su(fo_hi); fm_hi = pk::opaque_su(fm_hi); }
  }

  PW_FN int tfirst_of(int j) const {      // first step of slot j's diagonal; never for a diagonal outside the band
    const int dd = li * BK + j, d = pd.dmin + dd;
    if (MAT && ANYB && valid && dd == ndiag) return 0;   // the first diagonal above the band: see cellpair, the diagonal add
    return (valid && dd < ndiag) ? (d < 0 ? -d : d) - pd.s0 : 32767;
  }
  PW_FN int tlast_of(int j) const {
    const int dd = li * BK + j, d = pd.dmin + dd;
    if (!valid || dd >= ndiag) return -1;
    const int len = 1 + (d > 0 ? 0 : d) + (X - d > Y ? Y : X - d);
    return (d < 0 ? -d : d) - pd.s0 + 2 * (len - 1);
  }
  PW_FN int tbegin_of(int j) const {      // RULE != 0: the step of the diagonal's cell that may begin an alignment
    const int dd = li * BK + j, d = pd.dmin + dd;
    if (!valid || dd >= ndiag) return 32767;
    if ((RL == 2 || RL == 5 || a.brule == BRULE_ORIGIN) && d != 0) return 32767;   // begin at cell (0, 0) only (B_GLOBAL, GLOBAL, START_ANCHORED, START_ANCHORED_OVERLAP)
    return (d < 0 ? -d : d) - pd.s0;                       // the first cell of the diagonal lies on the table edge
  }
  // MAT: the row of origin letter l (uniform rows, selected by compares: scalar code where l is wave-uniform)
  // (the rows are copied out of the kernel arguments once -- MR0 .. MR3 -- so that the selection is a chain of selects on
  //  values already in registers; read in place, each arm became a load behind a branch, and a branch in the unrolled block
  //  serialises the packed ops)
  PW_FN uint32_t row_of(uint32_t l) const {
    uint32_t r = l == 3u ? MR3 : 0u;
    r = l == 2u ? MR2 : r;
    r = l == 1u ? MR1 : r;
    return l == 0u ? MR0 : r;
  }
  // ... of the k-th letter of a block's 8 origin letters, selected on the letter's two bits where they lie in the feed
  // words (k is a constant in the unrolled block): two bit tests and three selects -- against four compares and four
  // selects behind an extraction of the letter.  Knows letters 0 .. 3 only: feed_commit gives the letters outside the
  // sequence their all-zero row.
  PW_FN uint32_t row_bits(uint32_t lo, uint32_t hi, int k) const {
    const uint32_t w = k < 4 ? lo : hi;
    const bool b0 = (w & (1u << (8 * (k & 3)))) != 0, b1 = (w & (2u << (8 * (k & 3)))) != 0;
    const uint32_t r01 = b0 ? MR1 : MR0, r23 = b0 ? MR3 : MR2;
    return b1 ? r23 : r01;
  }
  PW_FN uint32_t row_at(int i) const { return (uint32_t)i < (uint32_t)X ? row_of((uint32_t)oseq[i]) : 0u; }
  // selector code of mutant letter i; plus4: the code reads v_perm_b32's first operand
  PW_FN uint32_t msel(int i, uint32_t plus4) const { return MSEL | (((uint32_t)i < (uint32_t)Y ? (uint32_t)mseq[i] : MOUT) + 4u * plus4); }
  PW_FN uint32_t letter_o(int i) const { return (uint32_t)i < (uint32_t)X ? (uint32_t)oseq[i] : SENT_O; }
  PW_FN uint32_t letter_m(int i) const { return (uint32_t)i < (uint32_t)Y ? (uint32_t)mseq[i] : SENT_M; }
  PW_FN int blocked(int j) const { return li * BK + j == ndiag ? NEG16 : 0; }   // first diagonal above the band
  // RAMPF with ramp_free: what slot j holds before step 0 -- 0 in the band and on the first diagonal above it (see RAMPF)
  PW_FN int start_of(int j) const { return (valid && li * BK + j <= ndiag) ? 0 : NEG16; }
  // the planner's ramp_free (the CPU emulator: as its test set it, and under the planner's knob)
  PW_FN bool ramp_free_on() const {
#if !defined(__HIPCC__)
    if (pk::ramp_free_emu() >= 0) {
      const char* knob = getenv("PWLIB_RAMP_BLOCKS");
      return pk::ramp_free_emu() != 0 && !(knob && atoi(knob) != 0);
    }
#endif
    return a.ramp_free != 0;
  }

  PW_FN void run() {
    const int lane = P::lane();
    const int nl = wd.nl;
    const int seg = lane / nl;
    li = lane - seg * nl;
    valid = seg < wd.count;
    segfirst = li == 0; seglast = li == nl - 1;
    const int slot = wd.first + ((SEG && valid) ? seg : 0);   // lanes beyond the last pair shadow the first one
    pair_slot = a.order ? a.order[slot] : slot;
    if (!SEG) pair_slot = P::uniform(pair_slot);             // one pair: keep its descriptor in scalar registers
    pd = a.pairs[pair_slot];
    X = pd.X; Y = pd.Y; ndiag = pd.ndiag;
    oseq = a.arena + pd.o_off; mseq = a.arena + pd.m_off;
    owlast = (X > 0 ? X - 1 : 0) >> 2; mwlast = (Y > 0 ? Y - 1 : 0) >> 2;
    const int e = (pd.s0 + pd.dmin) >> 1;       // x of diagonal dd = 0 on step t = 0 (s0 == dmin mod 2)
    const int f = (pd.s0 - pd.dmin) >> 1;       // y likewise
    const int xbase = e + li * R, ybase = f - li * R;
    xfeed_o = e + nl * R - 1;                   // the letter a virtual lane `nl` would hand down
    yfeed_m = f;
    fo_w = (uint32_t)xfeed_o & ~3u; fm_w = (uint32_t)yfeed_m & ~3u;
    fo_lim = 4u * (uint32_t)(owlast > 1 ? owlast - 1 : 0); fm_lim = 4u * (uint32_t)(mwlast > 1 ? mwlast - 1 : 0);
    rf = RAMPF && (GRP == 4 || ramp_free_on());      // (the grouped kernel is launched for ramp_free batches only)
#if !defined(__HIPCC__)
    grp4_rt = GRP == 4 || (GOK && rf && P::nwaves() == 1 && pk::stamp_group_emu() == 4);
#endif
#if !defined(__HIPCC__)
    pairk_rt = grp4_rt && pk::pair_keys_emu() == 1;
#endif
    if (grp4()) {
      if (pairk()) {
#pragma unroll
        for (int k = 0; k < 4; k++) POS[k] = pk::opaque_su(pk::both(15 - k));
      } else {
#pragma unroll
        for (int k = 0; k < 8; k++) POS[k] = pk::opaque_su(pk::both(31 - k));
      }
    }
    ONE =pk::opaque(0x00010001u); SH15 = pk::opaque(0x000f000fu);
    C2 = pk::opaque(0x00020002u); C4 = pk::opaque(0x00040004u); C16 = pk::opaque(0x00100010u);
    C8 = pk::opaque(0x00080008u); SEVEN = pk::opaque(0x00070007u);
    NEGV = pk::both(NEG16); LIMV = pk::both(-32767);
    NDELTA = pk::both(SCL * (a.mismatch - a.match)); MATCHV = pk::both(SCL * a.match);
    // the multipliers of the "not kept" values: 0 / 1 each, or (SC4) 0 / 2 for D and 0 / 4 for I; KEPT: of the kept values 2 and
    // 4, which take 4 go back out of an offer that starts with it (geb below)
    GOV = pk::both(KEPT ? -2 * a.go : (SC4 ? 2 * a.go : a.go)); GOVI = pk::both(KEPT ? -a.go : a.go);
    BIASV = pk::both(a.mat_bias); MADJ = 0x0003fffcu;
    MR0 = a.mat_rows[0]; MR1 = a.mat_rows[1]; MR2 = a.mat_rows[2]; MR3 = a.mat_rows[3];
    if (MAT) {
#pragma unroll
      for (int i = 0; i < (MAT ? R : 1); i++) ROW[i] = row_at(xbase + i - 1);
    }
#pragma unroll
    for (int p = 0; p < RH; p++) {
      const int e0 = 2 * p, e1 = 2 * p + R, o0 = 2 * p + 1, o1 = 2 * p + 1 + R;
      if (ANYB) {
        const int geo = SCL * a.ge + (KEPT ? SCL * a.go : 0);
        gebE[p] = pk::pack(geo + blocked(e0), geo + blocked(e1));
        gebO[p] = pk::pack(geo + blocked(o0), geo + blocked(o1));
        tfE[p] = pk::pack(tfirst_of(e0), tfirst_of(e1)); tfO[p] = pk::pack(tfirst_of(o0), tfirst_of(o1));
        clE[p] = clO[p] = 0;
      } else {
        gebE[p] = gebO[p] = pk::both(a.ge);
        clE[p] = pk::pack(blocked(e0) ? NEG16 : 32767, blocked(e1) ? NEG16 : 32767);
        clO[p] = pk::pack(blocked(o0) ? NEG16 : 32767, blocked(o1) ? NEG16 : 32767);
        tfE[p] = pk::pack(tbegin_of(e0), tbegin_of(e1)); tfO[p] = pk::pack(tbegin_of(o0), tbegin_of(o1));
      }
      tlE[p] = pk::pack(tlast_of(e0), tlast_of(e1)); tlO[p] = pk::pack(tlast_of(o0), tlast_of(o1));
      HE[p] = UE[p] = LE[p] = HO[p] = UO[p] = LO[p] = NEGV;
      if (RAMPF && rf) {        // (the offers stay at the sentinel: nothing was offered before step 0)
        HE[p] = pk::pack(start_of(e0), start_of(e1)); HO[p] = pk::pack(start_of(o0), start_of(o1));
      }
      up_prev = left_next = NEGV; phase_l = 0; phase_r = 0;
      // tracking rules: best 0 and no stamp yet (finish(): such a diagonal reports its first cell under rule 0)
      bestE[p] = bestO[p] = NEGV;
      kbE[p] = kbO[p] = 0u; btE[p] = btO[p] = 0u; kgE[p] = kgO[p] = 0u;
      OW[p] = pk::pack((int32_t)letter_o(xbase + p - 1), (int32_t)letter_o(xbase + p + RH - 1));
      if (MAT) {
        // (FIXSEL: letter y was, or would have been, fed on iteration y - f)
        const int yl = ybase - p - 1, yh = ybase - p - RH - 1;
        MW[p] = pk::pack((int32_t)msel(yl, FIXSEL ? sel4_fed(yl - f) : 0u), (int32_t)msel(yh, FIXSEL ? sel4_fed(yh - f) : 1u));
      }
      else MW[p] = pk::pack((int32_t)letter_m(ybase - p - 1), (int32_t)letter_m(ybase - p - RH - 1));
    }
    // The planner's steady range allows a diagonal's LAST cell to be the last step of a steady block (every cell of
    // the block is still valid); rules 1 / 2 capture that cell, which only the edge body does: give up that block.
    const int sb1 = CAP ? wd.steady_b1 - 1 : wd.steady_b1;
    mgroup = 4u * (uint32_t)pd.nl;
    mspare = (uint32_t)mask_word_index(BK, pd.nl, pd.nblocks, 0, 0);
    const bool mrow_ok = valid && li < pd.nl;
    mrow0 = mrow_ok ? (uint32_t)mask_word_index(BK, pd.nl, 0, li, 0) : mspare;
    mrow_step = mrow_ok ? (uint32_t)mask_word_index(BK, pd.nl, 1, 0, 0) : 0u;
    mrowb = 4u * mrow0;
    if (SBASE) {
#pragma unroll
      for (int g = 0; g < BK / 4; g++)   // (opaque: left to itself the compiler adds the group's distance per lane, in 64 bits)
        mbase[g] = pk::opaque_s((uint8_t*)(a.masks + pd.mask_off) + (uint64_t)(4u * (uint32_t)g * mgroup));
    }
#if !defined(__HIPCC__)
    ldsf_rt = LOK && rf && P::nwaves() == 1 && pk::lds_feed_emu() == 1;
#endif
    PW_IF_LDSF { fe = e; ff = f; ring_begin(); }
    else feed_issue<true>(0);
    if constexpr (XLDS != 0) offers_begin();
    if constexpr (SPLIT) {
      // One loop per kind of block, in the order a pair runs through them: with a single body the loop-carried state stays in
      // the registers it was computed in.  (One loop that chose among the four bodies joined them in a shared tail, and the
      // allocator then copied about 14 registers of state on every back edge.)
      const int nb = nblocks_run();
      const int b0 = wd.steady_b0 < nb ? (wd.steady_b0 > 0 ? wd.steady_b0 : 0) : nb;
      const int b1 = sb1 < nb ? sb1 : nb;
      // RAMPF with ramp_free: the steady loop takes every block, the other three run none
      const int r0 = (RAMPF && rf) ? 0 : b0, r1 = (RAMPF && rf) ? nb : b1;
      flimx = (uint32_t)(X > 7 ? X - 7 : 0); flimy = (uint32_t)(Y > 7 ? Y - 7 : 0);
      int b = 0;
      if (GRP != 4) {                                                  // (the grouped kernel: the steady loop alone)
        if (sb1 > wd.steady_b0) for (; b < r0; b++) blocks_step<1>(b);   // some have not started; none has ended before the steady range
        else for (; b < r0; b++) blocks_step<3>(b);                      // (no steady range: the planner's bounds cannot tell)
      }
      for (; b < r1; b++) blocks_step<0>(b);
      if (GRP != 4) for (; b < nb; b++) blocks_step<2>(b);             // every diagonal has started, some may have ended
      // grouped: a last group of fewer than four blocks has not been stamped yet
      if (grp4() && (nb & 3) != 0 && nb > 0) stamp_group((uint32_t)(nb >> 2) + 1u);
    } else {
      for (int b = 0, nb = nblocks_run(); b < nb; b++) {
        const bool steady = b >= wd.steady_b0 && b < sb1;
        feed_commit(b, !steady);
        if (b + 1 < nb) feed_issue(b + 1);
        if (steady) block16<0>(b);
        else if (!ANYB) block16<3>(b);
        else if (b >= wd.steady_b0) block16<2>(b);                   // every diagonal has started, some may have ended
        else if (sb1 > wd.steady_b0) block16<1>(b);                  // some have not started; none has ended before the steady range
        else block16<3>(b);                                          // (no steady range: the planner's bounds cannot tell)
      }
    }
    finish();
  }
  // One pair per wavefront (or workgroup): the wavefront's block count IS the pair's (plan_waves); the minimum keeps the mask
  // stores, which no longer test the block against the pair's count, inside the plane whatever a descriptor says.
  PW_FN int nblocks_run() const { return SBASE ? (wd.nblocks < pd.nblocks ? wd.nblocks : pd.nblocks) : wd.nblocks; }
  template <int EK>
  PW_FN void blocks_step(int b) {
    // (the steady loop, RAMPF with ramp_free: the letters are replaced in every block that is fed one from outside a
    //  sequence -- the first of its eight origin or mutant letters has a negative index or lies past length - 8)
    PW_IF_LDSF {
      // (letters from LDS: no feeders -- the rings are restaged at the end of every eighth block, block16)
    } else {
      if constexpr (RAMPF && EK == 0)
        feed_commit<true>(b, rf & (((uint32_t)(xfeed_o + 8 * b) >= flimx) | ((uint32_t)(yfeed_m + 8 * b) >= flimy)));
      else feed_commit(b, EK != 0);
      if (b + 1 < nblocks_run()) feed_issue(b + 1);
    }
    block16<EK>(b);
  }

  // PAIRK: whether slot j's key, taken for the cells of iterations itp - 1 and itp of diagonal d, belongs to the second of the
  // two, c' = cell aap of the diagonal: c' lies in the table off its edges, kept the diagonal move alone -- its tie nibble,
  // read back from the dword of the mask plane this very lane stored -- and its letters score above 0 (see pairk()).  Reads
  // nothing outside the pair's plane and frames, whatever the stamp says.
  PW_FN bool second_of_pair(int j, int d, int itp, int aap) const {
    const int xp = aap + (d > 0 ? d : 0), yp = aap - (d < 0 ? d : 0);
    const int bp = itp >> 3;
    if (!(valid && li * BK + j < ndiag && li < pd.nl && bp >= 0 && bp < pd.nblocks && xp >= 1 && yp >= 1 && xp <= X && yp <= Y)) return false;
    const uint32_t w = (a.masks + pd.mask_off)[mask_word_index(BK, pd.nl, bp, li, j)];
    const uint32_t nib = (w >> (4 * (7 - (itp & 7)))) & 7u;
    const uint32_t row = row_of((uint32_t)oseq[xp - 1]);
    const int32_t sc = (int32_t)((row >> (8u * ((uint32_t)mseq[yp - 1] & 3u))) & 0xffu) - a.mat_bias;
    return nib == 0u && sc > 0;
  }

  // End-cell search for the two rules this kernel serves (END_STD_LOCAL, END_BANDED_LOCAL): the first best
  // cell of every in-band diagonal, reduced on (score desc, scan rank asc) -- once per pair of the wave.
  PW_FN void finish() {
    const int endrule = a.endrule;
    int32_t cs = -32768; uint64_t ck = ~(uint64_t)0; int cx = -1, cy = -1; bool have = false;
#if !defined(__HIPCC__)
    int csec = -1;
#endif
    // Runs once per pair: keep it out of the register budget of the fill loop.  The packed bests are parked
    // in a small private array and scanned by a rolled loop.
    uint32_t parked[4 * RH];
#pragma unroll
    for (int p = 0; p < RH; p++) {
      // (copies made here, after the block loops: parked straight from the loop-carried registers, the array's register
      //  tuple was kept up to date by moves in every block)
      parked[4 * p] = TRK ? pk::opaque(kbE[p]) : bestE[p]; parked[4 * p + 1] = TRK ? pk::opaque(btE[p]) : 0u;
      parked[4 * p + 2] = TRK ? pk::opaque(kbO[p]) : bestO[p]; parked[4 * p + 3] = TRK ? pk::opaque(btO[p]) : 0u;
    }
#pragma unroll 1
    for (int q = 0; q < 2 * RH; q++) {
      const int p = q >> 1, odd = q & 1;
      const uint32_t bq = parked[4 * p + 2 * odd], tq = parked[4 * p + 2 * odd + 1];
#pragma unroll 1
      for (int h = 0; h < 2; h++) {
        const int j = 2 * p + odd + h * R;
        const int dd = li * BK + j, d = pd.dmin + dd;
        const int tfirst = (d < 0 ? -d : d) - pd.s0;
        int32_t s; int bt;
#if !defined(__HIPCC__)
        int s_second = -1;           // (the CPU emulator: how this slot's key was resolved, pk::pair_key_counts)
#endif
        if (TRK) {
          // key = 8 score + (7 - cell) with the score unscaled (SC4: 2 (4 score) + ..); stamp = 8 (block + 1) + 7 - cell of the
          // cell that first reached it, below 8 while the best stayed 0.  Rule 0: scores never go below 0, and a diagonal whose
          // best stays 0 reports its first cell (score 0 on the table edge).  (Rule 5: a best of 0 never wins -- the end cell
          // must beat 0 -- so where it "was reached" does not matter.)
          const uint32_t key = h ? (bq >> 16) : (bq & 0xffffu), stamp = h ? (tq >> 16) : (tq & 0xffffu);
          // Grouped: key = 32 score + (31 - cell within the group), stamp = 32 (group + 1) + 31 - cell, below 32 while the best
          // stayed 0; a group is 64 steps.
          if (!grp4()) {
            s = (int32_t)(key >> 3);
            if (stamp < 8u) bt = ANYB ? (int)((uint32_t)tfirst & 0xffffu) : 0;
            else bt = 16 * ((int)(stamp >> 3) - 1) + 2 * (7 - (int)(stamp & 7u)) + odd;
          } else {
            s = (int32_t)(key >> 5);
            if (stamp < 32u) bt = ANYB ? (int)((uint32_t)tfirst & 0xffffu) : 0;
            else if (!pairk()) bt = 64 * ((int)(stamp >> 5) - 1) + 2 * (31 - (int)(stamp & 31u)) + odd;
            else {
              // one key per two cells: the code is 15 - pair within the group; c' is the pair's second cell
              const int itp = 32 * ((int)(stamp >> 5) - 1) + 2 * (15 - (int)(stamp & 31u)) + 1;
              bt = 2 * itp + odd;
              const bool second = second_of_pair(j, d, itp, (bt - tfirst) >> 1);
              if (!second) bt -= 2;
#if !defined(__HIPCC__)
              if (valid && dd < ndiag) pk::pair_key_counts()[second ? 1 : 0]++;
              s_second = second;
#endif
            }
          }
        } else {
          s = (h ? pk::hi_s(bq) : pk::lo_s(bq)) / SCL;                 // (exact: every running value is a multiple of SCL)
          bt = 0;
        }
        const int aa = (bt - tfirst) >> 1;
        int x = aa + (d > 0 ? d : 0), y = aa - (d < 0 ? d : 0);
        uint64_t k;
        bool ok = true;
        if (CAP) {
          // `s` is the captured value of the diagonal's last cell (_banded_find_optimal, _pw_internals.c:364-414)
          const bool ends_right = d < X - Y;
          x = ends_right ? d + Y : X; y = ends_right ? Y : X - d;
          // ties: banded overlap takes the diagonals in ascending order, standard overlap the last column top-down and then
          // the last row left to right (_std_find_optimal: on the full band every diagonal ends on one of the two)
          k = endrule == END_STD_OVERLAP ? (uint64_t)(uint32_t)(x < X ? x : X + y) : (uint64_t)(uint32_t)dd;
          if (RL == 2 || RL == 4 || endrule == END_CORNER) ok = d == X - Y;      // end at cell (X, Y) only
        } else if (endrule == END_STD_LOCAL) k = (uint64_t)(uint32_t)x * (uint64_t)(uint32_t)(Y + 1) + (uint64_t)(uint32_t)y;
        else k = ((uint64_t)(uint32_t)dd << 32) | (uint64_t)(uint32_t)aa;
        const bool better = ok && valid && dd < ndiag && (!have || s > cs || (s == cs && k < ck));
        if (better) { cs = s; ck = k; cx = x; cy = y; have = true; }
#if !defined(__HIPCC__)
        if (better) csec = s_second;
#endif
      }
    }
    const int lane = P::lane();
    const int seg = lane / wd.nl;
    for (int sidx = 0; sidx < wd.count; sidx++) {
      int hv = (have && seg == sidx) ? 1 : 0;
      int32_t rs = cs; uint64_t rk = ck; int rx = cx, ry = cy;
#if !defined(__HIPCC__)
      int rsec = csec;
#endif
#pragma unroll
      for (int off = 32; off >= 1; off >>= 1) {
        const int32_t os = P::shfl_xor(rs, off);
        const uint64_t ok_ = xshfl_xor<P>(rk, off);
        const int ox = P::shfl_xor(rx, off), oy = P::shfl_xor(ry, off), oh = P::shfl_xor(hv, off);
        const bool take = oh && (!hv || os > rs || (os == rs && ok_ < rk));
#if !defined(__HIPCC__)
        const int osec = P::shfl_xor(rsec, off);
        if (take) rsec = osec;
#endif
        if (take) { rs = os; rk = ok_; rx = ox; ry = oy; hv = 1; }
      }
#if !defined(__HIPCC__)
      if (P::nwaves() == 1 && seg == sidx && li == 0 && hv && rsec >= 0) pk::pair_key_counts()[2 + rsec]++;
#endif
      // several wavefronts per pair (K2a with this body; one pair, SEG = false): the per-wave winners the same way
      if (P::nwaves() > 1) {
        int32_t bs = rs; uint64_t bk_ = rk; int bx = rx, by = ry, bh = 0;
        for (int wv = 0; wv < P::nwaves(); wv++) {
          const int32_t os = P::wave_bcast(rs, wv);
          const uint64_t ok_ = xwave_bcast<P>(rk, wv);
          const int ox = P::wave_bcast(rx, wv), oy = P::wave_bcast(ry, wv), oh = P::wave_bcast(hv, wv);
          const bool take = oh && (!bh || os > bs || (os == bs && ok_ < bk_));
          if (take) { bs = os; bk_ = ok_; bx = ox; by = oy; bh = 1; }
        }
        rs = bs; rk = bk_; rx = bx; ry = by; hv = bh;
      }
      if (seg == sidx && li == 0) {
        Result r;
        r.score = (double)rs * a.score_mul;
        r.opt_i = a.banded ? rx - ry - pd.dmin : rx;
        r.opt_j = a.banded ? (rx < ry ? rx : ry) : ry;
        r.origin_idx = 0; r.mutant_idx = 0; r.tx_len = 0; r.status = 0;
        // LOCAL starts from the score of cell (0,0), i.e. 0 (_pw_internals.c:342)
        if (!hv || (endrule == END_STD_LOCAL && !(rs > 0))) { r.opt_i = -1; r.opt_j = -1; r.score = 0.0; }
        a.results[pair_slot] = r;
      }
    }
  }
  // LDSF (declared last: the members above keep the places they had)
  uint32_t ring_h = 0;          // the device's LDS address of the origin ring; the mutant ring lies kRingWords words behind it
  uint32_t ro, rm;              // byte offset of this lane's word within a row, as of the current block: origin, mutant ring
  uint32_t nx_o, nx_m;          // this lane's two letters of the chunk the next restage writes
  int fe, ff;                   // e, f of run()
  uint32_t xch_a = 0;           // XLDS: the device's LDS address of this lane's dword of the up offers' array (offers_begin)
#if !defined(__HIPCC__)
  bool pairk_rt = false;        // (the CPU emulator: PAIRK at run time, pk::pair_keys_emu)
#endif
};
#undef PW_IF_LDSF

// =================================================================================================
// K4: traceback of one pair by one lane, over the tie-mask plane.
// Predecessor rule after a gap op g (pinned by oracle `maskrule_ok`): go < 0 -> g if g is
// kept in the predecessor else its first kept op; go == 0 -> first kept; go > 0 -> first kept op
// other than g, else g.  After M/S: first kept (_pw_internals.c:235).
// =================================================================================================
PW_FN int pw_first_op(uint32_t mask) {   // index of the lowest set bit: 0 B, 1 D, 2 I, 3 M
  return (mask & 1u) ? 0 : (mask & 2u) ? 1 : (mask & 4u) ? 2 : 3;
}


// ---- K4a: the walk --------------------------------------------------------------------------------
// One lane walks one pair; a wavefront holds 64 walkers.  The walk is a chain of dependent steps, and
// 64 divergent walkers share one program counter, so ANY lane touching memory stalls all 64.  The loop
// is therefore split: an outer iteration in which every unfinished lane refills a private register
// cache with ONE batched access -- the 16-byte mask groups (4 adjacent diagonals) of its current block
// and of the block before it -- and an inner loop that only steps while the next cell is inside that
// cache: no loads at all, just byte stores of the ops.  A lane that leaves its cached window idles
// until the others do; all refill together.  Sequence letters are not read here: diagonal moves are
// written as 'X' and turned into 'M'/'S' by the fix-up pass (K4b), which is fully parallel.
// Window of the mask plane a walker keeps on chip: WIN_B consecutive blocks x 2 adjacent diagonal groups
// (4 diagonals each), one dword per (block, group, diagonal): 64 steps along the path x 8 diagonals.
enum { WIN_B = 4, WIN_WORDS = WIN_B * 2 * 4 };

PW_FN void trace_walk(const TraceParams& p, int pair, uint32_t* win /* WIN_WORDS dwords private to this walker (LDS) */) {
  // everything the loops need is copied into locals first: the byte stores of the ops go through a
  // uint8_t*, which the compiler must assume aliases the descriptors
  const PairDesc pdv = p.pairs[pair];
  if (!pdv.solvable || pdv.layout != 0) return;      // (strip-layout pairs have their own walker: pw_strip.h)
  Result r = p.results[pair];
  const int ei = p.ends ? p.ends[2 * pair] : r.opt_i;
  const int ej = p.ends ? p.ends[2 * pair + 1] : r.opt_j;
  if (ei < 0 || ej < 0) { r.tx_len = 0; r.status = 0; p.results[pair] = r; return; }
  const int dmin = pdv.dmin, s0 = pdv.s0, ndiag = pdv.ndiag, bk = pdv.bk, nl = pdv.nl, gosign = p.gosign;
  int x = ei, y = ej;
  if (p.banded) {                 // _xy_from_cellpos (_pw_internals.c:100-114)
    const int d = ei + dmin;
    x = ej + (d > 0 ? d : 0); y = ej - (d > 0 ? 0 : d);
  }
  const uint32_t* __restrict__ plane = p.masks + pdv.mask_off;
  uint8_t* __restrict__ tx = p.transcripts + pdv.tx_off;
  const int lgG = bk < 4 ? 1 : 2;               // log2 of the dwords per lane group (pw_types.h: mask_word_index)
  const int G = 1 << lgG;
  const int njg = bk >> lgG;                    // groups per lane
  const int ngroups = (ndiag + G - 1) >> lgG;   // groups that hold in-band diagonals
  int pos = pdv.tx_cap;           // ops are written backwards, ending right-aligned in the slot
  int nms = 0, bad = 0;
  int prev = 3;                   // op that led to the current cell; "M" makes the end cell use its first choice (pw.c:123)
  bool done = false;
  while (!done) {
    // ---- refill: blocks cb .. cb - 3 of the current cell's diagonal group and of the neighbouring group on
    //      the side the cell sits on (paths drift by single diagonals); all loads issued back to back ----
    const int dd0 = x - y - dmin, t0 = x + y - s0;
    // (never expected -- see below; x > X or y > Y would index the mask plane behind its last block)
    if (x < 0 || y < 0 || x > pdv.X || y > pdv.Y || dd0 < 0 || dd0 >= ndiag) { bad = 1; break; }
    const int cb = t0 >> 4;
    const int ga = dd0 >> lgG;
    int gb = ((dd0 & (G - 1)) >= (G >> 1)) ? ga + 1 : ga - 1;
    gb = gb < 0 ? ga + 1 : (gb >= ngroups ? ga - 1 : gb);
    if (gb < 0) gb = ga;          // a band of a single group
#pragma unroll
    for (int s2 = 0; s2 < 2; s2++) {
      const int gg = s2 ? gb : ga;
      const int ln = gg / njg, jg = gg - ln * njg;
#pragma unroll
      for (int k = 0; k < WIN_B; k++) {
        const int bb = cb - k > 0 ? cb - k : 0;
        // (for bk = 2 a group is 8 bytes: the upper half of the 16-byte load is the neighbouring lane's group,
        //  in bounds thanks to the slack behind the mask workspace, and never selected below)
        const U4 v = *(const U4*)(plane + ((uint64_t)((uint64_t)bb * njg + jg) * nl + ln) * G);
        uint32_t* wslot = win + (k * 2 + s2) * 4;
        wslot[0] = v.x; wslot[1] = v.y; wslot[2] = v.z; wslot[3] = v.w;
      }
    }
    // ---- step while the cell is inside the window: no global loads, only byte stores of the ops ----
    while (true) {
      const int dd = x - y - dmin, t = x + y - s0;
      // a well-formed mask plane never leads outside the table; if it ever did (a kernel bug), stop
      if (x < 0 || y < 0 || x > pdv.X || y > pdv.Y || dd < 0 || dd >= ndiag) { bad = 1; done = true; break; }
      const int gg = dd >> lgG, b = t >> 4, kb = cb - b;
      if ((gg != ga && gg != gb) || kb < 0 || kb >= WIN_B) break;              // miss: refill
      const uint32_t w = win[(kb * 2 + (gg == ga ? 0 : 1)) * 4 + (dd & (G - 1))];
      const uint32_t pm = (w >> (4 * (7 - ((t & 15) >> 1)))) & 15u;
      // which kept choice of this cell is the base of the step that led here
      int op;
      if (prev == 3 || gosign == 0) op = pw_first_op(pm);
      else if (gosign < 0) op = (pm & (1u << prev)) ? prev : pw_first_op(pm);
      else { const uint32_t others = pm & ~(1u << prev); op = others ? pw_first_op(others) : prev; }
      if (op == 0 || pos <= 0) { done = true; break; }
      tx[--pos] = op == 3 ? 'X' : (op == 1 ? 'D' : 'I');
      nms += (op == 3);
      x -= (op != 2); y -= (op != 1);
      prev = op;
      if (op == 3) {
        // bulk step: a run of diagonal moves stays on this diagonal and, while the cell index n inside the
        // block stays >= 0, inside this very dword.  After M the next op is the cell's first kept choice,
        // which is M again exactly when none of B, D, I is kept: (nibble & 7) == 0.  Count those cells
        // with one ctz and write eight 'X' at once: ops are written backwards, so the bytes below the
        // run are overwritten by the ops that follow (the slot's first 8 bytes are left to the slow path).
        const int n = ((t & 15) >> 1) - 1;           // cell index of the new (x, y) within the dword
        if (n >= 0 && pos >= 16) {
          const uint64_t v = (uint64_t)((w & 0x77777777u) >> (4 * (7 - n))) | ((uint64_t)1 << (4 * (n + 1)));
          int k = (int)(__builtin_ctzll(v) >> 2);     // pure-M cells ahead, at most n + 1
          const int lim = x < y ? x : y;               // a diagonal move needs x >= 1 and y >= 1
          k = k < lim ? k : lim;
          if (k > 0) {
            PackedU64 xs; xs.v = 0x5858585858585858ull;
            *(PackedU64*)(tx + pos - 8) = xs;
            pos -= k; nms += k; x -= k; y -= k;
          }
        }
      }
    }
  }
  r.origin_idx = x; r.mutant_idx = y;
  r.tx_len = pdv.tx_cap - pos;
  r.status = ST_TRACED | (r.tx_len == 0 ? ST_EMPTY : 0) | ((x + y + nms <= 0) ? ST_PANICK : 0) | (bad ? ST_BADPATH : 0);
  p.results[pair] = r;
}

// ---- K4b: turn the diagonal moves 'X' into 'M' / 'S' (_pw_internals.c:232) ------------------------
// Serial form (one pair, one thread): what the wave-parallel device version in pw_trace.hip computes
// with ballots + popcounts; the CPU lane emulator uses this one.
PW_FN void trace_fixup_serial(const TraceParams& p, int pair) {
  const PairDesc& pd = p.pairs[pair];
  if (!pd.solvable) return;
  const Result r = p.results[pair];
  if (!(r.status & ST_TRACED) || r.tx_len <= 0) return;
  const uint8_t* oseq = p.arena + pd.o_off;
  const uint8_t* mseq = p.arena + pd.m_off;
  uint8_t* tx = p.transcripts + pd.tx_off + pd.tx_cap - r.tx_len;
  int x = r.origin_idx, y = r.mutant_idx;
  for (int k = 0; k < r.tx_len; k++) {
    const uint8_t ch = tx[k];
    if (ch == 'X') { tx[k] = (oseq[x] == mseq[y]) ? 'M' : 'S'; x++; y++; }
    else if (ch == 'D') x++;
    else y++;
  }
}

}  // namespace pw
#endif

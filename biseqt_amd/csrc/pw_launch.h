// pw_launch.h -- host-visible launchers of the gfx950 kernels in pw_kernels.hip.
#ifndef PW_LAUNCH_H
#define PW_LAUNCH_H

#include <hip/hip_runtime_api.h>

#include "pw_plan.h"     // the variants, diagonals per lane and kernel geometry the planner chooses from
#include "pw_types.h"

namespace pw {

hipError_t launch_fill(const FillParams<int32_t>& a, int variant, int bk, int nblocks, hipStream_t st);
hipError_t launch_fill(const FillParams<double>& a, int variant, int bk, int nblocks, hipStream_t st);
// lane-packed 16-bit kernel (VAR_FAST16): one block per WaveDesc
// seg != 0: several pairs per wavefront (WaveDesc.nl lanes each); seg == 0: one pair per wavefront, WaveDesc.nl == 64
// rule: 0 .. 5 (pw_wave.h, WaveFill16); mat != 0: scores from FillParams::mat_rows (rules 0 .. 3 only)
hipError_t launch_fill16(const FillParams<int32_t>& a, int bk, int seg, int rule, int mat, int nwaves, hipStream_t st);
hipError_t launch_fill16_mw(const FillParams<int32_t>& a, int bk, int rule, int mat, int nw, int npairs, hipStream_t st);   // nw wavefronts per pair
// the grouped kernel k_fill16g<8, false, 3, true> (pw_plan.h, stamp_group == 4): rule 3, matrix form, 8 diagonals per lane, one
// pair per wavefront, FillParams::ramp_free set
hipError_t launch_fill16g(const FillParams<int32_t>& a, int nwaves, hipStream_t st);
// ... and the same form with its letters read from LDS, k_fill16l<8, false, 3, true> (pw_plan.h, lds_feed)
hipError_t launch_fill16l(const FillParams<int32_t>& a, int nwaves, hipStream_t st);
// ... and with one running-best key per two cells, k_fill16p<8, false, 3, true> (pw_plan.h, pair_keys)
hipError_t launch_fill16p(const FillParams<int32_t>& a, int nwaves, hipStream_t st);
// ... and with the offers that cross lanes handed on through LDS, k_fill16x<8, false, 3, true> (pw_plan.h, lds_exchange)
hipError_t launch_fill16x(const FillParams<int32_t>& a, int nwaves, hipStream_t st);
// wide bands: one workgroup of nw wavefronts (2048 diagonals each, nw <= kMaxWavesPerPair) per pair
hipError_t launch_fill_mw(const FillParams<int32_t>& a, int variant, int bk, int nw, int nblocks, hipStream_t st);
hipError_t launch_fill_mw(const FillParams<double>& a, int variant, int bk, int nw, int nblocks, hipStream_t st);
// tiled single-pair kernel (K2b), geometry in pw_plan.h
hipError_t launch_tile(const FillParams<int32_t>& a, int variant, int pair, int ntiles, hipStream_t st);
hipError_t launch_tile(const FillParams<double>& a, int variant, int pair, int ntiles, hipStream_t st);
hipError_t launch_tile_finish(const FillParams<int32_t>& a, int pair, hipStream_t st);
hipError_t launch_tile_finish(const FillParams<double>& a, int pair, hipStream_t st);
hipError_t launch_trace(const TraceParams& p, hipStream_t st);
// compaction of the transcripts: offsets[n + 1] = exclusive prefix sum of tx_len, packed = the ops back to back
hipError_t launch_tx_pack(const PairDesc* pairs, const Result* results, const uint8_t* slots, int n, uint64_t* offsets,
                          uint8_t* packed, hipStream_t st);
// alignment summaries (pw_txsum.hip; `out` is pw_tx_summary[n] of include/pw_txsum.h): one wavefront per transcript, over
// the slots of a batch or over a packed buffer and its offsets[n + 1]
hipError_t launch_tx_summary(const PairDesc* pairs, const Result* results, const uint8_t* slots, int n, void* out, hipStream_t st);
hipError_t launch_tx_summary_packed(const uint8_t* ops, const uint64_t* offsets, int n, void* out, hipStream_t st);
// CIGARs (pw_cigar.hip; forms and the run dword in include/pw_cigar.h): one wavefront per transcript, over the slots of a
// batch or over a packed buffer and its offsets[n + 1].  count: the runs per transcript and, behind them on the stream,
// their exclusive prefix sums in offsets[n + 1] ([n] = total); write: every run to runs[offsets[k] + index]
hipError_t launch_cigar_count(const PairDesc* pairs, const Result* results, const uint8_t* slots, int n, int form, uint64_t* offsets,
                              hipStream_t st);
hipError_t launch_cigar_write(const PairDesc* pairs, const Result* results, const uint8_t* slots, int n, int form, const uint64_t* offsets,
                              uint32_t* runs, hipStream_t st);
hipError_t launch_cigar_count_packed(const uint8_t* ops, const uint64_t* offsets, int n, int form, uint64_t* run_offsets, hipStream_t st);
hipError_t launch_cigar_write_packed(const uint8_t* ops, const uint64_t* offsets, int n, int form, const uint64_t* run_offsets, uint32_t* runs,
                                     hipStream_t st);
// pileups (pw_pileup.hip; the definition in include/pw_pileup.h): add -- one wavefront per pair scatters its ops into
// counts[n_cols][L + 2] (col0: device array of frame starts per pair, or null for o_off - arena_first); call -- one thread per
// column writes sites[n_cols] (pw_pileup_site; ref: device letters or null)
hipError_t launch_pileup_add(const PairDesc* pairs, const Result* results, const uint8_t* slots, const uint8_t* arena, int n,
                             const int64_t* col0, int64_t arena_first, uint32_t* counts, int64_t n_cols, int L, hipStream_t st);
hipError_t launch_pileup_call(const uint32_t* counts, const uint8_t* ref, int64_t n_cols, int L, uint32_t min_depth, void* sites,
                              hipStream_t st);
// read correction (pw_polish.hip; the definitions in include/pw_polish.h).  add -- one wavefront per pair and side (sides: 1
// origin, 2 mutant, 3 both) into counts and, when not null, ins[n_cols][J][L]; ocol0 / mcol0 / reversed: device arrays per pair
// or null; comp: the complement table, 32 bytes by value.  letters -- the self vote over [lo, hi).  count -- per read the
// emitted length into lens[n + 1] and the statistics record, then offsets[n + 1] = the exclusive sums of lens ([n] = total)
// through rocprim_run in `tmp`; write -- the letters at out[offsets[read] ..]
struct PolishComplement { uint32_t w[8]; };
}  // namespace pw
struct DeviceBuffer;
namespace pw {
hipError_t launch_polish_add(const PairDesc* pairs, const Result* results, const uint8_t* slots, const uint8_t* arena, int n, int sides,
                             const int64_t* ocol0, const int64_t* mcol0, const uint8_t* reversed, const PolishComplement& comp,
                             int64_t arena_first, uint32_t* counts, uint32_t* ins, int64_t n_cols, int L, int J, hipStream_t st);
hipError_t launch_polish_letters(uint32_t* counts, const uint8_t* letters, int64_t lo, int64_t hi, int L, uint32_t weight, hipStream_t st);
hipError_t launch_polish_count(const uint32_t* counts, const uint32_t* ins, const uint8_t* letters, const int64_t* roff, const int32_t* rlen,
                               int64_t n, int L, int J, uint32_t min_depth, uint64_t* lens, uint64_t* offsets, void* stats, DeviceBuffer& tmp,
                               hipStream_t st);
hipError_t launch_polish_write(const uint32_t* counts, const uint32_t* ins, const uint8_t* letters, const int64_t* roff, const int32_t* rlen,
                               int64_t n, int L, int J, uint32_t min_depth, const uint64_t* offsets, uint8_t* out, hipStream_t st);
// strip pipeline (pw_strip.h / pw_strip.hip): one standard-mode pair wider than a workgroup
struct StripParams;
struct StripTraceParams;
hipError_t launch_strip_fill(const StripParams& a, bool track, bool byte_rows, const uint32_t* ctl_init, int nworkers, int lds_bytes,
                             hipStream_t st);
hipError_t launch_strip_trace(const StripTraceParams& p, hipStream_t st);
hipError_t launch_xcc_census(uint32_t* d_seen8, hipStream_t st);
hipError_t launch_table_rowmajor(const void* plane, bool f64, int X, int Y, int pitch, double mul, double* out, hipStream_t st);

}  // namespace pw
#endif

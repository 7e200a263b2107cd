/* pw_overlap.h -- overlap band selection for MANY read pairs in one pass, on one MI355X.
 *
 * The reference discovers overlaps by scoring every pair of reads separately
 * (experiments/blot_overlaps.py:262-272: WordBlotOverlapRef(reads[i]).highest_scoring_overlap_band(reads[j])),
 * i.e. per pair biseqt/blot.py:497-579: all exact k-mer seeds, for every seed the number of seeds within 1 of it on
 * the scaled diagonal axis d / r(d), the estimated match probability of its diagonal band, the best band.
 * Everything in that computation depends on a seed only through its DIAGONAL, so for a batch of pairs the device
 * builds one histogram of seeds per (pair, diagonal) directly from a segmented sort-merge join of the k-mers
 * -- rows are never materialised -- and evaluates every occupied diagonal of every pair:
 *
 *   L(d)  = ceil( (2 / (2 - g)) * (min(|S| - d, |T|) + min(d, 0)) )          blot.py:78-112
 *   r(d)  = max(1, ceil( C * sqrt(L(d)) )),  C = erfcinv(1 - sensitivity) sqrt(2 g)   blot.py:116-139
 *   n(d)  = #{seeds with |d / r(d) - d' / r(d')| <= 1} - 1                   blot.py:521-527
 *   w(d)  = (n(d) + 1 - 2 r(d) L(d) p0^k) / L(d)                             blot.py:533-540  (p̂ = w^(1/k), monotone)
 *
 * in IEEE double with the reference's operation order.  The caller turns w into p̂ = min(exp(log(w) / k), 1)
 * (0 where w <= 0) and the z-score with the reference's closed forms; `tie` tells it when more than one diagonal
 * could reach the same p̂, in which case the reference's answer depends on its row order and the single-pair path
 * (pw_seeds.h) must be used for that pair.
 */
#ifndef PW_OVERLAP_H
#define PW_OVERLAP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
  uint64_t s_off, t_off;   /* offsets of the two reads in the letter arena (one byte per letter) */
  int32_t s_len, t_len;
} pw_read_pair;

typedef struct {
  int64_t n_seeds;         /* rows the pair's seeds table would hold */
  double w_best;           /* largest w(d) over the occupied diagonals (undefined when n_seeds == 0) */
  int32_t d_best;          /* its diagonal; among equal w the smallest d */
  int32_t n_best;          /* n(d_best): neighbours of a seed on that diagonal */
  int32_t r_best, len_best;        /* r(d_best), L(d_best) */
  int32_t band_best;       /* seeds with d in [d_best - r_best, d_best + r_best] (seed_count of the band) */
  int32_t tie;             /* occupied diagonals whose w is within 1e-9 relative of min(w_best, 1), i.e.
                              w >= c - |c| * 1e-9 with c = min(w_best, 1); all of them when w_best <= 0 */
  /* the first row of the reference's table order (k-mer asc, i asc, j asc): it wins when every p̂ is 0 */
  int32_t d_first, n_first, r_first, len_first, band_first;
  int32_t pad_;
} pw_overlap_band;         /* 64 bytes */

/* Scores all pairs.  radius_coeff = C above, len_coeff = 2 / (2 - g), word_p_null = (1 / alphabet_len)^wordlen --
 * computed by the caller exactly as the reference computes them (scipy erfcinv, numpy sqrt).  Synchronous.
 * Returns 0, or -1 (pw_overlap_last_error()). */
int pw_overlap_bands(int device, const uint8_t* arena, uint64_t arena_bytes, const pw_read_pair* pairs,
                     int64_t n_pairs, int alphabet_len, int wordlen, double len_coeff, double radius_coeff,
                     double word_p_null, pw_overlap_band* out);

/* ALL pairs of a set of reads through ONE k-mer index (every read is encoded and sorted once): the pairs (a < b)
 * that share at least one seed are found by a self join of the index; every other pair has no seeds and the
 * reference returns None for it.  read a plays S and read b plays T, as in the reference's double loop
 * (experiments/blot_overlaps.py:267-271).  On return *n_out pairs are listed in pair_a / pair_b (ascending
 * (a, b)) with their records in out; capacity max_pairs each.  Multi-GPU: rank shard_rank of shard_world scores
 * only the pairs with a mod shard_world == shard_rank (no data-path collective; (0, 1) = everything).
 * Returns 0 or -1. */
int pw_overlap_all_pairs(int device, const uint8_t* arena, uint64_t arena_bytes, const uint64_t* read_off,
                         const int32_t* read_len, int64_t n_reads, int alphabet_len, int wordlen, double len_coeff,
                         double radius_coeff, double word_p_null, int shard_rank, int shard_world,
                         int64_t max_pairs, int32_t* pair_a, int32_t* pair_b, pw_overlap_band* out,
                         int64_t* n_out);

/* ---- both strands ---------------------------------------------------------------------------------------------
 * Reads come from both strands of the molecule.  A minus-strand pair (a, b, '-') is the pair S = reads[a],
 * T = rc(reads[b]), the reverse complement of read b: position j' of T is letter len(b) - 1 - j' of reads[b],
 * complemented.  Diagonals, bands, the *_first fields -- and downstream start indices, end cells and transcripts -- are
 * all in the frame of that T; every record equals what the unstranded call returns for (a, rc(b)) with rc(b)
 * materialised.  The k-mer at position j' of rc(b) is the reverse complement of the k-mer of b at len(b) - k - j', so
 * the device computes the reverse-strand keys from the forward letters: rc(b) is never materialised for seeding.
 * `complement` is a table of alphabet_len bytes, a permutation of the letters that is its own inverse
 * (complement[complement[c]] == c); anything else is refused.
 * Documented exclusion: a read is never paired with its own reverse complement (hairpins are not looked for). */
#define PW_STRAND_PLUS 1
#define PW_STRAND_MINUS 2
#define PW_STRAND_BOTH 3

/* pw_overlap_bands with one strand flag per pair (0: T = the read as given, 1: T = its reverse complement).  strand == NULL
 * is pw_overlap_bands itself (the complement is then not read). */
int pw_overlap_bands_stranded(int device, const uint8_t* arena, uint64_t arena_bytes, const pw_read_pair* pairs,
                              int64_t n_pairs, int alphabet_len, int wordlen, double len_coeff, double radius_coeff,
                              double word_p_null, const uint8_t* complement, const uint8_t* strand, pw_overlap_band* out);

/* pw_overlap_all_pairs for the strands selected by `strands` (PW_STRAND_*): forward a x forward b and / or forward a x
 * reverse b, for a < b -- half of what an index over the reads plus their reverse complements would join.  pair_strand
 * receives 0 (+) or 1 (-) per listed pair; the order is ascending (a, b, strand).  PW_STRAND_PLUS runs the kernels of
 * pw_overlap_all_pairs and needs no complement.  Otherwise a second index of the same size holds the reverse-strand
 * k-mers: the limit of 2^32 k-mers applies per strand.  Sharding by a mod shard_world as above. */
int pw_overlap_all_pairs_stranded(int device, const uint8_t* arena, uint64_t arena_bytes, const uint64_t* read_off,
                                  const int32_t* read_len, int64_t n_reads, int alphabet_len, int wordlen,
                                  double len_coeff, double radius_coeff, double word_p_null, const uint8_t* complement,
                                  int strands, int shard_rank, int shard_world, int64_t max_pairs, int32_t* pair_a,
                                  int32_t* pair_b, uint8_t* pair_strand, pw_overlap_band* out, int64_t* n_out);

/* ---- the occurrence cap -----------------------------------------------------------------------------------------
 * pw_overlap_all_pairs_stranded with repetitive k-mers left out of the join.  occ(x) of a k-mer x is counted over the
 * WHOLE read set, whatever the shard (every rank builds the whole index): the forward entries with key x when strands ==
 * PW_STRAND_PLUS, otherwise those plus the reverse-index entries with key x -- exactly count(x) of a pw_kmers_build
 * (pw_kmers.h) with the same strands (PW_STRAND_MINUS counts as PW_STRAND_BOTH does).  A seed whose k-mer has occ(x) >
 * max_occ does not exist: it is not in n_seeds, in no histogram, band_* or *_first field, and a pair left without seeds
 * is not listed; occ(x) == max_occ is kept.  The masked entries never reach the seed expansion, so the refusals (2^32
 * seeds, max_pairs) are judged on what survives the cap, and the union of the ranks' outputs equals the unsharded output.
 * max_occ == 0: no cap -- the call is pw_overlap_all_pairs_stranded bit for bit, and stats is zeroed.
 * stats (may be NULL; zeroed first, filled once the join has run, also where a refusal follows it):
 *   entries          rows of the index: the k-mers of all reads, twice that with the reverse strand
 *   masked_entries   rows whose k-mer is masked           } over the whole read set,
 *   distinct_masked  distinct masked k-mers               } the same on every rank
 *   seeds_kept       the seeds this rank expanded (the sum of n_seeds over its listed pairs)
 *   seeds_dropped    the seeds this rank's masked entries would have produced: a 64-bit sum, never expanded */
typedef struct { uint64_t entries, masked_entries, distinct_masked, seeds_kept, seeds_dropped; } pw_overlap_cap_stats;
int pw_overlap_all_pairs_capped(int device, const uint8_t* arena, uint64_t arena_bytes, const uint64_t* read_off,
                                const int32_t* read_len, int64_t n_reads, int alphabet_len, int wordlen,
                                double len_coeff, double radius_coeff, double word_p_null, const uint8_t* complement,
                                int strands, int shard_rank, int shard_world, int64_t max_pairs, int32_t* pair_a,
                                int32_t* pair_b, uint8_t* pair_strand, pw_overlap_band* out, int64_t* n_out,
                                uint32_t max_occ, pw_overlap_cap_stats* stats);

/* ---- minimizer sampling ----------------------------------------------------------------------------------------------
 * pw_overlap_all_pairs_capped over an index that holds the WINDOW MINIMIZERS of every read only (pw_kmers.h states the rule:
 * the order value is mix(x) with PW_STRAND_PLUS and the canonical mix(min(x, rc(x))) with PW_STRAND_MINUS or PW_STRAND_BOTH,
 * every position that attains a window's minimum is selected).  Both indexes hold the same number of rows: under the
 * canonical order the selected positions of rc(read) mirror the read's own.  A seed exists only between two selected rows;
 * everything after the index is unchanged, so every field of every record is the documented record of the surviving seed
 * set.  The estimate behind w_best therefore sees fewer seeds than the unsampled call's and lies below it; d_best and r_best
 * are of the same kind as ever.  occ(x) of the cap counts the SAMPLED rows: count(x) of a pw_kmers_build_sampled with the same
 * strands and window; `entries` of the cap's stats counts sampled rows.  Two reads that share an exact stretch of window +
 * wordlen - 1 letters, on the strand joined, share a seed inside it.  Every rank samples the whole read set; the union of
 * the ranks equals the unsharded call.  The 2^32 limit on k-mers is judged on the unsampled positions, the one on seeds on
 * what survives.  window 0 or 1: pw_overlap_all_pairs_capped bit for bit; a window outside 0..128 is refused.
 * sample (may be NULL): the forward positions of the read set and how many of them the index kept (equal without a window). */
typedef struct { uint64_t positions, sampled; } pw_overlap_sample_stats;
int pw_overlap_all_pairs_sampled(int device, const uint8_t* arena, uint64_t arena_bytes, const uint64_t* read_off,
                                 const int32_t* read_len, int64_t n_reads, int alphabet_len, int wordlen,
                                 double len_coeff, double radius_coeff, double word_p_null, const uint8_t* complement,
                                 int strands, int shard_rank, int shard_world, int64_t max_pairs, int32_t* pair_a,
                                 int32_t* pair_b, uint8_t* pair_strand, pw_overlap_band* out, int64_t* n_out,
                                 uint32_t max_occ, pw_overlap_cap_stats* stats, int window,
                                 pw_overlap_sample_stats* sample);

/* Reads for the alignment stage: a device arena of total_bytes (+ the slack the kernels read) whose first `bytes` are the
 * host arena, uploaded once; behind them the device writes the reverse complement of n_frames reads: frame f =
 * rc(arena[src_off[f], src_off[f] + len[f])) at dst_off[f].  The dst frames ascend without overlap inside
 * [bytes, total_bytes) and start on 4-byte boundaries; the bytes between them are zero.  Batches created with
 * PW_FLAG_SHARED_ARENA (pw_batch.h) refer to these frames as ordinary mutant frames.  Free with pw_arena_free.
 * NULL on error.  pw_overlap_arena_read copies a piece of such an arena back to the host. */
void* pw_overlap_arena_upload(int device, const uint8_t* host_arena, uint64_t bytes, uint64_t total_bytes,
                              int64_t n_frames, const uint64_t* src_off, const uint64_t* dst_off, const int32_t* len,
                              const uint8_t* complement, int alphabet_len);
int pw_overlap_arena_read(int device, const void* dev_arena, uint64_t off, uint64_t bytes, uint8_t* host_out);

double pw_overlap_last_ms(void);           /* device time of the last call (HIP events) */
const char* pw_overlap_last_error(void);

#ifdef __cplusplus
}
#endif
#endif

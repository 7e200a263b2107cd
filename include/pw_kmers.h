/* pw_kmers.h -- the k-mer table of a whole read set, on one MI355X.
 *
 * The reference keeps the occurrences of every k-mer of a body of sequences in an SQLite table (biseqt/kmers.py:386-523,
 * KmerIndex: index_kmers, hits, kmers) and counts them in experiments/kmer_freq.py.  This is the computation in them, not
 * the storage: the sorted (k-mer, read, position) table of a read set in HBM, its runs of equal k-mers, and the questions
 * asked of it -- how often a k-mer occurs, where, and what the count-of-counts spectrum looks like.
 *
 * THE TABLE.  One row per (read r, position q) with 0 <= q <= read_len[r] - wordlen; a read shorter than wordlen, or empty,
 * has no rows.  The key of a row is the k-mer at q with its letters as digits in base alphabet_len (kmers.py:164-210).
 * With PW_STRAND_BOTH every such position contributes a SECOND row: its key is the k-mer at position q of rc(read r), the
 * reverse complement of the read (computed from the forward letters, rc(read) is never materialised), and its hit carries
 * strand 1 and q in the frame of rc(read).  count(x), the rows with key x, is then n_f(x) + n_f(rc(x)) with n_f the forward
 * rows: A K-MER THAT IS ITS OWN REVERSE COMPLEMENT COUNTS TWICE per occurrence.
 * Rows are ordered by (key, strand, read, pos); a hit is (read << 32) | (strand << 31) | pos.
 *
 * Limits and argument checks are those of pw_overlap_all_pairs (pw_overlap.h), with its messages: alphabet_len 1..36,
 * wordlen 1..31, alphabet_len ^ wordlen <= 2^62, fewer than 2^32 rows per strand, reads inside the arena, letters inside
 * the alphabet, the complement a permutation that is its own inverse.  Counts are 32-bit: a count above 2^32 - 1 (one k-mer
 * in every row of a two-strand table at the row limit) is reported as 2^32 - 1.
 *
 * THE SAMPLED TABLE (pw_kmers_build_sampled, window w in 1..128) keeps the WINDOW MINIMIZERS only.  For a read with
 * n = len - wordlen + 1 >= 1 positions let ww = min(w, n).  x(p) is the key at position p, x'(p) the key of its reverse
 * complement; the order value is h(p) = mix(x(p)) with PW_STRAND_PLUS and mix(min(x(p), x'(p))) with PW_STRAND_BOTH, where
 * mix is this bijection of the 64-bit integers (all arithmetic mod 2^64):
 *     z = x + 0x9E3779B97F4A7C15;  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9;  z = (z ^ (z >> 27)) * 0x94D049BB133111EB;
 *     mix = z ^ (z >> 31)
 * Position p is selected when some window of ww consecutive positions inside the read contains p and h(p) equals that
 * window's minimum; EVERY position that attains the minimum is selected, no tie is broken.  Equivalently: with lg the number
 * of consecutive positions left of p with h >= h(p) and rg the same to the right, both stopping at the read's ends and at
 * ww - 1, p is selected exactly when lg + rg + 1 >= ww.  So window 1 selects every position (pw_kmers_build, in every
 * output); a read with fewer than w positions still gets its minima; two sequences that share an exact substring of
 * w + wordlen - 1 letters share a selected k-mer inside it (on opposite strands too with BOTH); and with BOTH the selected set
 * of rc(read) is the mirror image n - 1 - p of the read's own, so the table holds as many strand-1 rows as strand-0 rows.
 * On random DNA about 2 / (w + 1) of the positions are selected.  The table holds the selected rows only, in the same row
 * order and hit format (positions are positions in the read, not ranks among the selected), and every query answers from
 * it: count(x) counts the selected occurrences.  All limits are judged on the unsampled positions.  The sampled build waits
 * for the number of selected rows before it sizes the table: it is synchronous up to there.
 *
 * pw_kmers_build waits for its uploads only (the host arrays are the caller's again once it returns); encode, sort, run
 * heads, scan and run lengths are asynchronous on `stream`, and the first call that returns host data waits for them.  It
 * may be called again on the same handle.  Every call returns 0, or -1 (pw_kmers_last_error(), per thread).
 * pw_kmers_last_ms(): the device time (HIP events) of the last query on this thread that ran a kernel; for the build, once
 * a call has waited for it -- e.g. pw_kmers_num_distinct straight after pw_kmers_build.
 */
#ifndef PW_KMERS_H
#define PW_KMERS_H

#include <stdint.h>

#include "pw_overlap.h" /* PW_STRAND_PLUS, PW_STRAND_BOTH */

#ifdef __cplusplus
extern "C" {
#endif

typedef struct pw_kmer_index pw_kmer_index;

pw_kmer_index* pw_kmers_create(int device, int alphabet_len, int wordlen);     /* NULL on error */
int pw_kmers_build(pw_kmer_index*, const uint8_t* arena, uint64_t arena_bytes, const uint64_t* read_off,
                   const int32_t* read_len, int64_t n_reads, int strands /* PW_STRAND_PLUS | PW_STRAND_BOTH */,
                   const uint8_t* complement /* alphabet_len bytes; read only for BOTH */, void* stream);
/* pw_kmers_build keeping the window minimizers only (above); window 1 is pw_kmers_build, a window outside 1..128 is refused */
int pw_kmers_build_sampled(pw_kmer_index*, const uint8_t* arena, uint64_t arena_bytes, const uint64_t* read_off,
                           const int32_t* read_len, int64_t n_reads, int strands, const uint8_t* complement, int window,
                           void* stream);
int64_t pw_kmers_num_entries(const pw_kmer_index*);     /* table rows; -1 before a build */
/* forward positions of the read set, sampled or not: the density of a sampled table is its forward rows (num_entries, half of
 * it for BOTH) divided by this; -1 before a build */
int64_t pw_kmers_num_positions(const pw_kmer_index*);
/* the whole table in table order: num_entries keys and hits; cap < num_entries is refused */
int pw_kmers_rows(pw_kmer_index*, uint64_t* keys_out, uint64_t* hits_out, int64_t cap);
/* out[r] = the forward rows of the reads before r, out[n_reads] = all forward rows: the rstart of pw_kmers_occurrences */
int pw_kmers_read_starts(pw_kmer_index*, uint64_t* out /* n_reads + 1 */);
int64_t pw_kmers_num_distinct(const pw_kmer_index*);    /* distinct keys; -1 on error */
/* the distinct k-mers, ascending, with their counts; cap < num_distinct is refused */
int pw_kmers_distinct(pw_kmer_index*, uint64_t* keys_out, uint32_t* counts_out, int64_t cap);
/* counts_out[i] = count(keys[i]); keys: host, any order, duplicates allowed; 0 for a k-mer that is absent (a key of
 * alphabet_len ^ wordlen or more is absent) */
int pw_kmers_lookup(pw_kmer_index*, const uint64_t* keys, int64_t n, uint32_t* counts_out);
/* the hits of one k-mer in table order; *n_out = count(key) always; cap < count(key) is refused, nothing is truncated */
int pw_kmers_hits(pw_kmer_index*, uint64_t key, uint64_t* hits_out, int64_t cap, int64_t* n_out);
/* hist_out[m], 1 <= m < max_mult: the distinct k-mers with count == m; hist_out[max_mult]: those with count >= max_mult;
 * hist_out[0] = 0.  max_mult in 1..65536.  64-bit integer counters: no result depends on the order of arrival. */
int pw_kmers_spectrum(pw_kmer_index*, int max_mult, uint64_t* hist_out /* max_mult + 1 */);
/* occ_out[rstart[r] + q] = count(key of (r, q)) for every FORWARD row, rstart[r] = the forward rows of the reads before r
 * (reads in the order given, positions ascending): the repeat profile of every read, num_entries (half of it for BOTH)
 * values.  On a sampled table: one value per sampled forward row in (read, pos) order, read r at the rstart[r] of
 * pw_kmers_read_starts. */
int pw_kmers_occurrences(pw_kmer_index*, uint32_t* occ_out);
void pw_kmers_destroy(pw_kmer_index*);

double pw_kmers_last_ms(void);
const char* pw_kmers_last_error(void);

#ifdef __cplusplus
}
#endif
#endif

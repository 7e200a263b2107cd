/* pw_polish.h -- read correction computed where the alignments are: two-sided pileups with the inserted letters recorded,
 * the self vote of every read, and polished reads (a count, a scan and a write), all on the device.
 *
 * NEW SURFACE (no reference counterpart), on top of include/pw_pileup.h: that header piles a pair onto its origin only and
 * counts insertion events without their letters, so a consensus from it can delete and substitute but cannot put a missing
 * letter back, and read b of a pair (a, b) never sees the pair.  Same shared object and error channel (pw_last_error) as
 * include/pw_batch.h.  Nothing of pw_pileup.h changes: pw_batch_pileup_add, pw_pileup_call and a pileup made by
 * pw_pileup_create behave as before.
 *
 * THE INSERTION PLANE.  A pileup may own, beside counts[n_cols][L + 2], a second array uint32_t ins[n_cols][J][L],
 * row-major, J = ins_slots in 1 .. 8.  Take a contributing pair in the sense of pw_pileup.h, with c = f + origin_idx,
 * q = mutant_idx, o(k) and m(k) as there, and a maximal run of l 'I' ops that starts at op k with o(k) > 0.  With
 * col = c + o(k) - 1, for every j < min(l, J):
 *     ins[col][j][y_j]++ with y_j = letter q + m(k) + j of the mutant frame; y_j >= L adds nothing.
 * A run with o(k) == 0 is anchored nowhere, exactly as its INS event is.  counts receives exactly what
 * pw_batch_pileup_add gives it.
 *
 * THE MUTANT SIDE.  Adding the pair (origin, mutant, t, origin_idx, mutant_idx) to its mutant's columns IS the origin-side
 * add of the swapped pair (mutant, origin, swap(t), mutant_idx, origin_idx), where swap exchanges 'D' and 'I'.  Its frame
 * starts at mutant_col0[pair], or at mutant_off - arena_first without that array, and the frame test is the origin side's:
 * the whole frame [f, f + Y) must lie inside [0, n_cols), else this side of the pair adds nothing.
 *
 * A REVERSED MUTANT SIDE (a minus-strand pair: the mutant frame holds rc(read b), the columns are read b's forward
 * letters).  Let n be the number of ops of t, so that o(n) and m(n) are its totals of origin-consuming and mutant-consuming
 * ops, and X, Y the lengths of the origin and the mutant frame.  The add IS the origin-side add of
 *     (b, rc(origin frame), reverse(swap(t))) with origin_idx' = Y - (mutant_idx + m(n)), mutant_idx' = X - (origin_idx + o(n)),
 * where letter u of rc(origin frame) is complement[origin[X - 1 - u]] (a letter >= L stays what it is and adds nothing).
 * Everything else follows from the one primitive: an insertion is anchored to the FORWARD letter on its left, the slot
 * order is forward order.
 *
 * POLISHING.  A read with letters s[0 .. n) at columns off .. off + n.  Its columns are visited in order; per column,
 * depth = the letter channels + DEL, summed in 64 bits.
 *     depth < min_depth:  emit s[x], nothing else.
 *     otherwise:          call = the first largest channel among the letters and DEL (the rule of pw_pileup_call); emit it
 *                         unless it is DEL.  Then for j = 0, 1, ..: with n_j = the sum over the letters of ins[col][j], emit
 *                         the first largest letter of slot j while j < J and 2 * n_j > depth (in 64 bits); stop at the
 *                         first slot that fails.
 * A pileup without an insertion plane emits no insertions.  A column emits 0 .. 1 + J letters.
 *
 * PER-READ STATISTICS.  pw_polish_stats, 16 bytes: kept (covered or not, the emitted letter is s[x]), substituted (another
 * letter was emitted), deleted (DEL was called), inserted (letters emitted from the slots).
 */
#ifndef PW_POLISH_H
#define PW_POLISH_H

#include <stdint.h>

#include "pw_pileup.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PW_POLISH_MAX_SLOTS 8
#define PW_SIDE_ORIGIN 1
#define PW_SIDE_MUTANT 2
#define PW_SIDE_BOTH 3

typedef struct { uint32_t kept; uint32_t substituted; uint32_t deleted; uint32_t inserted; } pw_polish_stats;   /* 16 bytes */

/* A pileup as pw_pileup_create makes it that also owns the insertion plane, zeroed.  NULL (and pw_last_error) for what
 * pw_pileup_create refuses, and for ins_slots outside 1 .. 8.  pw_pileup_clear zeroes the plane too; every function of
 * pw_pileup.h works on such a pileup as on any other. */
pw_pileup* pw_pileup_create_ins(int device, int64_t n_cols, int alphabet_len, int ins_slots);
int pw_pileup_ins_slots(const pw_pileup*);                 /* 0 for a pileup without a plane (and for NULL) */
void* pw_pileup_ins_counts_device(pw_pileup*);             /* uint32_t[n_cols][J][L]; NULL without a plane */
/* Synchronous D2H of the plane's columns [lo, hi), (hi - lo) * J * L counters; an error without a plane. */
int pw_pileup_ins_counts(pw_pileup*, int64_t lo, int64_t hi, uint32_t* host_out);

/* pw_batch_pileup_add for either side or both (the definitions above), asynchronous on `stream`.  sides: PW_SIDE_ORIGIN,
 * PW_SIDE_MUTANT or PW_SIDE_BOTH.  origin_col0, mutant_col0: host arrays of n_pairs frame starts, or NULL for
 * origin_off - arena_first and mutant_off - arena_first.  reversed: a host array of n_pairs bytes, non-zero where the
 * mutant side is reversed, or NULL; complement (alphabet_len bytes, complement[complement[c]] == c) is required as soon
 * as a byte of it is set.  Every host array is consumed at return, as col0 of pw_batch_pileup_add.  The pileup may or may
 * not own an insertion plane.  An error for any other `sides`, before any traceback of the batch, and when batch and
 * pileup live on different devices. */
int pw_batch_pileup_add_sides(pw_batch* b, pw_pileup* p, int sides, const int64_t* origin_col0, const int64_t* mutant_col0,
                              const uint8_t* reversed, const uint8_t* complement, int complement_len, int64_t arena_first,
                              void* stream);

/* The self vote: counts[c][letters_device[c - lo]] += weight for c in [lo, hi); a letter >= alphabet_len adds nothing.
 * Asynchronous on `stream`. */
int pw_pileup_add_letters(pw_pileup*, const uint8_t* letters_device /* hi - lo letters */, int64_t lo, int64_t hi, uint32_t weight,
                          void* stream);

/* Polish n_reads reads (the definition above): read r has its letters at letters_device[read_offs[r] ..] and its columns at
 * read_offs[r] .. read_offs[r] + read_lens[r] -- letters_device holds one letter per column of the pileup.  read_offs and
 * read_lens are host arrays, consumed at return.  The call counts on `stream`, waits for the total, allocates the output
 * from it, writes on `stream` and waits again: it is synchronous, nothing is ever written on an estimate.  An error for a
 * read that leaves [0, n_cols) or has a negative length. */
int pw_pileup_polish(pw_pileup*, const uint8_t* letters_device, const int64_t* read_offs, const int32_t* read_lens, int64_t n_reads,
                     uint32_t min_depth, void* stream);
/* The results of the last polish; each is an error (-1; NULL for the _device accessors) before the first one. */
int64_t pw_pileup_polished_total(pw_pileup*);                              /* letters emitted over all reads */
int pw_pileup_polished_offsets(pw_pileup*, int64_t* host_out);             /* n_reads + 1: read r is letters [off[r], off[r + 1]) */
int pw_pileup_polished_letters(pw_pileup*, uint8_t* host_out);             /* pw_pileup_polished_total bytes */
int pw_pileup_polished_stats(pw_pileup*, pw_polish_stats* host_out);       /* n_reads records */
void* pw_pileup_polished_letters_device(pw_pileup*);
void* pw_pileup_polished_offsets_device(pw_pileup*);

#ifdef __cplusplus
}
#endif
#endif

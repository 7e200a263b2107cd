/* pw_pileup.h -- pileups computed where the alignments are: the transcripts of a batch scattered into per-column base
 * counts of their origins, and the columns called (depth, consensus letter, variant flags), all on the device.
 *
 * NEW SURFACE (no reference counterpart): the reference keeps one alignment per Python object and has no column view; a
 * user who wants depth, a consensus or the sites where the reads disagree walks every transcript string op by op.  Here
 * the op bytes in the transcript slots, the letters in the arena and the start indices in the 32-byte records are read
 * where they are, and only counts or 8-byte site records come to the host.  Same shared object and error channel
 * (pw_last_error) as include/pw_batch.h.
 *
 * A pileup is uint32_t counts[n_cols][alphabet_len + 2], row-major: per column one channel per letter, then
 * PW_PILEUP_DEL (the 'D' ops over the column) and PW_PILEUP_INS (the insertion events anchored to the column).  The
 * counts are integers accumulated with integer atomics: they do not depend on the order of arrival.  A cell wraps past
 * 2^32 - 1 silently; keeping the depth below that is the caller's business.
 *
 * THE DEFINITION.  A pair contributes exactly when it has a summary in pw_txsum.h: PW_ST_TRACED set, none of PW_ST_EMPTY,
 * PW_ST_PANICK, PW_ST_BADPATH, tx_len > 0.  Its origin frame [f, f + X) must lie inside [0, n_cols), where f is
 * col0[pair], or origin_off - arena_first without a col0 array; a pair with f < 0 or f + X > n_cols contributes nothing.
 * Let t be the transcript, c = f + origin_idx, q = mutant_idx, o(k) the number of 'M', 'S', 'D' in t[:k] and m(k) the
 * number of 'M', 'S', 'I' in t[:k].  Then
 *     t[k] in 'M', 'S':  counts[c + o(k)][y]++ with y = letter q + m(k) of the mutant frame; y >= alphabet_len adds nothing;
 *     t[k] == 'D':       counts[c + o(k)][PW_PILEUP_DEL]++;
 *     t[k] == 'I' with k == 0 or t[k-1] != 'I' (an insertion EVENT, the rule of n_gaps):
 *                        counts[c + o(k) - 1][PW_PILEUP_INS]++ -- the event is anchored to the origin letter on its left
 *                        (samtools' convention) and counted nowhere when o(k) == 0;
 *     any other byte:    nothing.
 * The inserted letters themselves are not recorded, and only the origin side is piled up.
 */
#ifndef PW_PILEUP_H
#define PW_PILEUP_H

#include <stdint.h>

#include "pw_batch.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct pw_pileup pw_pileup;      /* device-resident uint32_t counts[n_cols][alphabet_len + 2], zeroed at creation */
#define PW_PILEUP_DEL(L) (L)             /* channel of 'D' ops */
#define PW_PILEUP_INS(L) ((L) + 1)       /* channel of insertion events */

/* NULL (and pw_last_error) for n_cols < 0, alphabet_len outside 1 .. 32, or a failed allocation. */
pw_pileup* pw_pileup_create(int device, int64_t n_cols, int alphabet_len);
void pw_pileup_destroy(pw_pileup*);
/* All counts back to zero, asynchronous on `stream`. */
int pw_pileup_clear(pw_pileup*, void* stream);
/* After pw_batch_traceback or pw_batch_traceback_from on the same stream: every contributing pair of the batch added to
 * the pileup (the definition above), asynchronous on `stream`.  col0: a host array of n_pairs frame starts, consumed at
 * return (the batch keeps its own host copy and uploads from that, as for the end cells of pw_batch_traceback_from: the
 * caller may overwrite or free the array as soon as the call returns, pageable or page-locked), or NULL for
 * origin_off - arena_first.  Adding is cumulative: two adds of one batch double its counts, several batches may
 * add to one pileup.  An error before any traceback of the batch, and when batch and pileup live on different devices. */
int pw_batch_pileup_add(pw_batch* b, pw_pileup* p, const int64_t* col0 /* host, n_pairs, or NULL */, int64_t arena_first,
                        void* stream);
void* pw_pileup_counts_device(pw_pileup*);
/* Synchronous D2H of columns [lo, hi) (as for pw_batch_results: callers that launched on another stream synchronise it
 * first); pw_pileup_set_counts is the opposite direction -- a pileup saved earlier, or one summed over several devices. */
int pw_pileup_counts(pw_pileup*, int64_t lo, int64_t hi, uint32_t* host_out);
int pw_pileup_set_counts(pw_pileup*, int64_t lo, int64_t hi, const uint32_t* host_in);

typedef struct { uint32_t depth; uint8_t call; uint8_t ref; uint16_t flags; } pw_pileup_site;   /* 8 bytes */
#define PW_PILEUP_COVERED 1   /* depth >= min_depth */
#define PW_PILEUP_DIFFERS 2   /* covered, a reference letter was given, call != ref */
#define PW_PILEUP_INSERT 4    /* covered and 2 * counts[INS] > depth */
/* One record per column, asynchronous on `stream`: depth = the sum of the alphabet_len letter channels plus DEL (modulo
 * 2^32); call = the channel in 0 .. alphabet_len (letters, then DEL) with the largest count, a tie going to the lowest
 * channel, or 255 when depth < min_depth or depth == 0; ref = ref_letters_device[column], or 255 when the pointer is
 * NULL; flags as above. */
int pw_pileup_call(pw_pileup*, const uint8_t* ref_letters_device /* n_cols letters, or NULL */, uint32_t min_depth, void* stream);
void* pw_pileup_sites_device(pw_pileup*);                                            /* pw_pileup_site[n_cols]; NULL before the first call */
int pw_pileup_sites(pw_pileup*, int64_t lo, int64_t hi, pw_pileup_site* host_out);   /* synchronous D2H; an error before the first call */

#ifdef __cplusplus
}
#endif
#endif

/* pw_txsum.h -- alignment summaries computed where the transcripts are: one 48-byte record per pair with the op
 * counts, the gap runs and the bounds of the first and last match, reduced on the device from the op bytes the
 * traceback left in the transcript slots.
 *
 * NEW SURFACE (no reference counterpart): the reference counts ops on Python strings, one alignment at a time
 * (pw.py:367-389 transcript lengths, pw.py:430-448 truncate_to_match).  A mapper or an overlapper that wants identity,
 * aligned length, gap counts and the match-to-match sub-alignment of many pairs reads these records instead of moving
 * and decoding the transcripts.  Same shared object and error channel (pw_last_error) as include/pw_batch.h.
 */
#ifndef PW_TXSUM_H
#define PW_TXSUM_H

#include <stdint.h>

#include "pw_batch.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Summary of one transcript t of length n; 12 int32, 48 bytes.  Identical on host and device, one per pair.  Bytes other
 * than 'M', 'S', 'I', 'D' are counted nowhere. */
typedef struct {
  int32_t n_match;      /* number of 'M' */
  int32_t n_subst;      /* number of 'S' */
  int32_t n_ins;        /* number of 'I' */
  int32_t n_del;        /* number of 'D' */
  int32_t n_gaps;       /* maximal runs of one gap letter: k with t[k] in {I, D} and (k == 0 or t[k-1] != t[k]); an I run
                           directly followed by a D run counts as two */
  int32_t first_match;  /* t.find('M'); -1 when there is no 'M' */
  int32_t last_match;   /* t.rfind('M'); -1 when there is no 'M' */
  int32_t head_origin;  /* letters of origin ('S' + 'D') consumed by t[:first_match]: what truncate_to_match adds to */
  int32_t head_mutant;  /* origin_start, and of mutant ('S' + 'I'): what it adds to mutant_start; 0 when there is no 'M' */
  int32_t tail_origin;  /* the same two counts over t[last_match + 1:]; 0 when there is no 'M' */
  int32_t tail_mutant;
  int32_t flags;        /* PW_TXSUM_DONE: a transcript was summarised.  A pair whose record lacks PW_ST_TRACED, or has
                           PW_ST_EMPTY, PW_ST_PANICK or PW_ST_BADPATH, or has tx_len <= 0, gets flags 0, both match
                           indices -1 and every other field 0. */
} pw_tx_summary;

#define PW_TXSUM_DONE 1

/* One wavefront per pair reduces the pair's ops (after pw_batch_traceback or pw_batch_traceback_from on the same stream)
 * into the batch's summary buffer, which is allocated on the first call and freed with the batch.  Asynchronous on
 * `stream`.  An error before any traceback of the batch.
 *
 * The summaries describe the traceback that preceded the call: after another traceback -- pw_batch_traceback,
 * pw_batch_traceback_from, or the repair of an abandoned strip pair inside pw_batch_results -- the buffer is stale until
 * pw_batch_summarize runs again.  pw_batch_summaries_device and pw_batch_summaries_async read the buffer as it is;
 * pw_batch_summaries (synchronous) runs the kernel again itself when a traceback has happened since the last summary. */
int pw_batch_summarize(pw_batch* b, void* stream);
void* pw_batch_summaries_device(pw_batch* b);            /* pw_tx_summary[n_pairs]; NULL before the first summary */
int pw_batch_summaries_async(pw_batch* b, pw_tx_summary* host_out, void* stream);   /* D2H ordered on `stream`; pinned memory */
int pw_batch_summaries(pw_batch* b, pw_tx_summary* host_out);                       /* synchronous D2H */

/* Stand-alone: n transcripts back to back in `ops`, transcript k being ops[offsets[k] .. offsets[k + 1]) (the layout of
 * pw_batch_pack_transcripts; offsets[n + 1] ascending, each transcript shorter than 2^31).  Host pointers: the bytes are
 * copied to `device`, summarised by the same device routine, and the n records copied back.  An empty transcript gets the
 * record of a pair without one.  n == 0 returns 0 and writes nothing. */
int pw_tx_summarize_packed(int device, const uint8_t* ops, const uint64_t* offsets, int64_t n, pw_tx_summary* out);

#ifdef __cplusplus
}
#endif
#endif

/* pw_cigar.h -- CIGARs computed where the transcripts are: the op bytes the traceback left in the transcript slots,
 * run-length encoded on the device into one dword per run, all pairs back to back, with their exclusive offsets.
 *
 * NEW SURFACE (no reference counterpart): the reference keeps an alignment as a Python string with one letter per op
 * (pw.py:322-365) and has no run-length form.  A mapper that writes PAF or BAM reads these runs instead of moving one byte
 * per op to the host and grouping Python strings.  Same shared object and error channel (pw_last_error) as
 * include/pw_batch.h.
 *
 * A run is one uint32_t, (length << 4) | op -- BAM's encoding.  The origin is the target and the mutant is the query:
 * transcript 'I' consumes a letter of the mutant only, 'D' of the origin only.
 *
 *     transcript byte   PW_CIGAR_EXTENDED      PW_CIGAR_CLASSIC
 *     'M'               '=' (op 7)             'M' (op 0)
 *     'S'               'X' (op 8)             'M' (op 0): adjacent 'M' and 'S' runs merge into one run
 *     'I'               'I' (op 1)             'I' (op 1)
 *     'D'               'D' (op 2)             'D' (op 2)
 *
 * A run is a maximal stretch of bytes of one op class; an 'I' run directly followed by a 'D' run is two runs (as for n_gaps
 * of pw_tx_summary).  Run lengths stay below 2^28: a batch with a transcript slot of 2^28 bytes or more, or a stand-alone
 * transcript that long, is refused.  Runs appear in transcript order.
 */
#ifndef PW_CIGAR_H
#define PW_CIGAR_H

#include <stdint.h>

#include "pw_batch.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PW_CIGAR_EXTENDED 0
#define PW_CIGAR_CLASSIC 1

#define PW_CIGAR_OP_M 0
#define PW_CIGAR_OP_I 1
#define PW_CIGAR_OP_D 2
#define PW_CIGAR_OP_EQ 7
#define PW_CIGAR_OP_X 8
#define PW_CIGAR_MAX_LEN 268435456 /* 2^28: every run length, hence every transcript, stays below it */

/* After pw_batch_traceback or pw_batch_traceback_from on the same stream: the runs of all pairs back to back in pair
 * order (uint32_t[total]) and their exclusive offsets (uint64_t[n_pairs + 1]; [n_pairs] = total runs), both
 * device-resident in buffers the batch owns.  A pair whose record lacks PW_ST_TRACED, or has PW_ST_EMPTY, PW_ST_PANICK or
 * PW_ST_BADPATH, or has tx_len <= 0 -- a pair without a summary in pw_txsum.h -- has zero runs.
 *
 * Three launches on `stream`: count the runs per pair, prefix-sum them, write the runs.  Between the second and the third
 * the 8-byte total is read back and `stream` is synchronised -- THE ONE BLOCKING READ of this call -- because the run
 * buffer is sized by it (it only grows).  An error before any traceback of the batch, or for an unknown form.
 *
 * The runs describe the traceback that preceded the call and the form of the call; pw_batch_cigar_runs_device and
 * pw_batch_cigar_offsets_device return the buffers as they are (NULL before the first call).  Both buffers are rewritten
 * in place by the next call: a call on another stream than the one before first waits for what was launched for the batch. */
int pw_batch_cigars(pw_batch* b, int form, void* stream);
void* pw_batch_cigar_runs_device(pw_batch* b);       /* uint32_t[total runs] */
void* pw_batch_cigar_offsets_device(pw_batch* b);    /* uint64_t[n_pairs + 1] */
uint64_t pw_batch_cigar_total(const pw_batch* b);    /* total runs of the last pw_batch_cigars (its read-back); 0 before */
/* Synchronous D2H of the offsets (n_pairs + 1) and / or the runs (either may be NULL).  Runs pw_batch_cigars itself (on
 * the default stream) when there are no runs yet, when a traceback has happened since, or when `form` differs from the
 * stored one.  With fewer than total runs of room (`cap`, in runs) it fails and writes nothing. */
int pw_batch_cigar(pw_batch* b, int form, uint32_t* runs_out, uint64_t cap, uint64_t* offsets_out);

/* Stand-alone: n transcripts back to back in `ops`, transcript k being ops[offsets[k] .. offsets[k + 1]) (the layout of
 * pw_batch_pack_transcripts).  Host pointers: the bytes are copied to `device`, encoded by the same device routine, and the
 * run offsets (uint64_t[n + 1]) and the runs (`cap` = room in runs_out, in runs) copied back.  runs_out == NULL: the
 * offsets alone, as a size query.  An empty transcript has zero runs.  n == 0 returns 0 and writes nothing.  Refused, before
 * anything is uploaded and with both outputs untouched: offsets that do not ascend, a transcript of 2^28 ops or more, any
 * byte other than 'M', 'S', 'I', 'D', an unknown form; and, with both outputs untouched, a `cap` below the total. */
int pw_tx_cigar_packed(int device, const uint8_t* ops, const uint64_t* offsets, int64_t n, int form, uint32_t* runs_out,
                       uint64_t cap, uint64_t* run_offsets_out);

#ifdef __cplusplus
}
#endif
#endif

/* pw_rounds.h -- iterated contig consensus: a polish that works one column at a time and yields, as a by-product, the map
 * from the columns of the draft to the letters of the polished contigs; the remap of the read placements through that map;
 * and the next round's tasks and arena laid out from the polished letters, all on the device.
 *
 * NEW SURFACE (no reference counterpart), on top of include/pw_polish.h (whose pileup, rule and result accessors it uses) and
 * include/pw_consensus.h (whose layout it iterates).  Same shared object and error channel (pw_last_error).  This comment IS
 * the contract: the CPU oracle (tests/rounds_ref.py) and the kernels (biseqt_amd/csrc/pw_rounds.hip) restate exactly this.
 * Nothing of the two headers changes: pw_pileup_polish, pw_graph_consensus_layout and every accessor behave as before.
 *
 * COLUMN POLISH.  The inputs of pw_pileup_polish, with one further condition: the reads come in column order and do not
 * overlap, read_offs[r] + read_lens[r] <= read_offs[r + 1].  Anything else is an error.  (pw_pileup_polish itself keeps
 * accepting overlapping reads.)
 *     e[c]      = the number of letters the POLISHING rule of pw_polish.h emits for column c when c lies in a read, 0 when
 *                 c lies in no read, for c in [0, n_cols);
 *     colmap[c] = the sum of e[c'] over c' < c, for c in 0 .. n_cols: n_cols + 1 entries of uint64;
 *     the letters of column c stand at out[colmap[c] ..];
 *     offsets[r] = colmap[read_offs[r]],  offsets[n_reads] = colmap[n_cols].
 * Letters, offsets, total and pw_polish_stats are exactly what pw_pileup_polish gives for the same arguments, and the
 * pw_pileup_polished_* accessors of pw_polish.h return them.
 *
 * ROUND REMAP.  A layout has contig lengths n_u, starts cstart, and a position pos per placed read; in round 1 these are the
 * build's lengths and the pos of pw_cons_place.  Given colmap of a column polish over exactly that layout's contigs (read u
 * of the polish is contig u: offset cstart[u], length n_u), define
 *     emap_u[x] = colmap[cstart[u] + x] - colmap[cstart[u]]  for x in 0 .. n_u,    n'_u = emap_u[n_u].
 * Then, in 64 bits,
 *     pos' = pos                    for pos < 0,
 *     pos' = emap_u[pos]            for 0 <= pos <= n_u,
 *     pos' = n'_u + (pos - n_u)     for pos > n_u.
 * unitig, rev, root and depth do not change; an unplaced read stays unplaced.
 *
 * RELAYOUT.  The next round's cstart, tasks and arena are the TASKS and CONSENSUS ARENA definitions of pw_consensus.h, word
 * for word, with three substitutions: length[u] := n'_u, pos := pos', contig letters := the polished letters.  The padding
 * bytes are 255, the frames come in task order with the same alignment rules.  A contig may polish to length 0; it then has
 * no tasks.  A contig of 2^31 letters or more is an error.  The task count may differ from the previous round's.
 */
#ifndef PW_ROUNDS_H
#define PW_ROUNDS_H

#include <stdint.h>

#include "pw_consensus.h"
#include "pw_polish.h"

#ifdef __cplusplus
extern "C" {
#endif

/* pw_pileup_polish by columns (the definition above).  Synchronous, as pw_pileup_polish is: counts, scans, waits for the
 * total, allocates from it and writes.  An error for what pw_pileup_polish refuses, for reads that are not in column order
 * and for reads that overlap; a refused call leaves the results of the last polish as they were. */
int pw_pileup_polish_columns(pw_pileup*, const uint8_t* letters_device, const int64_t* read_offs, const int32_t* read_lens,
                             int64_t n_reads, uint32_t min_depth, void* stream);
void* pw_pileup_colmap_device(pw_pileup*);                                   /* uint64_t[n_cols + 1]; NULL unless the last polish was by columns */
int pw_pileup_colmap(pw_pileup*, int64_t lo, int64_t hi, uint64_t* host_out);   /* entries [lo, hi), hi <= n_cols + 1; an error likewise */

/* The next round's layout (ROUND REMAP and RELAYOUT above) from plain device arrays: the polished contig letters, their
 * n_unitigs + 1 offsets (contig u is letters [off[u], off[u + 1]), n'_u of them) and the n_cols + 1 entries of colmap over
 * the CURRENT layout.  The three arrays are consumed before the current layout is dropped; they must not alias the graph's
 * arena.  letters_device, read_offs, complement, complement_len, slack, drift: as for pw_graph_consensus_layout.
 * Synchronous, as the layout is.  Afterwards the pw_graph_cons_* accessors of pw_consensus.h return the new round's values;
 * pw_graph_placements keeps returning the build's placements.  A new build, pw_graph_contigs or pw_graph_consensus_layout
 * resets to round 1.  An error before a layout, for whatever the layout refuses, and for offsets that disagree with colmap
 * about a contig's length; after an error there is no layout. */
int pw_graph_consensus_relayout(pw_graph*, const uint8_t* polished_device, const uint64_t* polished_offsets_device,
                                const uint64_t* colmap_device, const uint8_t* letters_device, const int64_t* read_offs,
                                const uint8_t* complement, int complement_len, int32_t slack, double drift, void* stream);
int pw_graph_cons_round(pw_graph*);                         /* 1 after pw_graph_consensus_layout, + 1 per relayout; an error (-1) before */
int pw_graph_cons_positions(pw_graph*, int64_t* host_out);  /* n_reads: pos of the current round, 0 for an unplaced read */
int pw_graph_cons_lengths(pw_graph*, int64_t* host_out);    /* n_unitigs: contig lengths of the current round */

#ifdef __cplusplus
}
#endif
#endif

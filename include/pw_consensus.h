/* pw_consensus.h -- the consensus stage of an overlap-layout-consensus assembler, prepared where the layout is: where every
 * read lies on its contig, the read-against-contig alignment tasks that follow from it, and one device arena that holds
 * the contig letters and the oriented reads, so that the existing aligner (include/pw_batch.h), pileup
 * (include/pw_pileup.h) and polish rule (include/pw_polish.h) turn draft contigs into polished ones without a letter or
 * a transcript leaving the device.
 *
 * NEW SURFACE (no reference counterpart).  Same shared object and error channel (pw_last_error) as include/pw_graph.h, on
 * whose graph (pw_graph) every call here works.  This comment IS the contract: the CPU oracle (tests/consensus_ref.py) and
 * the kernels (biseqt_amd/csrc/pw_consensus.hip) restate exactly this.  Terms of include/pw_graph.h (vertex, record,
 * class, contained, unitig, member, offset, advance, contig letters) are used as defined there.
 *
 * PLACEMENT.  After pw_graph_build every read r has one pw_cons_place record.  unitig == -1 means unplaced, and every
 * other field is then 0.  Otherwise the oriented read -- reads[r] for rev == 0, rc(reads[r]) for rev == 1 -- nominally
 * begins at letter pos of contig `unitig`; pos may be negative or reach past the contig's end.  root is the member read
 * the read hangs on (itself for a member), depth the containment links followed to reach it (0 for a member).
 *
 *   Members.  The member with the LOWEST member index whose vertex is 2r + o gives (unitig, rev = o, pos = its offset,
 *   root = r, depth = 0).  (A read occurs twice in a unitig that holds both of its orientations.)
 *
 *   Contained reads.  The parent record of a contained read c is chosen among the records with cls == A_CONTAINED && a == c
 *   or cls == B_CONTAINED && b == c: the largest n_match wins, a tie goes to the lowest record index (on the device: one
 *   64-bit atomic max of n_match << 32 | ~index, which does not depend on arrival order).  It gives (parent, rel, off):
 *   read c in orientation rel begins at off in the parent's FORWARD frame.  With la, lb the read lengths:
 *
 *     class                           strand  delta          parent  rel  off
 *     A_CONTAINED (child a, parent b)   0     b_beg - a_beg    b      0   delta
 *     A_CONTAINED                       1     b_beg - a_beg    b      1   lb - delta - la
 *     B_CONTAINED (child b, parent a)   0     a_beg - b_beg    a      0   delta
 *     B_CONTAINED                       1     a_beg - b_beg    a      1   delta
 *
 *   Dropped reads (include/pw_graph.h, CLEANING).  The parent record of a dropped read d is chosen among the records with cls
 *   in {A_TO_B, B_TO_A} that have d on one side and a LIVE read -- neither contained nor dropped -- on the other: the largest
 *   n_match wins, a tie goes to the lowest record index (the same 64-bit atomic max; a dropped read is never contained, so
 *   no entry sees both kinds of offer).  d is the child, and (parent, rel, off) follow the table above unchanged, by the rows
 *   "child a" / "child b" and the strand: the table's geometry does not depend on the class, only off may now be negative
 *   or pass the parent's end.  A dropped read without such a record is unplaced.  A contained read whose parent is dropped
 *   resolves through the doubling below like any other chain.  With nothing dropped the placements are what they were.
 *
 *   Composition.  A child placement (p, rel_c, off_c) of a read of lc letters on a read p of lp letters, composed with the
 *   placement (F, rel_p, off_p) of p -- F a grand-parent read or, at the root, a contig -- is
 *     rel_p == 0:  (F, rel_c,     off_p + off_c)
 *     rel_p == 1:  (F, rel_c ^ 1, off_p + lp - off_c - lc).
 *   The operation is associative; the device resolves the chains by pointer doubling in a fixed number of rounds,
 *   ceil(log2(max(n_reads, 2))) + 1, on ping-pong buffers, with 64-bit offsets.  A read whose chain reaches no member --
 *   it lies on, or leads into, a containment cycle (mutually contained duplicates) -- is unplaced, and so is a read whose
 *   root is no member.
 *
 * TASKS.  Parameters slack (int32 >= 0) and drift (a finite double >= 0; evaluated as written, no contraction).  The contig
 * starts form a padded layout, so that every origin frame is 4-byte aligned:
 *     cstart[0] = 0,  cstart[u + 1] = (cstart[u] + length[u] + 3) & ~3,  n_cols = cstart[n_unitigs];
 * a contig of 2^31 letters or more is an error.  For a placed read of l letters on contig u, with
 * radius = slack + (int64)((double)l * drift):
 *     lo = max(0, pos - radius) & ~3,  hi = min(length[u], pos + l + radius);
 * the read has a task iff l > 0 and max(pos, 0) < min(pos + l, length[u]).  With d0 = pos - lo the task is
 *     col0 = cstart[u] + lo,  mut_off (below),  read = r,  win_len = hi - lo,  dmin = max(d0 - radius, -l),
 *     dmax = min(d0 + radius, win_len),  rev = the placement's,  pad_ = 0:
 * the band of a B_OVERLAP alignment of the window [col0, col0 + win_len) (origin) with the oriented read (mutant) around the
 * nominal diagonal.  Tasks come in read order; they are counted, scanned and written -- nothing is written on an estimate.
 *
 * CONSENSUS ARENA.  One device allocation of arena_bytes bytes, with the 16 zero bytes of slack behind it that
 * pw_arena_upload gives.  Columns [0, n_cols) hold contig u at cstart[u], copied on the device from the contig letters of
 * pw_graph_contigs; the padding between two contigs is 255 (a letter that votes for nothing).  Behind them, from
 * base = (n_cols + 15) & ~15, come the mutant frames in task order: mut_off of the first task is base, every frame takes
 * (l + 15) / 16 * 16 + 16 bytes -- a 16-byte boundary and 16 bytes of slack each, as pack_reads lays reads out -- and
 * arena_bytes is the end of the last frame + 16.  A frame holds the read as stored (rev == 0) or its reverse complement
 * under the call's table (rev == 1; a letter >= complement_len stays what it is).  Every other byte from n_cols on is 0.
 *
 * Circular unitigs are NOT wrapped: a contig is a line from its head's cut.  A read that lies across the cut is placed at
 * one end, its window is clipped there, the overlap alignment clips the read, and the columns near the cut see less depth.
 */
#ifndef PW_CONSENSUS_H
#define PW_CONSENSUS_H

#include <stdint.h>

#include "pw_graph.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Plain records, identical on host and device. */
typedef struct {
  int32_t unitig, rev;
  int64_t pos;
  int32_t root, depth;
} pw_cons_place;                        /* 24 bytes */
typedef struct {
  int64_t col0, mut_off;
  int32_t read, win_len, dmin, dmax, rev, pad_;
} pw_cons_task;                         /* 40 bytes */

/* The placements of the last build (synchronous on `stream`).  An error before the first pw_graph_build.  A new
 * pw_graph_build drops the placements, the layout and everything the accessors below return. */
int pw_graph_place(pw_graph*, void* stream);
int pw_graph_placements(pw_graph*, pw_cons_place* host_out);        /* n_reads records; an error before pw_graph_place */
void* pw_graph_placements_device(pw_graph*);                        /* NULL before pw_graph_place */

/* cstart, the tasks and the consensus arena (the definitions above).  Runs pw_graph_place when the build has no
 * placements yet, and pw_graph_contigs (with these letters, offsets and table) when it has no contig letters yet.
 * letters_device, read_offs, complement, complement_len: as for pw_graph_contigs; the mutant frames are read from
 * letters_device[read_offs[r] .. + read_lens[r]).  Synchronous, as pw_graph_build is: counts, scans, waits for the totals,
 * allocates from them and writes.  An error before pw_graph_build, for a negative slack, a drift that is negative or not
 * finite, what pw_graph_contigs refuses, and for a contig of 2^31 letters or more.  A later pw_graph_contigs drops the
 * layout (the arena holds the letters of the earlier one); the placements stay. */
int pw_graph_consensus_layout(pw_graph*, const uint8_t* letters_device, const int64_t* read_offs, const uint8_t* complement,
                              int complement_len, int32_t slack, double drift, void* stream);
/* Its results; each is an error (-1; NULL) before the first pw_graph_consensus_layout after a build. */
int64_t pw_graph_cons_num_tasks(pw_graph*);
int64_t pw_graph_cons_num_cols(pw_graph*);
int64_t pw_graph_cons_arena_bytes(pw_graph*);
int pw_graph_cons_cstart(pw_graph*, int64_t* host_out);             /* num_unitigs + 1 */
int pw_graph_cons_tasks(pw_graph*, pw_cons_task* host_out);         /* num_tasks records */
void* pw_graph_cons_cstart_device(pw_graph*);
void* pw_graph_cons_tasks_device(pw_graph*);
void* pw_graph_cons_arena_device(pw_graph*);                        /* owned by the graph: never free it */

#ifdef __cplusplus
}
#endif
#endif

/* pw_graph.h -- the layout stage of an overlap-layout-consensus assembler, computed where the alignments are: overlap
 * records, their containment / dovetail classification, the overlap graph, its transitive reduction, unitigs and contig
 * letters, all on the device.
 *
 * NEW SURFACE (no reference counterpart: biseqt has no assembler).  The classification is the published containment /
 * dovetail rule of string-graph assemblers (Myers 2005, "The fragment assembly string graph"; Li 2016, "Minimap and
 * miniasm"), restated below.  Same shared object and error channel (pw_last_error) as include/pw_batch.h.  This comment IS
 * the contract: the CPU oracle (tests/graph_ref.py) and the kernels (biseqt_amd/csrc/pw_graph.hip) restate exactly this.
 *
 * VERTICES.  Read r has two vertices: 2r (the read as stored) and 2r + 1 (its reverse complement).  v ^ 1 is the other
 * orientation of v.  V = 2 * n_reads.
 *
 * OVERLAP RECORD.  One record per aligned pair (a, b, strand), a != b, both below n_reads.  A = reads[a]; B' = reads[b]
 * (strand 0) or rc(reads[b]) (strand 1) -- the frame of a minus pair of the overlap path.  The intervals are
 * [a_beg, a_end) on A and [b_beg, b_end) on B'; n_match and n_ops are recorded beside them.  la, lb: the read lengths.
 * From a batch (pw_batch_graph_add), with the pair's pw_result and pw_tx_summary:
 *     a_beg = origin_idx, a_end = a_beg + n_match + n_subst + n_del;
 *     b_beg = mutant_idx, b_end = b_beg + n_match + n_subst + n_ins;   n_ops = the sum of the four counts.
 * A pair without an alignment (no PW_TXSUM_DONE) is stored with every interval end, n_match and n_ops zero: n_ops == 0
 * IS "no alignment", for a planted record too.  At most one record per key (a, b, strand); a duplicate key is an error
 * (found on the host when the record is added, reported by pw_graph_build).
 *
 * CLASSIFICATION.  Parameters max_hang, int_frac, min_overlap, min_identity, fuzz.  Doubles are evaluated as written, no
 * contraction; min(x, y) of two doubles is y < x ? y : x; integer sums are taken in 64 bits.  The first rule that applies
 * decides:
 *   1. NONE         n_ops == 0.
 *   2. WEAK         min(a_end - a_beg, b_end - b_beg) < min_overlap, or (double)n_match < min_identity * (double)n_ops.
 *   3. INTERNAL     with ext = min(a_beg, b_beg) + min(la - a_end, lb - b_end) and span = max(a_end - a_beg, b_end - b_beg):
 *                   (double)ext > min((double)max_hang, (double)span * int_frac).
 *   4. A_CONTAINED  a_beg <= b_beg && la - a_end <= lb - b_end.
 *   5. B_CONTAINED  a_beg >= b_beg && la - a_end >= lb - b_end.
 *   6. A_TO_B       a_beg > b_beg.
 *   7. B_TO_A       otherwise.
 * Read r is CONTAINED iff some record classifies it so: a for A_CONTAINED, b for B_CONTAINED.
 *
 * ARCS.  Only dovetail records (A_TO_B, B_TO_A) whose two reads are both not contained give arcs.  The t-th such record,
 * in record order, gives exactly two, an arc and its twin, at the generation positions 2t and 2t + 1:
 *   A_TO_B:  (2a -> 2b + strand,           len = a_beg - b_beg,                   ol = a_end - a_beg)
 *            ((2b + strand) ^ 1 -> 2a + 1, len = (lb - b_end) - (la - a_end),     ol = b_end - b_beg)
 *   B_TO_A:  (2b + strand -> 2a,           len = b_beg - a_beg,                   ol = b_end - b_beg)
 *            (2a + 1 -> (2b + strand) ^ 1, len = (la - a_end) - (lb - b_end),     ol = a_end - a_beg)
 * Every len >= 1, because the containment rules take every tie.  ol is the overlap length on the arc's tail read, src the
 * index of its record.  The arc table is the generated arcs sorted by (v, len, generation position) -- a stable sort on
 * (v, len) -- and rows[V + 1] is the CSR row index over v: the arcs leaving v are [rows[v], rows[v + 1]).
 *
 * TRANSITIVE REDUCTION.  E is the arc table.  Arc v -> x is REDUCED iff there are arcs v -> w and w -> x in E with w != x
 * and len(v -> w) + len(w -> x) <= len(v -> x) + fuzz.  The definition is order-independent: whether v -> w is itself
 * reduced does not matter.  An arc is REMOVED iff it or its twin is reduced.  The kept arcs are the rest.
 *
 * UNITIGS.  out(v) is the number of kept arcs leaving v.  A kept arc v -> w is a CHAIN link iff out(v) == 1 &&
 * out(w ^ 1) == 1 && w != v && w != (v ^ 1).  Every vertex then has at most one chain successor and at most one chain
 * predecessor, and the components over the vertices of the reads that are not contained are paths or cycles; an isolated
 * vertex is a path of one.  A cycle's head is its smallest vertex: the link entering it is cut, and the unitig is flagged
 * circular.  A component is kept iff its smallest vertex is even -- its reverse-complement twin is the one dropped; a
 * component that holds both orientations of its smallest read is its own twin and is kept once.  Unitigs are numbered in
 * ascending order of their head vertex.  A member has its rank in the path (its index among the unitig's members), its
 * advance -- the len of its chain link to the next member; for the last member of a linear unitig the read length; for the
 * last member of a circular one the len of its link back to the head -- and its offset, the sum of the advances before
 * it.  The unitig's length is the sum of all advances.
 *
 * CLEANING (pw_graph_build_clean: tip removal and bubble popping, between the reduction and the unitigs).  Parameters, all
 * int32: max_tip_reads >= 0, max_bubble_reads >= 0, rounds in 0 .. 8.  With rounds == 0, or both maxima 0, nothing is dropped
 * and the build is exactly pw_graph_build's.  Everything is evaluated on the arcs that are not REMOVED, after reduction and
 * twins.  A read is LIVE iff it is neither contained nor dropped; a vertex is live iff its read is.  out(v) is as in UNITIGS,
 * and in(v) = out(v ^ 1): REMOVED is twin-symmetric and reads are dropped whole, so the kept arcs entering v are the twins
 * of the kept arcs leaving v ^ 1.  Where UNITIGS says "the reads that are not contained", read "the live reads".
 *   A ROUND.  (1) The chain links and components over the live vertices, exactly as UNITIGS defines them.  (2) For a linear
 *   (not circular) component C: h is its head, t its tail (its last member), n its member count, mr(C) its smallest vertex
 *   >> 1.  (3) TIPS and BUBBLES below are decided for every component, of both orientations, on this one decomposition.
 *   (4) Every read that has a vertex in a dropped component is dropped: dropped[r] = 1 for a tip, 2 for a bubble.  (5) Every
 *   arc that is not yet REMOVED and has an end on a dropped read gets REMOVED | DROPPED.
 *   The rounds are a fixed count, not a loop on a flag: a round that drops nothing changes nothing.  After the last round
 *   the UNITIGS pass runs once over the live vertices and gives the unitigs, the members and the CHAIN flags; the chain
 *   links of the rounds leave no CHAIN flag behind.  A dropped read is in no unitig.
 *   TIPS (max_tip_reads > 0).  C is a tip candidate iff it is linear, n <= max_tip_reads, in(h) == 0 and out(t) >= 1.  A kept
 *   arc u -> w with u != t COMPETES with C at w iff C has a kept arc t -> w; u is then the tail of its component D (w has
 *   two kept arcs entering it, so u -> w is no chain link).  D is STRONGER than C iff D is no tip candidate, or n_D > n_C,
 *   or n_D == n_C and mr(D) < mr(C).  C is dropped iff some competing arc at some w comes from a stronger D.
 *     - A dead-end spur (in(h) >= 1, out(t) == 0) is caught through its reverse-complement component, which is a dead start.
 *     - Of the two short branches of a Y the better one survives: the longer, at equal length the one with the smaller mr.
 *     - A short path that is the only way into a fork is kept: nothing competes with it.
 *     - An isolated component is never a tip: out(t) == 0.
 *   BUBBLES (max_bubble_reads > 0).  C is a bubble candidate iff it is linear, n <= max_bubble_reads, in(h) == 1,
 *   out(t) == 1, and, with s the tail of the one kept arc entering h and z the head of the one kept arc leaving t, neither
 *   s >> 1 nor z >> 1 is the read of h or of t.  C is dropped iff another bubble candidate D with (s_D, z_D) == (s_C, z_C)
 *   has n_D > n_C, or n_D == n_C and mr(D) < mr(C).  Of k parallel paths exactly one survives; equal n and equal mr (a
 *   component against its own twin, in a hairpin z == s ^ 1) drops neither.
 *   Both rules compare only n and mr, which a component shares with its twin C ^ 1 (the reverse complements of its members
 *   in reverse order), so the decisions for C and C ^ 1 never contradict each other: C is a bubble candidate, and dropped as
 *   one, iff C ^ 1 is; C and C ^ 1 are never both tip candidates; and no read is dropped as a tip through one of its
 *   vertices and as a bubble through the other.  dropped[r] is therefore one well-defined value.
 *
 * CONTIG LETTERS.  Members in order; each contributes the first `advance` letters of its oriented read.  The letters of
 * 2r + 1 are those of rc(reads[r]) under the call's complement table; a letter >= complement_len stays what it is.  There
 * is no consensus here.
 */
#ifndef PW_GRAPH_H
#define PW_GRAPH_H

#include <stdint.h>

#include "pw_batch.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { PW_OVL_NONE = 0, PW_OVL_WEAK = 1, PW_OVL_INTERNAL = 2, PW_OVL_A_CONTAINED = 3, PW_OVL_B_CONTAINED = 4, PW_OVL_A_TO_B = 5,
       PW_OVL_B_TO_A = 6 };
#define PW_ARC_REDUCED 1
#define PW_ARC_REMOVED 2
#define PW_ARC_CHAIN 4
#define PW_ARC_DROPPED 0x8              /* 8: removed by CLEANING (always beside PW_ARC_REMOVED) */

/* Plain records, identical on host and device. */
typedef struct {
  int32_t a, b, strand;
  int32_t cls;                          /* output of pw_graph_build (PW_OVL_*); ignored on input, 0 until the first build */
  int32_t a_beg, a_end, b_beg, b_end;
  int32_t n_match, n_ops;
} pw_graph_overlap;                     /* 40 bytes */
typedef struct {
  int32_t max_hang, min_overlap, fuzz, pad_;
  double int_frac, min_identity;
} pw_graph_params;                      /* 32 bytes */
typedef struct { int32_t max_tip_reads, max_bubble_reads, rounds, pad_; } pw_graph_clean_params;      /* 16 bytes; CLEANING */
typedef struct { int32_t v, w, len, ol, src, flags; } pw_graph_arc;              /* 24 bytes; flags: PW_ARC_* */
typedef struct {
  int64_t first_member;                 /* its members are [first_member, first_member + n_members) */
  int64_t length;
  int32_t n_members, head, circular, pad_;
} pw_unitig;                            /* 32 bytes */
typedef struct { int32_t vertex, advance; int64_t offset; } pw_unitig_member;    /* 16 bytes; the rank is the index */

typedef struct pw_graph pw_graph;

/* An empty graph over n_reads reads of the lengths read_lens (host array, consumed at return).  NULL (and pw_last_error)
 * for n_reads outside 0 .. 2^28 and for a negative length. */
pw_graph* pw_graph_create(int device, int64_t n_reads, const int32_t* read_lens);
void pw_graph_free(pw_graph*);
int64_t pw_graph_num_overlaps(const pw_graph*);
int64_t pw_graph_device_bytes(const pw_graph*);            /* what the graph holds on the device at present */

/* Append n planted records (host array).  An error, and nothing is appended, for a read index outside the graph, a == b,
 * a strand other than 0 / 1, an interval with not 0 <= beg <= end <= len, and not 0 <= n_match <= n_ops. */
int pw_graph_add_overlaps(pw_graph*, const pw_graph_overlap* host_records, int64_t n);

/* Append one record per pair of the batch, after a traceback of the batch on `stream`: pair k is the pair
 * (read_a[k], read_b[k], strand[k]) (host arrays of n_pairs entries, consumed at return; strand NULL: all 0), so the
 * index of its record is the number of records before the call + k.  A pair without an alignment gives a NONE record.
 * Runs pw_batch_summarize itself when the batch's summaries are stale (the rule of pw_batch_summaries).  Asynchronous on
 * `stream`.  An error unless the origin frame of pair k is as long as read read_a[k] and the mutant frame as long as read
 * read_b[k] (the frames must be the whole reads), for what pw_graph_add_overlaps refuses, before any traceback, and when
 * batch and graph live on different devices. */
int pw_batch_graph_add(pw_batch*, pw_graph*, const int32_t* read_a, const int32_t* read_b, const uint8_t* strand, void* stream);

/* Classification, contained flags, arcs, sort and row index, reduction, twins, chain links, unitigs and members of the
 * records added so far.  Synchronous: every stage counts on `stream`, waits for its total, allocates from it and writes;
 * nothing is ever written on an estimate.  A second build, with other parameters or after more records, replaces the
 * first and drops the contig letters.  An error for a duplicate key, for int_frac or min_identity that is not finite, and
 * for a negative max_hang, min_overlap or fuzz. */
int pw_graph_build(pw_graph*, const pw_graph_params*, void* stream);
/* pw_graph_build with the CLEANING rounds between the reduction and the unitigs.  A NULL third argument is pw_graph_build
 * (which is this call).  An error, besides what pw_graph_build refuses, for a negative maximum and for rounds outside 0 .. 8. */
int pw_graph_build_clean(pw_graph*, const pw_graph_params*, const pw_graph_clean_params*, void* stream);

/* Results of the last build.  The counts are -1 and every accessor an error (NULL for the _device forms) before the
 * first build -- except the overlaps, which may be read at any time (cls is then that of the last build, 0 for records
 * added since).  The host forms are synchronous copies into arrays of the stated sizes. */
int64_t pw_graph_num_arcs(pw_graph*);
int64_t pw_graph_num_unitigs(pw_graph*);
int64_t pw_graph_num_members(pw_graph*);
/* Device time of the reduction kernel in the last build, in ms, between two events on the build's stream; -1 before the
 * first build and when the build had no arcs. */
double pw_graph_reduce_ms(pw_graph*);
int pw_graph_overlaps(pw_graph*, pw_graph_overlap* host_out);       /* num_overlaps records */
int pw_graph_contained(pw_graph*, uint8_t* host_out);               /* n_reads bytes, 0 / 1 */
int pw_graph_dropped(pw_graph*, uint8_t* host_out);                 /* n_reads bytes: 0, 1 (tip) or 2 (bubble); all 0 without cleaning */
int pw_graph_arcs(pw_graph*, pw_graph_arc* host_out);               /* num_arcs records, sorted */
int pw_graph_rows(pw_graph*, int64_t* host_out);                    /* 2 * n_reads + 1 */
int pw_graph_unitigs(pw_graph*, pw_unitig* host_out);               /* num_unitigs records */
int pw_graph_members(pw_graph*, pw_unitig_member* host_out);        /* num_members records */
void* pw_graph_overlaps_device(pw_graph*);
void* pw_graph_contained_device(pw_graph*);
void* pw_graph_dropped_device(pw_graph*);
void* pw_graph_arcs_device(pw_graph*);
void* pw_graph_rows_device(pw_graph*);
void* pw_graph_unitigs_device(pw_graph*);
void* pw_graph_members_device(pw_graph*);

/* The contig letters of the last build (the definition above): read r has its letters at
 * letters_device[read_offs[r] .. read_offs[r] + read_lens[r]) (read_offs: host array of n_reads entries, consumed at
 * return).  complement: complement_len bytes (1 .. 256); NULL stands for the identity (an odd vertex is then read backwards
 * and nothing more -- right only when no member is an odd vertex).  Counts, scans and writes on `stream`, synchronous as
 * pw_graph_build.  The first `advance` letters of a member never pass its read: advance <= the read length by
 * construction, and the kernel stops at the read's end all the same. */
int pw_graph_contigs(pw_graph*, const uint8_t* letters_device, const int64_t* read_offs, const uint8_t* complement, int complement_len,
                     void* stream);
/* Its results; each is an error (-1; NULL) before the first pw_graph_contigs after a build. */
int64_t pw_graph_contig_total(pw_graph*);                           /* letters over all contigs */
int pw_graph_contig_offsets(pw_graph*, int64_t* host_out);          /* num_unitigs + 1: contig u is [off[u], off[u + 1]) */
int pw_graph_contig_letters(pw_graph*, uint8_t* host_out);          /* pw_graph_contig_total bytes */
void* pw_graph_contig_letters_device(pw_graph*);
void* pw_graph_contig_offsets_device(pw_graph*);

#ifdef __cplusplus
}
#endif
#endif

/* pw_qseeds.h -- exact-match k-mer seeds of MANY queries against ONE reference sequence, in diagonal coordinates, on
 * one MI355X.
 *
 * C ABI of the query-batched Word-Blot.  The reference's in-memory class (biseqt/blot.py:582-700, WordBlotLocalRef)
 * keeps the k-mer hits of one sequence and is then asked about one query after the other; its experiments loop over
 * hundreds of short queries (experiments/blot_ig_genotyping.py:50-76).  Here the reference sequence is encoded and sorted
 * once, and the seeds, the neighbourhood graph, its components and the segments' seed counts of ALL queries come out of
 * one set of launches whose number does not depend on the number of queries.
 *
 * A row is (q, d, a): query number, d = i - j, a = i + j for position i of the reference and j of query q.  Rows are in
 * (q, j, i) order -- per query the order in which the in-memory classes list their seeds (blot.py:607-620: the query
 * scanned left to right, the reference's hits of a k-mer ascending).  No mask (the in-memory classes take none) and no
 * self comparison: a query equal to the reference is compared like any other (the caller routes such a query elsewhere).
 *
 * Strands (pw_qseeds_build_stranded): a listed query with strand 1 IS the sequence T = rc(query) -- position j' of T is
 * letter len - 1 - j' of the query, complemented; the convention of include/pw_overlap.h.  Its rows, and everything
 * derived from them (graph, components, box counts), are in the frame of that T and equal, field for field, what the
 * unstranded build returns when rc(query) is materialised and passed as an ordinary query.  The device computes the
 * reverse-strand keys from the forward letters: rc(query) is never materialised for seeding.
 *
 * Plain pointers and sizes only; letters are one byte each (index into the alphabet).  Everything fails loudly
 * (NULL / negative return + pw_qseeds_last_error()); there is no CPU fallback.
 */
#ifndef PW_QSEEDS_H
#define PW_QSEEDS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct pw_qseed_index pw_qseed_index;

/* Copies ref[0 .. n_ref) to the device `device`, encodes its k-mers and sorts them (and, for small key spaces, fills the
 * direct-address table of the join); every later call on the handle reuses that.  n_ref < 2^31; alphabet_len L <= 36 and
 * wordlen k with L^k < 2^62 (4-byte keys when L^k < 2^32 - 1). */
pw_qseed_index* pw_qseeds_create(int device, const uint8_t* ref, int64_t n_ref, int alphabet_len, int wordlen);

/* The seeds of n_queries queries on `stream` (a hipStream_t); synchronous.  Query q occupies
 * arena[offsets[q] .. offsets[q] + lengths[q]) -- the layout of a read arena; a k-mer never runs past the end of its own
 * query.  `arena` is a host pointer (copied to the device) or, with arena_on_device != 0, a device pointer to an arena of
 * arena_bytes bytes that is read in place.  The lengths sum to less than 2^31.  The row total saturates at 2^64 - 1
 * instead of wrapping.  Returns 0, or -1 when a letter lies outside the alphabet or the table would hold more than
 * max_rows rows (max_rows <= 0: the default, 2^30; never more than 2^31 - 1, the graph indexes rows with int32). */
int pw_qseeds_build(pw_qseed_index* idx, const uint8_t* arena, uint64_t arena_bytes, int arena_on_device,
                    const int64_t* offsets, const int32_t* lengths, int64_t n_queries, int64_t max_rows, void* stream);

/* pw_qseeds_build with a strand per listed query: strand[q] is 0 (as given) or 1 (reverse complement); any other value
 * returns -1.  strand == NULL is pw_qseeds_build itself, and the complement is not read.  `complement` is alphabet_len
 * bytes, complement[c] for every letter c: a permutation that is its own inverse (checked as pw_overlap.h's; anything else
 * returns -1).  It is required only when some strand[q] == 1.  Two listed entries may name the same bytes with different
 * strands: that is how a caller asks for both strands of a query.  The limit "lengths sum to less than 2^31" applies to
 * the LISTED entries, so both strands of a read set allow 2^30 letters.  A row of a minus entry is (q, i - j', i + j') for
 * position j' of rc(query); rows are in (q, j', i) order.  Every letter of every listed query is validated on either
 * strand; a minus entry is read backwards from its last letter and never below offsets[q].  After a refused build the
 * handle stays usable. */
int pw_qseeds_build_stranded(pw_qseed_index* idx, const uint8_t* arena, uint64_t arena_bytes, int arena_on_device,
                             const int64_t* offsets, const int32_t* lengths, const uint8_t* strand,
                             const uint8_t* complement, int64_t n_queries, int64_t max_rows, void* stream);

int64_t pw_qseeds_num_queries(const pw_qseed_index* idx);
int64_t pw_qseeds_num_rows(const pw_qseed_index* idx);

/* Rows in table order, 3 int32 each: (q, d, a); the rows of query q are [row_offsets[q], row_offsets[q + 1]).  On the
 * device (valid until the next build / destroy) or copied to the host (cap = capacity in rows; row_offsets:
 * n_queries + 1 entries). */
const int32_t* pw_qseeds_rows_device(const pw_qseed_index* idx);
int pw_qseeds_rows(const pw_qseed_index* idx, int32_t* rows, int64_t cap);
int pw_qseeds_row_offsets(const pw_qseed_index* idx, int64_t* row_offsets);

/* COUNT(*) of the rows of query q[b] with dmin[b] <= d <= dmax[b] and amin[b] <= a <= amax[b], for n_boxes boxes in one
 * launch.  counts: n_boxes entries. */
int pw_qseeds_count_boxes(const pw_qseed_index* idx, int64_t n_boxes, const int32_t* q, const int32_t* dmin,
                          const int32_t* dmax, const int32_t* amin, const int32_t* amax, int64_t* counts);

/* Local-similarity support (blot.py:343-374, 410-490).  pw_qseeds_graph_build links every two rows OF THE SAME QUERY with
 *     fl(|fl(d c) - fl(d' c)|) <= radius  and  |a - a'| <= radius
 * -- cKDTree.query_ball_tree(radius, p = inf) over (d c, a) per query, each row's own entry removed -- and keeps the
 * adjacency in HBM as CSR.  Returns the number of directed edges (every pair counts twice), or -1 -- also when the sort
 * key (query, diagonal, antidiagonal) would need more than 64 bits. */
int64_t pw_qseeds_graph_build(pw_qseed_index* idx, double d_coeff, double radius);
int pw_qseeds_graph_counts(const pw_qseed_index* idx, int32_t* counts, int64_t cap);     /* neighbours per row */
/* offsets: num_rows + 1 entries; neighbours: pw_qseeds_graph_build's return value entries (row indices, order inside a
 * row's list unspecified). */
int pw_qseeds_graph_fetch(const pw_qseed_index* idx, int64_t* offsets, int32_t* neighbours);
/* Connected components of the graph restricted to the rows with avail[row] != 0: labels[row] = smallest row index of
 * its component -- the query's first seed of that component in presentation order -- and -1 for rows that are not
 * available.  Edges never cross queries: one fixed-point iteration serves all of them. */
int pw_qseeds_graph_components(const pw_qseed_index* idx, const uint8_t* avail, int32_t* labels);

double pw_qseeds_build_ms(const pw_qseed_index* idx);           /* device time of the last build (HIP events) */
double pw_qseeds_graph_ms(const pw_qseed_index* idx);           /* ... of the last graph build */
double pw_qseeds_components_ms(const pw_qseed_index* idx);      /* ... of the last components call */
double pw_qseeds_count_ms(const pw_qseed_index* idx);           /* ... of the last count_boxes call */
int pw_qseeds_components_rounds(const pw_qseed_index* idx);     /* hook rounds of the last components call */
void pw_qseeds_destroy(pw_qseed_index* idx);
const char* pw_qseeds_last_error(void);

#ifdef __cplusplus
}
#endif
#endif

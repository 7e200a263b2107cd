/* pw_mseeds.h -- exact-match k-mer seeds shared by N = 2 .. 16 sequences, in diagonal coordinates, on one MI355X.
 *
 * C ABI of the multiple-sequence Word-Blot.  It replaces, for N sequences, what the reference builds in Python:
 *
 *   biseqt/seeds.py:234-433   SeedIndexMultiple           one row (d_1 .. d_{N-1}, a) per N-tuple of positions that
 *                                                         carry the same k-mer: d_k = i_1 - i_{k+1}, a = sum of i_k
 *                                                         (seeds.py:262-274); seed_count over hyper-boxes
 *   biseqt/blot.py:1040-1083  WordBlotMultipleFast.seeds  the same enumeration in memory
 *   biseqt/blot.py:833-868    find_all_neighbors          cKDTree.query_ball_tree(R, p = inf) over the points
 *                                                         (d_1 c, .., d_{N-1} c, a)
 *
 * Row order is WordBlotMultipleFast.seeds()'s (blot.py:1061-1071): k-mers ascending, then itertools.product over the
 * sequences' positions -- sequence 0 varies slowest, sequence N-1 fastest, positions ascending.  No mask: the
 * reference's multiple-sequence index builds its k-mers without one (seeds.py:341-343).
 *
 * Plain pointers and sizes only; letters are one byte each (index into the alphabet).  Everything fails loudly
 * (NULL / negative return + pw_mseeds_last_error()); there is no CPU fallback.
 */
#ifndef PW_MSEEDS_H
#define PW_MSEEDS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct pw_mseed_index pw_mseed_index;

/* Plan an index for seqs[0 .. n_seqs): copies the sequences to the device `device`; nothing is computed yet.
 *   2 <= n_seqs <= 16; the sum of lens below 2^31 (a fits int32); alphabet_len L <= 36 and wordlen k with L^k < 2^62. */
pw_mseed_index* pw_mseeds_create(int device, const uint8_t* const* seqs, const int64_t* lens, int n_seqs,
                                 int alphabet_len, int wordlen);

/* Build the seeds table on the device (k-mer encoding, N sorts, N-way join, expansion) on `stream` (a hipStream_t);
 * synchronous.  The per-k-mer row count (the product of the N hit counts) and the total saturate at 2^64 - 1 instead of
 * wrapping.  Returns 0, or -1 when the table would hold more than max_rows rows (max_rows <= 0: the default, the
 * largest count whose rows stay within 16 GB; never more than 2^31 - 1, the graph indexes rows with int32). */
int pw_mseeds_build(pw_mseed_index* idx, int64_t max_rows, void* stream);

int pw_mseeds_num_seqs(const pw_mseed_index* idx);
int64_t pw_mseeds_num_rows(const pw_mseed_index* idx);

/* Rows in table order, n_seqs int32 each: (d_1, .., d_{N-1}, a).  On the device (valid until the next build / destroy)
 * or copied to the host (cap = capacity in rows). */
const int32_t* pw_mseeds_rows_device(const pw_mseed_index* idx);
int pw_mseeds_rows(const pw_mseed_index* idx, int32_t* rows, int64_t cap);

/* COUNT(*) of the rows inside each of n_boxes hyper-boxes (seeds.py:391-433), all in one launch.  Box b occupies
 * lo[b N .. b N + N), hi[...] and have[...] in row order (d_1 .. d_{N-1}, a): coordinate k is bounded by
 * lo <= x <= hi when have != 0 and unbounded otherwise.  counts: n_boxes entries. */
int pw_mseeds_count_many(const pw_mseed_index* idx, int64_t n_boxes, const int32_t* lo, const int32_t* hi,
                         const uint8_t* have, int64_t* counts);

/* Local-similarity support (blot.py:833-868, 870-1018).  pw_mseeds_graph_build links every pair of rows with
 *     |d_k c - d'_k c| <= radius for every k  and  |a - a'| <= radius
 * (d_k c one double multiply) -- cKDTree.query_ball_tree(radius, p = inf) over (d_1 c, .., d_{N-1} c, a), each row's
 * own entry removed -- and keeps the adjacency in HBM as CSR.  Returns the number of directed edges (every pair counts
 * twice), or -1.  The points of the graph are the rows, in table order. */
int64_t pw_mseeds_graph_build(pw_mseed_index* idx, double d_coeff, double radius);
int pw_mseeds_graph_counts(const pw_mseed_index* idx, int32_t* counts, int64_t cap);     /* neighbours per row */
/* offsets: num_rows + 1 entries; neighbours: pw_mseeds_graph_build's return value entries (row indices; the order inside
 * a row's list is unspecified -- it is in the reference as well). */
int pw_mseeds_graph_fetch(const pw_mseed_index* idx, int64_t* offsets, int32_t* neighbours);
/* Connected components of the graph restricted to the rows with avail[row] != 0: labels[row] = smallest row index of
 * its component, -1 for rows that are not available. */
int pw_mseeds_graph_components(const pw_mseed_index* idx, const uint8_t* avail, int32_t* labels);

double pw_mseeds_build_ms(const pw_mseed_index* idx);           /* device time of the last build (HIP events) */
double pw_mseeds_graph_ms(const pw_mseed_index* idx);           /* ... of the last graph build */
double pw_mseeds_components_ms(const pw_mseed_index* idx);      /* ... of the last components call */
double pw_mseeds_count_ms(const pw_mseed_index* idx);           /* ... of the last count_many call */
int64_t pw_mseeds_algorithmic_bytes(const pw_mseed_index* idx); /* the sequences read + 4 N bytes per row written */
void pw_mseeds_destroy(pw_mseed_index* idx);
const char* pw_mseeds_last_error(void);

#ifdef __cplusplus
}
#endif
#endif

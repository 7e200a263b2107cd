"""Dense, assumption-free statement of the query-batched seed index (include/pw_qseeds.h, kernels K10): rows, row offsets,
the neighbour relation per query, components and box counts in plain numpy.  No search, no sort, no prefix sum and no
KD-tree: the reference's k-mers go into a dict while it is walked left to right (mseeds_dense_oracle.positions, python
ints: any L ** wordlen), every query is walked left to right against that dict, every ordered pair of rows of one query is
evaluated, and components come from a union-find.  Quadratic in the rows of a query and meant for a few thousand of them;
tests/test_qseeds_dense_oracle.py anchors it to seeds_oracle.seeds_by_mutant and blot_oracle.find_all_neighbors.
"""
import numpy as np

from . import mseeds_dense_oracle as DO


def rows(ref, queries, wordlen, L):
    """((rows, 3) int64 of (q, d, a) = (q, i - j, i + j), row offsets int64 of len(queries) + 1 entries): per query j
    ascends, and for each j the positions i of that k-mer in the reference ascend."""
    hits = DO.positions(ref, wordlen, L)
    out, off = [], [0]
    for q, t in enumerate(queries):
        s = [int(c) for c in t]
        for j in range(len(s) - wordlen + 1):
            v = 0
            for c in s[j:j + wordlen]:
                v = v * L + c
            for i in hits.get(v, ()):
                out.append((q, i - j, i + j))
        off.append(len(out))
    return np.array(out, np.int64).reshape(-1, 3), np.array(off, np.int64)


def neighbours(rows, off, c, R, block=256):
    """Per row the ascending list of the rows OF ITS QUERY with |fl(d c) - fl(d' c)| <= R and |a - a'| <= R, itself
    removed; indices are rows of the whole table."""
    rows = np.asarray(rows, np.int64).reshape(-1, 3)
    out = []
    for q in range(len(off) - 1):
        b = int(off[q])
        out.extend([b + v for v in ns] for ns in DO.neighbours_cr(rows[b:int(off[q + 1]), 1:], c, R, block))
    return out


def components(neighs, avail):
    """labels[i] = smallest row of i's component among the available rows, -1 for an unavailable row."""
    return DO.components(neighs, avail)


def box_counts(rows, off, q, dmin, dmax, amin, amax):
    """Rows of query q[b] with dmin[b] <= d <= dmax[b] and amin[b] <= a <= amax[b] (inclusive); 0 for an inverted box and
    for a query without rows."""
    rows = np.asarray(rows, np.int64).reshape(-1, 3)
    out = np.zeros(len(q), np.int64)
    for b, (k, d0, d1, a0, a1) in enumerate(zip(*[np.asarray(v, np.int64).tolist() for v in (q, dmin, dmax, amin, amax)])):
        r = rows[int(off[k]):int(off[k + 1])]
        out[b] = int(((r[:, 1] >= d0) & (r[:, 1] <= d1) & (r[:, 2] >= a0) & (r[:, 2] <= a1)).sum())
    return out

"""CPU yardstick for the N-way seed index (include/pw_mseeds.h): a short numpy + cKDTree restatement of what the
reference computes in ``WordBlotMultipleFast.seeds`` (blot.py:1061-1071), ``find_all_neighbors`` (:833-868) and the
depth-first growth of ``similar_segments`` (:961-975).  Used by the tests on inputs larger than the goldens; it is not
part of the product."""
from itertools import product

import numpy as np
from scipy.spatial import cKDTree


def kmers(seq, wordlen, L):
    """The k-mer of every position as an integer in base L (kmers.py:164-241, no mask)."""
    a = np.asarray(seq, np.int64)
    n = len(a) - wordlen + 1
    if n <= 0:
        return np.zeros(0, np.int64)
    v = np.zeros(n, np.int64)
    for t in range(wordlen):
        v = v * L + a[t:t + n]
    return v


def seed_rows(seqs, wordlen, L):
    """(rows, N) int64: k-mers ascending, then itertools.product of the positions, sequence 0 slowest."""
    N = len(seqs)
    hits = []
    for s in seqs:
        ks = kmers(s, wordlen, L)
        order = np.argsort(ks, kind='stable')
        uniq, start = np.unique(ks[order], return_index=True)
        ends = np.r_[start[1:], len(order)]
        hits.append({int(k): order[b:e].tolist() for k, b, e in zip(uniq, start, ends)})
    out = []
    for k in sorted(hits[0]):
        if not all(k in h for h in hits):
            continue
        for idxs in product(*[h[k] for h in hits]):
            out.append([idxs[0] - idxs[j] for j in range(1, N)] + [sum(idxs)])
    return np.array(out, np.int64).reshape(-1, N)


def neighbours(rows, d_radius, a_radius):
    """Per row the sorted indices of the other rows in its L-inf neighbourhood, over the points
    (d_1 c, .., d_{N-1} c, a), c = a_radius / d_radius, radius a_radius."""
    if not len(rows):
        return []
    c = 1. * a_radius / d_radius
    pts = np.array([[float(d) * c for d in r[:-1]] + [float(r[-1])] for r in rows.tolist()])
    tree = cKDTree(pts)
    res = tree.query_ball_tree(tree, a_radius, p=float('inf'))
    return [sorted(x for x in lst if x != i) for i, lst in enumerate(res)]


def components(neighs, avail):
    """labels[i] = smallest index of i's component in the sub-graph of available rows, -1 for the others."""
    n = len(neighs)
    labels = [-1] * n
    for i in range(n):
        if not avail[i] or labels[i] >= 0:
            continue
        labels[i] = i
        stack = [i]
        while stack:
            u = stack.pop()
            for v in neighs[u]:
                if avail[v] and labels[v] < 0:
                    labels[v] = i
                    stack.append(v)
    return labels


def box_count(rows, ds_band, a_band):
    """seed_count(ds_band, a_band): inclusive bounds, None = unbounded (seeds.py:391-433)."""
    ok = np.ones(len(rows), bool)
    for k, b in enumerate(ds_band or []):
        if b is not None:
            ok &= (rows[:, k] >= b[0]) & (rows[:, k] <= b[1])
    if a_band is not None:
        ok &= (rows[:, -1] >= a_band[0]) & (rows[:, -1] <= a_band[1])
    return int(ok.sum())

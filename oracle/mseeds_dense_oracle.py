"""Dense, assumption-free statement of the N-way seed index (include/pw_mseeds.h, kernels K9): rows, the neighbour
relation, components and hyper-box counts in plain numpy.  No tree, no sort of the k-mers' positions, no search and no
prefix sum: the positions of every k-mer are collected into a dict while the sequence is walked left to right, every
ordered pair of rows is evaluated, and components come from a union-find.  It is quadratic in the rows and meant for a
few thousand of them; tests/mseeds_ref.py (a cKDTree, the reference's own structure) is the yardstick it is anchored to.
"""
from itertools import product

import numpy as np


def positions(seq, wordlen, L):
    """{k-mer value: ascending list of its positions}, by one left-to-right walk (python ints: any L ** wordlen)."""
    out = {}
    s = [int(c) for c in seq]
    for i in range(len(s) - wordlen + 1):
        v = 0
        for c in s[i:i + wordlen]:
            v = v * L + c
        out.setdefault(v, []).append(i)
    return out


def run_lengths(seqs, wordlen, L):
    """[(k-mer, (run length in sequence 0, .., N - 1), first row)] for the k-mers present in every sequence, ascending:
    the radices of the index's mixed-radix row decode and where each k-mer's rows start."""
    hits = [positions(s, wordlen, L) for s in seqs]
    out, at = [], 0
    for k in sorted(hits[0]):
        if all(k in h for h in hits):
            rl = tuple(len(h[k]) for h in hits)
            out.append((k, rl, at))
            at += int(np.prod([int(x) for x in rl], dtype=object))
    return out


def seed_rows(seqs, wordlen, L):
    """(rows, N) int64 of (i_1 - i_2, .., i_1 - i_N, sum i): k-mers ascending, then itertools.product of the ascending
    position lists (sequence 0 slowest)."""
    N = len(seqs)
    hits = [positions(s, wordlen, L) for s in seqs]
    out = []
    for k in sorted(hits[0]):
        if not all(k in h for h in hits):
            continue
        idx = np.array(list(product(*[h[k] for h in hits])), np.int64).reshape(-1, N)
        out.append(np.concatenate([idx[:, :1] - idx[:, 1:], idx.sum(1, keepdims=True)], axis=1))
    return np.concatenate(out).reshape(-1, N) if out else np.zeros((0, N), np.int64)


def connected(rows, c, R, block=256):
    """Yields (first row of the block, boolean matrix block x rows): the pair (i, j) is connected when
    |d_k c - d'_k c| <= R in float64 for every k and |a - a'| <= R; self pairs removed."""
    rows = np.asarray(rows, np.int64)
    n = len(rows)
    x = rows[:, :-1].astype(np.float64) * np.float64(c)       # fl(d_k c), one rounding each
    a = rows[:, -1]
    R = np.float64(R)
    for b in range(0, n, block):
        e = min(n, b + block)
        ok = np.abs(a[b:e, None] - a[None, :]) <= R
        for k in range(x.shape[1]):
            ok &= np.abs(x[b:e, None, k] - x[None, :, k]) <= R
        ok[np.arange(e - b), np.arange(b, e)] = False
        yield b, ok


def neighbours_cr(rows, c, R, block=256):
    """Per row the ascending list of the rows connected to it, for the scale c and radius R that graph_build takes."""
    out = []
    for _, ok in connected(rows, c, R, block):
        out.extend(np.flatnonzero(r).tolist() for r in ok)
    return out


def neighbours(rows, d_radius, a_radius, block=256):
    """As find_all_neighbors(d_radius, a_radius): c = a_radius / d_radius, R = a_radius."""
    return neighbours_cr(rows, 1. * a_radius / d_radius, a_radius, block)


def components(neighs, avail):
    """labels[i] = smallest row of i's component in the sub-graph of available rows, -1 for an unavailable row."""
    n = len(neighs)
    parent = list(range(n))

    def find(v):
        while parent[v] != v:
            parent[v] = parent[parent[v]]
            v = parent[v]
        return v

    for u in range(n):
        if not avail[u]:
            continue
        for v in neighs[u]:
            if avail[v]:
                ru, rv = find(u), find(v)
                if ru != rv:
                    parent[max(ru, rv)] = min(ru, rv)       # the root is always the smallest row of its tree
    return [find(u) if avail[u] else -1 for u in range(n)]


def box_counts(rows, lo, hi, have):
    """Rows inside each box: lo[b, k] <= row[k] <= hi[b, k] wherever have[b, k]; (boxes, N) arrays, as count_many."""
    rows = np.asarray(rows, np.int64)
    lo, hi = np.asarray(lo, np.int64).reshape(-1, rows.shape[1]), np.asarray(hi, np.int64).reshape(-1, rows.shape[1])
    have = np.asarray(have).reshape(lo.shape).astype(bool)
    out = np.zeros(len(lo), np.int64)
    if len(rows) < len(lo):                     # fewer rows than boxes: walk the rows, all boxes at once
        for r in rows:
            out += (~have | ((lo <= r) & (r <= hi))).all(1)
        return out
    for b in range(len(lo)):
        ok = np.ones(len(rows), bool)
        for k in np.flatnonzero(have[b]):
            ok &= (rows[:, k] >= lo[b, k]) & (rows[:, k] <= hi[b, k])
        out[b] = ok.sum()
    return out


def box_count(rows, ds_band, a_band):
    """seed_count(ds_band, a_band): inclusive bounds; a None band, or a None entry of ds_band, is unbounded."""
    N = np.asarray(rows).shape[1]
    lo, hi, have = [0] * N, [0] * N, [0] * N
    for k, b in enumerate(ds_band or []):
        if b is not None:
            lo[k], hi[k], have[k] = b[0], b[1], 1
    if a_band is not None:
        lo[-1], hi[-1], have[-1] = a_band[0], a_band[1], 1
    return int(box_counts(rows, [lo], [hi], [have])[0])


def diameter_from(neighs, start):
    """Eccentricity of `start` by breadth-first search: a lower bound of the graph's diameter."""
    dist = {start: 0}
    front = [start]
    while front:
        nxt = []
        for u in front:
            for v in neighs[u]:
                if v not in dist:
                    dist[v] = dist[u] + 1
                    nxt.append(v)
        front = nxt
    return max(dist.values()), len(dist)

"""Plain numpy restatement of the DOCUMENTED overlap band record (TEST INFRASTRUCTURE, never the product path).

What is restated: the field comments of `pw_overlap_band` in include/pw_overlap.h, with `L(d)`, `r(d)` and the
neighbour predicate of oracle/blot_oracle.py (blot.py:78-139, 521-548).  It is not a port of the kernels:

  * seeds are enumerated outright, in the reference's table order (k-mer ascending, then i, then j), by numpy sorts;
    the first row gives `d_first`;
  * the neighbours of a seed on an occupied diagonal d are counted DENSELY: n(d) + 1 is the number of seeds on the
    occupied diagonals d' with abs(d' / r(d') - d / r(d)) <= 1.0 in float64 -- the KD-tree's own Chebyshev predicate
    evaluated for every pair of occupied diagonals, in row blocks.  No binary search, no prefix sums, and no
    assumption that d / r(d) is monotone;
  * w(d) = ((n(d) + 1) - (2 r(d) L(d)) p0) / L(d) in float64 with p0 = (1. / alphabet_len) ** wordlen.

Parity pin: tests/test_overlap_record_oracle.py anchors every per-diagonal n, r, L (through every seed's p) and the
chosen band to blot_oracle.score_seeds / highest_scoring_overlap_band, i.e. to the KD-tree restatement of the reference.
The KD-tree oracle keeps one neighbour LIST per seed (about 10^9 entries for 3 * 10^5 seeds); this one keeps one row
block of the diagonal-by-diagonal predicate and scores such a pair in about a second.
"""
import numpy as np
from scipy.special import erfcinv

FIELDS = ('n_seeds', 'w_best', 'd_best', 'n_best', 'r_best', 'len_best', 'band_best', 'tie',
          'd_first', 'n_first', 'r_first', 'len_first', 'band_first')
_ROW_BLOCK = 512


def kmer_keys(x, wordlen, alphabet_len):
    """The k-mer at every position of x as an integer, letters as digits in base alphabet_len (kmers.py:164-210)."""
    x = np.asarray(x, np.int64)
    n = len(x) - wordlen + 1
    if n <= 0:
        return np.zeros(0, np.int64)
    assert alphabet_len ** wordlen <= 2 ** 62 and (len(x) == 0 or (0 <= x.min() and x.max() < alphabet_len))
    keys = np.zeros(n, np.int64)
    for t in range(wordlen):
        keys = keys * alphabet_len + x[t:t + n]
    return keys


def seed_positions(S, T, wordlen, alphabet_len):
    """(i, j) of every seed of S against T as two different sequences, in table order: k-mer ascending, then i, then j."""
    kS, kT = kmer_keys(S, wordlen, alphabet_len), kmer_keys(T, wordlen, alphabet_len)
    if len(kS) == 0 or len(kT) == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    oT = np.argsort(kT, kind='stable')                     # positions of T by (k-mer, j)
    oS = np.argsort(kS, kind='stable')                     # positions of S by (k-mer, i)
    sT = kT[oT]
    lo = np.searchsorted(sT, kS[oS], 'left')               # the run of equal k-mers on the T side, per S position
    cnt = np.searchsorted(sT, kS[oS], 'right') - lo
    i = np.repeat(oS, cnt)
    start = np.repeat(np.cumsum(cnt) - cnt, cnt)
    j = oT[np.repeat(lo, cnt) + (np.arange(len(i)) - start)]
    return i.astype(np.int64), j.astype(np.int64)


def seed_diagonals(S, T, wordlen, alphabet_len):
    i, j = seed_positions(S, T, wordlen, alphabet_len)
    return i - j


def coefficients(alphabet_len, wordlen, g_max, sensitivity):
    """(len_coeff, radius_coeff, p0) exactly as overlap.raw_bands computes them (blot.py:109, 134-136, 538)."""
    assert 0 < g_max < 1 and 0 < sensitivity < 1
    len_coeff = 2. / (2 - g_max)
    radius_coeff = erfcinv(1. - sensitivity) * np.sqrt(2 * g_max)
    p0 = (1. / alphabet_len) ** wordlen
    return len_coeff, radius_coeff, p0


def overlap_lengths(d, len_s, len_t, len_coeff):
    """L(d) = ceil(len_coeff * (min(|S| - d, |T|) + min(d, 0)))   (blot.py:78-112)"""
    d = np.asarray(d, np.int64)
    wall = np.minimum(len_s - d, len_t) + np.minimum(d, 0)
    return np.ceil(len_coeff * wall).astype(np.int64)


def band_radii(L, radius_coeff):
    """r = max(1, ceil(radius_coeff * sqrt(L)))   (blot.py:116-139)"""
    return np.maximum(1, np.ceil(radius_coeff * np.sqrt(np.asarray(L, np.int64))).astype(np.int64))


def band_record(S, T, wordlen, alphabet_len, g_max, sensitivity):
    """The documented record of the pair (S, T): every field of `pw_overlap_band` but the padding, `nocc` (occupied
    diagonals) and the per-diagonal arrays `d` (ascending), `n`, `L`, `r`, `w`.  Without seeds only `n_seeds`, `nocc`
    and empty arrays mean anything (the record's other fields are then undefined; they are reported as 0)."""
    len_coeff, radius_coeff, p0 = coefficients(alphabet_len, wordlen, g_max, sensitivity)
    ds = seed_diagonals(S, T, wordlen, alphabet_len)
    out = dict.fromkeys(FIELDS, 0)
    out['w_best'] = 0.
    out['n_seeds'] = int(len(ds))
    d, cnt = np.unique(ds, return_counts=True)             # the per-diagonal histogram: occupied diagonals, ascending
    cnt = cnt.astype(np.int64)
    out['nocc'] = int(len(d))
    if len(ds) == 0:
        empty = np.zeros(0, np.int64)
        out.update(d=empty, n=empty, L=empty, r=empty, w=np.zeros(0))
        return out
    L = overlap_lengths(d, len(S), len(T), len_coeff)
    r = band_radii(L, radius_coeff)
    x = d / r                                              # float64 true division, as the reference's d / _rad(d)
    n = np.empty(len(d), np.int64)
    for b in range(0, len(d), _ROW_BLOCK):
        near = np.abs(x[None, :] - x[b:b + _ROW_BLOCK, None]) <= 1.0
        n[b:b + _ROW_BLOCK] = (near * cnt[None, :]).sum(axis=1) - 1
    w = ((n + 1) - (2 * r * L) * p0) / L
    best = int(np.lexsort((d, -w))[0])                     # largest w, then smallest d
    w_best = float(w[best])
    if w_best > 0:
        wcap = min(w_best, 1.)
        tie = int((w >= wcap - abs(wcap) * 1e-9).sum())
    else:
        tie = len(d)
    first = int(np.flatnonzero(d == ds[0])[0])

    def band(q):
        return int(((ds >= d[q] - r[q]) & (ds <= d[q] + r[q])).sum())

    out.update(w_best=w_best, d_best=int(d[best]), n_best=int(n[best]), r_best=int(r[best]), len_best=int(L[best]),
               band_best=band(best), tie=tie, d_first=int(d[first]), n_first=int(n[first]), r_first=int(r[first]),
               len_first=int(L[first]), band_first=band(first), d=d, n=n, L=L, r=r, w=w)
    return out

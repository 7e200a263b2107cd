"""Band selection for overlap alignments (host side; mirrors ``biseqt/blot.py``).

What is here: the closed-form geometry and statistics of Word-Blot (``wall_to_wall_distance`` :78-89,
``expected_overlap_len`` :92-112, ``band_radius`` / ``band_radii`` :116-160, ``H0_moments`` / ``H1_moments``
:163-218, ``find_peaks`` :37-76) -- scalar arithmetic, evaluated on the host exactly as the reference writes it --
``WordBlot`` (:228-490: ``score_seeds``, ``similar_segments``) and ``WordBlotOverlap`` (:490-579), whose heavy
parts -- for every seed the seeds in its neighbourhood (KD-tree ball queries in the reference) and the growth of
neighbouring seeds into segments (a depth-first search there) -- run on the GPU (kernels K6, K7 of pw_seeds.hip).
``highest_scoring_overlap_band()`` returns the ``d_band`` that the banded overlap aligner
(``Aligner(..., alnmode=BANDED_MODE, alntype=B_OVERLAP, diag_range=d_band)``) is given.
``WordBlotMultiple`` / ``WordBlotMultipleFast`` (:726-1083) do the same local-similarity search for more than two
sequences on the N-way seed table of pw_mseeds.hip (kernels K9).  ``WordBlotLocalRef.similar_segments_many`` answers many
queries against one reference out of one set of launches (kernels K10 of pw_qseeds.hip).
"""
import numpy as np
from scipy.special import erfcinv

from .batch import pack_reads
from .seeds import SeedIndex, SeedIndexMultiple, _QIndex
from .sequence import Sequence


def find_peaks(xs, rs, threshold):
    """Maximal disjoint bands ``(i - 1, i + 1)`` around positions with ``xs[i] >= threshold``; bands closer than
    the radius are merged (``blot.py:37-76``)."""
    peaks, cur_peak = [], None
    for idx, x in enumerate(xs):
        radius = rs[idx] if isinstance(rs, (list, tuple, np.ndarray)) else rs
        if x < threshold:
            continue
        peak_l, peak_r = max(0, idx - 1), min(len(xs) - 1, idx + 1)
        if cur_peak is None:
            cur_peak = (peak_l, peak_r)
            continue
        if peak_l < cur_peak[1] + radius:
            assert peak_r >= cur_peak[1]
            cur_peak = (cur_peak[0], peak_r)
        else:
            peaks.append(cur_peak)
            cur_peak = (peak_l, peak_r)
    if cur_peak is not None:
        peaks.append(cur_peak)
    return [(int(l), int(r)) for (l, r) in peaks]


def wall_to_wall_distance(len0, len1, diag):
    return min(len0 - diag, len1) + min(diag, 0)


def expected_overlap_len(len0, len1, diag, gap_prob):
    L = wall_to_wall_distance(len0, len1, diag)
    expected_len = (2. / (2 - gap_prob)) * L
    assert expected_len >= 0
    return int(np.ceil(expected_len))


def band_radius(expected_len, gap_prob, sensitivity):
    assert 0 < gap_prob < 1 and 0 < sensitivity < 1
    epsilon = 1. - sensitivity
    C = erfcinv(epsilon) * np.sqrt(2 * gap_prob)
    radius = C * np.sqrt(expected_len)
    return max(1, int(np.ceil(radius)))


def band_radii(expected_lens, gap_prob, sensitivity):
    assert 0 < gap_prob < 1 and 0 < sensitivity < 1
    epsilon = 1. - sensitivity
    C = erfcinv(epsilon) * np.sqrt(2 * gap_prob)
    K = np.asarray(list(expected_lens), dtype=np.float64)
    return np.maximum(1, np.ceil(C * np.sqrt(K)).astype(np.int64))


def H0_moments(alphabet_len, wordlen, area):
    p_H0 = 1. / alphabet_len
    pw_H0 = p_H0 ** wordlen
    mu_H0 = area * pw_H0
    sd_H0 = np.sqrt(area * ((1 - pw_H0) * (pw_H0 + 2 * p_H0 * pw_H0 / (1 - p_H0)) - 2 * wordlen * pw_H0 ** 2))
    return mu_H0, sd_H0


def H1_moments(alphabet_len, wordlen, area, seglen, p_match):
    mu_H0, sd_H0 = H0_moments(alphabet_len, wordlen, area)
    p_H1 = p_match
    if p_H1 == 1.:
        p_H1 = 1 - np.finfo(float).eps
    pw_H1 = p_H1 ** wordlen
    mu_H1 = mu_H0 + seglen * pw_H1
    sd_H1 = np.sqrt(sd_H0 ** 2 + seglen * ((1 - pw_H1) * (pw_H1 + 2 * p_H1 * pw_H1 / (1 - p_H1)) - 2 * wordlen * pw_H1 ** 2))
    return mu_H1, sd_H1


def score_num_seeds(alphabet_len, wordlen, num_seeds, area, seglen, p_match):
    """z-scores of an observed number of seeds in a region against H0 and H1 (``blot.py:238-271``)."""
    if area == 0:
        return float('-inf'), float('-inf')
    mu_H0, sd_H0 = H0_moments(alphabet_len, wordlen, area)
    mu_H1, sd_H1 = H1_moments(alphabet_len, wordlen, area, seglen, p_match)
    return (num_seeds - mu_H0) / sd_H0, (num_seeds - mu_H1) / sd_H1


def seed_ps_from_counts(n, d_radius, a_radius, alphabet_len, wordlen):
    """Per seed the estimated match probability of the segment centred there (``blot.py:376-408``), from its number of
    neighbours ``n`` (itself excluded).  Every seed's segment has the same dimensions: K' = a_radius,
    A = 2 d_radius a_radius (``segment_dims`` of the bands ``(-d_radius, d_radius)``, ``(-a_radius, a_radius)``)."""
    n = np.asarray(n).astype(np.int64)
    Kp = (a_radius - -a_radius) // 2
    area = (d_radius - -d_radius) * Kp
    word_p_null = (1. / alphabet_len) ** wordlen
    word_p = (n + 1 - area * word_p_null) / Kp
    p = np.zeros(len(n))
    pos = word_p > 0
    p[pos] = np.exp(np.log(word_p[pos]) / wordlen)
    return np.minimum(p, 1)


def available_seeds_many(p, p_min, row_offsets, at_least_one=False):
    """Which seeds of a query-batched table (rows of query q: ``row_offsets[q]:row_offsets[q + 1]``, in the order the
    in-memory classes list their seeds) the segments grow from: those with ``p >= p_min``; with ``at_least_one``, a query
    none of whose seeds passes contributes its first seed of highest p (``blot.py:432-436``) -- and a query without seeds
    is refused as the per-query call refuses it."""
    p, row_offsets = np.asarray(p, np.float64), np.asarray(row_offsets, np.int64)
    per_q = np.diff(row_offsets)
    assert len(p) == row_offsets[-1]
    if at_least_one:
        assert (per_q > 0).all(), 'no seeds found while at_least_one=True'
    avail = p >= p_min
    if at_least_one and len(p):
        nq = len(per_q)
        qid = np.repeat(np.arange(nq), per_q)
        has = np.zeros(nq, bool)
        has[qid[avail]] = True
        p_max = np.maximum.reduceat(p, row_offsets[:-1])           # (every query has rows here)
        cand = np.flatnonzero((p == p_max[qid]) & ~has[qid])
        _, first = np.unique(qid[cand], return_index=True)          # np.argmax over the query's list: its first maximum
        avail[cand[first]] = True
    return avail


def segments_from_arrays(counts, labels, rows, row_offsets, query_lens, ref_len, d_radius, a_radius, alphabet_len, wordlen,
                         count_boxes):
    """The host half of :meth:`WordBlotLocalRef.similar_segments_many` as a pure function of arrays: from the neighbour
    counts of every seed, the component label of every seed (the smallest row index of its component, -1 for seeds that
    take no part), the rows ``(q, d, a)`` in (q, j, i) order and their per-query offsets to one list of segment dicts per
    query -- what ``WordBlot.similar_segments`` yields for that query, in its order (``blot.py:410-490``).

    A component's bounding segment is clamped with ITS query's length, its averaged p sums in presentation order with the
    starting seed counted twice (:449,455), and segments come in the order of their first seeds.  ``count_boxes(q, d_min,
    d_max, a_min, a_max)`` returns the seed count of every segment's box (arrays in, array out): one call for all."""
    rows = np.asarray(rows).reshape(-1, 3)
    labels = np.asarray(labels)
    row_offsets, query_lens = np.asarray(row_offsets, np.int64), np.asarray(query_lens, np.int64)
    nq = len(query_lens)
    assert len(row_offsets) == nq + 1 and len(rows) == len(labels) == len(counts) == row_offsets[-1]
    out = [[] for _ in range(nq)]
    idx = np.flatnonzero(labels >= 0)
    if not len(idx):
        return out
    p = seed_ps_from_counts(counts, d_radius, a_radius, alphabet_len, wordlen)
    order = idx[np.lexsort((idx, labels[idx]))]              # grouped by component, seed order inside; a label is its
    lab = labels[order]                                       # component's first row, so the groups ascend by (q, first seed)
    starts = np.flatnonzero(np.r_[True, lab[1:] != lab[:-1]])
    d, a = rows[order, 1].astype(np.int64), rows[order, 2].astype(np.int64)
    firsts = order[starts]                                    # the seed each search starts from
    q = rows[firsts, 0].astype(np.int64)
    lenS, lenT = ref_len, query_lens[q]
    d_min = np.minimum(lenS, np.maximum(np.minimum.reduceat(d, starts) - d_radius, -lenT))
    d_max = np.minimum(lenS, np.maximum(np.maximum.reduceat(d, starts) + d_radius, -lenT))
    a_min = np.maximum(np.minimum.reduceat(a, starts) - a_radius, 0)
    a_max = np.minimum(np.maximum.reduceat(a, starts) + a_radius, lenS + lenT)
    cnt = np.diff(np.r_[starts, len(order)])
    p_hat = (np.add.reduceat(p[order], starts) + p[firsts]) / (cnt + 1)      # ... and it is counted twice (:449,455)
    n = np.asarray(count_boxes(q, d_min, d_max, a_min, a_max))
    assert len(n) == len(starts)
    for s, (qs, d0, d1, a0, a1, ns) in enumerate(zip(q.tolist(), d_min.tolist(), d_max.tolist(), a_min.tolist(),
                                                     a_max.tolist(), n.tolist())):
        K_hat = (a1 - a0) // 2                                # segment_dims (blot.py:283-303)
        area_hat = (d1 - d0) * K_hat
        out[qs].append({'segment': ((d0, d1), (a0, a1)), 'p': p_hat[s],
                        'scores': score_num_seeds(alphabet_len, wordlen, ns, area_hat, K_hat, p_hat[s])})
    return out


class WordBlot(SeedIndex):
    """A similarity finder based on m-dependent CLT statistics (``blot.py:228-490``).

    Keyword Args:
        g_max (float): upper bound for indel probabilities.  sensitivity (float): desired band sensitivity.
        wordlen, alphabet, mask, device: as :class:`biseqt_amd.seeds.SeedIndex`.
    """

    def __init__(self, S, T, g_max=None, sensitivity=None, **kw):
        assert 0 < g_max < 1 and 0 < sensitivity < 1
        self.g_max = g_max
        self.sensitivity = sensitivity
        super(WordBlot, self).__init__(S, T, **kw)
        self._graph_key = None

    def _presentation(self):
        """Order in which the class iterates its seeds, as indices into the table rows (None = table order).  The
        in-memory *Ref variants scan T left to right instead (``blot.py:607-620``)."""
        return None

    def score_num_seeds(self, **kw):
        """z-scores of an observed number of seeds in a region against H0 and H1 (``blot.py:238-271``)."""
        return score_num_seeds(len(self.alphabet), self.wordlen, kw['num_seeds'], kw['area'], kw['seglen'], kw['p_match'])

    def band_radius(self, K):
        return band_radius(K, self.g_max, self.sensitivity)

    def segment_dims(self, d_band=None, a_band=None):
        """Edit path length and area of a diagonal / antidiagonal segment (``blot.py:283-303``; the reference
        divides with python 2's integer ``/``)."""
        a_min, a_max = a_band
        d_min, d_max = d_band
        K = (a_max - a_min) // 2
        A = (d_max - d_min) * K
        return K, A

    def estimate_match_probability(self, num_seeds, d_band=None, a_band=None):
        """``p = ((n - A p0^w) / K)^(1/w)``, 0 where the logarithm is undefined (``blot.py:305-341``)."""
        K, area = self.segment_dims(d_band=d_band, a_band=a_band)
        word_p_null = (1. / len(self.alphabet)) ** self.wordlen
        word_p = (num_seeds - area * word_p_null) / K
        if not word_p > 0:
            match_p = 0
        else:
            match_p = np.exp(np.log(word_p) / self.wordlen)
        return min(match_p, 1)

    def _graph(self, d_radius, a_radius):
        """The neighbourhood graph of ``find_all_neighbors`` (``blot.py:343-374``), built on the GPU once per
        (d_radius, a_radius)."""
        key = (d_radius, a_radius)
        if self._graph_key != key:
            self._idx.graph_build(1. * a_radius / d_radius, a_radius)
            self._graph_key = key

    def _seed_ps(self, K):
        d_radius = int(np.ceil(self.band_radius(K)))
        a_radius = K
        self._graph(d_radius, a_radius)
        p = seed_ps_from_counts(self._idx.graph_counts(), d_radius, a_radius, len(self.alphabet), self.wordlen)
        return p, d_radius, a_radius

    def score_seeds(self, K):
        """One dict per seed, in the class's seed order: ``seed`` (d, a), ``neighs`` (indices of the seeds in its
        neighbourhood), ``p`` estimated match probability of a segment centred there (``blot.py:376-408``)."""
        if not self.seed_count():
            return []
        p, _, _ = self._seed_ps(K)
        rows = self._idx.graph_points()
        if not len(rows):
            return []
        off, adj = self._idx.graph_fetch()
        perm = self._presentation()
        if perm is None:
            return [{'seed': (int(rows[k, 0]), int(rows[k, 1])), 'neighs': adj[off[k]:off[k + 1]].tolist(), 'p': p[k]}
                    for k in range(len(rows))]
        inv = np.empty(len(perm), np.int64)
        inv[perm] = np.arange(len(perm))
        return [{'seed': (int(rows[k, 0]), int(rows[k, 1])), 'neighs': inv[adj[off[k]:off[k + 1]]].tolist(), 'p': p[k]}
                for k in perm.tolist()]

    def similar_segments(self, K_min, p_min, at_least_one=False):
        """All maximal local similarities of a minimum length and match probability (``blot.py:410-490``): seeds
        with ``p >= p_min`` are grown into connected groups (the reference's depth-first search finds the
        connected components of the neighbourhood graph; they are computed on the GPU), each group's bounding
        segment is clamped to the table, scored and yielded in the order of its first seed."""
        if not self.seed_count():
            assert not at_least_one, 'no seeds found while at_least_one=True'
            return
        p, d_radius, a_radius = self._seed_ps(K_min)
        rows = self._idx.graph_points()              # the seeds as the class iterates them (mirrored for S == T)
        if not len(rows):
            assert not at_least_one, 'no seeds found while at_least_one=True'
            return
        perm = self._presentation()
        if perm is None:
            rank = np.arange(len(rows))                  # position of every table row in the class's seed order
        else:
            rank = np.empty(len(perm), np.int64)
            rank[perm] = np.arange(len(perm))
        avail = p >= p_min
        if not avail.any() and at_least_one:
            cand = np.flatnonzero(p == p.max())
            avail[cand[np.argmin(rank[cand])]] = True    # np.argmax over the class's list: its first maximum
        if not avail.any():
            return
        labels = self._idx.graph_components(avail)
        idx = np.flatnonzero(labels >= 0)
        order = idx[np.lexsort((rank[idx], labels[idx]))]       # grouped by component, seed order inside
        lab = labels[order]
        starts = np.flatnonzero(np.r_[True, lab[1:] != lab[:-1]])
        d, a = rows[order, 0].astype(np.int64), rows[order, 1].astype(np.int64)
        lenS, lenT = len(self.S), len(self.T)
        d_lo = np.minimum.reduceat(d, starts) - d_radius
        d_hi = np.maximum.reduceat(d, starts) + d_radius
        a_lo = np.minimum.reduceat(a, starts) - a_radius
        a_hi = np.maximum.reduceat(a, starts) + a_radius
        psum = np.add.reduceat(p[order], starts)
        cnt = np.diff(np.r_[starts, len(order)])
        firsts = order[starts]                                   # the seed each search starts from
        for s in np.argsort(rank[firsts], kind='stable').tolist():
            first = int(firsts[s])                       # ... and it is counted twice (:449,455)
            d_min = min(lenS, max(int(d_lo[s]), -lenT))
            d_max = min(lenS, max(int(d_hi[s]), -lenT))
            a_min = max(int(a_lo[s]), 0)
            a_max = min(int(a_hi[s]), lenS + lenT)
            seg = (d_min, d_max), (a_min, a_max)
            p_hat = (psum[s] + p[first]) / (cnt[s] + 1)
            res = {'segment': seg, 'p': p_hat}
            n = self.seed_count(d_band=seg[0], a_band=seg[1])
            K_hat, area_hat = self.segment_dims(d_band=seg[0], a_band=seg[1])
            res['scores'] = self.score_num_seeds(num_seeds=n, area=area_hat, seglen=K_hat, p_match=p_hat)
            yield res


class WordBlotOverlap(WordBlot):
    """Overlap (suffix-prefix) similarity detection between two sequences (``blot.py:228-236, 490-579``).

    Keyword Args:
        g_max (float): upper bound for indel probabilities.  sensitivity (float): desired band sensitivity.
        wordlen, alphabet, mask, device: as :class:`biseqt_amd.seeds.SeedIndex`.
    """

    def __init__(self, S, T, g_max=None, sensitivity=None, **kw):
        super(WordBlotOverlap, self).__init__(S, T, g_max=g_max, sensitivity=sensitivity, **kw)
        assert not self.self_comp, 'overlap detection compares two different sequences'

    def _tables(self):
        """L(d) and r(d) for every diagonal d = -|T| .. |S| (index d + |T|), the reference's `_len` / `_rad`."""
        lenS, lenT = len(self.S), len(self.T)
        d = np.arange(-lenT, lenS + 1, dtype=np.int64)
        wall = np.minimum(lenS - d, lenT) + np.minimum(d, 0)
        L = np.ceil((2. / (2 - self.g_max)) * wall).astype(np.int64)
        rad = band_radii(L, self.g_max, self.sensitivity)
        return L, rad

    def score_seeds(self):
        """One dict per seed, in table order: ``seed`` (d, a), ``r`` band radius at its diagonal, ``L`` expected
        overlap length, ``p`` estimated match probability (``blot.py:497-556``)."""
        rows = self.rows()
        if not len(rows):
            return []
        L_tab, r_tab = self._tables()
        n = self._idx.band_neighbours(r_tab.astype(np.float64)).astype(np.int64)
        lenT = len(self.T)
        d = rows[:, 0].astype(np.int64)
        L = L_tab[d + lenT]
        rad = r_tab[d + lenT]
        area = 2 * rad * L
        word_p_null = (1. / len(self.alphabet)) ** self.wordlen
        word_p = (n + 1 - area * word_p_null) / L
        pos = word_p > 0                      # log(x <= 0) warns, which the reference answers with p = 0 (:541-545)
        p = np.zeros(len(rows))
        p[pos] = np.exp(np.log(word_p[pos]) / self.wordlen)
        p = np.minimum(p, 1)
        perm = self._presentation()
        ks = range(len(rows)) if perm is None else perm.tolist()
        return [{'seed': (int(rows[k, 0]), int(rows[k, 1])), 'r': np.float64(rad[k]), 'L': int(L[k]), 'p': p[k]}
                for k in ks]

    def highest_scoring_overlap_band(self):
        """The diagonal band with the highest estimated match probability: ``d_band``, ``p``, ``len``, ``score``
        (z-score under H1), or None without seeds (``blot.py:558-579``)."""
        scored = self.score_seeds()
        if not scored:
            return None
        idx = max(range(len(scored)), key=lambda i: scored[i]['p'])
        seed, rad = scored[idx]['seed'], scored[idx]['r']
        p_hat, overlap_len = scored[idx]['p'], scored[idx]['L']
        d_band = seed[0] - rad, seed[0] + rad
        res = {'d_band': d_band, 'p': p_hat, 'len': overlap_len}
        area = 2 * rad * overlap_len
        mu_H1, sd_H1 = H1_moments(len(self.alphabet), self.wordlen, area, overlap_len, p_hat)
        num_seeds = self.seed_count(d_band=d_band)
        res['score'] = (num_seeds - mu_H1) / sd_H1
        return res


def _check_ref_memory(alphabet, wordlen, allowed_memory):
    """The in-memory variants refuse word lengths whose k-mer table would not fit the allowed memory
    (``blot.py:596-604``: one python int -- 24 bytes under python 2 -- per possible k-mer)."""
    num_kmers = len(alphabet) ** wordlen
    mem_needed_gb = np.power(2, np.log2(24. * num_kmers) - 30)
    assert allowed_memory > 0, 'allowed memory must be positive'
    if mem_needed_gb > allowed_memory:
        raise MemoryError('not enough memory (max = %.2f GB) to store %d-mers (%.2f GB needed)'
                          % (allowed_memory, wordlen, mem_needed_gb))


class _RefMixin(object):
    """Shared behaviour of the reference's in-memory classes: built around ONE sequence (``ref``), every query
    names the other one, and seeds are iterated with T scanned left to right, hits of S ascending
    (``blot.py:607-620``) -- i.e. the table rows ordered by (j, i)."""

    def _init_ref(self, ref, allowed_memory, kw):
        self._ref_kw = dict(kw)
        self.allowed_memory = allowed_memory
        _check_ref_memory(kw['alphabet'], kw['wordlen'], allowed_memory)
        self.wordlen, self.alphabet = kw['wordlen'], kw['alphabet']
        self.g_max, self.sensitivity = kw['g_max'], kw['sensitivity']
        self.S, self.T = ref, None
        self._idx = None
        self._qidx = None                           # the query-batched index (similar_segments_many)

    def _set_query(self, seq):
        if self.T is not None and self.T == seq and self._idx is not None:
            return
        if self._idx is not None:
            self._idx.close()
        kw = dict(self._ref_kw)
        g_max, sensitivity = kw.pop('g_max'), kw.pop('sensitivity')
        self._base.__init__(self, self.S, seq, g_max=g_max, sensitivity=sensitivity, **kw)
        self._perm = None

    def _points(self):
        """The (d, a) points the class works on, in the order the device lists them: the table rows, or -- when the
        query IS the reference (``blot.py:612``: trivial seeds skipped, every other pair met from both sides) -- each
        non-trivial row followed by its mirror image."""
        rows = self.rows().astype(np.int64)
        if not self.self_comp:
            return rows
        nt = rows[rows[:, 0] != 0]
        pts = np.empty((2 * len(nt), 2), np.int64)
        pts[0::2] = nt
        pts[1::2] = nt * np.array([-1, 1])
        return pts

    def _presentation(self):
        if self._perm is None:
            pts = self._points()
            i, j = (pts[:, 1] + pts[:, 0]) // 2, (pts[:, 1] - pts[:, 0]) // 2
            self._perm = np.lexsort((i, j))
        return self._perm

    def seeds(self, exclude_trivial=True):
        assert self.T is not None
        pts = self._points()[self._presentation()]
        return list(zip(((pts[:, 1] + pts[:, 0]) // 2).tolist(), ((pts[:, 1] - pts[:, 0]) // 2).tolist()))

    def seed_count(self, d_band=None, a_band=None):
        """The in-memory classes count their own seed list (``blot.py:622-637, 683-698``), not table rows: for a self
        comparison that is every non-trivial row and its mirror image."""
        if not self.self_comp:
            return self._base.seed_count(self, d_band=d_band, a_band=a_band)

        def nontrivial(db):
            c = self._idx.count(db, a_band)
            if db is None or db[0] <= 0 <= db[1]:
                c -= self._idx.count((0, 0), a_band)
            return c
        mirror = None if d_band is None else (-d_band[1], -d_band[0])
        return nontrivial(d_band) + nontrivial(mirror)


class WordBlotLocalRef(_RefMixin, WordBlot):
    """In-memory variant of :class:`WordBlot` (``blot.py:626-700``): ``WordBlotLocalRef(ref, allowed_memory=1, **kw)``,
    then ``similar_segments(seq, K_min, p_min)`` / ``score_seeds_(seq, K)`` for any number of query sequences."""
    _base = WordBlot

    def __init__(self, ref, allowed_memory=1, **kw):
        self._init_ref(ref, allowed_memory, kw)

    def score_seeds_(self, seq, K):
        self._set_query(seq)
        return WordBlot.score_seeds(self, K)

    def similar_segments(self, seq, K_min, p_min, at_least_one=False):
        self._set_query(seq)
        return WordBlot.similar_segments(self, K_min, p_min, at_least_one=at_least_one)

    def similar_segments_many(self, queries, K_min, p_min, at_least_one=False, arena=None, strands='+', complement=None):
        """``[list(self.similar_segments(q, K_min, p_min, at_least_one)) for q in queries]`` -- same segments, order, p
        and scores -- out of one set of kernel launches for all queries (kernels K10 of pw_qseeds.hip) instead of one index
        per query: the reference sequence is encoded and sorted once per object, the queries' seeds come out in the order
        the class lists them (the query scanned left to right), and the neighbour counts, the components and the segments'
        seed counts of all queries take one launch each.

        ``K_min`` and ``p_min`` are scalars for the whole call.  A query equal to the reference is a self comparison
        (``blot.py:612``) and goes through the per-query path.  ``arena``, optional: ``(device_arena, offsets, lengths)``
        of a :class:`biseqt_amd.batch.DeviceArena` that already holds the queries, in order, to be read in place.

        ``strands``: ``'+'`` (the default: the queries as written), ``'-'`` or ``'both'``.  A query on the minus strand IS the
        sequence ``T = rc(query)`` -- position ``j'`` of ``T`` is letter ``len - 1 - j'`` of the query, complemented, the
        convention :mod:`biseqt_amd.overlap` documents -- and everything reported for it (segments, their diagonals and
        antidiagonals) is in the frame of that ``T``: with ``'-'``, ``out[q]`` is
        ``list(self.similar_segments(reverse_complement(queries[q], complement), K_min, p_min, at_least_one))``; with
        ``'both'`` it is the plus list followed by the minus list, out of ONE build that lists every query on both strands.
        Every dict then also has ``'strand'``.  ``at_least_one`` applies to each strand on its own.  The device forms the
        minus strand's k-mers from the forward letters (with ``arena`` the caller's frames are read in place for both
        strands); no reverse complement is materialised for seeding.  A listed entry whose letters equal the reference
        after its own strand is applied -- a query equal to ``rc(ref)`` under ``'-'`` -- is a self comparison and goes
        through the per-query path.  ``complement``: a table (:func:`biseqt_amd.sequence.complement_table`) or the
        ``mappings`` of ``Alphabet.transform``; a missing or invalid one raises ``ValueError`` before any device call."""
        queries = list(queries)
        assert all(isinstance(T, Sequence) and T.alphabet == self.alphabet for T in queries), \
            'queries are Sequences over the index alphabet'
        assert np.ndim(K_min) == 0 and np.ndim(p_min) == 0, 'K_min and p_min are scalars for the whole call'
        assert K_min > 0, 'K_min must be positive'
        if strands not in ('+', '-', 'both'):
            raise ValueError("strands is '+', '-' or 'both', not %r" % (strands,))
        if strands != '+':
            return self._similar_segments_stranded(queries, K_min, p_min, at_least_one, arena, strands, complement)
        batched = [k for k, T in enumerate(queries) if not T == self.S]
        if at_least_one:                              # (a query shorter than a word has no seeds: known without the device)
            assert all(len(queries[k]) >= self.wordlen for k in batched), 'no seeds found while at_least_one=True'
        out = [None] * len(queries)
        if batched:
            if arena is None:
                letters, offs, lens = pack_reads([queries[k] for k in batched])
            else:
                letters, offs, lens = arena
                offs, lens = np.asarray(offs, np.int64), np.asarray(lens, np.int64)
                assert len(offs) == len(lens) == len(queries) and lens.tolist() == [len(T) for T in queries]
                offs, lens = offs[batched], lens[batched]
            for k, s in zip(batched, self._batched_segments(letters, offs, lens, K_min, p_min, at_least_one)):
                out[k] = s
        for k, T in enumerate(queries):
            if out[k] is None:                        # the reference itself: mirrored points, the per-query path
                out[k] = list(self.similar_segments(T, K_min, p_min, at_least_one=at_least_one))
        return out

    def _batched_segments(self, letters, offs, lens, K_min, p_min, at_least_one, strands=None, comp=None):
        """One list of segments per listed entry ``letters[offs[e]:offs[e] + lens[e]]`` (``strands``: one flag per entry, a
        minus entry being the reverse complement of its letters), out of one build of the query-batched index."""
        if self._qidx is None:
            self._qidx = _QIndex(self.S, self.wordlen, self.alphabet, device=self._ref_kw.get('device', 0))
        qi = self._qidx
        qi.build(letters, offs, lens, self._ref_kw.get('max_rows', 0), strands=strands, complement=comp)
        row_offsets = qi.row_offsets()
        d_radius, a_radius = int(np.ceil(self.band_radius(K_min))), K_min
        L = len(self.alphabet)
        qi.graph_build(1. * a_radius / d_radius, a_radius)
        counts = qi.graph_counts()
        p = seed_ps_from_counts(counts, d_radius, a_radius, L, self.wordlen)
        avail = available_seeds_many(p, p_min, row_offsets, at_least_one)
        labels = qi.graph_components(avail) if avail.any() else np.full(len(p), -1, np.int32)
        return segments_from_arrays(counts, labels, qi.rows(), row_offsets, lens, len(self.S), d_radius, a_radius, L,
                                    self.wordlen, qi.count_boxes)

    def _similar_segments_stranded(self, queries, K_min, p_min, at_least_one, arena, strands, complement):
        """:meth:`similar_segments_many` for ``strands`` ``'-'`` / ``'both'``: every query is listed once per selected
        strand (all plus entries, then all minus entries) over ONE copy of the forward letters."""
        from .overlap import _complement
        from .sequence import reverse_complement
        comp = _complement(complement, len(self.alphabet), self.alphabet)         # (ValueError before any device call)
        n = len(queries)
        entries = [(k, f) for f in ((0, 1) if strands == 'both' else (1,)) for k in range(n)]
        ref = self.S.as_array(np.uint8)
        rc_ref = comp[ref[::-1]]                      # rc(T) == S  <=>  T == rc(S): no query is reversed to find out

        def is_self(k, f):
            return len(queries[k]) == len(ref) and bool((queries[k].as_array(np.uint8) == (rc_ref if f else ref)).all())
        batched = [e for e in entries if not is_self(*e)]
        if at_least_one:
            assert all(len(queries[k]) >= self.wordlen for k, _ in batched), 'no seeds found while at_least_one=True'
        if arena is None:
            letters, offs, lens = pack_reads(queries)
        else:
            letters, offs, lens = arena
            assert len(offs) == len(lens) == n and np.asarray(lens).tolist() == [len(T) for T in queries]
        offs, lens = np.asarray(offs, np.int64), np.asarray(lens, np.int64)
        found = {}
        if batched:
            qs = np.array([k for k, _ in batched], np.int64)
            flags = np.array([f for _, f in batched], np.uint8)
            found = dict(zip(batched, self._batched_segments(letters, offs[qs], lens[qs], K_min, p_min, at_least_one,
                                                             strands=flags, comp=comp)))
        out = [[] for _ in queries]
        for k, f in entries:
            if (k, f) in found:
                segs = found[(k, f)]
            else:                                     # the reference itself on this strand: the per-query path
                T = reverse_complement(queries[k], comp) if f else queries[k]
                segs = [dict(rec) for rec in self.similar_segments(T, K_min, p_min, at_least_one=at_least_one)]
            for rec in segs:
                rec['strand'] = '-' if f else '+'
            out[k] += segs
        return out

    def batched_timings(self):
        """Device milliseconds of the last :meth:`similar_segments_many`: build, graph, components, counts; hook rounds."""
        return self._qidx.timings() if self._qidx is not None else None

    def close(self):
        if self._qidx is not None:
            self._qidx.close()
            self._qidx = None
        if self._idx is not None:
            self._idx.close()


class WordBlotOverlapRef(_RefMixin, WordBlotOverlap):
    """In-memory variant of :class:`WordBlotOverlap` (``blot.py:582-624``)."""
    _base = WordBlotOverlap

    def __init__(self, ref, allowed_memory=1, **kw):
        self._init_ref(ref, allowed_memory, kw)

    def score_seeds_(self, seq):
        self._set_query(seq)
        return WordBlotOverlap.score_seeds(self)

    def highest_scoring_overlap_band(self, seq):
        self._set_query(seq)
        return WordBlotOverlap.highest_scoring_overlap_band(self)


class WordBlotMultiple(SeedIndexMultiple):
    """Local similarities shared by more than two sequences (``blot.py:726-1038``).

    Keyword Args:
        g_max (float): upper bound for indel probabilities.  sensitivity (float): desired band sensitivity.
        wordlen, alphabet, device, max_rows: as :class:`biseqt_amd.seeds.SeedIndexMultiple`.
    """

    def __init__(self, *seqs, **kw):
        g_max, sensitivity = kw.pop('g_max'), kw.pop('sensitivity')
        assert 0 < g_max < 1 and 0 < sensitivity < 1
        self.g_max = g_max
        self.sensitivity = sensitivity
        super(WordBlotMultiple, self).__init__(*seqs, **kw)
        self._graph_key = None

    def band_radius(self, K):
        return band_radius(K, self.g_max, self.sensitivity)

    def estimate_match_probability(self, num_seeds, K, volume):
        """``p = ((n - V p0^(w (N-1))) / K)^(1/w)``: the null word probability has the exponent ``w (N-1)``, the root
        is the ``w``-th (``blot.py:787-801``).  0 without seeds or where the logarithm is undefined (the reference
        turns numpy's warning into an error and answers it with 0, :34); capped at 1."""
        word_p_null = (1. / len(self.alphabet)) ** (self.wordlen * (len(self.seqs) - 1))
        if not num_seeds > 0:
            return 0
        word_p = (num_seeds - volume * word_p_null) / K
        if not word_p > 0:
            return 0
        return min(np.exp(np.log(word_p) / self.wordlen), 1)

    def _radii(self, K):
        d_radius = int(np.ceil(self.band_radius(K)))
        a_radius = int(np.ceil(len(self.seqs) * K / 2.))           # blot.py:822, :939
        return d_radius, a_radius

    def _graph(self, d_radius, a_radius):
        """The neighbourhood graph of ``find_all_neighbors`` (``blot.py:833-868``), built on the GPU once per radii."""
        key = (d_radius, a_radius)
        if self._graph_key != key:
            self._idx.graph_build(1. * a_radius / d_radius, a_radius)
            self._graph_key = key

    def find_all_neighbors(self, d_radius, a_radius):
        """``[((ds, a), neighs), ..]``: for every seed the indices of the other seeds with ``|d_k c - d'_k c| <= R`` for
        all k and ``|a - a'| <= R``, ``c = a_radius / d_radius``, ``R = a_radius`` (``blot.py:833-868``)."""
        if not self.seed_count():
            return []
        self._graph(d_radius, a_radius)
        off, adj = self._idx.graph_fetch()
        return [(seed, adj[off[k]:off[k + 1]].tolist()) for k, seed in enumerate(self.seeds())]

    def _seed_ps(self, K):
        """Per seed (table order) the ``p`` of ``score_seeds``, and the radii.  The neighbour counts take few distinct
        values: ``p`` is evaluated once per value, with the reference's scalar arithmetic."""
        d_radius, a_radius = self._radii(K)
        self._graph(d_radius, a_radius)
        n = self._idx.graph_counts()
        volume = (2 * d_radius) ** (len(self.seqs) - 1) * K        # blot.py:825: a python number, never int64
        uniq, inv = np.unique(n, return_inverse=True)
        vals = np.array([self.estimate_match_probability(int(c) + 1, K, volume) for c in uniq.tolist()], np.float64)
        return vals[inv.reshape(-1)], d_radius, a_radius

    def score_seeds(self, K):
        """One dict per seed, in table order: ``seed`` (ds, a), ``neighs`` (indices of the seeds in its neighbourhood),
        ``p`` estimated match probability of a segment of length K centred there (``blot.py:803-831``)."""
        if not self.seed_count():
            return []
        p, _, _ = self._seed_ps(K)
        off, adj = self._idx.graph_fetch()
        return [{'seed': seed, 'neighs': adj[off[k]:off[k + 1]].tolist(), 'p': p[k]}
                for k, seed in enumerate(self.seeds())]

    def score_num_seeds(self, num_seeds, **kw):
        """z-scores of an observed number of seeds in a volume against H0 and H1 (``blot.py:870-916``)."""
        p_match, seglen, volume = kw['p_match'], kw['seglen'], kw['volume']
        if volume == 0:
            return float('-inf'), float('-inf')
        if p_match == 1.:
            p_match = 1 - np.finfo(float).eps
        p_H0 = (1. / len(self.alphabet)) ** (len(self.seqs) - 1)
        pw_H0 = p_H0 ** self.wordlen
        mu_H0 = volume * pw_H0
        sd_H0 = np.sqrt(volume * ((1 - pw_H0) * (pw_H0 + 2 * p_H0 * pw_H0 / (1 - p_H0)) - 2 * self.wordlen * pw_H0 ** 2))
        p_H1 = p_match
        pw_H1 = p_H1 ** self.wordlen
        mu_H1 = mu_H0 + seglen * pw_H1
        sd_H1 = np.sqrt(sd_H0 ** 2 + seglen * ((1 - pw_H1) * (pw_H1 + 2 * p_H1 * pw_H1 / (1 - p_H1)) -
                                               2 * self.wordlen * pw_H1 ** 2))
        return (num_seeds - mu_H0) / sd_H0, (num_seeds - mu_H1) / sd_H1

    def similar_segments(self, K_min, p_min, at_least_one=False):
        """All maximal local similarities of a minimum length and match probability (``blot.py:918-1038``): seeds
        with ``p >= p_min`` grouped into the connected components of the neighbourhood graph (the reference's
        depth-first search; on the GPU), each group's bounding segment clamped, scored and yielded in the order of
        its first seed.  Every group's seed count comes from one ``count_many`` launch."""
        if not self.seed_count():
            assert not at_least_one, 'no seeds found while at_least_one=True'
            return
        N = len(self.seqs)
        p, d_radius, a_radius = self._seed_ps(K_min)
        avail = p >= p_min
        if not avail.any() and at_least_one:
            avail[np.argmax(p)] = True                   # the first seed of highest p
        if not avail.any():
            return
        labels = self._idx.graph_components(avail)
        idx = np.flatnonzero(labels >= 0)
        order = idx[np.argsort(labels[idx], kind='stable')]     # grouped by component, table order inside
        starts = np.flatnonzero(np.r_[True, labels[order][1:] != labels[order][:-1]])
        rows = self.rows()[order].astype(np.int64)
        firsts = order[starts]                           # the seed each search starts from: its smallest index
        first_rows = self.rows()[firsts].astype(np.int64)
        # d ranges: the first seed opens them with +-d_radius, every later one only widens them to its own d_k
        # (blot.py:946-958); a is widened by +-a_radius for every seed
        d_lo = np.minimum(np.minimum.reduceat(rows[:, :-1], starts), first_rows[:, :-1] - d_radius)
        d_hi = np.maximum(np.maximum.reduceat(rows[:, :-1], starts), first_rows[:, :-1] + d_radius)
        a_lo = np.minimum.reduceat(rows[:, -1], starts) - a_radius
        a_hi = np.maximum.reduceat(rows[:, -1], starts) + a_radius
        psum = np.add.reduceat(p[order], starts)
        cnt = np.diff(np.r_[starts, len(order)])
        len0, total = len(self.seqs[0]), sum(len(S) for S in self.seqs)
        segs = []
        for s in range(len(starts)):                     # labels ascend: the order of the first seeds
            ds = [(min(len0, max(int(d_lo[s, k]), -len(self.seqs[k + 1]))),
                   min(len0, max(int(d_hi[s, k]), -len(self.seqs[k + 1])))) for k in range(N - 1)]
            segs.append((ds, (max(int(a_lo[s]), 0), min(int(a_hi[s]), total))))
        counts = self.seed_counts(segs)
        for s, seg in enumerate(segs):
            ds_band, a_band = seg
            p_hat = (psum[s] + p[firsts[s]]) / (cnt[s] + 1)       # the start seed is counted twice (:977-980)
            K_hat = np.ceil((a_band[1] - a_band[0]) // N)          # python 2's integer `/` (:1016)
            volume = a_band[1] - a_band[0]                          # python ints: no int64 overflow
            for d_min, d_max in ds_band:
                volume *= d_max - d_min
            scores = self.score_num_seeds(num_seeds=counts[s], volume=volume, seglen=K_hat, p_match=p_hat)
            yield {'segment': seg, 'p': p_hat, 'scores': scores}


class WordBlotMultipleFast(WordBlotMultiple):
    """The reference's in-memory variant of :class:`WordBlotMultiple` (``blot.py:1040-1083``): same results, two or more
    sequences, and the same refusal of word lengths whose per-k-mer hit lists would not fit ``allowed_memory`` GB."""

    def __init__(self, *seqs, **kw):
        self.allowed_memory = kw.pop('allowed_memory', 1)
        _check_ref_memory(kw['alphabet'], kw['wordlen'], self.allowed_memory)
        g_max, sensitivity = kw.pop('g_max'), kw.pop('sensitivity')
        assert 0 < g_max < 1 and 0 < sensitivity < 1
        self.g_max = g_max
        self.sensitivity = sensitivity
        self._graph_key = None
        self._init_index(seqs, kw)

"""Exact-match k-mer seeds in diagonal coordinates (host side of include/pw_seeds.h).

Mirrors ``biseqt/seeds.py:SeedIndex`` (:21-237): same constructor keywords (``wordlen``, ``alphabet``, ``mask``;
``path`` / ``kmer_cache`` / ``log_level`` are accepted and ignored -- there is no SQLite file, the table lives in
HBM), same classmethods for the coordinate maps, same ``seeds()`` / ``seed_count()`` results in the same order.

    >>> from biseqt_amd.seeds import SeedIndex
    >>> from biseqt_amd.sequence import Alphabet
    >>> A = Alphabet('ACGT')
    >>> S, T = A.parse('TAAGCGT'), A.parse('GGCGTAA')
    >>> list(SeedIndex(S, T, wordlen=3, alphabet=A).seeds())
    [(4, 2), (3, 1), (0, 4)]
"""
import ctypes as C
from itertools import product

import numpy as np

from . import _pwlib as W
from .batch import DeviceBuffer
from .kmers import check_limits, mask_bits
from .sequence import Sequence


class _Handle(object):
    """What the three index owners share: the library's error channel, the handle's lifetime, and the neighbourhood graph
    of the index's points -- the rows of its table, except for a pairwise self comparison -- behind ``<_prefix>graph_*``."""
    _prefix = None                                   # 'pw_seeds_', 'pw_mseeds_' or 'pw_qseeds_'
    _edges = None                                    # edge count of the last graph_build; None before one

    def _call(self, name, *args):
        """``<_prefix><name>(handle, *args)``; a negative return raises with the library's message."""
        r = getattr(self.lib, self._prefix + name)(self.handle, *args)
        if r < 0:
            raise RuntimeError('%s%s failed: %s' % (self._prefix, name, self.error()))
        return r

    def error(self):
        return (getattr(self.lib, self._prefix + 'last_error')() or b'').decode('utf-8', 'replace')

    def _num_points(self):
        return self.num_rows()

    def graph_build(self, d_coeff, radius):
        """Neighbourhood graph of the points: max(|d - d'| * d_coeff, |a - a'|) <= radius -- for an N-way index with every
        diagonal coordinate held to it, max_k |d_k c - d'_k c| <= radius and |a - a'| <= radius; for a query-batched one
        query by query.  Returns the edge count."""
        self._edges = self._call('graph_build', float(d_coeff), float(radius))
        return self._edges

    def graph_counts(self):
        n = self._num_points()
        out = np.zeros(max(n, 1), np.int32)
        self._call('graph_counts', out.ctypes.data, n)
        return out[:n]

    def graph_fetch(self):
        """CSR adjacency: (offsets[n + 1], neighbours[edges])."""
        edges = self._edges or 0                     # (None before a graph_build: the library refuses the call below)
        off = np.zeros(max(self._num_points(), 0) + 1, np.int64)
        adj = np.zeros(max(edges, 1), np.int32)
        self._call('graph_fetch', off.ctypes.data, adj.ctypes.data)
        return off, adj[:edges]

    def graph_components(self, avail):
        n = self._num_points()
        av = np.ascontiguousarray(avail, np.uint8)
        assert av.size == n
        out = np.full(max(n, 1), -1, np.int32)
        self._call('graph_components', av.ctypes.data, out.ctypes.data)
        return out[:n]

    def close(self):
        if getattr(self, 'handle', None):
            getattr(self.lib, self._prefix + 'destroy')(self.handle)
            self.handle = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _Index(_Handle):
    """Thin owner of a ``pw_seed_index`` handle."""
    _prefix = 'pw_seeds_'

    def __init__(self, S, T, wordlen, alphabet, mask=(), self_comp=-1, device=0):
        self.lib = W.load()
        s = S.as_array(np.uint8) if isinstance(S, Sequence) else np.ascontiguousarray(S, np.uint8)
        t = T.as_array(np.uint8) if isinstance(T, Sequence) else np.ascontiguousarray(T, np.uint8)
        bits = mask_bits(list(mask))
        marr = (C.c_uint64 * max(len(bits), 1))(*bits)
        self.nS, self.nT, self.wordlen = len(s), len(t), wordlen
        self.handle = self.lib.pw_seeds_create(device, s.ctypes.data, len(s), t.ctypes.data, len(t), len(alphabet),
                                               wordlen, marr, len(bits), self_comp)
        if not self.handle:
            raise RuntimeError('pw_seeds_create failed: ' + self.error())
        self.built = False

    def build(self, max_rows=0, stream=None):
        if self.lib.pw_seeds_build(self.handle, max_rows, stream) != 0:
            raise RuntimeError('pw_seeds_build failed: ' + self.error())
        self.built = True
        return self.lib.pw_seeds_num_rows(self.handle)

    def rows(self):
        """(n, 2) int32 array of (d, a) in table order."""
        n = self.lib.pw_seeds_num_rows(self.handle)
        out = np.zeros((max(n, 1), 2), np.int32)
        if self.lib.pw_seeds_rows(self.handle, out.ctypes.data, n) != 0:
            raise RuntimeError('pw_seeds_rows failed: ' + self.error())
        return out[:n]

    def rows_device(self):
        n = self.lib.pw_seeds_num_rows(self.handle)
        return DeviceBuffer(self.lib.pw_seeds_rows_device(self.handle), 8 * n, self)

    def count(self, d_band=None, a_band=None):
        d = d_band if d_band is not None else (0, 0)
        a = a_band if a_band is not None else (0, 0)
        n = self.lib.pw_seeds_count(self.handle, d_band is not None, int(d[0]), int(d[1]),
                                    a_band is not None, int(a[0]), int(a[1]))
        if n < 0:
            raise RuntimeError('pw_seeds_count failed: ' + self.error())
        return n

    def band_neighbours(self, radius):
        """Per row: how many other rows lie within 1 on the axis d / radius(d) (radius: table over d = -nT .. nS)."""
        n = self.lib.pw_seeds_num_rows(self.handle)
        rad = np.ascontiguousarray(radius, np.float64)
        out = np.zeros(max(n, 1), np.int32)
        if self.lib.pw_seeds_band_neighbours(self.handle, rad.ctypes.data, rad.size, out.ctypes.data, n) != 0:
            raise RuntimeError('pw_seeds_band_neighbours failed: ' + self.error())
        return out[:n]

    def graph_points(self):
        """(n, 2) int32 array of the graph's points (d, a): the rows, or for a self comparison the non-trivial rows
        each followed by its mirror image."""
        n = self.lib.pw_seeds_graph_num_points(self.handle)
        out = np.zeros((max(n, 1), 2), np.int32)
        if self.lib.pw_seeds_graph_points(self.handle, out.ctypes.data, n) != 0:
            raise RuntimeError('pw_seeds_graph_points failed: ' + self.error())
        return out[:n]

    def _num_points(self):
        return self.lib.pw_seeds_graph_num_points(self.handle)

    def kmers(self, which):
        n = (self.nT if which else self.nS) - self.wordlen + 1
        out = np.zeros(max(n, 1), np.int64)
        got = self.lib.pw_seeds_kmers(self.handle, which, out.ctypes.data, max(n, 0))
        if got < 0:
            raise RuntimeError('pw_seeds_kmers failed: ' + self.error())
        return out[:got]

    @property
    def is_self(self):
        return bool(self.lib.pw_seeds_is_self(self.handle))

    def build_ms(self):
        return self.lib.pw_seeds_build_ms(self.handle)

    def algorithmic_bytes(self):
        return self.lib.pw_seeds_algorithmic_bytes(self.handle)


class SeedIndex(object):
    """An index for seeds in diagonal coordinates (``seeds.py:21-47``).

    Args:
        S, T (Sequence): the 1st and 2nd sequence; equal contents make it a self comparison.
    Keyword Args:
        wordlen (int), alphabet (Alphabet), mask (list of sets): as in the reference.
        device (int): HIP device ordinal.  max_rows (int): refuse tables larger than this (default 2^31 - 1).
    """

    def __init__(self, S, T, kmer_cache=None, **kw):
        alphabet, wordlen = kw['alphabet'], kw['wordlen']
        check_limits(alphabet, wordlen)
        assert isinstance(S, Sequence) and isinstance(T, Sequence)
        assert S.alphabet == alphabet and T.alphabet == alphabet
        self.alphabet, self.wordlen = alphabet, wordlen
        self.mask = kw.get('mask', [])
        self.S, self.T = S, T
        self.self_comp = S == T                               # seeds.py:33
        self._idx = _Index(S, T, wordlen, alphabet, self.mask, self_comp=int(self.self_comp),
                           device=kw.get('device', 0))
        self._idx.build(kw.get('max_rows', 0))
        self._rows = None

    # ---- coordinate maps (seeds.py:55-106) ----
    @classmethod
    def to_diagonal_coordinates(cls, i, j):
        return i - j, i + j

    @classmethod
    def to_ij_coordinates(cls, d, a):
        # the reference divides with python 2's integer `/`; a + d and a - d are even for every seed
        return (a + d) // 2, (a - d) // 2

    @classmethod
    def to_ij_coordinates_seg(cls, seg):
        corners = [cls.to_ij_coordinates(d, a) for d, a in product(*seg)]
        i_start = max(min(i for i, _ in corners), 0)
        j_start = max(min(j for _, j in corners), 0)
        i_end = max(i for i, j in corners)
        j_end = max(j for _, j in corners)
        return (i_start, i_end), (j_start, j_end)

    # ---- the table ----
    def rows(self):
        """(n, 2) int32 array of (d, a) in the reference's rowid order (cached)."""
        if self._rows is None:
            self._rows = self._idx.rows()
        return self._rows

    def rows_device(self):
        return self._idx.rows_device()

    def seeds(self, d_band=None, exclude_trivial=False):
        """Yields all seeds ``(i, j)``, optionally those in a diagonal band (``seeds.py:164-197``); a self
        comparison also yields the mirror image of every non-trivial seed."""
        rows = self.rows()
        if d_band is not None:
            assert len(d_band) == 2, 'need a 2-tuple for diagonal band'
            rows = rows[(rows[:, 0] >= d_band[0]) & (rows[:, 0] <= d_band[1])]
        d, a = rows[:, 0].astype(np.int64), rows[:, 1].astype(np.int64)
        ii, jj = ((a + d) // 2).tolist(), ((a - d) // 2).tolist()
        for i, j in zip(ii, jj):
            if self.self_comp and exclude_trivial and i == j:
                continue
            yield (i, j)
            if self.self_comp and i != j:
                yield (j, i)

    def seed_count(self, d_band=None, a_band=None):
        """Number of rows of the table, optionally inside a diagonal and / or an antidiagonal band
        (``seeds.py:199-237``); counted on the device."""
        if d_band is not None:
            assert len(d_band) == 2, 'need a 2-tuple for diagonal band'
        if a_band is not None:
            assert len(a_band) == 2, 'need a 2-tuple for antidiagonal band'
        return self._idx.count(d_band, a_band)

    def build_ms(self):
        return self._idx.build_ms()

    def close(self):
        self._idx.close()


class _MIndex(_Handle):
    """Thin owner of a ``pw_mseed_index`` handle (include/pw_mseeds.h)."""
    _prefix = 'pw_mseeds_'

    def __init__(self, seqs, wordlen, alphabet, device=0):
        self.lib = W.load()
        arrs = [s.as_array(np.uint8) if isinstance(s, Sequence) else np.ascontiguousarray(s, np.uint8) for s in seqs]
        self.n = len(arrs)
        ptrs = (C.c_void_p * max(self.n, 1))(*[a.ctypes.data for a in arrs])
        lens = (C.c_int64 * max(self.n, 1))(*[len(a) for a in arrs])
        self.handle = self.lib.pw_mseeds_create(device, ptrs, lens, self.n, len(alphabet), wordlen)
        if not self.handle:
            raise RuntimeError('pw_mseeds_create failed: ' + self.error())
        self._edges = None

    def build(self, max_rows=0, stream=None):
        if self.lib.pw_mseeds_build(self.handle, max_rows, stream) != 0:
            raise RuntimeError('pw_mseeds_build failed: ' + self.error())
        self._edges = None
        return self.num_rows()

    def num_rows(self):
        return self.lib.pw_mseeds_num_rows(self.handle)

    def rows(self):
        """(rows, N) int32 array of (d_1, .., d_{N-1}, a) in table order."""
        n = self.num_rows()
        out = np.zeros((max(n, 1), self.n), np.int32)
        if self.lib.pw_mseeds_rows(self.handle, out.ctypes.data, n) != 0:
            raise RuntimeError('pw_mseeds_rows failed: ' + self.error())
        return out[:n]

    def rows_device(self):
        return DeviceBuffer(self.lib.pw_mseeds_rows_device(self.handle), 4 * self.n * self.num_rows(), self)

    def count_many(self, lo, hi, have):
        """Row counts of many hyper-boxes in one launch: lo, hi, have are (boxes, N) arrays (have: bound or not)."""
        lo = np.ascontiguousarray(lo, np.int32).reshape(-1, self.n)
        hi = np.ascontiguousarray(hi, np.int32).reshape(-1, self.n)
        have = np.ascontiguousarray(have, np.uint8).reshape(-1, self.n)
        assert lo.shape == hi.shape == have.shape
        out = np.zeros(max(len(lo), 1), np.int64)
        if self.lib.pw_mseeds_count_many(self.handle, len(lo), lo.ctypes.data, hi.ctypes.data, have.ctypes.data,
                                         out.ctypes.data) != 0:
            raise RuntimeError('pw_mseeds_count_many failed: ' + self.error())
        return out[:len(lo)]

    def timings(self):
        """Device milliseconds of the last build, graph build, components and count_many calls (HIP events)."""
        L = self.lib
        return {'build': L.pw_mseeds_build_ms(self.handle), 'graph': L.pw_mseeds_graph_ms(self.handle),
                'components': L.pw_mseeds_components_ms(self.handle), 'counts': L.pw_mseeds_count_ms(self.handle)}

    def algorithmic_bytes(self):
        return self.lib.pw_mseeds_algorithmic_bytes(self.handle)


class _QIndex(_Handle):
    """Thin owner of a ``pw_qseed_index`` handle (include/pw_qseeds.h): one reference sequence, indexed once, and the
    seeds of any number of queries against it per :meth:`build`."""
    _prefix = 'pw_qseeds_'

    def __init__(self, ref, wordlen, alphabet, device=0):
        self.lib = W.load()
        r = ref.as_array(np.uint8) if isinstance(ref, Sequence) else np.ascontiguousarray(ref, np.uint8)
        self.device, self.alphabet_len = device, len(alphabet)
        self.handle = self.lib.pw_qseeds_create(device, r.ctypes.data, len(r), len(alphabet), wordlen)
        if not self.handle:
            raise RuntimeError('pw_qseeds_create failed: ' + self.error())
        self._edges = None

    def build(self, arena, offsets, lengths, max_rows=0, stream=None, strands=None, complement=None):
        """Seeds of the queries ``arena[offsets[q]:offsets[q] + lengths[q]]``.  ``arena`` is a uint8 array (the layout of
        :func:`biseqt_amd.batch.pack_reads`) or a :class:`biseqt_amd.batch.DeviceArena`, which is read in place.
        Returns the number of rows.

        ``strands``: one ``'+'`` / ``'-'`` (or 0 / 1) per listed entry.  A minus entry IS the sequence ``T = rc(query)``
        (position ``j'`` of ``T`` is letter ``len - 1 - j'`` of the query, complemented -- the convention of
        :mod:`biseqt_amd.overlap`): its rows are those of the materialised reverse complement passed as an ordinary query,
        and the device forms its k-mers from the forward letters.  Two entries may name the same letters with different
        strands.  ``complement`` (a table of ``len(alphabet)`` letter indices, its own inverse) is needed when some entry is
        ``'-'``; bad strands or a bad complement raise ``ValueError`` before any device call."""
        offsets = np.ascontiguousarray(offsets, np.int64)
        lengths = np.ascontiguousarray(lengths, np.int32)
        assert offsets.ndim == 1 and offsets.shape == lengths.shape
        if strands is not None:
            from .overlap import _complement, _strand_flags
            flags = _strand_flags(strands, len(offsets))
            comp = _complement(complement, self.alphabet_len) if flags.any() or complement is not None else None
        if isinstance(arena, np.ndarray):
            arena = np.ascontiguousarray(arena, np.uint8)
            ptr, nbytes, on_device = arena.ctypes.data, arena.nbytes, 0
        else:
            assert arena.device == self.device, 'the arena lives on another device'
            ptr, nbytes, on_device = arena.ptr, arena.nbytes, 1
        self._edges = None
        if strands is not None:
            if self.lib.pw_qseeds_build_stranded(self.handle, ptr, nbytes, on_device, offsets.ctypes.data, lengths.ctypes.data,
                                                 flags.ctypes.data, None if comp is None else comp.ctypes.data, len(offsets),
                                                 max_rows, stream) != 0:
                raise RuntimeError('pw_qseeds_build_stranded failed: ' + self.error())
        elif self.lib.pw_qseeds_build(self.handle, ptr, nbytes, on_device, offsets.ctypes.data, lengths.ctypes.data, len(offsets),
                                      max_rows, stream) != 0:
            raise RuntimeError('pw_qseeds_build failed: ' + self.error())
        return self.num_rows()

    def num_rows(self):
        return self.lib.pw_qseeds_num_rows(self.handle)

    def num_queries(self):
        return self.lib.pw_qseeds_num_queries(self.handle)

    def rows(self):
        """(rows, 3) int32 array of (q, d, a) in (q, j, i) order."""
        n = self.num_rows()
        out = np.zeros((max(n, 1), 3), np.int32)
        if self.lib.pw_qseeds_rows(self.handle, out.ctypes.data, n) != 0:
            raise RuntimeError('pw_qseeds_rows failed: ' + self.error())
        return out[:n]

    def row_offsets(self):
        """int64 array of num_queries + 1 entries: the rows of query q are ``rows[off[q]:off[q + 1]]``."""
        out = np.zeros(self.num_queries() + 1, np.int64)
        if self.lib.pw_qseeds_row_offsets(self.handle, out.ctypes.data) != 0:
            raise RuntimeError('pw_qseeds_row_offsets failed: ' + self.error())
        return out

    def rows_device(self):
        return DeviceBuffer(self.lib.pw_qseeds_rows_device(self.handle), 12 * self.num_rows(), self)

    def count_boxes(self, q, dmin, dmax, amin, amax):
        """Row counts of many (query, d band, a band) boxes in one launch."""
        arrs = [np.ascontiguousarray(v, np.int32).reshape(-1) for v in (q, dmin, dmax, amin, amax)]
        n = len(arrs[0])
        assert all(len(v) == n for v in arrs)
        out = np.zeros(max(n, 1), np.int64)
        if self.lib.pw_qseeds_count_boxes(self.handle, n, *([v.ctypes.data for v in arrs] + [out.ctypes.data])) != 0:
            raise RuntimeError('pw_qseeds_count_boxes failed: ' + self.error())
        return out[:n]

    def timings(self):
        """Device milliseconds of the last build, graph build, components and count_boxes calls (HIP events), and the hook
        rounds the components took."""
        L = self.lib
        return {'build': L.pw_qseeds_build_ms(self.handle), 'graph': L.pw_qseeds_graph_ms(self.handle),
                'components': L.pw_qseeds_components_ms(self.handle), 'counts': L.pw_qseeds_count_ms(self.handle),
                'rounds': L.pw_qseeds_components_rounds(self.handle)}


MAX_SEQS = 16


class SeedIndexMultiple(object):
    """Seeds shared by more than two sequences, in diagonal coordinates (``seeds.py:234-433``).

    A seed is an N-tuple of positions ``(i_1, .., i_N)`` carrying the same k-mer, stored as ``(d_1, .., d_{N-1}, a)``
    with ``d_k = i_1 - i_{k+1}`` and ``a = sum(i_k)``.  The table lives in HBM (kernels K9 of pw_mseeds.hip); every
    argument is its own sequence and rows come in ``WordBlotMultipleFast.seeds()`` order (``blot.py:1061-1071``: k-mers
    ascending, then ``itertools.product`` of the positions, sequence 0 slowest) -- the SQL-backed reference drops
    repeated sequences and leaves its row order unspecified.

    Args:
        *seqs (Sequence): the sequences, more than two (``seeds.py:243``) and at most 16.
    Keyword Args:
        wordlen (int), alphabet (Alphabet): as in the reference; ``path`` / ``kmer_cache`` / ``log_level`` are accepted
        and ignored.  device (int): HIP device ordinal.  max_rows (int): refuse larger tables (default: 16 GB of rows).
    """

    def __init__(self, *seqs, **kw):
        assert len(seqs) > 2
        self._init_index(seqs, kw)

    def _init_index(self, seqs, kw):
        alphabet, wordlen = kw['alphabet'], kw['wordlen']
        check_limits(alphabet, wordlen)
        assert 2 <= len(seqs) <= MAX_SEQS, 'between 2 and %d sequences' % MAX_SEQS
        assert all(isinstance(S, Sequence) and S.alphabet == alphabet for S in seqs)
        self.alphabet, self.wordlen = alphabet, wordlen
        self.seqs = tuple(seqs)
        self._idx = _MIndex(self.seqs, wordlen, alphabet, device=kw.get('device', 0))
        self._idx.build(kw.get('max_rows', 0))
        self._rows = None

    # ---- coordinate maps (seeds.py:262-310) ----
    @classmethod
    def to_diagonal_coordinates(cls, *idxs):
        ds = tuple(idxs[0] - idxs[k] for k in range(1, len(idxs)))
        return ds, sum(idxs)

    @classmethod
    def to_ij_coordinates(cls, ds, a):
        # the reference divides with python 2's integer `/` (seeds.py:287)
        i0 = (a + sum(ds)) // (len(ds) + 1)
        return tuple([i0] + [i0 - d for d in ds])

    @classmethod
    def to_ij_coordinates_seg(cls, seg):
        """Start and end coordinate in every sequence of a segment ``([(d_min, d_max), ..], (a_min, a_max))``: the
        extremes over its corners, starts clipped at 0 (``seeds.py:291-310``)."""
        ds_range, a_range = seg
        corners = [cls.to_ij_coordinates(c[:-1], c[-1]) for c in product(*(list(ds_range) + [a_range]))]
        return [(max(min(c[k] for c in corners), 0), max(c[k] for c in corners)) for k in range(len(ds_range) + 1)]

    # ---- the table ----
    def rows(self):
        """(n, N) int32 array of (d_1, .., d_{N-1}, a) in table order (cached)."""
        if self._rows is None:
            self._rows = self._idx.rows()
        return self._rows

    def rows_device(self):
        return self._idx.rows_device()

    def seeds(self):
        """Yields every seed as ``(ds, a)``, ``ds`` a list (``seeds.py:377-389``)."""
        for r in self.rows().tolist():
            yield r[:-1], r[-1]

    def _box(self, ds_band, a_band):
        """One hyper-box as the (lo, hi, have) rows of count_many; a None band, or a None entry of ds_band, is
        unbounded."""
        N = len(self.seqs)
        lo, hi, have = [0] * N, [0] * N, [0] * N
        if ds_band is not None:
            assert len(ds_band) == N - 1
            for k, band in enumerate(ds_band):
                if band is None:
                    continue
                assert len(band) == 2
                lo[k], hi[k], have[k] = int(band[0]), int(band[1]), 1
        if a_band is not None:
            assert len(a_band) == 2, 'need a 2-tuple for antidiagonal band'
            lo[-1], hi[-1], have[-1] = int(a_band[0]), int(a_band[1]), 1
        return lo, hi, have

    def seed_counts(self, boxes):
        """``seed_count`` of many ``(ds_band, a_band)`` boxes, counted in one launch."""
        if not boxes:
            return []
        lo, hi, have = zip(*[self._box(ds, a) for ds, a in boxes])
        return [int(c) for c in self._idx.count_many(lo, hi, have)]

    def seed_count(self, ds_band=None, a_band=None):
        """Number of seeds, optionally inside a hyper-box (``seeds.py:391-433``); counted on the device."""
        return self.seed_counts([(ds_band, a_band)])[0]

    def close(self):
        self._idx.close()

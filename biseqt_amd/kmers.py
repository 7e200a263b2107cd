"""k-mers as integers (host side of include/pw_seeds.h).

Mirrors ``biseqt/kmers.py``: :func:`kmer_as_int` (:164-210) and :func:`as_kmer_seq` (:213-241) with the same
arguments and return values.  ``kmer_as_int`` is plain integer arithmetic on a handful of letters and runs on
the host; ``as_kmer_seq`` of a whole sequence is computed by the GPU encoder (kernel K5a).

:class:`KmerIndex` is the computation in the reference's SQLite-backed ``KmerIndex`` (``kmers.py:386-523``) without its
storage: ``index_kmers``, ``hits`` and ``kmers`` with the reference's arguments and return values, answered from the sorted
(k-mer, read, position) table of all indexed sequences in HBM (``include/pw_kmers.h``), and beside them what
``experiments/kmer_freq.py`` computes from such a table -- :meth:`KmerIndex.counts`, :meth:`KmerIndex.count` (batched
lookup), :meth:`KmerIndex.spectrum` (count of counts) and :meth:`KmerIndex.occurrences` (the per-position repeat profile
of a sequence).  :func:`kmer_spectrum` builds one from a read list in one call.  A database ``path``, masked indexing and
``KmerCache`` are storage or out of scope and are refused or absent.

``window`` (:class:`KmerIndex`, :func:`kmer_spectrum`) samples the table by WINDOW MINIMIZERS (``include/pw_kmers.h`` states the
rule): only the positions whose order value is the minimum of some window of ``window`` consecutive positions of their read are
rows, every query answers from those rows, and :attr:`KmerIndex.density` tells which share of the positions they are.
"""
import ctypes as C

import numpy as np

from .sequence import Alphabet, Sequence

DIGITS = '0123456789abcdefghijklmnopqrstuvwxyz'     # kmers.py:162: at most 36 letters


def check_limits(alphabet, wordlen):
    """The reference's limits (``kmers.py:262-271``): |alphabet| <= 36, wordlen < 31.5 on 64-bit."""
    assert isinstance(wordlen, int)
    assert isinstance(alphabet, Alphabet)
    assert len(alphabet) <= len(DIGITS), 'Maximum alphabet size of %d exceeded' % len(DIGITS)
    assert wordlen < (64 - 1) / 2., 'Maximum kmer length %d for %d-bit integers exceeded' % (wordlen, 64)
    assert len(alphabet) ** wordlen < 2 ** 62, 'alphabet size ** word length must stay below 2^62'


def check_window(window, name='window'):
    """A minimizer window of the Python calls: None or 0 (no sampling), or an integer in 1..128 (1 selects every position).
    Returns the integer the C calls take (0 for None); anything else is a ValueError."""
    if window is None:
        return 0
    if isinstance(window, bool) or not isinstance(window, (int, np.integer)) or not 0 <= int(window) <= 128:
        raise ValueError('%s is None or an integer in 1..128, not %r' % (name, window))
    return int(window)


def kmer_as_int(contents, alphabet):
    """Integer representation of a k-mer: its letters as digits in base ``len(alphabet)``."""
    assert isinstance(alphabet, Alphabet)
    v, L = 0, len(alphabet)
    for c in contents:
        v = v * L + int(c)
    return v


def mask_bits(mask):
    """A list of sets of letter indices -> the bit masks the C ABI takes."""
    assert all(isinstance(lets, set) for lets in mask)
    bits = []
    for lets in mask:
        b = 0
        for c in lets:
            b |= 1 << int(c)
        bits.append(b)
    return bits


def as_kmer_seq(seq, wordlen, mask=[]):
    """The k-mer at every position of ``seq`` as an integer, ``None`` where the set of letters of the k-mer
    equals one of the sets in ``mask`` (computed on the GPU)."""
    assert isinstance(seq, Sequence)
    from .seeds import _Index
    with _Index(seq, seq, wordlen, seq.alphabet, mask, self_comp=1) as idx:
        ks = idx.kmers(0)
    return [None if k < 0 else int(k) for k in ks]


class KmerIndex(object):
    """The k-mer table of a body of sequences on the device (``include/pw_kmers.h``), with the interface of the
    reference's ``KmerIndex`` (``kmers.py:386-523``) where it computes: the constructor's checks, :meth:`index_kmers`,
    :meth:`hits`, :meth:`kmers`.  Only ``path=':memory:'`` and an empty ``mask`` are taken: storage and masked indexing are
    not built.  The device table is rebuilt lazily, on the first query after the last :meth:`index_kmers`.

    ``strands='both'`` (with ``complement``: a table, or the ``mappings`` of ``Alphabet.transform``) adds, for every
    position, the k-mer of the reverse complement of the sequence: ``count(x) = n_f(x) + n_f(rc(x))``, so a k-mer that is its
    own reverse complement counts twice, and :meth:`hits` returns ``(seqid, pos, strand)`` with ``pos`` of a strand-1 hit
    in the frame of the reverse complement.

    ``window`` (None: every position, today's table): the table holds the window minimizers only (``pw_kmers_build_sampled``).
    The order value of a k-mer is a fixed 64-bit mix of its key with ``strands='+'`` and of the smaller of its key and its
    reverse complement's with ``strands='both'``; every position that attains the minimum of a window of ``window`` consecutive
    positions is a row.  Counts, hits, the spectrum and the occurrence profile are those of the sampled rows; positions in
    hits stay positions in the read.  :attr:`read_starts` and :meth:`occurrences` follow the sampled rows of every read."""

    def __init__(self, name='', alphabet=None, wordlen=None, path=':memory:', mask=[], device=0, strands='+', complement=None,
                 window=None):
        self.name = name
        assert all(isinstance(lets, set) for lets in mask)
        assert isinstance(wordlen, int)                   # kmers.py:263-271; the table itself takes alphabet ** wordlen == 2^62
        assert isinstance(alphabet, Alphabet)
        assert len(alphabet) <= len(DIGITS), 'Maximum alphabet size of %d exceeded' % len(DIGITS)
        assert wordlen < (64 - 1) / 2., 'Maximum kmer length %d for %d-bit integers exceeded' % (wordlen, 64)
        assert len(alphabet) ** wordlen <= 2 ** 62, 'alphabet size ** word length must not exceed 2^62'
        if path != ':memory:':
            raise ValueError("KmerIndex keeps its table on the device: only path=':memory:' is supported, not %r" % (path,))
        if mask:
            raise ValueError('KmerIndex does not support masked indexing: mask must be empty')
        if strands not in ('+', 'both'):
            raise ValueError("strands is '+' or 'both', not %r" % (strands,))
        self.window = check_window(window)
        self.mask, self.path, self.alphabet, self.wordlen, self.device, self.strands = mask, path, alphabet, wordlen, device, strands
        self._comp = None
        if strands == 'both':
            from .overlap import _complement
            self._comp = np.ascontiguousarray(_complement(complement, len(alphabet), alphabet), np.uint8)
        from . import _pwlib as W
        self._W, self._lib = W, W.load()
        self._seqids, self._reads = {}, []                # content_id -> seqid; the letters, seqid - 1 -> array
        self._dirty = True
        self._rstart = np.zeros(1, np.int64)
        self._handle = self._lib.pw_kmers_create(device, len(alphabet), wordlen)
        if not self._handle:
            raise RuntimeError('pw_kmers_create failed: ' + self._error())

    def _error(self):
        return (self._lib.pw_kmers_last_error() or b'').decode()

    def close(self):
        if getattr(self, '_handle', None):
            self._lib.pw_kmers_destroy(self._handle)
            self._handle = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        self.close()

    def index_kmers(self, seq):
        """Adds all k-mers of ``seq`` and returns its seqid (1, 2, ... as AUTOINCREMENT numbers them); a sequence whose
        ``content_id`` was indexed before returns its old seqid and adds nothing (``kmers.py:464-472``)."""
        assert isinstance(seq, Sequence) and seq.alphabet == self.alphabet
        seqid = self._seqids.get(seq.content_id)
        if seqid is None:
            self._reads.append(np.ascontiguousarray(seq.as_array(np.uint8)))
            seqid = self._seqids[seq.content_id] = len(self._reads)
            self._dirty = True
        return seqid

    def _add_arrays(self, reads):
        """The letters of a read list as they are (no content ids: equal reads stay two reads)."""
        for r in reads:
            self._reads.append(r.as_array(np.uint8) if isinstance(r, Sequence) else np.ascontiguousarray(r, np.uint8))
        self._dirty = True

    def _table(self):
        if not self._handle:
            raise ValueError('the KmerIndex is closed')
        if self._dirty:
            lens = np.array([len(a) for a in self._reads], np.int32)
            offs = np.zeros(len(lens) + 1, np.uint64)
            offs[1:] = np.cumsum(lens, dtype=np.uint64)
            arena = np.ascontiguousarray(np.concatenate(self._reads)) if self._reads else np.zeros(0, np.uint8)
            roff = np.ascontiguousarray(offs[:-1])
            W = self._W
            args = (self._handle, arena.ctypes.data, arena.size, roff.ctypes.data, lens.ctypes.data, len(lens),
                    W.PW_STRAND_BOTH if self.strands == 'both' else W.PW_STRAND_PLUS, None if self._comp is None else self._comp.ctypes.data)
            if self.window > 1:
                if self._lib.pw_kmers_build_sampled(*(args + (self.window, None))) != 0:
                    raise RuntimeError('pw_kmers_build_sampled failed: ' + self._error())
                starts = np.zeros(len(lens) + 1, np.uint64)
                if self._lib.pw_kmers_read_starts(self._handle, starts.ctypes.data) != 0:
                    raise RuntimeError('pw_kmers_read_starts failed: ' + self._error())
                self._rstart = starts.astype(np.int64)
            else:
                if self._lib.pw_kmers_build(*(args + (None,))) != 0:
                    raise RuntimeError('pw_kmers_build failed: ' + self._error())
                self._rstart = np.zeros(len(lens) + 1, np.int64)
                self._rstart[1:] = np.cumsum(np.maximum(lens.astype(np.int64) - self.wordlen + 1, 0))
            self._dirty = False
        return self._handle

    @property
    def num_entries(self):
        """Rows of the table."""
        return int(self._lib.pw_kmers_num_entries(self._table()))

    @property
    def num_positions(self):
        """Forward k-mer positions of the indexed sequences, sampled or not."""
        return int(self._lib.pw_kmers_num_positions(self._table()))

    @property
    def density(self):
        """Forward rows per forward position: 1.0 without a window, about ``2 / (window + 1)`` on random sequence; ``nan`` for an
        index without positions."""
        n = self.num_positions
        return float(self.read_starts[-1]) / n if n else float('nan')

    def rows(self):
        """``(keys uint64, hits uint64)`` of the whole table in table order: by (key, strand, read, pos), a hit is
        ``(read << 32) | (strand << 31) | pos``."""
        h = self._table()
        n = int(self._lib.pw_kmers_num_entries(h))
        keys, hits = np.zeros(n, np.uint64), np.zeros(n, np.uint64)
        if self._lib.pw_kmers_rows(h, keys.ctypes.data, hits.ctypes.data, n) != 0:
            raise RuntimeError('pw_kmers_rows failed: ' + self._error())
        return keys, hits

    @property
    def last_ms(self):
        """Device time of the last build or query (HIP events)."""
        return float(self._lib.pw_kmers_last_ms())

    def counts(self):
        """``(keys uint64 ascending, counts uint32)`` of the distinct k-mers."""
        h = self._table()
        n = int(self._lib.pw_kmers_num_distinct(h))
        if n < 0:
            raise RuntimeError('pw_kmers_num_distinct failed: ' + self._error())
        keys, cnt = np.zeros(n, np.uint64), np.zeros(n, np.uint32)
        if self._lib.pw_kmers_distinct(h, keys.ctypes.data, cnt.ctypes.data, n) != 0:
            raise RuntimeError('pw_kmers_distinct failed: ' + self._error())
        return keys, cnt

    def kmers(self):
        """All observed k-mers, ascending (``kmers.py:512-523``)."""
        return [int(k) for k in self.counts()[0]]

    def count(self, kmers):
        """Batched lookup: the count of every k-mer of ``kmers`` (any order, duplicates allowed), 0 where it is absent."""
        q = np.ascontiguousarray(kmers, np.uint64).reshape(-1)
        out = np.zeros(len(q), np.uint32)
        if self._lib.pw_kmers_lookup(self._table(), q.ctypes.data, len(q), out.ctypes.data) != 0:
            raise RuntimeError('pw_kmers_lookup failed: ' + self._error())
        return out

    def raw_hits(self, kmer):
        """The packed hits ``(read << 32) | (strand << 31) | pos`` of a k-mer, in table order (read = seqid - 1)."""
        h = self._table()
        n = int(self.count([kmer])[0])
        out, got = np.zeros(max(n, 1), np.uint64), C.c_int64(0)
        if self._lib.pw_kmers_hits(h, int(kmer), out.ctypes.data, n, C.byref(got)) != 0:
            raise RuntimeError('pw_kmers_hits failed: ' + self._error())
        return out[:got.value]

    def hits(self, kmer):
        """All hits of a k-mer as ``(seqid, pos)``, ascending (``kmers.py:497-510``); ``(seqid, pos, strand)`` with
        ``strands='both'``."""
        assert isinstance(kmer, (int, np.integer))
        raw = self.raw_hits(kmer)
        seqid, strand, pos = (raw >> np.uint64(32)).astype(np.int64) + 1, (raw >> np.uint64(31)) & np.uint64(1), raw & np.uint64(0x7fffffff)
        if self.strands == 'both':
            return sorted(zip(seqid.tolist(), pos.tolist(), strand.tolist()))
        return list(zip(seqid.tolist(), pos.tolist()))

    def spectrum(self, max_mult):
        """``hist`` (uint64, ``max_mult + 1`` entries): ``hist[m]`` distinct k-mers occur ``m`` times, ``hist[max_mult]`` of
        them ``max_mult`` times or more; ``hist[0] == 0``."""
        hist = np.zeros(int(max_mult) + 1 if 1 <= int(max_mult) <= 65536 else 1, np.uint64)
        if self._lib.pw_kmers_spectrum(self._table(), int(max_mult), hist.ctypes.data) != 0:
            raise RuntimeError('pw_kmers_spectrum failed: ' + self._error())
        return hist

    def all_occurrences(self):
        """``count(k-mer at (read, pos))`` for every forward position of every read, reads in index order (uint32); read ``r``
        (seqid ``r + 1``) starts at ``read_starts[r]``.  With a window: for every SAMPLED forward row, in ``(read, pos)`` order."""
        h = self._table()
        occ = np.zeros(int(self._rstart[-1]), np.uint32)
        if self._lib.pw_kmers_occurrences(h, occ.ctypes.data) != 0:
            raise RuntimeError('pw_kmers_occurrences failed: ' + self._error())
        return occ

    @property
    def read_starts(self):
        """The forward rows before every read (``len(reads) + 1`` entries); with a window, the sampled ones."""
        self._table()
        return self._rstart

    def occurrences(self, seqid):
        """The repeat profile of one sequence: how often the k-mer at each of its positions occurs in the whole index."""
        if not 1 <= seqid <= len(self._reads):
            raise KeyError('no sequence with seqid %r' % (seqid,))
        occ = self.all_occurrences()
        return occ[self._rstart[seqid - 1]:self._rstart[seqid]]


def kmer_spectrum(reads, wordlen, alphabet, strands='+', complement=None, device=0, window=None):
    """A :class:`KmerIndex` over ``reads`` (Sequences or letter arrays; equal reads stay separate reads, seqid = position in
    the list + 1), built in one device pass.  ``window``: the minimizer window of :class:`KmerIndex`."""
    idx = KmerIndex(alphabet=alphabet, wordlen=wordlen, device=device, strands=strands, complement=complement, window=window)
    idx._add_arrays(reads)
    return idx

"""The k-mer table on the device (include/pw_kmers.h) against the dense numpy reference tests/kmer_ref.py: every array the C
calls return is compared for equality -- the distinct keys and their counts, the hits of every k-mer in table order, batched
lookups, the spectrum at three clamps, the occurrence profile -- on the planted-repeat read sets, at table sizes around the
256-row block edge, at every key width, with odd alphabets and both strands; then the Python class and the refusals."""
import ctypes as C

import numpy as np
import pytest

from tests import kmer_ref as KR
from tests import wide_words as WW

pytestmark = pytest.mark.gpu

PLUS, BOTH = 1, 3


def _lib():
    from biseqt_amd import _pwlib as W
    return W.load()


def _err():
    return (_lib().pw_kmers_last_error() or b'').decode()


class Table(object):
    """The C calls, one handle."""

    def __init__(self, L, k):
        self.lib, self.L, self.k = _lib(), L, k
        self.h = self.lib.pw_kmers_create(0, L, k)
        assert self.h, _err()

    def build(self, reads, strands='+', comp=None):
        lens = np.array([len(r) for r in reads], np.int32)
        offs = np.zeros(len(reads) + 1, np.uint64)
        offs[1:] = np.cumsum(lens, dtype=np.uint64)
        arena = np.ascontiguousarray(np.concatenate([np.zeros(0, np.uint8)] + [np.asarray(r, np.uint8) for r in reads]))
        roff = np.ascontiguousarray(offs[:-1])
        comp = None if comp is None else np.ascontiguousarray(comp, np.uint8)
        return self.lib.pw_kmers_build(self.h, arena.ctypes.data, arena.size, roff.ctypes.data, lens.ctypes.data, len(reads),
                                       BOTH if strands == 'both' else PLUS, None if comp is None else comp.ctypes.data, None)

    def distinct(self):
        n = self.lib.pw_kmers_num_distinct(self.h)
        assert n >= 0, _err()
        keys, cnt = np.zeros(n, np.uint64), np.zeros(n, np.uint32)
        assert self.lib.pw_kmers_distinct(self.h, keys.ctypes.data, cnt.ctypes.data, n) == 0, _err()
        return keys, cnt

    def lookup(self, q):
        q = np.ascontiguousarray(q, np.uint64)
        out = np.full(len(q), 0xdeadbeef, np.uint32)
        assert self.lib.pw_kmers_lookup(self.h, q.ctypes.data, len(q), out.ctypes.data) == 0, _err()
        return out

    def hits(self, key, cap):
        out, n = np.zeros(max(cap, 1), np.uint64), C.c_int64(-1)
        rc = self.lib.pw_kmers_hits(self.h, int(key), out.ctypes.data, cap, C.byref(n))
        return rc, out[:max(min(n.value, cap), 0)], n.value

    def spectrum(self, max_mult):
        hist = np.full(max_mult + 1, 0xdeadbeef, np.uint64)
        assert self.lib.pw_kmers_spectrum(self.h, max_mult, hist.ctypes.data) == 0, _err()
        return hist

    def occurrences(self, n):
        occ = np.full(n, 0xdeadbeef, np.uint32)
        assert self.lib.pw_kmers_occurrences(self.h, occ.ctypes.data) == 0, _err()
        return occ

    def close(self):
        self.lib.pw_kmers_destroy(self.h)


def _check(reads, k, L, strands='+', comp=None):
    """Everything the C calls return for this read set equals the reference."""
    keys, hits = KR.table(reads, k, L, strands, comp)
    u, c = KR.counts(reads, k, L, strands, comp)
    t = Table(L, k)
    try:
        assert t.build(reads, strands, comp) == 0, _err()
        assert t.lib.pw_kmers_num_entries(t.h) == len(keys)
        assert t.lib.pw_kmers_num_distinct(t.h) == len(u)
        gk, gc = t.distinct()
        assert np.array_equal(gk, u) and np.array_equal(gc, c)
        got = [np.zeros(0, np.uint64)]
        for key, n in zip(u.tolist(), c.tolist()):
            rc, h, n_out = t.hits(key, n)
            assert rc == 0 and n_out == n, (key, _err())
            got.append(h)
        assert np.array_equal(np.concatenate(got), hits)
        top = L ** k - 1
        absent = [x for x in (0, 1, top, top - 1, int(u[len(u) // 2]) + 1 if len(u) else 5) if x not in set(u.tolist()) and 0 <= x <= top]
        q = np.array(u[::-1].tolist() + absent + [top + 1, 2 ** 64 - 1] + u[:2].tolist() + u[:1].tolist(), np.uint64)
        assert np.array_equal(t.lookup(q), KR.lookup(reads, k, L, q, strands, comp))
        assert len(t.lookup(np.zeros(0, np.uint64))) == 0
        biggest = int(c.max()) if len(c) else 1
        for max_mult in sorted({1, max(biggest - 1, 1), biggest, biggest + 1}):
            hist = t.spectrum(max_mult)
            assert np.array_equal(hist, KR.spectrum(c, max_mult)), max_mult
            assert hist[0] == 0 and int(hist.sum()) == len(u)
            if max_mult >= biggest:
                assert int((np.arange(max_mult + 1, dtype=np.uint64) * hist).sum()) == len(keys)
        want = KR.occurrences(reads, k, L, strands, comp)
        assert np.array_equal(t.occurrences(len(want)), want)
    finally:
        t.close()
    return u, c


@pytest.mark.parametrize('strands', ['+', 'both'])
@pytest.mark.parametrize('seed', KR.PLANTED_SEEDS)
def test_planted_repeat_sets(seed, strands):
    u, c = _check(KR.planted_reads(seed), KR.PLANTED_K, KR.PLANTED_L, strands, KR.DNA_COMPLEMENT)
    assert c.max() >= 39 and len(u) > 1000


def _homopolymers(runs, k):
    """Reads of one letter each: `runs` = [(letter, rows), ...] -> the table is those runs in letter order."""
    return [np.full(rows + k - 1, letter, np.uint8) for letter, rows in runs]


# rows -> reads (L = 4, k = 6): the runs of equal keys against the 256-row blocks of the run-head kernels
BLOCK_EDGE = {
    1: [(2, 1)],
    255: [(0, 100), (1, 100), (3, 55)],
    256: [(1, 128), (1, 128)],                       # one run covers the whole table: two homopolymers of one letter
    257: [(0, 250), (2, 7)],                         # the second run crosses the block edge at row 256
    513: [(0, 200), (0, 56), (1, 257)],              # the second run starts on the block edge and crosses the next one
}


@pytest.mark.parametrize('strands', ['+', 'both'])
@pytest.mark.parametrize('rows', sorted(BLOCK_EDGE))
def test_table_sizes_around_the_block_edge(rows, strands):
    reads = _homopolymers(BLOCK_EDGE[rows], 6) + [np.zeros(3, np.uint8), np.zeros(0, np.uint8)]     # (two reads without rows)
    u, c = _check(reads, 6, 4, strands, KR.DNA_COMPLEMENT)
    if strands == '+':
        assert int(c.sum()) == rows
        if rows == 256:
            assert len(u) == 1
        if rows in (257, 513):
            start = np.cumsum(c) - c
            assert any(s < 256 < s + n for s, n in zip(start, c)) or any(s == 256 for s in start)


@pytest.mark.parametrize('strands', ['+', 'both'])
@pytest.mark.parametrize('L,k', [(4, 15), (4, 16), (4, 31)], ids=['30-bit', '32-bit-first-8-byte-key', '2^62'])
def test_key_widths(L, k, strands):
    x = WW.basic(L, k)
    u, c = _check([x.S, x.T, x.S[:k - 1]], k, L, strands, KR.DNA_COMPLEMENT)
    assert int(u.max()) == L ** k - 1 and int(u.min()) == 0 and c.max() >= 2


def test_three_letters_with_a_fixed_point_and_thirty_six():
    rng = np.random.default_rng(5)
    comp3 = np.array([2, 1, 0], np.uint8)                                           # letter 1 is its own complement
    _check([rng.integers(0, 3, n).astype(np.uint8) for n in (300, 7, 150, 4)], 5, 3, 'both', comp3)
    comp36 = np.arange(36, dtype=np.uint8) ^ 1                                      # (0 1)(2 3) ... (34 35)
    reads = [rng.integers(0, 36, n).astype(np.uint8) for n in (200, 90)]
    reads.append(np.concatenate([reads[0][50:120], np.full(6, 35, np.uint8), np.zeros(6, np.uint8)]))
    _check(reads, 3, 36, 'both', comp36)
    _check(reads, 3, 36, '+')


def test_a_palindromic_kmer_counts_twice_on_both_strands():
    acgt = np.array([0, 1, 2, 3], np.uint8)                                         # ACGT is its own reverse complement
    reads = [np.concatenate([[0, 0], acgt, [0, 0, 1], acgt, [3]]).astype(np.uint8), np.concatenate([[2, 2], acgt]).astype(np.uint8)]
    key = 0 * 64 + 1 * 16 + 2 * 4 + 3
    t = Table(4, 4)
    try:
        assert t.build(reads, '+') == 0
        assert t.lookup([key]).tolist() == [3]
        assert t.build(reads, 'both', KR.DNA_COMPLEMENT) == 0
        assert t.lookup([key]).tolist() == [6]
        rc, hits, n = t.hits(key, 6)
        assert rc == 0 and n == 6 and ((hits >> np.uint64(31)) & np.uint64(1)).tolist() == [0, 0, 0, 1, 1, 1]
    finally:
        t.close()
    _check(reads, 4, 4, 'both', KR.DNA_COMPLEMENT)


def test_hits_with_too_small_a_capacity_are_refused_not_truncated():
    reads = KR.planted_reads(0)
    u, c = KR.counts(reads, KR.PLANTED_K, KR.PLANTED_L)
    key, n = int(u[np.argmax(c)]), int(c.max())
    t = Table(KR.PLANTED_L, KR.PLANTED_K)
    try:
        assert t.build(reads) == 0
        rc, hits, n_out = t.hits(key, n - 1)
        assert rc == -1 and n_out == n
        assert _err() == 'pw_kmers_hits: the k-mer has %d hits (capacity %d)' % (n, n - 1)
        rc, hits, n_out = t.hits(key, n)
        assert rc == 0 and len(hits) == n
        rc, hits, n_out = t.hits(4 ** KR.PLANTED_K, 0)                              # absent: no hits, nothing to refuse
        assert rc == 0 and n_out == 0
    finally:
        t.close()


def test_a_handle_is_rebuilt_and_an_empty_table_answers():
    t = Table(4, 8)
    try:
        assert t.lib.pw_kmers_num_entries(t.h) == -1
        assert t.lib.pw_kmers_num_distinct(t.h) == -1 and _err() == 'pw_kmers_num_distinct before a successful pw_kmers_build'
        assert t.build([np.zeros(5, np.uint8), np.zeros(0, np.uint8)]) == 0
        assert t.lib.pw_kmers_num_entries(t.h) == 0 and t.lib.pw_kmers_num_distinct(t.h) == 0
        assert t.lookup([0, 7]).tolist() == [0, 0] and t.spectrum(4).tolist() == [0] * 5
        assert t.build([]) == 0 and t.lib.pw_kmers_num_entries(t.h) == 0
        reads = KR.planted_reads(1)
        assert t.build(reads) == 0
        u, c = KR.counts(reads, 8, 4)
        gk, gc = t.distinct()
        assert np.array_equal(gk, u) and np.array_equal(gc, c)
        assert t.build(reads[:3], 'both', KR.DNA_COMPLEMENT) == 0                 # a smaller table in the same buffers
        u, c = KR.counts(reads[:3], 8, 4, 'both', KR.DNA_COMPLEMENT)
        gk, gc = t.distinct()
        assert np.array_equal(gk, u) and np.array_equal(gc, c)
    finally:
        t.close()


def test_refusals_by_message():
    lib = _lib()
    for L, k, msg in ((0, 5, 'alphabet_len 1..36, wordlen 1..31'), (37, 5, 'alphabet_len 1..36, wordlen 1..31'),
                      (4, 32, 'alphabet_len 1..36, wordlen 1..31'), (4, 0, 'alphabet_len 1..36, wordlen 1..31'),
                      (5, 27, 'alphabet_len ^ wordlen must be below 2^62')):
        assert not lib.pw_kmers_create(0, L, k) and _err() == msg
    t = Table(4, 8)
    try:
        reads = [np.arange(20, dtype=np.uint8) % 4]
        assert t.build(reads, 'both', None) == -1
        assert _err() == 'complement must be alphabet_len bytes with complement[complement[c]] == c for every letter'
        assert t.build(reads, 'both', [1, 2, 0, 3]) == -1
        assert _err() == 'complement must be alphabet_len bytes with complement[complement[c]] == c for every letter'
        assert t.build([np.array([0, 1, 4, 2, 0, 0, 0, 0, 0], np.uint8)]) == -1 and _err() == 'letter outside the alphabet'
        arena = np.zeros(16, np.uint8)
        off, ln = np.array([8], np.uint64), np.array([9], np.int32)
        assert lib.pw_kmers_build(t.h, arena.ctypes.data, 16, off.ctypes.data, ln.ctypes.data, 1, PLUS, None, None) == -1
        assert _err() == 'a read lies outside the arena'
        assert lib.pw_kmers_build(t.h, arena.ctypes.data, 16, off.ctypes.data, ln.ctypes.data, 1, 2, None, None) == -1
        assert _err() == 'strands must be 1 (+) or 3 (both)'
        assert lib.pw_kmers_build(t.h, arena.ctypes.data, 16, None, None, 1, PLUS, None, None) == -1 and _err() == 'bad arguments'
        assert lib.pw_kmers_lookup(t.h, None, 0, None) == -1 and _err() == 'pw_kmers_lookup before a successful pw_kmers_build'
        assert t.build(reads) == 0
        hist = np.zeros(4, np.uint64)
        for bad in (0, 65537):
            assert lib.pw_kmers_spectrum(t.h, bad, hist.ctypes.data) == -1 and _err() == 'max_mult must be 1..65536'
        keys, cnt = np.zeros(1, np.uint64), np.zeros(1, np.uint32)
        assert lib.pw_kmers_distinct(t.h, keys.ctypes.data, cnt.ctypes.data, 1) == -1 and _err() == 'pw_kmers_distinct: capacity too small'
    finally:
        t.close()


def test_spectrum_beyond_the_lds_bins():
    """A multiplicity above the 4096 bins a workgroup keeps in LDS goes to the histogram directly: one homopolymer run of 5000
    rows beside a few hundred singletons, clamped above, at and below it."""
    rng = np.random.default_rng(9)
    reads = [np.full(5000 + 11, 2, np.uint8), rng.integers(0, 4, 300).astype(np.uint8)]
    _, c = KR.counts(reads, 12, 4)
    assert c.max() >= 5000
    t = Table(4, 12)
    try:
        assert t.build(reads) == 0
        for max_mult in (4095, 4096, 4097, int(c.max()), 65536):
            assert np.array_equal(t.spectrum(max_mult), KR.spectrum(c, max_mult)), max_mult
    finally:
        t.close()


# ---- the Python class ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('wordlen', [3, 13])
def test_index_kmers(wordlen):
    """The assertions of the reference's tests/test_kmers.py::test_index_kmers, and the seqids of AUTOINCREMENT."""
    from biseqt_amd.kmers import KmerIndex, as_kmer_seq
    from biseqt_amd.sequence import Alphabet, Sequence
    A = Alphabet('ACGT')
    rng = np.random.default_rng(wordlen)
    S = Sequence(A, tuple(rng.integers(0, 4, 50).tolist()))
    with KmerIndex(path=':memory:', alphabet=A, wordlen=wordlen) as index:
        seqid = index.index_kmers(S)
        assert seqid == 1
        kmers = index.kmers()
        assert kmers == sorted(set(as_kmer_seq(S, wordlen)))
        assert sum(len(index.hits(kmer)) for kmer in kmers) == len(S) - wordlen + 1
        assert seqid == index.index_kmers(S), 'same sequence should not be indexed twice'
        T = Sequence(A, tuple(rng.integers(0, 4, 10).tolist()))
        assert index.index_kmers(T) == 2
        assert index.index_kmers(Sequence(A, tuple(S.as_array(np.uint8).tolist()))) == 1
        reads = [S.as_array(np.uint8), T.as_array(np.uint8)]
        u, c = KR.counts(reads, wordlen, 4)
        keys, cnt = index.counts()
        assert np.array_equal(keys, u) and np.array_equal(cnt, c) and index.num_entries == int(c.sum())
        hits = KR.table(reads, wordlen, 4)[1]
        want = [(int(h >> np.uint64(32)) + 1, int(h & np.uint64(0x7fffffff))) for h in hits]
        assert [hit for kmer in index.kmers() for hit in index.hits(kmer)] == want
        assert np.array_equal(index.count([int(u[0]), 4 ** wordlen - 1 if 4 ** wordlen - 1 not in u else int(u[0])]),
                              KR.lookup(reads, wordlen, 4, [int(u[0]), 4 ** wordlen - 1 if 4 ** wordlen - 1 not in u else int(u[0])]))
        assert np.array_equal(index.spectrum(3), KR.spectrum(c, 3))
        occ = KR.occurrences(reads, wordlen, 4)
        assert np.array_equal(index.occurrences(1), occ[:50 - wordlen + 1]) and np.array_equal(index.occurrences(2), occ[50 - wordlen + 1:])
    with pytest.raises(ValueError):
        index.kmers()                                                               # closed


def test_constructor_checks_and_kmer_spectrum():
    from biseqt_amd.kmers import KmerIndex, kmer_spectrum
    from biseqt_amd.sequence import Alphabet
    with pytest.raises(AssertionError):
        KmerIndex(':memory:', wordlen=32, alphabet=Alphabet('ACGT'))                # the reference's tests/test_kmers.py:11-20
    with pytest.raises(AssertionError):
        KmerIndex(':memory:', wordlen=5, alphabet=Alphabet(str(i) for i in range(37)))
    with pytest.raises(ValueError, match="only path=':memory:'"):
        KmerIndex(path='/tmp/kmers.db', wordlen=5, alphabet=Alphabet('ACGT'))
    with pytest.raises(ValueError, match='masked indexing'):
        KmerIndex(wordlen=5, alphabet=Alphabet('ACGT'), mask=[{0}])
    reads = KR.planted_reads(2)
    for strands in ('+', 'both'):
        with kmer_spectrum(reads, 8, Alphabet('ACGT'), strands=strands, complement=[('A', 'T'), ('C', 'G')]) as index:
            u, c = KR.counts(reads, 8, 4, strands, KR.DNA_COMPLEMENT)
            keys, cnt = index.counts()
            assert np.array_equal(keys, u) and np.array_equal(cnt, c)
            assert np.array_equal(index.spectrum(50), KR.spectrum(c, 50))
            assert np.array_equal(index.all_occurrences(), KR.occurrences(reads, 8, 4, strands, KR.DNA_COMPLEMENT))
            assert index.read_starts.tolist() == np.concatenate([[0], np.cumsum([max(len(r) - 7, 0) for r in reads])]).tolist()

"""The sampled k-mer table on the device (pw_kmers_build_sampled, ``KmerIndex(window=...)``) against the dense numpy oracle
tests/minimizer_ref.py: ``rows()``, ``counts()``, ``read_starts`` and ``all_occurrences()`` must equal it exactly -- at every
window that takes another path through the kernel (1, 2, 3, 8, 16, 128 and one above every read's positions), at every key
width, on both orders (plain for ``'+'``, canonical for ``'both'``), on reads whose halos cross read boundaries and tile
edges, with ties (a homopolymer, a tandem repeat, a reverse-palindromic stretch).  Window 1 must equal an unsampled build in
every output."""
import ctypes as C

import numpy as np
import pytest

from tests import kmer_ref as KR
from tests import minimizer_ref as MR

pytestmark = pytest.mark.gpu

DIGITS = '0123456789abcdefghijklmnopqrstuvwxyz'
COMP36 = np.arange(36, dtype=np.uint8) ^ 1
WIDTHS = [(4, 3), (4, 15), (4, 16), (4, 31), (36, 1)]
WINDOWS = [1, 2, 3, 8, 16, 128]


def _alphabet(L):
    from biseqt_amd.sequence import Alphabet
    return Alphabet('ACGT' if L == 4 else DIGITS[:L])


def _comp(L):
    return KR.DNA_COMPLEMENT if L == 4 else COMP36


def _index(reads, k, L, strands, window):
    from biseqt_amd.kmers import kmer_spectrum
    return kmer_spectrum(reads, k, _alphabet(L), strands=strands, complement=_comp(L) if strands == 'both' else None, window=window)


def _check(reads, k, L, w, strands):
    comp = _comp(L)
    keys, hits = MR.table(reads, k, L, w, strands, comp)
    u, c = MR.counts(reads, k, L, w, strands, comp)
    starts = MR.read_starts(reads, k, L, w, strands, comp)
    with _index(reads, k, L, strands, w) as idx:
        gk, gh = idx.rows()
        assert np.array_equal(gk, keys) and np.array_equal(gh, hits), (np.flatnonzero(gk != keys)[:5] if len(gk) == len(keys) else (len(gk), len(keys)))
        assert idx.num_entries == len(keys) and idx.num_positions == MR.num_positions(reads, k)
        du, dc = idx.counts()
        assert np.array_equal(du, u) and np.array_equal(dc, c)
        assert idx.read_starts.tolist() == starts.tolist()
        assert np.array_equal(idx.all_occurrences(), MR.occurrences(reads, k, L, w, strands, comp))
        assert idx.density == starts[-1] / MR.num_positions(reads, k)
        # the other queries answer from the sampled table too
        q = np.concatenate([u[:3], u[-3:], np.array([L ** k - 1, 0, L ** k], np.uint64)])
        table_of = dict(zip(u.tolist(), c.tolist()))
        assert idx.count(q).tolist() == [table_of.get(int(x), 0) for x in q]
        assert np.array_equal(idx.spectrum(5), KR.spectrum(c, 5))
        top = int(u[np.argmax(c)])
        assert np.array_equal(idx.raw_hits(top), hits[keys == np.uint64(top)])
        for r in (1, 3, len(reads)):                                                  # seqids
            assert np.array_equal(idx.occurrences(r), idx.all_occurrences()[starts[r - 1]:starts[r]])
    return len(keys)


@pytest.mark.parametrize('L,k', WIDTHS, ids=['6-bit', '30-bit', '32-bit-first-8-byte-key', '2^62', '36-letters'])
@pytest.mark.parametrize('w', WINDOWS)
def test_sampled_table_equals_the_oracle(w, L, k):
    reads = MR.edge_reads(L, k, w, _comp(L))
    for strands in ('+', 'both'):
        rows = _check(reads, k, L, w, strands)
        full = MR.num_positions(reads, k) * (2 if strands == 'both' else 1)
        assert rows == full if w == 1 else rows < full


def test_a_window_above_every_read_s_positions():
    """ww = n for every read: the rows are the minima of whole reads (all of them where they tie)."""
    rng = np.random.default_rng(11)
    k = 6
    reads = [rng.integers(0, 4, n + k - 1).astype(np.uint8) for n in (1, 5, 40, 100, 127)] + [np.zeros(0, np.uint8), np.full(30, 2, np.uint8)]
    for strands in ('+', 'both'):
        _check(reads, k, 4, 128, strands)
    with _index(reads, k, 4, '+', 128) as idx:
        minima = [int((h == h.min()).sum()) if len(h) else 0 for h in (MR.order_values(r, k, 4) for r in reads)]
        assert np.diff(idx.read_starts).tolist() == minima and minima[-2:] == [0, 25] and minima[0] == 1


def _c_build(lib, h, reads, strands, comp, window):
    lens = np.array([len(r) for r in reads], np.int32)
    offs = np.zeros(len(reads) + 1, np.uint64)
    offs[1:] = np.cumsum(lens, dtype=np.uint64)
    arena = np.ascontiguousarray(np.concatenate([np.zeros(0, np.uint8)] + [np.asarray(r, np.uint8) for r in reads]))
    roff = np.ascontiguousarray(offs[:-1])
    comp = None if comp is None else np.ascontiguousarray(comp, np.uint8)
    args = (h, arena.ctypes.data, arena.size, roff.ctypes.data, lens.ctypes.data, len(reads), 3 if strands == 'both' else 1,
            None if comp is None else comp.ctypes.data)
    return lib.pw_kmers_build(*(args + (None,))) if window is None else lib.pw_kmers_build_sampled(*(args + (window, None)))


def _c_outputs(lib, h, n_reads):
    n = lib.pw_kmers_num_entries(h)
    keys, hits = np.full(n, 7, np.uint64), np.full(n, 7, np.uint64)
    assert lib.pw_kmers_rows(h, keys.ctypes.data, hits.ctypes.data, n) == 0
    d = lib.pw_kmers_num_distinct(h)
    u, c = np.zeros(d, np.uint64), np.zeros(d, np.uint32)
    assert lib.pw_kmers_distinct(h, u.ctypes.data, c.ctypes.data, d) == 0
    starts = np.full(n_reads + 1, 7, np.uint64)
    assert lib.pw_kmers_read_starts(h, starts.ctypes.data) == 0
    occ = np.full(int(starts[-1]), 7, np.uint32)
    assert lib.pw_kmers_occurrences(h, occ.ctypes.data) == 0
    hist = np.zeros(9, np.uint64)
    assert lib.pw_kmers_spectrum(h, 8, hist.ctypes.data) == 0
    return [n, lib.pw_kmers_num_positions(h), d] + [x.tobytes() for x in (keys, hits, u, c, starts, occ, hist)]


@pytest.mark.parametrize('strands', ['+', 'both'])
def test_window_one_is_the_unsampled_build_in_every_output(strands):
    from biseqt_amd import _pwlib as W
    lib = W.load()
    reads = KR.planted_reads(0)
    h = lib.pw_kmers_create(0, 4, 8)
    try:
        assert _c_build(lib, h, reads, strands, KR.DNA_COMPLEMENT, None) == 0
        plain = _c_outputs(lib, h, len(reads))
        assert _c_build(lib, h, reads, strands, KR.DNA_COMPLEMENT, 5) == 0            # (a sampled table in between)
        assert _c_outputs(lib, h, len(reads))[0] < plain[0]
        assert _c_build(lib, h, reads, strands, KR.DNA_COMPLEMENT, 1) == 0
        assert _c_outputs(lib, h, len(reads)) == plain
        keys, hits = KR.table(reads, 8, 4, strands, KR.DNA_COMPLEMENT)
        assert plain[3] == keys.tobytes() and plain[4] == hits.tobytes()              # pw_kmers_rows on an unsampled table
        assert plain[1] == 12 * 393 and plain[7] == np.concatenate([[0], np.cumsum([393] * 12 + [0, 0])]).astype(np.uint64).tobytes()
    finally:
        lib.pw_kmers_destroy(h)
    with _index(reads, 8, 4, strands, 1) as one, _index(reads, 8, 4, strands, None) as none:
        assert all(np.array_equal(x, y) for x, y in zip(one.rows() + one.counts(), none.rows() + none.counts()))
        assert np.array_equal(one.all_occurrences(), none.all_occurrences()) and one.read_starts.tolist() == none.read_starts.tolist()
        assert one.density == none.density == 1.0


def test_refusals_and_a_rebuilt_handle():
    from biseqt_amd import _pwlib as W
    lib = W.load()
    err = lambda: (lib.pw_kmers_last_error() or b'').decode()
    reads = KR.planted_reads(2)
    h = lib.pw_kmers_create(0, 4, 8)
    try:
        assert lib.pw_kmers_num_positions(h) == -1
        for bad in (0, -3, 129):
            assert _c_build(lib, h, reads, '+', None, bad) == -1 and err() == 'window must be 1..128'
        assert lib.pw_kmers_rows(h, None, None, 0) == -1 and err() == 'pw_kmers_rows before a successful pw_kmers_build'
        assert lib.pw_kmers_read_starts(h, None) == -1 and err() == 'pw_kmers_read_starts before a successful pw_kmers_build'
        assert _c_build(lib, h, reads, 'both', None, 4) == -1
        assert err() == 'complement must be alphabet_len bytes with complement[complement[c]] == c for every letter'
        assert _c_build(lib, h, reads, 'both', KR.DNA_COMPLEMENT, 128) == 0
        n = lib.pw_kmers_num_entries(h)
        keys, hits = np.zeros(n, np.uint64), np.zeros(n, np.uint64)
        assert lib.pw_kmers_rows(h, keys.ctypes.data, hits.ctypes.data, n - 1) == -1 and err() == 'pw_kmers_rows: capacity too small'
        assert lib.pw_kmers_rows(h, keys.ctypes.data, hits.ctypes.data, n) == 0
        want = MR.table(reads, 8, 4, 128, 'both', KR.DNA_COMPLEMENT)
        assert np.array_equal(keys, want[0]) and np.array_equal(hits, want[1])
        # a sampled table without rows, then a larger one in the same handle
        assert _c_build(lib, h, [np.zeros(5, np.uint8), np.zeros(0, np.uint8)], '+', None, 7) == 0
        starts = np.full(3, 9, np.uint64)
        assert lib.pw_kmers_num_entries(h) == 0 and lib.pw_kmers_num_positions(h) == 0
        assert lib.pw_kmers_read_starts(h, starts.ctypes.data) == 0 and starts.tolist() == [0, 0, 0]
        assert _c_build(lib, h, reads, '+', None, 3) == 0
        n = lib.pw_kmers_num_entries(h)
        keys, hits = np.zeros(n, np.uint64), np.zeros(n, np.uint64)
        assert lib.pw_kmers_rows(h, keys.ctypes.data, hits.ctypes.data, n) == 0
        want = MR.table(reads, 8, 4, 3, '+')
        assert np.array_equal(keys, want[0]) and np.array_equal(hits, want[1])
        got = C.c_int64(-1)
        assert lib.pw_kmers_hits(h, int(keys[0]), hits.ctypes.data, n, C.byref(got)) == 0 and got.value == int((want[0] == want[0][0]).sum())
    finally:
        lib.pw_kmers_destroy(h)

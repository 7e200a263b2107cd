"""Minimizer-sampled all-pairs overlap discovery (pw_overlap_all_pairs_sampled, ``minimizer_window``) against
tests/minimizer_ref.py: on the planted-repeat read sets the listed pairs, their order, the strand column, every field of every
record and all stats equal ``sampled_join`` -- at three windows, every strand selection, with and without the occurrence cap,
sharded and unsharded; window None, 0 and 1 are today's calls field for field; reads cut error-free from one genome are found
wherever they overlap by ``w + k - 1`` letters, with the true diagonal inside the band, and align clean."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import kmer_ref as KR
from tests import minimizer_ref as MR

pytestmark = pytest.mark.gpu

K, L = KR.PLANTED_K, KR.PLANTED_L
STRANDS = ('+', '-', 'both')
WINDOWS = (2, 5, 12)
CAPS = (0, 7)


def _fields():
    from biseqt_amd.overlap import BAND_DTYPE
    return [name for name in BAND_DTYPE.names if name != 'pad_']


@functools.lru_cache(maxsize=None)
def _reads(seed):
    return KR.planted_reads(seed)


@functools.lru_cache(maxsize=None)
def _ref(seed, w, max_occ, strands, rank=0, world=1):
    reads = _reads(seed)
    join = MR.sampled_join(reads, K, L, w, max_occ, strands, KR.DNA_COMPLEMENT, rank, world)
    recs = [KR.band_record(d, len(reads[a]), len(reads[b]), K, L) for (a, b, _), d in join.pairs.items()]
    return join, recs


def _raw(seed, strands, **kw):
    from biseqt_amd.overlap import raw_all_pairs
    stats = {}
    out = raw_all_pairs(_reads(seed), K, L, KR.G_MAX, KR.SENSITIVITY, strands=strands, complement=KR.DNA_COMPLEMENT, with_strand=True,
                        stats=stats, **kw)
    return out[0], out[1], out[2], stats


def _check(seed, w, max_occ, strands, got, rank=0, world=1):
    pairs, flags, recs, stats = got
    join, want = _ref(seed, w, max_occ, strands, rank, world)
    assert [(int(a), int(b), int(f)) for (a, b), f in zip(pairs.tolist(), flags.tolist())] == list(join.pairs)
    bad = {}
    for key, rec, o in zip(join.pairs, recs, want):
        diff = {f: (rec[f].item(), o[f]) for f in _fields() if rec[f].item() != o[f]}
        if diff:
            bad[key] = diff
    assert not bad, bad
    assert stats == join.stats


@pytest.mark.parametrize('strands', STRANDS)
@pytest.mark.parametrize('max_occ', CAPS)
@pytest.mark.parametrize('w', WINDOWS)
@pytest.mark.parametrize('seed', KR.PLANTED_SEEDS)
def test_sampled_records_equal_the_reference(seed, w, max_occ, strands):
    _check(seed, w, max_occ, strands, _raw(seed, strands, minimizer_window=w, max_kmer_occ=max_occ))


@pytest.mark.parametrize('strands', STRANDS)
def test_the_cap_counts_the_sampled_table(strands):
    """occ(x) under a window is count(x) of a sampled k-mer table with the same strands and window."""
    from biseqt_amd.kmers import kmer_spectrum
    from biseqt_amd.sequence import Alphabet
    w, max_occ = 5, 7
    got = _raw(1, strands, minimizer_window=w, max_kmer_occ=max_occ)
    table_strands = '+' if strands == '+' else 'both'
    with kmer_spectrum(_reads(1), K, Alphabet('ACGT'), strands=table_strands, complement=KR.DNA_COMPLEMENT, window=w) as idx:
        _, c = idx.counts()
        assert got[3]['entries'] == idx.num_entries == int(c.sum())
        assert got[3]['masked_entries'] == int(c[c > max_occ].sum()) > 0 and got[3]['distinct_masked'] == int((c > max_occ).sum())
        assert got[3]['sampled'] == idx.read_starts[-1] and got[3]['positions'] == idx.num_positions


@pytest.mark.parametrize('strands', STRANDS)
@pytest.mark.parametrize('max_occ', CAPS)
def test_none_zero_and_one_are_today_s_call(max_occ, strands):
    from biseqt_amd import _pwlib as W
    from biseqt_amd.overlap import BAND_DTYPE, _band_coeffs, raw_all_pairs
    kw = dict(strands=strands, complement=KR.DNA_COMPLEMENT, max_kmer_occ=max_occ)
    plain_stats = {}
    plain = raw_all_pairs(_reads(0), K, L, KR.G_MAX, KR.SENSITIVITY, stats=plain_stats, **kw)
    for window in (None, 0, 1):
        stats = {}
        got = raw_all_pairs(_reads(0), K, L, KR.G_MAX, KR.SENSITIVITY, minimizer_window=window, stats=stats, **kw)
        assert len(got) == len(plain) and all(x.tobytes() == y.tobytes() for x, y in zip(got[:-1], plain[:-1]))
        assert stats == plain_stats
    # the C entry point with window 0 or 1 is the capped call bit for bit; the sample stats then report no sampling
    lib = W.load()
    reads = _reads(0)
    lens = np.array([len(r) for r in reads], np.int32)
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    arena, roff = np.ascontiguousarray(np.concatenate(reads)), np.ascontiguousarray(offs[:-1])
    out = {}
    for window in (None, 0, 1):
        pa, pb, ps, recs = np.zeros(200, np.int32), np.zeros(200, np.int32), np.zeros(200, np.uint8), np.zeros(200, BAND_DTYPE)
        n, cs, ss = C.c_int64(0), W.pw_overlap_cap_stats(1, 2, 3, 4, 5), W.pw_overlap_sample_stats(6, 7)
        args = [0, arena.ctypes.data, arena.size, roff.ctypes.data, lens.ctypes.data, len(reads), L, K] + \
            list(_band_coeffs(KR.G_MAX, KR.SENSITIVITY, L, K)) + \
            [KR.DNA_COMPLEMENT.ctypes.data, {'+': 1, '-': 2, 'both': 3}[strands], 0, 1, 200, pa.ctypes.data, pb.ctypes.data, ps.ctypes.data,
             recs.ctypes.data, C.byref(n), max_occ, C.byref(cs)]
        rc = lib.pw_overlap_all_pairs_capped(*args) if window is None else lib.pw_overlap_all_pairs_sampled(*(args + [window, C.byref(ss)]))
        assert rc == 0, lib.pw_overlap_last_error()
        out[window] = (n.value, pa.tobytes(), pb.tobytes(), ps.tobytes(), recs.tobytes(), [getattr(cs, f) for f, _ in cs._fields_])
        if window is not None:
            assert (ss.positions, ss.sampled) == (12 * 393, 12 * 393)
    assert out[None] == out[0] == out[1] and out[None][0] > 0
    for bad in (-1, 129):
        assert lib.pw_overlap_all_pairs_sampled(*(args + [bad, None])) == -1
        assert lib.pw_overlap_last_error() == b'window must be 0..128'


@pytest.mark.parametrize('strands', STRANDS)
@pytest.mark.parametrize('world', [2, 3])
def test_sharded_ranks_add_up_to_the_unsharded_call(world, strands):
    seed, w, max_occ = 1, 5, 7
    whole = _raw(seed, strands, minimizer_window=w, max_kmer_occ=max_occ)
    parts = [_raw(seed, strands, minimizer_window=w, max_kmer_occ=max_occ, rank=rank, world=world) for rank in range(world)]
    for rank, part in enumerate(parts):
        _check(seed, w, max_occ, strands, part, rank, world)
        assert all(int(a) % world == rank for a in part[0][:, 0])
        for f in ('entries', 'masked_entries', 'distinct_masked', 'positions', 'sampled', 'density'):   # over the whole read set
            assert part[3][f] == whole[3][f]
    for f in ('seeds_kept', 'seeds_dropped'):
        assert sum(part[3][f] for part in parts) == whole[3][f]
    pairs = np.concatenate([p[0] for p in parts])
    flags = np.concatenate([p[1] for p in parts])
    recs = np.concatenate([p[2] for p in parts])
    order = np.lexsort((flags, pairs[:, 1], pairs[:, 0]))
    assert pairs[order].tobytes() == whole[0].tobytes() and flags[order].tobytes() == whole[1].tobytes()
    assert recs[order].tobytes() == whole[2].tobytes()


def test_plain_call_without_the_strand_column():
    from biseqt_amd.overlap import raw_all_pairs
    stats = {}
    pairs, recs, ms = raw_all_pairs(_reads(2), K, L, KR.G_MAX, KR.SENSITIVITY, minimizer_window=5, stats=stats)
    join, want = _ref(2, 5, 0, '+')
    assert [tuple(p) + (0,) for p in pairs.tolist()] == list(join.pairs) and ms > 0
    assert [r['n_seeds'].item() for r in recs] == [o['n_seeds'] for o in want]
    assert stats == join.stats and 0.3 < stats['density'] < 0.4


def test_overlapping_reads_are_found_with_the_true_diagonal_in_the_band_and_align_clean():
    """The guarantee (fixture confirmed on the oracle in tests/test_minimizer_ref.py): 10 reads of 400 letters cut error-free
    from one genome, every other one reverse-complemented, k = 8, w = 10.  Every pair that overlaps by at least w + k - 1 = 17
    letters is listed on the right strand with the true diagonal in [d_best - r_best, d_best + r_best]; overlap_all_pairs
    followed by overlap_alignments re-scores clean on those pairs, and the long overlaps come back as all matches."""
    from biseqt_amd import verify
    from biseqt_amd.overlap import overlap_all_pairs, overlap_alignments, raw_all_pairs
    from biseqt_amd.sequence import Alphabet
    k, w = MR.GUARANTEE_K, MR.GUARANTEE_W
    reads, starts, flipped = MR.guarantee_reads()
    truth = MR.guarantee_truth(starts, flipped, w + k - 1)
    pairs, flags, recs, _ = raw_all_pairs(reads, k, 4, KR.G_MAX, KR.SENSITIVITY, strands='both', complement=KR.DNA_COMPLEMENT,
                                          minimizer_window=w)
    listed = {(int(a), int(b), int(f)): r for (a, b), f, r in zip(pairs.tolist(), flags.tolist(), recs)}
    join = MR.sampled_join(reads, k, 4, w, 0, 'both', KR.DNA_COMPLEMENT)
    assert list(listed) == list(join.pairs)
    for (a, b), (strand, d) in truth.items():
        r = listed[(a, b, strand)]
        assert r['d_best'] - r['r_best'] <= d <= r['d_best'] + r['r_best'], (a, b, d, r)
    A = Alphabet('ACGT')
    stats = {}
    bands = overlap_all_pairs(reads, k, A, KR.G_MAX, KR.SENSITIVITY, strands='both', complement=[('A', 'T'), ('C', 'G')],
                              minimizer_window=w, stats=stats)
    assert stats['fallback_pairs'] == 0 and stats['positions'] == 10 * 393 and stats['sampled'] == join.stats['sampled']
    assert 0 < stats['density'] == join.stats['density'] < .3
    keys = [(a, b, '-' if s else '+') for (a, b), (s, _) in truth.items()]
    assert all(key in bands for key in keys)
    alns = overlap_alignments(reads, [key[:2] for key in keys], [bands[key] for key in keys], A, strands=[key[2] for key in keys],
                              complement=[('A', 'T'), ('C', 'G')])
    n_long = 0
    for (a, b, s), aln in zip(keys, alns):
        assert aln is not None and aln['strand'] == s, (a, b, s)
        T = MR.revcomp(reads[b], KR.DNA_COMPLEMENT) if s == '-' else reads[b]
        sc, ex, ey, ok = verify.rescore(reads[a], T, aln['transcript'], aln['origin_start'], aln['mutant_start'], 1, -3, -5, -2)
        assert ok and sc == aln['score'], (a, b, s, sc, aln['score'])
        ov = 400 - abs(starts[a] - starts[b])
        if ov >= 100:
            tx = aln['transcript'] if isinstance(aln['transcript'], str) else bytes(aln['transcript']).decode()
            assert tx == 'M' * ov and aln['score'] == ov, (a, b, s, ov)
            assert aln['origin_start'] - aln['mutant_start'] == truth[(a, b)][1]
            n_long += 1
    assert n_long >= 5

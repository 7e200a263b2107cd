"""The occurrence cap of the all-pairs join (pw_overlap_all_pairs_capped, `max_kmer_occ`) against tests/kmer_ref.py: on the
planted-repeat read sets, which tests/test_kmer_ref.py proves (on the CPU) to hold a k-mer at and one above every cap, a pair
that loses all its seeds and one that changes scoring tier, the listed pairs, their order, the strand column, every field of
every record and the five counters equal the reference -- at every strand selection, sharded and unsharded."""
import functools

import numpy as np
import pytest

from tests import kmer_ref as KR

pytestmark = pytest.mark.gpu

K, L = KR.PLANTED_K, KR.PLANTED_L
STRANDS = ('+', '-', 'both')


def _fields():
    from biseqt_amd.overlap import BAND_DTYPE
    return [name for name in BAND_DTYPE.names if name != 'pad_']


@functools.lru_cache(maxsize=None)
def _reads(seed):
    return KR.planted_reads(seed)


@functools.lru_cache(maxsize=None)
def _ref(seed, max_occ, strands, rank=0, world=1):
    """The reference join and the record of every surviving pair, computed once per case."""
    reads = _reads(seed)
    join = KR.capped_join(reads, K, L, max_occ, strands, KR.DNA_COMPLEMENT, rank, world)
    recs = [KR.band_record(d, len(reads[a]), len(reads[b]), K, L) for (a, b, _), d in join.pairs.items()]
    return join, recs


def _raw(seed, strands, **kw):
    from biseqt_amd.overlap import raw_all_pairs
    stats = {}
    out = raw_all_pairs(_reads(seed), K, L, KR.G_MAX, KR.SENSITIVITY, strands=strands, complement=KR.DNA_COMPLEMENT, with_strand=True,
                        stats=stats, **kw)
    return out[0], out[1], out[2], stats


def _check(seed, max_occ, strands, got, rank=0, world=1):
    pairs, flags, recs, stats = got
    join, want = _ref(seed, max_occ, strands, rank, world)
    assert [(int(a), int(b), int(f)) for (a, b), f in zip(pairs.tolist(), flags.tolist())] == list(join.pairs)
    bad = {}
    for key, rec, o in zip(join.pairs, recs, want):
        diff = {f: (rec[f].item(), o[f]) for f in _fields() if rec[f].item() != o[f]}
        if diff:
            bad[key] = diff
    assert not bad, bad
    assert stats == join.stats


@pytest.mark.parametrize('strands', STRANDS)
@pytest.mark.parametrize('max_occ', KR.PLANTED_CAPS)
@pytest.mark.parametrize('seed', KR.PLANTED_SEEDS)
def test_capped_records_equal_the_reference(seed, max_occ, strands):
    _check(seed, max_occ, strands, _raw(seed, strands, max_kmer_occ=max_occ))


@pytest.mark.parametrize('strands', STRANDS)
@pytest.mark.parametrize('seed', KR.PLANTED_SEEDS)
def test_a_cap_at_the_largest_count_masks_nothing(seed, strands):
    from biseqt_amd.overlap import raw_all_pairs
    top = _ref(seed, 10 ** 6, strands)[0].max_count
    got = _raw(seed, strands, max_kmer_occ=top)
    _check(seed, top, strands, got)
    assert got[3]['masked_entries'] == 0 and got[3]['seeds_dropped'] == 0 and got[3]['distinct_masked'] == 0
    plain = raw_all_pairs(_reads(seed), K, L, KR.G_MAX, KR.SENSITIVITY, strands=strands, complement=KR.DNA_COMPLEMENT, with_strand=True)
    assert got[0].tobytes() == plain[0].tobytes() and got[1].tobytes() == plain[1].tobytes() and got[2].tobytes() == plain[2].tobytes()
    below = _raw(seed, strands, max_kmer_occ=top - 1)                                  # one below: the largest k-mer goes
    _check(seed, top - 1, strands, below)
    assert below[3]['distinct_masked'] >= 1 and below[3]['masked_entries'] >= top


@pytest.mark.parametrize('strands', STRANDS)
def test_none_and_zero_are_today_s_call(strands):
    from biseqt_amd.overlap import raw_all_pairs
    kw = dict(strands=strands, complement=KR.DNA_COMPLEMENT)
    plain = raw_all_pairs(_reads(0), K, L, KR.G_MAX, KR.SENSITIVITY, **kw)
    for cap in (None, 0):
        stats = {}
        got = raw_all_pairs(_reads(0), K, L, KR.G_MAX, KR.SENSITIVITY, max_kmer_occ=cap, stats=stats, **kw)
        assert len(got) == len(plain) and all(x.tobytes() == y.tobytes() for x, y in zip(got[:-1], plain[:-1]))
        assert stats == {}
    # the C entry point with max_occ = 0 is the stranded call bit for bit, and its stats are zeroed
    import ctypes as C
    from biseqt_amd import _pwlib as W
    from biseqt_amd.overlap import BAND_DTYPE, _band_coeffs
    lib = W.load()
    reads = _reads(0)
    lens = np.array([len(r) for r in reads], np.int32)
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    arena, roff = np.ascontiguousarray(np.concatenate(reads)), np.ascontiguousarray(offs[:-1])
    out = {}
    for capped in (False, True):
        pa, pb, ps, recs = np.zeros(200, np.int32), np.zeros(200, np.int32), np.zeros(200, np.uint8), np.zeros(200, BAND_DTYPE)
        n, cs = C.c_int64(0), W.pw_overlap_cap_stats(1, 2, 3, 4, 5)
        args = [0, arena.ctypes.data, arena.size, roff.ctypes.data, lens.ctypes.data, len(reads), L, K] + \
            list(_band_coeffs(KR.G_MAX, KR.SENSITIVITY, L, K)) + \
            [KR.DNA_COMPLEMENT.ctypes.data, {'+': 1, '-': 2, 'both': 3}[strands], 0, 1, 200, pa.ctypes.data, pb.ctypes.data, ps.ctypes.data,
             recs.ctypes.data, C.byref(n)]
        rc = lib.pw_overlap_all_pairs_capped(*(args + [0, C.byref(cs)])) if capped else lib.pw_overlap_all_pairs_stranded(*args)
        assert rc == 0
        out[capped] = (n.value, pa.tobytes(), pb.tobytes(), ps.tobytes(), recs.tobytes())
        if capped:
            assert [getattr(cs, f) for f, _ in cs._fields_] == [0] * 5
    assert out[False] == out[True]


@pytest.mark.parametrize('strands', STRANDS)
@pytest.mark.parametrize('world', [2, 3])
def test_sharded_ranks_add_up_to_the_unsharded_call(world, strands):
    seed, max_occ = 1, 7
    whole = _raw(seed, strands, max_kmer_occ=max_occ)
    parts = [_raw(seed, strands, max_kmer_occ=max_occ, rank=rank, world=world) for rank in range(world)]
    for rank, part in enumerate(parts):
        _check(seed, max_occ, strands, part, rank, world)
        assert all(int(a) % world == rank for a in part[0][:, 0])
        for f in ('entries', 'masked_entries', 'distinct_masked'):                      # counted over the whole read set
            assert part[3][f] == whole[3][f]
    for f in ('seeds_kept', 'seeds_dropped'):
        assert sum(part[3][f] for part in parts) == whole[3][f]
    pairs = np.concatenate([p[0] for p in parts])
    flags = np.concatenate([p[1] for p in parts])
    recs = np.concatenate([p[2] for p in parts])
    order = np.lexsort((flags, pairs[:, 1], pairs[:, 0]))
    assert pairs[order].tobytes() == whole[0].tobytes() and flags[order].tobytes() == whole[1].tobytes()
    assert recs[order].tobytes() == whole[2].tobytes()


@pytest.mark.parametrize('strands', ['+', 'both'])
def test_the_cap_lifts_the_capacity_refusal(strands):
    """max_pairs is judged on what survives the cap: with the capacity of the capped pair list the uncapped call is refused
    and the capped call succeeds -- which no implementation that filters after the expansion can do."""
    seed, max_occ = 0, 3
    join = _ref(seed, max_occ, strands)[0]
    n_capped, n_plain = len(join.pairs), len(join.uncapped)
    assert n_capped < n_plain
    with pytest.raises(RuntimeError) as e:
        _raw(seed, strands, max_pairs=n_capped)
    assert str(e.value).endswith('%d pairs of reads share a seed (capacity %d): raise max_pairs or the word length' % (n_plain, n_capped))
    _check(seed, max_occ, strands, _raw(seed, strands, max_pairs=n_capped, max_kmer_occ=max_occ))
    with pytest.raises(RuntimeError) as e:
        _raw(seed, strands, max_pairs=n_capped - 1, max_kmer_occ=max_occ)
    assert str(e.value).endswith('%d pairs of reads share a seed (capacity %d): raise max_pairs or the word length' % (n_capped, n_capped - 1))


@pytest.mark.parametrize('strands', ['+', 'both'])
def test_overlap_all_pairs_with_a_cap(strands):
    from biseqt_amd.overlap import _result, overlap_all_pairs
    from biseqt_amd.sequence import Alphabet
    seed, max_occ = 2, 7
    stats = {}
    got = overlap_all_pairs(_reads(seed), K, Alphabet('ACGT'), KR.G_MAX, KR.SENSITIVITY, stats=stats, strands=strands,
                            complement=[('A', 'T'), ('C', 'G')], max_kmer_occ=max_occ)
    join, recs = _ref(seed, max_occ, strands)
    keys = [(a, b) if strands == '+' else (a, b, '-' if s else '+') for a, b, s in join.pairs]
    assert list(got) == keys
    for key, r in zip(keys, recs):
        if r['w_best'] > 0:
            want = _result(r['d_best'], r['r_best'], r['len_best'], r['band_best'], r['w_best'], L, K)
        else:
            word_p = (r['n_first'] + 1 - (2 * r['r_first'] * r['len_first']) * ((1. / L) ** K)) / r['len_first']
            want = _result(r['d_first'], r['r_first'], r['len_first'], r['band_first'], word_p, L, K)
        assert got[key] == want, key
    assert stats['fallback_pairs'] == 0 and stats['pairs'] == len(keys)
    assert {f: stats[f] for f in join.stats} == join.stats


def test_a_tie_is_decided_by_the_record_under_a_cap():
    """U against U + U: two diagonals reach the same w.  Without a cap the pair goes to the single-pair fallback; with one (here
    above every count, so nothing is masked) the record's own rule decides -- largest w, then smallest d -- and no pair does."""
    from biseqt_amd.overlap import _result, overlap_all_pairs
    from biseqt_amd.sequence import Alphabet
    from tests import wide_words as WW
    x = WW.doubled(L, K)
    reads = [x.S, x.T]
    join = KR.capped_join(reads, K, L, 1000)
    r = KR.band_record(join.pairs[(0, 1, 0)], len(x.S), len(x.T), K, L)
    assert r['tie'] == 2 and r['w_best'] > 0 and join.stats['masked_entries'] == 0
    plain, capped = {}, {}
    overlap_all_pairs(reads, K, Alphabet('ACGT'), KR.G_MAX, KR.SENSITIVITY, stats=plain)
    got = overlap_all_pairs(reads, K, Alphabet('ACGT'), KR.G_MAX, KR.SENSITIVITY, stats=capped, max_kmer_occ=1000)
    assert plain['fallback_pairs'] == 1 and capped['fallback_pairs'] == 0
    assert got == {(0, 1): _result(r['d_best'], r['r_best'], r['len_best'], r['band_best'], r['w_best'], L, K)}

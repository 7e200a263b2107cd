"""The three sort-merge joins at every width of the k-mer key L^k against their CPU oracles, on the inputs of
tests/wide_words.py (tests/test_wide_words.py proves on the CPU that each can tell a wrong join from a right one):

  * the pairwise index (pw_seeds.hip) on every rung of the ladder -- 4-byte keys up to L^k = 3^20, 8-byte keys from 4^16 on --
    as two sequences, as a self comparison and with mask sets, row for row against oracle/seeds_oracle.py; and on either side
    of the switch between the direct-address table and the two binary searches, at the smallest and the largest table;
  * the N-way index (pw_mseeds.hip) against tests/mseeds_ref.py;
  * the overlap entry points at L^k = 2^62, which only they accept, against oracle/overlap_record_oracle.py (the rungs below
    it run through tests/test_gpu_overlap_records.py as the `wide_` groups of tests/overlap_cases.py).
Every comparison is exact equality; a mismatch names the case, the field and both values."""
import itertools

import numpy as np
import pytest

from oracle import overlap_record_oracle as RO, seeds_oracle as SO
from tests import mseeds_ref as R
from tests import overlap_cases as OC
from tests import wide_words as WW

pytestmark = pytest.mark.gpu

RUNGS = list(WW.LADDER)
IDS = ['L%d_k%d' % r for r in RUNGS]


def _alphabet(L):
    from biseqt_amd.sequence import Alphabet
    return Alphabet('0123456789abcdefghijklmnopqrstuvwxyz'[:L])


def _seq(A, x):
    from biseqt_amd.sequence import Sequence
    return Sequence(A, np.asarray(x, np.int64))


def _same_list(got, want, what):
    """Exact equality of two lists, reported by the first entry that differs."""
    got, want = list(got), list(want)
    for q, (g, w) in enumerate(zip(got, want)):
        assert g == w, '%s: entry %d is %r, the oracle has %r' % (what, q, g, w)
    assert len(got) == len(want), '%s: %d entries, the oracle has %d' % (what, len(got), len(want))


def _check_index(S, T, k, L, mask, what, min_rows=1):
    """rows(), seeds(), seeds(exclude_trivial=True), four band counts and the k-mers of both sides against the seeds oracle."""
    from biseqt_amd.seeds import SeedIndex
    A = _alphabet(L)
    rows, sc = SO.seed_rows(S.tolist(), T.tolist(), k, L, mask)
    assert len(rows) >= min_rows, what
    idx = SeedIndex(_seq(A, S), _seq(A, T), wordlen=k, alphabet=A, mask=mask)
    try:
        assert idx.self_comp == sc, what
        _same_list([tuple(r) for r in idx._idx.rows().tolist()], rows, what + ' rows')
        _same_list(idx.seeds(), SO.seeds(rows, sc), what + ' seeds')
        _same_list(idx.seeds(exclude_trivial=True), SO.seeds(rows, sc, exclude_trivial=True), what + ' seeds(exclude_trivial)')
        assert idx.seed_count() == len(rows), what
        rng = np.random.default_rng([L, k, len(S)])
        for q in range(4):
            d, a = rows[int(rng.integers(0, len(rows)))] if rows else (0, 0)
            db, ab = (d - int(rng.integers(0, 40)), d + q), (a - int(rng.integers(0, 300)), a + 20 * q)
            got = (idx.seed_count(d_band=db), idx.seed_count(a_band=ab), idx.seed_count(d_band=db, a_band=ab))
            want = (SO.seed_count(rows, d_band=db), SO.seed_count(rows, a_band=ab), SO.seed_count(rows, db, ab))
            assert got == want, '%s seed_count d_band=%r a_band=%r: %r, the oracle has %r' % (what, db, ab, got, want)
        for which, x in ((0, S), (1, S if sc else T)):
            want = [-1 if v is None else v for v in SO.as_kmer_seq(x.tolist(), k, L, mask)]
            _same_list(idx._idx.kmers(which).tolist(), want, '%s kmers(%d)' % (what, which))
    finally:
        idx.close()


# ---- pairwise index: every rung ----------------------------------------------------------------------------------------
@pytest.mark.parametrize('variant', ['two_sequences', 'self', 'masked'])
@pytest.mark.parametrize('rung', RUNGS, ids=IDS)
def test_pairwise_index_on_every_rung(rung, variant):
    L, k = rung
    x = WW.inputs(L, k)['basic']
    what = 'L%d k%d basic %s' % (L, k, variant)
    if variant == 'two_sequences':
        _check_index(x.S, x.T, k, L, [], what, min_rows=250)
    elif variant == 'self':
        _check_index(x.S, x.S.copy(), k, L, [], what, min_rows=len(x.S) - k + 1 + 1)        # the repeated word: a non-trivial row
    else:
        # the zero word is dropped (and with 36 letters the top word, by a set that holds letter 35); the masked key L^k takes
        # part in the sort: at L^k = 2^32 it is the only key with bit 32
        _check_index(x.S, x.T, k, L, WW.mask_sets(L), what, min_rows=1 if L == 2 else 250)


@pytest.mark.parametrize('rung', RUNGS, ids=IDS)
def test_pairwise_index_without_seeds_and_with_few(rung):
    L, k = rung
    ins = WW.inputs(L, k)
    _check_index(ins['empty'].S, ins['empty'].T, k, L, [], 'L%d k%d empty' % rung, min_rows=0)
    _check_index(ins['sparse'].S, ins['sparse'].T, k, L, [], 'L%d k%d sparse' % rung, min_rows=6)
    _check_index(ins['periodic'].S, ins['periodic'].T, k, L, [], 'L%d k%d periodic' % rung, min_rows=2049)


# ---- the switch between the direct-address table and the binary searches ----------------------------------------------------
@pytest.mark.parametrize('variant', ['plain', 'masked', 'self'])
@pytest.mark.parametrize('n_kmers', [1008, 1009], ids=['search_1008', 'table_1009'])
def test_table_switch_smallest(n_kmers, variant):
    """L = 4, k = 8: 4^8 // 1008 == 65 joins by binary search, 4^8 // 1009 == 64 through the table."""
    S, T = WW.table_edge_small(n_kmers)
    assert 4 ** 8 // (len(T) - 7) == (65 if n_kmers == 1008 else 64)
    what = 'L4 k8 %d k-mers %s' % (n_kmers, variant)
    if variant == 'self':
        _check_index(T, T.copy(), 8, 4, [], what, min_rows=n_kmers + 1)
    else:
        _check_index(S, T, 8, 4, [{0}, {0, 3}] if variant == 'masked' else [], what, min_rows=200)


@pytest.mark.parametrize('n_kmers', [1032444, 1032445], ids=['search_1032444', 'table_1032445'])
def test_table_switch_largest(n_kmers):
    """L = 4, k = 13: the largest table the rule admits (2^26 keys, 256 MB) and the densest T that still joins by search."""
    from biseqt_amd.seeds import _Index
    S, T = WW.table_edge_large(n_kmers)
    assert 4 ** 13 // (len(T) - 12) == (65 if n_kmers == 1032444 else 64)
    i, j = RO.seed_positions(S, T, 13, 4)
    assert len(i) > 5000
    with _Index(S, T, 13, _alphabet(4), self_comp=0) as idx:
        n = idx.build()
        rows = idx.rows().astype(np.int64)
    assert n == len(i), 'L4 k13 %d k-mers: %d rows, the oracle has %d' % (n_kmers, n, len(i))
    bad = np.flatnonzero((rows[:, 0] != i - j) | (rows[:, 1] != i + j))
    assert not len(bad), 'L4 k13 %d k-mers: row %d is %r, the oracle has %r' % (
        n_kmers, bad[0], rows[bad[0]].tolist(), [int(i[bad[0]] - j[bad[0]]), int(i[bad[0]] + j[bad[0]])])
    kS, kT = RO.kmer_keys(S, 13, 4), RO.kmer_keys(T, 13, 4)
    assert 0 in kS[i] and 4 ** 13 - 1 in kS[i] and (kS[i] == kT[j]).all()                # the first and the last table entry


# ---- N-way index -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('L,k,N', WW.NWAY, ids=['L%d_k%d_N%d' % t for t in WW.NWAY])
def test_nway_index(L, k, N):
    from biseqt_amd.seeds import SeedIndexMultiple
    A = _alphabet(L)
    raw = WW.nway(L, k, N)
    want = R.seed_rows(raw, k, L)
    assert len(want) >= 50
    idx = SeedIndexMultiple(*[_seq(A, s) for s in raw], wordlen=k, alphabet=A)
    try:
        got = idx.rows()
        _same_list([tuple(r) for r in got.tolist()], [tuple(r) for r in want.tolist()], 'L%d k%d N%d rows' % (L, k, N))
        rng = np.random.default_rng([L, k, N])
        boxes = []
        for t in rng.integers(0, len(want), 20):
            r = want[t]
            ds = [None if rng.random() < .3 else (int(r[q]) - int(rng.integers(0, 30)), int(r[q]) + 3) for q in range(N - 1)]
            boxes.append((ds, None if rng.random() < .2 else (int(r[-1]) - 200, int(r[-1]) + 200)))
        _same_list(idx.seed_counts(boxes), [R.box_count(want, ds, a) for ds, a in boxes], 'L%d k%d N%d box counts' % (L, k, N))
        assert idx.seed_count() == len(want)
    finally:
        idx.close()


# ---- the acceptance edge: L^k = 2^62 -------------------------------------------------------------------------------------
def _record_diff(rec, o):
    from biseqt_amd.overlap import BAND_DTYPE
    if int(rec['n_seeds']) != o['n_seeds'] or o['n_seeds'] == 0:
        return {'n_seeds': (int(rec['n_seeds']), o['n_seeds'])} if int(rec['n_seeds']) != o['n_seeds'] else {}
    return {f: (rec[f].item(), o[f]) for f in BAND_DTYPE.names if f != 'pad_' and rec[f].item() != o[f]}


def _edge_inputs():
    L, k = WW.EDGE
    return [WW.basic(L, k), WW.sparse(L, k), WW.doubled(L, k)]


def test_overlap_pair_list_at_2_62_one_pair_per_chunk():
    """kbits = 62: no bit is left for the pair id, every pair is a chunk of its own -- three pairs in one call, forward and
    with the middle one on the minus strand."""
    from biseqt_amd.overlap import raw_bands
    L, k = WW.EDGE
    ins = _edge_inputs()
    assert WW.chunk_sizes(len(ins), L, k) == [1, 1, 1]
    want = [RO.band_record(x.S, x.T, k, L, .2, .99) for x in ins]
    assert [o['n_seeds'] > 0 for o in want] == [True] * 3 and want[2]['tie'] == 2
    for x in ins:
        assert WW.max_key_bits(x) == 62
    reads = [r for x in ins for r in (x.S, x.T)]
    recs, _ = raw_bands(reads, [(0, 1), (2, 3), (4, 5)], k, L, .2, .99)
    bad = {x.name: _record_diff(rec, o) for x, rec, o in zip(ins, recs, want) if _record_diff(rec, o)}
    assert not bad, bad
    reads[3] = OC.revcomp(reads[3], L)
    recs, _ = raw_bands(reads, [(0, 1), (2, 3), (4, 5)], k, L, .2, .99, strands=['+', '-', '+'], complement=OC.COMPLEMENT[L])
    bad = {x.name: _record_diff(rec, o) for x, rec, o in zip(ins, recs, want) if _record_diff(rec, o)}
    assert not bad, bad


@pytest.mark.parametrize('strands', ['+', 'both'])
def test_overlap_all_pairs_at_2_62(strands):
    from biseqt_amd.overlap import raw_all_pairs
    L, k = WW.EDGE
    reads = [r for x in _edge_inputs()[:2] for r in (x.S, x.T)]
    want = []
    for a, b in itertools.combinations(range(len(reads)), 2):
        for st in ((0,) if strands == '+' else (0, 1)):
            o = RO.band_record(reads[a], OC.revcomp(reads[b], L) if st else reads[b], k, L, .2, .99)
            if o['n_seeds']:
                want.append((a, b, st, o))
    assert len(want) >= 6
    if strands == '+':
        pairs, recs, _ = raw_all_pairs(reads, k, L, .2, .99)
        flags = np.zeros(len(pairs), np.uint8)
    else:
        pairs, flags, recs, _ = raw_all_pairs(reads, k, L, .2, .99, strands=strands, complement=OC.COMPLEMENT[L])
    assert [(a, b, f) for (a, b), f in zip(pairs.tolist(), flags.tolist())] == [t[:3] for t in want]
    bad = {t[:3]: _record_diff(rec, t[3]) for rec, t in zip(recs, want) if _record_diff(rec, t[3])}
    assert not bad, bad


def _refusal(call):
    with pytest.raises(RuntimeError) as e:
        call()
    return str(e.value)


def test_what_each_entry_point_refuses():
    """L^k = 2^62 is refused by both indices (their masked key is L^k itself) and taken by the overlap entry points; 36^12 and
    wordlen = 32 are refused by all four."""
    from biseqt_amd.overlap import raw_all_pairs, raw_bands
    from biseqt_amd.seeds import _Index, _MIndex
    below = 'alphabet_len ^ wordlen must be below 2^62'
    for L, k, index_msg, overlap_msg in ((4, 31, below, None), (36, 12, below, below),
                                         (4, 32, 'wordlen must be 1..31 (kmers.py:269)', 'alphabet_len 1..36, wordlen 1..31'),
                                         (36, 32, 'wordlen must be 1..31 (kmers.py:269)', 'alphabet_len 1..36, wordlen 1..31')):
        rng = np.random.default_rng([L, k])
        s, t, u = (rng.integers(0, L, 80).astype(np.uint8) for _ in range(3))
        A = _alphabet(L)
        assert _refusal(lambda: _Index(s, t, k, A)) == 'pw_seeds_create failed: ' + index_msg
        assert _refusal(lambda: _MIndex([s, t, u], k, A)) == 'pw_mseeds_create failed: ' + index_msg
        if overlap_msg is None:
            recs, _ = raw_bands([s, s[10:]], [(0, 1)], k, L, .2, .99)
            assert int(recs[0]['n_seeds']) == 80 - 10 - k + 1
            pairs, recs, _ = raw_all_pairs([s, s[10:], t], k, L, .2, .99)
            assert pairs.tolist() == [[0, 1]] and int(recs[0]['n_seeds']) == 80 - 10 - k + 1
        else:
            assert _refusal(lambda: raw_bands([s, t], [(0, 1)], k, L, .2, .99)) == 'pw_overlap_bands failed: ' + overlap_msg
            assert _refusal(lambda: raw_all_pairs([s, t, u], k, L, .2, .99)) == 'pw_overlap_all_pairs failed: ' + overlap_msg
            assert _refusal(lambda: raw_bands([s, t], [(0, 1)], k, L, .2, .99, strands=['-'], complement=OC.COMPLEMENT[L])) == \
                'pw_overlap_bands_stranded failed: ' + overlap_msg
            assert _refusal(lambda: raw_all_pairs([s, t, u], k, L, .2, .99, strands='both', complement=OC.COMPLEMENT[L])) == \
                'pw_overlap_all_pairs_stranded failed: ' + overlap_msg

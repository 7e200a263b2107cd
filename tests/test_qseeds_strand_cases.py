"""CPU proofs for the stranded query-batched index: every case of tests/qseeds_strand_cases.py does what it is for (from the
dense oracle and arithmetic alone), bad arguments are refused before any device call, the ranking rule of
pipeline.map_queries on hand-written segment lists, and a tripwire on the compiled stranded match kernels."""
import os

import numpy as np
import pytest

from biseqt_amd.overlap import minus_to_forward, reverse_strand_keys
from biseqt_amd.sequence import Alphabet, Sequence
from tests import qseeds_cases as QC, qseeds_strand_cases as SC

A = Alphabet('ACGT')


def per_entry(sc):
    rows, off = QC.rows_of(sc)
    return [rows[off[e]:off[e + 1], 1:].tolist() for e in range(len(sc['queries']))]


def kmers(t, k):
    return {tuple(int(x) for x in t[j:j + k]) for j in range(len(t) - k + 1)}


# ---- the cases land where meant ------------------------------------------------------------------------------
def test_a_listed_minus_entry_is_the_reverse_complement_and_its_keys_come_from_the_forward_letters():
    sc = SC.lengths_around_k()
    k, L = sc['wordlen'], sc['L']
    for e, (s, f) in enumerate(zip(sc['source'], sc['strands'])):
        given = sc['base'][s]
        assert sc['queries'][e].tolist() == (SC.rc(given, sc['comp']) if f else given).tolist()
        if f:       # the host restatement of the device's encoder, on the forward letters == the forward keys of rc(query)
            want = [sum(int(x) * L ** (k - 1 - t) for t, x in enumerate(sc['queries'][e][j:j + k])) for j in range(len(given) - k + 1)]
            assert reverse_strand_keys(given, k, L, sc['comp']).tolist() == want


def test_lengths_around_k():
    sc = SC.lengths_around_k()
    k = sc['wordlen']
    assert [len(t) for t in sc['base']] == [n for n in range(7) for _ in (0, 1)] and len(sc['queries']) == 28
    assert sum(len(t) for t in sc['queries']) <= QC.MATCH_WG                     # one workgroup
    rows = per_entry(sc)
    for e, t in enumerate(sc['queries']):
        assert bool(rows[e]) <= (len(t) >= k)
    for n in range(k, 7):                       # the slice hits on its plus entry, the reversed slice on its minus entry
        fwd, rev = 2 * (2 * n), 2 * (2 * n + 1) + 1
        assert sc['strands'][fwd] == 0 and sc['strands'][rev] == 1
        assert len(rows[fwd]) >= len(sc['queries'][fwd]) - k + 1 and len(rows[rev]) >= len(sc['queries'][rev]) - k + 1
    assert any(rows[e] != rows[e + 1] for e in range(0, 28, 2))


@pytest.mark.parametrize('assign', SC.ASSIGNMENTS)
def test_boundary_traps_are_live(assign):
    """Every word a slip by one letter would form on the minus strand is in the reference, is no k-mer of the entry read
    correctly, and reading the frame one letter off changes the oracle's rows."""
    sc = SC.boundary_traps(assign)
    k = sc['wordlen']
    arena, offs, lens = SC.listing(sc)
    assert offs.tolist() == np.cumsum([0] + [len(t) for t in sc['base']])[:3].tolist()        # back to back
    words = SC.trap_words(*sc['base'])
    refk = kmers(sc['ref'], k)
    rows, off = QC.rows_of(sc)
    for (name, side), w in words.items():
        e = 'ABC'.index(name)
        assert tuple(w.tolist()) in refk
        assert tuple(w.tolist()) not in kmers(SC.rc(sc['base'][e], sc['comp']), k)
        if assign[e]:
            got, got_off = SC.slipped(sc, e, -1 if side == 'left' else 1)
            assert got.tolist() != rows.tolist() and got_off[e + 1] - got_off[e] != 0
            assert tuple(w.tolist()) in kmers(SC.rc(arena[offs[e] + (-1 if side == 'left' else 1):][:lens[e]], sc['comp']), k)
    assert all(len(r) >= 3 for r in per_entry(sc))                   # every entry has rows on the strand it is listed on


@pytest.mark.parametrize('pattern', SC.PATTERNS)
def test_edge_cases_keep_their_edges_under_strands(pattern):
    cases = [QC.query_edge_at_position(p) for p in QC.POSITION_EDGES] + [QC.many_queries_in_one_workgroup(), QC.empties_at_a_window_edge()] + \
            [QC.npos_around_a_workgroup(n) for n in QC.NPOS]
    for c in cases:
        sc = SC.with_strands(c, pattern)
        n = len(c['queries'])
        if pattern == 'twice':
            assert sc['source'] == [q for q in range(n) for _ in (0, 1)] and sc['strands'].tolist() == [0, 1] * n
            rows = per_entry(sc)
            assert [rows[2 * q] for q in range(n)] == per_entry(c)                # the plus entries are the case's own
            if sum(len(t) for t in c['queries']) > 1:
                assert any(rows[2 * q + 1] and rows[2 * q + 1] != rows[2 * q] for q in range(n))
        else:
            assert sc['strands'].tolist() == ([1] * n if pattern == 'minus' else [q % 2 for q in range(n)])
            assert all(a.tolist() == b.tolist() for a, b in zip(sc['queries'], c['queries']))       # seen == the case's queries
            assert QC.pstart(sc).tolist() == QC.pstart(c).tolist()                                  # ... on the case's positions
            assert QC.rows_of(sc)[0].tolist() == QC.rows_of(c)[0].tolist()
            flipped = [e for e in range(n) if sc['strands'][e] and len(sc['base'][e]) > 1]
            assert any(sc['base'][e].tolist() != c['queries'][e].tolist() for e in flipped) or not flipped
            assert any(per_entry(sc)[e] for e in range(n) if sc['strands'][e]) or len(QC.rows_of(c)[0]) == 0


@pytest.mark.parametrize('name', SC.STRAND_LOOKUPS)
def test_lookup_cases_reach_their_join(name):
    L, k, nref = QC.LOOKUPS[name]
    assert QC.lookup_of(L, k, nref) == QC.LOOKUP_PATH[name]
    assert {QC.LOOKUP_PATH[n] for n in SC.STRAND_LOOKUPS} == {'table', 'search32', 'search64'}
    assert QC.LOOKUPS['first64'][:2] == (4, 16) and 4 ** 16 >= 0xffffffff > 4 ** 15
    for pattern in ('minus', 'alternating'):
        sc = SC.lookup_case(name, pattern)
        assert (sc['comp'][sc['comp']] == np.arange(L)).all()
        assert all(per_entry(sc)[e] for e in (0, 1, 3, 4) if sc['strands'][e])     # both extreme keys hit on the minus strand


@pytest.mark.parametrize('L', sorted(SC.ALPHABETS))
def test_alphabet_cases(L):
    sc = SC.alphabet_case(L)
    comp = np.array(SC.ALPHABETS[L])
    assert (comp[comp] == np.arange(L)).all() and int((comp == np.arange(L)).sum()) == {2: 0, 3: 1, 5: 1}[L]
    assert sc['strands'].tolist() == [0, 1, 0, 1, 0, 1] and all(per_entry(sc)[e] for e in (3, 5))
    assert sc['base'][3].tolist() != sc['queries'][3].tolist()


def test_palindromes():
    sc = SC.palindromes()
    rows = per_entry(sc)
    for q in range(4):
        assert sc['queries'][2 * q].tolist() == sc['queries'][2 * q + 1].tolist() and rows[2 * q] == rows[2 * q + 1] and rows[2 * q]


# ---- argument validation: before the device is touched -------------------------------------------------------
def _untouchable_index():
    """A _QIndex without a handle or a library: any call into the device would fail on None."""
    from biseqt_amd.seeds import _QIndex
    qi = _QIndex.__new__(_QIndex)
    qi.lib, qi.handle, qi.device, qi.alphabet_len, qi._edges = None, None, 0, 4, None
    return qi


def test_bad_strands_and_complements_are_refused_by_the_index():
    qi = _untouchable_index()
    arena, offs, lens = QC.pack_tight([np.array([0, 1, 2, 3]), np.array([3, 2, 1])])
    for strands in (['+', 'x'], [0, 2], ['+', None], ['-'], ['+', '-', '+']):
        with pytest.raises(ValueError):
            qi.build(arena, offs, lens, strands=strands, complement=SC.COMP4)
    for comp in (None, [1, 2, 3, 0], [3, 2, 1], [3, 2, 1, 4], [[3, 2], [1, 0]]):
        with pytest.raises(ValueError):
            qi.build(arena, offs, lens, strands=['+', '-'], complement=comp)
    with pytest.raises(ValueError):                                   # a complement that is given is checked, minus entry or not
        qi.build(arena, offs, lens, strands=['+', '+'], complement=[1, 2, 3, 0])
    with pytest.raises((AttributeError, TypeError)):                  # ... and valid arguments do reach the (absent) library
        qi.build(arena, offs, lens, strands=['+', '-'], complement=SC.COMP4)


def test_bad_strands_and_complements_are_refused_by_the_flows(monkeypatch):
    from biseqt_amd import blot, pipeline

    def touched(*a, **kw):
        raise AssertionError('the device was touched')
    monkeypatch.setattr(blot, '_QIndex', touched)
    monkeypatch.setattr(pipeline, 'DeviceArena', touched)
    ref, q = Sequence(A, (0, 1, 2, 3) * 10), Sequence(A, (3, 2, 1, 0, 0, 1))
    loc = blot.WordBlotLocalRef(ref, wordlen=3, alphabet=A, g_max=.2, sensitivity=.99)
    for kw in (dict(strands='x'), dict(strands='-'), dict(strands='both', complement=[1, 2, 3, 0]), dict(strands='-', complement={'A': 'C'}),
               dict(strands='both', complement=[3, 2, 1])):
        with pytest.raises(ValueError):
            loc.similar_segments_many([q], 10, .5, **kw)
        with pytest.raises(ValueError):
            pipeline.map_queries(ref, [q], 10, .5, 3, .2, .99, **kw)
    with pytest.raises(AssertionError, match='the device was touched'):           # valid arguments go on to the device
        loc.similar_segments_many([q], 10, .5, strands='both', complement=[('A', 'T'), ('C', 'G')])


# ---- the ranking rule of map_queries -------------------------------------------------------------------------
def _seg(p, a_min, a_max, strand, d=(0, 10)):
    return {'segment': (d, (a_min, a_max)), 'p': p, 'strand': strand}


def test_a_tie_goes_to_the_plus_strand():
    from biseqt_amd.pipeline import rank_segments
    plus, minus = _seg(.5, 0, 100, '+'), _seg(.5, 40, 140, '-')
    assert rank_segments([plus, minus], 1) == [plus] and rank_segments([plus, minus], 2) == [plus, minus]
    assert rank_segments([_seg(.25, 0, 200, '+'), _seg(.5, 40, 140, '-', d=(-3, 4))], 1)[0]['strand'] == '+'     # 50 == 50


def test_keep_cuts_across_strands():
    from biseqt_amd.pipeline import rank_segments
    segs = [_seg(.9, 0, 100, '+'), _seg(.8, 0, 50, '+'), _seg(.7, 0, 20, '+'), _seg(.9, 0, 90, '-'), _seg(.6, 0, 200, '-')]
    got = rank_segments(segs, 3)
    assert [(s['strand'], s['p']) for s in got] == [('-', .6), ('+', .9), ('-', .9)]
    assert rank_segments(segs, 10) == sorted(segs, key=lambda s: -s['p'] * (s['segment'][1][1] - s['segment'][1][0]))
    assert rank_segments(segs, 0) == [] and rank_segments([], 3) == []


def test_query_interval_on_both_strands():
    from biseqt_amd.pipeline import query_interval
    qlen = 40
    for tx, start in (('MMMSMMIMMDDMM', 5), ('M', 0), ('MMMM', 36), ('IIMDM', 17), ('M' * 40, 0)):
        on_query = sum(tx.count(op) for op in 'MSI')
        assert query_interval('+', start, on_query, qlen) == (start, start + on_query)
        assert query_interval('-', start, on_query, qlen) == minus_to_forward(start, tx, qlen)
    # the letters the minus interval names, reversed and complemented, are the letters of rc(query) the alignment covers
    rng = np.random.default_rng(5)
    t = rng.integers(0, 4, qlen)
    lo, hi = query_interval('-', 5, 11, qlen)
    assert SC.rc(t[lo:hi], SC.COMP4).tolist() == SC.rc(t, SC.COMP4)[5:16].tolist()
    with pytest.raises(AssertionError):
        query_interval('-', 35, 6, qlen)


# ---- the compiled kernels ------------------------------------------------------------------------------------
def test_stranded_match_kernels_use_no_scratch():
    """Both key widths exist; the complement table and the window are all the LDS there is (36 + 16 bytes); nothing in
    scratch: a by-value table indexed per lane would land there."""
    from biseqt_amd.csrc import build as B, codeobj
    path = os.path.join(B.OBJ_DIR, 'pw_qseeds.o')
    if not os.path.exists(path):
        B.build()
    md = {n: k for n, k in codeobj.kernel_metadata(path).items() if 'k_qmatch_stranded<' in n}
    assert sorted(n.split('k_qmatch_stranded<')[1].split('>')[0] for n in md) == ['unsigned int', 'unsigned long'], sorted(md)
    for name, k in md.items():
        assert k['private_segment_fixed_size'] == 0 and k['vgpr_spill_count'] == 0 and k['sgpr_spill_count'] == 0, (name, k)
        assert k['group_segment_fixed_size'] <= 64, (name, k['group_segment_fixed_size'])

"""pipeline.map_queries(strands=...) on reads from both strands (qseeds_strand_cases.flipped_mixed: every odd-numbered
query of the mixed sets reverse-complemented): every record against the C oracle (= the compiled reference) on (ref, query)
or (ref, rc(query)) by its strand, as test_gpu_map_queries.py does; against the default call on the ORIGINAL queries; and
against the stable merge of two default calls, one on the queries and one on their host reverse complements."""
import pytest

from biseqt_amd.overlap import minus_to_forward
from biseqt_amd.pipeline import map_queries, rank_segments
from biseqt_amd.sequence import reverse_complement
from tests import blot_many_cases as Cs, qseeds_strand_cases as SC

pytestmark = pytest.mark.gpu
COMP = [('A', 'T'), ('C', 'G')]
TODAY = {'segment', 'p', 'diag_range', 'score', 'alignment', 'p_aln', 'len_aln'}


def _args(name):
    ref, queries, wordlen, K_min, p_min = SC.flipped_mixed(name)
    return Cs.mk(ref), [Cs.mk(t) for t in queries], (K_min, p_min, wordlen, Cs.G_MAX, Cs.SENS)


def _aligned(rec):
    aln = rec['alignment']
    return (rec['segment'], rec['p'], rec['diag_range'], rec['score'], rec['p_aln'], rec['len_aln'],
            None if aln is None else (aln.transcript, aln.origin_start, aln.mutant_start))


def test_both_strands_vs_oracle_and_the_default_call_on_the_original_queries(oracle):
    ref, queries, wordlen, K_min, p_min = SC.flipped_mixed('a')
    original = Cs.mixed_case('a', 30)[1]
    R, Q, args = _args('a')
    got = map_queries(R, Q, *args, strands='both', complement=COMP)
    assert len(got) == len(queries)
    best = {'+': 0, '-': 0}
    aligned = 0
    for q, recs in enumerate(got):
        if recs:
            best[recs[0]['strand']] += 1
        for rec in recs:
            assert set(rec) == TODAY | {'strand', 'query_interval'}
            d_band = rec['segment'][0]
            assert rec['diag_range'] == (int(d_band[0]), int(d_band[1]))
            mutant = SC.rc(queries[q], SC.COMP4) if rec['strand'] == '-' else queries[q]
            r = oracle.solve(ref, mutant, L=4, mode=1, alntype=1, diag_range=rec['diag_range'], match=1, mismatch=-3, go=-5, ge=-2)
            if r['init_rc'] != 0 or r['opt'][0] == -1 or r['would_panick'] or r['tb_null'] or not r['transcript']:
                assert rec['alignment'] is None and rec['score'] is None and rec['p_aln'] is None and rec['query_interval'] is None
                continue
            aln = rec['alignment']
            assert aln is not None, (q, rec)
            assert rec['score'] == r['score'] and aln.transcript == r['transcript']
            assert (aln.origin_start, aln.mutant_start) == (r['origin_idx'], r['mutant_idx'])
            assert aln.origin == R and aln.mutant == (reverse_complement(Q[q], COMP) if rec['strand'] == '-' else Q[q])
            tx = r['transcript']
            on_query = sum(tx.count(op) for op in 'MSI')
            assert rec['len_aln'] == on_query and rec['p_aln'] == round(1. * tx.count('M') / on_query, 2)
            if rec['strand'] == '-':
                assert rec['query_interval'] == minus_to_forward(aln.mutant_start, tx, len(queries[q]))
            else:
                assert rec['query_interval'] == (aln.mutant_start, aln.mutant_start + on_query)
            aligned += 1
    assert best['-'] >= 5 and best['+'] >= 5 and aligned >= 15, (best, aligned)
    # a flipped query maps, on its minus strand, as the original query does by default
    default = map_queries(Cs.mk(ref), [Cs.mk(t) for t in original], *args)
    for q in range(1, len(queries), 2):
        assert SC.rc(queries[q], SC.COMP4).tolist() == original[q].tolist()
        on_minus = [rec for rec in got[q] if rec['strand'] == '-']               # (case 'a' has no query with segments on both:
        assert [_aligned(rec) for rec in on_minus] == [_aligned(rec) for rec in default[q]], q       # `keep` cuts one strand only)
    assert SC.strand_census('a')[2] == 0


def test_both_strands_are_the_stable_merge_of_two_default_calls():
    R, Q, args = _args('b')
    keep = 2
    got = map_queries(R, Q, *args, keep=keep, strands='both', complement=COMP)
    plus = map_queries(R, Q, *args, keep=10 ** 6)
    minus = map_queries(R, [reverse_complement(T, COMP) for T in Q], *args, keep=10 ** 6)
    cut = across = 0
    for q in range(len(Q)):
        merged = rank_segments([dict(r, strand='+') for r in plus[q]] + [dict(r, strand='-') for r in minus[q]], keep)
        assert [(r['strand'],) + _aligned(r) for r in got[q]] == [(r['strand'],) + _aligned(r) for r in merged], q
        cut += len(plus[q]) + len(minus[q]) > keep
        across += len({r['strand'] for r in got[q]}) == 2
    assert cut >= 2 and across >= 3, (cut, across)
    only_minus = map_queries(R, Q, *args, keep=keep, strands='-', complement=COMP)
    for q in range(len(Q)):
        assert [('-',) + _aligned(r) for r in minus[q][:keep]] == [(r['strand'],) + _aligned(r) for r in only_minus[q]], q


def test_summaries_alone_give_the_same_fields():
    R, Q, args = _args('b')
    full = map_queries(R, Q, *args, strands='both', complement=COMP)
    lean = map_queries(R, Q, *args, strands='both', complement=COMP, alignments=False)
    n = 0
    for q in range(len(Q)):
        assert len(full[q]) == len(lean[q])
        for a, b in zip(full[q], lean[q]):
            assert b['alignment'] is None and set(b) == TODAY | {'strand', 'query_interval', 'origin_start', 'mutant_start', 'summary'}
            aln = a['alignment']
            starts = (None, None) if aln is None else (aln.origin_start, aln.mutant_start)
            assert (a['segment'], a['score'], a['p_aln'], a['len_aln'], a['strand'], a['query_interval'], starts) == \
                (b['segment'], b['score'], b['p_aln'], b['len_aln'], b['strand'], b['query_interval'], (b['origin_start'], b['mutant_start']))
            n += aln is not None
    assert n >= 15


def test_the_default_call_has_todays_keys():
    R, Q, args = _args('b')
    got = map_queries(R, Q[:12], *args)
    assert sum(len(recs) for recs in got) >= 4 and all(set(rec) == TODAY for recs in got for rec in recs)
    lean = map_queries(R, Q[:12], *args, alignments=False)
    assert all(set(rec) == TODAY | {'origin_start', 'mutant_start', 'summary'} for recs in lean for rec in recs)

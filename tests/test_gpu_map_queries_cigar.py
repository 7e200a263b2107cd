"""pipeline.map_queries(cigar=...) and pipeline.paf_lines on the mixed set 'a' (blot_many_cases.mixed_case('a', 30)) and on the
same set with every odd query reverse-complemented under strands='both' (qseeds_strand_cases.flipped_mixed('a')): every
``rec['cigar']`` against the ``itertools.groupby`` oracle of tests/cigar_ref.py on the record's transcript, the same strings
with ``alignments=False`` (no transcript on the host), every other field as without ``cigar``, and the PAF columns against
the runs of the ``cg`` tag."""
import re

import pytest

from biseqt_amd.overlap import minus_to_forward
from biseqt_amd.pipeline import map_queries, paf_lines
from tests import blot_many_cases as Cs, cigar_ref as R, qseeds_strand_cases as SC

pytestmark = pytest.mark.gpu
COMP = [('A', 'T'), ('C', 'G')]
# the keys of the records before map_queries had `cigar`, by call
TODAY = {'segment', 'p', 'diag_range', 'score', 'alignment', 'p_aln', 'len_aln'}
LEAN = {'origin_start', 'mutant_start', 'summary'}
STRANDED = {'strand', 'query_interval'}


def _case(stranded):
    ref, queries, wordlen, K_min, p_min = SC.flipped_mixed('a') if stranded else Cs.mixed_case('a', 30)
    kw = dict(strands='both', complement=COMP) if stranded else {}
    return ref, queries, Cs.mk(ref), [Cs.mk(t) for t in queries], (K_min, p_min, wordlen, Cs.G_MAX, Cs.SENS), kw


@pytest.fixture(scope='module', params=[False, True], ids=['plus', 'both-strands'])
def runs(request):
    """The calls every test of a case shares: the default call in both ``alignments=`` modes and both forms in both modes."""
    ref, queries, Rf, Q, args, kw = _case(request.param)
    out = dict(stranded=request.param, ref=ref, queries=queries, extra=STRANDED if request.param else set())
    out['full'] = map_queries(Rf, Q, *args, **kw)
    out['lean'] = map_queries(Rf, Q, *args, alignments=False, **kw)
    for form in ('extended', 'classic'):
        out['full', form] = map_queries(Rf, Q, *args, cigar=form, **kw)
        out['lean', form] = map_queries(Rf, Q, *args, alignments=False, cigar=form, **kw)
    return out


def _without_cigar(rec):
    aln = rec['alignment']
    return dict({k: v for k, v in rec.items() if k not in ('cigar', 'alignment')},
                alignment=None if aln is None else (aln.transcript, aln.origin_start, aln.mutant_start, aln.score))


def test_the_default_call_has_todays_keys(runs):
    assert sum(len(recs) for recs in runs['full']) >= 10
    assert all(set(rec) == TODAY | runs['extra'] for recs in runs['full'] for rec in recs)
    assert all(set(rec) == TODAY | LEAN | runs['extra'] for recs in runs['lean'] for rec in recs)


@pytest.mark.parametrize('form', ['extended', 'classic'])
def test_cigars_equal_the_oracle_and_nothing_else_changes(runs, form):
    code = dict(R.FORMS)[form]
    aligned = 0
    for mode, keys in (('full', TODAY), ('lean', TODAY | LEAN)):
        got, base = runs[mode, form], runs[mode]
        assert len(got) == len(base)
        for q in range(len(got)):
            assert len(got[q]) == len(base[q]), (mode, q)
            for rec, old, full in zip(got[q], base[q], runs['full'][q]):
                assert set(rec) == keys | runs['extra'] | {'cigar'}
                assert _without_cigar(rec) == _without_cigar(old), (mode, q)
                aln = full['alignment']                  # the transcript of the default call: the oracle's input
                if aln is None:
                    assert rec['cigar'] is None and rec['score'] is None
                    continue
                assert rec['cigar'] == R.string(aln.transcript, code), (mode, q)
                if mode == 'lean':
                    assert rec['alignment'] is None
                else:
                    assert rec['alignment'].transcript == aln.transcript
                aligned += 1
    assert aligned >= 20
    if form == 'classic':
        assert all('=' not in rec['cigar'] and 'X' not in rec['cigar'] for recs in runs['full', form] for rec in recs if rec['cigar'])


def test_a_bad_form_is_refused():
    ref, queries, Rf, Q, args, kw = _case(False)
    with pytest.raises(ValueError):
        map_queries(Rf, Q[:2], *args, cigar='bam')


def _consumed(cg, ops):
    return sum(int(n) for n, op in re.findall(r'(\d+)([MIDNSHP=X])', cg) if op in ops)


@pytest.mark.parametrize('mode', ['full', 'lean'])
def test_paf_lines(runs, mode):
    queries = runs['queries']
    names = ['q%d' % q for q in range(len(queries))]
    lens = [len(t) for t in queries]
    mapped = runs[mode, 'extended']
    lines = paf_lines(mapped, 'ref', len(runs['ref']), names, lens)
    recs = [(q, rec) for q, recs in enumerate(mapped) for rec in recs if rec['score'] is not None]
    assert len(lines) == len(recs) >= 10
    assert len(lines) == sum(full['alignment'] is not None for recs in runs['full'] for full in recs)
    minus = 0
    for line, (q, rec), full in zip(lines, recs, [f for fs in runs['full'] for f in fs if f['alignment'] is not None]):
        col = line.split('\t')
        assert len(col) == 14 and col[0] == names[q] and int(col[1]) == lens[q] and col[5] == 'ref' and int(col[6]) == len(runs['ref'])
        assert col[11] == '255' and col[12] == 'AS:i:%d' % rec['score'] and col[13] == 'cg:Z:' + rec['cigar']
        qs, qe, ts, te, nmatch, nall = int(col[2]), int(col[3]), int(col[7]), int(col[8]), int(col[9]), int(col[10])
        cg = rec['cigar']
        assert te - ts == _consumed(cg, '=XD') and qe - qs == _consumed(cg, '=XI')
        assert nmatch == _consumed(cg, '=') and nall == _consumed(cg, '=XID')
        aln = full['alignment']
        assert ts == aln.origin_start and 0 <= qs < qe <= lens[q] and 0 <= ts < te <= len(runs['ref'])
        assert col[4] == (rec['strand'] if runs['stranded'] else '+')
        if col[4] == '-':
            assert (qs, qe) == minus_to_forward(aln.mutant_start, aln.transcript, lens[q])
            minus += 1
        else:
            assert (qs, qe) == (aln.mutant_start, aln.mutant_start + _consumed(cg, '=XI'))
    assert (minus >= 5) if runs['stranded'] else (minus == 0)
    # the classic form in the tag, the same columns
    classic = paf_lines(runs[mode, 'classic'], 'ref', len(runs['ref']), names, lens)
    assert [l.split('\t')[:13] for l in classic] == [l.split('\t')[:13] for l in lines]
    assert all(te - ts == _consumed(cg, 'MD') for ts, te, cg in ((int(l.split('\t')[7]), int(l.split('\t')[8]), l.split('\t')[13]) for l in classic))
    # without `cigar` there is no cg tag and the other columns are the same
    plain = paf_lines(runs[mode], 'ref', len(runs['ref']), names, lens)
    assert plain == ['\t'.join(l.split('\t')[:13]) for l in lines]

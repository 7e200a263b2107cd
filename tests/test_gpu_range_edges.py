"""The planner's range bounds at their edges on the GPU (tests/range_edges.py): every case through ``BatchAligner``, its
whole batch.  The kernel is the one ``plan_only`` chose, every distinct pair equals the oracle, the whole batch equals a
run off the kernel under test (``PW_FLAG_NO_PACKED16``, or ``PW_FLAG_FORCE_F64`` for the int32, strip and dyadic rows) --
records and transcripts --, and the packed transcripts equal the slots."""
import numpy as np
import pytest

from biseqt_amd.batch import BatchAligner
from tests import range_edges as R
from tests.test_range_edges import CASES, FIELDS, check_plan, planned

pytestmark = pytest.mark.gpu


def _run(case, flags):
    kw = case['kw']
    bkw = dict(alnmode=kw['mode'], alntype=kw['alntype'], alphabet_len=kw['L'], go_score=kw['go'], ge_score=kw['ge'],
               check_band=False)
    if kw.get('subst') is not None:
        bkw['subst_scores'] = kw['subst']
    else:
        bkw.update(match_score=kw['match'], mismatch_score=kw['mismatch'])
    if kw.get('diag_range') is not None:
        bkw['diag_range'] = kw['diag_range']
    with BatchAligner(R.batch_of(case), flags=flags, **bkw) as b:
        name = b.kernel_name
        res = b.run().copy()
        txs = b.transcripts(res)
        b.pack_transcripts()
        packed = b.transcripts_from_packed(*b.packed())
    return name, res, txs, packed


@pytest.mark.parametrize('case', CASES, ids=[c['id'] for c in CASES])
def test_gpu_range_edge(case, monkeypatch, oracle):
    plan = planned(case, monkeypatch)
    check_plan(case, plan)
    if plan['strips']:
        monkeypatch.setenv('PWLIB_NO_STRIP_REPAIR', '1')
    flags = case.get('flags', 0)
    name, res, txs, packed = _run(case, flags)
    assert name == plan['kernel'], (case['id'], name, plan['kernel'])
    assert packed == txs, case['id']
    c = case['copies']
    for k, (o, m) in enumerate(case['pairs']):
        want = oracle.solve(o, m, **case['kw'])
        for i in range(k * c, (k + 1) * c):
            got = dict(init_rc=want['init_rc'], opt=(int(res['opt_i'][i]), int(res['opt_j'][i])))
            if got['opt'] == (-1, -1) or want['init_rc'] != 0:
                assert got['opt'] == (want['opt'] or (-1, -1)), (case['id'], i)
                continue
            assert got['opt'] == tuple(want['opt']) and res['score'][i] == want['score'], (case['id'], i, res[i], want['score'])
            if not want['would_panick'] and not want['tb_null']:
                assert txs[i] == want['transcript'], (case['id'], i)
                assert (res['origin_idx'][i], res['mutant_idx'][i]) == (want['origin_idx'], want['mutant_idx']), (case['id'], i)
    rname, rres, rtxs, _ = _run(case, flags | case['reference'])
    assert np.array_equal(res, rres) and txs == rtxs, (case['id'], name, rname)


def test_gpu_int_max_floor_refused_or_exact():
    """Every problem of tests/golden/extreme_scores.json (scores around the reference's -INT_MAX floor) is either refused
    by the planner or equals the compiled reference's answer: none returns a different one."""
    from tests.helpers import check_against_expect, dec, kw_of, load_golden
    refused = 0
    for k, rec in enumerate(load_golden('extreme_scores.json')):
        kw = kw_of(rec)
        bkw = dict(alnmode=kw['mode'], alntype=kw['alntype'], alphabet_len=kw['L'], match_score=kw['match'],
                   mismatch_score=kw['mismatch'], go_score=kw['go'], ge_score=kw['ge'], check_band=False)
        if 'diag_range' in kw:
            bkw['diag_range'] = kw['diag_range']
        o, m = np.array(dec(rec['origin']), np.uint8), np.array(dec(rec['mutant']), np.uint8)
        try:
            b = BatchAligner([(o, m)], **bkw)
        except RuntimeError as e:
            assert 'INT_MAX' in str(e), (k, e)
            refused += 1
            continue
        with b:
            res = b.run()
            tx = b.transcripts(res)[0]
            st = int(res['status'][0])
            got = dict(init_rc=b.init_rc(0), opt=(int(res['opt_i'][0]), int(res['opt_j'][0])), score=float(res['score'][0]),
                       would_panick=bool(st & 4), tb_null=bool(st & 2) and not (st & 4), transcript=tx,
                       origin_idx=int(res['origin_idx'][0]), mutant_idx=int(res['mutant_idx'][0]))
            if 'band' in rec['expect']:
                got['band'] = b.band(0)[:2]
        check_against_expect(got, rec['expect'], where='extreme[%d]' % k)
    assert refused >= 10

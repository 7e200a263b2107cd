"""The planner's range bounds at their edges on the CPU (tests/range_edges.py): for every row, side, rule and layout,
``batch.plan_only`` reports the kernel the row expects, and every pair solved by the CPU lane emulator on THAT kernel
(``emu.solve_planned``) equals the oracle.  The outside case runs on its fallback kernel and must agree too.  Cases the
emulator cannot run in this suite's time are marked ``gpu_only`` in the table: here only their plan is checked;
tests/test_gpu_range_edges.py runs them."""
import pytest

from biseqt_amd.batch import plan_only
from tests import range_edges as R
from tests.emu import emu

CASES = R.cases()
FIELDS = ('init_rc', 'opt', 'score', 'transcript', 'origin_idx', 'mutant_idx', 'tb_null', 'would_panick')


def planned(case, monkeypatch):
    """plan_only on the case's whole batch under its knobs (set in the environment, undone after the test)."""
    for k, v in case['env'].items():
        monkeypatch.setenv(k, v)
    kw = case['kw']
    pairs = R.batch_of(case)
    L = kw['L']
    subst = kw.get('subst') or [[kw['match'] if i == j else kw['mismatch'] for i in range(L)] for j in range(L)]
    dr = kw.get('diag_range')
    shapes = [(len(o), len(m)) + (tuple(dr) if dr else ()) for o, m in pairs]
    return plan_only(shapes, alnmode=kw['mode'], alntype=kw['alntype'], alphabet_len=L, subst_scores=subst,
                     go_score=kw['go'], ge_score=kw['ge'], flags=case.get('flags', 0))


def check_plan(case, plan):
    exp = dict(case['expect'])
    has, lacks = exp.pop('kernel_has', []), exp.pop('kernel_lacks', [])
    if exp.get('strips') == 'all':
        exp['strips'] = len(R.batch_of(case))
    for k, v in exp.items():
        assert plan[k] == v, (case['id'], k, plan)
    assert all(s in plan['kernel'] for s in has) and not any(s in plan['kernel'] for s in lacks), (case['id'], plan)


def test_table_covers_every_row_on_both_sides():
    rows = {}
    for c in CASES:
        rows.setdefault(c['row'], set()).add(c['side'])
    assert len(rows) >= 18 and all(s == {'inside', 'outside'} for s in rows.values()), rows


@pytest.mark.parametrize('case', CASES, ids=[c['id'] for c in CASES])
def test_range_edge(case, monkeypatch, oracle):
    plan = planned(case, monkeypatch)
    check_plan(case, plan)
    if case['gpu_only']:
        return                                   # (tests/test_gpu_range_edges.py runs it: see the table)
    pairs = case['pairs']                        # (copies of a pair are solved once: the plan is the whole batch's)
    plan2, got = emu.solve_planned(R.batch_of(case), flags=case.get('flags', 0), **case['kw'])
    assert plan2 == plan
    for k, (o, m) in enumerate(pairs):
        want = oracle.solve(o, m, **case['kw'])
        g = got[k * case['copies']]
        for f in FIELDS:
            assert g[f] == want[f], (case['id'], k, f, g[f], want[f], plan['kernel'])


# ---- the reference's -INT_MAX floor (pw_plan.h, reaches_reference_floor) ----

def test_oracle_matches_reference_at_the_int_max_floor(oracle):
    """The oracle against the compiled reference with scores up to +-3e9, where the reference floors gap candidates and end
    cells at -INT_MAX (tests/golden/make_extreme_golden.py), field by field."""
    from tests.helpers import check_against_expect, dec, kw_of, load_golden
    recs = load_golden('extreme_scores.json')
    assert len(recs) >= 50 and sum(r['expect'].get('opt') == [-1, -1] for r in recs) >= 2
    for k, rec in enumerate(recs):
        check_against_expect(oracle.solve(dec(rec['origin']), dec(rec['mutant']), **kw_of(rec)), rec['expect'],
                             where='extreme[%d]' % k)


def test_int_max_floor_refused_or_exact_in_the_emulator():
    """Every problem of extreme_scores.json is refused by the planner or, on the kernel the planner picks, equals the
    reference: the accepted ones (huge substitution scores with gap steps the bound allows) show that no cell maximum gets
    near the floor there."""
    from tests.helpers import check_against_expect, dec, kw_of, load_golden
    refused = 0
    for k, rec in enumerate(load_golden('extreme_scores.json')):
        try:
            plan, (got,) = emu.solve_planned([(dec(rec['origin']), dec(rec['mutant']))], **kw_of(rec))
        except RuntimeError as e:
            assert 'INT_MAX' in str(e), (k, e)
            refused += 1
            continue
        check_against_expect(got, rec['expect'], where='extreme[%d] %s' % (k, plan['kernel']))
    assert refused >= 10 and refused <= 44


def test_plan_refuses_scores_that_reach_the_int_max_floor(oracle):
    """(X + Y + 2) * h < INT_MAX, except for the begin-anywhere rules; h = -(ge + min(go, 0)), what one gap step can lower
    a cell's maximum by, and on a band of one diagonal the lowest substitution too (pw_plan.h, reaches_reference_floor).
    At the edge: 50 x 45 (span 97) with h = 22139006 is planned (f64) and the emulator's f64 kernel equals the oracle;
    22139007 is refused.  A mismatch that low is accepted where gap steps are there (standard mode, a band of 3
    diagonals), refused on a one-diagonal band one unit past the edge.  LOCAL and B_LOCAL with go = -3e9 stay accepted and
    equal the oracle."""
    import numpy as np
    INT_MAX = 2147483647
    rng = np.random.default_rng(97)
    o = rng.integers(0, 4, 50)
    m = np.delete(o, range(20, 25))
    span = len(o) + len(m) + 2
    a = (INT_MAX - 1) // span                   # the largest max|score| with span * a < INT_MAX
    assert (a, span * (a + 1) >= INT_MAX) == (22139006, True)
    for go, refused in ((-float(a), False), (-float(a + 1), True)):
        kw = dict(alnmode=0, alntype=0, alphabet_len=4, match_score=1, mismatch_score=-1, go_score=go + 1, ge_score=-1)
        if refused:
            with pytest.raises(RuntimeError, match='INT_MAX'):
                plan_only([(50, 45)], **kw)
            continue
        assert plan_only([(50, 45)], **kw)['score_dtype'] == 'f64'
        okw = dict(mode=0, alntype=0, L=4, match=1., mismatch=-1., go=go + 1, ge=-1.)
        _, (got,) = emu.solve_planned([(o, m)], **okw)
        want = oracle.solve(o, m, **okw)
        assert all(got[f] == want[f] for f in FIELDS), (got, want)
    # the substitution scores count on one-diagonal bands only: 45 x 45 on diagonal 0 (span 92)
    b = (INT_MAX - 1) // 92
    q = m[:45]
    for band, mm, refused in (((0, 0), -b, False), ((0, 0), -b - 1, True), ((-1, 1), -b - 1, False), (None, -3e9, False)):
        okw = dict(mode=0 if band is None else 1, alntype=0, L=4, match=1., mismatch=float(mm), go=-1., ge=-1.)
        if band is not None:
            okw['diag_range'] = band
        if refused:
            with pytest.raises(RuntimeError, match='INT_MAX'):
                emu.solve_planned([(o[:45], q)], **okw)
            continue
        _, (got,) = emu.solve_planned([(o[:45], q)], **okw)
        want = oracle.solve(o[:45], q, **okw)
        assert all(got[f] == want[f] for f in FIELDS), (okw, got, want)
    for okw in (dict(mode=0, alntype=1), dict(mode=1, alntype=1, diag_range=(-8, 8))):
        okw.update(L=4, match=1., mismatch=-1., go=-3e9, ge=-1.)
        plan, (got,) = emu.solve_planned([(o, m)], **okw)
        assert plan['score_dtype'] == 'f64'
        want = oracle.solve(o, m, **okw)
        assert all(got[f] == want[f] for f in FIELDS), (okw, got, want)

"""The planner's `pair_keys` (pw_plan.h): the kernel that reads its letters from LDS keeps one running-best key per two cells
exactly where `lds_feed` is true -- config 2's form -- and the scores let the end-cell search tell the two cells apart:
ge < 0, go <= 0 and no entry of the substitution matrix equal to 0.  Otherwise, and under PWLIB_PAIR_KEYS=0, `k_fill16l` runs
as before.  The reported kernel name, `stamp_group` and `lds_feed` do not change.  No GPU needed."""
import pytest

from biseqt_amd.batch import plan_only

CFG2 = [(2000, 2010, -200, 200)] * 10000
BASE = dict(alnmode=1, alntype=1)
KNOBS = ('PWLIB_PAIR_KEYS', 'PWLIB_LDS_FEED', 'PWLIB_STAMP_GROUP', 'PWLIB_RAMP_BLOCKS', 'PWLIB_PACKED_BK', 'PWLIB_SIMPLE_AS_MATRIX',
         'PWLIB_NO_SCALED16', 'PWLIB_LATENCY_MODE')
NAME = 'k_fill16<8, false> x4 matrix'


def _plan(monkeypatch, match=1, mismatch=-3, go=-5, ge=-2, shapes=CFG2, env=None, **kw):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    return plan_only(shapes, match_score=match, mismatch_score=mismatch, go_score=go, ge_score=ge, ramp_free=True, stamp_group=True,
                     lds_feed=True, pair_keys=True, **dict(BASE, **kw))


def test_config_2_takes_one_key_per_two_cells(monkeypatch):
    r = _plan(monkeypatch)
    assert r['kernel'] == NAME and r['matrix'] and r['packed_rule'] == 3 and r['ramp_free'] is True and r['stamp_group'] == 4, r
    assert r['lds_feed'] is True and r['pair_keys'] is True, r
    assert _plan(monkeypatch, go=0)['pair_keys'] is True             # go = 0 is admitted: go <= 0


def test_the_knob_keeps_one_key_per_cell_and_everything_else(monkeypatch):
    r = _plan(monkeypatch, env={'PWLIB_PAIR_KEYS': '0'})
    assert r['kernel'] == NAME and r['ramp_free'] is True and r['stamp_group'] == 4 and r['lds_feed'] is True, r
    assert r['pair_keys'] is False, r
    for v in ('1', '2', ''):
        assert _plan(monkeypatch, env={'PWLIB_PAIR_KEYS': v})['pair_keys'] is True, v


def _matrix(zero):
    S = [[1.0 if i == j else -3.0 for j in range(4)] for i in range(4)]
    if zero is not None:
        S[zero[0]][zero[1]] = 0.0
    return S


@pytest.mark.parametrize('zero', [(0, 1), (3, 2), (2, 2)])
def test_off_when_one_matrix_entry_is_zero(monkeypatch, zero):
    r = _plan(monkeypatch, subst_scores=_matrix(zero))
    assert r['kernel'] == NAME and r['stamp_group'] == 4 and r['lds_feed'] is True and r['pair_keys'] is False, (zero, r)
    r = _plan(monkeypatch, subst_scores=_matrix(None))
    assert r['lds_feed'] is True and r['pair_keys'] is True, r


def test_off_when_ge_is_zero(monkeypatch):
    r = _plan(monkeypatch, ge=0)
    assert r['pair_keys'] is False and r['lds_feed'] is False, r


@pytest.mark.parametrize('why, kw', [
    ('letters through the lanes: the knob', dict(env={'PWLIB_LDS_FEED': '0'})),
    ('not ramp_free: the knob', dict(env={'PWLIB_RAMP_BLOCKS': '1'})),
    ('the stamp per block', dict(env={'PWLIB_STAMP_GROUP': '1'})),
    ('the unscaled form, rule 0', dict(env={'PWLIB_NO_SCALED16': '1'})),
    ('16 diagonals per lane', dict(shapes=[(2000, 2010, -400, 400)] * 3000)),
    ('lane-packed', dict(shapes=[(400, 390, -40, 40)] * 2000, env={'PWLIB_PACKED_BK': '8s', 'PWLIB_SIMPLE_AS_MATRIX': '1'})),
    ('several wavefronts per pair', dict(shapes=[(1700, 60, -1, 1600)] * 8, env={'PWLIB_LATENCY_MODE': '1', 'PWLIB_SIMPLE_AS_MATRIX': '1'})),
    ('the match / mismatch form', dict(shapes=[(300, 300, -10, 10)] * 20000)),
])
def test_one_condition_short_of_lds_feed(monkeypatch, why, kw):
    r = _plan(monkeypatch, **kw)
    assert r['lds_feed'] is False and r['pair_keys'] is False, (why, r)


def test_the_edges_of_the_lane_width(monkeypatch):
    for radius, want in ((200, True), (255, True), (256, False)):
        r = _plan(monkeypatch, shapes=[(2000, 2010, -radius, radius)] * 10000)
        assert r['lds_feed'] is want and r['pair_keys'] is want, (radius, r)


def test_the_key_is_not_there_unless_asked(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    r = plan_only(CFG2, match_score=1, mismatch_score=-3, go_score=-5, ge_score=-2, stamp_group=True, lds_feed=True, **BASE)
    assert 'pair_keys' not in r and r['stamp_group'] == 4 and r['lds_feed'] is True, r

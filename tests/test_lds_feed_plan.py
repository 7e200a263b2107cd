"""The planner's `lds_feed` (pw_plan.h): the grouped kernel reads its letters from LDS exactly where `stamp_group` says 4 --
config 2's form: packed rule 3, matrix form, 8 diagonals per lane, one pair per wavefront, one wavefront per pair, ramp_free
-- and keeps its edge-lane feeders as soon as one of the conditions fails and under PWLIB_LDS_FEED=0.  The reported kernel
name does not change.  No GPU needed."""
import pytest

from biseqt_amd.batch import plan_only

CFG2 = [(2000, 2010, -200, 200)] * 10000
BASE = dict(alnmode=1, alntype=1)
KNOBS = ('PWLIB_LDS_FEED', 'PWLIB_STAMP_GROUP', 'PWLIB_RAMP_BLOCKS', 'PWLIB_PACKED_BK', 'PWLIB_SIMPLE_AS_MATRIX', 'PWLIB_NO_SCALED16',
         'PWLIB_LATENCY_MODE')
NAME = 'k_fill16<8, false> x4 matrix'


def _plan(monkeypatch, match=1, mismatch=-3, go=-5, ge=-2, shapes=CFG2, env=None, **kw):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    return plan_only(shapes, match_score=match, mismatch_score=mismatch, go_score=go, ge_score=ge, ramp_free=True, stamp_group=True,
                     lds_feed=True, **dict(BASE, **kw))


def test_config_2_reads_its_letters_from_lds(monkeypatch):
    r = _plan(monkeypatch)
    assert r['kernel'] == NAME and r['matrix'] and r['packed_rule'] == 3 and r['ramp_free'] is True and r['stamp_group'] == 4, r
    assert r['lds_feed'] is True, r


def test_the_knob_keeps_the_feeders_and_the_name(monkeypatch):
    r = _plan(monkeypatch, env={'PWLIB_LDS_FEED': '0'})
    assert r['kernel'] == NAME and r['ramp_free'] is True and r['stamp_group'] == 4 and r['lds_feed'] is False, r
    for v in ('1', '2', ''):
        assert _plan(monkeypatch, env={'PWLIB_LDS_FEED': v})['lds_feed'] is True, v


@pytest.mark.parametrize('why, kw', [
    ('not ramp_free: ge = 0', dict(ge=0)),
    ('not ramp_free: the knob', dict(env={'PWLIB_RAMP_BLOCKS': '1'})),
    ('the stamp per block', dict(env={'PWLIB_STAMP_GROUP': '1'})),
    ('the unscaled form, rule 0', dict(env={'PWLIB_NO_SCALED16': '1'})),
    ('16 diagonals per lane', dict(shapes=[(2000, 2010, -400, 400)] * 3000)),
    ('lane-packed', dict(shapes=[(400, 390, -40, 40)] * 2000, env={'PWLIB_PACKED_BK': '8s', 'PWLIB_SIMPLE_AS_MATRIX': '1'})),
    ('several wavefronts per pair', dict(shapes=[(1700, 60, -1, 1600)] * 8, env={'PWLIB_LATENCY_MODE': '1', 'PWLIB_SIMPLE_AS_MATRIX': '1'})),
    ('the match / mismatch form', dict(shapes=[(300, 300, -10, 10)] * 20000)),
])
def test_one_condition_short_of_the_form(monkeypatch, why, kw):
    r = _plan(monkeypatch, **kw)
    assert r['stamp_group'] == 1 and r['lds_feed'] is False, (why, r)


def test_the_edges_of_the_lane_width(monkeypatch):
    """8 diagonals per lane, one pair per wavefront: config 2's band of 401 diagonals, the widest that fits (511), one wider."""
    for radius, want in ((200, True), (255, True), (256, False)):
        r = _plan(monkeypatch, shapes=[(2000, 2010, -radius, radius)] * 10000)
        assert (r['kernel'] == NAME) is want and r['lds_feed'] is want, (radius, r)


def test_the_key_is_not_there_unless_asked(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    r = plan_only(CFG2, match_score=1, mismatch_score=-3, go_score=-5, ge_score=-2, stamp_group=True, **BASE)
    assert 'lds_feed' not in r and r['stamp_group'] == 4, r

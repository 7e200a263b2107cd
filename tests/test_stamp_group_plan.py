"""The planner's `stamp_group` (pw_plan.h): 4 -- the grouped kernel -- for config 2's form (packed rule 3, matrix form, 8
diagonals per lane, one pair per wavefront, one wavefront per pair, ramp_free), 1 as soon as one of the conditions fails and
under PWLIB_STAMP_GROUP=1.  The reported kernel name does not change.  No GPU needed."""
from biseqt_amd.batch import plan_only

CFG2 = [(2000, 2010, -200, 200)] * 10000
BASE = dict(alnmode=1, alntype=1)
KNOBS = ('PWLIB_STAMP_GROUP', 'PWLIB_RAMP_BLOCKS', 'PWLIB_PACKED_BK', 'PWLIB_SIMPLE_AS_MATRIX', 'PWLIB_NO_SCALED16', 'PWLIB_LATENCY_MODE')


def _plan(monkeypatch, match=1, mismatch=-3, go=-5, ge=-2, shapes=CFG2, env=None, **kw):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    return plan_only(shapes, match_score=match, mismatch_score=mismatch, go_score=go, ge_score=ge, ramp_free=True, stamp_group=True,
                     **dict(BASE, **kw))


def test_config_2_takes_the_group_of_four(monkeypatch):
    r = _plan(monkeypatch)
    assert r['kernel'] == 'k_fill16<8, false> x4 matrix' and r['matrix'] and r['packed_rule'] == 3 and r['ramp_free'] is True, r
    assert r['stamp_group'] == 4, r


def test_not_ramp_free(monkeypatch):
    r = _plan(monkeypatch, ge=0)
    assert r['kernel'] == 'k_fill16<8, false> x4 matrix' and r['ramp_free'] is False and r['stamp_group'] == 1, r
    r = _plan(monkeypatch, env={'PWLIB_RAMP_BLOCKS': '1'})
    assert r['kernel'] == 'k_fill16<8, false> x4 matrix' and r['ramp_free'] is False and r['stamp_group'] == 1, r


def test_the_unscaled_form(monkeypatch):
    r = _plan(monkeypatch, env={'PWLIB_NO_SCALED16': '1'})
    assert r['kernel'] == 'k_fill16<8, false> matrix' and r['packed_rule'] == 0 and r['ramp_free'] is True, r
    assert r['stamp_group'] == 1, r


def test_sixteen_per_lane(monkeypatch):
    r = _plan(monkeypatch, shapes=[(2000, 2010, -400, 400)] * 3000)
    assert r['kernel'] == 'k_fill16<16, false> x4 matrix' and r['ramp_free'] is True and r['stamp_group'] == 1, r


def test_lane_packed(monkeypatch):
    r = _plan(monkeypatch, shapes=[(400, 390, -40, 40)] * 2000, env={'PWLIB_PACKED_BK': '8s', 'PWLIB_SIMPLE_AS_MATRIX': '1'})
    assert r['kernel'] == 'k_fill16<8, true> x4 matrix' and r['ramp_free'] is True and r['stamp_group'] == 1, r


def test_several_wavefronts_per_pair_and_the_plain_form(monkeypatch):
    r = _plan(monkeypatch, shapes=[(1700, 60, -1, 1600)] * 8, env={'PWLIB_LATENCY_MODE': '1', 'PWLIB_SIMPLE_AS_MATRIX': '1'})
    assert r['kernel'].startswith('k_fill16_mw<') and r['stamp_group'] == 1, r
    r = _plan(monkeypatch, shapes=[(300, 300, -10, 10)] * 20000)
    assert 'matrix' not in r['kernel'] and r['stamp_group'] == 1, r


def test_the_knob(monkeypatch):
    r = _plan(monkeypatch, env={'PWLIB_STAMP_GROUP': '1'})
    assert r['kernel'] == 'k_fill16<8, false> x4 matrix' and r['ramp_free'] is True and r['stamp_group'] == 1, r
    assert _plan(monkeypatch, env={'PWLIB_STAMP_GROUP': '0'})['stamp_group'] == 4
    assert _plan(monkeypatch, env={'PWLIB_STAMP_GROUP': '4'})['stamp_group'] == 4


def test_the_key_is_not_asked_for_unless_asked(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    r = plan_only(CFG2, match_score=1, mismatch_score=-3, go_score=-5, ge_score=-2, **BASE)
    assert 'stamp_group' not in r and r['matrix'] is True, r

"""The planner's `lds_exchange` (pw_plan.h): the kernel with one running-best key per two cells hands its two lane-crossing
offers on through LDS -- the kernel `k_fill16x` -- exactly where `pair_keys` is true; there is no bound of its own, the values
are the same ones.  Under PWLIB_LDS_EXCHANGE=0 `k_fill16p` runs as before.  The reported kernel name, `stamp_group`,
`lds_feed` and `pair_keys` do not change, and no older kernel's code does.  No GPU needed."""
import json
import os

import pytest

from biseqt_amd.batch import plan_only
from tests import test_pair_keys_plan as PK

CFG2 = PK.CFG2
KNOBS = ('PWLIB_LDS_EXCHANGE',) + PK.KNOBS
NAME = 'k_fill16<8, false> x4 matrix'
HERE = os.path.dirname(os.path.abspath(__file__))


def _plan(monkeypatch, match=1, mismatch=-3, go=-5, ge=-2, shapes=CFG2, env=None, **kw):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    return plan_only(shapes, match_score=match, mismatch_score=mismatch, go_score=go, ge_score=ge, ramp_free=True, stamp_group=True,
                     lds_feed=True, pair_keys=True, lds_exchange=True, **dict(PK.BASE, **kw))


def test_config_2_hands_its_offers_on_through_lds(monkeypatch):
    r = _plan(monkeypatch)
    assert r['kernel'] == NAME and r['matrix'] and r['packed_rule'] == 3 and r['ramp_free'] is True and r['stamp_group'] == 4, r
    assert r['lds_feed'] is True and r['pair_keys'] is True and r['lds_exchange'] is True, r


def test_the_knob_keeps_the_dpp_moves_and_everything_else(monkeypatch):
    r = _plan(monkeypatch, env={'PWLIB_LDS_EXCHANGE': '0'})
    assert r['kernel'] == NAME and r['ramp_free'] is True and r['stamp_group'] == 4 and r['lds_feed'] is True, r
    assert r['pair_keys'] is True and r['lds_exchange'] is False, r
    for v in ('1', '2', ''):
        assert _plan(monkeypatch, env={'PWLIB_LDS_EXCHANGE': v})['lds_exchange'] is True, v


@pytest.mark.parametrize('why, kw', [
    ('the pair keys: the knob', dict(env={'PWLIB_PAIR_KEYS': '0'})),
    ('ge = 0', dict(ge=0)),
    ('a matrix entry 0', dict(subst_scores=PK._matrix((3, 2)))),
    ('letters through the lanes: the knob', dict(env={'PWLIB_LDS_FEED': '0'})),
    ('not ramp_free: the knob', dict(env={'PWLIB_RAMP_BLOCKS': '1'})),
    ('the stamp per block', dict(env={'PWLIB_STAMP_GROUP': '1'})),
    ('the unscaled form, rule 0', dict(env={'PWLIB_NO_SCALED16': '1'})),
    ('16 diagonals per lane', dict(shapes=[(2000, 2010, -400, 400)] * 3000)),
    ('lane-packed', dict(shapes=[(400, 390, -40, 40)] * 2000, env={'PWLIB_PACKED_BK': '8s', 'PWLIB_SIMPLE_AS_MATRIX': '1'})),
    ('several wavefronts per pair', dict(shapes=[(1700, 60, -1, 1600)] * 8, env={'PWLIB_LATENCY_MODE': '1', 'PWLIB_SIMPLE_AS_MATRIX': '1'})),
    ('the match / mismatch form', dict(shapes=[(300, 300, -10, 10)] * 20000)),
])
def test_follows_pair_keys_where_they_are_off(monkeypatch, why, kw):
    r = _plan(monkeypatch, **kw)
    assert r['pair_keys'] is False and r['lds_exchange'] is False, (why, r)


@pytest.mark.parametrize('kw', [dict(), dict(go=0), dict(subst_scores=PK._matrix(None)),
                                dict(shapes=[(2000, 2010, -255, 255)] * 10000), dict(shapes=[(300, 300, -150, 150)] + [(400, 390, -20, 20)] * 64,
                                     env={'PWLIB_LATENCY_MODE': '0'})])
def test_follows_pair_keys_where_they_are_on(monkeypatch, kw):
    r = _plan(monkeypatch, **kw)
    assert r['pair_keys'] is True and r['lds_exchange'] is True, (kw, r)
    r = _plan(monkeypatch, **dict(kw, env=dict(kw.get('env', {}), PWLIB_LDS_EXCHANGE='0')))
    assert r['pair_keys'] is True and r['lds_exchange'] is False, (kw, r)


def test_the_key_is_not_there_unless_asked(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    r = plan_only(CFG2, match_score=1, mismatch_score=-3, go_score=-5, ge_score=-2, pair_keys=True, **PK.BASE)
    assert 'lds_exchange' not in r and r['pair_keys'] is True, r


def test_every_older_kernel_keeps_its_code():
    """tests/golden/kernel_hashes_before_lds_exchange.json: the fingerprints of the build before this kernel existed (the ninth
    template argument of WaveFill16 and the offer functions changed no instruction of any other kernel).  A later change that
    means to alter one of those kernels replaces the file with the build's kernel_hashes.json, less this kernel's entry."""
    from biseqt_amd.csrc import build as B
    B.build(verbose=False)
    with open(os.path.join(B.OUT_DIR, 'kernel_hashes.json')) as f:
        now = json.load(f)
    with open(os.path.join(HERE, 'golden', 'kernel_hashes_before_lds_exchange.json')) as f:
        before = json.load(f)
    assert len(before) >= 27
    assert {k: now.get(k) for k in before} == before
    assert sorted(set(now) - set(before)) == ['void pw::k_fill16x<8, false, 3, true>(pw::FillParams<int>)']

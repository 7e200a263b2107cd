"""The planner's `ramp_free` (pw_plan.h): true for config 2 and its linear-gap rerun, false one step past each of its three
bounds -- where the plan still names a packed kernel -- and false under PWLIB_RAMP_BLOCKS=1.  No GPU needed."""
import pytest

from biseqt_amd.batch import plan_only
from tests import ramp_free_cases as RC

CFG2 = [(2000, 2010, -200, 200)] * 10000
BASE = dict(alnmode=1, alntype=1)


def _plan(match, mismatch, go, ge, shapes=CFG2, **kw):
    return plan_only(shapes, match_score=match, mismatch_score=mismatch, go_score=go, ge_score=ge, ramp_free=True, **dict(BASE, **kw))


def test_config_2_and_its_linear_gap_rerun_are_ramp_free():
    for go, ge in ((-5, -2), (0, -2)):
        r = _plan(1, -3, go, ge)
        assert r['kernel'] == 'k_fill16<8, false> x4 matrix' and r['matrix'] and r['packed_rule'] == 3, r
        assert r['ramp_free'] is True, r


@pytest.mark.parametrize('sset', RC.REFUSED_SETS, ids=[s[0] for s in RC.REFUSED_SETS])
def test_one_step_past_each_bound_is_refused_and_stays_packed(sset):
    _, match, mismatch, go, ge = sset
    assert not RC.ramp_free(mismatch, go, ge)
    r = _plan(match, mismatch, go, ge)
    assert r['ramp_free'] is False, r
    assert r['kernel'].startswith('k_fill16<') and r['packed_rule'] in (0, 3), r
    # ... and the neighbour inside the bound, on the same kernel, is taken
    inside = _plan(match, min(mismatch, -1), go, min(ge, -1))
    assert inside['ramp_free'] is True and inside['kernel'] == r['kernel'], (inside, r)


def test_a_matrix_whose_minimum_is_zero_is_refused():
    S = [[2, 0, 1, 0], [0, 2, 0, 1], [1, 0, 2, 0], [0, 1, 0, 2]]
    r = plan_only(CFG2[:1000], subst_scores=S, go_score=-5, ge_score=-2, ramp_free=True, **BASE)
    assert r['kernel'].startswith('k_fill16<') and r['matrix'] and r['ramp_free'] is False, r
    S[0][1] = -1
    r = plan_only(CFG2[:1000], subst_scores=S, go_score=-5, ge_score=-2, ramp_free=True, **BASE)
    assert r['matrix'] and r['ramp_free'] is True, r


@pytest.mark.parametrize('sset', RC.SCORE_SETS, ids=[s[0] for s in RC.SCORE_SETS])
def test_the_score_sets_the_kernel_tests_run_are_admitted(sset):
    match = RC.match_of(sset, True, 2000, 2010)
    assert RC.ramp_free(sset[2], sset[3], sset[4])
    r = _plan(match, sset[2], sset[3], sset[4])
    assert r['matrix'] and r['ramp_free'] is True, r


def test_the_knob_turns_it_off(monkeypatch):
    monkeypatch.setenv('PWLIB_RAMP_BLOCKS', '1')
    r = _plan(1, -3, -5, -2)
    assert r['kernel'] == 'k_fill16<8, false> x4 matrix' and r['ramp_free'] is False, r
    monkeypatch.setenv('PWLIB_RAMP_BLOCKS', '0')
    assert _plan(1, -3, -5, -2)['ramp_free'] is True


def test_only_the_forms_with_a_loop_per_block_kind_report_it():
    """The plain (match / mismatch) form, the lane-packed plain form, the rules that begin on the table edge and the 32-bit
    kernels keep their bodies."""
    cfg = (1, -3, -5, -2)
    assert _plan(*cfg, shapes=[(300, 300, -10, 10)] * 20000)['ramp_free'] is False          # k_fill16<4, true> x4: plain form
    assert _plan(*cfg, alntype=2)['ramp_free'] is False                                      # the overlap rule
    assert plan_only([(1000, 1000)] * 5000, alnmode=0, alntype=0, match_score=1, mismatch_score=-3, go_score=-5,
                     ge_score=-2, ramp_free=True)['ramp_free'] is False                                      # GLOBAL, matrix form, rule 2
    r = _plan(100, -300, -500, -200)
    assert 'k_fill16' not in r['kernel'] and r['ramp_free'] is False, r
    # the wider matrix-form layouts of the local rule take it too
    r = _plan(*cfg, shapes=[(2000, 2010, -400, 400)] * 3000)
    assert r['kernel'] == 'k_fill16<16, false> x4 matrix' and r['ramp_free'] is True, r


def test_baseline_configs_are_unchanged():
    """tests/test_planner.py::test_baseline_configs runs as it stands."""
    from tests.test_planner import test_baseline_configs
    test_baseline_configs()

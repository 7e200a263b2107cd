"""ramp_free on the GPU: the packed matrix form of the local rules with its start and end blocks on the steady body
(pw_wave.h, WaveFill16::RAMPF; pw_plan.h, ramp_free).

The score sets and shapes of tests/ramp_free_cases.py in small batches, alongside 64 pairs of 400 x 390 with band radius 40,
on every layout of the form: one pair per wavefront at 8 diagonals per lane (config 2's kernel) and at 28, lane-packed, and
several wavefronts per pair; scores times 4 (rule 3) and as given (rule 0).  Each batch runs once as planned and once with
PWLIB_RAMP_BLOCKS=1 (the four loops' old split): records, transcripts and every pair's tie masks must be equal between the
two and equal to the 32-bit kernels' (bits 0-2: the packed kernels store no M bit, go <= 0); a sample of pairs is held to
the oracle.  The score sets the predicate refuses run the same way (both runs then take the old split).
"""
import numpy as np
import pytest

from tests import ramp_free_cases as RC

SHAPES = RC.shapes()
SMALL = [s for s in SHAPES if s[0] != 'wait1600' and not s[0].startswith('bulk')]
WIDE = [s for s in SHAPES if s[0] in ('wait1600', 'X<<Y', 'mid-block')]
FIELDS = ('score', 'opt_i', 'opt_j', 'origin_idx', 'mutant_idx', 'tx_len', 'status')


def _wide_pair():
    """301 diagonals: the batch takes 8 diagonals per lane, one pair per wavefront."""
    rng = np.random.default_rng(78)
    o = rng.integers(0, 4, 300).astype(np.uint8)
    m = o.copy()
    m[::7] = (m[::7] + 1) % 4
    return ('band301', o, m, (-150, 150))


# (id, pairs, environment, kernel as planned with scores times 4 / as given)
LAYOUTS = [
    ('wave-bk8', SMALL + [_wide_pair()] + RC.bulk(), {}, 'k_fill16<8, false> x4 matrix', 'k_fill16<8, false> matrix'),
    ('lanes-bk8', SMALL + RC.bulk(), {'PWLIB_PACKED_BK': '8s', 'PWLIB_SIMPLE_AS_MATRIX': '1'},
     'k_fill16<8, true> x4 matrix', 'k_fill16<8, true> matrix'),
    ('wave-bk28', WIDE + RC.bulk(), {'PWLIB_LATENCY_MODE': '0', 'PWLIB_SIMPLE_AS_MATRIX': '1'},
     'k_fill16<28, false> x4 matrix', 'k_fill16<28, false> matrix'),
    ('workgroup', WIDE + RC.bulk(), {'PWLIB_LATENCY_MODE': '1', 'PWLIB_SIMPLE_AS_MATRIX': '1'},
     'k_fill16_mw<4, 3> x 7 wavefronts matrix', 'k_fill16_mw<4, 0> x 7 wavefronts matrix'),
]
ORACLE_SAMPLE = 12        # pairs per batch held to the oracle: every named shape and some of the 64


def _scoring(sset, x4, pairs):
    n = max(min(len(o), len(m)) for _, o, m, _ in pairs)
    match = RC.match_of(sset, x4, n, n)
    return dict(alnmode=1, alntype=RC.B_LOCAL, alphabet_len=4, match_score=match, mismatch_score=sset[2], go_score=sset[3],
                ge_score=sset[4])


def _env(monkeypatch, env, x4, knob):
    for k in ('PWLIB_PACKED_BK', 'PWLIB_SIMPLE_AS_MATRIX', 'PWLIB_LATENCY_MODE', 'PWLIB_NO_SCALED16', 'PWLIB_RAMP_BLOCKS'):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    if not x4:
        monkeypatch.setenv('PWLIB_NO_SCALED16', '1')
    if knob:
        monkeypatch.setenv('PWLIB_RAMP_BLOCKS', '1')


@pytest.mark.parametrize('x4', [True, False], ids=['x4', 'x1'])
@pytest.mark.parametrize('layout', LAYOUTS, ids=[l[0] for l in LAYOUTS])
@pytest.mark.parametrize('sset', RC.SCORE_SETS + RC.REFUSED_SETS, ids=[s[0] for s in RC.SCORE_SETS + RC.REFUSED_SETS])
def test_the_planner_reaches_the_form(sset, layout, x4, monkeypatch):
    """(No GPU.)  Every batch of the GPU test below is planned onto the kernel it names, with ramp_free as the predicate says
    and off under the knob."""
    from biseqt_amd.batch import plan_only
    lid, pairs, env, name4, name1 = layout
    sc = _scoring(sset, x4, pairs)
    shapes = [(len(o), len(m)) + tuple(band) for _, o, m, band in pairs]
    admitted = RC.ramp_free(sset[2], sset[3], sset[4])
    for knob in (False, True):
        _env(monkeypatch, env, x4, knob)
        p = plan_only(shapes, ramp_free=True, **sc)
        assert p['kernel'] == (name4 if x4 else name1), (lid, p)
        assert p['ramp_free'] is (admitted and not knob), (lid, knob, p)


_ORACLE = {}


def _oracle(oracle, sid, o, m, okw):
    """The oracle's answer and whole plane, computed once per problem and scoring."""
    key = (sid, o.tobytes(), m.tobytes(), okw['match'], okw['mismatch'], okw['go'], okw['ge'])
    if key not in _ORACLE:
        _ORACLE[key] = oracle.solve(o, m, want_table=True, **okw)
    return _ORACLE[key]


def _run(pairs, sc, flags=0):
    from biseqt_amd.batch import BatchAligner
    with BatchAligner([(o, m) for _, o, m, _ in pairs], diag_range=[band for _, _, _, band in pairs], check_band=False,
                      flags=flags, **sc) as b:
        name = b.kernel_name
        res = b.run()
        txs = b.transcripts(res)
        masks = [b.masks(k) for k in range(len(pairs))]
    return name, res, txs, masks


@pytest.mark.gpu
@pytest.mark.parametrize('x4', [True, False], ids=['x4', 'x1'])
@pytest.mark.parametrize('layout', LAYOUTS, ids=[l[0] for l in LAYOUTS])
@pytest.mark.parametrize('sset', RC.SCORE_SETS + RC.REFUSED_SETS, ids=[s[0] for s in RC.SCORE_SETS + RC.REFUSED_SETS])
def test_both_paths_equal_each_other_the_32_bit_kernels_and_the_oracle(sset, layout, x4, oracle, monkeypatch):
    from biseqt_amd import _pwlib as W
    lid, pairs, env, name4, name1 = layout
    sc = _scoring(sset, x4, pairs)
    _env(monkeypatch, env, x4, False)
    name, res, txs, masks = _run(pairs, sc)
    assert name == (name4 if x4 else name1), (lid, name)
    _env(monkeypatch, env, x4, True)
    kname, kres, ktxs, kmasks = _run(pairs, sc)
    assert kname == name
    wname, wres, wtxs, wmasks = _run(pairs, sc, flags=W.PW_FLAG_NO_PACKED16)
    assert wname.startswith('k_fill<int') or wname.startswith('k_fill_mw<int'), wname
    label = '%s %s on %s' % (sset[0], lid, name)
    for f in FIELDS:
        assert np.array_equal(res[f], kres[f]), (label, 'knob', f, np.nonzero(res[f] != kres[f])[0][:8])
        assert np.array_equal(res[f], wres[f]), (label, '32-bit', f, np.nonzero(res[f] != wres[f])[0][:8])
    assert txs == ktxs and txs == wtxs, label
    for k in range(len(pairs)):
        assert np.array_equal(masks[k], kmasks[k]), (label, 'knob', k, pairs[k][0])
        assert np.array_equal(masks[k] & 7, wmasks[k] & 7), (label, '32-bit', k, pairs[k][0])
    # the oracle: every named shape and a few of the 64
    okw = dict(mode=1, alntype=RC.B_LOCAL, L=4, match=float(sc['match_score']), mismatch=float(sc['mismatch_score']),
               go=float(sc['go_score']), ge=float(sc['ge_score']))
    named = [k for k, p in enumerate(pairs) if p[0] != 'bulk']
    sample = named + [k for k, p in enumerate(pairs) if p[0] == 'bulk'][:max(2, ORACLE_SAMPLE - len(named))]
    for k in sample:
        sid, o, m, band = pairs[k]
        want = _oracle(oracle, sid, o, m, dict(okw, diag_range=band))
        assert want['init_rc'] == 0
        assert masks[k].shape == want['mask'].shape, (label, sid)
        bad = np.nonzero((masks[k] & 7) != (want['mask'] & 7))[0]
        assert bad.size == 0, (label, sid, '%d of %d cells differ' % (bad.size, masks[k].size), bad[:8].tolist())
        assert (int(res['opt_i'][k]), int(res['opt_j'][k])) == tuple(want['opt']), (label, sid)
        if want['opt'][0] >= 0:
            assert float(res['score'][k]) == want['score'], (label, sid)
            assert (txs[k] or None) == (want['transcript'] or None), (label, sid)
            if want['transcript']:
                assert (int(res['origin_idx'][k]), int(res['mutant_idx'][k])) == (want['origin_idx'], want['mutant_idx']), (label, sid)

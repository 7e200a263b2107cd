"""The stamp group of the running best on the GPU (pw_wave.h, WaveFill16, GRP; pw_plan.h, stamp_group): the grouped kernel
`k_fill16g<8, false, 3, true>` against the per-block kernel it stands beside.

The shapes of tests/stamp_group_cases.py beside 64 pairs of 400 x 390 in one batch, and the pair whose best score is 2047 in a
batch of its own scoring.  Each batch runs as planned (group 4), with PWLIB_STAMP_GROUP=1 (the per-block kernel) and on the
32-bit kernels: records and transcripts must be equal among the three, a sample of pairs is held to the oracle, and the
kernel name is the same with the knob on and off.
"""
import numpy as np
import pytest

from tests import ramp_free_cases as RC
from tests import stamp_group_cases as SC

FIELDS = ('score', 'opt_i', 'opt_j', 'origin_idx', 'mutant_idx', 'tx_len', 'status')
NAME = 'k_fill16<8, false> x4 matrix'
B_LOCAL = 1


def _wide_pair():
    """301 diagonals: the batch takes 8 diagonals per lane, one pair per wavefront."""
    rng = np.random.default_rng(78)
    o = rng.integers(0, 4, 300).astype(np.uint8)
    m = o.copy()
    m[::7] = (m[::7] + 1) % 4
    return ('band301', o, m, (-150, 150))


# (id, pairs, scoring of the batch, the oracle's scoring)
BATCHES = [
    ('cfg2', SC.shapes() + [_wide_pair()] + RC.bulk(),
     dict(alnmode=1, alntype=B_LOCAL, alphabet_len=4, match_score=1, mismatch_score=-3, go_score=-5, ge_score=-2),
     dict(mode=1, alntype=B_LOCAL, L=4, subst=SC.cfg2_matrix(), go=-5., ge=-2.)),
    ('best2047', [SC.top_shape()] * 3,
     dict(alnmode=1, alntype=B_LOCAL, alphabet_len=4, subst_scores=SC.top_matrix(), go_score=-5, ge_score=-2),
     dict(mode=1, alntype=B_LOCAL, L=4, subst=SC.top_matrix(), go=-5., ge=-2.)),
]


def _env(monkeypatch, knob):
    for k in ('PWLIB_STAMP_GROUP', 'PWLIB_RAMP_BLOCKS', 'PWLIB_PACKED_BK', 'PWLIB_SIMPLE_AS_MATRIX', 'PWLIB_NO_SCALED16'):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv('PWLIB_LATENCY_MODE', '0')
    if knob:
        monkeypatch.setenv('PWLIB_STAMP_GROUP', '1')


@pytest.mark.parametrize('batch', BATCHES, ids=[b[0] for b in BATCHES])
def test_the_planner_reaches_the_form(batch, monkeypatch):
    """(No GPU.)  Both batches of the GPU test are planned onto the grouped kernel, and onto the per-block one under the knob."""
    from biseqt_amd.batch import plan_only
    bid, pairs, sc, _ = batch
    shapes = [(len(o), len(m)) + tuple(band) for _, o, m, band in pairs]
    for knob in (False, True):
        _env(monkeypatch, knob)
        p = plan_only(shapes, ramp_free=True, stamp_group=True, **sc)
        assert p['kernel'] == NAME and p['ramp_free'] is True and p['stamp_group'] == (1 if knob else 4), (bid, knob, p)


def _run(pairs, sc, flags=0):
    from biseqt_amd.batch import BatchAligner
    with BatchAligner([(o, m) for _, o, m, _ in pairs], diag_range=[band for _, _, _, band in pairs], check_band=False,
                      flags=flags, **sc) as b:
        name = b.kernel_name
        res = b.run().copy()
        txs = b.transcripts(res)
    return name, res, txs


@pytest.mark.gpu
@pytest.mark.parametrize('batch', BATCHES, ids=[b[0] for b in BATCHES])
def test_grouped_per_block_and_32_bit_kernels_agree_and_equal_the_oracle(batch, oracle, monkeypatch):
    from biseqt_amd import _pwlib as W
    bid, pairs, sc, okw = batch
    _env(monkeypatch, False)
    name, res, txs = _run(pairs, sc)
    _env(monkeypatch, True)
    kname, kres, ktxs = _run(pairs, sc)
    assert name == NAME and kname == NAME, (name, kname)
    wname, wres, wtxs = _run(pairs, sc, flags=W.PW_FLAG_NO_PACKED16)
    assert wname.startswith('k_fill<int'), wname
    for f in FIELDS:
        assert np.array_equal(res[f], kres[f]), (bid, 'per block', f, [pairs[k][0] for k in np.nonzero(res[f] != kres[f])[0][:8]])
        assert np.array_equal(res[f], wres[f]), (bid, '32-bit', f, [pairs[k][0] for k in np.nonzero(res[f] != wres[f])[0][:8]])
    assert txs == ktxs and txs == wtxs, bid
    # the oracle: every named shape and four of the 64
    named = [k for k, p in enumerate(pairs) if p[0] != 'bulk']
    seen = set()
    for k in named + [k for k, p in enumerate(pairs) if p[0] == 'bulk'][:4]:
        sid, o, m, band = pairs[k]
        if sid in seen and sid != 'bulk':
            continue
        seen.add(sid)
        want = oracle.solve(o, m, diag_range=band, **okw)
        assert want['init_rc'] == 0
        assert (int(res['opt_i'][k]), int(res['opt_j'][k])) == tuple(want['opt']), (bid, sid)
        if want['opt'][0] >= 0:
            assert float(res['score'][k]) == want['score'], (bid, sid)
            assert (txs[k] or None) == (want['transcript'] or None), (bid, sid)
            if want['transcript']:
                assert (int(res['origin_idx'][k]), int(res['mutant_idx'][k])) == (want['origin_idx'], want['mutant_idx']), (bid, sid)
    if bid == 'best2047':
        assert float(res['score'][0]) == 2047.0

"""The lane-crossing offers handed on through LDS, on the GPU (pw_wave.h, WaveFill16, XLDS, offer_up / offer_left; pw_plan.h,
lds_exchange): the kernel `k_fill16x<8, false, 3, true>` against the kernel it stands beside and the 32-bit kernels.

Two batches, config 2's scores and a 4 x 4 matrix with positive entries off its diagonal.  Every batch runs as planned (offers
through LDS), with PWLIB_LDS_EXCHANGE=0 (`k_fill16p`, DPP moves) and on the 32-bit kernels (PW_FLAG_NO_PACKED16): records,
transcripts and every pair's whole tie-mask plane must be equal among the three (bits 0-2: the packed kernels store no M bit,
go <= 0); every named shape and a sample of the 64 are held to the oracle -- record, transcript, whole plane; the kernel name
is the same with the knob on and off.  The named shapes are the smallest at which the exchange can go wrong:
  * 400 x 390 at radius 20: 41 diagonals on 6 lanes -- the last active lane's right neighbour is a spare lane;
  * 400 x 390 at radius 200: 401 diagonals on 51 lanes, config 2's layout;
  * bands of exactly 512 and of 505 diagonals: lane 63 is in use and takes the seed of the left offers, lane 0 that of the up
    offers;
  * a pair shorter than one block; 400 x 24 and 24 x 400;
  * 1200 x 1190 at radius 200: the letter rings wrap more than twice, and the stamp and restage sections lie between exchanges;
  * 64 pairs of 400 x 390 in one batch.
One more run of the first batch, the 64 pairs among them, reads the same letters from a caller-owned arena whose last frame
ends it.
"""
import numpy as np
import pytest

from tests import pair_keys_cases as PC
from tests import ramp_free_cases as RC
from tests import stamp_group_cases as SC

FIELDS = ('score', 'opt_i', 'opt_j', 'origin_idx', 'mutant_idx', 'tx_len', 'status')
NAME = 'k_fill16<8, false> x4 matrix'
B_LOCAL = 1
KNOBS = ('PWLIB_LDS_EXCHANGE', 'PWLIB_PAIR_KEYS', 'PWLIB_LDS_FEED', 'PWLIB_STAMP_GROUP', 'PWLIB_RAMP_BLOCKS', 'PWLIB_PACKED_BK',
         'PWLIB_SIMPLE_AS_MATRIX', 'PWLIB_NO_SCALED16')
ORACLE_BULK = 2           # of the 64 pairs; every named shape is held to the oracle


def _related(seed, X, Y):
    rng = np.random.default_rng(seed)
    o = RC._rand(rng, max(X, Y))
    m = RC._mutate(rng, o)
    if X > 40 and Y > 40:
        m = np.delete(m, [17, 18, 90, 91, 92][:5])
        m = np.concatenate([m, RC._rand(rng, max(X, Y))])
    return o[:X].copy(), m[:Y].copy()


def named_shapes():
    by = {s[0]: s for s in SC.shapes()}
    out = [by['400x390-r20'], by['400x390-r200']]
    o, m = _related(512, 300, 290)
    out.append(('band512', o, m, (-256, 255)))
    out.append(('band505', o, m, (-252, 252)))
    out.append(by['short'])
    o, m = _related(24, 400, 24)
    out.append(('400x24', o, m, (-200, 200)))
    out.append(('24x400', m, o, (-200, 200)))
    o, m = _related(1200, 1200, 1190)
    out.append(('1200x1190-r200', o, m, (-200, 200)))
    return out


def _batches():
    """[(id, pairs, scoring of the batch, the oracle's scoring)]"""
    pairs = named_shapes() + RC.bulk()
    out = []
    for bid, S, go, ge in (('cfg2', PC.cfg2_matrix(), PC.CFG2[2], PC.CFG2[3]), ('mixed', PC.mixed_matrix(), -5., -2.)):
        # (rule 3 holds scores below 2048: under the matrix whose match is 5 the pair of 1190 letters is left out)
        out.append((bid, [q for q in pairs if bid == 'cfg2' or len(q[1]) <= 400], dict(alnmode=1, alntype=B_LOCAL, alphabet_len=4, subst_scores=S, go_score=go, ge_score=ge),
                    dict(mode=1, alntype=B_LOCAL, L=4, subst=S, go=go, ge=ge)))
    return out


BATCHES = _batches()
IDS = [b[0] for b in BATCHES]


def _env(monkeypatch, knob):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv('PWLIB_LATENCY_MODE', '0')
    if knob:
        monkeypatch.setenv('PWLIB_LDS_EXCHANGE', '0')


def test_the_batches_are_what_they_say():
    pairs = BATCHES[0][1]
    assert len(pairs) == 8 + 64 and [p[0] for p in pairs[8:]] == ['bulk'] * 64
    assert BATCHES[1][1] == pairs[:7] + pairs[8:]
    lanes = {}
    for sid, o, m, band in pairs[:8]:
        dmin, dmax = max(band[0], -len(m)), min(band[1], len(o))
        lanes[sid] = (dmax - dmin + 1, -(-(dmax - dmin + 1) // 8))
    assert lanes['400x390-r20'] == (41, 6) and lanes['400x390-r200'] == (401, 51), lanes
    assert lanes['band512'] == (512, 64) and lanes['band505'] == (505, 64), lanes
    assert PC.nblocks(pairs[4]) == 1 and PC.nblocks(pairs[7]) > 2 * 64 + 8, (PC.nblocks(pairs[4]), PC.nblocks(pairs[7]))
    assert [(len(p[1]), len(p[2])) for p in pairs[5:8]] == [(400, 24), (24, 400), (1200, 1190)]
    S = BATCHES[1][2]['subst_scores']
    assert all(v != 0 for row in S for v in row) and any(S[i][j] > 0 for i in range(4) for j in range(4) if i != j)


@pytest.mark.parametrize('batch', BATCHES, ids=IDS)
def test_the_planner_reaches_the_form(batch, monkeypatch):
    """(No GPU.)  Every batch of the GPU tests is planned onto the kernel with its offers through LDS, and onto the one beside
    it under the knob."""
    from biseqt_amd.batch import plan_only
    bid, pairs, sc, _ = batch
    shapes = [(len(o), len(m)) + tuple(band) for _, o, m, band in pairs]
    for knob in (False, True):
        _env(monkeypatch, knob)
        p = plan_only(shapes, ramp_free=True, stamp_group=True, lds_feed=True, pair_keys=True, lds_exchange=True, **sc)
        assert p['kernel'] == NAME and p['ramp_free'] is True and p['stamp_group'] == 4 and p['lds_feed'] is True, (bid, knob, p)
        assert p['pair_keys'] is True and p['lds_exchange'] is (not knob), (bid, knob, p)


def _collect(b, n):
    res = b.run().copy()
    return b.kernel_name, res, b.transcripts(res), [b.masks(k) for k in range(n)]


def _run(batch, flags=0):
    from biseqt_amd.batch import BatchAligner
    _, pairs, sc, _ = batch
    with BatchAligner([(o, m) for _, o, m, _ in pairs], diag_range=[band for _, _, _, band in pairs], check_band=False,
                      flags=flags, **sc) as b:
        return _collect(b, len(pairs))


_REF = {}


def _reference(batch):
    """The 32-bit kernels' answer, computed once per batch."""
    from biseqt_amd import _pwlib as W
    if batch[0] not in _REF:
        name, res, txs, masks = _run(batch, W.PW_FLAG_NO_PACKED16)
        assert name.startswith('k_fill<int') or name.startswith('k_fill_mw<int'), name
        _REF[batch[0]] = dict(res=res, txs=txs, masks=masks)
    return _REF[batch[0]]


def _same_as_reference(label, batch, res, txs, masks):
    ref, pairs = _reference(batch), batch[1]
    for f in FIELDS:
        assert np.array_equal(res[f], ref['res'][f]), (label, f, [pairs[k][0] for k in np.nonzero(res[f] != ref['res'][f])[0][:8]])
    assert txs == ref['txs'], label
    for k in range(len(pairs)):
        assert np.array_equal(masks[k] & 7, ref['masks'][k] & 7), (label, k, pairs[k][0])


@pytest.mark.gpu
@pytest.mark.parametrize('batch', BATCHES, ids=IDS)
def test_offers_through_lds_equal_the_32_bit_kernels_and_the_oracle(batch, oracle, monkeypatch):
    bid, pairs, sc, okw = batch
    _env(monkeypatch, False)
    name, res, txs, masks = _run(batch)
    assert name == NAME, name
    _same_as_reference(bid + ': offers through LDS', batch, res, txs, masks)
    named = [k for k, p in enumerate(pairs) if p[0] != 'bulk']
    for k in named + [k for k, p in enumerate(pairs) if p[0] == 'bulk'][:ORACLE_BULK]:
        sid, o, m, band = pairs[k]
        want = oracle.solve(o, m, want_table=True, diag_range=band, **okw)
        assert want['init_rc'] == 0 and masks[k].shape == want['mask'].shape, sid
        bad = np.nonzero((masks[k] & 7) != (want['mask'] & 7))[0]
        assert bad.size == 0, (sid, '%d of %d cells differ' % (bad.size, masks[k].size), bad[:8].tolist())
        assert (int(res['opt_i'][k]), int(res['opt_j'][k])) == tuple(want['opt']), sid
        if want['opt'][0] >= 0:
            assert float(res['score'][k]) == want['score'], sid
            assert (txs[k] or None) == (want['transcript'] or None), sid
            if want['transcript']:
                assert (int(res['origin_idx'][k]), int(res['mutant_idx'][k])) == (want['origin_idx'], want['mutant_idx']), sid


@pytest.mark.gpu
@pytest.mark.parametrize('batch', BATCHES, ids=IDS)
def test_the_knob_keeps_the_dpp_moves_and_the_name(batch, monkeypatch):
    _env(monkeypatch, True)
    name, res, txs, masks = _run(batch)
    assert name == NAME, name
    _same_as_reference(batch[0] + ': offers by DPP moves', batch, res, txs, masks)


@pytest.mark.gpu
def test_caller_owned_arena_whose_last_frame_ends_the_arena(monkeypatch):
    from biseqt_amd.batch import BatchAligner, DeviceArena
    batch = BATCHES[0]
    _, pairs, sc, _ = batch
    _env(monkeypatch, False)
    reads = [np.asarray(s, np.uint8) for _, o, m, _ in pairs for s in (o, m)]
    lens = np.array([len(r) for r in reads], np.int64)
    offs = np.concatenate([[0], np.cumsum((lens + 3) // 4 * 4)[:-1]]).astype(np.int64)
    arena = np.full(int(offs[-1] + lens[-1]), 0xee, np.uint8)       # the last frame ends the arena; 0xee is no letter
    for r, o in zip(reads, offs):
        arena[o:o + len(r)] = r
    idx = np.arange(2 * len(pairs)).reshape(-1, 2)
    with DeviceArena(arena) as dev:                                  # (allocates arena.nbytes + 16)
        with BatchAligner.from_arena(arena, offs, lens, idx, diag_ranges=[band for _, _, _, band in pairs], device_arena=dev,
                                     check_band=False, **sc) as b:
            name, res, txs, masks = _collect(b, len(pairs))
    assert name == NAME, name
    _same_as_reference('caller-owned arena', batch, res, txs, masks)

"""The letter rings on the GPU (pw_wave.h, WaveFill16, LDSF; pw_plan.h, lds_feed): the kernel `k_fill16l<8, false, 3, true>`
against the grouped kernel it stands beside.

The shapes of tests/lds_feed_cases.py -- the pair whose rings wrap more than twice among them -- in ONE batch beside 64 pairs of
400 x 390.  The batch runs as planned (letters from LDS), with PWLIB_LDS_FEED=0 (the grouped kernel with its edge-lane
feeders) and on the 32-bit kernels (PW_FLAG_NO_PACKED16): records, transcripts and every pair's whole tie-mask plane must be
equal among the three (bits 0-2: the packed kernels store no M bit, go <= 0); every named shape and a sample of the 64 are held
to the oracle -- record, transcript, whole plane; the kernel name is the same with the knob on and off.  One more run reads the
same letters from a caller-owned arena (PW_FLAG_SHARED_ARENA) laid out as tight as the API allows -- frames on 4-byte
boundaries, the first at offset 0, the last ending exactly at arena_bytes, the allocation exactly arena_bytes + 16 -- and must
compute the same.
"""
import numpy as np
import pytest

from tests import lds_feed_cases as LC
from tests import ramp_free_cases as RC

FIELDS = ('score', 'opt_i', 'opt_j', 'origin_idx', 'mutant_idx', 'tx_len', 'status')
NAME = 'k_fill16<8, false> x4 matrix'
B_LOCAL = 1
SC = dict(alnmode=1, alntype=B_LOCAL, alphabet_len=4, match_score=1, mismatch_score=-3, go_score=-5, ge_score=-2)
OKW = dict(mode=1, alntype=B_LOCAL, L=4, match=1., mismatch=-3., go=-5., ge=-2.)
KNOBS = ('PWLIB_LDS_FEED', 'PWLIB_STAMP_GROUP', 'PWLIB_RAMP_BLOCKS', 'PWLIB_PACKED_BK', 'PWLIB_SIMPLE_AS_MATRIX', 'PWLIB_NO_SCALED16')
ORACLE_BULK = 2           # of the 64 pairs; every named shape is held to the oracle


def _wide_pair():
    """301 diagonals: the batch takes 8 diagonals per lane, one pair per wavefront."""
    rng = np.random.default_rng(78)
    o = rng.integers(0, 4, 300).astype(np.uint8)
    m = o.copy()
    m[::7] = (m[::7] + 1) % 4
    return ('band301', o, m, (-150, 150))


# the first pair's origin (1200 letters, offset 0 of the tight arena); the last pair's mutant (17 letters) ends the arena
_SHAPES = LC.shapes()
PAIRS = [LC.long_shape(), _wide_pair()] + _SHAPES[17:] + RC.bulk() + _SHAPES[:17]


def _env(monkeypatch, knob):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv('PWLIB_LATENCY_MODE', '0')
    if knob:
        monkeypatch.setenv('PWLIB_LDS_FEED', '0')


def test_the_planner_reaches_the_form(monkeypatch):
    """(No GPU.)  The batch of the GPU tests is planned onto the kernel that reads LDS, and onto the grouped one under the knob."""
    from biseqt_amd.batch import plan_only
    shapes = [(len(o), len(m)) + tuple(band) for _, o, m, band in PAIRS]
    for knob in (False, True):
        _env(monkeypatch, knob)
        p = plan_only(shapes, ramp_free=True, stamp_group=True, lds_feed=True, **SC)
        assert p['kernel'] == NAME and p['ramp_free'] is True and p['stamp_group'] == 4 and p['lds_feed'] is (not knob), (knob, p)
    assert PAIRS[0][0] == '1200x1190-r200' and PAIRS[-1][0] == 'len17'


def _collect(b):
    res = b.run().copy()
    return b.kernel_name, res, b.transcripts(res), [b.masks(k) for k in range(len(PAIRS))]


def _run(flags=0):
    from biseqt_amd.batch import BatchAligner
    with BatchAligner([(o, m) for _, o, m, _ in PAIRS], diag_range=[band for _, _, _, band in PAIRS], check_band=False,
                      flags=flags, **SC) as b:
        return _collect(b)


_REF = {}


def _reference():
    """The 32-bit kernels' answer, computed once."""
    from biseqt_amd import _pwlib as W
    if not _REF:
        name, res, txs, masks = _run(W.PW_FLAG_NO_PACKED16)
        assert name.startswith('k_fill<int') or name.startswith('k_fill_mw<int'), name
        _REF.update(res=res, txs=txs, masks=masks)
    return _REF


def _same_as_reference(label, res, txs, masks):
    ref = _reference()
    for f in FIELDS:
        assert np.array_equal(res[f], ref['res'][f]), (label, f, [PAIRS[k][0] for k in np.nonzero(res[f] != ref['res'][f])[0][:8]])
    assert txs == ref['txs'], label
    for k in range(len(PAIRS)):
        assert np.array_equal(masks[k] & 7, ref['masks'][k] & 7), (label, k, PAIRS[k][0])


@pytest.mark.gpu
def test_letters_from_lds_equal_the_32_bit_kernels_and_the_oracle(oracle, monkeypatch):
    _env(monkeypatch, False)
    name, res, txs, masks = _run()
    assert name == NAME, name
    _same_as_reference('letters from LDS', res, txs, masks)
    named = [k for k, p in enumerate(PAIRS) if p[0] != 'bulk']
    for k in named + [k for k, p in enumerate(PAIRS) if p[0] == 'bulk'][:ORACLE_BULK]:
        sid, o, m, band = PAIRS[k]
        want = oracle.solve(o, m, want_table=True, diag_range=band, **OKW)
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
def test_the_knob_keeps_the_grouped_kernel_and_the_name(monkeypatch):
    _env(monkeypatch, True)
    name, res, txs, masks = _run()
    assert name == NAME, name
    _same_as_reference('edge-lane feeders', res, txs, masks)


@pytest.mark.gpu
def test_caller_owned_arena_whose_last_frame_ends_the_arena(monkeypatch):
    from biseqt_amd.batch import BatchAligner, DeviceArena
    _env(monkeypatch, False)
    reads = [np.asarray(s, np.uint8) for _, o, m, _ in PAIRS for s in (o, m)]
    lens = np.array([len(r) for r in reads], np.int64)
    offs = np.concatenate([[0], np.cumsum((lens + 3) // 4 * 4)[:-1]]).astype(np.int64)
    arena = np.full(int(offs[-1] + lens[-1]), 0xee, np.uint8)       # the last frame ends the arena; 0xee is no letter
    for r, o in zip(reads, offs):
        arena[o:o + len(r)] = r
    idx = np.arange(2 * len(PAIRS)).reshape(-1, 2)
    with DeviceArena(arena) as dev:                                  # (allocates arena.nbytes + 16)
        with BatchAligner.from_arena(arena, offs, lens, idx, diag_ranges=[band for _, _, _, band in PAIRS], device_arena=dev,
                                     check_band=False, **SC) as b:
            name, res, txs, masks = _collect(b)
    assert name == NAME, name
    _same_as_reference('caller-owned arena', res, txs, masks)

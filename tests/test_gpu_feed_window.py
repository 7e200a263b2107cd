"""The edge-lane feeders of the packed kernels on the GPU (pw_wave.h, WaveFill16::feed_issue: two dwords per sequence and
block, loaded a block ahead where the letter window lies inside the sequence's frame).

The shapes of tests/test_emu_feed_window.py -- feeds at every residue mod 4, sequences of 1 .. 17 letters, 400 x 24 and
24 x 400, 400 x 390 at band radius 20 and 200 -- in ONE batch beside 64 pairs of 400 x 390, on config 2's kernel (scores times
4) and on the same kernel with the scores as given.  Records, transcripts and every pair's whole tie-mask plane must equal
the 32-bit kernels' (PW_FLAG_NO_PACKED16; bits 0-2: the packed kernels store no M bit, go <= 0), and a sample the
oracle's.  One more run reads the same letters from a caller-owned arena (PW_FLAG_SHARED_ARENA) laid out as tight as the
API allows -- frames on 4-byte boundaries, the first at offset 0, the last ending exactly at arena_bytes, the allocation
exactly arena_bytes + 16 -- and must compute the same.
"""
import numpy as np
import pytest

from tests import ramp_free_cases as RC
from tests.test_emu_feed_window import SCORES, SHAPES

FIELDS = ('score', 'opt_i', 'opt_j', 'origin_idx', 'mutant_idx', 'tx_len', 'status')
# the first pair's origin (400 letters, offset 0 of the tight arena) loads ahead; the last pair's mutant (17 letters) ends it
PAIRS = [s for s in SHAPES['config2'][:2]] + [s[:4] for g in ('residues', 'short-origin', 'lopsided') for s in SHAPES[g]] + \
    RC.bulk() + [s for s in SHAPES['short-mutant']]
KERNELS = {True: 'k_fill16<8, false> x4 matrix', False: 'k_fill16<8, false> matrix'}
SC = dict(alnmode=1, alntype=RC.B_LOCAL, alphabet_len=4, match_score=SCORES[1], mismatch_score=SCORES[2], go_score=SCORES[3],
          ge_score=SCORES[4])
ORACLE_BULK = 2           # of the 64 pairs; every named shape is held to the oracle


def _env(monkeypatch, x4):
    for k in ('PWLIB_PACKED_BK', 'PWLIB_SIMPLE_AS_MATRIX', 'PWLIB_LATENCY_MODE', 'PWLIB_NO_SCALED16', 'PWLIB_RAMP_BLOCKS'):
        monkeypatch.delenv(k, raising=False)
    if not x4:
        monkeypatch.setenv('PWLIB_NO_SCALED16', '1')


@pytest.mark.parametrize('x4', [True, False], ids=['x4', 'x1'])
def test_the_planner_reaches_the_kernel(x4, monkeypatch):
    """(No GPU.)  The batch is planned onto the kernel the GPU tests name."""
    from biseqt_amd.batch import plan_only
    _env(monkeypatch, x4)
    shapes = [(len(o), len(m)) + tuple(band) for _, o, m, band in PAIRS]
    assert plan_only(shapes, **SC)['kernel'] == KERNELS[x4]
    assert PAIRS[0][0] == 'r20' and len(PAIRS[-1][2]) == 17


def _collect(b):
    res = b.run()
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
        assert np.array_equal(res[f], ref['res'][f]), (label, f, np.nonzero(res[f] != ref['res'][f])[0][:8])
    assert txs == ref['txs'], label
    for k in range(len(PAIRS)):
        assert np.array_equal(masks[k] & 7, ref['masks'][k] & 7), (label, k, PAIRS[k][0])


@pytest.mark.gpu
@pytest.mark.parametrize('x4', [True, False], ids=['x4', 'x1'])
def test_packed_equals_the_32_bit_kernels_and_the_oracle(x4, oracle, monkeypatch):
    _env(monkeypatch, x4)
    name, res, txs, masks = _run()
    assert name == KERNELS[x4], name
    _same_as_reference(name, res, txs, masks)
    okw = dict(mode=1, alntype=RC.B_LOCAL, L=4, match=float(SCORES[1]), mismatch=float(SCORES[2]), go=float(SCORES[3]),
               ge=float(SCORES[4]))
    named = [k for k, p in enumerate(PAIRS) if p[0] != 'bulk']
    for k in named + [k for k, p in enumerate(PAIRS) if p[0] == 'bulk'][:ORACLE_BULK]:
        sid, o, m, band = PAIRS[k]
        want = oracle.solve(o, m, want_table=True, diag_range=band, **okw)
        assert want['init_rc'] == 0 and masks[k].shape == want['mask'].shape, (name, sid)
        bad = np.nonzero((masks[k] & 7) != (want['mask'] & 7))[0]
        assert bad.size == 0, (name, sid, '%d of %d cells differ' % (bad.size, masks[k].size), bad[:8].tolist())
        assert (int(res['opt_i'][k]), int(res['opt_j'][k])) == tuple(want['opt']), (name, sid)
        if want['opt'][0] >= 0:
            assert float(res['score'][k]) == want['score'], (name, sid)
            assert (txs[k] or None) == (want['transcript'] or None), (name, sid)


@pytest.mark.gpu
def test_caller_owned_arena_with_nothing_behind_it_but_the_slack(monkeypatch):
    from biseqt_amd.batch import BatchAligner, DeviceArena
    _env(monkeypatch, True)
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
    assert name == KERNELS[True], name
    _same_as_reference('caller-owned arena', res, txs, masks)

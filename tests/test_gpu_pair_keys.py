"""One running-best key per two cells on the GPU (pw_wave.h, WaveFill16, PAIRK; pw_plan.h, pair_keys): the kernel
`k_fill16p<8, false, 3, true>` against the kernel it stands beside and the 32-bit kernels.

The cases of tests/pair_keys_cases.py, one batch per scoring: config 2's scores beside 64 pairs of 400 x 390, the scores under
which the cell behind the best keeps both gaps, the matrix whose best is 2047, the matrix with positive entries off its
diagonal.  Every batch runs as planned (one key per two cells), with PWLIB_PAIR_KEYS=0 (`k_fill16l`, one key per cell) and on
the 32-bit kernels (PW_FLAG_NO_PACKED16): records, transcripts and every pair's whole tie-mask plane must be equal among the
three (bits 0-2: the packed kernels store no M bit, go <= 0); every named shape and a sample of the 64 are held to the oracle --
record, transcript, whole plane; the kernel name is the same with the knob on and off.  One more run of the first batch reads
the same letters from a caller-owned arena (PW_FLAG_SHARED_ARENA) laid out as tight as the API allows -- frames on 4-byte
boundaries, the first at offset 0, the last ending exactly at arena_bytes, the allocation exactly arena_bytes + 16 -- and must
compute the same: the end-cell search reads two letters per diagonal, and never one outside a frame.
"""
import numpy as np
import pytest

from tests import pair_keys_cases as PC
from tests import ramp_free_cases as RC

FIELDS = ('score', 'opt_i', 'opt_j', 'origin_idx', 'mutant_idx', 'tx_len', 'status')
NAME = 'k_fill16<8, false> x4 matrix'
B_LOCAL = 1
KNOBS = ('PWLIB_PAIR_KEYS', 'PWLIB_LDS_FEED', 'PWLIB_STAMP_GROUP', 'PWLIB_RAMP_BLOCKS', 'PWLIB_PACKED_BK', 'PWLIB_SIMPLE_AS_MATRIX',
         'PWLIB_NO_SCALED16')
ORACLE_BULK = 2           # of the 64 pairs; every named shape is held to the oracle


def _wide_pair():
    """301 diagonals: the batch takes 8 diagonals per lane, one pair per wavefront."""
    rng = np.random.default_rng(78)
    o = rng.integers(0, 4, 300).astype(np.uint8)
    m = o.copy()
    m[::7] = (m[::7] + 1) % 4
    return ('band301', o, m, (-150, 150))


def _batches():
    """[(id, pairs, scoring of the batch, the oracle's scoring)]: the cases grouped by their scores, in the order they come."""
    groups = []
    for shape, S, go, ge in PC.cases():
        key = (repr(S), go, ge)
        for g in groups:
            if g[0] == key:
                g[1].append(shape)
                break
        else:
            groups.append((key, [shape], S, go, ge))
    names = {repr(PC.cfg2_matrix()): 'cfg2', repr(PC.gaps_matrix()): 'gaps', repr(PC.mixed_matrix()): 'mixed'}
    out = []
    for key, shapes, S, go, ge in groups:
        bid = names.get(key[0], 'best2047')
        # (the pair of 301 diagonals would score past 2047 under the matrix whose match is 23: that batch is its own pair, 401
        #  diagonals wide, three times)
        pairs = shapes * 3 if bid == 'best2047' else [_wide_pair()] + (RC.bulk() if bid == 'cfg2' else []) + shapes
        out.append((bid, pairs, dict(alnmode=1, alntype=B_LOCAL, alphabet_len=4, subst_scores=S, go_score=go, ge_score=ge),
                    dict(mode=1, alntype=B_LOCAL, L=4, subst=S, go=go, ge=ge)))
    return out


BATCHES = _batches()
IDS = [b[0] for b in BATCHES]


def _env(monkeypatch, knob):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv('PWLIB_LATENCY_MODE', '0')
    if knob:
        monkeypatch.setenv('PWLIB_PAIR_KEYS', '0')


def test_the_batches_are_what_they_say():
    assert IDS == ['cfg2', 'gaps', 'best2047', 'mixed']
    assert sum(len(b[1]) for b in BATCHES) == len(PC.cases()) + 3 + 2 + 64


@pytest.mark.parametrize('batch', BATCHES, ids=IDS)
def test_the_planner_reaches_the_form(batch, monkeypatch):
    """(No GPU.)  Every batch of the GPU tests is planned onto the kernel with one key per two cells, and onto the one beside it
    under the knob."""
    from biseqt_amd.batch import plan_only
    bid, pairs, sc, _ = batch
    shapes = [(len(o), len(m)) + tuple(band) for _, o, m, band in pairs]
    for knob in (False, True):
        _env(monkeypatch, knob)
        p = plan_only(shapes, ramp_free=True, stamp_group=True, lds_feed=True, pair_keys=True, **sc)
        assert p['kernel'] == NAME and p['ramp_free'] is True and p['stamp_group'] == 4 and p['lds_feed'] is True, (bid, knob, p)
        assert p['pair_keys'] is (not knob), (bid, knob, p)


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
def test_pair_keys_equal_the_32_bit_kernels_and_the_oracle(batch, oracle, monkeypatch):
    bid, pairs, sc, okw = batch
    _env(monkeypatch, False)
    name, res, txs, masks = _run(batch)
    assert name == NAME, name
    _same_as_reference(bid + ': one key per two cells', batch, res, txs, masks)
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
def test_the_knob_keeps_one_key_per_cell_and_the_name(batch, monkeypatch):
    _env(monkeypatch, True)
    name, res, txs, masks = _run(batch)
    assert name == NAME, name
    _same_as_reference(batch[0] + ': one key per cell', batch, res, txs, masks)


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

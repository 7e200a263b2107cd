"""The matrix form's 32-bit diagonal add (pw_wave.h, WaveFill16::cellpair, pk::add32) on the GPU, at the largest magnitudes
the planner admits -- the score sets of tests/test_emu_carry_free_add.py on 64 pairs of 400 x 390, band radius 200.

With 390 letters in the shorter sequence min(X, Y) * max(subst) <= 8000 leaves a best substitution of 20, and every score
stays within +-100, so a matrix range of 127 is not admitted at this shape (27 * 390 > 8000): the range-127 set runs on
400 x 80 (100 * 80 = 8000), and the scores-times-4 set whose best score is exactly 2047 on 400 x 89 (23 * 89).  Some pairs
are exact copies, so the bound on the best score is reached.

Every record, every transcript and every in-table cell's mask (bits 0-2: the packed kernels store no M bit, go <= 0) must
equal the forced 32-bit kernel's (PW_FLAG_NO_PACKED16) for all 64 pairs, and the oracle's on a sample."""
import numpy as np
import pytest

from tests.plane_checks import bkw_of, okw_of

pytestmark = pytest.mark.gpu

B_GLOBAL, B_LOCAL, B_OVERLAP = 0, 1, 2
NPAIRS = 64


def _matrix(hi, lo, pm):
    S = [[float(lo)] * 4 for _ in range(4)]
    for i in range(4):
        S[i][i] = float(hi)
    S[0][2] = S[2][0] = float(pm)          # a mismatch that scores
    return S


# (id, kernel name, matrix, Y, go, ge, alignment type, the best score an exact copy reaches)
SETS = [('r0-range120-ge100', 'k_fill16<8, false> matrix', _matrix(20, -100, 5), 390, 0., -100., B_LOCAL, 7800.),
        ('r0-range120-go50-ge50', 'k_fill16<8, false> matrix', _matrix(20, -100, 5), 390, -50., -50., B_LOCAL, 7800.),
        ('r0-range127-best8000', 'k_fill16<8, false> matrix', _matrix(100, -27, 5), 80, 0., -100., B_LOCAL, 8000.),
        ('r3-range31-ge100', 'k_fill16<8, false> x4 matrix', _matrix(5, -26, 3), 390, 0., -100., B_LOCAL, 1950.),
        ('r3-range31-best2047', 'k_fill16<8, false> x4 matrix', _matrix(23, -8, 3), 89, -5., -2., B_LOCAL, 2047.),
        ('r1-ge30', 'k_fill16<8, false, 1> matrix', _matrix(76, -27, 5), 390, 0., -30., B_OVERLAP, None),
        ('r2-ge30', 'k_fill16<8, false, 2> matrix', _matrix(76, -27, 5), 390, 0., -30., B_GLOBAL, None)]


def _pairs(Y, seed):
    from biseqt_amd import synth
    rng = synth.rng_for(seed)
    pairs = []
    for k in range(NPAIRS):
        o = rng.integers(0, 4, 400).astype(np.uint8)
        if k % 8 == 0:
            m = o[k % 5:k % 5 + Y].copy()                          # an exact copy: the best score at its bound
        elif k % 8 == 1:
            m = rng.integers(0, 4, Y).astype(np.uint8)             # unrelated
        else:
            m = synth.mutate(rng, o, 0.05, 0.03, 0.4)
            m = np.concatenate([m, rng.integers(0, 4, Y).astype(np.uint8)])[:Y]
        pairs.append((o, m))
    return pairs


def _run(pairs, kw, flags):
    from biseqt_amd.batch import BatchAligner
    # (check_band=False: the short mutants' band is clamped to the table by the library, as dptable_init clamps it)
    with BatchAligner(pairs, flags=flags, check_band=False, **bkw_of(kw)) as b:
        name = b.kernel_name
        res = b.run().copy()
        txs = b.transcripts(res)
        masks = [b.masks(k) for k in range(len(pairs))]
    return name, res, txs, masks


@pytest.mark.parametrize('sset', SETS, ids=[s[0] for s in SETS])
def test_extreme_scores_equal_the_32_bit_kernel_and_the_oracle(sset, oracle, monkeypatch):
    from biseqt_amd import _pwlib as W
    monkeypatch.setenv('PWLIB_LATENCY_MODE', '0')
    sid, kernel, S, Y, go, ge, alntype, best = sset
    pairs = _pairs(Y, 7100 + Y)
    kw = dict(mode=1, alntype=alntype, diag_range=(-200, 200), subst=S, go=go, ge=ge)
    name, res, txs, masks = _run(pairs, kw, 0)
    assert kernel in name, name
    name32, res32, txs32, masks32 = _run(pairs, kw, W.PW_FLAG_NO_PACKED16)
    assert 'k_fill16' not in name32, name32
    assert (res == res32).all(), (sid, np.nonzero(res != res32)[0][:8])
    assert txs == txs32, sid
    for k in range(NPAIRS):
        assert masks[k].shape == masks32[k].shape
        bad = np.nonzero((masks[k] & 7) != (masks32[k] & 7))[0]
        assert bad.size == 0, (sid, k, '%d of %d cells differ' % (bad.size, masks[k].size), bad[:8].tolist())
    if best is not None:
        assert float(res['score'].max()) == best, (sid, float(res['score'].max()))
    okw = okw_of(kw)
    for k in (0, 1, 2, 8, 27, 63):
        o, m = pairs[k]
        want = oracle.solve(o, m, want_table=True, **okw)
        assert want['init_rc'] == 0
        assert (int(res['opt_i'][k]), int(res['opt_j'][k])) == tuple(want['opt']), (sid, k)
        assert np.array_equal(masks[k] & 7, want['mask'] & 7), (sid, k)
        if want['opt'][0] < 0:
            continue
        assert float(res['score'][k]) == want['score'], (sid, k)
        st = int(res['status'][k])
        assert bool(st & W.PW_ST_PANICK) == bool(want['would_panick']), (sid, k)
        if not st & (W.PW_ST_PANICK | W.PW_ST_EMPTY):
            assert txs[k] == want['transcript'], (sid, k)
            assert (int(res['origin_idx'][k]), int(res['mutant_idx'][k])) == (want['origin_idx'], want['mutant_idx']), (sid, k)

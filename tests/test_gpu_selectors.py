"""Fixed mutant selector codes and kept-bit tie nibbles of `k_fill16<8, false> x4 matrix` on the GPU (pw_wave.h, WaveFill16:
FIXSEL, KEPT): the shapes of tests/test_emu_selectors.py in one batch on the kernel bench.py times.

64 pairs of 400 x 390 at radius 200, the 96 x 90 pairs whose bands start at -203 .. -200 (clamped to the table) and at
-47 .. -40 (the first fed mutant letter at every residue mod 4), a pair shorter than one block and pairs whose mutant ends in
the middle of a block.  Every result record and transcript must equal what the 32-bit kernels give for the same batch
(PW_FLAG_NO_PACKED16), and every cell's tie mask the oracle's (bits 0-2: the packed kernels store no M bit).
"""
import numpy as np
import pytest

from tests.test_emu_selectors import ASYM, SHAPES, first_fed
from tests.test_gpu_whole_plane import bkw_of, check_masks, okw_of, related

pytestmark = pytest.mark.gpu

KERNEL = 'k_fill16<8, false> x4 matrix'
FIELDS = ('score', 'opt_i', 'opt_j', 'origin_idx', 'mutant_idx', 'tx_len', 'status')


def batch():
    pairs, bands = [], []
    for k in range(64):
        pairs.append(related(400, 600 + k, 390))
        bands.append((-200, 200))
    for k, (_, X, Y, dr) in enumerate(SHAPES):
        o, m = related(max(X, Y) + 8, 700 + k)
        assert len(m) >= Y
        pairs.append((o[:X], m[:Y]))
        bands.append(dr)
    pairs.append(related(400, 800, 387))             # Y = 3 (mod 8) at the bench's band
    bands.append((-200, 200))
    return pairs, bands


@pytest.mark.parametrize('scores', ['match-mismatch', 'asymmetric'])
def test_x4_matrix_kernel_equals_32bit_kernels_and_oracle(scores, oracle, monkeypatch):
    from biseqt_amd import _pwlib as W
    from biseqt_amd.batch import BatchAligner
    monkeypatch.setenv('PWLIB_LATENCY_MODE', '0')
    pairs, bands = batch()
    assert {first_fed(len(o), len(m), dr) % 4 for (o, m), dr in zip(pairs, bands) if len(o) == 96} == {0, 1, 2, 3}
    kw = dict(mode=1, alntype=1, go=-5, ge=-2)
    kw.update(dict(subst=ASYM) if scores == 'asymmetric' else dict(match=1, mismatch=-3))
    bkw = dict(bkw_of(kw), diag_range=bands, check_band=False)
    with BatchAligner(pairs, flags=W.PW_FLAG_NO_PACKED16, **bkw) as b:
        assert 'k_fill16' not in b.kernel_name, b.kernel_name
        want = b.run()
        want_tx = b.transcripts(want)
    with BatchAligner(pairs, **bkw) as b:
        assert KERNEL in b.kernel_name, b.kernel_name
        got = b.run()
        got_tx = b.transcripts(got)
        for f in FIELDS:
            assert np.array_equal(got[f], want[f]), (f, np.nonzero(got[f] != want[f])[0][:8])
        assert got_tx == want_tx, [k for k in range(len(pairs)) if got_tx[k] != want_tx[k]][:8]
        assert sum(1 for t in got_tx if t) >= 64
        for k, ((o, m), dr) in enumerate(zip(pairs, bands)):
            check_masks(oracle, b, k, o, m, dict(okw_of(kw), diag_range=dr), True, '%s pair %d' % (scores, k))

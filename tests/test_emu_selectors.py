"""Fixed mutant selector codes and kept-bit tie nibbles of the packed x4 matrix fill (pw_wave.h, WaveFill16: FIXSEL, KEPT)
on the CPU lane emulator, against the oracle.

In the matrix form with 8 diagonals per lane a mutant letter gets its `v_perm_b32` selector code once -- from the iteration
on which it is fed, or would have been fed for the letters the window holds at the start -- and the cell pairs pass the
two matrix rows in the order the iteration number dictates.  What can go wrong is the phase: which letters carry the + 4
at the start of a pair, at the feed, and outside the sequence.  So the shapes here move the first fed mutant letter
(``f = (s0 - dmin) >> 1`` of pw_plan.h) through every residue mod 4, run out of mutant letters in the middle of a block,
and stay below one block altogether; each on one pair per wavefront and on the 2-wavefront form, with a 4-letter
asymmetric matrix and with match / mismatch scores written as a matrix.  Compared with the oracle: the result record, the
transcript, every cell's tie mask (bits 0-2: the packed kernels store no M bit, tests/test_emu_whole_plane.py) and walks
from every cell (a sample on the larger tables).
"""
import numpy as np
import pytest

from tests.emu import emu
from tests.test_emu_whole_plane import run_form, seqs

ASYM = [[3., -2., -1., -4.], [-1., 2., -3., 0.], [-2., -1., 4., -2.], [0., -3., -1., 1.]]
PLAIN = [[1. if i == j else -3. for j in range(4)] for i in range(4)]
GAPS = dict(go=-5., ge=-2.)


def first_fed(X, Y, dr):
    """Index of the first mutant letter lane 0 is fed (pw_plan.h: the band after the clamp, s0 == dmin mod 2)."""
    dmin, dmax = max(dr[0], -Y), min(dr[1], X)
    amin = dmin if dmin > 0 else (-dmax if dmax < 0 else 0)
    s0 = amin - (amin - dmin) % 2
    return (s0 - dmin) >> 1


# (id, X, Y, band)
SHAPES = [('96x90 dmin %d' % d, 96, 90, (d, d + 400)) for d in range(-203, -199)]       # radius 200: the clamp makes them one band
SHAPES += [('96x90 dmin %d' % d, 96, 90, (d, d + 70)) for d in range(-47, -39)]         # below the clamp: f = 20 .. 23
SHAPES += [('5x5', 5, 5, (-5, 5)), ('5x5 narrow', 5, 5, (-2, 1)),                       # shorter than one block
           ('70x67', 70, 67, (-30, 25)), ('41x35', 41, 35, (-35, 41)),                  # Y = 3 (mod 8): the mutant ends mid-block
           ('60x11', 60, 11, (-11, 40))]


def test_shapes_cover_every_phase_of_the_first_fed_letter():
    assert {first_fed(X, Y, dr) % 4 for _, X, Y, dr in SHAPES if X == 96} == {0, 1, 2, 3}
    assert sum(1 for _, _, Y, _ in SHAPES if Y % 8 == 3) >= 3


@pytest.mark.parametrize('waves', [1, 2], ids=['wave', 'mw2'])
@pytest.mark.parametrize('scores', ['asymmetric', 'match-mismatch'])
def test_x4_matrix_form_records_transcripts_and_planes(waves, scores, oracle):
    subst = ASYM if scores == 'asymmetric' else PLAIN
    ekw = dict(bk=8, packed16=3, waves=waves, matrix=True)
    for k, (sid, X, Y, dr) in enumerate(SHAPES):
        for related in ((True, False) if k % 3 == 0 else (True,)):      # (unrelated letters: every third shape)
            o, m = seqs(X, Y, 300 + k, related=related)
            kw = dict(mode=1, alntype=1, L=4, subst=subst, diag_range=dr, **GAPS)
            label = 'x4 matrix %s %s %s' % (scores, sid, 'related' if related else 'unrelated')
            run_form(oracle, o, m, kw, ekw, True, label, seed=k)
            want = oracle.solve(o, m, **kw)
            got = emu.solve(o, m, **dict(kw, **ekw))
            for key in ('init_rc', 'opt', 'score', 'transcript', 'origin_idx', 'mutant_idx', 'tb_null', 'would_panick'):
                assert want.get(key) == got.get(key), (label, key, want.get(key), got.get(key))


def test_wider_lanes_keep_the_half_bound_codes(oracle):
    """16 diagonals per lane (four packed registers per parity) is outside FIXSEL and still repairs the spliced register:
    the same shapes, so that the two code paths are seen side by side."""
    ekw = dict(bk=16, packed16=3, waves=1, matrix=True)
    for k, (sid, X, Y, dr) in enumerate(SHAPES[::3]):
        o, m = seqs(X, Y, 400 + k)
        kw = dict(mode=1, alntype=1, L=4, subst=ASYM, diag_range=dr, **GAPS)
        run_form(oracle, o, m, kw, ekw, True, 'x4 matrix bk16 %s' % sid, seed=k)

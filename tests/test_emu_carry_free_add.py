"""The matrix form's diagonal add as a plain 32-bit add (pw_wave.h, WaveFill16::cellpair, pk::add32), on the CPU lane
emulator at the largest magnitudes the planner admits.

Under the begin-anywhere rules (0, and 3 = rule 0 with scores times 4) `H + row byte` is one 32-bit add of two packed halves.
That is the packed add's result only while no half of H lies in [0xff80, 0xffff].  The emulator's pk::add32 counts every
breach of that (exported by the emulator's library as pw_pk_add32_breaches); the rules that begin on the table edge (1, 2)
hold negative scores and keep the packed add -- they run here too, on the same shapes.

Score sets, each AT a bound of admit_packed / packed_matrix_bytes_ok (pw_plan.h):
  * unscaled: matrix max - min = 127 (100 .. -27), min(X, Y) * max = 80 * 100 = 8000, a positive mismatch (+5), |ge| = 100
    (and go + ge = -100) under the local rule; under the overlap / global rules ge = -12, the lowest for which
    min(X, Y) * -min + |go| + |ge| * (diagonals + 2) stays within 23000;
  * times 4: max - min = 31 (23 .. -8), min(X, Y) * max = 89 * 23 = 2047, a positive mismatch (+3), ge = -100.
Shapes: X << Y and X >> Y with a 1665-diagonal band from the main diagonal outwards, so the outermost diagonals wait 1644
steps at the sentinel before their first cell (the shape of tests/golden/regress/mw_mismatch_9551.npz); the shorter sequence
sits in the longer one as a whole, so the best score IS the bound.  1665 = 1 (mod 32, 8 and 4): the first diagonal above the
band is the LOW half of its register, the one that can carry into a neighbour.
Every record, the transcript and every in-table cell's mask (bits 0-2: the packed kernels store no M bit, go <= 0) must be
the oracle's.  The cases just outside each bound must be refused by the planner -- they are not run.
"""
import ctypes

import numpy as np
import pytest

from biseqt_amd.batch import plan_only
from tests.emu import emu

KEYS = ('init_rc', 'opt', 'score', 'transcript', 'origin_idx', 'mutant_idx', 'tb_null', 'would_panick')
LONG, WAIT = 1700, 1644
B_GLOBAL, B_LOCAL, B_OVERLAP = 0, 1, 2


def _matrix(hi, lo, pm):
    S = [[float(lo)] * 4 for _ in range(4)]
    for i in range(4):
        S[i][i] = float(hi)
    S[0][2] = S[2][0] = float(pm)          # a mismatch that scores
    return S


UNSCALED, TIMES4 = _matrix(100, -27, 5), _matrix(23, -8, 3)
# (id, matrix, the shorter length, go, ge, alignment type, the packed body's rule)
SETS = [('r0-ge100', UNSCALED, 80, 0., -100., B_LOCAL, 0), ('r0-go50-ge50', UNSCALED, 80, -50., -50., B_LOCAL, 0),
        ('r3-ge100', TIMES4, 89, 0., -100., B_LOCAL, 3), ('r3-go5-ge2', TIMES4, 89, -5., -2., B_LOCAL, 3),
        ('r1-ge12', UNSCALED, 80, 0., -12., B_OVERLAP, 1), ('r2-ge12', UNSCALED, 80, 0., -12., B_GLOBAL, 2)]
# (id, packed16 mode of emu.solve for rule != 3 / rule 3, diagonals per lane, wavefronts)
FORMS = [('wave-bk32', 2, 3, 32, 1), ('lanes-bk32', 1, 4, 32, 1), ('mw4-bk8', 2, 3, 8, 4), ('mw7-bk4', 2, 3, 4, 7)]


def _breaches():
    fn = emu.lib().pw_pk_add32_breaches
    fn.restype = ctypes.c_uint
    return int(fn(1))                      # (read and reset)


def _pair(short, tall, seed):
    """The short sequence planted whole in the long one, 1580 letters in; `tall`: X << Y, else X >> Y."""
    rng = np.random.default_rng(seed)
    s = rng.integers(0, 4, short).astype(np.uint8)
    l = rng.integers(0, 4, LONG).astype(np.uint8)
    l[1580:1580 + short] = s
    return (s, l, (-WAIT, 20)) if tall else (l, s, (-20, WAIT))


_ORACLE = {}


def _want(oracle, sid, tall, o, m, kw):
    if (sid, tall) not in _ORACLE:
        _ORACLE[(sid, tall)] = oracle.solve(o, m, want_table=True, **kw)
    return _ORACLE[(sid, tall)]


@pytest.mark.parametrize('tall', [True, False], ids=['X<<Y', 'X>>Y'])
@pytest.mark.parametrize('form', FORMS, ids=[f[0] for f in FORMS])
@pytest.mark.parametrize('sset', SETS, ids=[s[0] for s in SETS])
def test_extreme_admitted_scores_equal_the_oracle_and_never_breach(sset, form, tall, oracle):
    sid, S, short, go, ge, alntype, rule = sset
    _, mode, mode_x4, bk, waves = form
    o, m, band = _pair(short, tall, 7 + short)
    kw = dict(L=4, mode=1, alntype=alntype, diag_range=band, subst=S, go=go, ge=ge)
    # the planner admits a batch of this shape to the packed matrix form, on this rule
    shape = (len(o), len(m)) + band
    for n in (1, 2048):
        p = plan_only([shape] * n, alnmode=1, alntype=alntype, alphabet_len=4, subst_scores=S, go_score=go, ge_score=ge)
        assert p['packed_rule'] == rule and p['matrix'], (n, p)
    want = _want(oracle, sid, tall, o, m, kw)
    assert want['init_rc'] == 0
    if rule in (0, 3):
        assert want['score'] == (8000. if rule == 0 else 2047.)        # the best score at the admission limit
    _breaches()
    got = emu.solve(o, m, bk=bk, packed16=mode_x4 if rule == 3 else mode, waves=waves, matrix=True, want_masks=True, **kw)
    n = _breaches()
    for key in KEYS:
        assert got.get(key) == want.get(key), (key, got.get(key), want.get(key))
    assert got['mask'].shape == want['mask'].shape
    bad = np.nonzero((got['mask'] & 7) != (want['mask'] & 7))[0]
    assert bad.size == 0, ('%d of %d cells differ' % (bad.size, want['mask'].size), bad[:8].tolist())
    assert n == 0, 'pk::add32 saw a half of H in [0xff80, 0xffff] %d times' % n


def test_ordinary_bands_never_breach(oracle):
    """Config 2's scores on bands of every residue modulo the lane width, one pair per wavefront and lane-packed, both
    scalings: the first diagonal above the band takes every place in its register."""
    rng = np.random.default_rng(41)
    o = rng.integers(0, 4, 150).astype(np.uint8)
    m = o.copy()
    flip = rng.random(150) < 0.15
    m[flip] = rng.integers(0, 4, int(flip.sum()))
    m = np.delete(m, [40, 41, 97])
    total = 0
    for r in range(3, 12):
        kw = dict(L=4, mode=1, alntype=B_LOCAL, diag_range=(-r, r + r % 2), match=1., mismatch=-3., go=-5., ge=-2.)
        want = oracle.solve(o, m, **kw)
        for mode in (1, 2, 3, 4):
            for bk in (4, 8):
                got = emu.solve(o, m, bk=bk, packed16=mode, matrix=True, **kw)
                for key in KEYS:
                    assert got.get(key) == want.get(key), (r, mode, bk, key)
                total += 1
    assert total == 72 and _breaches() == 0


OUTSIDE = [('best-8100', UNSCALED, 81, 0., -100., B_LOCAL, -1), ('range-128', _matrix(100, -28, 5), 80, 0., -100., B_LOCAL, -1),
           ('ge-101', UNSCALED, 80, 0., -101., B_LOCAL, -1), ('x4-best-2070', TIMES4, 90, 0., -100., B_LOCAL, 0),
           ('x4-range-32', _matrix(23, -9, 3), 89, 0., -100., B_LOCAL, 0), ('r2-ge13', UNSCALED, 80, 0., -13., B_GLOBAL, -1)]


@pytest.mark.parametrize('case', OUTSIDE, ids=[c[0] for c in OUTSIDE])
def test_just_outside_admission_the_planner_refuses(case):
    """One step past each bound the batch does not reach the body the bound protects: no packed kernel at all (-1), or
    -- past a bound of the scores-times-4 form only -- the unscaled rule 0.  Nothing is run: it is the planner that keeps
    the invariant, not the check."""
    _, S, short, go, ge, alntype, rule = case
    for tall in (True, False):
        shape = (short, LONG, -WAIT, 20) if tall else (LONG, short, -20, WAIT)
        for n in (1, 2048):
            p = plan_only([shape] * n, alnmode=1, alntype=alntype, alphabet_len=4, subst_scores=S, go_score=go, ge_score=ge)
            assert p['packed_rule'] == rule, (n, p)
            assert ('k_fill16' in p['kernel']) == (rule >= 0), p

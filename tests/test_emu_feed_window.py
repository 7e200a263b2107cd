"""The edge-lane feeders of the packed kernels, one pair per wavefront, on the CPU lane emulator (pw_wave.h,
WaveFill16::feed_issue / feed_commit): the two dwords a block's letter window gains are loaded a block ahead by ONE
two-dword load where the window lies inside the sequence's frame ("ahead"), and fetched by the block itself elsewhere
("late": the clamped loads of before, or no load where the window lies beyond an end altogether).

Every run checks
  * the record, the transcript and EVERY in-table cell's tie mask equal the oracle's, and walks from a sample of end cells;
  * the emulator's reader was never asked for a dword outside [0, last dword] of the frame it read (pw_feed_breaches);
  * the emulator's path counters (pw_feed_path_counts) equal the counts restated here from the definition: block b's window
    starts at word w = (first fed letter + 8 b) >> 2, is loaded ahead iff b >= 1, 0 <= w and w + 2 <= last word, and late
    otherwise (a pair's first block is loaded in front of the loops, so it counts as late only where its window is clamped).
Forms: rules 0 and 3 (scores times 4), matrix and match / mismatch form; the matrix form with ramp_free on and, through
PWLIB_RAMP_BLOCKS=1, off (the match / mismatch form knows no ramp_free).  The origin frame is always the first of the
emulator's arena.  The emulator's harness lays its arena out itself, padded, so a last frame that ends exactly at
arena_bytes cannot be built here: the reader's count of dwords outside the frame is what holds in any layout, and the
layout itself -- frames on 4-byte boundaries, the last ending the arena, an allocation of arena_bytes + 16 -- runs on the
GPU (tests/test_gpu_feed_window.py).

Which cases run both paths: all whose frame has 3 dwords or more AND whose window is inside it in some block after the
first.  A sequence of up to 8 letters (2 dwords) never loads ahead, by design, and the origin feed runs 64 lanes x 4 letters
ahead of the band, so an origin shorter than that is late in every block; the groups below say what they expect.
"""
import ctypes

import numpy as np
import pytest

from tests import ramp_free_cases as RC
from tests.emu import emu
from tests.test_emu_whole_plane import check_plane, pick_ends, table_cells

KEYS = ('init_rc', 'opt', 'score', 'transcript', 'origin_idx', 'mutant_idx', 'tb_null', 'would_panick')
SCORES = ('cfg2', 1, -3, -5, -2)
WALKS = 12
LENGTHS = (1, 3, 4, 7, 8, 9, 11, 12, 13, 16, 17)


def _pair(seed, X, Y):
    rng = np.random.default_rng(seed)
    long = rng.integers(0, 4, max(X, Y) + 8).astype(np.uint8)
    o = long[:X].copy()
    m = long[3:3 + Y].copy() if Y < X else long[:Y].copy()
    flip = rng.random(len(m)) < 0.12
    m[flip] = rng.integers(0, 4, int(flip.sum()))
    return o, m


def _shapes():
    """{group: [(id, origin, mutant, band)]}"""
    g = {}
    # the first fed origin letter sits at e - 1 (mod 4) and the first fed mutant letter at f (mod 4), e = (s0 + dmin) >> 1,
    # f = (s0 - dmin) >> 1: eight consecutive dmin walk both through every residue (test_what_the_shapes_cover)
    # (an origin of 300 letters: its feed starts at letter 250 or so, see 'short-origin' below)
    o, m = _pair(1, 300, 58)
    g['residues'] = [('dmin%d' % d, o, m, (d, d + 19)) for d in range(-10, -2)]
    g['short-origin'] = [('X%d' % n,) + _pair(100 + n, n, 40) + ((-12, 12),) for n in LENGTHS]
    g['short-mutant'] = [('Y%d' % n,) + _pair(200 + n, 40, n) + ((-1, 12),) for n in LENGTHS]
    g['lopsided'] = [('400x24',) + _pair(7, 400, 24) + ((-24, 400),), ('24x400',) + _pair(8, 24, 400) + ((-400, 24),)]
    o, m = _pair(9, 400, 390)
    g['config2'] = [('r20', o, m, (-20, 20)), ('r200', o, m, (-200, 200))]
    return g


SHAPES = _shapes()
FORMS = [(rule, mat) for rule in (0, 3) for mat in (True, False)]


def _u(name, *args):
    fn = getattr(emu.lib(), name)
    fn.restype = ctypes.c_uint
    return fn(*args)


def _path_counts():
    out = (ctypes.c_uint * 4)()
    emu.lib().pw_feed_path_counts(out, 1)
    return [int(v) for v in out]           # [origin ahead, origin late, mutant ahead, mutant late], read and reset


def _geometry(X, Y, band, bk):
    """(blocks, first fed origin letter, first fed mutant letter) of the pair on 64 lanes of bk diagonals."""
    nb = RC.plan_blocks(X, Y, *band)[0]
    dmin, dmax = max(band[0], -Y), min(band[1], X)
    amin = dmin if dmin > 0 else (-dmax if dmax < 0 else 0)
    s0 = amin - (amin - dmin) % 2
    return nb, ((s0 + dmin) >> 1) + 64 * (bk // 2) - 1, (s0 - dmin) >> 1


def _expected_paths(n, first, nb):
    wlast = (max(n, 1) - 1) >> 2
    inside = [0 <= (first + 8 * b) >> 2 and ((first + 8 * b) >> 2) + 2 <= wlast for b in range(nb)]
    return sum(inside[1:]), sum(not x for x in inside)


@pytest.fixture
def ramp(monkeypatch):
    monkeypatch.delenv('PWLIB_RAMP_BLOCKS', raising=False)
    emu.lib().pw_emu_ramp_free(1)
    yield monkeypatch
    emu.lib().pw_emu_ramp_free(-1)


_ORACLE = {}


def _run(oracle, monkeypatch, group, shape, rule, mat):
    sid, o, m, band = shape
    X, Y = len(o), len(m)
    kw = dict(L=4, mode=1, alntype=RC.B_LOCAL, diag_range=band, subst=RC.matrix(SCORES[1], SCORES[2]), go=float(SCORES[3]),
              ge=float(SCORES[4]))
    key = (group, sid)
    if key not in _ORACLE:
        want = oracle.solve(o, m, **kw)
        _ORACLE[key] = (want, pick_ends(table_cells(want, X, Y, 1), WALKS, 5))
    want, ends = _ORACLE[key]
    nd = min(band[1], X) - max(band[0], -Y) + 1
    bk = next(b for b in (8, 16, 32) if 64 * b >= nd)
    nb, fo, fm = _geometry(X, Y, band, bk)
    expect = list(_expected_paths(X, fo, nb) + _expected_paths(Y, fm, nb))
    ekw = dict(bk=bk, packed16=3 if rule == 3 else 2, waves=1, matrix=mat)
    seen = None
    for knob in ((False, True) if mat else (False,)):           # ramp_free on, then off through the planner's knob
        label = '%s %s rule %d %s bk%d%s' % (group, sid, rule, 'matrix' if mat else 'plain', bk, ' PWLIB_RAMP_BLOCKS=1' if knob else '')
        if knob:
            monkeypatch.setenv('PWLIB_RAMP_BLOCKS', '1')
        _u('pw_feed_breaches', 1), _path_counts()
        try:
            got = emu.solve(o, m, want_masks=True, ends=ends, **dict(kw, **ekw))
        finally:
            monkeypatch.delenv('PWLIB_RAMP_BLOCKS', raising=False)
        breaches, counts = _u('pw_feed_breaches', 1), _path_counts()
        print(label, 'paths [origin ahead, late, mutant ahead, late]:', counts)
        assert breaches == 0, (label, 'the feeders asked for %d dwords outside their frames' % breaches)
        assert counts == expect, (label, counts, expect)
        check_plane(oracle, o, m, kw, got, ends, True, label)
        for k in KEYS:
            assert got.get(k) == want.get(k), (label, k, got.get(k), want.get(k))
        if seen is not None:
            assert np.array_equal(seen['mask'] & 7, got['mask'] & 7), label
        seen = got
    return expect


@pytest.mark.parametrize('form', FORMS, ids=['rule%d-%s' % (r, 'matrix' if t else 'plain') for r, t in FORMS])
@pytest.mark.parametrize('group', sorted(SHAPES))
def test_feed_window_equals_the_oracle(group, form, oracle, ramp):
    paths = [_run(oracle, ramp, group, shape, *form) for shape in SHAPES[group]]
    ids = [s[0] for s in SHAPES[group]]
    both_o = [i for i, p in zip(ids, paths) if p[0] and p[1]]
    both_m = [i for i, p in zip(ids, paths) if p[2] and p[3]]
    ahead_o = [i for i, p in zip(ids, paths) if p[0]]
    ahead_m = [i for i, p in zip(ids, paths) if p[2]]
    if group == 'short-origin':
        # the origin feed starts 64 lanes x 4 letters ahead of the band, far past the end of an origin this short: late in
        # every block (an origin of up to 8 letters has no third dword anyway); the tables are a block or three long, and
        # the mutant's window (40 letters) is inside its frame in all of them: ahead in every block but the first
        assert ahead_o == [] and ahead_m == ids[1:] and both_m == [], (ahead_o, ahead_m, both_m)
    elif group == 'short-mutant':
        # ... likewise the origin of 40 letters.  The mutant is fed from letter 0; block 1's window is words 2 .. 4, which
        # only the 17-letter mutant (5 dwords) holds: the one load ahead of the group, every other window is clamped
        assert ahead_o == [] and ahead_m == ['Y17'] and both_m == ['Y17'], (ahead_o, ahead_m, both_m)
    elif group == 'lopsided':
        assert both_o == ['400x24'] and both_m == ['24x400'], (both_o, both_m)     # the long sequence of each pair
    else:
        assert both_o == ids and both_m == ids, (group, both_o, both_m)


def test_what_the_shapes_cover():
    res = set()
    for _, o, m, band in SHAPES['residues']:
        _, fo, fm = _geometry(len(o), len(m), band, 8)
        res.add((fo & 3, fm & 3))
    assert {r[0] for r in res} == {0, 1, 2, 3} and {r[1] for r in res} == {0, 1, 2, 3}, res
    assert {len(s[1]) for s in SHAPES['short-origin']} == set(LENGTHS) == {len(s[2]) for s in SHAPES['short-mutant']}

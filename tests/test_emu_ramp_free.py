"""ramp_free on the CPU lane emulator: the packed matrix form of the local rules (0, and 3 = scores times 4) with its start
and end blocks on the steady body (pw_wave.h, WaveFill16::RAMPF; pw_plan.h, ramp_free), against the oracle.

Forms: rules 0 and 3, matrix form; one pair per wavefront, lane-packed, two wavefronts per pair.  Score sets and shapes:
tests/ramp_free_cases.py.  Every run checks
  * the record, the transcript and EVERY in-table cell's tie mask equal the oracle's (bits 0-2: the packed kernels store no
    M bit, go <= 0 -- tests/test_emu_whole_plane.py), and walks from a sample of end cells;
  * pk::add32 saw no half of H in [0xff80, 0xffff] (pw_pk_add32_breaches);
  * the emulator's block counters (pw_ramp_block_counts): every block ran on the steady body;
  * with PWLIB_RAMP_BLOCKS=1 the counters show the four loops' old split (restated in tests/ramp_free_cases.py from the
    planner's definition of a steady block) and the record and the plane are the same.
The score sets the predicate refuses run too, on the old split, and equal the oracle.
"""
import ctypes

import numpy as np
import pytest

from tests import ramp_free_cases as RC
from tests.emu import emu
from tests.test_emu_whole_plane import check_plane, pick_ends, table_cells

KEYS = ('init_rc', 'opt', 'score', 'transcript', 'origin_idx', 'mutant_idx', 'tb_null', 'would_panick')
SHAPES = RC.shapes()
# (id, packed16 mode of emu.solve for rule 0 / rule 3, wavefronts)
LAYOUTS = [('wave', 2, 3, 1), ('lanes', 1, 4, 1), ('mw2', 2, 3, 2)]
WALKS = 24


def _lane_width(layout, nd):
    if layout == 'lanes':
        return next(b for b in (4, 8, 12, 16, 20, 32) if 64 * b >= nd and (nd + b - 1) // b < 64)
    waves = 2 if layout == 'mw2' else 1
    return next(b for b in ((8, 16, 32) if layout == 'wave' else (4, 8, 16, 32)) if 64 * waves * b >= nd)


def _breaches():
    fn = emu.lib().pw_pk_add32_breaches
    fn.restype = ctypes.c_uint
    return int(fn(1))                      # (read and reset)


def _block_counts():
    out = (ctypes.c_uint * 4)()
    emu.lib().pw_ramp_block_counts(out, 1)
    return [int(v) for v in out]           # [steady, not started, ended, both], read and reset


@pytest.fixture
def ramp(monkeypatch):
    """Sets the planner's answer for the emulated launches that follow; back to "as FillParams says" afterwards."""
    monkeypatch.delenv('PWLIB_RAMP_BLOCKS', raising=False)
    yield lambda on: emu.lib().pw_emu_ramp_free(1 if on else 0)
    emu.lib().pw_emu_ramp_free(-1)


_ORACLE = {}


def _problem(oracle, sset, x4, shape):
    sid, o, m, band = shape
    match = RC.match_of(sset, x4, len(o), len(m))
    kw = dict(L=4, mode=1, alntype=RC.B_LOCAL, diag_range=band, subst=RC.matrix(match, sset[2]), go=float(sset[3]), ge=float(sset[4]))
    key = (sset[0], match, sid)
    if key not in _ORACLE:
        probe = oracle.solve(o, m, **kw)
        _ORACLE[key] = pick_ends(table_cells(probe, len(o), len(m), 1), WALKS, 5)
    return o, m, band, kw, _ORACLE[key]


def _run(oracle, ramp, monkeypatch, sset, rule, layout, shape, admitted):
    lid, mode, mode_x4, waves = layout
    o, m, band, kw, ends = _problem(oracle, sset, rule == 3, shape)
    X, Y = len(o), len(m)
    nd = min(band[1], X) - max(band[0], -Y) + 1
    ekw = dict(bk=_lane_width(lid, nd), packed16=mode_x4 if rule == 3 else mode, waves=waves, matrix=True)
    label = '%s rule %d %s %s bk%d' % (sset[0], rule, lid, shape[0], ekw['bk'])
    assert RC.ramp_free(sset[2], sset[3], sset[4]) == admitted, label
    old = RC.block_kinds(X, Y, *band)
    nb = sum(old)
    ramp(admitted)
    _breaches(), _block_counts()
    got = emu.solve(o, m, want_masks=True, ends=ends, **dict(kw, **ekw))
    breaches, counts = _breaches(), _block_counts()
    check_plane(oracle, o, m, kw, got, ends, True, label)
    want = oracle.solve(o, m, **kw)
    for key in KEYS:
        assert got.get(key) == want.get(key), (label, key, got.get(key), want.get(key))
    assert breaches == 0, (label, 'pk::add32 saw a half of H in [0xff80, 0xffff] %d times' % breaches)
    assert counts == ([nb, 0, 0, 0] if admitted else old), (label, counts, old)
    if not admitted:
        return
    # the knob: the old split, the same record and plane
    monkeypatch.setenv('PWLIB_RAMP_BLOCKS', '1')
    try:
        knob = emu.solve(o, m, want_masks=True, **dict(kw, **ekw))
    finally:
        monkeypatch.delenv('PWLIB_RAMP_BLOCKS')
    breaches, counts = _breaches(), _block_counts()
    assert counts == old and counts != [nb, 0, 0, 0], (label, counts, old)
    assert breaches == 0, label
    for key in KEYS:
        assert knob.get(key) == got.get(key), (label, key)
    assert np.array_equal(knob['mask'] & 7, got['mask'] & 7), label


@pytest.mark.parametrize('layout', LAYOUTS, ids=[f[0] for f in LAYOUTS])
@pytest.mark.parametrize('rule', [0, 3])
@pytest.mark.parametrize('sset', RC.SCORE_SETS, ids=[s[0] for s in RC.SCORE_SETS])
def test_ramp_blocks_on_the_steady_body_equal_the_oracle(sset, rule, layout, oracle, ramp, monkeypatch):
    for shape in SHAPES:
        _run(oracle, ramp, monkeypatch, sset, rule, layout, shape, True)


@pytest.mark.parametrize('layout', LAYOUTS, ids=[f[0] for f in LAYOUTS])
@pytest.mark.parametrize('rule', [0, 3])
@pytest.mark.parametrize('sset', RC.REFUSED_SETS, ids=[s[0] for s in RC.REFUSED_SETS])
def test_refused_score_sets_keep_the_old_split(sset, rule, layout, oracle, ramp, monkeypatch):
    for shape in SHAPES:
        _run(oracle, ramp, monkeypatch, sset, rule, layout, shape, False)


def test_what_the_shapes_cover():
    """The shapes are what the test says they are."""
    by = {s[0]: s for s in SHAPES}
    kinds = {sid: RC.block_kinds(len(o), len(m), *band) for sid, o, m, band in SHAPES}
    assert sum(kinds['short']) == 1                                       # shorter than one block
    _, o, m, band = by['wait1600']
    dmin, dmax = max(band[0], -len(m)), min(band[1], len(o))
    assert max(abs(dmin), abs(dmax)) - min(abs(d) for d in (dmin, dmax, 0) if dmin <= d <= dmax) > 1500
    _, o, m, band = by['band>table']
    assert band[0] < -len(m) and band[1] > len(o)
    _, o, m, band = by['mid-block']
    assert (len(o) + len(m) + 1) % 16 not in (0, 15)
    for sid, k in kinds.items():
        assert k[1] + k[2] + k[3] > 0, sid                                 # every shape has blocks the old split sends to an edge loop
    assert any(k[3] for k in kinds.values()) and any(k[1] and k[2] and k[0] for k in kinds.values())

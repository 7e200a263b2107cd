"""The stamp group of the running best on the CPU lane emulator (pw_wave.h, WaveFill16, GRP; the emulator takes the group at
run time: pw_emu_stamp_group), against the oracle.

Form: rule 3 (scores times 4), matrix form, one pair per wavefront, 8 diagonals per lane, ramp_free on.  Every shape of
tests/stamp_group_cases.py runs with the knob at 4 and at 1; each run checks
  * the record, the transcript and EVERY in-table cell's tie mask equal the oracle's (bits 0-2: the packed kernels store no
    M bit, go <= 0 -- tests/test_emu_whole_plane.py), and walks from a sample of end cells;
  * pk::add32 saw no half of H in [0xff80, 0xffff] (pw_pk_add32_breaches);
  * every block ran on the steady body (pw_ramp_block_counts).
"""
import ctypes

import pytest

from tests import stamp_group_cases as SC
from tests.emu import emu
from tests.test_emu_whole_plane import check_plane, pick_ends, table_cells

KEYS = ('init_rc', 'opt', 'score', 'transcript', 'origin_idx', 'mutant_idx', 'tb_null', 'would_panick')
WALKS = 12
B_LOCAL = 1
SHAPES = SC.shapes()
# (shape, matrix, go, ge)
CASES = [(s, SC.cfg2_matrix(), float(SC.CFG2[3]), float(SC.CFG2[4])) for s in SHAPES] + [(SC.top_shape(), SC.top_matrix(), -5., -2.)]


def _breaches():
    fn = emu.lib().pw_pk_add32_breaches
    fn.restype = ctypes.c_uint
    return int(fn(1))                      # (read and reset)


def _block_counts():
    out = (ctypes.c_uint * 4)()
    emu.lib().pw_ramp_block_counts(out, 1)
    return [int(v) for v in out]           # [steady, not started, ended, both], read and reset


def _group_stamps():
    fn = emu.lib().pw_group_stamps
    fn.restype = ctypes.c_uint
    return int(fn(1))                      # (read and reset)


@pytest.fixture
def group(monkeypatch):
    """Sets ramp_free on and the stamp group for the emulated launches that follow; both back to their defaults afterwards."""
    monkeypatch.delenv('PWLIB_RAMP_BLOCKS', raising=False)
    emu.lib().pw_emu_ramp_free(1)
    yield lambda g: emu.lib().pw_emu_stamp_group(int(g))
    emu.lib().pw_emu_stamp_group(-1)
    emu.lib().pw_emu_ramp_free(-1)


_ORACLE = {}


def _oracle(oracle, sid, o, m, kw):
    if sid not in _ORACLE:
        want = oracle.solve(o, m, **kw)
        _ORACLE[sid] = (want, pick_ends(table_cells(want, len(o), len(m), 1), WALKS, 5))
    return _ORACLE[sid]


@pytest.mark.parametrize('grp', [4, 1])
@pytest.mark.parametrize('case', CASES, ids=[c[0][0] for c in CASES])
def test_grouped_and_per_block_stamps_equal_the_oracle(case, grp, oracle, group):
    (sid, o, m, band), S, go, ge = case
    kw = dict(L=4, mode=1, alntype=B_LOCAL, diag_range=band, subst=S, go=go, ge=ge)
    want, ends = _oracle(oracle, sid, o, m, kw)
    label = '%s group %d' % (sid, grp)
    group(grp)
    _breaches(), _block_counts(), _group_stamps()
    got = emu.solve(o, m, want_masks=True, ends=ends, bk=8, packed16=3, waves=1, matrix=True, **kw)
    breaches, counts, stamps = _breaches(), _block_counts(), _group_stamps()
    # the form that ran: one stamp per four blocks and one for a last, shorter group -- none with the stamp per block
    assert stamps == ((SC.nblocks(case[0]) + 3) // 4 if grp == 4 else 0), (label, stamps)
    check_plane(oracle, o, m, kw, got, ends, True, label)
    for key in KEYS:
        assert got.get(key) == want.get(key), (label, key, got.get(key), want.get(key))
    assert breaches == 0, (label, 'pk::add32 saw a half of H in [0xff80, 0xffff] %d times' % breaches)
    assert counts == [SC.nblocks(case[0]), 0, 0, 0], (label, counts)



def test_what_the_shapes_cover(oracle):
    """The shapes are what the module says they are."""
    by = {s[0]: s for s in SHAPES}
    assert sorted(SC.nblocks(by['blocks%d' % n]) % 4 for n in (4, 5, 6, 7)) == [0, 1, 2, 3]
    assert [SC.nblocks(by['blocks%d' % n]) for n in (4, 5, 6, 7)] == [4, 5, 6, 7]
    assert SC.nblocks(by['short']) == 1 and len(by['short'][1]) + len(by['short'][2]) + 1 < 16
    cfg = dict(L=4, mode=1, alntype=B_LOCAL, subst=SC.cfg2_matrix(), go=float(SC.CFG2[3]), ge=float(SC.CFG2[4]))

    def best(sid):
        _, o, m, band = by[sid]
        r = oracle.solve(o, m, diag_range=band, **cfg)
        d = max(band[0], -len(m)) + r['opt'][0]              # banded table coordinates: (diagonal - dmin, index along it)
        return r['score'], d, r['opt'][1] + max(d, 0)         # score, diagonal, x of the end cell
    # the periodic pair: 12 at the end of the first run, although every later run reaches it again, in later blocks and groups
    assert best('periodic') == (12.0, 0, 12)
    # ... one more in the last run: the rise lies in the last group, which holds fewer than four blocks
    score, d, x = best('periodic-late-rise')
    nb = SC.nblocks(by['periodic-late-rise'])
    assert (score, d, x) == (13.0, 0, 21 * 18 + 13) and nb % 4 != 0 and (2 * x) // 64 == (nb - 1) // 4
    # first and last cell of a group: the main diagonal's cell x is iteration x, and a group holds 32 iterations
    assert best('cell0') == (10.0, 0, 64) and best('cell31') == (10.0, 0, 95)
    _, o, m, band = by['disjoint']
    r = oracle.solve(o, m, diag_range=band, **cfg)
    assert r['score'] in (None, 0.0), r
    _, o, m, band = SC.top_shape()
    r = oracle.solve(o, m, L=4, mode=1, alntype=B_LOCAL, diag_range=band, subst=SC.top_matrix(), go=-5., ge=-2.)
    assert r['score'] == 2047.0

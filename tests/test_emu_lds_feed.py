"""The letter rings on the CPU lane emulator (pw_wave.h, WaveFill16, LDSF; the emulator takes the switch at run time:
pw_emu_lds_feed), against the oracle.

Form: matrix form, one pair per wavefront, 8 diagonals per lane, ramp_free on; rule 3 (scores times 4) with the stamp group
at 4 -- the device kernel's form -- and rule 0 with the stamp per block.  Every shape of tests/lds_feed_cases.py runs with the
rings; each run checks
  * the record, the transcript and EVERY in-table cell's tie mask equal the oracle's (bits 0-2: the packed kernels store no
    M bit, go <= 0 -- tests/test_emu_whole_plane.py), and walks from a sample of end cells;
  * no byte was asked for outside a frame (pw_feed_breaches) and pk::add32 saw no half of H in [0xff80, 0xffff];
  * the rings ran: six chunks staged in front of the loop and one per eight blocks run in full (pw_ring_restages), and none
    with the switch off;
  * every block ran on the steady body (pw_ramp_block_counts).
"""
import ctypes

import pytest

from tests import lds_feed_cases as LC
from tests.emu import emu
from tests.test_emu_whole_plane import check_plane, pick_ends, table_cells

KEYS = ('init_rc', 'opt', 'score', 'transcript', 'origin_idx', 'mutant_idx', 'tb_null', 'would_panick')
WALKS = 12
B_LOCAL = 1
SHAPES = LC.shapes()
RULES = {3: dict(packed16=3, group=4), 0: dict(packed16=2, group=1)}


def _uint(name):
    fn = getattr(emu.lib(), name)
    fn.restype = ctypes.c_uint
    return int(fn(1))                      # (read and reset)


def _block_counts():
    out = (ctypes.c_uint * 4)()
    emu.lib().pw_ramp_block_counts(out, 1)
    return [int(v) for v in out]           # [steady, not started, ended, both], read and reset


@pytest.fixture
def rings(monkeypatch):
    """Sets ramp_free on, the stamp group and the letter rings for the emulated launches that follow; all back to their
    defaults afterwards."""
    monkeypatch.delenv('PWLIB_RAMP_BLOCKS', raising=False)
    emu.lib().pw_emu_ramp_free(1)

    def set_(group, on):
        emu.lib().pw_emu_stamp_group(int(group))
        emu.lib().pw_emu_lds_feed(int(on))
    yield set_
    emu.lib().pw_emu_lds_feed(-1)
    emu.lib().pw_emu_stamp_group(-1)
    emu.lib().pw_emu_ramp_free(-1)


_ORACLE = {}


def _oracle(oracle, shape):
    sid, o, m, band = shape
    kw = dict(L=4, mode=1, alntype=B_LOCAL, diag_range=band, subst=LC.cfg2_matrix(), go=float(LC.CFG2[3]), ge=float(LC.CFG2[4]))
    if sid not in _ORACLE:
        want = oracle.solve(o, m, **kw)
        _ORACLE[sid] = (want, pick_ends(table_cells(want, len(o), len(m), 1), WALKS, 5))
    return (kw,) + _ORACLE[sid]


def _run_and_check(oracle, rings, shape, rule, on=1):
    sid, o, m, band = shape
    kw, want, ends = _oracle(oracle, shape)
    label = '%s rule %d rings %d' % (sid, rule, on)
    rings(RULES[rule]['group'], on)
    for name in ('pw_pk_add32_breaches', 'pw_feed_breaches', 'pw_ring_restages'):
        _uint(name)
    _block_counts()
    got = emu.solve(o, m, want_masks=True, ends=ends, bk=8, packed16=RULES[rule]['packed16'], waves=1, matrix=True, **kw)
    add32, outside, staged, counts = _uint('pw_pk_add32_breaches'), _uint('pw_feed_breaches'), _uint('pw_ring_restages'), _block_counts()
    nb = LC.nblocks(shape)
    assert staged == ((6 + nb // 8) if on == 1 else 0), (label, staged, nb)
    check_plane(oracle, o, m, kw, got, ends, True, label)
    for key in KEYS:
        assert got.get(key) == want.get(key), (label, key, got.get(key), want.get(key))
    assert outside == 0, (label, '%d bytes or dwords asked for outside a frame' % outside)
    assert add32 == 0, (label, 'pk::add32 saw a half of H in [0xff80, 0xffff] %d times' % add32)
    assert counts == [nb, 0, 0, 0], (label, counts)


@pytest.mark.parametrize('rule', [3, 0])
@pytest.mark.parametrize('shape', SHAPES, ids=[s[0] for s in SHAPES])
def test_letters_from_the_rings_equal_the_oracle(shape, rule, oracle, rings):
    _run_and_check(oracle, rings, shape, rule)


@pytest.mark.parametrize('rule', [3, 0])
def test_rings_that_wrap_more_than_twice(rule, oracle, rings):
    shape = LC.long_shape()
    assert LC.nblocks(shape) * 8 > 2 * 512
    _run_and_check(oracle, rings, shape, rule)


@pytest.mark.parametrize('on', [0, -1])
def test_the_switch_off_keeps_the_feeders(on, oracle, rings):
    by = {s[0]: s for s in SHAPES}
    _run_and_check(oracle, rings, by['400x390-r20'], 3, on)


def test_what_the_shapes_cover():
    """The shapes are what the module says they are."""
    by = {s[0]: s for s in SHAPES}
    assert [len(by['len%d' % n][1]) for n in range(1, 18)] == list(range(1, 18))
    assert sorted(LC.nblocks(by['blocks%d' % n]) % 8 for n in range(8, 16)) == list(range(8))
    res = [LC.feed_residues(by['dmin%d' % d]) for d in range(-1, -9, -1)]
    assert {e for e, _ in res} == {0, 1, 2, 3} and {f for _, f in res} == {0, 1, 2, 3}
    assert (len(by['400x24'][1]), len(by['400x24'][2]), len(by['24x400'][1]), len(by['24x400'][2])) == (400, 24, 24, 400)
    _, o, m, band = by['mutant-ends-mid-chunk']
    assert len(m) % 64 not in (0, 63) and len(o) > len(m) + 128
    _, o, m, band = LC.long_shape()
    assert (len(o), len(m), band) == (1200, 1190, (-200, 200))

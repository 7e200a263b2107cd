"""One running-best key per two cells on the CPU lane emulator (pw_wave.h, WaveFill16, PAIRK; the emulator takes the switch at
run time: pw_emu_pair_keys), against the oracle.

Form: rule 3 (scores times 4), matrix form, one pair per wavefront, 8 diagonals per lane, ramp_free on, the stamp group at 4 and
the letters from the rings -- the device kernel's form.  Every case of tests/pair_keys_cases.py runs with the switch on and
off; each run checks
  * the record, the transcript and EVERY in-table cell's tie mask equal the oracle's (bits 0-2: the packed kernels store no
    M bit, go <= 0 -- tests/test_emu_whole_plane.py), and walks from a sample of end cells;
  * no byte was asked for outside a frame (pw_feed_breaches) and pk::add32 saw no half of H in [0xff80, 0xffff];
  * what the end-cell search resolved (pw_pair_key_counts): the reported end cell exactly once where the best is above 0 --
    to the first or the second cell of its pair as the cell's iteration says --, nothing with the switch off;
  * every block ran on the steady body (pw_ramp_block_counts).
"""
import ctypes

import pytest

from tests import pair_keys_cases as PC
from tests.emu import emu
from tests.test_emu_whole_plane import check_plane, pick_ends, table_cells

KEYS = ('init_rc', 'opt', 'score', 'transcript', 'origin_idx', 'mutant_idx', 'tb_null', 'would_panick')
WALKS = 12
B_LOCAL = 1
CASES = PC.cases()
IDS = [c[0][0] for c in CASES]


def _uint(name):
    fn = getattr(emu.lib(), name)
    fn.restype = ctypes.c_uint
    return int(fn(1))                      # (read and reset)


def _four(name):
    out = (ctypes.c_uint * 4)()
    getattr(emu.lib(), name)(out, 1)
    return [int(v) for v in out]           # (read and reset)


@pytest.fixture
def form(monkeypatch):
    """Sets ramp_free on, the stamp group at 4, the letter rings and the pair keys for the emulated launches that follow; all back
    to their defaults afterwards."""
    monkeypatch.delenv('PWLIB_RAMP_BLOCKS', raising=False)
    emu.lib().pw_emu_ramp_free(1)
    emu.lib().pw_emu_stamp_group(4)
    emu.lib().pw_emu_lds_feed(1)
    yield lambda on: emu.lib().pw_emu_pair_keys(int(on))
    emu.lib().pw_emu_pair_keys(-1)
    emu.lib().pw_emu_lds_feed(-1)
    emu.lib().pw_emu_stamp_group(-1)
    emu.lib().pw_emu_ramp_free(-1)


_ORACLE = {}


def _oracle(oracle, case):
    (sid, o, m, band), S, go, ge = case
    kw = dict(L=4, mode=1, alntype=B_LOCAL, diag_range=band, subst=S, go=go, ge=ge)
    if sid not in _ORACLE:
        want = oracle.solve(o, m, **kw)
        _ORACLE[sid] = (want, pick_ends(table_cells(want, len(o), len(m), 1), WALKS, 5))
    return (kw,) + _ORACLE[sid]


def _end_xy(case, want):
    """(x, y) of the oracle's end cell, None where there is none."""
    _, o, m, band = case[0]
    if want['opt'] is None or want['opt'][0] < 0:
        return None
    d = max(band[0], -len(m)) + want['opt'][0]                # banded table coordinates: (diagonal - dmin, index along it)
    return want['opt'][1] + max(d, 0), want['opt'][1] - min(d, 0)


def _run_and_check(oracle, form, case, on):
    sid, o, m, band = case[0]
    kw, want, ends = _oracle(oracle, case)
    label = '%s pair keys %d' % (sid, on)
    form(on)
    for name in ('pw_pk_add32_breaches', 'pw_feed_breaches', 'pw_group_stamps'):
        _uint(name)
    _four('pw_ramp_block_counts'), _four('pw_pair_key_counts')
    got = emu.solve(o, m, want_masks=True, ends=ends, bk=8, packed16=3, waves=1, matrix=True, **kw)
    add32, outside, stamps = _uint('pw_pk_add32_breaches'), _uint('pw_feed_breaches'), _uint('pw_group_stamps')
    blocks, resolved = _four('pw_ramp_block_counts'), _four('pw_pair_key_counts')
    nb = PC.nblocks(case[0])
    print(label, 'resolved [slots c, slots c\', end cell c, end cell c\'] =', resolved)
    check_plane(oracle, o, m, kw, got, ends, True, label)
    for key in KEYS:
        assert got.get(key) == want.get(key), (label, key, got.get(key), want.get(key))
    assert outside == 0, (label, '%d bytes or dwords asked for outside a frame' % outside)
    assert add32 == 0, (label, 'pk::add32 saw a half of H in [0xff80, 0xffff] %d times' % add32)
    assert stamps == (nb + 3) // 4 and blocks == [nb, 0, 0, 0], (label, stamps, blocks)
    xy = _end_xy(case, want)
    if on != 1:
        assert resolved == [0, 0, 0, 0], (label, resolved)
    elif xy is None or not want['score']:
        assert resolved[2:] == [0, 0], (label, resolved)
    else:
        second = PC.iteration_of(case[0], *xy) & 1
        assert resolved[2:] == [1 - second, second], (label, xy, resolved)
    return resolved


@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_pair_keys_equal_the_oracle(case, oracle, form):
    _run_and_check(oracle, form, case, 1)


@pytest.mark.parametrize('on', [0, -1])
@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_the_switch_off_keeps_one_key_per_cell(case, on, oracle, form):
    _run_and_check(oracle, form, case, on)


def test_both_resolutions_are_taken(oracle, form):
    by = dict(zip(IDS, CASES))
    first = _run_and_check(oracle, form, by['run-d0-x30'], 1)
    second = _run_and_check(oracle, form, by['run-d0-x31'], 1)
    assert first[2:] == [1, 0] and second[2:] == [0, 1], (first, second)
    # ... and among the slots that lose: A...A against A...A stamps every diagonal of the band
    ties = _run_and_check(oracle, form, by['all-A'], 1)
    assert ties[0] > 0 and ties[1] > 0, ties


def test_what_the_cases_cover(oracle):
    """The cases are what the module says they are."""
    by = dict(zip(IDS, CASES))

    def solve(sid, **extra):
        (_, o, m, band), S, go, ge = by[sid]
        return oracle.solve(o, m, L=4, mode=1, alntype=B_LOCAL, diag_range=band, subst=S, go=go, ge=ge, **extra)

    def end(sid):
        want = solve(sid)
        return want['score'], _end_xy(by[sid], want)

    def nibble(sid, x, y):
        want = solve(sid, want_table=True)
        (_, o, m, band) = by[sid][0]
        cells = table_cells(want, len(o), len(m), 1)
        return int(want['mask'][cells.index((x - y - max(band[0], -len(m)), min(x, y)))])
    # the runs: first and second cell of a pair, in slots 0 (even step, low half), 1 (odd, low), 4 (even, high), 5 (odd, high)
    seen = set()
    for d in (0, 1, 4, 5):
        for xend in (30, 31):
            sid = 'run-d%d-x%d' % (d, xend)
            assert end(sid) == (10.0, (xend, xend - d)), sid
            seen.add((PC.slot_of(by[sid][0], d), PC.iteration_of(by[sid][0], xend, xend - d) & 1))
    assert seen == {(j, r) for j in (0, 1, 4, 5) for r in (0, 1)}
    # behind a best in the first cell of a pair: the diagonal move alone on a mismatch; with the other scores: both gaps kept
    assert PC.iteration_of(by['run-d0-x30'][0], 30, 30) & 1 == 0 and nibble('run-d0-x30', 31, 31) & 7 == 0
    assert end('gaps-kept') == (20.0, (30, 30)) and nibble('gaps-kept', 31, 31) & 7 == 6
    # a diagonal's start: the edge cell is the second cell of a pair (diagonal 0) and the first (diagonal 2)
    assert end('first-d0') == (1.0, (1, 1)) and end('first-d2') == (1.0, (3, 1))
    assert PC.iteration_of(by['first-d0'][0], 0, 0) & 1 == 0 and PC.iteration_of(by['first-d2'][0], 2, 0) & 1 == 1
    # a diagonal's last cell: (X, Y), the first cell of a pair three times out of four
    par = []
    for X in (40, 41):
        for Y in (40, 41):
            sid = 'last-%dx%d' % (X, Y)
            assert end(sid) == (10.0, (X, Y)), sid
            par.append(PC.iteration_of(by[sid][0], X, Y) & 1)
    assert par == [0, 0, 0, 1]
    assert end('all-A')[0] == 37.0
    assert solve('disjoint')['score'] in (None, 0.0) and solve('best2047')['score'] == 2047.0
    # the late rise: the pair's last cell, in the last group
    for nb in (4, 5, 6, 7):
        sid = 'blocks%d-late-rise' % nb
        n = len(by[sid][0][1])
        assert PC.nblocks(by[sid][0]) == nb and end(sid) == (10.0, (n, n)) and (2 * n) // 64 == (nb - 1) // 4, sid
    assert PC.nblocks(by['short'][0]) == 1
    assert (len(by['400x390-r200'][0][1]), len(by['400x390-r200'][0][2]), by['400x390-r200'][0][3]) == (400, 390, (-200, 200))
    S = by['mixed-150x140'][1]
    assert all(v != 0 for row in S for v in row) and any(S[i][j] > 0 for i in range(4) for j in range(4) if i != j)

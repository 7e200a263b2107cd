"""The cleaning oracle (tests/graph_clean_ref.py) against what the CLEANING paragraph of include/pw_graph.h says, without a GPU:
with cleaning off it is tests/graph_ref.py; dropping never separates the two vertices of a read or an arc from its twin; one
case small enough to work out by hand, with every array written out; and a second build on the survivors drops nothing."""
import ctypes as C
import os
import re

import pytest

from tests import graph_cases as GC
from tests import graph_clean_cases as CC
from tests import graph_clean_ref as K
from tests import graph_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _layouts():
    yield 'spur', CC.spur(2, True, 4, flip=True)[0], dict(max_tip_reads=2)
    yield 'fork', CC.fork(2, 2)[0], dict(max_tip_reads=2)
    yield 'bubble3', CC.bubble((1, 2, 3))[0], dict(max_bubble_reads=3)
    yield 'ring', CC.bubble((1, 2), circular=True, orient=1)[0], dict(max_bubble_reads=2)
    yield 'spur_on_bubble', CC.spur_on_bubble()[0], dict(max_tip_reads=2, max_bubble_reads=2, rounds=2)
    yield 'hairpin', CC.hairpin()[0], dict(max_bubble_reads=2)
    yield 'comb', CC.comb()[0], dict(max_tip_reads=2, max_bubble_reads=2)


@pytest.mark.parametrize('case', ['linear', 'ring', 'ladder', 'spur', 'bubble'])
def test_with_cleaning_off_the_oracle_is_graph_ref(case):
    lens, recs = dict(linear=lambda: _lr(GC.linear(2)), ring=lambda: _lr(GC.ring(12)),
                      ladder=lambda: _lr(GC.ladder(40, 400, 20, both_strands=True)),
                      spur=lambda: (CC.spur(1, False, 4)[0].lens, CC.spur(1, False, 4)[0].records()),
                      bubble=lambda: (CC.bubble((1, 2))[0].lens, CC.bubble((1, 2))[0].records()))[case]()
    want = R.build(lens, recs)
    for params in (dict(), dict(max_tip_reads=3, max_bubble_reads=3, rounds=0), dict(rounds=2)):
        got = K.build(lens, recs, **params)
        assert got.pop('dropped') == [0] * len(lens)
        assert got == want


def _lr(case):
    return [len(r) for r in case[1]], case[2]


@pytest.mark.parametrize('name,lay,params', list(_layouts()), ids=[x[0] for x in _layouts()])
def test_dropping_keeps_reads_whole_and_arcs_in_twin_pairs(name, lay, params):
    b = K.build(lay.lens, lay.records(), **params)
    assert any(b['dropped'])
    kept = {(a[0], a[1], a[4]) for a in b['arcs'] if not a[5] & K.REMOVED}
    assert kept and all((w ^ 1, v ^ 1, src) in kept for v, w, src in kept)
    for v, w, _, _, _, f in b['arcs']:
        assert bool(f & K.DROPPED) <= bool(f & K.REMOVED) and bool(f & K.CHAIN) <= (not f & K.REMOVED)
        assert bool(f & K.DROPPED) <= bool(b['dropped'][v >> 1] or b['dropped'][w >> 1])
        assert (not f & K.REMOVED) <= (not b['dropped'][v >> 1] and not b['dropped'][w >> 1])
    member_reads = {v >> 1 for v, _, _ in b['members']}
    assert member_reads == {r for r in range(len(lay.lens)) if not b['contained'][r] and not b['dropped'][r]}


@pytest.mark.parametrize('name,lay,params', list(_layouts()), ids=[x[0] for x in _layouts()])
def test_a_second_build_on_the_survivors_drops_nothing(name, lay, params):
    if name == 'spur_on_bubble':
        params = dict(params, rounds=3)                      # (two rounds are what this case needs to come to rest)
    recs = lay.records()
    b = K.build(lay.lens, recs, **params)
    alive = [i for i, r in enumerate(recs) if not b['dropped'][r[0]] and not b['dropped'][r[1]]]
    again = K.build(lay.lens, [recs[i] for i in alive], **params)
    assert again['dropped'] == [0] * len(lay.lens)
    # the dropped reads are now reads without a record, each a unitig of its own; the others lie as they lay
    gone = {2 * r for r in range(len(lay.lens)) if b['dropped'][r]}
    assert [u[1:] for u in again['unitigs'] if u[3] not in gone] == [u[1:] for u in b['unitigs']]


def test_a_case_worked_out_by_hand():
    """A line of 8 reads of 100 letters at every 60 (reads 0 .. 7); read 8 a dead start entering read 4; read 9 a dead end
    leaving read 3; reads 10, 11 a second path from read 5 to read 7 beside read 6.  One round with max_tip_reads = 1 and
    max_bubble_reads = 2: the components are {0 2 4 6} {8 10} {12} {20 22} {14} {16} {18} and their twins.  {16} has
    in = 0, out = 1, and 6 -> 8 of the 4-member component competes at 8: read 8 is a tip.  {19}, the twin of the dead end
    {18}, has in = 0, out = 1, and 9 -> 7 of {11 9} competes at 7: read 9 is a tip.  {12} and {20 22} both run from 10 to 14;
    the longer stays: read 6 is a bubble."""
    lay = CC.Layout()
    lay.line(8)
    lay.join(lay.read(180), 4)
    lay.join(3, lay.read(240))
    lay.join(5, lay.read(340), lay.read(380), 7)
    recs = lay.records()
    assert recs == [(0, 1, 0, 60, 100, 0, 40, 40, 40), (1, 2, 0, 60, 100, 0, 40, 40, 40), (2, 3, 0, 60, 100, 0, 40, 40, 40),
                    (3, 4, 0, 60, 100, 0, 40, 40, 40), (4, 5, 0, 60, 100, 0, 40, 40, 40), (5, 6, 0, 60, 100, 0, 40, 40, 40),
                    (6, 7, 0, 60, 100, 0, 40, 40, 40), (4, 8, 0, 0, 40, 60, 100, 40, 40), (3, 9, 0, 60, 100, 0, 40, 40, 40),
                    (5, 10, 0, 40, 100, 0, 60, 60, 60), (10, 11, 0, 40, 100, 0, 60, 60, 60), (7, 11, 0, 0, 60, 40, 100, 60, 60)]
    b = K.build(lay.lens, recs, max_tip_reads=1, max_bubble_reads=2, rounds=1)
    assert b['cls'] == [5, 5, 5, 5, 5, 5, 5, 6, 5, 5, 5, 6]
    assert b['contained'] == [0] * 12
    assert b['dropped'] == [0, 0, 0, 0, 0, 0, 2, 0, 1, 1, 0, 0]
    assert b['rows'] == [0, 1, 1, 2, 3, 4, 5, 7, 8, 9, 11, 13, 14, 15, 16, 16, 18, 19, 19, 19, 20, 21, 22, 23, 24]
    C_, D_ = K.CHAIN, K.REMOVED | K.DROPPED
    assert b['arcs'] == [(0, 2, 60, 40, 0, C_), (2, 4, 60, 40, 1, C_), (3, 1, 60, 40, 0, C_), (4, 6, 60, 40, 2, C_), (5, 3, 60, 40, 1, C_),
                         (6, 8, 60, 40, 3, C_), (6, 18, 60, 40, 8, D_), (7, 5, 60, 40, 2, C_), (8, 10, 60, 40, 4, C_), (9, 7, 60, 40, 3, C_),
                         (9, 17, 60, 40, 7, D_), (10, 20, 40, 60, 9, C_), (10, 12, 60, 40, 5, D_), (11, 9, 60, 40, 4, C_),
                         (12, 14, 60, 40, 6, D_), (13, 11, 60, 40, 5, D_), (15, 23, 40, 60, 11, C_), (15, 13, 60, 40, 6, D_),
                         (16, 8, 60, 40, 7, D_), (19, 7, 60, 40, 8, D_), (20, 22, 40, 60, 10, C_), (21, 11, 40, 60, 9, C_),
                         (22, 14, 40, 60, 11, C_), (23, 21, 40, 60, 10, C_)]
    assert b['unitigs'] == [(0, 520, 9, 0, 0)]
    assert b['members'] == [(0, 60, 0), (2, 60, 60), (4, 60, 120), (6, 60, 180), (8, 60, 240), (10, 40, 300), (20, 40, 340),
                            (22, 40, 380), (14, 100, 420)]
    # read 6 hangs on read 5 (records 5 and 6 tie at 40 matches: the lower index), read 8 on read 4, read 9 on read 3
    assert K.place(lay.lens, recs, b) == [(0, 0, 0, 0, 0), (0, 0, 60, 1, 0), (0, 0, 120, 2, 0), (0, 0, 180, 3, 0), (0, 0, 240, 4, 0),
                                          (0, 0, 300, 5, 0), (0, 0, 360, 5, 1), (0, 0, 420, 7, 0), (0, 0, 180, 4, 1), (0, 0, 240, 3, 1),
                                          (0, 0, 340, 10, 0), (0, 0, 380, 11, 0)]
    # without cleaning: seven unitigs where there is one line
    assert len(K.build(lay.lens, recs)['unitigs']) == 7


def test_rounds_are_a_fixed_count_and_a_spur_can_hide_a_bubble():
    lay, spur, short, long_ = CC.spur_on_bubble()
    one = K.build(lay.lens, lay.records(), max_tip_reads=2, max_bubble_reads=2, rounds=1)
    two = K.build(lay.lens, lay.records(), max_tip_reads=2, max_bubble_reads=2, rounds=2)
    assert [r for r, d in enumerate(one['dropped']) if d] == spur and one['dropped'][spur[0]] == K.TIP
    assert {r: d for r, d in enumerate(two['dropped']) if d} == {spur[0]: K.TIP, short[0]: K.BUBBLE}
    assert len(one['unitigs']) > 1 and len(two['unitigs']) == 1
    assert K.build(lay.lens, lay.records(), max_tip_reads=2, max_bubble_reads=2, rounds=8) == two


def test_what_the_oracle_refuses():
    for bad in (dict(max_tip_reads=-1), dict(max_bubble_reads=-1), dict(rounds=-1), dict(rounds=9)):
        with pytest.raises(ValueError):
            K.build([100], [], **bad)


def test_the_new_surface_matches_the_header():
    from biseqt_amd import _pwlib as W
    from biseqt_amd import graph as G
    txt = open(os.path.join(ROOT, 'include', 'pw_graph.h')).read()
    assert ' * CLEANING ' in txt and 'Dropped reads' in open(os.path.join(ROOT, 'include', 'pw_consensus.h')).read()
    code = re.sub(r'/\*.*?\*/', '', txt, flags=re.S)
    assert int(re.search(r'#define\s+PW_ARC_DROPPED\s+(\w+)', code).group(1), 0) == 8 == W.PW_ARC_DROPPED == G.ARC_DROPPED == K.DROPPED
    fields = re.search(r'typedef struct \{ int32_t ([\w, ]+); \} pw_graph_clean_params;', code).group(1).split(', ')
    assert fields == [n for n, _ in W.pw_graph_clean_params._fields_]
    assert C.sizeof(W.pw_graph_clean_params) == 16 == W.SIZEOF['pw_graph_clean_params'] and C.sizeof(W.pw_graph_params) == 32
    lib = W.load()
    for name in ('pw_graph_build_clean', 'pw_graph_dropped', 'pw_graph_dropped_device'):
        assert name in W.GRAPH_EXPORTS and getattr(lib, name).argtypes is not None

"""Tip removal and bubble popping on the device (pw_clean.hip, K19) against tests/graph_clean_ref.py on the same planted
records (``OverlapGraph.add``): every array -- classes, contained and dropped flags, the sorted arcs with their flags, the row
index, unitigs, members, and the placements -- with ``==``, at the smallest shapes at which a kernel can still go wrong."""
import numpy as np
import pytest

from tests import graph_cases as GC
from tests import graph_clean_cases as CC
from tests import graph_clean_ref as K
from tests import graph_ref as R

pytestmark = pytest.mark.gpu
KEYS = ('cls', 'contained', 'dropped', 'rows', 'arcs', 'unitigs', 'members')


def _snapshot(G):
    got = GC.snapshot(G)
    got['dropped'] = G.dropped().tolist()
    return got


def _check(lens, records, max_tip_reads=0, max_bubble_reads=0, clean_rounds=1, **params):
    from biseqt_amd.graph import OverlapGraph
    want = K.build(lens, records, max_tip_reads=max_tip_reads, max_bubble_reads=max_bubble_reads, rounds=clean_rounds, **params)
    with OverlapGraph(lens) as G:
        G.add(records)
        G.build(max_tip_reads=max_tip_reads, max_bubble_reads=max_bubble_reads, clean_rounds=clean_rounds, **params)
        got = _snapshot(G)
        places = G.placements()[['unitig', 'rev', 'pos', 'root', 'depth']].tolist()
    for key in KEYS:
        assert got[key] == want[key], key
    assert places == K.place(lens, records, want)
    return want


def _gone(want):
    return {r: d for r, d in enumerate(want['dropped']) if d}


def test_empty_graph_one_read_and_a_line_without_a_branch():
    assert _check([], [], max_tip_reads=2, max_bubble_reads=2)['unitigs'] == []
    assert _check([100], [], max_tip_reads=2, max_bubble_reads=2, clean_rounds=2)['unitigs'] == [(0, 100, 1, 0, 0)]
    lay = CC.Layout()
    lay.line(9, orient=[0, 1, 1, 0, 1, 0, 0, 1, 0])
    want = _check(lay.lens, lay.records(), max_tip_reads=4, max_bubble_reads=4, clean_rounds=3)
    assert _gone(want) == {} and len(want['unitigs']) == 1
    assert want == dict(R.build(lay.lens, lay.records()), dropped=[0] * 9)


@pytest.mark.parametrize('flip', [False, True])
@pytest.mark.parametrize('dead_end', [False, True])
@pytest.mark.parametrize('k', [1, 2, 3])
def test_spurs_at_the_bound_and_one_past_it(k, dead_end, flip):
    lay, _, ids = CC.spur(k, dead_end, 4, flip)
    want = _check(lay.lens, lay.records(), max_tip_reads=2)
    assert _gone(want) == ({x: K.TIP for x in ids} if k <= 2 else {})
    assert len(want['unitigs']) == (1 if k <= 2 else 3)


@pytest.mark.parametrize('k', [1, 2, 3])
def test_a_spur_beside_the_line_s_own_short_start(k):
    """Attached to read 1, the spur competes with read 0, a tip candidate of one read itself: at equal length the smaller read
    index stays, a longer spur wins, and a spur past the bound is no candidate and therefore stronger."""
    lay, _, ids = CC.spur(k, False, 1)
    want = _check(lay.lens, lay.records(), max_tip_reads=2)
    assert _gone(want) == ({ids[0]: K.TIP} if k == 1 else {0: K.TIP})
    lay, _, ids = CC.spur(k, True, 1, flip=True)             # as a dead end it has no competitor but the line itself
    want = _check(lay.lens, lay.records(), max_tip_reads=2)
    assert _gone(want) == ({x: K.TIP for x in ids} if k <= 2 else {})


def test_a_y_whose_branches_tie_and_paths_that_stay():
    lay, _, b1, b2 = CC.fork(2, 2)
    assert _gone(_check(lay.lens, lay.records(), max_tip_reads=2)) == {x: K.TIP for x in b2}       # mr decides: b1 holds the smaller read
    lay, _, b1, b2 = CC.fork(1, 2)
    assert _gone(_check(lay.lens, lay.records(), max_tip_reads=2)) == {b1[0]: K.TIP}
    lay = CC.only_way_in()[0]                               # the only predecessor of a fork
    assert _gone(_check(lay.lens, lay.records(), max_tip_reads=2, max_bubble_reads=4, clean_rounds=2)) == {}
    lay = CC.Layout()                                       # an isolated component of two reads
    lay.line(2)
    assert _gone(_check(lay.lens, lay.records(), max_tip_reads=2, max_bubble_reads=2)) == {}
    lay = CC.different_sinks()[0]                           # one source, two sinks: no bubble
    assert _gone(_check(lay.lens, lay.records(), max_bubble_reads=3, clean_rounds=2)) == {}


@pytest.mark.parametrize('circular', [False, True])
@pytest.mark.parametrize('sizes,bound,loser', [((1, 2), 2, [0]), ((2, 2), 2, [1]), ((1, 2, 3), 3, [0, 1]), ((2, 3), 3, [0]), ((2, 3), 2, []),
                                               ((2, 1), 1, [])])
def test_bubbles_at_the_bound_and_one_past_it(sizes, bound, loser, circular):
    """The longer path stays, at equal length the one with the smaller read; a path past the bound is no candidate, and then
    nothing is popped.  ``circular``: the same bubble on a ring -- a circular unitig once it is popped."""
    lay, _, paths, _ = CC.bubble(sizes, circular=circular, orient=int(circular))
    want = _check(lay.lens, lay.records(), max_bubble_reads=bound)
    assert _gone(want) == {x: K.BUBBLE for q in loser for x in paths[q]}
    if loser:
        assert [u[4] for u in want['unitigs']] == [int(circular)]


def test_a_hairpin():
    lay, s, x, ys = CC.hairpin(second_path=False)           # {x} against its own twin: equal n, equal mr, neither goes
    assert _gone(_check(lay.lens, lay.records(), max_bubble_reads=2)) == {}
    lay, s, x, ys = CC.hairpin()
    assert _gone(_check(lay.lens, lay.records(), max_bubble_reads=2)) == {x: K.BUBBLE}


def test_a_spur_on_a_bubble_needs_two_rounds():
    lay, spur, short, _ = CC.spur_on_bubble()
    one = _check(lay.lens, lay.records(), max_tip_reads=2, max_bubble_reads=2, clean_rounds=1)
    assert _gone(one) == {spur[0]: K.TIP} and len(one['unitigs']) > 1
    two = _check(lay.lens, lay.records(), max_tip_reads=2, max_bubble_reads=2, clean_rounds=2)
    assert _gone(two) == {spur[0]: K.TIP, short[0]: K.BUBBLE} and len(two['unitigs']) == 1
    assert _check(lay.lens, lay.records(), max_tip_reads=2, max_bubble_reads=2, clean_rounds=8) == two


def test_more_than_one_workgroup_and_a_row_longer_than_a_wavefront():
    lay, spurs, iso = CC.comb()
    want = _check(lay.lens, lay.records(), max_tip_reads=2, max_bubble_reads=2)
    assert max(b - a for a, b in zip(want['rows'], want['rows'][1:])) > 64 and len(want['rows']) - 1 > 256
    assert _gone(want) == {x: K.TIP for x in spurs}
    assert [u[2] for u in want['unitigs']] == [140, 2]


def test_contigs_and_placements_after_cleaning():
    from biseqt_amd.graph import OverlapGraph
    lay, x1, x2, c = CC.hanging()
    lens, recs, reads = lay.lens, lay.records(), lay.reads()
    want = K.build(lens, recs, max_tip_reads=2)
    assert _gone(want) == {x1: K.TIP, x2: K.TIP} and want['contained'][c] == 1
    with OverlapGraph(lens) as G:
        G.add(recs)
        G.build(max_tip_reads=2)
        assert _snapshot(G) == want
        got = [x.tolist() for x in G.contigs(reads, complement=GC.COMPLEMENT)]
        places = G.placements()[['unitig', 'rev', 'pos', 'root', 'depth']].tolist()
    assert got == R.contigs(reads, want['unitigs'], want['members'], GC.COMPLEMENT)
    assert places == K.place(lens, recs, want)
    assert places[x1][0] == 0 and places[x1][3:] == (2, 1)   # the dropped read hangs on read 2, its live neighbour
    assert places[x2] == (-1, 0, 0, 0, 0)                   # no live neighbour: unplaced
    assert places[c][0] == 0 and places[c][3:] == (2, 2)     # the contained read resolves through the dropped one


def test_rebuilds_refusals_and_accessors_before_a_build():
    from biseqt_amd import _pwlib as W
    from biseqt_amd.graph import OverlapGraph
    import ctypes as C
    lay, _, ids = CC.spur(1, True, 4)
    lens, recs = lay.lens, lay.records()
    with OverlapGraph(lens) as G:
        with pytest.raises(RuntimeError, match='before pw_graph_build'):
            G.dropped()
        assert not G.lib.pw_graph_dropped_device(G.handle)
        G.add(recs)
        for bad in (dict(max_tip_reads=-1), dict(max_bubble_reads=-1), dict(max_tip_reads=1, clean_rounds=9), dict(clean_rounds=-1)):
            with pytest.raises(ValueError):
                G.build(**bad)
        p = W.pw_graph_params(1000, 0, 10, 0, .8, 0.)
        for bad in ((-1, 0, 1), (0, -1, 1), (1, 1, -1), (1, 1, 9)):
            c = W.pw_graph_clean_params(bad[0], bad[1], bad[2], 0)
            assert G.lib.pw_graph_build_clean(G.handle, C.byref(p), C.byref(c), None) != 0
            assert 'pw_graph_build_clean' in W.last_error()
        with pytest.raises(RuntimeError, match='before pw_graph_build'):
            G.dropped()                                      # (a refused build builds nothing)
        G.build(max_tip_reads=2)
        assert _snapshot(G) == K.build(lens, recs, max_tip_reads=2) and G.dropped()[ids[0]] == 1
        bytes_on = G.device_bytes
        G.build()                                            # cleaning off after cleaning on: exactly the plain build
        assert _snapshot(G) == dict(R.build(lens, recs), dropped=[0] * len(lens))
        assert G.lib.pw_graph_dropped_device(G.handle) and G.device_bytes >= bytes_on      # (the cleaning arrays stay allocated)
        assert G.lib.pw_graph_build_clean(G.handle, C.byref(p), None, None) == 0           # a NULL third argument is pw_graph_build
        assert _snapshot(G) == dict(R.build(lens, recs), dropped=[0] * len(lens))
        G.build(max_tip_reads=2, clean_rounds=0)
        assert _snapshot(G) == dict(R.build(lens, recs), dropped=[0] * len(lens))
    with OverlapGraph(lens) as G:                            # the new arrays are counted
        G.add(recs)
        G.build()
        plain = G.device_bytes
        G.build(max_tip_reads=2)
        assert G.device_bytes > plain

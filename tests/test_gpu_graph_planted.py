"""The overlap graph on the device against tests/graph_ref.py on the same planted records (``OverlapGraph.add``): every
array -- classes, contained flags, the sorted arcs with their flags, the row index, unitigs and members -- with ``==``."""
import numpy as np
import pytest

from tests import graph_cases as GC
from tests import graph_ref as R

pytestmark = pytest.mark.gpu


def _check(lens, records, **params):
    want = R.build(lens, records, **params)
    got = GC.device_build(lens, records, **params)
    for key in ('cls', 'contained', 'rows', 'arcs', 'unitigs', 'members'):
        assert got[key] == want[key], key
    return want


def test_empty_graph_and_one_read():
    assert _check([], [])['unitigs'] == []
    want = _check([100], [])
    assert want['unitigs'] == [(0, 100, 1, 0, 0)] and want['members'] == [(0, 100, 0)]
    want = _check([100, 0, 7], [])                         # no records: every read is a unitig of one, a read of no letters too
    assert [u[1] for u in want['unitigs']] == [100, 0, 7]


# (name, lens, record, params, class)
TWO_READS = [
    ('none', [100, 100], (0, 1, 0, 0, 0, 0, 0, 0, 0), {}, R.NONE),
    ('weak', [100, 100], (0, 1, 0, 70, 100, 0, 30, 30, 30), dict(min_overlap=40), R.WEAK),
    ('internal', [100, 100], (0, 1, 0, 30, 60, 30, 60, 30, 30), {}, R.INTERNAL),
    ('a_contained', [50, 100], (0, 1, 0, 0, 50, 20, 70, 50, 50), {}, R.A_CONTAINED),
    ('b_contained', [100, 50], (0, 1, 0, 20, 70, 0, 50, 50, 50), {}, R.B_CONTAINED),
    ('a_to_b', [100, 100], (0, 1, 0, 60, 100, 0, 40, 40, 40), {}, R.A_TO_B),
    ('b_to_a', [100, 100], (0, 1, 0, 0, 40, 60, 100, 40, 40), {}, R.B_TO_A),
    ('a_to_b minus', [100, 90], (0, 1, 1, 60, 100, 0, 40, 38, 42), {}, R.A_TO_B),
    ('b_to_a minus', [100, 90], (0, 1, 1, 0, 40, 50, 90, 40, 40), {}, R.B_TO_A),
    # ext against max_hang: 100 is not above 100, 101 is
    ('hang at', [2000, 2000], (0, 1, 0, 600, 2000, 100, 1500, 1400, 1400), dict(max_hang=100), R.A_TO_B),
    ('hang past', [2000, 2000], (0, 1, 0, 601, 2000, 101, 1500, 1399, 1399), dict(max_hang=100), R.INTERNAL),
    # ext against span * int_frac: 200 * .5 and 125 * .8 are 100.0
    ('frac at', [400, 600], (0, 1, 0, 200, 400, 100, 300, 200, 200), dict(int_frac=.5), R.A_TO_B),
    ('frac past', [400, 600], (0, 1, 0, 200, 400, 101, 301, 200, 200), dict(int_frac=.5), R.INTERNAL),
    ('frac .8 at', [325, 600], (0, 1, 0, 200, 325, 100, 225, 125, 125), {}, R.A_TO_B),
    ('frac .8 past', [325, 600], (0, 1, 0, 200, 325, 101, 226, 125, 125), {}, R.INTERNAL),
    # a_beg == b_beg is a containment, one past it a dovetail
    ('begs equal', [100, 120], (0, 1, 0, 40, 100, 40, 100, 60, 60), {}, R.A_CONTAINED),
    ('begs one apart', [100, 120], (0, 1, 0, 41, 100, 40, 99, 59, 59), {}, R.A_TO_B),
    # equal tails are a containment, one past them a dovetail
    ('tails equal', [100, 60], (0, 1, 0, 50, 100, 10, 60, 50, 50), {}, R.B_CONTAINED),
    ('tails one apart', [100, 61], (0, 1, 0, 50, 100, 10, 60, 50, 50), {}, R.A_TO_B),
    ('min_overlap at', [100, 100], (0, 1, 0, 60, 100, 0, 41, 40, 41), dict(min_overlap=40), R.A_TO_B),
    ('min_overlap past', [100, 100], (0, 1, 0, 60, 100, 0, 41, 40, 41), dict(min_overlap=41), R.WEAK),
    ('min_identity at', [100, 100], (0, 1, 0, 60, 100, 0, 40, 9, 10), dict(min_identity=.9), R.A_TO_B),
    ('min_identity past', [100, 100], (0, 1, 0, 60, 100, 0, 40, 9, 10), dict(min_identity=.91), R.WEAK),
    ('min_identity .7', [100, 100], (0, 1, 0, 60, 100, 0, 40, 7, 10), dict(min_identity=.7), R.A_TO_B),
    ('min_identity .7 below', [100, 100], (0, 1, 0, 60, 100, 0, 40, 6, 10), dict(min_identity=.7), R.WEAK),
]


@pytest.mark.parametrize('name,lens,record,params,cls', TWO_READS, ids=[c[0] for c in TWO_READS])
def test_two_reads_in_every_class_and_at_every_boundary(name, lens, record, params, cls):
    want = _check(lens, [record], **params)
    assert want['cls'] == [cls]
    assert len(want['arcs']) == (2 if cls in (R.A_TO_B, R.B_TO_A) else 0)


@pytest.mark.parametrize('fuzz,reduced', [(10, True), (9, False)])
def test_fuzz_at_its_edge_and_one_past(fuzz, reduced):
    # 0 -> 2 and 2 -> 4 of 40 each against 0 -> 4 of 70: 80 <= 70 + 10, 80 > 70 + 9
    recs = [(0, 1, 0, 40, 100, 0, 60, 60, 60), (1, 2, 0, 40, 100, 0, 60, 60, 60), (0, 2, 0, 70, 100, 0, 30, 30, 30)]
    want = _check([100, 100, 100], recs, fuzz=fuzz)
    assert [a[5] for a in want['arcs'] if (a[0], a[1]) == (0, 4)] == [R.REDUCED | R.REMOVED if reduced else 0]
    assert len(want['unitigs']) == (1 if reduced else 3)


def test_dense_ladder_rows_longer_than_a_wavefront():
    _, reads, recs = GC.ladder(100, 400, 5)
    want = _check([len(r) for r in reads], recs)
    assert max(np.diff(want['rows'])) == 79 and [u[2] for u in want['unitigs']] == [100]


@pytest.mark.parametrize('n', [32, 33, 64, 65])
def test_chains_at_the_edges_of_the_doubling_rounds(n):
    _, reads, recs = GC.ladder(n, 100, 60, both_strands=True)
    want = _check([len(r) for r in reads], recs)
    assert [u[2] for u in want['unitigs']] == [n]


@pytest.mark.parametrize('n', [12, 65])
def test_rings(n):
    _, reads, recs = GC.ring(n)
    want = _check([len(r) for r in reads], recs)
    assert want['unitigs'] == [(0, 100 * n, n, 0, 1)] and len(want['arcs']) == 6 * n


def test_every_read_contained_but_one():
    lens = [1000] + [100] * 10
    recs = [(0, k, k & 1, 80 * k, 80 * k + 100, 0, 100, 100, 100) for k in range(1, 11)]
    want = _check(lens, recs)
    assert want['contained'] == [0] + [1] * 10 and want['arcs'] == [] and want['unitigs'] == [(0, 1000, 1, 0, 0)]


@pytest.mark.parametrize('seed,n_reads', [(1, 150), (2, 150), (1, 60), (3, 60)])
def test_linear_layouts_on_both_strands(seed, n_reads):
    _, reads, recs = GC.linear(seed, n_reads=n_reads)
    want = _check([len(r) for r in reads], recs)
    assert (len(want['unitigs']) == 1) == (n_reads == 150)          # 60 reads cover too thinly for one unitig
    _check([len(r) for r in reads], recs, fuzz=0, min_overlap=120, max_hang=40)


def test_a_branch_breaks_the_unitigs():
    _, reads, recs = GC.ladder(6, 100, 60)
    recs = recs + [(2, 6, 0, 50, 100, 0, 50, 50, 50)]      # read 6 follows read 2 as read 3 does, and knows nothing of read 3
    want = _check([100] * 7, recs)
    assert sorted(a[1] for a in want['arcs'] if a[0] == 4 and not a[5] & R.REMOVED) == [6, 12]
    assert [u[2] for u in want['unitigs']] == [3, 3, 1]


def test_rebuild_with_other_parameters_and_more_records():
    from biseqt_amd.graph import OverlapGraph
    _, reads, recs = GC.linear(2, n_reads=60)
    lens = [len(r) for r in reads]
    with OverlapGraph(lens) as G:
        G.add(recs[:100])
        for params in (dict(), dict(min_overlap=150, fuzz=0), dict(max_hang=10, int_frac=.1)):
            G.build(**params)
            assert GC.snapshot(G) == R.build(lens, recs[:100], **params)
        G.add(recs[100:])
        G.build()
        assert GC.snapshot(G) == R.build(lens, recs)
        assert len(G) == len(recs) and G.device_bytes > 0


def test_what_the_library_refuses():
    from biseqt_amd.graph import OverlapGraph
    ok = (0, 1, 0, 60, 100, 0, 40, 40, 40)
    with OverlapGraph([100, 100]) as G:
        for bad, what in (((0, 0, 0, 60, 100, 0, 40, 40, 40), 'itself'), ((0, 2, 0, 60, 100, 0, 40, 40, 40), 'outside the graph'),
                          ((-1, 1, 0, 60, 100, 0, 40, 40, 40), 'outside the graph'), ((0, 1, 2, 60, 100, 0, 40, 40, 40), 'strand'),
                          ((0, 1, 0, 60, 101, 0, 40, 40, 40), 'interval'), ((0, 1, 0, 60, 100, 41, 40, 40, 40), 'interval'),
                          ((0, 1, 0, 60, 100, -1, 40, 40, 40), 'interval'), ((0, 1, 0, 60, 100, 0, 40, 41, 40), 'n_match')):
            with pytest.raises(RuntimeError, match=what):
                G.add([ok, bad])
        assert len(G) == 0                                 # a refused call appends nothing
        with pytest.raises(RuntimeError, match='before pw_graph_build'):
            G.arcs()
        with pytest.raises(ValueError):
            G.build(fuzz=-1)
        G.add([ok])
        G.build()
        G.add([(0, 1, 1, 60, 100, 0, 40, 40, 40)])        # the other strand is another key
        G.build()
        G.add([ok])
        with pytest.raises(RuntimeError, match=r'duplicate overlap key \(0, 1, 0\)'):
            G.build()
    with pytest.raises(ValueError):
        R.build([100, 100], [ok, ok])

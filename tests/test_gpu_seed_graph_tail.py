"""The host code the three seed indexes share behind their graphs' count pass (pw_seed_host.h: graph_sort, graph_finish,
the read-backs and graph_components; seeds._Handle on the Python side), on the paths the rest of the suite reaches
unevenly: no points at all, points without an edge, a small graph against the dense oracle
(oracle/mseeds_dense_oracle.py, applied to the index's own points), and a second graph_build on the same handle.  The
indexes: seeds._Index for a pair and for a self comparison, seeds._MIndex with three sequences, seeds._QIndex with three
queries of which one is empty.  Sequences hold at most 40 letters of 'ACGT'.  Every comparison is exact."""
import numpy as np
import pytest

from biseqt_amd.seeds import _Index, _MIndex, _QIndex
from biseqt_amd.sequence import Alphabet
from oracle import mseeds_dense_oracle as DO
from tests.qseeds_cases import pack_tight

pytestmark = pytest.mark.gpu

A = Alphabet('ACGT')
K, D_COEFF, RADIUS, LARGER = 2, 0.5, 3., 6.
KINDS = ('pair', 'self', 'nway', 'queries')


def _letters(seed, n=30):
    return np.random.default_rng(seed).integers(0, 4, n).astype(np.uint8)


def _none():
    return np.zeros(0, np.uint8)


def make(kind, points=True):
    """A built index of `kind`: with points, K-mers of 30 random letters per sequence; without, a word longer than one of
    the sequences -- for the self comparison 'ACGT' with k = 4, whose only seed is the trivial one."""
    if kind == 'pair':
        x = _Index(_letters(1), _letters(2), K, A, self_comp=0) if points else _Index(_letters(1, 4), _letters(2), 5, A, self_comp=0)
    elif kind == 'self':
        s = _letters(3) if points else np.arange(4, dtype=np.uint8)
        x = _Index(s, s, K if points else 4, A, self_comp=1)
    elif kind == 'nway':
        x = _MIndex([_letters(4), _letters(5, 4 if not points else 30), _letters(6)], K if points else 5, A)
    else:
        x = _QIndex(_letters(7), K if points else 5, A)
        x.build(*pack_tight([_letters(8), _none(), _letters(9, 20)] if points else [_letters(8, 4), _none(), _letters(9, 3)]))
        return x
    x.build()
    return x


def points_of(kind, x):
    """(the points the oracle takes -- (d.., a) per point --, the index ranges edges stay inside); after a graph_build"""
    if kind in ('pair', 'self'):
        p = x.graph_points()
        return p, [(0, len(p))]
    if kind == 'nway':
        p = x.rows()
        return p, [(0, len(p))]
    off = x.row_offsets().tolist()
    return x.rows()[:, 1:], list(zip(off[:-1], off[1:]))


def oracle_neighbours(kind, x, radius):
    """The dense oracle on the index's own points, query by query for the query-batched index (shifted by its row offsets)"""
    p, ranges = points_of(kind, x)
    out = []
    for b, e in ranges:
        out.extend([b + v for v in ns] for ns in DO.neighbours_cr(p[b:e], D_COEFF, radius))
    return out


def adjacency(x, n):
    off, adj = x.graph_fetch()
    assert off.dtype == np.int64 and adj.dtype == np.int32
    assert off[0] == 0 and len(off) == n + 1 and (np.diff(off) >= 0).all() and off[-1] == len(adj)
    assert np.array_equal(np.diff(off), x.graph_counts())
    return [sorted(adj[off[i]:off[i + 1]].tolist()) for i in range(n)]


def check_graph(kind, x, radius, want):
    """graph_build's return value, graph_counts, the sorted lists of graph_fetch and the component labels == the oracle"""
    n = len(want)
    assert x.graph_build(D_COEFF, radius) == sum(len(v) for v in want)
    assert len(points_of(kind, x)[0]) == n
    counts = x.graph_counts()
    assert counts.dtype == np.int32 and counts.tolist() == [len(v) for v in want]
    assert adjacency(x, n) == want
    rng = np.random.default_rng(n)
    for avail in (np.zeros(n, bool), rng.random(n) < .5, np.ones(n, bool)):
        got = x.graph_components(avail)
        assert got.dtype == np.int32 and got.tolist() == DO.components(want, avail.tolist())


@pytest.fixture(scope='module', params=KINDS)
def built(request):
    """(kind, an index with points, the oracle's neighbour lists at RADIUS and at LARGER): one handle per kind for the
    whole module, so every test below that builds a graph builds it on a handle that has held another"""
    kind = request.param
    x = make(kind)
    x.graph_build(D_COEFF, RADIUS)                    # (the pairwise index lists its points only after a graph_build)
    want = {r: oracle_neighbours(kind, x, r) for r in (RADIUS, LARGER)}
    yield kind, x, want
    x.close()


@pytest.mark.parametrize('kind', KINDS)
def test_no_points_at_all(kind):
    x = make(kind, points=False)
    assert x.graph_build(D_COEFF, RADIUS) == 0
    assert len(points_of(kind, x)[0]) == 0
    counts = x.graph_counts()
    assert counts.dtype == np.int32 and counts.shape == (0,)
    off, adj = x.graph_fetch()
    assert off.tolist() == [0] and off.dtype == np.int64 and adj.shape == (0,)
    labels = x.graph_components(np.zeros(0, np.uint8))
    assert labels.dtype == np.int32 and labels.shape == (0,)
    x.close()


def test_points_but_no_edges(built):
    """Radius 0: the points of an index differ in (d.., a), so nothing is within 0 of anything else."""
    kind, x, _ = built
    assert x.graph_build(D_COEFF, 0.) == 0
    p, ranges = points_of(kind, x)
    n = len(p)
    assert n >= 24 and all(len(np.unique(p[b:e], axis=0)) == e - b for b, e in ranges)
    assert x.graph_counts().tolist() == [0] * n
    off, adj = x.graph_fetch()
    assert off.tolist() == [0] * (n + 1) and adj.shape == (0,)
    assert x.graph_components(np.ones(n, np.uint8)).tolist() == list(range(n))
    avail = np.random.default_rng(n).random(n) < .5
    assert x.graph_components(avail).tolist() == np.where(avail, np.arange(n), -1).tolist()


def test_a_few_dozen_points_with_edges(built):
    kind, x, want = built
    neighs = want[RADIUS]
    labels = DO.components(neighs, [True] * len(neighs))
    assert 24 <= len(neighs) <= 200 and sum(len(v) for v in neighs) >= 1 and 2 <= len(set(labels)) < len(neighs)
    check_graph(kind, x, RADIUS, neighs)
    if kind == 'queries':
        assert x.timings()['rounds'] >= 1


def test_a_smaller_graph_after_a_larger_one_on_the_same_handle(built):
    kind, x, want = built
    assert sum(len(v) for v in want[RADIUS]) < sum(len(v) for v in want[LARGER])
    check_graph(kind, x, LARGER, want[LARGER])
    check_graph(kind, x, RADIUS, want[RADIUS])        # the buffers of the larger graph are reused: nothing of it is left


@pytest.mark.parametrize('kind', ('pair', 'nway', 'queries'))
def test_graph_fetch_before_any_graph_build_is_refused(kind):
    x = make(kind)
    with pytest.raises(RuntimeError, match='graph_fetch before a successful pw_m?q?seeds_graph_build'):
        x.graph_fetch()
    x.close()

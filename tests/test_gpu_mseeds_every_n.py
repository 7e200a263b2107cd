"""The N-way seed index (kernels K9 of pw_mseeds.hip) at every sequence count 2 .. 16 and at the edges of its chunks,
windows and radii, against the dense oracle (oracle/mseeds_dense_oracle.py).  The inputs are the named cases of
tests/mseeds_cases.py; tests/test_mseeds_cases.py proves on the CPU that each reaches what it is named for.  Every
comparison is exact."""
import numpy as np
import pytest

from biseqt_amd.blot import WordBlotMultipleFast
from biseqt_amd.seeds import _MIndex
from biseqt_amd.sequence import Alphabet, Sequence
from oracle import mseeds_dense_oracle as DO
from tests import mseeds_cases as MC

pytestmark = pytest.mark.gpu

_LETTERS = '0123456789ABCDEFGHIJKLMNOPQRSTUVWXYZ'


def alphabet(c):
    return Alphabet('ACGT' if c['L'] == 4 else _LETTERS[:c['L']])


def index(c):
    idx = _MIndex(c['seqs'], c['wordlen'], alphabet(c))
    idx.build()
    return idx


def blot(c):
    A = alphabet(c)
    return WordBlotMultipleFast(*[Sequence(A, s) for s in c['seqs']], wordlen=c['wordlen'], alphabet=A, g_max=.2,
                                sensitivity=.9, allowed_memory=2)


def check_rows(idx, c):
    want = MC.rows_of(c)
    got = idx.rows()
    assert idx.num_rows() == len(want) and got.shape == want.shape and got.dtype == np.int32
    assert np.array_equal(got, want)
    return want


def adjacency(idx):
    off, adj = idx.graph_fetch()
    assert off[0] == 0 and len(off) == idx.num_rows() + 1 and (np.diff(off) >= 0).all() and off[-1] == len(adj)
    return [sorted(adj[off[i]:off[i + 1]].tolist()) for i in range(idx.num_rows())]


def check_graph(idx, rows, c, R_):
    """graph_build(c, R): edge total, graph_counts and the sorted lists of graph_fetch == the dense oracle."""
    want = DO.neighbours_cr(rows, c, R_)
    assert idx.graph_build(c, R_) == sum(len(x) for x in want)
    assert idx.graph_counts().tolist() == [len(x) for x in want]
    assert adjacency(idx) == want
    return want


def check_boxes(idx, rows, n_boxes, batches, WB=None):
    lo, hi, have = MC.boxes(rows, n_boxes, 1)
    want = DO.box_counts(rows, lo, hi, have)              # once; every batch is a prefix
    for nb in batches:
        got = idx.count_many(lo[:nb], hi[:nb], have[:nb])
        assert got.dtype == np.int64 and got.tolist() == want[:nb].tolist(), nb
    if WB is not None:
        bands = MC.as_bands(lo, hi, have)[:min(n_boxes, 129)]
        assert WB.seed_counts(bands) == want[:len(bands)].tolist()
        assert [WB.seed_count(ds_band=ds, a_band=a) for ds, a in bands[:8]] == want[:8].tolist()
        assert WB.seed_count() == len(rows)


# ---- every N -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('N', [2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16])
def test_every_sequence_count(N):
    c = MC.every_n(N)
    WB = blot(c)
    idx = WB._idx
    rows = check_rows(idx, c)
    assert np.array_equal(WB.rows(), rows) and [list(ds) + [a] for ds, a in WB.seeds()] == rows.tolist()
    d_radius, a_radius = MC.EVERY_N_RADII
    found = WB.find_all_neighbors(d_radius, a_radius)
    want = check_graph(idx, rows, 1. * a_radius / d_radius, a_radius)
    assert [list(ds) + [a] for (ds, a), _ in found] == rows.tolist() and [sorted(nb) for _, nb in found] == want
    rng = np.random.default_rng(N)
    for avail in (np.ones(len(rows), bool), rng.random(len(rows)) < .5, rng.random(len(rows)) < .9, np.zeros(len(rows), bool)):
        assert idx.graph_components(avail).tolist() == DO.components(want, avail.tolist())
    check_boxes(idx, rows, 129, (129,), WB)


@pytest.mark.parametrize('make', [MC.with_an_empty_member, MC.with_a_member_one_short_of_a_word])
def test_a_member_without_a_word_leaves_an_empty_index(make):
    c = make()
    idx = index(c)
    assert idx.num_rows() == 0 and idx.rows().shape == (0, c['N'])
    N = c['N']
    assert idx.count_many(np.zeros((3, N)), np.zeros((3, N)), np.zeros((3, N))).tolist() == [0, 0, 0]
    assert idx.graph_build(2., 10.) == 0 and idx.graph_counts().tolist() == []
    off, adj = idx.graph_fetch()
    assert off.tolist() == [0] and len(adj) == 0
    assert idx.graph_components(np.zeros(0, bool)).tolist() == []


# ---- mixed radix ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('N', MC.MIXED_N)
def test_unequal_radices(N):
    c = MC.mixed_radix(N)
    WB = blot(c)
    rows = check_rows(WB._idx, c)
    want = check_graph(WB._idx, rows, 10. * N / 12, 10. * N)
    assert [sorted(nb) for _, nb in WB.find_all_neighbors(12, 10 * N)] == want
    rng = np.random.default_rng(N)
    for avail in (np.ones(len(rows), bool), rng.random(len(rows)) < .5):
        assert WB._idx.graph_components(avail).tolist() == DO.components(want, avail.tolist())
    check_boxes(WB._idx, rows, 129, (129,), WB)


@pytest.mark.parametrize('start', MC.WINDOW_STARTS)
@pytest.mark.parametrize('N', MC.MIXED_N)
def test_a_kmer_across_whole_expand_windows(N, start):
    c = MC.windows(N, start)
    idx = index(c)
    rows = check_rows(idx, c)
    check_boxes(idx, rows, 129, (65, 129))


def test_sixteen_sequences_of_radix_two():
    c = MC.radix_two_everywhere()
    idx = index(c)
    rows = check_rows(idx, c)
    check_boxes(idx, rows, 129, (64, 129))


# ---- near misses ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('N', MC.NEAR_N)
def test_one_coordinate_on_the_radius_and_one_past_it(N):
    for delta in (MC.NEAR_D, MC.NEAR_D + 1):
        c = MC.near_miss(N, delta)
        WB = blot(c)
        rows = check_rows(WB._idx, c)
        found = WB.find_all_neighbors(MC.NEAR_D, MC.NEAR_A)
        want = check_graph(WB._idx, rows, 1. * MC.NEAR_A / MC.NEAR_D, MC.NEAR_A)
        assert [sorted(nb) for _, nb in found] == want
        assert sum(len(x) for x in want) == (2 * (N - 1) if delta == MC.NEAR_D else 0)


@pytest.mark.parametrize('N', MC.A_AXIS_N)
def test_the_a_axis_on_the_radius_and_one_short_of_it(N):
    c = MC.a_axis(N)
    idx = index(c)
    rows = check_rows(idx, c)
    R_ = c['radius']
    first, last = 0, len(rows) - 1
    if len(rows) <= 6000:
        assert sum(len(x) for x in check_graph(idx, rows, R_, R_)) == 2
        assert sum(len(x) for x in check_graph(idx, rows, R_, R_ - 1)) == 0
    else:
        # past the quadratic oracle; tests/test_mseeds_cases.py shows that this edge is the whole graph
        assert DO.neighbours_cr(rows[[first, last]], R_, R_) == [[1], [0]]
        assert idx.graph_build(R_, R_) == 2
        counts, adj = idx.graph_counts(), adjacency(idx)
        assert np.flatnonzero(counts).tolist() == [first, last] and adj[first] == [last] and adj[last] == [first]
        assert idx.graph_build(R_, R_ - 1) == 0 and not idx.graph_counts().any()
    assert idx.graph_build(R_, R_) == 2
    labels = idx.graph_components(np.ones(len(rows), bool))
    assert labels[last] == first and np.array_equal(np.delete(labels, last), np.delete(np.arange(len(rows)), last))


# ---- rounding ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('axis', [1, 2])
@pytest.mark.parametrize('c_R_d0', [(MC.ROUND_C, MC.ROUND_R, MC.ROUNDING_D0[0]), (MC.ROUND_C, MC.ROUND_R, MC.ROUNDING_D0[1]),
                                    MC.ROUNDING_OTHER_WAY])
def test_the_neighbour_test_rounds_as_the_kd_tree_does(axis, c_R_d0):
    c_, R_, d0 = c_R_d0
    c = MC.rounding(axis, d0)
    idx = index(c)
    rows = check_rows(idx, c)
    check_graph(idx, rows, c_, R_)


# ---- chains --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('R_', MC.CHAIN_RADII)
def test_components_along_a_scrambled_chain(R_):
    c = MC.chain()
    idx = index(c)
    rows = check_rows(idx, c)
    want = check_graph(idx, rows, 1., R_)
    for name, avail in MC.chain_masks(len(rows)).items():
        assert idx.graph_components(avail).tolist() == DO.components(want, avail.tolist()), name


# ---- boxes ---------------------------------------------------------------------------------------------------
def test_box_batches_around_the_chunk_on_a_large_index():
    c = MC.many_rows()
    WB = blot(c)
    rows = check_rows(WB._idx, c)
    assert len(rows) > 1024 * 256
    check_boxes(WB._idx, rows, 1000, MC.BOX_BATCHES, WB)


def test_box_batches_around_the_chunk_at_sixteen_sequences():
    c = MC.every_n(16)
    WB = blot(c)
    check_boxes(WB._idx, MC.rows_of(c), 1000, MC.BOX_BATCHES, WB)


def test_no_boxes_and_the_most_boxes_the_abi_takes():
    c = MC.tiny_pair()
    idx = index(c)
    rows = check_rows(idx, c)
    none = idx.count_many(np.zeros((0, 2)), np.zeros((0, 2)), np.zeros((0, 2)))
    assert none.shape == (0,) and none.dtype == np.int64
    lo, hi, have = MC.max_boxes(rows)
    assert idx.count_many(lo, hi, have).tolist() == DO.box_counts(rows, lo, hi, have).tolist()
    one_more = [np.concatenate([v, v[:1]]) for v in (lo, hi, have)]
    with pytest.raises(RuntimeError) as e:
        idx.count_many(*one_more)
    assert str(e.value) == 'pw_mseeds_count_many failed: at most 64 * 65535 boxes per call'


# ---- refusals ------------------------------------------------------------------------------------------------
def _refusal(f):
    with pytest.raises(RuntimeError) as e:
        f()
    return str(e.value)


def test_refusals_of_the_c_abi():
    A = Alphabet('ACGT')
    s = np.array([0, 1, 2, 3, 0, 1, 2, 3, 1], np.uint8)
    for n in (1, 17):
        assert _refusal(lambda: _MIndex([s] * n, 3, A)) == 'pw_mseeds_create failed: n_seqs must be 2..16'
    bad = s.copy()
    bad[4] = 4
    assert _refusal(lambda: _MIndex([s, bad, s], 3, A)) == \
        'pw_mseeds_create failed: letter outside the alphabet in sequence 1'
    idx = _MIndex([s, s, s], 3, A)
    assert _refusal(idx.rows) == 'pw_mseeds_rows failed: pw_mseeds_rows before a successful pw_mseeds_build'
    assert _refusal(lambda: idx.count_many([[0] * 3], [[0] * 3], [[0] * 3])) == \
        'pw_mseeds_count_many failed: pw_mseeds_count_many before a successful pw_mseeds_build'
    assert _refusal(lambda: idx.graph_build(1., 1.)) == \
        'pw_mseeds_graph_build failed: pw_mseeds_graph_build before a successful pw_mseeds_build'
    assert idx.build() == len(DO.seed_rows([s, s, s], 3, 4))
    for call in ('counts', 'components'):
        f = idx.graph_counts if call == 'counts' else lambda: idx.graph_components(np.ones(idx.num_rows(), bool))
        assert _refusal(f) == 'pw_mseeds_graph_%s failed: pw_mseeds_graph_%s before a successful pw_mseeds_graph_build' % (call, call)
    off, adj = np.zeros(idx.num_rows() + 1, np.int64), np.zeros(1, np.int32)
    assert idx.lib.pw_mseeds_graph_fetch(idx.handle, off.ctypes.data, adj.ctypes.data) == -1
    assert idx.error() == 'pw_mseeds_graph_fetch before a successful pw_mseeds_graph_build'
    for d_coeff, radius in ((0., 1.), (-1., 1.), (float('nan'), 1.), (1., float('nan')), (1., -1.)):
        assert _refusal(lambda: idx.graph_build(d_coeff, radius)) == \
            'pw_mseeds_graph_build failed: d_coeff must be positive and radius non-negative'
    rows = DO.seed_rows([s, s, s], 3, 4)                   # and a good call after the refused ones works
    check_graph(idx, rows, 1., 2.)

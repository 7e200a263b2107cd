"""The query-batched seed index (kernels K10 of pw_qseeds.hip, seeds._QIndex) at the edges of its windows, chunks, lookup
paths, sort-key fields and radii, against the dense oracle (oracle/qseeds_dense_oracle.py).  The inputs are the named
cases of tests/qseeds_cases.py; tests/test_qseeds_cases.py proves on the CPU that each reaches what it is named for.
Unless a test says otherwise the queries lie back to back in the arena, with no gap between them.  Every comparison is
exact."""
import numpy as np
import pytest

from biseqt_amd.batch import DeviceArena, pack_reads
from biseqt_amd.seeds import _QIndex
from biseqt_amd.sequence import Alphabet
from oracle import qseeds_dense_oracle as QO
from tests import blot_many_cases as Cs, qseeds_cases as QC

pytestmark = pytest.mark.gpu

_LETTERS = '0123456789ABCDEFGHIJKLMNOPQRSTUVWXYZ'


def alphabet(c):
    return Alphabet('ACGT' if c['L'] == 4 else _LETTERS[:c['L']])


def index(c, pack=QC.pack_tight):
    qi = _QIndex(c['ref'], c['wordlen'], alphabet(c))
    qi.build(*pack(c['queries']))
    return qi


def check_rows(qi, c):
    want, off = QC.rows_of(c)
    got, got_off = qi.rows(), qi.row_offsets()
    assert qi.num_rows() == len(want) and qi.num_queries() == len(c['queries'])
    assert got.dtype == np.int32 and got.shape == want.shape and got_off.dtype == np.int64 and got_off.shape == off.shape
    assert np.array_equal(got_off, off)
    assert np.array_equal(got, want)
    return want, off


def adjacency(qi):
    off, adj = qi.graph_fetch()
    assert off[0] == 0 and len(off) == qi.num_rows() + 1 and (np.diff(off) >= 0).all() and off[-1] == len(adj)
    assert np.array_equal(np.diff(off), qi.graph_counts())
    return [sorted(adj[off[i]:off[i + 1]].tolist()) for i in range(qi.num_rows())]


def check_graph(qi, c, R=None, d_coeff=None):
    """graph_build(c, R): its return value, graph_counts and the sorted lists of graph_fetch == the dense oracle."""
    rows, off = QC.rows_of(c)
    d_coeff, R = c['c'] if d_coeff is None else d_coeff, c['R'] if R is None else R
    want = QO.neighbours(rows, off, d_coeff, R)
    assert qi.graph_build(d_coeff, R) == sum(len(x) for x in want)
    counts = qi.graph_counts()
    assert counts.dtype == np.int32 and counts.tolist() == [len(x) for x in want]
    assert adjacency(qi) == want
    return want


def check_components(qi, c, want, masks=()):
    n = qi.num_rows()
    rng = np.random.default_rng(n)
    named = [('all', np.ones(n, bool)), ('none', np.zeros(n, bool)), ('half', rng.random(n) < .5), ('most', rng.random(n) < .9)]
    for name, avail in named + list(masks):
        got = qi.graph_components(avail)
        assert got.dtype == np.int32 and got.tolist() == QO.components(want, avail.tolist()), name


def check_boxes(qi, c, batches=QC.BOX_BATCHES):
    b = QC.boxes(c, max(batches), 1)
    want = QC.box_counts(c, b)                               # once; every batch is a prefix
    for nb in batches:
        got = qi.count_boxes(*[b[f][:nb] for f in ('q', 'dmin', 'dmax', 'amin', 'amax')])
        assert got.dtype == np.int64 and got.shape == (nb,) and got.tolist() == want[:nb].tolist(), nb


def check_all(c, graph=True, masks=(), pack=QC.pack_tight):
    qi = index(c, pack)
    check_rows(qi, c)
    if qi.num_rows():
        check_boxes(qi, c)
    if graph:
        check_components(qi, c, check_graph(qi, c), masks)
    qi.close()


# ---- k_qmatch ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('p', QC.POSITION_EDGES)
def test_a_query_starts_on_a_window_edge(p):
    check_all(QC.query_edge_at_position(p))


def test_a_hundred_queries_in_one_window_and_one_query_in_three():
    check_all(QC.many_queries_in_one_workgroup())


def test_runs_of_empty_queries_on_the_window_edges():
    check_all(QC.empties_at_a_window_edge())


@pytest.mark.parametrize('n', QC.NPOS)
def test_the_positions_end_around_a_workgroup(n):
    check_all(QC.npos_around_a_workgroup(n))


@pytest.mark.parametrize('present', [True, False])
@pytest.mark.parametrize('name', sorted(QC.LOOKUPS))
def test_every_lookup_path_at_its_extreme_keys(name, present):
    check_all(QC.lookup_path(name, present))


# ---- k_qexpand -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('start', QC.CHUNK_EDGES)
def test_a_run_across_whole_expand_chunks(start):
    check_all(QC.run_across_chunks(start), graph=False)


@pytest.mark.parametrize('r', QC.CHUNK_EDGES)
def test_a_query_starts_on_a_chunk_edge(r):
    check_all(QC.query_edge_at_row(r))


@pytest.mark.parametrize('n', QC.TOTALS)
def test_the_table_ends_around_a_chunk(n):
    check_all(QC.total_rows(n))


# ---- k_qcount ------------------------------------------------------------------------------------------------
def test_rows_per_query_around_the_ballot():
    check_all(QC.rows_per_query_ladder())


def test_no_boxes_at_all():
    qi = index(QC.rows_per_query_ladder())
    none = qi.count_boxes([], [], [], [], [])
    assert none.shape == (0,) and none.dtype == np.int64
    qi.close()


# ---- k_qgraph_* ----------------------------------------------------------------------------------------------
def test_seeds_on_the_extreme_diagonals():
    check_all(QC.corners())


@pytest.mark.parametrize('nq', QC.FIELD_NQ)
@pytest.mark.parametrize('s', QC.FIELD_SUMS)
def test_the_sort_key_at_every_field_width(s, nq):
    check_all(QC.field_widths(s, nq))


def test_twin_queries_share_no_edge():
    c = QC.twins()
    qi = index(c)
    rows, off = check_rows(qi, c)
    want = check_graph(qi, c)
    adj = adjacency(qi)
    n = int(off[2] - off[1])
    assert [[v + n for v in x] for x in adj[off[1]:off[2]]] == adj[off[2]:off[3]]
    check_components(qi, c, want)
    check_boxes(qi, c)
    qi.close()


def test_one_pair_on_the_d_radius_and_one_past_it():
    for delta, total in ((QC.NEAR_D, 2), (QC.NEAR_D + 1, 0)):
        c = QC.near_miss_d(delta)
        qi = index(c)
        check_rows(qi, c)
        assert sum(len(x) for x in check_graph(qi, c)) == total
        qi.close()


def test_one_pair_on_the_a_radius_and_one_past_it():
    c = QC.near_miss_a()
    qi = index(c)
    check_rows(qi, c)
    assert sum(len(x) for x in check_graph(qi, c, c['R_past'])) == 0
    want = check_graph(qi, c)
    assert sum(len(x) for x in want) == 2
    check_components(qi, c, want)
    qi.close()


def test_a_radius_that_is_no_integer():
    check_all(QC.non_integer_radius())


@pytest.mark.parametrize('which', range(len(QC.ROUNDINGS)))
def test_the_neighbour_test_rounds_as_the_kd_tree_does(which):
    check_all(QC.rounding(which))


def test_radius_zero():
    c = QC.radius_zero()
    qi = index(c)
    check_rows(qi, c)
    want = check_graph(qi, c)
    assert qi.graph_build(c['c'], c['R']) == 0 and not qi.graph_counts().any()
    check_components(qi, c, want)
    qi.close()


def test_a_window_wider_than_the_table():
    check_all(QC.window_clamped())


def test_components_along_two_scrambled_chains():
    c = QC.chain()
    check_all(c, masks=list(QC.chain_masks(2 * QC.CHAIN_M).items()))


# ---- the state of the handle ---------------------------------------------------------------------------------
def _refusal(f):
    with pytest.raises(RuntimeError) as e:
        f()
    return str(e.value)


def _graph_is_refused(qi):
    for call, f in (('counts', qi.graph_counts), ('fetch', qi.graph_fetch),
                    ('components', lambda: qi.graph_components(np.ones(qi.num_rows(), bool)))):
        assert _refusal(f) == 'pw_qseeds_graph_%s failed: pw_qseeds_graph_%s before a successful pw_qseeds_graph_build' % (call, call)


def test_one_handle_three_builds():
    """Fewer queries, then more again: the buffers are reused, and the graph of the build before is gone."""
    ladder, two = QC.rows_per_query_ladder(), QC.total_rows(1)
    assert np.array_equal(ladder['ref'], two['ref']) and len(two['queries']) == 2
    qi = _QIndex(ladder['ref'], ladder['wordlen'], alphabet(ladder))
    for c in (ladder, two, ladder):
        qi.build(*QC.pack_tight(c['queries']))
        _graph_is_refused(qi)
        check_rows(qi, c)
        check_components(qi, c, check_graph(qi, c))
        check_boxes(qi, c)
    qi.close()


def _arena_case(name, ref, arena, offs, lens, k=QC.MATCH_K):
    return QC.case(name, ref, [arena[o:o + n] for o, n in zip(offs, lens)], k, 4, c=4., R=12.)


def test_a_build_refused_for_a_letter_leaves_no_table_and_the_next_is_exact():
    c = QC.query_edge_at_position(256)
    k = c['wordlen']
    qi = _QIndex(c['ref'], k, alphabet(c))
    short = np.array([1, 2, 3], np.uint8)                  # shorter than a word: only the tail's own check reads its letters
    for extra, q, at in (([], 1, -(k - 2)), ([short], 4, 1), ([], 0, 0), ([], 3, -1)):     # tails (j > len - k); first; last letter
        queries = [t.copy() for t in c['queries'] + extra]
        assert (q, at) == (0, 0) or at % len(queries[q]) > len(queries[q]) - k
        queries[q][at] = 4
        assert _refusal(lambda: qi.build(*QC.pack_tight(queries))) == 'pw_qseeds_build failed: letter outside the alphabet in a query'
        assert qi.num_rows() == -1 and qi.num_queries() == -1
        assert _refusal(qi.rows) == 'pw_qseeds_rows failed: pw_qseeds_rows before a successful pw_qseeds_build'
        qi.build(*QC.pack_tight(c['queries']))
        check_rows(qi, c)
        check_graph(qi, c)
    qi.close()


def test_letters_of_no_query_are_not_read():
    """Bytes outside the alphabet between and behind the queries (the padded layout of pack_reads) are not refused."""
    c = QC.query_edge_at_position(256)
    arena, offs, lens = pack_reads(c['queries'])
    used = np.zeros(len(arena), bool)
    for o, n in zip(offs, lens):
        used[o:o + n] = True
    assert (~used).sum() >= 16 * len(offs)
    arena[~used] = 255
    qi = _QIndex(c['ref'], c['wordlen'], alphabet(c))
    qi.build(arena, offs, lens)
    check_rows(qi, c)
    check_boxes(qi, c)
    qi.close()


def test_offsets_in_any_order_and_queries_that_share_letters():
    rng = np.random.default_rng(77)
    ref = rng.integers(0, 4, 400).astype(np.uint8)
    arena = np.r_[rng.integers(0, 4, 30), ref[50:250], rng.integers(0, 4, 30), np.zeros(16, int)].astype(np.uint8)
    offs = np.array([200, 120, 120, 60, 0, 10], np.int64)          # descending; two queries on one offset; overlapping slices
    lens = np.array([60, 100, 40, 100, 90, 5], np.int32)
    c = _arena_case('shared_letters', ref, arena, offs, lens)
    qi = _QIndex(ref, c['wordlen'], alphabet(c))
    qi.build(arena, offs, lens)
    rows, off = check_rows(qi, c)
    assert (np.diff(off)[:5] > 20).all()
    check_components(qi, c, check_graph(qi, c))
    check_boxes(qi, c)
    qi.close()


@pytest.mark.parametrize('queries', [[], [[0, 1, 2], [], [3, 3, 3, 3, 3]]], ids=['no_queries', 'all_shorter_than_a_word'])
def test_no_rows_at_all(queries):
    rng = np.random.default_rng(78)
    c = QC.case('no_rows_%d' % len(queries), rng.integers(0, 4, 100), queries, QC.MATCH_K, 4)
    qi = index(c)
    check_rows(qi, c)
    assert qi.num_rows() == 0 and qi.rows().shape == (0, 3) and qi.row_offsets().tolist() == [0] * (len(queries) + 1)
    assert qi.graph_build(2., 10.) == 0 and qi.graph_counts().tolist() == []
    off, adj = qi.graph_fetch()
    assert off.tolist() == [0] and len(adj) == 0
    assert qi.graph_components(np.zeros(0, bool)).tolist() == []
    nq = len(queries)
    assert qi.count_boxes(np.arange(nq), [QC.I32_MIN] * nq, [QC.I32_MAX] * nq, [QC.I32_MIN] * nq, [QC.I32_MAX] * nq).tolist() == [0] * nq
    qi.close()


def test_a_device_arena_is_read_in_place():
    c = QC.query_edge_at_position(256)
    arena, offs, lens = pack_reads(c['queries'])
    qi = _QIndex(c['ref'], c['wordlen'], alphabet(c))
    qi.build(arena, offs, lens)
    host_rows, host_off = qi.rows(), qi.row_offsets()
    with DeviceArena(arena) as dev:
        qi.build(dev, offs, lens)
        assert np.array_equal(qi.rows(), host_rows) and np.array_equal(qi.row_offsets(), host_off)
        check_rows(qi, c)
    qi.close()


# ---- refusals ------------------------------------------------------------------------------------------------
def test_refusals_of_the_c_abi():
    c = QC.rows_per_query_ladder()
    ref, k, A = c['ref'], c['wordlen'], alphabet(c)
    for L in (0, 37):
        assert _refusal(lambda: _QIndex(ref, k, 'x' * L)) == 'pw_qseeds_create failed: alphabet_len must be 1..36 (kmers.py:266)'
    for w in (0, 32):
        assert _refusal(lambda: _QIndex(ref, w, A)) == 'pw_qseeds_create failed: wordlen must be 1..31 (kmers.py:269)'
    assert _refusal(lambda: _QIndex(ref, 31, A)) == 'pw_qseeds_create failed: alphabet_len ^ wordlen must be below 2^62'
    _QIndex(ref, 30, A).close()                            # 4^30 = 2^60 is accepted
    bad = ref.copy()
    bad[7] = 4
    assert _refusal(lambda: _QIndex(bad, k, A)) == 'pw_qseeds_create failed: letter outside the alphabet in the reference'
    # every call before a build
    qi = _QIndex(ref, k, A)
    lib, h = qi.lib, qi.handle
    assert qi.num_rows() == -1 and qi.num_queries() == -1 and lib.pw_qseeds_rows_device(h) is None
    for call, f in (('rows', qi.rows), ('row_offsets', qi.row_offsets), ('count_boxes', lambda: qi.count_boxes([0], [0], [0], [0], [0])),
                    ('graph_build', lambda: qi.graph_build(1., 1.))):
        assert _refusal(f) == 'pw_qseeds_%s failed: pw_qseeds_%s before a successful pw_qseeds_build' % (call, call)
    buf = np.zeros(64, np.int64)
    for call, f in (('counts', lambda: lib.pw_qseeds_graph_counts(h, buf.ctypes.data, 16)),
                    ('fetch', lambda: lib.pw_qseeds_graph_fetch(h, buf.ctypes.data, buf.ctypes.data)),
                    ('components', lambda: lib.pw_qseeds_graph_components(h, buf.ctypes.data, buf.ctypes.data))):
        assert f() == -1 and qi.error() == 'pw_qseeds_graph_%s before a successful pw_qseeds_graph_build' % call
    # a query outside the arena
    arena, offs, lens = QC.pack_tight(c['queries'])
    for q, off_q, len_q in ((1, len(arena) - int(lens[1]) + 1, None), (2, -1, None), (3, None, -1), (0, len(arena) + 1, None)):
        o, n = offs.copy(), lens.copy()
        if off_q is not None:
            o[q] = off_q
        if len_q is not None:
            n[q] = len_q
        assert _refusal(lambda: qi.build(arena, o, n)) == 'pw_qseeds_build failed: query %d lies outside the arena' % q
        assert qi.num_rows() == -1
    total = len(QC.rows_of(c)[0])
    assert _refusal(lambda: qi.build(arena, offs, lens, max_rows=total - 1)) == \
        'pw_qseeds_build failed: the seeds table would hold %d rows (limit %d): raise max_rows or the word length' % (total, total - 1)
    assert qi.build(arena, offs, lens, max_rows=total) == total
    _graph_is_refused(qi)
    # capacities
    small = np.zeros((total, 3), np.int32)
    assert lib.pw_qseeds_rows(h, small.ctypes.data, total - 1) == -1 and qi.error() == 'pw_qseeds_rows: capacity too small'
    # boxes that name no query
    nq = len(c['queries'])
    for q in (-1, nq):
        assert _refusal(lambda: qi.count_boxes([0, q], [0, 0], [0, 0], [0, 0], [0, 0])) == \
            'pw_qseeds_count_boxes failed: box 1 names a query that does not exist'
    # the graph's parameters: d_coeff positive, radius non-negative (0 is a radius: test_radius_zero)
    for d_coeff, radius in ((0., 1.), (-1., 1.), (float('nan'), 1.), (1., float('nan')), (1., -1.)):
        assert _refusal(lambda: qi.graph_build(d_coeff, radius)) == \
            'pw_qseeds_graph_build failed: d_coeff must be positive and radius non-negative'
        _graph_is_refused(qi)
    qi.graph_build(1., 5.)
    assert lib.pw_qseeds_graph_counts(h, small.ctypes.data, total - 1) == -1 and qi.error() == 'pw_qseeds_graph_counts: capacity too small'
    # and a good call after the refused ones works
    check_rows(qi, c)
    check_components(qi, c, check_graph(qi, c))
    check_boxes(qi, c)
    qi.close()


# ---- through the class ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('make,K_min,p_min', [(lambda: QC.query_edge_at_position(256), 40, .7), (QC.rows_per_query_ladder, 10, .5),
                                              (QC.twins, 40, .7)], ids=['query_edge_at_position_256', 'rows_per_query_ladder', 'twins'])
def test_similar_segments_many_and_the_arrays_it_consumed(make, K_min, p_min):
    """Segments, p and scores == the loop over the per-query path, and the neighbour counts and component labels the host
    half was fed == blot_many_cases.cpu_arrays (the KD-tree per query, a union-find): arrays equal, not only segments."""
    from biseqt_amd.blot import WordBlotLocalRef, available_seeds_many, seed_ps_from_counts
    c = make()
    ref, queries, k = c['ref'], c['queries'], c['wordlen']
    loc = WordBlotLocalRef(Cs.mk(ref), wordlen=k, g_max=Cs.G_MAX, sensitivity=Cs.SENS, alphabet=Cs.A)
    seqs = [Cs.mk(t) for t in queries]
    got = loc.similar_segments_many(seqs, K_min, p_min)
    qi = loc._qidx
    check_rows(qi, c)
    cpu = Cs.cpu_arrays(ref, queries, k, K_min, p_min)
    assert np.array_equal(cpu['rows'], qi.rows()) and np.array_equal(cpu['row_offsets'], qi.row_offsets())
    counts = qi.graph_counts()
    assert np.array_equal(counts, cpu['counts'])
    avail = available_seeds_many(seed_ps_from_counts(counts, cpu['d_radius'], cpu['a_radius'], 4, k), p_min, qi.row_offsets())
    assert np.array_equal(avail, cpu['labels'] >= 0)
    assert np.array_equal(qi.graph_components(avail), cpu['labels'])
    for q, T in enumerate(seqs):
        Cs.assert_identical(got[q], list(loc.similar_segments(T, K_min, p_min)), q)
    assert sum(len(g) for g in got) >= 1
    loc.close()

"""pw_qseeds_build_stranded (k_qmatch_stranded of pw_qseeds.hip, seeds._QIndex.build(strands=...)) against the dense oracle
(oracle/qseeds_dense_oracle.py) on queries whose minus entries were reverse-complemented on the host: rows and row offsets
equal exactly.  The inputs are the named cases of tests/qseeds_strand_cases.py; tests/test_qseeds_strand_cases.py proves
on the CPU that each reaches what it is named for.  Unless a test says otherwise the base letters lie back to back in the
arena, with no gap between them."""
import numpy as np
import pytest

from biseqt_amd.batch import DeviceArena, pack_reads
from biseqt_amd.seeds import _QIndex
from tests import qseeds_cases as QC, qseeds_strand_cases as SC
from tests.test_gpu_qseeds_edges import alphabet, check_boxes, check_components, check_graph, check_rows

pytestmark = pytest.mark.gpu


def index(sc, pack=QC.pack_tight):
    qi = _QIndex(sc['ref'], sc['wordlen'], alphabet(sc))
    qi.build(*SC.listing(sc, pack), strands=sc['strands'], complement=sc['comp'])
    return qi


def check(sc, pack=QC.pack_tight):
    qi = index(sc, pack)
    check_rows(qi, sc)
    qi.close()


def test_lengths_around_k():
    check(SC.lengths_around_k())


@pytest.mark.parametrize('assign', SC.ASSIGNMENTS, ids=lambda a: '%d%d%d' % a)
def test_boundary_traps(assign):
    check(SC.boundary_traps(assign))


@pytest.mark.parametrize('pattern', SC.PATTERNS)
@pytest.mark.parametrize('p', QC.POSITION_EDGES)
def test_a_query_starts_on_a_window_edge(p, pattern):
    check(SC.with_strands(QC.query_edge_at_position(p), pattern))


@pytest.mark.parametrize('pattern', SC.PATTERNS)
def test_a_hundred_queries_in_one_window_and_one_query_in_three(pattern):
    check(SC.with_strands(QC.many_queries_in_one_workgroup(), pattern))


@pytest.mark.parametrize('pattern', SC.PATTERNS)
def test_runs_of_empty_queries_on_the_window_edges(pattern):
    check(SC.with_strands(QC.empties_at_a_window_edge(), pattern))


@pytest.mark.parametrize('pattern', SC.PATTERNS)
@pytest.mark.parametrize('n', QC.NPOS)
def test_the_positions_end_around_a_workgroup(n, pattern):
    check(SC.with_strands(QC.npos_around_a_workgroup(n), pattern))


@pytest.mark.parametrize('pattern', ['minus', 'alternating'])
@pytest.mark.parametrize('name', SC.STRAND_LOOKUPS)
def test_every_join_path(name, pattern):
    L, k, nref = QC.LOOKUPS[name]
    assert QC.lookup_of(L, k, nref) == {'table': 'table', 'big32': 'search32', 'first64': 'search64', 'letters36': 'search64'}[name]
    check(SC.lookup_case(name, pattern))


@pytest.mark.parametrize('L', sorted(SC.ALPHABETS))
def test_alphabets(L):
    check(SC.alphabet_case(L))


def test_palindromes_have_the_rows_of_the_plus_strand():
    sc = SC.palindromes()
    qi = index(sc)
    rows, off = check_rows(qi, sc)
    got = qi.rows()
    for q in range(4):
        plus, minus = got[off[2 * q]:off[2 * q + 1]], got[off[2 * q + 1]:off[2 * q + 2]]
        assert len(plus) and np.array_equal(plus[:, 1:], minus[:, 1:]) and (minus[:, 0] == 2 * q + 1).all()
    qi.close()


# ---- the frame -----------------------------------------------------------------------------------------------
def test_a_minus_query_at_every_offset_mod_4():
    sc = SC.with_strands(QC.query_edge_at_position(256), 'minus')
    want = None
    qi = _QIndex(sc['ref'], sc['wordlen'], alphabet(sc))
    for shift in range(4):
        arena, offs, lens = SC.listing(sc)
        arena = np.r_[np.full(shift, 255, np.uint8), arena]                     # (letters of no query are not read)
        qi.build(arena, offs + shift, lens, strands=sc['strands'], complement=sc['comp'])
        check_rows(qi, sc)
        want = qi.rows() if want is None else want
        assert np.array_equal(qi.rows(), want)
    qi.close()


def test_a_device_arena_is_read_in_place_on_both_strands():
    sc = SC.with_strands(QC.query_edge_at_position(256), 'twice')
    arena, offs, lens = SC.listing(sc, pack_reads)
    qi = _QIndex(sc['ref'], sc['wordlen'], alphabet(sc))
    qi.build(arena, offs, lens, strands=sc['strands'], complement=sc['comp'])
    host_rows, host_off = qi.rows(), qi.row_offsets()
    with DeviceArena(arena) as dev:
        qi.build(dev, offs, lens, strands=sc['strands'], complement=sc['comp'])
        assert np.array_equal(qi.rows(), host_rows) and np.array_equal(qi.row_offsets(), host_off)
        check_rows(qi, sc)
        assert np.array_equal(dev.read(), arena)                                # ... and is left as it was
    qi.close()


# ---- the C entry point ---------------------------------------------------------------------------------------
def _call(qi, arena, offs, lens, strand, comp, max_rows=0):
    arena, offs, lens = np.ascontiguousarray(arena, np.uint8), np.ascontiguousarray(offs, np.int64), np.ascontiguousarray(lens, np.int32)
    strand = None if strand is None else np.ascontiguousarray(strand, np.uint8)
    comp = None if comp is None else np.ascontiguousarray(comp, np.uint8)
    qi._edges = None
    return qi.lib.pw_qseeds_build_stranded(qi.handle, arena.ctypes.data, arena.nbytes, 0, offs.ctypes.data, lens.ctypes.data,
                                           None if strand is None else strand.ctypes.data, None if comp is None else comp.ctypes.data,
                                           len(offs), max_rows, None)


def test_no_strands_and_all_plus_are_the_old_entry_point():
    c = QC.query_edge_at_position(256)
    arena, offs, lens = QC.pack_tight(c['queries'])
    qi = _QIndex(c['ref'], c['wordlen'], alphabet(c))
    qi.build(arena, offs, lens)
    rows, off = qi.rows(), qi.row_offsets()
    check_rows(qi, c)
    for strand, comp in ((None, None), (np.zeros(len(offs), np.uint8), None), (None, [9, 9, 9, 9]), (np.zeros(len(offs), np.uint8), SC.COMP4)):
        assert _call(qi, arena, offs, lens, strand, comp) == 0, qi.error()
        assert np.array_equal(qi.rows(), rows) and np.array_equal(qi.row_offsets(), off)
    qi.build(arena, offs, lens, strands=['+'] * len(offs))                     # (no complement needed without a minus entry)
    assert np.array_equal(qi.rows(), rows)
    qi.close()


def test_refused_arguments_and_the_next_build():
    """Refused arguments, not faults: -1 with a message, no table left, and the next valid build on the handle is exact."""
    sc = SC.lengths_around_k()
    k = sc['wordlen']
    arena, offs, lens = SC.listing(sc)
    n = len(offs)
    qi = _QIndex(sc['ref'], k, alphabet(sc))

    def refused(strand, comp, message, arena=arena, offs=offs, lens=lens):
        assert _call(qi, arena, offs, lens, strand, comp) == -1
        assert qi.error() == message, qi.error()
        assert qi.num_rows() == -1 and qi.num_queries() == -1
        qi.build(*SC.listing(sc), strands=sc['strands'], complement=sc['comp'])      # the handle stays usable
        check_rows(qi, sc)
    bad_comp = 'complement must be alphabet_len bytes with complement[complement[c]] == c for every letter'
    refused([0, 1] * (n // 2 - 1) + [2, 1], SC.COMP4, 'strand %d must be 0 (as given) or 1 (reverse complement)' % (n - 2))
    refused([255] + [0] * (n - 1), SC.COMP4, 'strand 0 must be 0 (as given) or 1 (reverse complement)')
    refused(sc['strands'], [1, 2, 3, 0], bad_comp)
    refused(sc['strands'], [3, 2, 1, 4], bad_comp)
    refused(sc['strands'], None, bad_comp)
    # a letter outside the alphabet at each position in turn of a minus query of k + 2 letters, its neighbours directly
    # before and behind it: positions 0 .. 2 of rc(query) meet it in a k-mer, the tail positions in their own check
    before, letters, behind = sc['base'][12], sc['base'][10], sc['base'][13]
    assert k == 3 and len(letters) == k + 2
    for at in range(k + 2):
        t = letters.copy()
        t[at] = 4
        a1, o1, l1 = QC.pack_tight([before, t, behind])
        refused([0, 1, 0], SC.COMP4, 'letter outside the alphabet in a query', a1, o1, l1)
    with pytest.raises(RuntimeError, match='pw_qseeds_build_stranded failed: letter outside the alphabet in a query'):
        qi.build(a1, o1, l1, strands=[0, 1, 0], complement=SC.COMP4)
    qi.build(*SC.listing(sc), strands=sc['strands'], complement=sc['comp'])
    check_rows(qi, sc)
    qi.close()


# ---- everything behind K10a works on listed entries ----------------------------------------------------------
def test_graph_components_and_boxes_of_a_stranded_build():
    sc = SC.with_strands(QC.chain(), 'alternating')
    assert sc['strands'].tolist() == [0, 1]
    qi = index(sc)
    check_rows(qi, sc)
    want = check_graph(qi, sc)
    check_components(qi, sc, want, masks=list(QC.chain_masks(2 * QC.CHAIN_M).items()))
    check_boxes(qi, sc)
    qi.close()
    for delta in (QC.NEAR_D, QC.NEAR_D + 1):
        c = QC.near_miss_d(delta)
        sc = SC.with_strands(c, 'minus', tuple(range(c['L'] - 1, -1, -1)))
        qi = index(sc)
        check_rows(qi, sc)
        assert sum(len(x) for x in check_graph(qi, sc)) == (2 if delta == QC.NEAR_D else 0)
        qi.close()

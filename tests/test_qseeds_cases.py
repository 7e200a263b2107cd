"""Every named case of tests/qseeds_cases.py lands on the edge it is named for -- proved from the dense oracle
(oracle/qseeds_dense_oracle.py) and arithmetic alone, so that tests/test_gpu_qseeds_edges.py, which runs the same inputs
on the device, is known to reach the code it is meant to reach.  If a seed does not land, the seed changes, not the
assertion.  No GPU."""
from fractions import Fraction

import numpy as np
import pytest

from oracle import mseeds_dense_oracle as DO, qseeds_dense_oracle as QO
from tests import mseeds_cases as MC, qseeds_cases as QC


def _neighs(c, R=None):
    rows, off = QC.rows_of(c)
    return QO.neighbours(rows, off, c['c'], c['R'] if R is None else R)


def _has(ref_hits, word, L):
    v = 0
    for x in word:
        v = v * L + int(x)
    return v in ref_hits


def test_the_constants_are_the_kernels():
    """The copies in qseeds_cases.py against the source they name."""
    import os
    csrc = os.path.join(os.path.dirname(__file__), '..', 'biseqt_amd', 'csrc')
    src = open(os.path.join(csrc, 'pw_qseeds.hip')).read()
    host = open(os.path.join(csrc, 'pw_seed_host.h')).read()          # the table decision: shared by the seed indexes
    assert 'blockIdx.x * 256' in src and QC.MATCH_WG == 256
    assert 'constexpr int kExpRows = %d;' % QC.EXP_ROWS in src
    assert 'blockIdx.x * %d + (threadIdx.x >> 6)' % QC.BOX_WG in src and 'base += %d' % QC.BALLOT in src
    assert 'ws.kinv <= (1ull << 26) && ws.kinv / (uint64_t)n_other <= %d' % QC.TAB_SPARSITY in host and QC.TAB_MAX == 1 << 26
    assert 'if (table_pays(x->ws, x->nkR))' in src


# ---- k_qmatch ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('p', QC.POSITION_EDGES)
def test_a_query_starts_on_the_position_named(p):
    c = QC.query_edge_at_position(p)
    rows, off = QC.rows_of(c)
    q, k = c['edge_query'], c['wordlen']
    assert QC.pstart(c)[q] == p and off[q + 1] > off[q]
    assert rows[off[q], 2] - rows[off[q], 1] == 0              # the query's first position (j = 0) has a row
    # the query before it ends with a word of the reference, and every k-mer across the boundary is one too
    hits = DO.positions(c['ref'], k, 4)
    across = np.r_[c['queries'][q - 1][-k:], c['queries'][q][:k]]
    assert all(_has(hits, across[t:t + k], 4) for t in range(k + 1))
    last = rows[off[q] - 1]
    assert last[0] == q - 1 and (last[2] - last[1]) // 2 == len(c['queries'][q - 1]) - k
    # packed back to back, the arena holds that stretch
    arena, offs, lens = QC.pack_tight(c['queries'])
    assert (arena[offs[q] - k:offs[q] + k] == across).all() and offs[q] == p


def test_a_window_of_positions_holds_a_hundred_queries_and_a_query_spans_three():
    c = QC.many_queries_in_one_workgroup()
    lens, ps = QC.lengths(c), QC.pstart(c)
    assert len(lens) == 121 and c['wordlen'] == 2 and set(lens[:120].tolist()) == {0, 1, 2, 3}
    assert ((lens[:119] == 0) & (lens[1:120] > 0)).sum() >= 30                       # empties interleaved
    assert (ps[:120] < QC.MATCH_WG).sum() >= 100
    assert len(set(range(ps[120] // QC.MATCH_WG, (ps[121] - 1) // QC.MATCH_WG + 1))) >= 3
    rows, off = QC.rows_of(c)
    assert 0 < off[120] and 1000 < off[121] - off[120] < 3000
    assert (np.diff(off)[:120][lens[:120] < 2] == 0).all()


def test_runs_of_empty_queries_start_on_the_window_edges():
    c = QC.empties_at_a_window_edge()
    lens, ps = QC.lengths(c), QC.pstart(c)
    runs, q = [], 0
    while q < len(lens):
        if lens[q] == 0:
            e = q
            while e < len(lens) and lens[e] == 0:
                e += 1
            runs.append((int(ps[q]), e - q, e))
            q = e
        else:
            q += 1
    assert all(n >= 3 for _, n, _ in runs)
    assert [p for p, _, _ in runs] == [0, QC.MATCH_WG, int(ps[-1])] and runs[-1][2] == len(lens)
    rows, off = QC.rows_of(c)
    assert (np.diff(off)[lens > 0] > 50).all()


@pytest.mark.parametrize('n', QC.NPOS)
def test_the_positions_sum_to_the_number_named(n):
    c = QC.npos_around_a_workgroup(n)
    lens, k = QC.lengths(c), c['wordlen']
    rows, off = QC.rows_of(c)
    assert lens.sum() == n and lens[-1] > 0
    if n == 1:
        assert len(rows) == 0 and lens[-1] < k
        return
    # the last query's tail -- its last k - 1 positions, which hold letters and no k-mer -- ends on position n - 1
    assert lens[-1] >= k and off[-1] > off[-2]
    tail = range(n - (k - 1), n)
    assert tail[-1] == n - 1 and (n != 257 or tail[0] < QC.MATCH_WG <= tail[-1])
    assert (rows[off[-2]:, 2] - rows[off[-2]:, 1]).max() // 2 == lens[-1] - k   # its last whole word has a row


@pytest.mark.parametrize('present', [True, False])
@pytest.mark.parametrize('name', sorted(QC.LOOKUPS))
def test_the_lookup_is_the_one_named(name, present):
    c = QC.lookup_path(name, present)
    L, k, nref = QC.LOOKUPS[name]
    assert (c['L'], c['wordlen'], len(c['ref'])) == (L, k, nref)
    assert QC.lookup_of(L, k, nref) == QC.LOOKUP_PATH[name]
    kinv, nk = L ** k, nref - k + 1
    assert kinv < 2 ** 62
    if name == 'table_edge':
        assert kinv // nk == QC.TAB_SPARSITY
    if name == 'sparse32':
        assert kinv // nk == QC.TAB_SPARSITY + 1 and kinv <= QC.TAB_MAX
    if name == 'big32':
        assert QC.TAB_MAX < kinv < 2 ** 32 - 1
    if name == 'odd32':
        assert kinv < 2 ** 32 - 1 and QC.bits_for(kinv - 1) == 32 and kinv & (kinv - 1)
    if name == 'first64':
        assert kinv == 2 ** 32
    if name in ('wide64', 'letters36'):
        assert kinv > 2 ** 56
    hits = DO.positions(c['ref'], k, L)
    assert (len(hits.get(0, ())), len(hits.get(kinv - 1, ()))) == ((1, 1) if present else (0, 0))
    rows, off = QC.rows_of(c)
    qkeys = set()
    for t in c['queries']:
        qkeys |= set(DO.positions(t, k, L))
    assert 0 in qkeys and kinv - 1 in qkeys
    if not present:
        assert 0 < min(hits) and max(hits) < kinv - 1         # a k-mer below every key of the reference and one above
        assert off[4] - off[3] == 0 and off[5] - off[4] == 0
    else:
        assert off[4] - off[3] == 1 and off[5] - off[4] == 2
    assert off[1] - off[0] >= 21                               # the slice of the reference


# ---- k_qexpand -----------------------------------------------------------------------------------------------
def test_the_planted_words_give_the_rows_named():
    for n in (0, 1, 99, 100, 101, 250):
        r, off = QO.rows(QC.planted_ref(10), [QC.words(n)], QC.PLANT_K, 4)
        assert len(r) == n and off.tolist() == [0, n]


@pytest.mark.parametrize('start', QC.CHUNK_EDGES)
def test_a_run_starts_on_the_row_named_and_fills_a_whole_chunk(start):
    c = QC.run_across_chunks(start)
    rows, off = QC.rows_of(c)
    hits = DO.positions(c['ref'], c['wordlen'], 4)
    assert len(hits[0]) == QC.RUN > 2 * QC.EXP_ROWS
    j = (rows[:, 2] - rows[:, 1]) // 2
    run = np.flatnonzero((rows[:, 0] == 1) & (j == j[start]))
    assert run[0] == start and len(run) == QC.RUN and (np.diff(run) == 1).all()
    first_whole = -(-start // QC.EXP_ROWS) * QC.EXP_ROWS
    assert first_whole + QC.EXP_ROWS <= start + QC.RUN
    # the positions directly before and behind it have no hit
    js = set(j[off[1]:off[2]].tolist())
    assert int(j[start]) - 1 not in js and int(j[start]) + 1 not in js
    assert off[1] < start < off[2] and len(rows) == start + QC.RUN + 7 + 130 < 30000 and off[3] - off[2] == 130


@pytest.mark.parametrize('r', QC.CHUNK_EDGES)
def test_a_query_starts_on_the_row_named(r):
    c = QC.query_edge_at_row(r)
    rows, off = QC.rows_of(c)
    q = c['edge_query']
    assert off[q] == r and off[q] > off[q - 1] and off[q + 1] > off[q] and max(np.diff(off)) < 3000


@pytest.mark.parametrize('n', QC.TOTALS)
def test_the_table_has_the_rows_named(n):
    c = QC.total_rows(n)
    rows, off = QC.rows_of(c)
    assert len(rows) == n == off[-1] and off[-1] - off[-2] == 1      # the last row is a position's only one
    assert max(np.diff(off)) < 3000


# ---- k_qcount ------------------------------------------------------------------------------------------------
def test_the_ladder_has_the_rows_per_query_named():
    rows, off = QC.rows_of(QC.rows_per_query_ladder())
    assert np.diff(off).tolist() == [0, 1, 63, 64, 65, 128, 129] == list(QC.LADDER)
    assert {n % QC.BALLOT for n in QC.LADDER} >= {0, 1, 63}


@pytest.mark.parametrize('make', [QC.rows_per_query_ladder, QC.twins, lambda: QC.query_edge_at_row(2048)])
def test_the_named_boxes_are_what_they_are_named(make):
    c = make()
    rows, off = QC.rows_of(c)
    assert QC.BOX_BATCHES == (0, 1, 3, 4, 5, 257) and {b % QC.BOX_WG for b in QC.BOX_BATCHES} == {0, 1, 3}
    b = QC.boxes(c, 257, 1)
    want = QC.box_counts(c, b)
    kinds = np.array(b['kind'])
    assert len(want) == 257 and all(v.dtype == np.int32 and len(v) == 257 for f, v in b.items() if f != 'kind')
    for n in QC.BOX_BATCHES:                                    # a smaller batch is a prefix
        s = QC.boxes(c, n, 1)
        assert all(np.array_equal(s[f], b[f][:n]) for f in ('q', 'dmin', 'dmax', 'amin', 'amax')) and s['kind'] == b['kind'][:n]
    # a row on each inclusive edge: the box one step further in holds exactly the rows that do not lie on that edge
    big = int(b['q'][0])
    r = rows[off[big]:off[big + 1]]
    for i, (edge, col, f) in enumerate((('dmin', 1, 'dmin'), ('dmax', 1, 'dmax'), ('amin', 2, 'amin'), ('amax', 2, 'amax'))):
        assert b['kind'][2 * i] == edge + '_edge' and b['kind'][2 * i + 1] == edge + '_out'
        inside = (r[:, 1] >= b['dmin'][2 * i]) & (r[:, 1] <= b['dmax'][2 * i]) & (r[:, 2] >= b['amin'][2 * i]) & (r[:, 2] <= b['amax'][2 * i])
        on_edge = int((inside & (r[:, col] == b[f][2 * i])).sum())
        assert on_edge >= 1 and want[2 * i] - want[2 * i + 1] == on_edge
        assert abs(int(b[f][2 * i + 1]) - int(b[f][2 * i])) == 1
    # every kind has a box with rows -- but for the kinds that cannot -- and some box has none
    for kind in sorted(set(b['kind'])):
        if kind in QC.BOX_ALWAYS_ZERO:
            assert (want[kinds == kind] == 0).all(), kind
        elif not kind.endswith('_out'):
            assert (want[kinds == kind] > 0).any(), kind
    assert set(b['kind']) >= {'inverted_d', 'inverted_a', 'plane', 'several', 'random'}
    assert (kinds == 'empty_query').any() == bool((np.diff(off) == 0).any())
    assert (b['dmin'][kinds == 'inverted_d'] > b['dmax'][kinds == 'inverted_d']).all()
    assert (b['amin'][kinds == 'inverted_a'] > b['amax'][kinds == 'inverted_a']).all()
    plane = kinds == 'plane'
    assert (want[plane] == np.diff(off)[b['q'][plane]]).all() and b['dmin'][plane].min() == QC.I32_MIN
    assert (kinds == 'several').sum() == 5 and len(set(b['q'][kinds == 'several'].tolist())) == 1
    rq = b['q'][kinds == 'random']
    assert (np.diff(rq) < 0).any() and (np.diff(rq) > 0).any()                     # query order scrambled
    assert (want == 0).any() and len(set(want.tolist())) > 10


# ---- k_qgraph_* ----------------------------------------------------------------------------------------------
def test_the_corners_hold_the_extreme_diagonals():
    c = QC.corners()
    rows, off = QC.rows_of(c)
    k, nR, lens = c['wordlen'], len(c['ref']), QC.lengths(c)
    n = int(lens.max())
    assert n > nR and lens[1] == lens[2] == n and lens[0] == 0
    neighs = _neighs(c)
    ij = [((int(d) + int(a)) // 2, (int(a) - int(d)) // 2) for _, d, a in rows]
    lowest = [o for o, (i, j) in enumerate(ij) if (i, j) == (0, n - k) and rows[o, 0] == 1]
    highest = [o for o, (i, j) in enumerate(ij) if (i, j) == (nR - k, 0)]
    largest_a = [o for o, (i, j) in enumerate(ij) if (i, j) == (nR - k, n - k)]
    assert len(lowest) == 1 and len(highest) == 1 and len(largest_a) == 1
    assert rows[lowest[0], 1] == rows[:, 1].min() == -(n - k) and rows[highest[0], 1] == rows[:, 1].max() == nR - k
    assert rows[largest_a[0], 2] == rows[:, 2].max() == nR + n - 2 * k
    assert all(len(neighs[o[0]]) >= 1 for o in (lowest, highest, largest_a))
    assert 0 < sum(len(x) for x in neighs) < len(rows) * (len(rows) - 1)


@pytest.mark.parametrize('nq', QC.FIELD_NQ)
def test_the_sort_keys_fields_have_the_widths_named(nq):
    widths = []
    for s in QC.FIELD_SUMS:
        c = QC.field_widths(s, nq)
        nR, lens = len(c['ref']), QC.lengths(c)
        assert len(lens) == nq and nR + lens.max() == s and lens[-1] == lens.max()
        nd = nR + int(lens.max()) + 1
        widths.append((QC.bits_for(nd - 1), QC.bits_for(nR + int(lens.max()))))
        rows, off = QC.rows_of(c)
        k = c['wordlen']
        assert rows[:, 1].min() == -(lens[-1] - k) and rows[:, 1].max() == nR - k       # both extreme buckets in use
        assert max(np.diff(off)) < 3000 and (np.diff(off) > 0).sum() >= min(nq, 3)
        neighs = _neighs(c)
        assert 0 < sum(len(x) for x in neighs)
    assert widths == [(8, 8), (9, 9), (9, 9)]
    assert QC.bits_for(max(nq - 1, 1)) == {1: 1, 2: 1, 3: 2, 257: 9}[nq]


def test_twins_have_equal_lists_and_no_edge_crosses():
    c = QC.twins()
    rows, off = QC.rows_of(c)
    assert np.array_equal(c['queries'][1], c['queries'][2])
    n = off[2] - off[1]
    assert n == off[3] - off[2] > 50 and np.array_equal(rows[off[1]:off[2], 1:], rows[off[2]:off[3], 1:])
    neighs = _neighs(c)
    assert [[v + n for v in x] for x in neighs[off[1]:off[2]]] == neighs[off[2]:off[3]]
    assert sum(len(x) for x in neighs[off[1]:off[2]]) > 0
    for q in range(len(c['queries'])):
        assert all(off[q] <= v < off[q + 1] for x in neighs[off[q]:off[q + 1]] for v in x)


def test_a_pair_on_the_d_radius_and_one_past_it():
    D, A = QC.NEAR_D, QC.NEAR_A
    assert Fraction(A, D).denominator & (Fraction(A, D).denominator - 1)        # c is inexact in binary
    for delta, total in ((D, 2), (D + 1, 0)):
        c = QC.near_miss_d(delta)
        rows, off = QC.rows_of(c)
        assert np.diff(off).tolist() == [1, 2]
        diff = rows[2] - rows[1]
        assert diff.tolist() == [0, delta, delta] and delta < A
        neighs = _neighs(c)
        assert sum(len(x) for x in neighs) == total and (neighs[1:] == [[2], [1]]) == (total == 2)
        assert (Fraction(A, D) * delta <= A) == (total == 2)


def test_a_pair_on_the_a_radius_and_one_past_it():
    c = QC.near_miss_a()
    rows, off = QC.rows_of(c)
    t = QC.NEAR_T
    assert np.diff(off).tolist() == [1, 4]
    r = rows[1:]
    pairs = [(u, v) for u in range(4) for v in range(4) if r[u, 1] == r[v, 1] and r[v, 2] - r[u, 2] == 2 * t]
    assert len(pairs) == 1 and c['R'] == 2 * t and c['R_past'] == 2 * t - 1
    u, v = pairs[0]
    neighs = _neighs(c)
    assert sum(len(x) for x in neighs) == 2 and neighs[1 + u] == [1 + v] and neighs[1 + v] == [1 + u]
    assert sum(len(x) for x in _neighs(c, c['R_past'])) == 0


def test_a_radius_of_two_and_a_half_takes_two_and_leaves_three():
    c = QC.non_integer_radius()
    assert (c['c'], c['R']) == (1., 2.5)
    rows, off = QC.rows_of(c)
    assert np.diff(off).tolist() == [3, 6]
    neighs = _neighs(c)
    two = three = 0
    for u in range(off[1], off[2]):
        for v in range(off[1], off[2]):
            dd, da = abs(int(rows[u, 1] - rows[v, 1])), abs(int(rows[u, 2] - rows[v, 2]))
            if dd <= 2 and da == 2:
                assert v in neighs[u]
                two += 1
            if dd <= 2 and da == 3:                            # the d axis would let it pass: a alone keeps it out
                assert v not in neighs[u]
                three += 1
    assert two >= 2 and three >= 2
    # ... and a radius rounded up would take them
    assert sum(len(x) for x in _neighs(c, 3.)) >= sum(len(x) for x in neighs) + three


@pytest.mark.parametrize('which', range(len(QC.ROUNDINGS)))
def test_the_rounding_cases_hold_a_pair_on_which_float_and_exact_differ(which):
    exact_decimal, exact_binary, fl = ((True, False, False), (True, False, True), (True, True, False))[which]
    c = QC.rounding(which)
    c0, R0, d0 = QC.ROUNDINGS[which]
    assert c['c'] == QC.ROUND_SCALE * c0 and c['R'] == QC.ROUND_SCALE * R0 and c['d0'] == d0
    # the scaling is exact: the same doubles, two binary places up
    assert Fraction(c['c']) == QC.ROUND_SCALE * Fraction(c0) and Fraction(c['R']) == QC.ROUND_SCALE * Fraction(R0)
    assert all(np.float64(d) * c['c'] == QC.ROUND_SCALE * (np.float64(d) * c0) for d in range(-50, 50))
    rows, off = QC.rows_of(c)
    pairs = [(u, v) for u in range(off[1], off[2]) for v in range(off[1], off[2])
             if rows[u, 1] == d0 + 2 and rows[v, 1] == d0 - 1 and abs(int(rows[u, 2] - rows[v, 2])) == 1]
    assert pairs and c['R'] >= 1
    neighs = _neighs(c)
    assert all((v in neighs[u]) == fl and (u in neighs[v]) == fl for u, v in pairs)
    assert (Fraction(c0) * 3 <= Fraction(R0)) == exact_binary
    assert (Fraction(str(c0)) * 3 <= Fraction(str(R0))) == exact_decimal


def test_one_rounding_case_tells_a_diagonal_offset_off_by_one():
    """fl(d c) is no linear function of d: for the pair of one of the rounding cases the test comes out the other way
    when both diagonals are shifted by one, which is what an offset wrong by one in the scan's own d would do."""
    differ = []
    for which, (c0, R0, d0) in enumerate(QC.ROUNDINGS):
        c, R_ = QC.ROUND_SCALE * c0, QC.ROUND_SCALE * R0
        differ.append(MC.lands(d0 + 2, 3, c, R_) != MC.lands(d0 + 3, 3, c, R_))
    assert any(differ)


def test_radius_zero_leaves_no_edge():
    c = QC.radius_zero()
    rows, off = QC.rows_of(c)
    assert c['R'] == 0 and len(rows) > 50 and sum(len(x) for x in _neighs(c)) == 0


def test_the_window_is_clamped_and_every_query_is_a_clique():
    c = QC.window_clamped()
    rows, off = QC.rows_of(c)
    nd = len(c['ref']) + int(QC.lengths(c).max()) + 1
    assert np.floor(c['R'] / c['c']) + 2 > nd
    neighs = _neighs(c)
    assert all(np.diff(off) >= 5)
    for q in range(2):
        assert all(x == [v for v in range(off[q], off[q + 1]) if v != off[q] + u] for u, x in enumerate(neighs[off[q]:off[q + 1]]))


def test_each_query_of_the_chain_is_one_scrambled_path():
    c = QC.chain()
    rows, off = QC.rows_of(c)
    m = QC.CHAIN_M
    assert np.diff(off).tolist() == [m, m]
    neighs = _neighs(c)
    for q in range(2):
        word = c['perms'][q]                                    # row off[q] + p holds word word[p]
        assert ((rows[off[q]:off[q + 1], 2] + rows[off[q]:off[q + 1], 1]) // 2 == word * QC.CHAIN_STRIDE).all()
        at = np.argsort(word)                                   # at[w] = the row (within the query) of word w
        assert np.abs(np.diff(at)).mean() > m / 5               # scrambled along the path
        for p in range(m):
            want = sorted(int(off[q] + at[w]) for w in (word[p] - 1, word[p] + 1) if 0 <= w < m)
            assert neighs[off[q] + p] == want
        ecc, reached = DO.diameter_from(neighs, int(off[q] + at[0]))
        assert reached == m and ecc == m - 1
    masks = QC.chain_masks(len(rows))
    comps = {name: QO.components(neighs, mk.tolist()) for name, mk in masks.items()}
    assert set(comps['all']) == {min(comps['all'][:m]), min(comps['all'][m:])} and set(comps['none']) == {-1}
    assert len(set(comps['every_50th_off']) - {-1}) >= 3 and len(set(comps['random_half']) - {-1}) > m // 4

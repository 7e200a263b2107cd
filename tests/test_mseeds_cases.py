"""Every named case of tests/mseeds_cases.py lands in the class it is named for -- proved from the dense oracle alone
(oracle/mseeds_dense_oracle.py), so that tests/test_gpu_mseeds_every_n.py, which runs the same inputs on the device,
is known to reach the code it is meant to reach.  If a seed does not land, the seed changes, not the assertion.
No GPU."""
from fractions import Fraction

import numpy as np
import pytest

from oracle import mseeds_dense_oracle as DO
from tests import mseeds_cases as MC


def _runs(c):
    return DO.run_lengths(c['seqs'], c['wordlen'], c['L'])


# ---- every N -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('N', MC.ALL_N)
def test_every_n_leaves_between_50_and_3000_rows(N):
    c = MC.every_n(N)
    assert len(c['seqs']) == N and 100 <= c['core'] <= 200
    rows = MC.rows_of(c)
    assert rows.shape[1] == N and 50 <= len(rows) <= 3000, len(rows)
    # a graph worth comparing: some rows have neighbours, and not every pair is connected
    neighs = DO.neighbours(rows, *MC.EVERY_N_RADII)
    edges = sum(len(x) for x in neighs)
    assert 0 < edges < len(rows) * (len(rows) - 1)


def test_the_mutation_rate_falls_as_n_grows():
    rates = [MC.mutation_rate(N) for N in MC.ALL_N]
    assert all(a > b for a, b in zip(rates, rates[1:]))
    assert .004 <= MC.mutation_rate(16) <= .008


def test_an_empty_and_a_short_member_leave_no_rows():
    for c in (MC.with_an_empty_member(), MC.with_a_member_one_short_of_a_word()):
        assert len(MC.rows_of(c)) == 0 and MC.rows_of(c).shape == (0, c['N'])
    assert len(MC.with_an_empty_member()['seqs'][2]) == 0
    assert len(MC.with_a_member_one_short_of_a_word()['seqs'][-1]) == MC.EVERY_N_W - 1


# ---- mixed radix ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('N', MC.MIXED_N)
def test_mixed_radix_sets_hold_the_radices_they_name(N):
    c = MC.mixed_radix(N)
    runs = _runs(c)
    # the shared k-mers are the planted words and nothing else, with the planted multiplicities
    want = sorted((sum(x * MC.PLANT_L ** (MC.PLANT_W - 1 - t) for t, x in enumerate(MC.word(j))), rl)
                  for j, rl in c['runs'].items())
    assert [(k, rl) for k, rl, _ in runs] == want
    rls = [rl for _, rl, _ in runs]
    # neighbouring sequences never share a radix, three values or more
    assert any(all(rl[s] != rl[s + 1] for s in range(N - 1)) and len(set(rl)) >= 3 for rl in rls)
    # a radix of 1 at s = 0, at s = N - 1 and between two larger ones
    assert any(rl[0] == 1 and max(rl) > 1 for rl in rls)
    assert any(rl[-1] == 1 and max(rl) > 1 for rl in rls)
    assert any(rl[s] == 1 and rl[s - 1] > 1 and rl[s + 1] > 1 for rl in rls for s in range(1, N - 1))
    assert len(MC.rows_of(c)) == sum(int(np.prod(rl)) for rl in rls) <= 6000


@pytest.mark.parametrize('N', MC.MIXED_N)
def test_a_decode_with_the_radices_in_the_other_order_gives_other_rows(N):
    """What the unequal radices are for: the same seeds enumerated with sequence 0 fastest instead of slowest are a
    different table -- the same rows, in another order -- so a row-for-row comparison tells the two decodes apart."""
    from itertools import product
    c = MC.mixed_radix(N)
    hits = [DO.positions(s, c['wordlen'], c['L']) for s in c['seqs']]
    wrong = []
    for k in sorted(hits[0]):
        if all(k in h for h in hits):
            for idx in product(*[h[k] for h in hits][::-1]):
                idx = idx[::-1]
                wrong.append([idx[0] - x for x in idx[1:]] + [sum(idx)])
    rows = MC.rows_of(c).tolist()
    assert wrong != rows and sorted(wrong) == sorted(rows)
    # more than half the rows of the k-mers that have more than one row stand elsewhere
    several = sum(int(np.prod(rl)) for rl in c['runs'].values() if max(rl) > 1)
    assert sum(x != y for x, y in zip(wrong, rows)) > several // 2


@pytest.mark.parametrize('start', MC.WINDOW_STARTS)
@pytest.mark.parametrize('N', MC.MIXED_N)
def test_a_kmer_starts_on_the_row_named_and_fills_whole_windows(N, start):
    c = MC.windows(N, start)
    runs = _runs(c)
    sizes = {at: int(np.prod(rl)) for _, rl, at in runs}
    assert sizes[start] > 2 * MC.EXP_ROWS                  # the k-mer on row `start` has more than 4096 rows:
    first_whole = -(-start // MC.EXP_ROWS) * MC.EXP_ROWS   # a workgroup window lies inside it from end to end
    assert first_whole + MC.EXP_ROWS <= start + sizes[start]
    assert sizes[start + sizes[start]] > MC.EXP_ROWS       # and the next has more than 2048
    assert len(MC.rows_of(c)) == sum(sizes.values())
    # the padding before it: radices of 1 beside larger ones, the larger ones moving through the sequences
    assert len({tuple(np.flatnonzero(np.array(rl) > 1)) for _, rl, at in runs if at < start}) >= 2


def test_sixteen_sequences_of_radix_two():
    c = MC.radix_two_everywhere()
    runs = _runs(c)
    assert [rl for _, rl, _ in runs] == [(2,) * 16, (1,) * 16]
    assert len(MC.rows_of(c)) == 65537


# ---- near misses ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('N', MC.NEAR_N)
def test_a_pair_differs_in_one_coordinate_alone_and_sits_on_or_past_the_radius(N):
    D, A = MC.NEAR_D, MC.NEAR_A
    assert Fraction(A, D).denominator & (Fraction(A, D).denominator - 1)        # c is inexact in binary
    for delta, inside in ((D, True), (D + 1, False)):
        c = MC.near_miss(N, delta)
        rows = MC.rows_of(c)
        assert len(rows) == 2 * (N - 1)
        neighs = DO.neighbours(rows, D, A)
        seen = set()
        for i in range(0, len(rows), 2):                   # the two seeds of a word are adjacent rows
            diff = rows[i] - rows[i + 1]
            k = [int(x) for x in np.flatnonzero(diff[:-1])]
            assert len(k) == 1 and diff[k[0]] == delta and diff[-1] == -delta and delta < A
            seen.add(k[0])
            assert ((i + 1) in neighs[i]) == inside and (i in neighs[i + 1]) == inside
        assert seen == set(range(N - 1))                   # every coordinate d_1 .. d_{N-1} has its pair
        # and the pairs are all there is: words stand too far apart to be neighbours
        assert sum(len(x) for x in neighs) == (2 * (N - 1) if inside else 0)


@pytest.mark.parametrize('N', MC.NEAR_N)
def test_a_scan_that_skipped_one_coordinate_would_connect_its_pair(N):
    """The pairs one past the radius are there to catch a loop over d_2 .. d_{N-1} that stops short or starts late: with
    coordinate k left out of the test, the pair of word k -- and no other -- becomes an edge."""
    rows = MC.rows_of(MC.near_miss(N, MC.NEAR_D + 1))
    assert sum(len(x) for x in DO.neighbours(rows, MC.NEAR_D, MC.NEAR_A)) == 0
    for k in range(N - 1):
        blind = DO.neighbours(np.delete(rows, k, axis=1), MC.NEAR_D, MC.NEAR_A)
        assert [i for i, x in enumerate(blind) if x] == [2 * k, 2 * k + 1]
        assert blind[2 * k] == [2 * k + 1] and blind[2 * k + 1] == [2 * k]


@pytest.mark.parametrize('N', MC.A_AXIS_N)
def test_a_pair_differs_in_a_alone_by_the_radius(N):
    c = MC.a_axis(N)
    rows = MC.rows_of(c)
    assert len(rows) == 2 ** N
    first, last = 0, len(rows) - 1
    assert (rows[first, :-1] == rows[last, :-1]).all() and rows[last, -1] - rows[first, -1] == c['radius'] == N * c['t']
    only = DO.neighbours_cr(rows[[first, last]], c['radius'], c['radius'])
    assert only == [[1], [0]]
    assert DO.neighbours_cr(rows[[first, last]], c['radius'], c['radius'] - 1) == [[], []]
    if N <= 9:
        # d_coeff = N t keeps every other pair out: that edge is the whole graph
        neighs = DO.neighbours_cr(rows, c['radius'], c['radius'])
        assert neighs[first] == [last] and neighs[last] == [first] and sum(len(x) for x in neighs) == 2
        assert sum(len(x) for x in DO.neighbours_cr(rows, c['radius'], c['radius'] - 1)) == 0
    else:
        # 65 536 rows are past the quadratic oracle: no other row shares every d with these two, and any other d differs
        # by t, which d_coeff = N t scales past the radius
        same = (rows[:, :-1] == rows[first, :-1]).all(1)
        assert np.flatnonzero(same).tolist() == [first, last]
        assert np.float64(c['t']) * np.float64(c['radius']) > c['radius']


# ---- rounding ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('axis', [1, 2])
def test_the_rounding_sets_hold_a_pair_on_which_float_and_exact_differ(axis):
    for (c, R_, d0), exact_decimal, exact_binary, fl in (
            ((MC.ROUND_C, MC.ROUND_R, MC.ROUNDING_D0[0]), True, False, False),
            ((MC.ROUND_C, MC.ROUND_R, MC.ROUNDING_D0[1]), True, False, True),
            (MC.ROUNDING_OTHER_WAY, True, True, False)):
        rows = MC.rows_of(MC.rounding(axis, d0))
        k = axis - 1
        pairs = [(i, j) for i in range(len(rows)) for j in range(len(rows)) if rows[i, -1] == rows[j, -1] and
                 rows[i, k] == d0 + 2 and rows[j, k] == d0 - 1 and rows[i, 1 - k] == rows[j, 1 - k]]
        assert pairs
        neighs = DO.neighbours_cr(rows, c, R_)
        assert all((j in neighs[i]) == fl and (i in neighs[j]) == fl for i, j in pairs)
        assert (Fraction(c) * 3 <= Fraction(R_)) == exact_binary
        assert (Fraction(str(c)) * 3 <= Fraction(str(R_))) == exact_decimal


# ---- chains --------------------------------------------------------------------------------------------------
def test_the_chain_is_one_scrambled_path_a_thousand_hops_long():
    c = MC.chain()
    runs = _runs(c)
    assert all(rl == (1, 1, 1) for _, rl, _ in runs)       # no repeated k-mer
    rows = MC.rows_of(c)
    n = MC.CHAIN_LEN - MC.CHAIN_W + 1
    assert len(rows) == n and (rows[:, :2] == 0).all() and sorted(rows[:, 2].tolist()) == list(range(0, 3 * n, 3))
    # rows are in k-mer order: along the chain the row numbers are scrambled
    along = np.argsort(rows[:, 2])
    assert np.abs(np.diff(along)).mean() > n / 10
    for R_, hops in zip(MC.CHAIN_RADII, (1, 2)):
        neighs = DO.neighbours_cr(rows, 1., R_)
        assert max(len(x) for x in neighs) == 2 * hops
        ecc, reached = DO.diameter_from(neighs, int(along[0]))
        assert reached == n and ecc == -(-(n - 1) // hops) >= 1000
    # the masks: what each does to the one-hop chain
    neighs = DO.neighbours_cr(rows, 1., MC.CHAIN_RADII[0])
    masks = MC.chain_masks(n)
    comps = {name: DO.components(neighs, m.tolist()) for name, m in masks.items()}
    assert set(comps['all']) == {0} and set(comps['none']) == {-1}
    off = int((~masks['every_50th_off']).sum())
    assert off == -(-n // 50) and off // 2 < len(set(comps['every_50th_off']) - {-1}) <= off + 1
    assert len(set(comps['random_half']) - {-1}) > n // 8


# ---- boxes ---------------------------------------------------------------------------------------------------
def test_the_large_index_outgrows_one_pass_of_the_counting_grid():
    rows = MC.rows_of(MC.many_rows())
    assert 1024 * 256 < len(rows) < 1000000


def test_the_box_batches_straddle_the_chunk():
    assert MC.BOX_BATCHES == (1, 63, 64, 65, 128, 129, 1000)
    assert {b % MC.BOX_CHUNK for b in MC.BOX_BATCHES} >= {0, 1, 63} and max(MC.BOX_BATCHES) > 15 * MC.BOX_CHUNK


@pytest.mark.parametrize('which', ['many_rows', 'every_n_16'])
def test_the_named_boxes_are_what_they_are_named(which):
    c = MC.many_rows() if which == 'many_rows' else MC.every_n(16)
    rows = MC.rows_of(c)
    N = c['N']
    lo, hi, have = MC.boxes(rows, 1000 if which == 'many_rows' else 129, 1)
    want = DO.box_counts(rows, lo, hi, have)
    m = MC.n_named_boxes(N)
    assert (have[:N].sum(1) == 1).all() and (np.argmax(have[:N], 1) == np.arange(N)).all()      # each coordinate alone
    assert (want[:N] > 0).all() and (which != 'many_rows' or (want[:N] < len(rows)).all())
    assert (lo[N:2 * N] == hi[N:2 * N])[have[N:2 * N] > 0].all() and (want[N:2 * N] > 0).all()  # lo == hi == a value
    assert (lo[2 * N:3 * N] > hi[2 * N:3 * N])[have[2 * N:3 * N] > 0].all() and (want[2 * N:3 * N] == 0).all()
    assert (want[3 * N:4 * N + 3] == len(rows)).all()       # int32 extremes, nothing bounded, all extremes, bounding box
    assert have[4 * N].sum() == 0 and have[4 * N + 1].sum() == N
    assert lo[3 * N:4 * N].min() == MC.I32_MIN and hi[3 * N:4 * N].max() == MC.I32_MAX
    assert want[4 * N + 3] >= 1 and have[4 * N + 3].sum() == N                                   # one row exactly
    assert (want[4 * N + 4:m] == 0).all() and lo[4 * N + 4, 0] == MC.I32_MIN and hi[m - 1, N - 1] == MC.I32_MAX
    # the random rest: neither all empty nor all full, and boxes of one call differ
    rest = want[m:]
    assert len(rest) and 0 < (rest > 0).sum() and (rest < len(rows)).any() and len(set(rest.tolist())) > len(rest) // 10


def test_the_largest_batch_is_the_limit_of_the_abi():
    rows = MC.rows_of(MC.tiny_pair())
    assert 1 <= len(rows) <= 16
    lo, hi, have = MC.max_boxes(rows)
    assert len(lo) == MC.MAX_BOXES == 64 * 65535
    want = DO.box_counts(rows, lo, hi, have)
    assert len(set(want.tolist())) >= 3 and (want == 0).any() and (want == len(rows)).any()
    assert (lo > hi).any()

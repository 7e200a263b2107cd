"""The dense oracle of the N-way seed index (oracle/mseeds_dense_oracle.py) anchored on the CPU: it equals the cKDTree
yardstick tests/mseeds_ref.py on small seeded sets at every N, reproduces the reference's own fixtures, and sides with
the KD-tree -- not with exact arithmetic -- where the two differ.  No GPU."""
import gzip
import json
import os
from fractions import Fraction

import numpy as np
import pytest
from scipy.spatial import cKDTree

from oracle import mseeds_dense_oracle as DO
from tests import mseeds_cases as MC
from tests import mseeds_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


def _draw(N, L, w, rng):
    core = rng.integers(0, L, 36)
    seqs = []
    for _ in range(N):
        c = core.copy()
        flip = rng.random(len(c)) < .6 / N / w
        c[flip] = rng.integers(0, L, int(flip.sum()))
        seqs.append(np.r_[rng.integers(0, L, int(rng.integers(0, 6))), c, rng.integers(0, L, int(rng.integers(0, 6)))])
    return seqs


def _small_set(N, L, seed):
    """N short sequences sharing a mutated core; short words, so that k-mers repeat and radices are unequal.  Redrawn
    from the same generator until the product of the run lengths leaves 20 .. 3000 rows."""
    rng = np.random.default_rng(seed)
    w = {2: 6, 4: 3, 20: 2}[L] + (1 if N > 8 else 0)
    while True:
        seqs = _draw(N, L, w, rng)
        if 20 <= sum(int(np.prod(rl, dtype=np.int64)) for _, rl, _ in DO.run_lengths(seqs, w, L)) <= 3000:
            return seqs, w


SMALL = [(N, (2, 4, 20)[(N + t) % 3], 100 * N + t) for t in (0, 1) for N in MC.ALL_N]


@pytest.mark.parametrize('N,L,seed', SMALL)
def test_the_dense_oracle_equals_the_kd_tree_yardstick(N, L, seed):
    seqs, w = _small_set(N, L, seed)
    rows = DO.seed_rows(seqs, w, L)
    want = R.seed_rows(seqs, w, L)
    assert rows.shape == want.shape and np.array_equal(rows, want)
    assert 20 <= len(rows) <= 3000, len(rows)
    rng = np.random.default_rng(seed)
    for d_radius, a_radius in ((3, 2 * N), (7, 30), (2, 5 * N)):
        neighs = DO.neighbours(rows, d_radius, a_radius)
        assert neighs == R.neighbours(rows, d_radius, a_radius)
        for avail in (np.ones(len(rows), bool), rng.random(len(rows)) < .5, rng.random(len(rows)) < .9):
            assert DO.components(neighs, avail.tolist()) == R.components(neighs, avail.tolist())
    for t in rng.integers(0, len(rows), 12):
        r = rows[t]
        ds = [None if rng.random() < .3 else (int(r[k]) - 4, int(r[k]) + 3) for k in range(N - 1)]
        for a in (None, (int(r[-1]) - 10 * N, int(r[-1]) + 10 * N)):
            assert DO.box_count(rows, ds, a) == R.box_count(rows, ds, a)
    assert DO.box_count(rows, None, None) == len(rows)


def test_the_small_sets_cover_every_n_and_three_alphabets():
    assert len(SMALL) == 30
    assert {N for N, _, _ in SMALL} == set(MC.ALL_N) and {L for _, L, _ in SMALL} == {2, 4, 20}
    # and they are not all radix 1: somewhere a k-mer repeats in one sequence and not in another
    mixed = 0
    for N, L, seed in SMALL:
        seqs, w = _small_set(N, L, seed)
        mixed += any(len(set(rl)) > 1 for _, rl, _ in DO.run_lengths(seqs, w, L))
    assert mixed >= 10, mixed


def _fixture(name):
    with gzip.open(os.path.join(GOLDEN, name), 'rt') as f:
        return json.load(f)['cases']


def _radii(rec):
    """The radii score_seeds(K) uses (WordBlotMultiple._radii); band_radius is host arithmetic, no device is touched."""
    from biseqt_amd.blot import band_radius
    N, K = len(rec['seqs']), rec['score_seeds']['K']
    d_radius = int(np.ceil(band_radius(K, float.fromhex(rec['g_max']), float.fromhex(rec['sensitivity']))))
    return d_radius, int(np.ceil(N * K / 2.))


@pytest.mark.parametrize('name', ['blot_multi.json.gz', 'blot_multi_wide.json.gz'])
def test_the_dense_oracle_reproduces_the_reference_fixtures(name):
    cases = _fixture(name)
    assert cases
    for rec in cases:
        seqs = [['ACGT'.index(c) for c in s] for s in rec['seqs']]
        rows = DO.seed_rows(seqs, rec['wordlen'], 4)
        assert rows.tolist() == rec['rows']
        neighs = DO.neighbours(rows, *_radii(rec))
        assert neighs == [r['neighs'] for r in rec['score_seeds']['records']]
        for c in rec['counts']:
            assert DO.box_count(rows, c['ds_band'], c['a_band']) == c['count']


def test_the_wide_fixture_covers_the_sequence_counts_the_first_one_lacks():
    ns = [len(rec['seqs']) for rec in _fixture('blot_multi_wide.json.gz')]
    assert set(ns) == {7, 9, 10, 11, 12, 13, 14, 15, 16}
    kinds = {(len(rec['seqs']) >= 9, rec['kind']) for rec in _fixture('blot_multi_wide.json.gz')}
    assert (True, 'unrelated') in kinds and (True, 'identical') in kinds
    assert all(50 <= len(rec['rows']) <= 3000 for rec in _fixture('blot_multi_wide.json.gz'))
    assert os.path.getsize(os.path.join(GOLDEN, 'blot_multi_wide.json.gz')) < 1 << 20


# ---- the KD-tree's rounding ----------------------------------------------------------------------------------------
def _tree(rows, c, R_):
    pts = np.array([[float(d) * c for d in r[:-1]] + [float(r[-1])] for r in rows.tolist()])
    tree = cKDTree(pts)
    return [sorted(x for x in lst if x != i) for i, lst in enumerate(tree.query_ball_tree(tree, R_, p=float('inf')))]


def _rational(rows, c, R_):
    """The same relation with every product and difference exact: c and R as the fractions given."""
    out = []
    for i, r in enumerate(rows.tolist()):
        out.append([j for j, q in enumerate(rows.tolist()) if j != i and abs(r[-1] - q[-1]) <= R_ and
                    all(abs(x - y) * c <= R_ for x, y in zip(r[:-1], q[:-1]))])
    return out


@pytest.mark.parametrize('axis', [1, 2])
def test_on_the_rounding_cases_the_oracle_is_the_kd_tree_and_not_the_rationals(axis):
    c, R_ = MC.ROUND_C, MC.ROUND_R
    decimal = (Fraction(1, 10), Fraction(3, 10))            # what 0.1 and 0.3 are written as
    binary = (Fraction(c), Fraction(R_))                    # what the doubles 0.1 and 0.3 are
    differs = {}
    for d0 in MC.ROUNDING_D0:
        rows = MC.rows_of(MC.rounding(axis, d0))
        assert len(rows) == 12
        dense = DO.neighbours_cr(rows, c, R_)
        assert dense == _tree(rows, c, R_)
        differs[d0] = (dense != _rational(rows, *decimal), dense != _rational(rows, *binary))
        # the pairs in question: equal a, d_axis apart by 3, the other d equal
        k = axis - 1
        pairs = [(i, j) for i in range(12) for j in range(12) if rows[i, -1] == rows[j, -1] and
                 rows[i, k] - rows[j, k] == MC.ROUND_DELTA and rows[i, 1 - k] == rows[j, 1 - k]]
        assert pairs
        assert {int(rows[i, k]) for i, _ in pairs} == {d0 + 2} and {int(rows[j, k]) for _, j in pairs} == {d0 - 1}
        for i, j in pairs:
            assert (j in dense[i]) == MC.lands(d0 + 2, 3, c, R_) and (i in dense[j]) == (j in dense[i])
    # d0 = 1 (3 against 0): float says no, 3 / 10 <= 3 / 10 says yes, the doubles' exact values say no
    assert not MC.lands(3, 3, c, R_) and differs[1] == (True, False)
    # d0 = 7 (9 against 6): float says yes, decimal says yes, the doubles' exact values say no
    assert MC.lands(9, 3, c, R_) and differs[7] == (False, True)


def test_a_small_grid_holds_float_and_exact_disagreements_in_both_directions():
    """Searches (c, R, delta, d) for the float test |fl(d c) - fl((d - delta) c)| <= R disagreeing with the exact
    delta c <= R on the doubles c and R themselves, and records the first triple found each way."""
    found = {}
    for c in (.1, .2, .3, .7, 1.1, 30. / 7):
        for R_ in (.3, .6, .9, 2.1, 3.3, 30.):
            for delta in range(1, 12):
                exact = Fraction(c) * delta <= Fraction(R_)
                for d in range(delta, 40):
                    fl = MC.lands(d, delta, c, R_)
                    if fl != exact:
                        found.setdefault('float connects, exact does not' if fl else 'exact connects, float does not',
                                         (c, R_, delta, d))
    print(found)
    assert found['float connects, exact does not'][:3] == (.1, .3, 3)
    assert 'exact connects, float does not' in found
    c, R_, delta, d = found['exact connects, float does not']
    assert Fraction(c) * delta <= Fraction(R_) and not MC.lands(d, delta, c, R_)

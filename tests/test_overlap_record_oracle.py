"""oracle/overlap_record_oracle.py (dense numpy restatement of the documented band record) anchored on the CPU to the
KD-tree restatement of the reference, oracle/blot_oracle.py + oracle/seeds_oracle.py: the seed diagonals in table order,
the neighbour count / radius / length behind EVERY seed's p, and the chosen band.  No GPU."""
import numpy as np
import pytest

from oracle import blot_oracle as BO, overlap_record_oracle as RO, seeds_oracle as SO
from tests.overlap_cases import _mutate


def _pairs():
    """48 random small pairs: lengths 20..400, wordlen 3..7 over 4 letters plus a few over 2 and 20 letters, every third
    pair with a planted overlap, g_max and sensitivity varied; then the degenerate shapes."""
    rng = np.random.default_rng(20240917)
    out = []
    for q in range(48):
        if q % 8 == 6:
            L, k = 2, int(rng.integers(5, 9))
        elif q % 8 == 7:
            L, k = 20, int(rng.integers(1, 4))
        else:
            L, k = 4, 3 + q % 5
        ls, lt = int(rng.integers(20, 401)), int(rng.integers(20, 401))
        S, T = rng.integers(0, L, ls).astype(np.uint8), rng.integers(0, L, lt).astype(np.uint8)
        if q % 3 == 0:                                      # planted overlap: a suffix of S continues as a prefix of T
            ov = int(rng.integers(10, min(ls, lt) + 1))
            T = np.concatenate([_mutate(rng, S[ls - ov:], L, .03), T])[:lt]
        g, sens = (.1, .2, .3)[q % 3], (.9, .99)[q % 2]
        out.append((S, T, k, L, g, sens))
    e = np.zeros(0, np.uint8)
    r = rng.integers(0, 4, 50).astype(np.uint8)
    out += [(e, r, 4, 4, .2, .99), (r, e, 4, 4, .2, .99),                       # an empty read
            (r[:3], r, 4, 4, .2, .99), (r, r[10:13], 4, 4, .2, .9),             # a read shorter than the word
            (r[5:9], r, 4, 4, .2, .99), (r, r[20:24], 4, 4, .1, .9)]           # a read of exactly one word
    return out


PAIRS = _pairs()


def test_enough_pairs_of_every_kind():
    assert len(PAIRS) >= 40
    assert sum(L == 2 for _, _, _, L, _, _ in PAIRS) >= 3 and sum(L == 20 for _, _, _, L, _, _ in PAIRS) >= 3
    assert {k for _, _, k, L, _, _ in PAIRS if L == 4} >= {3, 4, 5, 6, 7}


@pytest.mark.parametrize('q', range(len(PAIRS)))
def test_record_oracle_vs_kdtree_oracle(q):
    S, T, k, L, g, sens = PAIRS[q]
    assert not (len(S) == len(T) and (S == T).all())        # (identical reads are a self comparison in the reference)
    o = RO.band_record(S, T, k, L, g, sens)
    # seeds, in table order
    rows, self_comp = SO.seed_rows(S.tolist(), T.tolist(), k, L)
    ij = SO.seeds(rows, self_comp)
    assert not self_comp
    i, j = RO.seed_positions(S, T, k, L)
    assert list(zip(i.tolist(), j.tolist())) == ij
    ds = RO.seed_diagonals(S, T, k, L)
    assert ds.tolist() == [d for d, _ in rows] and o['n_seeds'] == len(rows)
    hs = BO.highest_scoring_overlap_band(S.tolist(), T.tolist(), k, L, g, sens)
    if not rows:
        assert hs is None and o['nocc'] == 0
        return
    assert o['nocc'] == len(set(ds.tolist())) and (np.diff(o['d']) > 0).all()
    # every seed: the p, r and L the KD-tree search gives it
    scored = BO.score_seeds(S.tolist(), T.tolist(), k, L, g, sens)
    assert len(scored) == len(ds)
    at = {int(d): z for z, d in enumerate(o['d'])}
    for rec, d in zip(scored, ds.tolist()):
        z = at[d]
        assert rec['seed'][0] == d
        assert rec['r'] == o['r'][z] and rec['L'] == o['L'][z], (d, rec)
        assert rec['p'] == BO.match_p(int(o['n'][z]), int(o['r'][z]), int(o['L'][z]), L, k), (d, rec)
    # the per-diagonal score and the record's own fields hang together
    p0 = (1. / L) ** k
    for z in range(o['nocc']):
        assert o['w'][z] == (int(o['n'][z]) + 1 - 2 * int(o['r'][z]) * int(o['L'][z]) * p0) / int(o['L'][z])
    assert o['w_best'] == o['w'].max() and o['d_best'] == o['d'][o['w'] == o['w'].max()].min()
    assert o['d_first'] == ds[0]
    for tag in ('best', 'first'):
        z = at[o['d_' + tag]]
        assert (o['n_' + tag], o['r_' + tag], o['len_' + tag]) == (o['n'][z], o['r'][z], o['L'][z])
        lo, hi = o['d_' + tag] - o['r_' + tag], o['d_' + tag] + o['r_' + tag]
        assert o['band_' + tag] == SO.seed_count(rows, d_band=(lo, hi))

    def result(tag):
        rad = np.float64(o['r_' + tag])
        p = BO.match_p(o['n_' + tag], o['r_' + tag], o['len_' + tag], L, k)
        mu, sd = BO.H1_moments(L, k, 2 * rad * o['len_' + tag], o['len_' + tag], p)
        return {'d_band': (o['d_' + tag] - rad, o['d_' + tag] + rad), 'len': o['len_' + tag], 'p': p,
                'score': (o['band_' + tag] - mu) / sd}

    if o['w_best'] > 0:
        assert 1 <= o['tie'] <= o['nocc']
        if o['tie'] == 1:
            assert hs == result('best')
    else:
        assert o['tie'] == o['nocc']
        assert hs == result('first') and hs['p'] == 0

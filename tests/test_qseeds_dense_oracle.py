"""oracle/qseeds_dense_oracle.py, the yardstick of tests/test_gpu_qseeds_edges.py, anchored to the oracles the batched
Word-Blot was first tested with, on the three mixed cases of tests/blot_many_cases.py: rows == seeds_by_mutant per query,
neighbour lists == blot_oracle.find_all_neighbors (the reference's own cKDTree call) per query, labels ==
blot_many_cases.components, box counts == blot_oracle._seed_count.  Every comparison is exact.  No GPU."""
import functools

import numpy as np
import pytest

from oracle import blot_oracle as BO, qseeds_dense_oracle as QO
from tests import blot_many_cases as Cs

NAMES = ('a', 'b', 'c')


@functools.lru_cache(maxsize=None)
def dense(name):
    ref, queries, wordlen, K_min, _ = Cs.mixed_case(name)
    rows, off = QO.rows(ref, queries, wordlen, 4)
    d_radius, a_radius = Cs.radii(K_min)
    neighs = QO.neighbours(rows, off, 1. * a_radius / d_radius, a_radius)
    return rows, off, neighs


@functools.lru_cache(maxsize=None)
def restated(name):
    ref, queries, wordlen, K_min, p_min = Cs.mixed_case(name)
    return Cs.cpu_arrays(ref, queries, wordlen, K_min, p_min)


@pytest.mark.parametrize('name', NAMES)
def test_rows_are_seeds_by_mutant_per_query(name):
    ref, queries, wordlen, _, _ = Cs.mixed_case(name)
    rows, off, _ = dense(name)
    want, want_off = Cs.oracle_rows(ref, queries, wordlen)
    assert rows.dtype == np.int64 and off.dtype == np.int64 and rows.shape == want.shape and len(rows) > 500
    assert np.array_equal(rows, want) and np.array_equal(off, want_off)
    assert (np.diff(off) == 0).any() and (np.diff(off) > 100).any()


@pytest.mark.parametrize('name', NAMES)
def test_neighbours_are_the_kd_trees_per_query(name):
    _, queries, _, K_min, _ = Cs.mixed_case(name)
    rows, off, neighs = dense(name)
    d_radius, a_radius = Cs.radii(K_min)
    assert len(neighs) == len(rows)
    for q in range(len(queries)):
        b = int(off[q])
        pts = [(int(d), int(a)) for _, d, a in rows[b:off[q + 1]]]
        for k, (_, ns) in enumerate(BO.find_all_neighbors(pts, d_radius, a_radius)):
            assert neighs[b + k] == sorted(b + v for v in ns), (q, k)
    assert sum(len(x) for x in neighs) > 0
    assert [len(x) for x in neighs] == restated(name)['counts'].tolist()


@pytest.mark.parametrize('name', NAMES)
def test_labels_are_the_union_finds(name):
    rows, off, neighs = dense(name)
    cpu = restated(name)
    own = cpu['labels'] >= 0                         # the seeds the segments of this case grow from
    assert own.any() and (name == 'c' or not own.all())
    assert QO.components(neighs, own.tolist()) == cpu['labels'].tolist()
    rng = np.random.default_rng(5)
    for avail in (np.ones(len(rows), bool), rng.random(len(rows)) < .5, np.zeros(len(rows), bool)):
        assert QO.components(neighs, avail.tolist()) == Cs.components(neighs, avail.tolist()).tolist()


@pytest.mark.parametrize('name', NAMES)
def test_box_counts_are_the_in_memory_classes(name):
    _, queries, _, _, _ = Cs.mixed_case(name)
    rows, off, _ = dense(name)
    rng = np.random.default_rng(6)
    n = 50
    q = rng.integers(0, len(queries), n)
    q[:10] = np.flatnonzero(np.diff(off) > 0)[:10]              # at least ten boxes on queries that have rows
    pick = np.array([rows[rng.integers(off[k], off[k + 1])][1:] if off[k + 1] > off[k] else (0, 0) for k in q], np.int64)
    dmin, dmax = pick[:, 0] - rng.integers(0, 40, n), pick[:, 0] + rng.integers(0, 40, n)
    amin, amax = pick[:, 1] - rng.integers(0, 300, n), pick[:, 1] + rng.integers(0, 300, n)
    dmin[40:45], dmax[40:45] = pick[40:45, 0], pick[40:45, 0]   # a single diagonal
    amin[45:48] = amax[45:48] + 1                               # inverted
    got = QO.box_counts(rows, off, q, dmin, dmax, amin, amax)
    assert got.dtype == np.int64 and got.tolist() == restated(name)['count_boxes'](q, dmin, dmax, amin, amax).tolist()
    assert (got[:10] > 0).all() and (got[45:48] == 0).all() and len(set(got.tolist())) > 5

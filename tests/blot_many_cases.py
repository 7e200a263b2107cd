"""Inputs and CPU yardsticks shared by the tests of the query-batched Word-Blot (test_blot_many_host.py,
test_gpu_blot_many.py, test_gpu_map_queries.py): the mixed 40-query recipe, the oracle's answer per query (computed once
per case and shared), and the arrays the batched index produces -- rows, row offsets, neighbour counts, component labels,
box counts -- restated on the CPU from the oracles alone."""
import functools

import numpy as np

from biseqt_amd import synth
from biseqt_amd.blot import band_radius
from biseqt_amd.sequence import Alphabet, Sequence
from oracle import blot_oracle as BO, seeds_oracle as SO

A = Alphabet('ACGT')
G_MAX, SENS = .2, .99
# the mixed set: name -> (wordlen, reference length, K_min, p_min)
MIXED = {'a': (8, 3000, 100, .7), 'b': (6, 1200, 60, .7), 'c': (16, 3000, 100, .7)}


def mk(arr):
    return Sequence(A, tuple(int(c) for c in arr))


def mixed_queries(rng, ref, wordlen, n=40):
    """n queries cycling through five kinds: unrelated random (60-320 letters); 20 random letters, then a slice of the
    reference mutated at .05 / .03 / .03 (twice); two 150-letter mutated slices from different places with 40 random
    letters between them; a query of 1 .. wordlen + 1 letters."""
    out = []
    for k in range(n):
        kind = k % 5
        if kind == 0:
            out.append(synth.rand_seqs(rng, 1, int(rng.integers(60, 321)))[0])
        elif kind in (1, 2):
            ln = int(rng.integers(150, 281))
            at = int(rng.integers(0, len(ref) - ln))
            out.append(np.concatenate([synth.rand_seqs(rng, 1, 20)[0], synth.mutate(rng, ref[at:at + ln], .05, .03, .03)]))
        elif kind == 3:
            at1 = int(rng.integers(0, len(ref) // 2 - 150))
            at2 = int(rng.integers(len(ref) // 2, len(ref) - 150))
            out.append(np.concatenate([synth.mutate(rng, ref[at1:at1 + 150], .05, .03, .03), synth.rand_seqs(rng, 1, 40)[0],
                                       synth.mutate(rng, ref[at2:at2 + 150], .05, .03, .03)]))
        else:
            out.append(synth.rand_seqs(rng, 1, wordlen + 1 - (k // 5) % (wordlen + 1))[0])      # wordlen + 1, wordlen, ..
    return out


@functools.lru_cache(maxsize=None)
def mixed_case(name, n=40):
    """(ref, queries, wordlen, K_min, p_min) of one mixed case, as uint8 arrays."""
    wordlen, nref, K_min, p_min = MIXED[name]
    rng = synth.rng_for(9100 + wordlen)
    ref = synth.rand_seqs(rng, 1, nref)[0]
    return ref, mixed_queries(rng, ref, wordlen, n), wordlen, K_min, p_min


def oracle_segments(ref, query, wordlen, K_min, p_min, at_least_one=False):
    return BO.similar_segments(ref.tolist(), query.tolist(), wordlen, 4, G_MAX, SENS, K_min, p_min, at_least_one=at_least_one,
                               order='mutant')


@functools.lru_cache(maxsize=None)
def mixed_expected(name, n=40):
    ref, queries, wordlen, K_min, p_min = mixed_case(name, n)
    return [oracle_segments(ref, q, wordlen, K_min, p_min) for q in queries]


def assert_equals_oracle(got, exp, what=''):
    """Segments ==; the averaged p within 1e-12 relative (its last bits follow the KD-tree's neighbour order in the
    reference) and the z-scores derived from it with rtol 1e-9: the tolerances of test_blot_gpu.py."""
    assert [g['segment'] for g in got] == [e['segment'] for e in exp], what
    for g, e in zip(got, exp):
        assert abs(g['p'] - e['p']) <= 1e-12 * max(abs(e['p']), 1e-300), what
        assert np.allclose(g['scores'], e['scores'], rtol=1e-9, atol=0), what


def assert_identical(got, exp, what=''):
    """Everything ==: segments, order, p and scores bit for bit."""
    assert len(got) == len(exp), what
    for g, e in zip(got, exp):
        assert g['segment'] == e['segment'] and g['p'] == e['p'] and tuple(g['scores']) == tuple(e['scores']), (what, g, e)


def radii(K_min):
    return int(np.ceil(band_radius(K_min, G_MAX, SENS))), K_min


def oracle_rows(ref, queries, wordlen):
    """(rows (q, d, a), row offsets) of the batched table from seeds_oracle.seeds_by_mutant per query.  (A query equal to
    the reference is no self comparison here: it never enters the batched table.)"""
    rows, off = [], [0]
    for q, t in enumerate(queries):
        assert ref.tolist() != t.tolist()
        rows += [(q, i - j, i + j) for i, j in SO.seeds_by_mutant(ref.tolist(), t.tolist(), wordlen, 4)]
        off.append(len(rows))
    return np.array(rows, np.int32).reshape(-1, 3), np.array(off, np.int64)


def components(neighs, avail):
    """labels[k] = smallest index of k's component among the available points (-1: not available): a small union-find."""
    parent = list(range(len(neighs)))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    for u, ns in enumerate(neighs):
        if not avail[u]:
            continue
        for v in ns:
            if avail[v]:
                ru, rv = find(u), find(v)
                if ru != rv:
                    parent[max(ru, rv)] = min(ru, rv)
    return np.array([find(k) if avail[k] else -1 for k in range(len(neighs))], np.int32)


def cpu_arrays(ref, queries, wordlen, K_min, p_min, at_least_one=False):
    """What the device hands the host, from the oracles: rows, row offsets, neighbour counts (blot_oracle.find_all_neighbors
    per query), component labels (union-find over those lists, restricted to the available seeds) and a box counter
    (blot_oracle._seed_count in the in-memory classes' order)."""
    from biseqt_amd.blot import available_seeds_many, seed_ps_from_counts
    rows, off = oracle_rows(ref, queries, wordlen)
    d_radius, a_radius = radii(K_min)
    counts = np.zeros(len(rows), np.int32)
    neighs = [None] * len(rows)
    for q in range(len(queries)):
        pts = [(int(d), int(a)) for _, d, a in rows[off[q]:off[q + 1]]]
        for k, (_, ns) in enumerate(BO.find_all_neighbors(pts, d_radius, a_radius)):
            counts[off[q] + k] = len(ns)
            neighs[off[q] + k] = [int(off[q]) + v for v in ns]
    p = seed_ps_from_counts(counts, d_radius, a_radius, 4, wordlen)
    avail = available_seeds_many(p, p_min, off, at_least_one)
    labels = components(neighs, avail)

    def count_boxes(q, dmin, dmax, amin, amax):
        return np.array([BO._seed_count(ref.tolist(), queries[int(k)].tolist(), wordlen, 4, (), 'mutant',
                                        d_band=(int(d0), int(d1)), a_band=(int(a0), int(a1)))
                         for k, d0, d1, a0, a1 in zip(q, dmin, dmax, amin, amax)], np.int64)
    return dict(rows=rows, row_offsets=off, counts=counts, labels=labels, count_boxes=count_boxes,
                query_lens=np.array([len(t) for t in queries], np.int64), d_radius=d_radius, a_radius=a_radius)

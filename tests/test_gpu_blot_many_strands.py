"""WordBlotLocalRef.similar_segments_many(strands='-' / 'both') (k_qmatch_stranded of pw_qseeds.hip) against the per-query
GPU path on reverse complements materialised on the host -- segments, order, p and scores all ==, the comparison of
test_gpu_blot_many.py -- and against the CPU oracle with that file's tolerances.  Inputs: the mixed sets 'a' and 'b' of
tests/blot_many_cases.py with every odd-numbered query reverse-complemented (qseeds_strand_cases.flipped_mixed)."""
import numpy as np
import pytest

from biseqt_amd.sequence import reverse_complement
from tests import blot_many_cases as Cs, qseeds_strand_cases as SC
from tests.test_gpu_blot_many import _loc

pytestmark = pytest.mark.gpu
COMP = np.array(SC.COMP4, np.uint8)       # (a table: reverse_complement takes a list as mappings)
# queries with segments on '+', on '-', on both (from the CPU oracle: the inputs cannot drift)
CENSUS = {'a': (9, 9, 0), 'b': (12, 11, 5)}


def _strip(segs, strand):
    """The dicts without their 'strand', which must be ``strand`` on every one."""
    assert all(s['strand'] == strand for s in segs)
    return [{f: v for f, v in s.items() if f != 'strand'} for s in segs]


def _split(segs):
    """A 'both' list -> (plus part, minus part): plus first."""
    n = sum(s['strand'] == '+' for s in segs)
    return _strip(segs[:n], '+'), _strip(segs[n:], '-')


@pytest.mark.parametrize('name', ['a', 'b'])
def test_the_inputs_have_segments_on_both_strands(name):
    plus_only, minus_only, both = SC.strand_census(name)
    assert (plus_only + both, minus_only + both, both) == CENSUS[name]


@pytest.mark.parametrize('name', ['a', 'b'])
def test_minus_and_both_against_the_per_query_path_and_the_oracle(name):
    ref, queries, wordlen, K_min, p_min = SC.flipped_mixed(name)
    exp = SC.flipped_expected(name)
    loc = _loc(ref, wordlen)
    seqs = [Cs.mk(t) for t in queries]
    plus = loc.similar_segments_many(seqs, K_min, p_min)
    minus = loc.similar_segments_many(seqs, K_min, p_min, strands='-', complement=COMP)
    both = loc.similar_segments_many(seqs, K_min, p_min, strands='both', complement=[('A', 'T'), ('C', 'G')])
    assert loc._qidx.num_queries() == 2 * len(queries)                       # ONE build lists every query twice
    assert len(minus) == len(both) == len(queries)
    for q, T in enumerate(seqs):
        rcT = reverse_complement(T, COMP)
        assert rcT.as_array(np.uint8).tolist() == SC.rc(queries[q], SC.COMP4).tolist()
        per_query = list(loc.similar_segments(rcT, K_min, p_min))
        Cs.assert_identical(_strip(minus[q], '-'), per_query, q)
        Cs.assert_equals_oracle(minus[q], exp[q][1], q)
        # 'both' is the '+' result followed by the '-' result
        bp, bm = _split(both[q])
        assert [set(s) for s in both[q]] == [{'segment', 'p', 'scores', 'strand'}] * len(both[q])
        Cs.assert_identical(bp, plus[q], q)
        Cs.assert_identical(bm, _strip(minus[q], '-'), q)
        Cs.assert_equals_oracle(bp, exp[q][0], q)
        Cs.assert_equals_oracle(bm, exp[q][1], q)
    assert all('strand' not in s for segs in plus for s in segs)            # the default call's dicts are today's
    on_plus, on_minus = sum(bool(_split(b)[0]) for b in both), sum(bool(_split(b)[1]) for b in both)
    assert (on_plus, on_minus, sum(bool(_split(b)[0]) and bool(_split(b)[1]) for b in both)) == CENSUS[name]
    loc.close()


def test_at_least_one_applies_to_each_strand():
    ref, queries, wordlen, K_min, _ = SC.flipped_mixed('b')
    rows, off = Cs.oracle_rows(ref, queries + [SC.rc(t, SC.COMP4) for t in queries], wordlen)
    n = len(queries)
    qs = [t for k, t in enumerate(queries) if off[k + 1] > off[k] and off[n + k + 1] > off[n + k]]       # seeds on both strands
    assert len(qs) >= 15
    loc = _loc(ref, wordlen)
    seqs = [Cs.mk(t) for t in qs]
    got = loc.similar_segments_many(seqs, K_min, 1.5, at_least_one=True, strands='both', complement=COMP)
    for q, T in enumerate(seqs):
        bp, bm = _split(got[q])
        assert len(bp) == len(bm) == 1
        Cs.assert_identical(bp, list(loc.similar_segments(T, K_min, 1.5, at_least_one=True)), q)
        Cs.assert_identical(bm, list(loc.similar_segments(reverse_complement(T, COMP), K_min, 1.5, at_least_one=True)), q)
    loc.close()


def test_the_reference_and_its_reverse_complement_are_self_comparisons():
    """The list holds ref and rc(ref): (ref, '+') and (rc(ref), '-') equal the reference after their strand is applied and
    take the per-query path (mirrored points); (ref, '-') and (rc(ref), '+') are ordinary entries."""
    from biseqt_amd import synth
    rng = synth.rng_for(808)                 # (the repeat-carrying sequence of test_gpu_blot_many.test_queries_are_separate)
    unit = synth.rand_seqs(rng, 1, 300)[0]
    ref = np.concatenate([synth.rand_seqs(rng, 1, 400)[0], unit, synth.rand_seqs(rng, 1, 350)[0],
                          synth.mutate(rng, unit, .04, .02, .3), synth.rand_seqs(rng, 1, 200)[0]])
    t = np.concatenate([synth.rand_seqs(rng, 1, 30)[0], synth.mutate(rng, ref[300:800], .05, .03, .03)])
    loc = _loc(ref, 8)
    R, T = Cs.mk(ref), Cs.mk(t)
    rcR = reverse_complement(R, COMP)
    self_exp = list(loc.similar_segments(R, 200, .6))
    assert len(self_exp) >= 2 and loc.self_comp
    other = list(loc.similar_segments(rcR, 200, .6))
    assert not loc.self_comp
    both = loc.similar_segments_many([R, T, rcR], 200, .6, strands='both', complement=COMP)
    assert loc._qidx.num_queries() == 4                                     # six entries, two of them self comparisons
    (r_plus, r_minus), (t_plus, t_minus), (c_plus, c_minus) = [_split(b) for b in both]
    Cs.assert_identical(r_plus, self_exp, 'ref +')
    Cs.assert_identical(c_minus, self_exp, 'rc(ref) -')
    Cs.assert_identical(r_minus, other, 'ref -')
    Cs.assert_identical(c_plus, other, 'rc(ref) +')
    Cs.assert_identical(t_plus, list(loc.similar_segments(T, 200, .6)), 'query +')
    assert t_plus
    minus = loc.similar_segments_many([R, T, rcR], 200, .6, strands='-', complement=COMP)
    Cs.assert_identical(_strip(minus[2], '-'), self_exp, 'rc(ref) under -')
    Cs.assert_identical(_strip(minus[0], '-'), other, 'ref under -')
    loc.close()


def test_a_device_arena_is_read_in_place_for_both_strands():
    from biseqt_amd.batch import DeviceArena, pack_reads
    ref, queries, wordlen, K_min, p_min = SC.flipped_mixed('b')
    seqs = [Cs.mk(t) for t in queries]
    loc = _loc(ref, wordlen)
    host = loc.similar_segments_many(seqs, K_min, p_min, strands='both', complement=COMP)
    arena, offs, lens = pack_reads([ref] + queries)
    with DeviceArena(arena) as dev:
        got = loc.similar_segments_many(seqs, K_min, p_min, strands='both', complement=COMP, arena=(dev, offs[1:], lens[1:]))
        assert np.array_equal(dev.read(), arena)
    assert sum(len(g) for g in got) >= 20
    for q in range(len(seqs)):
        assert [s['strand'] for s in got[q]] == [s['strand'] for s in host[q]]
        Cs.assert_identical(got[q], host[q], q)
    loc.close()

"""WordBlotLocalRef.similar_segments_many (kernels K10 of pw_qseeds.hip) against the per-query GPU path -- segments, order,
p and scores all == -- and against the CPU oracle (segments ==, p within 1e-12 relative, scores rtol 1e-9: the tolerances
of test_blot_gpu.py, for the reason given there); the batched table's rows equal seeds_by_mutant per query exactly."""
import numpy as np
import pytest

from tests import blot_many_cases as Cs

pytestmark = pytest.mark.gpu
KW = dict(g_max=Cs.G_MAX, sensitivity=Cs.SENS, alphabet=Cs.A)


def _loc(ref, wordlen, **kw):
    from biseqt_amd.blot import WordBlotLocalRef
    return WordBlotLocalRef(Cs.mk(ref), wordlen=wordlen, **dict(KW, **kw))


def _check_rows(loc, ref, queries, wordlen):
    """The rows of the last batched build, per query, are seeds_by_mutant's (i, j) in its order."""
    from oracle import seeds_oracle as SO
    rows, off = loc._qidx.rows(), loc._qidx.row_offsets()
    assert len(off) == len(queries) + 1 and off[0] == 0 and off[-1] == len(rows)
    for q, t in enumerate(queries):
        r = rows[off[q]:off[q + 1]].astype(np.int64)
        assert (r[:, 0] == q).all()
        got = list(zip(((r[:, 2] + r[:, 1]) // 2).tolist(), ((r[:, 2] - r[:, 1]) // 2).tolist()))
        assert got == SO.seeds_by_mutant(ref.tolist(), t.tolist(), wordlen, 4), q


def _check_all(loc, ref, queries, wordlen, K_min, p_min, expected=None, at_least_one=False, rows=True):
    """One batched call against the loop over the per-query path (==) and the oracle (tolerances); returns the answer."""
    seqs = [Cs.mk(t) for t in queries]
    got = loc.similar_segments_many(seqs, K_min, p_min, at_least_one=at_least_one)
    assert len(got) == len(queries)
    if rows:
        _check_rows(loc, ref, queries, wordlen)
    for q, T in enumerate(seqs):
        Cs.assert_identical(got[q], list(loc.similar_segments(T, K_min, p_min, at_least_one=at_least_one)), q)
        exp = expected[q] if expected is not None else Cs.oracle_segments(ref, queries[q], wordlen, K_min, p_min, at_least_one)
        Cs.assert_equals_oracle(got[q], exp, q)
    return got


@pytest.mark.parametrize('name', ['a', 'b', 'c'])
def test_mixed_set_at_both_key_widths(name):
    """(a) wordlen 8 and (b) wordlen 6: 4-byte keys and the direct-address table; (c) wordlen 16: L^k = 2^32, the first
    8-byte key, binary searches."""
    ref, queries, wordlen, K_min, p_min = Cs.mixed_case(name)
    loc = _loc(ref, wordlen, allowed_memory=1 if wordlen < 12 else 200)
    got = _check_all(loc, ref, queries, wordlen, K_min, p_min, expected=Cs.mixed_expected(name))
    nseg = [len(g) for g in got]
    assert sum(n >= 1 for n in nseg) >= 20 and sum(n >= 2 for n in nseg) >= 5 and sum(n == 0 for n in nseg) >= 10, nseg
    assert all(got[q] == [] for q, t in enumerate(queries) if len(t) < wordlen)
    loc.close()
    assert loc._qidx is None


def test_arena_boundaries():
    """No k-mer straddles two queries that lie back to back in the arena: A ends with the first k - 1 letters of a word of
    the reference and B, directly behind it, starts with the rest.  Queries of k - 1, k, k + 1 letters; an empty first and
    an empty last query."""
    from biseqt_amd import synth
    from biseqt_amd.seeds import _QIndex
    k = 8
    rng = synth.rng_for(4711)
    ref = synth.rand_seqs(rng, 1, 600)[0]
    w = ref[100:100 + 2 * k - 2]
    qa = np.concatenate([synth.rand_seqs(rng, 1, 50)[0], w[:k - 1]])
    qb = np.concatenate([w[k - 1:], synth.rand_seqs(rng, 1, 50)[0]])
    queries = [np.zeros(0, np.uint8), qa, qb, ref[300:300 + k - 1], ref[320:320 + k], ref[340:340 + k + 1], np.zeros(0, np.uint8)]
    # packed with no gap at all between the queries: every k-mer that crosses a boundary is a word of the reference or
    # touches a neighbour's letters
    arena = np.concatenate(queries + [np.zeros(16, np.uint8)])
    lens = np.array([len(t) for t in queries], np.int32)
    offs = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
    assert (arena[offs[1] + 50:offs[1] + 50 + 2 * k - 2] == w).all()     # the straddling word IS there in the arena
    qi = _QIndex(ref, k, Cs.A)
    qi.build(arena, offs, lens)
    rows, off = qi.rows(), qi.row_offsets()
    from oracle import seeds_oracle as SO
    for q, t in enumerate(queries):
        r = rows[off[q]:off[q + 1]].astype(np.int64)
        got = list(zip(((r[:, 2] + r[:, 1]) // 2).tolist(), ((r[:, 2] - r[:, 1]) // 2).tolist()))
        assert got == SO.seeds_by_mutant(ref.tolist(), t.tolist(), k, 4), q
        assert all(j + k <= len(t) for _, j in got)
    assert off.tolist()[:2] == [0, 0] and off[-1] == off[-2] == len(rows)
    assert off[4] - off[3] == 0 and off[5] - off[4] >= 1 and off[6] - off[5] >= 2
    qi.close()
    # ... and through the class, in the padded arena of pack_reads
    loc = _loc(ref, k)
    _check_all(loc, ref, queries, k, 40, .7)
    loc.close()


def test_queries_are_separate():
    """The same query three times in one call, with the reference itself among the queries (the self-comparison route):
    the three answers equal one another and the single-query answer."""
    from biseqt_amd import synth
    rng = synth.rng_for(808)                 # (the repeat-carrying sequence of test_blot_gpu.test_self_similarity_vs_oracle)
    unit = synth.rand_seqs(rng, 1, 300)[0]
    ref = np.concatenate([synth.rand_seqs(rng, 1, 400)[0], unit, synth.rand_seqs(rng, 1, 350)[0],
                          synth.mutate(rng, unit, .04, .02, .3), synth.rand_seqs(rng, 1, 200)[0]])
    t = np.concatenate([synth.rand_seqs(rng, 1, 30)[0], synth.mutate(rng, ref[300:800], .05, .03, .03)])
    loc = _loc(ref, 8)
    T, R = Cs.mk(t), Cs.mk(ref)
    got = loc.similar_segments_many([T, R, T, T], 200, .6)
    single = list(loc.similar_segments(T, 200, .6))
    assert single
    for k in (0, 2, 3):
        Cs.assert_identical(got[k], single, k)
    self_exp = list(loc.similar_segments(R, 200, .6))
    assert len(self_exp) >= 2 and loc.self_comp
    Cs.assert_identical(got[1], self_exp, 'self')
    Cs.assert_equals_oracle(got[0], Cs.oracle_segments(ref, t, 8, 200, .6))
    loc.close()


def test_query_longer_than_reference():
    """Reference of 200 letters inside a query of 900: the diagonal offset is the query's length, and the clamps use it."""
    from biseqt_amd import synth
    rng = synth.rng_for(31)
    ref = synth.rand_seqs(rng, 1, 200)[0]
    t = np.concatenate([synth.rand_seqs(rng, 1, 350)[0], synth.mutate(rng, ref, .05, .03, .03), synth.rand_seqs(rng, 1, 350)[0]])[:900]
    short = synth.mutate(rng, ref[20:150], .05, .03, .03)
    loc = _loc(ref, 6)
    got = _check_all(loc, ref, [short, t, short], 6, 60, .7)
    assert got[1] and got[0] and got[1][0]['segment'][0][0] < -300
    loc.close()


def test_more_queries_than_any_grouping():
    """300 queries (60-120 letters) against a reference of 1000: more queries than a workgroup has threads or the
    box counter has wavefronts per workgroup, so every kernel's indexing by query runs over several workgroups."""
    from biseqt_amd import synth
    rng = synth.rng_for(300)
    ref = synth.rand_seqs(rng, 1, 1000)[0]
    queries = []
    for k in range(300):
        ln = int(rng.integers(60, 121))
        if k % 3 == 0:
            queries.append(synth.rand_seqs(rng, 1, ln)[0])
        else:
            at = int(rng.integers(0, 1000 - ln))
            queries.append(synth.mutate(rng, ref[at:at + ln], .05, .03, .03))
    loc = _loc(ref, 6)
    got = _check_all(loc, ref, queries, 6, 40, .7)
    assert sum(bool(g) for g in got) >= 150
    loc.close()


def test_low_complexity_and_the_row_limit():
    """A two-letter periodic reference: dense k-mer runs.  With a max_rows that the table exceeds the build returns the
    error -- it neither wraps nor truncates."""
    from biseqt_amd.seeds import _QIndex
    from biseqt_amd.batch import pack_reads
    ref = np.array(([0, 1] * 200), np.uint8)
    queries = [np.array(([0, 1] * 50) if q % 2 == 0 else ([1, 0] * 50), np.uint8) for q in range(8)]
    queries[3] = np.array([0, 1, 1, 0] * 25, np.uint8)
    loc = _loc(ref, 4)
    # (K_min 10: the oracle walks every neighbour list in python, and here a list grows with the square of the radius)
    exp, cache = [], {}
    for t in queries:
        if t.tobytes() not in cache:
            cache[t.tobytes()] = Cs.oracle_segments(ref, t, 4, 10, .7)
        exp.append(cache[t.tobytes()])
    assert sum(bool(e) for e in exp) == 7
    _check_all(loc, ref, queries, 4, 10, .7, expected=exp)
    nrows = loc._qidx.num_rows()
    assert nrows > 8 * 97 * 50
    loc.close()
    arena, offs, lens = pack_reads(queries)
    qi = _QIndex(ref, 4, Cs.A)
    with pytest.raises(RuntimeError, match='would hold %d rows' % nrows):
        qi.build(arena, offs, lens, max_rows=nrows - 1)
    assert qi.num_rows() == -1
    with pytest.raises(RuntimeError):
        qi.rows()
    assert qi.build(arena, offs, lens, max_rows=nrows) == nrows          # the limit itself is allowed
    qi.close()
    with pytest.raises(RuntimeError, match='would hold'):
        _loc(ref, 4, max_rows=1000).similar_segments_many([Cs.mk(t) for t in queries], 10, .7)


def test_at_least_one():
    """p_min = 1.5 passes no seed: every query yields one segment, grown from its first maximum in presentation order;
    a query without seeds raises what the per-query call raises."""
    ref, queries, wordlen, K_min, _ = Cs.mixed_case('b')
    rows, off = Cs.oracle_rows(ref, queries, wordlen)
    qs = [t for k, t in enumerate(queries) if off[k + 1] > off[k]]
    assert len(qs) >= 25
    loc = _loc(ref, wordlen)
    got = _check_all(loc, ref, qs, wordlen, K_min, 1.5, at_least_one=True, rows=False)
    assert all(len(g) == 1 for g in got)
    from oracle import seeds_oracle as SO
    present = set(SO.as_kmer_seq(ref.tolist(), wordlen, 4))
    absent = next(v for v in range(4 ** wordlen) if v not in present)     # a whole word, and still no seed
    seedless = np.array([(absent // 4 ** (wordlen - 1 - i)) % 4 for i in range(wordlen)], np.uint8)
    with pytest.raises(AssertionError, match='no seeds found while at_least_one=True'):
        loc.similar_segments_many([Cs.mk(qs[0]), Cs.mk(seedless)], K_min, 1.5, at_least_one=True)
    with pytest.raises(AssertionError, match='no seeds found while at_least_one=True'):
        list(loc.similar_segments(Cs.mk(seedless), K_min, 1.5, at_least_one=True))
    loc.close()


def test_graph_is_the_oracles_per_query():
    """Neighbour lists of the batched graph: per query the KD-tree's, shifted by the query's first row; none crosses."""
    from biseqt_amd.batch import pack_reads
    from biseqt_amd.seeds import _QIndex
    from oracle import blot_oracle as BO
    ref, queries, wordlen, K_min, _ = Cs.mixed_case('a')
    queries = queries[:15]
    qi = _QIndex(ref, wordlen, Cs.A)
    qi.build(*pack_reads(queries))
    d_radius, a_radius = Cs.radii(K_min)
    edges = qi.graph_build(1. * a_radius / d_radius, a_radius)
    rows, roff = qi.rows(), qi.row_offsets()
    goff, adj = qi.graph_fetch()
    counts = qi.graph_counts()
    assert goff[-1] == edges == counts.sum() and (np.diff(goff) == counts).all()
    neighs = [None] * len(rows)
    for q in range(len(queries)):
        pts = [(int(d), int(a)) for _, d, a in rows[roff[q]:roff[q + 1]]]
        for k, (_, ns) in enumerate(BO.find_all_neighbors(pts, d_radius, a_radius)):
            o = roff[q] + k
            neighs[o] = sorted(int(roff[q]) + v for v in ns)
            assert sorted(adj[goff[o]:goff[o + 1]].tolist()) == neighs[o], (q, k)
    assert edges > 0
    # ... and the components of that graph, every row available and a random half of them
    for avail in (np.ones(len(rows), bool), np.random.default_rng(15).random(len(rows)) < .5):
        assert np.array_equal(qi.graph_components(avail), Cs.components(neighs, avail.tolist()))
    qi.close()

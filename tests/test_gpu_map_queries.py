"""pipeline.map_queries -- all queries' segments from one pass, the kept ones aligned in one banded local batch -- against
the C oracle (= the compiled reference): every kept segment's alignment equals oracle.solve on (ref, query) inside the
segment's diagonal range in score, transcript and start indices."""
import pytest

from tests import blot_many_cases as Cs

pytestmark = pytest.mark.gpu


def test_map_queries_vs_oracle(oracle):
    from biseqt_amd.blot import WordBlotLocalRef
    from biseqt_amd.pipeline import map_queries
    ref, queries, wordlen, K_min, p_min = Cs.mixed_case('a', 30)
    R, Q = Cs.mk(ref), [Cs.mk(t) for t in queries]
    keep = 3
    got = map_queries(R, Q, K_min, p_min, wordlen, Cs.G_MAX, Cs.SENS, keep=keep)
    assert len(got) == len(queries)
    # the segments are those of the per-query path, ranked by p * (a_max - a_min), the best `keep` kept
    loc = WordBlotLocalRef(R, wordlen=wordlen, alphabet=Cs.A, g_max=Cs.G_MAX, sensitivity=Cs.SENS)
    good = aligned = 0
    for q, recs in enumerate(got):
        segs = list(loc.similar_segments(Q[q], K_min, p_min))
        ranked = sorted(segs, key=lambda rec: -(rec['p'] * (rec['segment'][1][1] - rec['segment'][1][0])))[:keep]
        assert [(r['segment'], r['p']) for r in recs] == [(r['segment'], r['p']) for r in ranked], q
        for rec in recs:
            d_band = rec['segment'][0]
            assert rec['diag_range'] == (int(d_band[0]), int(d_band[1]))
            r = oracle.solve(ref, queries[q], L=4, mode=1, alntype=1, diag_range=rec['diag_range'], match=1, mismatch=-3, go=-5,
                             ge=-2)
            if r['init_rc'] != 0 or r['opt'][0] == -1 or r['would_panick'] or r['tb_null'] or not r['transcript']:
                assert rec['alignment'] is None and rec['score'] is None and rec['p_aln'] is None
                continue
            aln = rec['alignment']
            assert aln is not None, (q, rec)
            assert rec['score'] == r['score'] and aln.transcript == r['transcript']
            assert (aln.origin_start, aln.mutant_start) == (r['origin_idx'], r['mutant_idx'])
            tx = r['transcript']
            on_query = sum(tx.count(op) for op in 'MSI')
            assert rec['len_aln'] == on_query and rec['p_aln'] == round(1. * tx.count('M') / on_query, 2)
            aligned += 1
            good += rec['p_aln'] >= .8
    loc.close()
    assert good >= 20, (good, aligned)
    assert sum(len(recs) == 0 for recs in got) >= 8 and max(len(recs) for recs in got) >= 2

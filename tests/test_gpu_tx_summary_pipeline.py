"""The pipeline functions with the transcripts left on the device (``alignments=False`` / ``want_summaries=True``): what
they report from the device-side summaries equals what the default path computes from the transcript strings."""
import numpy as np
import pytest

from tests import blot_many_cases as Cs
from tests import tx_summary_ref as R

pytestmark = pytest.mark.gpu


def test_map_queries_without_alignments():
    from biseqt_amd.pipeline import map_queries
    ref, queries, wordlen, K_min, p_min = Cs.mixed_case('a', 30)
    Rf, Q = Cs.mk(ref), [Cs.mk(t) for t in queries]
    full = map_queries(Rf, Q, K_min, p_min, wordlen, Cs.G_MAX, Cs.SENS, keep=3)
    lean = map_queries(Rf, Q, K_min, p_min, wordlen, Cs.G_MAX, Cs.SENS, keep=3, alignments=False)
    assert len(full) == len(lean) == len(queries)
    aligned = 0
    for q, (fr, lr) in enumerate(zip(full, lean)):
        assert len(fr) == len(lr), q
        for f, l in zip(fr, lr):
            assert set(l) == set(f) | {'origin_start', 'mutant_start', 'summary'}
            for key in ('segment', 'p', 'diag_range', 'score', 'p_aln', 'len_aln'):
                assert f[key] == l[key], (q, key, f[key], l[key])
            assert l['alignment'] is None
            if f['alignment'] is None:
                assert l['summary'] is None and l['origin_start'] is None and l['mutant_start'] is None
                continue
            assert (l['origin_start'], l['mutant_start']) == (f['alignment'].origin_start, f['alignment'].mutant_start)
            assert tuple(l['summary'][k] for k in R.FIELDS) == R.summarize(f['alignment'].transcript), (q, f['alignment'].transcript)
            aligned += 1
    assert aligned >= 20


def test_extend_segments_without_alignments():
    """The planted-homology pair of tests/test_pipeline_gpu.py."""
    from biseqt_amd import synth
    from biseqt_amd.blot import WordBlot
    from biseqt_amd.pipeline import extend_segments
    from biseqt_amd.pw import Alignment
    from biseqt_amd.sequence import Alphabet, Sequence
    A = Alphabet('ACGT')
    rng = synth.rng_for(55)
    n = 30000
    s = synth.rand_seqs(rng, 1, n)[0]
    t = synth.rand_seqs(rng, 1, n)[0]
    for q in range(6):
        ln = int(rng.integers(600, 2500))
        a, b = int(rng.integers(0, n - ln)), q * (n // 6) + int(rng.integers(0, 500))
        seg = synth.mutate(rng, s[a:a + ln], .06, .02, .3)
        seg = seg[:min(len(seg), n - b)]
        t[b:b + len(seg)] = seg
    S, T = Sequence(A, tuple(s.tolist())), Sequence(A, tuple(t.tolist()))
    K_min, p_min, wordlen = 400, .8, 10
    wb = WordBlot(S, T, g_max=.1, sensitivity=.99, alphabet=A, wordlen=wordlen, mask=[])
    try:
        segments = list(wb.similar_segments(K_min, p_min))
    finally:
        wb.close()
    kw = dict(match_score=1. / p_min - 1, mismatch_score=-1, ge_score=-1, go_score=0)
    full = extend_segments(S, T, segments, wordlen, **kw)
    lean = extend_segments(S, T, segments, wordlen, alignments=False, **kw)
    assert len(full) == len(lean) == len(segments) >= 6
    framed = 0
    for f, l in zip(full, lean):
        assert set(l) == set(f) | {'summary', 'truncated_frame'}
        for key in ('frame', 'diag_range', 'score', 'kernel'):
            assert f[key] == l[key], key
        assert l['alignment'] is None and l['truncated'] is None
        tr = f['truncated']
        assert (l['truncated_frame'] is None) == (tr is None)
        if f['alignment'] is not None:
            assert tuple(l['summary'][k] for k in R.FIELDS) == R.summarize(f['alignment'].transcript)
        if tr is None:
            continue
        assert l['truncated_frame'] == ((tr.origin_start, tr.origin_start + Alignment.projected_len(tr.transcript, on='origin')),
                                        (tr.mutant_start, tr.mutant_start + Alignment.projected_len(tr.transcript, on='mutant')))
        framed += 1
    assert framed >= 6


def test_overlap_alignments_with_summaries():
    from biseqt_amd import synth
    from biseqt_amd.overlap import overlap_alignments
    from biseqt_amd.sequence import Alphabet
    A = Alphabet('ACGT')
    rng = synth.rng_for(4831)
    genome = synth.rand_seqs(rng, 1, 4000)[0]
    reads, starts = [], []
    for k in range(30):
        a = int(rng.integers(0, 3200))
        reads.append(synth.mutate(rng, genome[a:a + 800], .03, .01, .3))
        starts.append(a)
    pairs, bands = [], []
    for i in range(30):
        for j in range(i + 1, 30):
            if abs(starts[i] - starts[j]) < 500:
                d = starts[j] - starts[i]
                pairs.append((i, j)); bands.append(dict(p=1., d_band=(d - 40, d + 40)))
    assert len(pairs) >= 20
    with_tx = overlap_alignments(reads, pairs, bands, A, want_transcripts=True)
    lean = overlap_alignments(reads, pairs, bands, A, want_transcripts=False, want_summaries=True)
    both = overlap_alignments(reads, pairs, bands, A, want_transcripts=True, want_summaries=True)
    assert all('summary' not in r for r in with_tx if r is not None)
    n = 0
    for f, l, bo in zip(with_tx, lean, both):
        assert (f is None) == (l is None) == (bo is None)
        if f is None:
            continue
        assert l['transcript'] is None and bo['transcript'] == f['transcript']
        for key in ('score', 'origin_start', 'mutant_start', 'diag_range'):
            assert f[key] == l[key] == bo[key]
        assert tuple(l['summary'][k] for k in R.FIELDS) == R.summarize(f['transcript']) == tuple(bo['summary'][k] for k in R.FIELDS)
        n += f['transcript'] is not None
    assert n >= 20

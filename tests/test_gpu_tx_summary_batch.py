"""The alignment summaries of a batch (``BatchAligner.summarize`` / ``summaries``; include/pw_txsum.h) against the
pure-Python oracle of tests/tx_summary_ref.py applied to ``b.transcripts(res)`` of the same batch: all 12 fields equal for
every pair.  A pair whose record carries PW_ST_EMPTY, PW_ST_PANICK or PW_ST_BADPATH, or no PW_ST_TRACED, has the record of
a pair without a transcript, as the header states -- this includes the all-gap alignments from cell (0, 0) (X == 0 or
Y == 0 under a global type), which the batch reports with PW_ST_PANICK beside their all-I / all-D transcript."""
import numpy as np
import pytest

from tests import tx_summary_ref as R
from tests.helpers import dec, kw_of, load_golden

pytestmark = pytest.mark.gpu

LOCAL_BANDED = dict(alnmode=1, alntype=1, diag_range=(-25, 25), match_score=1, mismatch_score=-3, go_score=-5, ge_score=-2)
GLOBAL_BANDED = dict(alnmode=1, alntype=0, diag_range=(-6, 6), match_score=1, mismatch_score=-1, go_score=0, ge_score=-1)
LOCAL_STD = dict(alnmode=0, alntype=1, match_score=2, mismatch_score=-3, go_score=-4, ge_score=-1)


def _expected(res, txs):
    return [R.summarize(t, int(st)) for t, st in zip(txs, res['status'])]


def _check(b, res=None, what=''):
    res = b.results() if res is None else res
    txs = b.transcripts(res)
    sums = b.summaries()
    R.assert_equal(sums, _expected(res, txs), what)
    for k, t in enumerate(txs):
        if t is None:
            assert sums['flags'][k] == 0 and sums['first_match'][k] == -1 and sums['last_match'][k] == -1, (what, k)
    return res, txs, sums


@pytest.fixture(scope='module')
def ragged_pairs():
    """The 700 ragged pairs of tests/test_gpu_packed_transcripts.py: lengths 0 .. 500, every fourth with nothing in common."""
    from biseqt_amd import synth
    rng = synth.rng_for(3601)
    pairs = []
    for k in range(700):
        n = int(rng.integers(0, 500)) if k % 9 else int(rng.integers(0, 3))
        o = synth.rand_seqs(rng, 1, n)[0]
        if k % 4 == 0:
            m = ((o + 2) % 4)[: max(0, n - int(rng.integers(0, 5)))].astype(np.uint8) if n else synth.rand_seqs(rng, 1, 3)[0]
        else:
            m = synth.mutate(rng, o, 0.06, 0.03, 0.4)
        pairs.append((o, m))
    return pairs


@pytest.mark.parametrize('kw', [LOCAL_BANDED, GLOBAL_BANDED, LOCAL_STD], ids=['banded-local', 'banded-global', 'standard-local'])
def test_summaries_equal_the_oracle_on_ragged_batches(ragged_pairs, kw):
    from biseqt_amd.batch import BatchAligner
    with BatchAligner(ragged_pairs, alphabet_len=4, check_band=False, **kw) as b:
        res = b.run()
        b.summarize()
        res, txs, sums = _check(b, res, 'first run')
        if kw is GLOBAL_BANDED:
            assert any(b.init_rc(k) != 0 for k in range(len(ragged_pairs)))
        assert any(t is None for t in txs) and any(t for t in txs)
        assert (sums['flags'] == 0).any() and (sums['flags'] == 1).any()
        res2 = b.run()                                   # the same batch again: the same records
        b.summarize()
        sums2 = b.summaries()
        assert (res2 == res).all() and (sums2 == sums).all()
        _check(b, res2, 'second run')


def test_transcripts_without_a_match_and_of_one_gap_letter():
    from biseqt_amd import _pwlib as W
    from biseqt_amd import synth
    from biseqt_amd.batch import BatchAligner
    rng = synth.rng_for(4821)
    pairs = []
    for k in range(40):
        o = (synth.rand_seqs(rng, 1, 1 + k * 7)[0] % 2).astype(np.uint8)      # letters 0, 1 against 2, 3: no letter in common
        pairs.append((o, ((o + 2) % 4).astype(np.uint8)))
    empty = np.zeros(0, np.uint8)
    pairs += [(empty, synth.rand_seqs(rng, 1, n)[0]) for n in (1, 5, 70)] + [(synth.rand_seqs(rng, 1, n)[0], empty) for n in (1, 5, 70)]
    with BatchAligner(pairs, alnmode=0, alntype=0, alphabet_len=4, match_score=1, mismatch_score=-1, go_score=-5, ge_score=-2) as b:
        res = b.run()
        res, txs, sums = _check(b, res, 'global, nothing in common')
        for k in range(40):                              # a transcript without an M: counted, no match bounds, no head / tail
            assert txs[k] == 'S' * (1 + k * 7)
            assert R.as_tuples(sums[k:k + 1])[0] == (0, 1 + k * 7, 0, 0, 0, -1, -1, 0, 0, 0, 0, 1)
        # X == 0 / Y == 0: all-I / all-D transcripts, all gaps from cell (0, 0): PW_ST_PANICK, so not summarised
        assert [txs[k] for k in range(40, 46)] == ['I', 'I' * 5, 'I' * 70, 'D', 'D' * 5, 'D' * 70]
        assert all(res['status'][k] & W.PW_ST_PANICK for k in range(40, 46))
        assert (sums['flags'][40:] == 0).all()
    # ... and the same strings through the packed entry point, where no status excludes them
    from biseqt_amd.batch import summarize_transcripts
    R.assert_equal(summarize_transcripts(txs[40:]), [R.summarize(t) for t in txs[40:]], 'one gap letter')


def test_summarize_needs_a_traceback_and_follows_the_latest_one():
    from biseqt_amd import synth
    from biseqt_amd.batch import BatchAligner, PinnedArray, SUMMARY_DTYPE
    origins, mutants = synth.pair_batch(12, 300, 280)
    with BatchAligner(list(zip(origins, mutants)), **LOCAL_BANDED, alphabet_len=4) as b:
        with pytest.raises(RuntimeError, match='before a traceback'):
            b.summarize()
        with pytest.raises(RuntimeError, match='before a traceback'):
            b.summaries()
        b.solve()
        with pytest.raises(RuntimeError, match='before a traceback'):
            b.summarize()
        pin = PinnedArray(48 * b.n, SUMMARY_DTYPE)
        with pytest.raises(RuntimeError, match='before pw_batch_summarize'):
            b.summaries_async(pin)
        b.traceback(); b.summarize(); b.summaries_async(pin); b.sync()
        res, txs, sums = _check(b, None, 'after the first traceback')
        assert (pin.array == sums).all() and (sums['flags'] == 1).all()
        pin.close()


def test_summaries_after_traceback_from_explicit_ends():
    """The standard-mode case of tests/test_explicit_ends.py: one problem, every recorded end cell a pair of the batch.  The
    summaries taken after run() are stale after traceback_from; summaries() takes them again."""
    from biseqt_amd.batch import BatchAligner
    recs = [r for r in load_golden('explicit_ends.json.gz') if r['kw']['mode'] == 0 and 'origin_range' not in r['kw']][:8]
    assert len({r['kw']['alntype'] for r in recs}) >= 3
    checked = 0
    for rec in recs:
        kw = kw_of(rec)
        ends = [e['end'] for e in rec['ends']]
        o, m = np.array(dec(rec['origin']), np.uint8), np.array(dec(rec['mutant']), np.uint8)
        with BatchAligner([(o, m)] * len(ends), alnmode=0, alntype=kw['alntype'], alphabet_len=4, subst_scores=kw['subst'],
                          go_score=kw['go'], ge_score=kw['ge']) as b:
            res = b.run()
            b.summarize()
            _, txs0, sums0 = _check(b, res, 'optimal end')
            b.traceback_from(ends)
            b.sync()
            res, txs, sums = _check(b, None, 'explicit ends')
            want = {tuple(e['end']): e['transcript'] for e in rec['ends'] if 'transcript' in e}
            for k, e in enumerate(ends):
                if tuple(e) in want:
                    assert txs[k] == want[tuple(e)]
                    checked += 1
            assert txs != txs0 and not (sums == sums0).all()
    assert checked >= 15


def test_summaries_of_a_strip_pipeline_batch():
    from biseqt_amd import _pwlib as W
    from biseqt_amd import synth
    from biseqt_amd.batch import BatchAligner
    rng = synth.rng_for(3602)
    pairs = []
    for n in (6000, 300, 1200):
        o = synth.rand_seqs(rng, 1, n)[0]
        pairs.append((o, synth.mutate(rng, o, 0.08, 0.04, 0.3)))
    with BatchAligner(pairs, alnmode=0, alntype=0, alphabet_len=4, match_score=1, mismatch_score=-3, go_score=-5, ge_score=-2,
                      flags=W.PW_FLAG_FORCE_STRIP) as b:
        res = b.run()
        res, txs, sums = _check(b, res, 'strip pipeline')
        assert len(txs[0]) >= 6000 and (sums['flags'] == 1).all()


def test_summaries_on_minus_strand_frames():
    """20 read pairs, every other one against the reverse complement of its mutant: rc frames in a shared device arena."""
    from biseqt_amd import synth
    from biseqt_amd.batch import pack_reads
    from biseqt_amd.overlap import aligned_batches
    rng = synth.rng_for(4822)
    comp = np.array([3, 2, 1, 0], np.uint8)
    reads, pidx, strands = [], [], []
    for k in range(20):
        o = synth.rand_seqs(rng, 1, 200 + 11 * k)[0]
        m = synth.mutate(rng, o, 0.05, 0.03, 0.3)
        minus = k % 2 == 1
        reads += [o, comp[m][::-1].copy() if minus else m]
        pidx.append((2 * k, 2 * k + 1)); strands.append('-' if minus else '+')
    arena, offs, lens = pack_reads(reads)
    dr = [(-30, 30)] * len(pidx)
    n = 0
    for lo, hi, b in aligned_batches(arena, offs, lens, pidx, dr, 4, strands=strands, complement=comp, match_score=1,
                                     mismatch_score=-3, go_score=-5, ge_score=-2):
        res, txs, sums = _check(b, None, 'strands')
        assert (sums['flags'] == 1).all() and (sums['n_match'] >= 150).all()
        n += hi - lo
    assert n == 20

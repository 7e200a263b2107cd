"""The CIGARs of a batch (``BatchAligner.cigars``; include/pw_cigar.h) against the ``itertools.groupby`` oracle of
tests/cigar_ref.py applied to ``b.transcripts(res)`` of the same batch, in both forms: for every alignment type, for pairs
without an alignment (PW_ST_EMPTY, PW_ST_PANICK: zero runs), through the strip pipeline, after a traceback from other end
cells and after a change of form."""
import numpy as np
import pytest

from tests import cigar_ref as R
from tests.helpers import dec, kw_of, load_golden

pytestmark = pytest.mark.gpu

SCORES = dict(match_score=1, mismatch_score=-3, go_score=-5, ge_score=-2)


def _check(b, res=None, what='', forms=R.FORMS):
    res = b.results() if res is None else res
    txs = b.transcripts(res)
    for name, form in forms:
        runs, off = b.cigars(name)
        R.assert_equal((runs, off), txs, form, '%s, %s' % (what, name), res['status'])
        assert int(off[-1]) == len(runs)
        lens = np.add.reduceat(np.append(runs >> 4, 0).astype(np.int64), off[:-1].astype(np.int64)) * (np.diff(off.astype(np.int64)) > 0)
        want = [int(n) if R.runs(t, form, int(st)) else 0 for t, n, st in zip(txs, res['tx_len'], res['status'])]
        assert lens.tolist() == want, (what, name)
        d_runs, d_off = b.cigars_device()
        assert d_runs.ptr and d_off.ptr and d_runs.nbytes == 4 * len(runs) and d_off.nbytes == 8 * (b.n + 1)
    return res, txs


@pytest.fixture(scope='module')
def pairs():
    """40 pairs of 30 .. 300 letters: mutated copies, and every eighth pair with no letter in common."""
    from biseqt_amd import synth
    rng = synth.rng_for(4921)
    out = []
    for k in range(40):
        n = int(rng.integers(30, 301))
        o = synth.rand_seqs(rng, 1, n)[0]
        if k % 8 == 7:
            o = (o % 2).astype(np.uint8)
            out.append((o, ((o + 2) % 4)[:max(30, n - int(rng.integers(0, 9)))].astype(np.uint8)))
        else:
            out.append((o, synth.mutate(rng, o, 0.08, 0.04, 0.4)))
    return out


@pytest.mark.parametrize('alntype', range(7))
def test_standard_types(pairs, alntype):
    from biseqt_amd import _pwlib as W
    from biseqt_amd.batch import BatchAligner
    with BatchAligner(pairs, alnmode=0, alntype=alntype, alphabet_len=4, **SCORES) as b:
        res, txs = _check(b, b.run(), 'standard type %d' % alntype)
        assert sum(1 for t in txs if t) >= 20
        if alntype == W.LOCAL:                          # nothing in common under LOCAL: no alignment (an empty traceback, or
            _, off = b.cigars()                         # no end cell to trace from), zero runs
            for k in range(7, 40, 8):
                st = int(res['status'][k])
                assert txs[k] is None and res['tx_len'][k] <= 0 and off[k] == off[k + 1], (k, st, txs[k])
                assert st & W.PW_ST_EMPTY or not st & W.PW_ST_TRACED, (k, st)


@pytest.mark.parametrize('alntype', range(3))
def test_banded_types(pairs, alntype):
    from biseqt_amd.batch import BatchAligner
    with BatchAligner(pairs, alnmode=1, alntype=alntype, alphabet_len=4, diag_range=(-25, 25), check_band=False, **SCORES) as b:
        res, txs = _check(b, b.run(), 'banded type %d' % alntype)
        assert sum(1 for t in txs if t) >= 20


def test_all_gap_alignments_from_the_corner_have_no_runs():
    """X == 0 (or Y == 0) under GLOBAL: the batch reports PW_ST_PANICK beside the all-I / all-D transcript -- no summary, so
    no runs; the same strings through the stand-alone entry point, where no status excludes them, have one."""
    from biseqt_amd import _pwlib as W
    from biseqt_amd import synth
    from biseqt_amd.batch import BatchAligner, cigar_strings, cigars_of_transcripts
    rng = synth.rng_for(4922)
    empty = np.zeros(0, np.uint8)
    o = synth.rand_seqs(rng, 1, 50)[0]
    pairs = [(empty, synth.rand_seqs(rng, 1, n)[0]) for n in (1, 5, 70)] + [(synth.rand_seqs(rng, 1, n)[0], empty) for n in (1, 5, 70)] + [(o, o)]
    with BatchAligner(pairs, alnmode=0, alntype=0, alphabet_len=4, **SCORES) as b:
        res, txs = _check(b, b.run(), 'X == 0 / Y == 0')
        assert txs == ['I', 'I' * 5, 'I' * 70, 'D', 'D' * 5, 'D' * 70, 'M' * 50]
        assert all(res['status'][k] & W.PW_ST_PANICK for k in range(6))
        assert cigar_strings(*b.cigars()) == [''] * 6 + ['50=']
        assert cigar_strings(*b.cigars('classic')) == [''] * 6 + ['50M']
    assert cigar_strings(*cigars_of_transcripts(txs)) == ['1I', '5I', '70I', '1D', '5D', '70D', '50=']


def test_strip_pipeline_batch():
    from biseqt_amd import _pwlib as W
    from biseqt_amd import synth
    from biseqt_amd.batch import BatchAligner
    rng = synth.rng_for(4923)
    pairs = []
    for n in (6000, 300, 1200):
        o = synth.rand_seqs(rng, 1, n)[0]
        pairs.append((o, synth.mutate(rng, o, 0.08, 0.04, 0.3)))
    with BatchAligner(pairs, alnmode=0, alntype=0, alphabet_len=4, flags=W.PW_FLAG_FORCE_STRIP, **SCORES) as b:
        res, txs = _check(b, b.run(), 'strip pipeline')
        assert len(txs[0]) >= 6000


def test_cigars_need_a_traceback_and_a_known_form():
    from biseqt_amd import _pwlib as W
    from biseqt_amd import synth
    from biseqt_amd.batch import BatchAligner
    origins, mutants = synth.pair_batch(12, 300, 280)
    with BatchAligner(list(zip(origins, mutants)), alnmode=1, alntype=1, diag_range=(-25, 25), alphabet_len=4, **SCORES) as b:
        with pytest.raises(RuntimeError, match='before a traceback'):
            b.cigars()
        with pytest.raises(RuntimeError, match='before cigars'):
            b.cigars_device()
        b.solve()
        with pytest.raises(RuntimeError, match='before a traceback'):
            b.cigars('classic')
        off = np.zeros(b.n + 1, np.uint64)
        assert b.lib.pw_batch_cigar(b.handle, 0, None, 0, off.ctypes.data) == -1 and 'before a traceback' in W.last_error()
        b.traceback()
        b.sync()
        with pytest.raises(ValueError):
            b.cigars('bam')
        assert b.lib.pw_batch_cigars(b.handle, 2, None) == -1 and 'unknown form' in W.last_error()
        assert b.lib.pw_batch_cigar(b.handle, -1, None, 0, off.ctypes.data) == -1 and 'unknown form' in W.last_error()
        assert not b.lib.pw_batch_cigar_runs_device(b.handle) and not b.lib.pw_batch_cigar_offsets_device(b.handle)
        # the synchronous reader runs the kernels itself; too little room fails and writes nothing
        assert b.lib.pw_batch_cigar(b.handle, 0, None, 0, off.ctypes.data) == 0
        assert b.lib.pw_batch_cigar_runs_device(b.handle) and b.lib.pw_batch_cigar_offsets_device(b.handle)
        total = int(off[-1])
        assert total >= b.n
        runs = np.full(total, 0xabcdef01, np.uint32)
        off2 = np.full(b.n + 1, 77, np.uint64)
        assert b.lib.pw_batch_cigar(b.handle, 0, runs.ctypes.data, total - 1, off2.ctypes.data) == -1 and 'too small' in W.last_error()
        assert (runs == 0xabcdef01).all() and (off2 == 77).all()
        assert b.lib.pw_batch_cigar(b.handle, 0, runs.ctypes.data, total, None) == 0
        R.assert_equal((runs, off), b.transcripts(), R.EXTENDED, 'synchronous reader')
        _check(b, None, 'after the traceback')


def test_a_change_of_form_runs_the_kernels_again():
    from biseqt_amd import synth
    from biseqt_amd.batch import BatchAligner
    origins, mutants = synth.pair_batch(20, 200, 281)
    with BatchAligner(list(zip(origins, mutants)), alnmode=1, alntype=0, diag_range=(-25, 25), alphabet_len=4, **SCORES) as b:
        res = b.run()
        txs = b.transcripts(res)
        assert any('S' in t for t in txs if t)
        ext = b.cigars('extended')
        off = np.zeros(b.n + 1, np.uint64)
        # the synchronous reader with the other form: the stored runs are of the wrong form, so it encodes again
        assert b.lib.pw_batch_cigar(b.handle, 1, None, 0, off.ctypes.data) == 0
        runs = np.zeros(int(off[-1]), np.uint32)
        assert b.lib.pw_batch_cigar(b.handle, 1, runs.ctypes.data, len(runs), None) == 0
        R.assert_equal((runs, off), txs, R.CLASSIC, 'classic behind extended')
        assert len(runs) < len(ext[0])
        again = b.cigars('extended')
        assert (again[0] == ext[0]).all() and (again[1] == ext[1]).all()
        R.assert_equal(again, txs, R.EXTENDED, 'extended again')


def test_cigars_after_traceback_from_explicit_ends():
    """The standard-mode case of tests/test_explicit_ends.py: one problem, every recorded end cell a pair of the batch.  The
    runs taken after run() are stale after traceback_from; the synchronous reader takes them again."""
    from biseqt_amd.batch import BatchAligner, cigar_strings
    recs = [r for r in load_golden('explicit_ends.json.gz') if r['kw']['mode'] == 0 and 'origin_range' not in r['kw']][:4]
    for rec in recs:
        kw = kw_of(rec)
        ends = [e['end'] for e in rec['ends']]
        o, m = np.array(dec(rec['origin']), np.uint8), np.array(dec(rec['mutant']), np.uint8)
        with BatchAligner([(o, m)] * len(ends), alnmode=0, alntype=kw['alntype'], alphabet_len=4, subst_scores=kw['subst'],
                          go_score=kw['go'], ge_score=kw['ge']) as b:
            res, txs0 = _check(b, b.run(), 'optimal end')
            before = b.cigars()
            b.traceback_from(ends)
            b.sync()
            off = np.zeros(b.n + 1, np.uint64)
            assert b.lib.pw_batch_cigar(b.handle, 0, None, 0, off.ctypes.data) == 0        # (notices the traceback itself)
            res, txs = _check(b, None, 'explicit ends')
            assert off.tolist() == b.cigars()[1].tolist()
            assert txs != txs0 and cigar_strings(*before) != cigar_strings(*b.cigars())

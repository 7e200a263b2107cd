"""The summary kernel on synthetic transcripts (``summarize_transcripts`` -> ``pw_tx_summarize_packed``): every record
equals the pure-Python oracle of tests/tx_summary_ref.py, all 12 fields, at every start alignment, across every dword, lane
share and pass boundary of the wavefront, and for one 10^5-op transcript among short ones."""
import itertools

import numpy as np
import pytest

from tests import tx_summary_ref as R

pytestmark = pytest.mark.gpu


def _check(txs, what):
    from biseqt_amd.batch import summarize_transcripts
    got = summarize_transcripts(txs)
    R.assert_equal(got, [R.summarize(t) for t in txs], what)
    return got


def _random(rng, n, letters='MSID'):
    return ''.join(letters[int(i)] for i in rng.integers(0, len(letters), n))


def test_every_string_up_to_six_ops():
    txs = [''.join(t) for n in range(7) for t in itertools.product('MSID', repeat=n)]
    assert len(txs) == 5461
    _check(txs, 'exhaustive')


LENGTHS = (0, 1, 2, 3, 4, 5, 7, 8, 63, 64, 65, 127, 128, 129, 255, 256, 257, 258, 259, 260, 511, 512, 513, 1023, 1025)


def _lengths_and_alignments():
    rng = np.random.default_rng(4811)
    txs = []
    for n in LENGTHS:
        t = _random(rng, n)
        txs.append(t)
        for junk in (1, 2, 3, 4):
            txs += [_random(rng, 1) for _ in range(junk)] + [t]
        # (1, 3, 6 and 10 junk bytes and four more copies do not reach every residue for every length: once more at each)
        for want in range(4):
            txs += ['S' * ((want - sum(len(x) for x in txs)) % 4), t]
    return txs


def test_every_length_at_every_start_alignment():
    txs = _lengths_and_alignments()
    starts = np.cumsum([0] + [len(t) for t in txs])[:-1]
    for n in LENGTHS:
        assert {int(s) % 4 for s, t in zip(starts, txs) if len(t) == n} == {0, 1, 2, 3}, n
    _check(txs, 'lengths and alignments')


def test_gap_runs_across_dword_lane_and_pass_boundaries():
    txs = []
    for a in (0, 3, 62, 63, 64, 254, 255, 256, 257):
        for g in (0, 1, 2, 5):
            for h in (0, 1, 2, 5):
                for b in (0, 1):
                    txs.append('M' * a + 'I' * g + 'D' * h + 'M' * b)
                    txs.append('M' * a + 'D' * g + 'I' * h + 'M' * b)
    exp = [R.summarize(t) for t in txs]
    gaps, nm = R.FIELDS.index('n_gaps'), R.FIELDS.index('n_match')
    assert any(e[gaps] == 2 and ('ID' in t or 'DI' in t) for t, e in zip(txs, exp))
    assert any(t and e[nm] == 0 and e[-1] == 1 for t, e in zip(txs, exp))
    _check(txs, 'gap runs')
    # every transcript once more behind 1, 2 and 3 bytes: the runs meet the dword boundaries at every phase
    for shift in (1, 2, 3):
        mixed = []
        for t in txs:
            mixed += ['S' * shift, t]
        _check(mixed, 'gap runs shifted by %d' % shift)


def test_a_single_match():
    rng = np.random.default_rng(4812)
    txs = []
    for at in (0, 299, 63, 64, 255, 256):
        t = list(_random(rng, 300, 'SID'))
        t[at] = 'M'
        txs.append(''.join(t))
    got = _check(txs, 'one match')
    assert [int(g['first_match']) for g in got] == [int(g['last_match']) for g in got] == [0, 299, 63, 64, 255, 256]


def test_one_long_transcript_among_short_ones():
    rng = np.random.default_rng(4813)
    txs = [_random(rng, int(rng.integers(0, 40))) for _ in range(50)]
    txs.insert(23, _random(rng, 100000))
    got = _check(txs, 'mixed sizes')
    assert sum(int(got[23][f]) for f in ('n_match', 'n_subst', 'n_ins', 'n_del')) == 100000


def test_packed_buffers_and_none_entries():
    from biseqt_amd.batch import summarize_transcripts
    txs = ['MMSI', None, '', 'DDM', None, 'S']
    exp = [R.summarize(t) for t in txs]
    R.assert_equal(summarize_transcripts(txs), exp, 'list with None')
    buf = np.frombuffer(''.join(t or '' for t in txs).encode(), np.uint8)
    off = np.cumsum([0] + [len(t or '') for t in txs]).astype(np.uint64)
    R.assert_equal(summarize_transcripts((buf, off)), exp, 'packed')
    assert len(summarize_transcripts([])) == 0


def test_refusals():
    from biseqt_amd import _pwlib as W
    from biseqt_amd.batch import SUMMARY_DTYPE
    lib = W.load()
    out = np.full(2, -7, SUMMARY_DTYPE)
    off = np.array([0, 3], np.uint64)
    assert lib.pw_tx_summarize_packed(0, None, off.ctypes.data, 0, out.ctypes.data) == 0
    assert (out == np.full(2, -7, SUMMARY_DTYPE)).all()                      # n == 0: nothing written
    assert lib.pw_tx_summarize_packed(0, None, off.ctypes.data, 1, out.ctypes.data) == -1
    assert 'null ops with a non-zero total' in W.last_error()
    assert (out == np.full(2, -7, SUMMARY_DTYPE)).all()

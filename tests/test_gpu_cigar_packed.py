"""The CIGAR kernels on synthetic transcripts (``cigars_of_transcripts`` -> ``pw_tx_cigar_packed``): runs and offsets equal
the ``itertools.groupby`` oracle of tests/cigar_ref.py, in both forms, at every start alignment, with run boundaries on every
dword, lane and pass edge of the wavefront, for one 10^5-op run among short transcripts and for transcript counts around the
chunking of the offsets scan."""
import numpy as np
import pytest

from tests import cigar_ref as R

LENGTHS = (0, 1, 2, 3, 4, 5, 7, 8, 63, 64, 65, 127, 128, 129, 255, 256, 257, 258, 259, 260, 511, 512, 513, 1023, 1025)


def _check(txs, what):
    from biseqt_amd.batch import cigars_of_transcripts
    for name, form in R.FORMS:
        R.assert_equal(cigars_of_transcripts(txs, name), txs, form, '%s, %s' % (what, name))


def _random(rng, n, letters='MSID'):
    return ''.join(letters[int(i)] for i in rng.integers(0, len(letters), n))


def _lengths_and_alignments():
    """Every length of LENGTHS at every start alignment mod 4 (the construction of tests/test_gpu_tx_summary_packed.py); the
    transcripts favour M so that runs longer than one op occur."""
    rng = np.random.default_rng(4911)
    txs = []
    for n in LENGTHS:
        t = _random(rng, n, 'MMMMSIDM')
        txs.append(t)
        for junk in (1, 2, 3, 4):
            txs += [_random(rng, 1) for _ in range(junk)] + [t]
        for want in range(4):
            txs += ['S' * ((want - sum(len(x) for x in txs)) % 4), t]
    return txs


def test_every_residue_is_reached():
    """(no GPU needed) the construction above puts every length at every start alignment"""
    txs = _lengths_and_alignments()
    starts = np.cumsum([0] + [len(t) for t in txs])[:-1]
    for n in LENGTHS:
        assert {int(s) % 4 for s, t in zip(starts, txs) if len(t) == n} == {0, 1, 2, 3}, n


@pytest.mark.gpu
def test_every_string_up_to_six_ops():
    _check(R.EXHAUSTIVE, 'exhaustive')


@pytest.mark.gpu
def test_every_length_at_every_start_alignment():
    _check(_lengths_and_alignments(), 'lengths and alignments')


@pytest.mark.gpu
def test_run_boundaries_on_dword_lane_and_pass_edges():
    txs = []
    for a in (0, 3, 62, 63, 64, 254, 255, 256, 257):
        for g in (0, 1, 2, 5):
            for h in (0, 1, 2, 5):
                for b in (0, 1):
                    txs.append('M' * a + 'S' * g + 'I' * h + 'D' * b)
    assert any(len(R.runs(t, R.CLASSIC)) < len(R.runs(t, R.EXTENDED)) for t in txs)        # M / S merges in the classic form
    _check(txs, 'run boundaries')
    for shift in (1, 2, 3):                              # ... and behind 1, 2 and 3 junk bytes: every phase of the dwords
        mixed = []
        for t in txs:
            mixed += ['D' * shift, t]
        _check(mixed, 'run boundaries shifted by %d' % shift)


@pytest.mark.gpu
def test_strictly_alternating_transcripts():
    from biseqt_amd.batch import cigars_of_transcripts
    txs = [('MS' * n)[:n] for n in (63, 64, 65, 127, 128, 129, 1025)]
    _check(txs, 'alternating')
    runs, off = cigars_of_transcripts(txs, 'extended')
    assert np.diff(off.astype(np.int64)).tolist() == [len(t) for t in txs] and (runs >> 4 == 1).all()      # one run per op
    runs, off = cigars_of_transcripts(txs, 'classic')
    assert runs.tolist() == [len(t) << 4 for t in txs]                                                     # one run


@pytest.mark.gpu
def test_one_long_run_among_short_transcripts():
    from biseqt_amd.batch import cigars_of_transcripts
    rng = np.random.default_rng(4913)
    txs = [_random(rng, int(rng.integers(0, 40))) for _ in range(50)]
    txs.insert(23, 'M' * 100000)
    _check(txs, 'one long run')
    runs, off = cigars_of_transcripts(txs)
    assert runs[int(off[23]):int(off[24])].tolist() == [100000 << 4 | 7]
    txs[23] = 'S' + _random(rng, 99998, 'MMMMMMMMMMMMMSID') + 'I'          # ... and 10^5 ops with runs of every length
    _check(txs, 'one long transcript')


@pytest.mark.gpu
@pytest.mark.parametrize('n', [1, 1023, 1024, 1025, 2049])
def test_transcript_counts_around_the_chunks_of_the_offsets_scan(n):
    rng = np.random.default_rng(4914 + n)
    _check([_random(rng, int(rng.integers(0, 4))) for _ in range(n)], '%d transcripts' % n)


@pytest.mark.gpu
def test_packed_buffers_and_none_entries():
    from biseqt_amd.batch import cigar_strings, cigars_of_transcripts
    txs = ['MMSI', None, '', 'DDM', None, 'S']
    _check(txs, 'list with None')
    buf = np.frombuffer(''.join(t or '' for t in txs).encode(), np.uint8)
    off = np.cumsum([0] + [len(t or '') for t in txs]).astype(np.uint64)
    for name, form in R.FORMS:
        R.assert_equal(cigars_of_transcripts((buf, off), name), txs, form, 'packed, ' + name)
    assert cigar_strings(*cigars_of_transcripts(txs)) == ['2=1X1I', '', '', '2D1=', '', '1X']
    assert cigar_strings(*cigars_of_transcripts(txs, 'classic')) == ['3M1I', '', '', '2D1M', '', '1M']
    # transcripts that start behind bytes of no transcript (offsets[0] > 0)
    R.assert_equal(cigars_of_transcripts((np.frombuffer(b'??MMSID', np.uint8), np.array([2, 7], np.uint64))), ['MMSID'], R.EXTENDED, 'offset')
    runs, roff = cigars_of_transcripts([])
    assert len(runs) == 0 and roff.tolist() == [0]
    runs, roff = cigars_of_transcripts([None, ''])
    assert len(runs) == 0 and roff.tolist() == [0, 0, 0]


@pytest.mark.gpu
def test_size_query_and_refusals_leave_the_outputs_untouched():
    from biseqt_amd import _pwlib as W
    lib = W.load()
    ops = np.frombuffer(b'MMSIDDM', np.uint8)
    off = np.array([0, 4, 7], np.uint64)
    runs = np.full(8, 0xabcdef01, np.uint32)
    roff = np.full(3, 77, np.uint64)

    def call(ops_, off_, n, form, runs_, cap, roff_):
        return lib.pw_tx_cigar_packed(0, None if ops_ is None else ops_.ctypes.data, off_.ctypes.data, n, form,
                                      None if runs_ is None else runs_.ctypes.data, cap, None if roff_ is None else roff_.ctypes.data)

    assert call(ops, off, 2, 0, None, 0, roff) == 0                       # runs_out == NULL: the offsets alone
    assert roff.tolist() == [0, 3, 5] and (runs == 0xabcdef01).all()
    roff[:] = 77
    assert call(ops, off, 2, 0, runs, 4, roff) == -1 and 'run buffer too small' in W.last_error()
    assert (runs == 0xabcdef01).all() and (roff == 77).all()
    assert call(ops, off, 0, 0, runs, 8, roff) == 0                       # n == 0: nothing written
    assert (runs == 0xabcdef01).all() and (roff == 77).all()
    for args, msg in (((ops, off, 2, 2, runs, 8, roff), 'unknown form'),
                      ((ops, off, -1, 0, runs, 8, roff), 'count out of range'),
                      ((ops, off, 2, 0, runs, 8, None), 'null offsets or output'),
                      ((None, off, 2, 0, runs, 8, roff), 'null ops with a non-zero total'),
                      ((ops, np.array([0, 5, 4], np.uint64), 2, 0, runs, 8, roff), 'offsets must ascend'),
                      ((ops, np.array([0, 4, 4 + (1 << 28)], np.uint64), 2, 0, runs, 8, roff), '2^28 ops or more'),
                      ((np.frombuffer(b'MMSIDNM', np.uint8), off, 2, 0, runs, 8, roff), 'byte 5 is none of M, S, I, D')):
        assert call(*args) == -1 and msg in W.last_error(), msg
        assert (runs == 0xabcdef01).all() and (roff == 77).all(), msg
    assert call(ops, off, 2, 0, runs, 5, roff) == 0                       # exactly enough room
    assert roff.tolist() == [0, 3, 5] and runs[:5].tolist() == R.runs('MMSI', 0) + R.runs('DDM', 0) and (runs[5:] == 0xabcdef01).all()

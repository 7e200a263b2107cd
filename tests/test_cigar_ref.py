"""The CIGARs without a GPU: the constants and exports of ``_pwlib`` against the text of include/pw_cigar.h, the refusals
the library makes before any device call, the host helpers of ``biseqt_amd.batch`` against the ``itertools.groupby`` oracle of
tests/cigar_ref.py, and ``pipeline.paf_lines`` on hand-written records."""
import os
import re

import numpy as np
import pytest

from tests import cigar_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    txt = open(os.path.join(ROOT, 'include', 'pw_cigar.h')).read()
    txt = re.sub(r'/\*.*?\*/', '', txt, flags=re.S)
    return re.sub(r'//[^\n]*', '', txt)


def test_constants_match_the_header():
    from biseqt_amd import _pwlib as W
    from biseqt_amd import batch as B
    defines = {m.group(1): int(m.group(2)) for m in re.finditer(r'#define\s+(PW_CIGAR_\w+)\s+(\d+)\b', _header())}
    assert set(defines) == {'PW_CIGAR_EXTENDED', 'PW_CIGAR_CLASSIC', 'PW_CIGAR_OP_M', 'PW_CIGAR_OP_I', 'PW_CIGAR_OP_D',
                            'PW_CIGAR_OP_EQ', 'PW_CIGAR_OP_X', 'PW_CIGAR_MAX_LEN'}, sorted(defines)
    for name, value in defines.items():
        assert getattr(W, name) == value, name
    assert defines['PW_CIGAR_MAX_LEN'] == 1 << 28
    assert (B.CIGAR_EXTENDED, B.CIGAR_CLASSIC) == (defines['PW_CIGAR_EXTENDED'], defines['PW_CIGAR_CLASSIC']) == (R.EXTENDED, R.CLASSIC)
    # BAM's op letters, and the oracle's table, by the header's codes
    for letter, name in (('M', 'M'), ('I', 'I'), ('D', 'D'), ('=', 'EQ'), ('X', 'X')):
        assert B.CIGAR_OPS[defines['PW_CIGAR_OP_' + name]] == letter == R.LETTERS[defines['PW_CIGAR_OP_' + name]]
    assert R.OPS[R.EXTENDED] == dict(M=defines['PW_CIGAR_OP_EQ'], S=defines['PW_CIGAR_OP_X'], I=defines['PW_CIGAR_OP_I'], D=defines['PW_CIGAR_OP_D'])
    assert R.OPS[R.CLASSIC] == dict(M=defines['PW_CIGAR_OP_M'], S=defines['PW_CIGAR_OP_M'], I=defines['PW_CIGAR_OP_I'], D=defines['PW_CIGAR_OP_D'])


def test_library_exports_every_symbol_of_the_header():
    from biseqt_amd import _pwlib as W
    lib = W.load()
    declared = set(re.findall(r'\b(pw_\w+)\s*\(', _header()))
    assert declared == set(W.CIGAR_EXPORTS), declared ^ set(W.CIGAR_EXPORTS)
    for name in declared:
        assert hasattr(lib, name), name
        assert getattr(lib, name).argtypes is not None, name


def test_known_answers():
    from biseqt_amd.batch import cigar_of_transcript, cigar_strings, transcript_of_cigar
    assert R.runs('MMSID', R.EXTENDED) == [2 << 4 | 7, 1 << 4 | 8, 1 << 4 | 1, 1 << 4 | 2]
    assert R.runs('MMSID', R.CLASSIC) == [3 << 4 | 0, 1 << 4 | 1, 1 << 4 | 2]
    assert cigar_of_transcript('MMSID', 'extended') == '2=1X1I1D' == R.string('MMSID', R.EXTENDED)
    assert cigar_of_transcript('MMSID', 'classic') == '3M1I1D' == R.string('MMSID', R.CLASSIC)
    assert cigar_of_transcript('IIDDII') == '2I2D2I'                       # an I run directly followed by a D run: two runs
    assert cigar_of_transcript('MSMSSM', 'classic') == '6M' and cigar_of_transcript('MSMSSM') == '1=1X1=2X1='
    assert cigar_of_transcript(None) == '' == cigar_of_transcript('')
    runs = np.array(R.runs('MMSID', R.EXTENDED) + R.runs('MMSID', R.CLASSIC), np.uint32)
    assert cigar_strings(runs, np.array([0, 4, 4, 7], np.uint64)) == ['2=1X1I1D', '', '3M1I1D']
    assert cigar_strings(np.zeros(0, np.uint32), np.zeros(1, np.uint64)) == []
    assert transcript_of_cigar('2=1X1I1D') == 'MMSID' and transcript_of_cigar('') == ''
    assert transcript_of_cigar('12=') == 'M' * 12
    for bad in ('3M1I', '2=1N', '=2', '2', '2=x1', '2 ='):
        with pytest.raises(ValueError):
            transcript_of_cigar(bad)
    with pytest.raises(ValueError):
        cigar_of_transcript('MMB')
    for bad in ('Extended', 2, -1, None, True):
        with pytest.raises(ValueError):
            cigar_of_transcript('MM', bad)
    assert cigar_of_transcript('MS', 0) == '1=1X' and cigar_of_transcript('MS', 1) == '2M'


def test_host_helpers_against_the_oracle_on_every_string_up_to_six_ops():
    from biseqt_amd.batch import cigar_of_transcript, cigar_strings, transcript_of_cigar
    for name, form in R.FORMS:
        strings = [cigar_of_transcript(t, name) for t in R.EXHAUSTIVE]
        assert strings == [R.string(t, form) for t in R.EXHAUSTIVE], name
        assert cigar_strings(*R.packed(R.EXHAUSTIVE, form)) == strings, name
    for t in R.EXHAUSTIVE:
        assert transcript_of_cigar(cigar_of_transcript(t, 'extended')) == t


def test_packed_entry_point_refuses_bad_input_before_any_device_call():
    from biseqt_amd import _pwlib as W
    lib = W.load()
    runs = np.full(4, 0xabcdef01, np.uint32)
    roff = np.full(2, 77, np.uint64)
    off = np.array([0, 3], np.uint64)
    ops = np.frombuffer(b'MIM', np.uint8)

    def call(ops_, off_, n, form=0, runs_=runs, cap=4, roff_=roff):
        return lib.pw_tx_cigar_packed(0, None if ops_ is None else ops_.ctypes.data, None if off_ is None else off_.ctypes.data, n, form,
                                      None if runs_ is None else runs_.ctypes.data, cap, None if roff_ is None else roff_.ctypes.data)

    assert lib.pw_tx_cigar_packed(0, None, None, 0, 0, None, 0, None) == 0        # nothing to do, nothing written
    assert call(ops, off, 0) == 0
    assert call(ops, off, -1) == -1 and b'count out of range' in lib.pw_last_error()
    for form in (2, -1, 7):
        assert call(ops, off, 1, form) == -1 and b'unknown form' in lib.pw_last_error()
        assert call(ops, off, 0, form) == -1 and b'unknown form' in lib.pw_last_error()
    assert call(ops, None, 1) == -1 and b'null offsets or output' in lib.pw_last_error()
    assert call(ops, off, 1, roff_=None) == -1 and b'null offsets or output' in lib.pw_last_error()
    assert call(None, off, 1) == -1 and b'null ops with a non-zero total' in lib.pw_last_error()
    assert call(ops, np.array([3, 0], np.uint64), 1) == -1 and b'offsets must ascend' in lib.pw_last_error()
    assert call(ops, np.array([0, 1 << 28], np.uint64), 1) == -1 and b'2^28 ops or more' in lib.pw_last_error()
    for junk in (b'MXM', b'M\x00M', b'MmM', b'M=M'):
        assert call(np.frombuffer(junk, np.uint8), off, 1) == -1 and b'byte 1 is none of M, S, I, D' in lib.pw_last_error()
    # (bytes in front of offsets[0] belong to no transcript: the refusal names the first byte of one)
    assert call(np.frombuffer(b'??MMB', np.uint8), np.array([2, 4, 5], np.uint64), 2) == -1 and b'byte 4 is none' in lib.pw_last_error()
    assert (runs == 0xabcdef01).all() and (roff == 77).all()


def _paf_records():
    """Hand-written records of the four shapes map_queries returns: {with, without} transcripts x {with, without} strands."""
    from biseqt_amd.pw import Alignment
    from biseqt_amd.sequence import Alphabet, Sequence
    A = Alphabet('ACGT')
    S = Sequence(A, (0, 1, 2, 3) * 8)
    tx = 'MMSIMDDM'                                      # 4 M, 1 S, 1 I, 2 D: 7 letters of the target, 6 of the query
    summary = dict(n_match=4, n_subst=1, n_ins=1, n_del=2, n_gaps=2, first_match=0, last_match=7, head_origin=0, head_mutant=0,
                   tail_origin=0, tail_mutant=0, flags=1)
    base = dict(segment=((0, 1), (2, 3)), p=.9, diag_range=(0, 1), p_aln=.67, len_aln=6)
    none = dict(base, score=None, alignment=None, p_aln=None, len_aln=None)
    full_plain = dict(base, score=3.0, alignment=Alignment(S, S, tx, score=3.0, origin_start=5, mutant_start=2))
    lean_plain = dict(base, score=-2.5, alignment=None, origin_start=5, mutant_start=2, summary=summary, cigar='2=1X1I1=2D1=')
    full_minus = dict(base, score=7.0, alignment=Alignment(S, S, tx, score=7.0, origin_start=9, mutant_start=1), strand='-',
                      query_interval=(13, 19), cigar='3M1I1M2D1M')
    lean_plus = dict(base, score=1e3, alignment=None, origin_start=0, mutant_start=4, summary=summary, strand='+', query_interval=(4, 10))
    none_stranded = dict(none, origin_start=None, mutant_start=None, summary=None, strand='-', query_interval=None, cigar=None)
    return [[full_plain, dict(none)], [], [lean_plain], [full_minus, none_stranded, lean_plus]]


def test_paf_lines_on_hand_written_records():
    from biseqt_amd.pipeline import paf_lines
    lines = paf_lines(_paf_records(), 'chr', 32, ['q0', 'q1', 'q2', 'q3'], [20, 21, 22, 20])
    assert lines == [
        'q0\t20\t2\t8\t+\tchr\t32\t5\t12\t4\t8\t255\tAS:i:3',
        'q2\t22\t2\t8\t+\tchr\t32\t5\t12\t4\t8\t255\tAS:f:-2.5\tcg:Z:2=1X1I1=2D1=',
        'q3\t20\t13\t19\t-\tchr\t32\t9\t16\t4\t8\t255\tAS:i:7\tcg:Z:3M1I1M2D1M',
        'q3\t20\t4\t10\t+\tchr\t32\t0\t7\t4\t8\t255\tAS:i:1000',
    ]
    assert paf_lines([[], []], 'chr', 32, ['a', 'b'], [1, 2]) == []

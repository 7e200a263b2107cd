"""The alignment summaries without a GPU: the pure-Python oracle (tests/tx_summary_ref.py) against
``Alignment.truncate_to_match`` -- the host code the summaries replace -- and the record layout of ``SUMMARY_DTYPE`` and the
ctypes structure against include/pw_txsum.h."""
import os
import re

import numpy as np
import pytest

from tests import tx_summary_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    txt = open(os.path.join(ROOT, 'include', 'pw_txsum.h')).read()
    txt = re.sub(r'/\*.*?\*/', '', txt, flags=re.S)
    return re.sub(r'//[^\n]*', '', txt)


def _random_transcripts(n, seed):
    """Short transcripts over MSID; a share of them has few or no M, so that every outcome of truncate_to_match occurs."""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n):
        ln = int(rng.integers(1, 40))
        letters = ('MSID', 'SID', 'MSIDSIDSID', 'MMMSID')[k % 4]
        out.append(''.join(letters[int(i)] for i in rng.integers(0, len(letters), ln)))
    return out


def test_oracle_agrees_with_truncate_to_match():
    from biseqt_amd.pipeline import truncated_frame
    from biseqt_amd.pw import Alignment
    from biseqt_amd.sequence import Alphabet, Sequence
    A = Alphabet('ACGT')
    S = Sequence(A, (0, 1, 2, 3) * 16)
    seen = {'none': 0, 'raise': 0, 'aln': 0}
    for k, tx in enumerate(_random_transcripts(500, 4801)):
        o0, m0 = k % 7, k % 5
        aln = Alignment(S, S, tx, origin_start=o0, mutant_start=m0)
        s = dict(zip(R.FIELDS, R.summarize(tx)))
        assert s['flags'] == 1
        assert s['n_match'] + s['n_subst'] + s['n_ins'] + s['n_del'] == len(tx)
        frame = truncated_frame(o0, m0, s)
        try:
            tr = aln.truncate_to_match()
        except IndexError:
            assert s['first_match'] == -1 and s['last_match'] == -1 and s['n_match'] == 0, tx
            assert (s['head_origin'], s['head_mutant'], s['tail_origin'], s['tail_mutant']) == (0, 0, 0, 0), tx
            assert frame is None
            seen['raise'] += 1
            continue
        assert s['first_match'] >= 0, tx
        if tr is None:
            assert s['first_match'] >= s['last_match'] and s['n_match'] == 1, tx
            assert frame is None
            seen['none'] += 1
            continue
        assert s['first_match'] < s['last_match'], tx
        assert tr.origin_start == o0 + s['head_origin'] and tr.mutant_start == m0 + s['head_mutant'], tx
        assert len(tr.transcript) == s['last_match'] - s['first_match'] + 1, tx
        assert frame == ((tr.origin_start, tr.origin_start + Alignment.projected_len(tr.transcript, on='origin')),
                         (tr.mutant_start, tr.mutant_start + Alignment.projected_len(tr.transcript, on='mutant'))), tx
        seen['aln'] += 1
    assert min(seen.values()) >= 20, seen


def test_oracle_conventions():
    assert R.summarize(None) == R.NONE and R.summarize('') == R.NONE
    for status in (0, R.ST_TRACED | R.ST_EMPTY, R.ST_TRACED | R.ST_PANICK, R.ST_TRACED | R.ST_BADPATH):
        assert R.summarize('MM', status) == R.NONE
    assert R.summarize('IIDDII')[4] == 3 and R.summarize('IMI')[4] == 2 and R.summarize('DDDD')[4] == 1
    assert R.summarize('SDMISMDS') == (2, 3, 1, 2, 3, 2, 5, 2, 1, 2, 1, 1)


def test_summary_dtype_is_48_bytes():
    from biseqt_amd import _pwlib as W
    from biseqt_amd.batch import SUMMARY_DTYPE
    import ctypes as C
    assert SUMMARY_DTYPE.itemsize == 48
    assert C.sizeof(W.pw_tx_summary) == 48
    W.check_layout()


def test_summary_dtype_matches_the_header():
    from biseqt_amd import _pwlib as W
    from biseqt_amd.batch import SUMMARY_DTYPE
    m = re.search(r'typedef\s+struct\s*\{([^}]*)\}\s*pw_tx_summary\s*;', _header())
    assert m
    fields = []
    for decl in m.group(1).split(';'):
        decl = decl.strip()
        if not decl:
            continue
        t, names = decl.split(None, 1)
        assert t == 'int32_t', decl
        fields += [n.strip() for n in names.split(',')]
    assert tuple(fields) == R.FIELDS
    assert SUMMARY_DTYPE.names == tuple(fields)
    for q, f in enumerate(fields):
        assert SUMMARY_DTYPE.fields[f][1] == 4 * q and SUMMARY_DTYPE.fields[f][0] == np.dtype('<i4'), f
        assert getattr(W.pw_tx_summary, f).offset == 4 * q and getattr(W.pw_tx_summary, f).size == 4, f
    assert [n for n, _ in W.pw_tx_summary._fields_] == fields
    assert re.search(r'#define\s+PW_TXSUM_DONE\s+1\b', _header()) and W.PW_TXSUM_DONE == 1


def test_library_exports_every_symbol_of_the_header():
    from biseqt_amd import _pwlib as W
    lib = W.load()
    declared = set(re.findall(r'\b(pw_\w+)\s*\(', _header()))
    assert declared == set(W.TXSUM_EXPORTS), declared ^ set(W.TXSUM_EXPORTS)
    for name in declared:
        assert hasattr(lib, name), name


def test_packed_entry_point_refuses_bad_input_before_any_device_call():
    from biseqt_amd import _pwlib as W
    lib = W.load()
    out = np.full(1, -7, np.dtype([(f, '<i4') for f in R.FIELDS]))
    off = np.array([0, 3], np.uint64)
    ops = np.frombuffer(b'MIM', np.uint8)
    assert lib.pw_tx_summarize_packed(0, None, None, 0, None) == 0              # nothing to do, nothing written
    assert lib.pw_tx_summarize_packed(0, ops.ctypes.data, off.ctypes.data, 0, out.ctypes.data) == 0
    assert all(int(out[0][f]) == -7 for f in R.FIELDS)
    assert lib.pw_tx_summarize_packed(0, ops.ctypes.data, off.ctypes.data, -1, out.ctypes.data) == -1
    assert b'count out of range' in lib.pw_last_error()
    assert lib.pw_tx_summarize_packed(0, ops.ctypes.data, None, 1, out.ctypes.data) == -1
    assert b'null offsets or output' in lib.pw_last_error()
    assert lib.pw_tx_summarize_packed(0, None, off.ctypes.data, 1, out.ctypes.data) == -1
    assert b'null ops with a non-zero total' in lib.pw_last_error()
    bad = np.array([3, 0], np.uint64)
    assert lib.pw_tx_summarize_packed(0, ops.ctypes.data, bad.ctypes.data, 1, out.ctypes.data) == -1
    assert b'offsets must ascend' in lib.pw_last_error()
    big = np.array([0, 1 << 31], np.uint64)
    assert lib.pw_tx_summarize_packed(0, ops.ctypes.data, big.ctypes.data, 1, out.ctypes.data) == -1
    assert b'2^31 ops or more' in lib.pw_last_error()
    assert all(int(out[0][f]) == -7 for f in R.FIELDS)

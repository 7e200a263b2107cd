"""Read correction without a GPU: the ctypes structure, constants and exports of ``_pwlib`` against the text of
include/pw_polish.h, and the argument checks of the library, ``Pileup``, ``BatchAligner.pileup_add`` and
``overlap_alignments`` that run before any device work.  (The refusals that need a live pileup -- a read outside it at the C
level, the polished accessors before a polish -- are in tests/test_gpu_polish_reads.py.)"""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    txt = open(os.path.join(ROOT, 'include', 'pw_polish.h')).read()
    txt = re.sub(r'/\*.*?\*/', '', txt, flags=re.S)
    return re.sub(r'//[^\n]*', '', txt)


def test_constants_exports_and_structure_match_the_header():
    from biseqt_amd import _pwlib as W
    from biseqt_amd import batch as B
    from tests import polish_ref as PR
    lib = W.load()
    txt = _header()
    defines = {m.group(1): int(m.group(2)) for m in re.finditer(r'#define\s+(PW_\w+)\s+(\d+)\b', txt)}
    assert defines == dict(PW_POLISH_MAX_SLOTS=8, PW_SIDE_ORIGIN=1, PW_SIDE_MUTANT=2, PW_SIDE_BOTH=3), defines
    for name, value in defines.items():
        assert getattr(W, name) == value, name
    declared = set(re.findall(r'\b(pw_\w+)\s*\(', txt))
    assert declared == set(W.POLISH_EXPORTS), declared ^ set(W.POLISH_EXPORTS)
    assert not declared & set(W.PILEUP_EXPORTS)
    for name in declared:
        assert hasattr(lib, name), name
        assert getattr(lib, name).argtypes is not None, name
    assert re.search(r'typedef struct \{ uint32_t kept; uint32_t substituted; uint32_t deleted; uint32_t inserted; \} pw_polish_stats;', txt)
    assert C.sizeof(W.pw_polish_stats) == 16 and W.SIZEOF['pw_polish_stats'] == 16
    W.check_layout()
    for dt in (B.POLISH_STATS_DTYPE, PR.STATS_DTYPE):
        assert dt.itemsize == 16 and [(n, dt.fields[n][1]) for n in dt.names] == \
            [('kept', 0), ('substituted', 4), ('deleted', 8), ('inserted', 12)]


def test_library_refuses_bad_arguments_before_any_device_call():
    from biseqt_amd import _pwlib as W
    lib = W.load()
    for J in (0, 9, -1):
        assert not lib.pw_pileup_create_ins(0, 5, 4, J) and 'ins_slots must be 1..8' in W.last_error()
    for sides in (0, 4, -1):
        assert lib.pw_batch_pileup_add_sides(None, None, sides, None, None, None, None, 0, 0, None) == -1
        assert 'sides must be 1 (origin), 2 (mutant) or 3 (both)' in W.last_error()
    for sides in (1, 2, 3):
        assert lib.pw_batch_pileup_add_sides(None, None, sides, None, None, None, None, 0, 0, None) == -1
        assert 'null batch or pileup' in W.last_error()
    out = np.zeros(8, np.int64)
    assert lib.pw_pileup_ins_slots(None) == 0 and not lib.pw_pileup_ins_counts_device(None)
    assert lib.pw_pileup_ins_counts(None, 0, 1, out.ctypes.data) == -1 and 'null pileup' in W.last_error()
    assert lib.pw_pileup_add_letters(None, None, 0, 1, 1, None) == -1 and 'null pileup' in W.last_error()
    assert lib.pw_pileup_polish(None, None, None, None, 0, 1, None) == -1 and 'null pileup' in W.last_error()
    assert lib.pw_pileup_polished_total(None) == -1 and 'null pileup' in W.last_error()
    for name in ('pw_pileup_polished_offsets', 'pw_pileup_polished_letters', 'pw_pileup_polished_stats'):
        assert getattr(lib, name)(None, out.ctypes.data) == -1 and 'null pileup' in W.last_error()
    assert not lib.pw_pileup_polished_letters_device(None) and not lib.pw_pileup_polished_offsets_device(None)


def _unopened(cls, **attrs):
    """An instance that never reached the device: the argument checks under test run before anything needs a handle."""
    obj = object.__new__(cls)
    obj.handle = None
    for k, v in attrs.items():
        setattr(obj, k, v)
    return obj


def test_python_argument_validation_needs_no_device():
    from biseqt_amd.batch import BatchAligner, Pileup
    from biseqt_amd.overlap import overlap_alignments, polish_reads
    from biseqt_amd.sequence import Alphabet, Sequence
    for J in (9, -1):
        with pytest.raises(ValueError, match='ins_slots'):
            Pileup(10, 4, ins_slots=J)
    b = _unopened(BatchAligner, n=2)
    for sides in ('left', 0, 4, None):
        with pytest.raises(ValueError, match="'origin', 'mutant' or 'both'"):
            b.pileup_add(object(), sides=sides)
    with pytest.raises(ValueError, match='need a complement'):
        b.pileup_add(object(), sides='both', reverse=[0, 1])                    # reversed pairs without a complement
    with pytest.raises(ValueError, match='mutant side'):
        b.pileup_add(object(), sides='origin', reverse=[0, 1], complement=[3, 2, 1, 0])
    with pytest.raises(ValueError, match='mutant_col0 has 3 entries'):
        b.pileup_add(object(), sides='mutant', mutant_col0=[0, 1, 2])
    with pytest.raises(ValueError, match='reverse has 1 entries'):
        b.pileup_add(object(), sides='mutant', reverse=[1], complement=[3, 2, 1, 0])
    with pytest.raises(ValueError, match='open Pileup'):
        b.pileup_add(object(), sides='both', reverse=[0, 0])                    # nothing reversed: no complement needed
    p = _unopened(Pileup, n_cols=10, alphabet_len=4, ins_slots=0, device=0, _ref=None)
    for offs, lens in (([8], [3]), ([-1], [2]), ([0, 11], [1, 0]), ([0], [-1])):  # a read outside the pileup
        with pytest.raises(ValueError, match='outside the pileup'):
            p.polish(np.zeros(10, np.uint8), offs, lens)
    with pytest.raises(ValueError, match='offsets for'):
        p.polish(np.zeros(10, np.uint8), [0, 1], [1])
    with pytest.raises(ValueError, match='no insertion plane'):
        p.ins_counts()
    with pytest.raises(ValueError, match='weight'):
        p.add_letters(np.zeros(10, np.uint8), weight=-1)
    A = Alphabet('ACGT')
    ref, q = Sequence(A, (0, 1, 2, 3) * 10), Sequence(A, (0, 1, 2, 3) * 5)
    with pytest.raises(ValueError, match="'origin' or 'both'"):
        overlap_alignments([ref, q], [(0, 1)], [None], A, pileup_sides='mutant')
    with pytest.raises(ValueError, match='ins_slots'):
        polish_reads([ref, q], [(0, 1)], [None], A, ins_slots=9)
